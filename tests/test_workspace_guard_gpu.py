"""Nothing writes outside the workspace it was given.  A forward and a training step run once as they are and once with every
workspace and context buffer being the interior of a larger allocation of the test's own, 4 KB of a fixed byte pattern on each side and
exactly as many bytes between them as the size entries asked for: results are bit-identical and the pattern is intact, so an overrun
shows as a changed byte, not as a fault.  fp32 takes the unfused paths, the ones that use every buffer of a layout."""
import dataclasses

import pytest
import torch

from sepreformer_amd.config import VARIANTS
from sepreformer_amd.model import Model
from sepreformer_amd.synth import synth_mixture, synth_sources

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, PATTERN = 4096, 0xA5


class GuardedPool:
    """Buffers of exactly the requested size between two guard zones."""

    def __init__(self):
        self.bufs = []
        self.cur = None

    def alloc(self, nbytes):
        nbytes = int(nbytes)
        big = torch.full((nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.bufs.append((big, nbytes))
        return big[GUARD:GUARD + nbytes]

    def workspace(self, nbytes):     # stands in for an engine's _workspace: grows like it, never hands out more than was asked for
        if self.cur is None or self.cur.numel() < nbytes:
            self.cur = self.alloc(nbytes)
        return self.cur.data_ptr(), self.cur.numel()

    def assert_intact(self):
        torch.cuda.synchronize()
        assert self.bufs
        for i, (big, n) in enumerate(self.bufs):
            lo, hi = big[:GUARD], big[GUARD + n:]
            assert hi.numel() == GUARD
            assert bool((lo == PATTERN).all()), f"buffer {i} ({n} bytes): {int((lo != PATTERN).sum())} bytes changed in front of it"
            assert bool((hi == PATTERN).all()), f"buffer {i} ({n} bytes): {int((hi != PATTERN).sum())} bytes changed behind it"


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_inference_stays_inside_its_workspaces(precision, monkeypatch):
    m = Model.from_config(VARIANTS["tiny"], init_seed=0, precision=precision).load_synthetic_(0).eval().to(DEV)
    x = (synth_mixture(2, 4000, seed=7) * 4).to(DEV)
    eng = m.engine()
    wav0, aux0 = eng.forward(x, with_aux=True)
    wav0, aux0 = wav0.clone(), [a.clone() for a in aux0]
    torch.cuda.synchronize()
    assert eng._ws2 is not None, "the auxiliary heads ran on the side stream"
    pool, side = GuardedPool(), GuardedPool()
    monkeypatch.setattr(eng, "_workspace", pool.workspace)
    eng._ws2 = side.alloc(eng._ws2.numel())          # prepare() keeps a side workspace that is large enough
    side_ptr = eng._ws2.data_ptr()
    wav1, aux1 = eng.forward(x, with_aux=True)
    pool.assert_intact()
    side.assert_intact()
    assert eng._ws2.data_ptr() == side_ptr and eng._wsargs[0] == pool.cur.data_ptr()
    assert torch.equal(wav0, wav1) and len(aux0) == len(aux1) > 0
    for a, b in zip(aux0, aux1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_training_step_stays_inside_its_buffers(precision, monkeypatch):
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    cfg = dataclasses.replace(VARIANTS["tiny"], dropout=0.0)
    m = Model.from_config(cfg, init_seed=0, precision=precision).load_synthetic_(0).to(DEV)
    m.train()
    src = torch.from_numpy(synth_sources(2, 4000, seed=11)) * 4              # [B, 2, T]
    srcd = [src[:, s].contiguous().to(DEV) for s in range(cfg.num_spks)]
    x = src.sum(dim=1).to(DEV)
    sizes = torch.full((x.shape[0],), x.shape[1])
    crit_t = PIT_SISNR_time(DEV, cfg.num_spks, True)
    crit_m = PIT_SISNR_mag(DEV, 512, 128, "hann", cfg.num_stages, cfg.num_spks, True, False)

    def step():
        for p in m.parameters():
            p.grad = None
        audio, aux = m(x)
        l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=srcd) for i, a in enumerate(aux)]
        loss = (0.6 * crit_t(estims=audio, input_sizes=sizes, target_attr=srcd) + 0.4 * sum(l_mag) / len(l_mag)) / cfg.num_spks
        loss.backward()
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in m.named_parameters()}

    g0 = step()
    eng = m.__dict__["_train_engine"]
    pool, ctxs = GuardedPool(), GuardedPool()
    plain_ctx = eng._ctx
    monkeypatch.setattr(eng, "_workspace", pool.workspace)
    monkeypatch.setattr(eng, "_ctx", lambda *a, **k: ctxs.alloc(plain_ctx(*a, **k).numel()))
    g1 = step()
    pool.assert_intact()
    ctxs.assert_intact()
    assert len(ctxs.bufs) > 4
    assert set(g0) == set(g1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
