"""The weight EMA on the device: sepr_adamw_step_ema and sepr_adamw_swap through the C ABI on synthetic tensors,
FlatAdamW(ema_decay=...) on the model, the skipped step, the in-place exchange, captured against eager, validation on the averaged
weights, a resumed run, and the checkpoint through the tools.  The EMA is compared bit for bit (int32 views) with tests/ema_ref.py: the
kernel makes three rounded fp32 operations and no FMA, so there is nothing for a tolerance to cover.  The ``tiny`` variant on the
four-key corpus of tests/golden/dynmix.npz, batch 2, 2000 samples, as tests/test_trainer_gpu.py."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_ref as dr                                                      # noqa: E402
import ema_ref as er                                                         # noqa: E402
import trainer_ref as tr                                                     # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import trainer as T                                     # noqa: E402
from sepreformer_amd.config import VARIANTS                                  # noqa: E402
from sepreformer_amd.model import Model                                      # noqa: E402
from sepreformer_amd.optim import FlatAdamW                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, MAXLEN, LR, WARMUP = 2, 2000, 1.0e-3, 3
DECAY, EMA_WARMUP = 0.9, 10.0
SIZES = (1, 3, 5, 1023, 1024, 1025, 4099)     # the scalar tail, an exact block, one element over a block, several blocks with a tail
PAD = 12345.0                                 # what the alignment padding of the flat buffers holds: no kernel may write it


# ---- the step and the exchange through the ABI -------------------------------------------------------------------------------------------
class _Flat:
    """A test-built table over tensors of SIZES: separate parameter allocations, 64-element slots in the flat buffers."""

    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda n: torch.randn(n, generator=g)                          # noqa: E731
        self.lib = L.load()
        blk = self.lib.sepr_adamw_block_elems()
        self.off, total = [], 0
        for n in SIZES:
            self.off.append(total)
            total += (n + 63) // 64 * 64
        self.total = total
        self.params = [rnd(n).to(DEV) for n in SIZES]
        assert all(p.data_ptr() % 16 == 0 for p in self.params)
        self.grads = torch.zeros(total, device=DEV)                          # the norm pass reads the padding: zero
        self.exp_avg, self.exp_avg_sq, self.ema = (torch.full((total,), PAD, device=DEV) for _ in range(3))
        for n, o in zip(SIZES, self.off):
            self.grads[o:o + n] = rnd(n).to(DEV)
            self.exp_avg[o:o + n] = (0.1 * rnd(n)).to(DEV)
            self.exp_avg_sq[o:o + n] = (0.01 * rnd(n) ** 2).to(DEV)
            self.ema[o:o + n] = rnd(n).to(DEV)
        self.step = torch.zeros(1, dtype=torch.float64, device=DEV)
        self.lr = torch.full((1,), 1.0e-2, dtype=torch.float32, device=DEV)
        self.scal = torch.full((8,), -7.0, dtype=torch.float32, device=DEV)
        self.ws = torch.zeros(self.lib.sepr_adamw_workspace(), dtype=torch.uint8, device=DEV)
        blocks = [(i, e) for i, n in enumerate(SIZES) for e in range(0, n, blk)]
        assert all(0 <= e < SIZES[i] for i, e in blocks)
        self.nblocks = len(blocks)
        self.t_params = torch.tensor([p.data_ptr() for p in self.params], dtype=torch.int64, device=DEV)
        self.t_off = torch.tensor(self.off, dtype=torch.int64, device=DEV)
        self.t_numel = torch.tensor(SIZES, dtype=torch.int32, device=DEV)
        self.t_blocks = torch.tensor(blocks, dtype=torch.int32, device=DEV).contiguous()

    def tables(self):
        return L.AdamWTables(params=self.t_params.data_ptr(), grad_off=self.t_off.data_ptr(), state_off=self.t_off.data_ptr(),
                             numel=self.t_numel.data_ptr(), blocks=self.t_blocks.data_ptr(), ntensors=len(SIZES), nblocks=self.nblocks)

    def call(self, ema, warmup=EMA_WARMUP, decay=DECAY, ema_ptr=None):
        t = self.tables()
        head = (C.byref(t), self.grads.data_ptr(), self.total, self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.step.data_ptr(),
                self.lr.data_ptr(), 0.9, 0.999, 1.0e-8, 1.0e-2, 5.0)
        tail = (self.scal.data_ptr(), self.ws.data_ptr(), self.ws.numel(), None)
        if ema:
            return self.lib.sepr_adamw_step_ema(*head, self.ema.data_ptr() if ema_ptr is None else ema_ptr, decay, warmup, *tail)
        return self.lib.sepr_adamw_step_guarded(*head, *tail)

    def slots(self, flat):
        return [flat[o:o + n].cpu().numpy() for n, o in zip(SIZES, self.off)]

    def padding_intact(self, flat):
        keep = torch.ones(self.total, dtype=torch.bool)
        for n, o in zip(SIZES, self.off):
            keep[o:o + n] = False
        return bool((flat.cpu()[keep] == PAD).all())


@pytest.mark.parametrize("warmup", [EMA_WARMUP, 0.0])
def test_step_through_the_abi(warmup):
    a, b = _Flat(1), _Flat(1)                                                # b: the twin sepr_adamw_step_guarded runs on
    for p, q in zip(a.params, b.params):
        assert tr.same_bits(p, q)
    for t in (1, 2, 3):
        before = a.slots(a.ema)
        assert a.call(True, warmup) == L.SEPR_OK and b.call(False) == L.SEPR_OK
        torch.cuda.synchronize()
        want_w = er.one_minus(t, DECAY, warmup)
        scal = a.scal.cpu().numpy()
        assert scal[6] == want_w and scal[5] == 0.0 and scal[7] == np.float32(-7.0), scal
        assert float(a.step) == float(b.step) == t
        assert np.array_equal(er.bits(scal[:6]), er.bits(b.scal.cpu().numpy()[:6]))
        for k, (p, q) in enumerate(zip(a.params, b.params)):
            assert tr.same_bits(p, q), SIZES[k]
        assert tr.same_bits(a.exp_avg, b.exp_avg) and tr.same_bits(a.exp_avg_sq, b.exp_avg_sq)
        for k, (e0, e1, p) in enumerate(zip(before, a.slots(a.ema), a.params)):
            assert er.same(e1, er.ema_step(e0, p.cpu().numpy(), t, DECAY, warmup)), (SIZES[k], t)
            assert not er.same(e1, e0)
        assert a.padding_intact(a.ema) and a.padding_intact(a.exp_avg) and a.padding_intact(a.exp_avg_sq)
    assert float(b.scal[6]) == -7.0                                          # the guarded entry never writes the slot
    if warmup:
        assert er.one_minus(1, DECAY, warmup) == np.float32(1.0 - 2.0 / 11.0) and er.one_minus(3, DECAY, warmup) != er.one_minus(3, DECAY, 0.0)


def test_abi_refuses_bad_ema_arguments():
    a = _Flat(2)
    snap = [p.clone() for p in a.params] + [a.ema.clone(), a.step.clone()]
    assert a.call(True, ema_ptr=0) == L.SEPR_EINVAL                          # null
    assert a.call(True, ema_ptr=a.ema.data_ptr() + 4) == L.SEPR_EINVAL       # misaligned
    for bad in (1.0, -0.1, 1.5, float("nan")):
        assert a.call(True, decay=bad) == L.SEPR_EINVAL
    t = a.tables()
    assert a.lib.sepr_adamw_swap(C.byref(t), None, None) == L.SEPR_EINVAL
    assert a.lib.sepr_adamw_swap(C.byref(t), a.ema.data_ptr() + 4, None) == L.SEPR_EINVAL
    torch.cuda.synchronize()
    for x, y in zip(snap, a.params + [a.ema, a.step]):
        assert tr.same_bits(x, y)                                            # nothing was launched


def test_swap_through_the_abi():
    a = _Flat(3)
    p0, e0 = [p.cpu().numpy().copy() for p in a.params], a.slots(a.ema)
    t = a.tables()
    assert a.lib.sepr_adamw_swap(C.byref(t), a.ema.data_ptr(), None) == L.SEPR_OK
    torch.cuda.synchronize()
    for k, (p, e) in enumerate(zip(a.params, a.slots(a.ema))):
        assert er.same(p, e0[k]) and er.same(e, p0[k]), SIZES[k]
    assert a.padding_intact(a.ema)
    assert a.lib.sepr_adamw_swap(C.byref(t), a.ema.data_ptr(), None) == L.SEPR_OK
    torch.cuda.synchronize()
    for k, (p, e) in enumerate(zip(a.params, a.slots(a.ema))):
        assert er.same(p, p0[k]) and er.same(e, e0[k]), SIZES[k]             # twice is the identity
    assert a.padding_intact(a.ema)


# ---- on the model ---------------------------------------------------------------------------------------------------------------------------
def tiny(dropout=0.0):
    cfg = VARIANTS["tiny"] if dropout is None else dataclasses.replace(VARIANTS["tiny"], dropout=dropout)
    return Model.from_config(cfg, init_seed=0).load_synthetic_(0).to(DEV)


def _batch(seed=5):
    from sepreformer_amd.synth import synth_mixture
    s1, s2 = synth_mixture(B, MAXLEN, seed=seed).to(DEV), synth_mixture(B, MAXLEN, seed=seed + 1).to(DEV)
    return (s1 + s2).contiguous(), [s1.contiguous(), s2.contiguous()]


class _Eager:
    """Eager steps of tiny on one fixed batch with the EMA on."""

    def __init__(self):
        from sepreformer_amd.criterion import PIT_SISNR_time
        self.model = tiny().train()
        self.opt = FlatAdamW(self.model, lr=LR, weight_decay=1.0e-2, skip_nonfinite=True, ema_decay=DECAY, ema_warmup=EMA_WARMUP)
        self.crit = PIT_SISNR_time(torch.device(DEV), 2, True)
        self.x, self.tg = _batch()
        self.sizes = torch.full((B,), MAXLEN)

    def backward(self):
        self.opt.zero_grad(set_to_none=True)
        audio, _ = self.model(self.x)
        (self.crit(estims=audio, input_sizes=self.sizes, target_attr=self.tg) / 2).backward()

    def step(self, n=1):
        for _ in range(n):
            self.backward()
            self.opt.step(max_norm=5.0)

    def weights(self):
        return {k: p.detach().cpu().numpy().copy() for k, p in self.model.named_parameters()}


def test_step_on_the_model():
    run = _Eager()
    want = run.weights()                                                     # the buffer starts at the parameters
    got = run.opt.ema_state_dict()
    assert list(got) == list(want) and all(er.same(got[k], want[k]) and got[k].shape == want[k].shape for k in want)
    for t in range(1, 6):
        run.step()
        now = run.weights()
        want = {k: er.ema_step(want[k], now[k], t, DECAY, EMA_WARMUP) for k in want}
        got = run.opt.ema_state_dict()
        for k in want:
            assert er.same(got[k], want[k]), (k, t)
        assert float(run.opt._scal[6]) == float(er.one_minus(t, DECAY, EMA_WARMUP))
    assert any(not er.same(got[k], now[k]) for k in want)
    # torch.optim.AdamW's layout: the optimizer's own state dict does not mention the average
    sd = run.opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    # load_ema_state_dict / reset_ema
    other = {k: v + 1.0 for k, v in got.items()}
    run.opt.load_ema_state_dict(other)
    back = run.opt.ema_state_dict()
    assert all(er.same(back[k], other[k]) for k in other)
    run.opt.reset_ema()
    back = run.opt.ema_state_dict()
    assert all(er.same(back[k], now[k]) for k in now)


def test_a_skipped_step_leaves_the_ema_alone():
    run = _Eager()
    run.step()
    ema, w, count = run.opt._ema.clone(), run.opt._scal[6].clone(), float(run.opt._step)
    assert count == 1.0
    run.backward()
    g = next(iter(run.model.parameters())).grad
    flat = run.model.__dict__["_grad_flat"]
    assert flat.data_ptr() <= g.data_ptr() < flat.data_ptr() + 4 * flat.numel()
    g.view(-1)[0] = float("inf")                                             # arithmetic, not a fault
    run.opt.step(max_norm=5.0)
    assert float(run.opt._scal[5]) == 1.0 and float(run.opt._step) == count
    assert tr.same_bits(run.opt._ema, ema) and tr.same_bits(run.opt._scal[6], w)
    before = run.opt.ema_state_dict()
    run.step()
    assert float(run.opt._scal[5]) == 0.0 and float(run.opt._step) == count + 1
    assert float(run.opt._scal[6]) == float(er.one_minus(count + 1, DECAY, EMA_WARMUP))
    now, got = run.weights(), run.opt.ema_state_dict()
    for k in now:
        assert er.same(got[k], er.ema_step(before[k].numpy(), now[k], count + 1, DECAY, EMA_WARMUP)), k


def test_averaged_swaps_in_place_and_repacks():
    run = _Eager()
    run.step(2)
    model, opt = run.model, run.opt
    model.eval()
    with torch.inference_mode():
        raw_out = [a.clone() for a in model(run.x)[0]]                       # packs the RAW weights: the context must not answer from them
    raw = [p.detach().clone() for p in opt._params]
    ema_flat = opt._ema.clone()
    ema_sd = opt.ema_state_dict()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    sd.update(ema_sd)                                                        # the averaged parameters plus the model's buffers
    fresh = tiny()
    fresh.load_state_dict(sd, strict=True)
    fresh.eval()
    with torch.inference_mode():
        want = [a.clone() for a in fresh(run.x)[0]]
    with opt.averaged():
        for p, r, so in zip(opt._params, raw, opt._soff):
            n = p.numel()
            assert tr.same_bits(p.detach().reshape(-1), ema_flat[so:so + n]) and tr.same_bits(opt._ema[so:so + n], r.reshape(-1))
        with torch.inference_mode():
            got = [a.clone() for a in model(run.x)[0]]
        for g, w_, r in zip(got, want, raw_out):
            assert tr.same_bits(g, w_) and not tr.same_bits(g, r)
        with pytest.raises(RuntimeError, match="nest"):
            with opt.averaged():
                pass
        with pytest.raises(RuntimeError, match="averaged"):
            opt.step(max_norm=5.0)
    for p, r in zip(opt._params, raw):
        assert tr.same_bits(p.detach(), r)
    assert tr.same_bits(opt._ema, ema_flat)
    with torch.inference_mode():
        again = [a.clone() for a in model(run.x)[0]]
    assert all(tr.same_bits(a, r) for a, r in zip(again, raw_out))           # re-packed on the way out too
    model.train()
    run.step()                                                               # and the run goes on
    assert float(opt._step) == 3.0
    plain = FlatAdamW(tiny(), lr=LR, skip_nonfinite=True)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with plain.averaged():
            pass


# ---- Trainer ----------------------------------------------------------------------------------------------------------------------------------
def corpus_and_keys(golden):
    g = golden("dynmix")
    arrays, roles = dr.fixture_corpus(g)
    c = df.Corpus.from_arrays(arrays, device=DEV, fs=8000)
    c.roles = roles
    return c, [str(k) for k in g["keys"]], arrays


def feeds(corpus, train_keys=None, valid_keys=None):
    train = df.DynamicMixFeed(corpus, df.plan_wsj0, batch=B, max_len=MAXLEN, seed=3, fixed_length=True, keys=train_keys)
    valid = df.DynamicMixFeed(corpus, df.plan_direct, batch=B, max_len=MAXLEN, seed=4, keys=valid_keys, drop_last=False)
    return train, valid


def make_trainer(corpus, directory, dropout=0.0, train_keys=None, valid_keys=None, **kw):
    train, valid = feeds(corpus, train_keys, valid_keys)
    kw.setdefault("max_epoch", 3)
    kw.setdefault("log", lambda s: None)
    return T.Trainer(tiny(dropout), train, valid, str(directory), lr=LR, seed=11, warmup_steps=WARMUP, **kw)


def _final(t):
    return ({k: v.detach().clone() for k, v in t.model.state_dict().items()}, t.opt._exp_avg.clone(), t.opt._exp_avg_sq.clone(), t.opt._step.clone())


def _same_final(a, b):
    return all(tr.same_bits(a[0][k], b[0][k]) for k in a[0]) and all(tr.same_bits(x, y) for x, y in zip(a[1:], b[1:]))


def test_captured_equals_eager(golden, tmp_path):
    """One epoch of four batches through Trainer (one eager step, three replays of the optimizer graph that carries the EMA launch) against
    the same four steps made eagerly with the public pieces."""
    corpus, keys, _ = corpus_and_keys(golden)
    t = make_trainer(corpus, tmp_path, train_keys=keys * 2, ema_decay=DECAY)
    assert t.train_epoch(1)[2] == 4 and t.step.calls == 3
    model = tiny().train()
    feed, _ = feeds(corpus, keys * 2)
    opt = FlatAdamW(model, lr=LR, weight_decay=1.0e-2, skip_nonfinite=True, ema_decay=DECAY)
    w_time = torch.full((), 1.0 - T.alpha(1), dtype=torch.float32, device=DEV)
    w_freq = torch.full((), T.alpha(1), dtype=torch.float32, device=DEV)
    sizes = torch.full((B,), MAXLEN)
    x, tg = torch.zeros(B, MAXLEN, device=DEV), [torch.zeros(B, MAXLEN, device=DEV) for _ in range(2)]
    for i in range(1, 5):
        opt.param_groups[0]["lr"] = tr.lambda_lr_rates(LR, WARMUP, i)[-1]
        feed.next_into(x, tg)
        opt.zero_grad(set_to_none=True)
        audio, aux = model(x)
        l_time = t.crit_t(estims=audio, input_sizes=sizes, target_attr=tg).reshape(())
        l_mag = [t.crit_m(estims=a, idx=k, input_sizes=sizes, target_attr=tg).reshape(()) for k, a in enumerate(aux)]
        T.mix_loss(l_time, l_mag, w_time, w_freq, 2).backward()
        opt.step(max_norm=5.0)
    got, want = t.opt.ema_state_dict(), opt.ema_state_dict()
    for k in want:
        assert er.same(got[k], want[k]), k
    for (k, a), (_, b) in zip(t.model.state_dict().items(), model.state_dict().items()):
        assert tr.same_bits(a, b), k
    assert tr.same_bits(t.opt._scal[6], opt._scal[6]) and float(opt._scal[6]) == float(er.one_minus(4, DECAY, EMA_WARMUP))
    assert t.read_ledger().steps == 4                                        # the ledger launch is where it was
    t.release()


def test_the_ema_does_not_touch_the_trajectory(golden, tmp_path):
    """Two epochs, each validated inside averaged(): the raw weights and the moments are those of a run without the EMA."""
    corpus, _, _ = corpus_and_keys(golden)
    a = make_trainer(corpus, tmp_path / "a", ema_decay=DECAY, validate_with="ema")
    a.run()
    b = make_trainer(corpus, tmp_path / "b")
    b.run()
    assert a.global_step == b.global_step == 4
    assert _same_final(_final(a), _final(b))
    assert a.last_train == b.last_train and a.last_valid != b.last_valid     # the same training losses; validation saw other weights


def test_validation_on_the_averaged_weights(golden, tmp_path):
    corpus, keys, _ = corpus_and_keys(golden)
    lines = []
    t = make_trainer(corpus, tmp_path / "both", max_epoch=2, start_scheduling=0, ema_decay=DECAY, validate_with="both", log=lines.append)
    t.run()
    ck = torch.load(t.last_checkpoint, map_location="cpu")
    # the averaged result: a hand loop over a fresh model loaded from the file's ema_state_dict alone
    model = tiny()
    model.load_state_dict(ck["ema_state_dict"], strict=True)
    model.eval()
    _, feed = feeds(corpus)
    per_batch = []
    with torch.inference_mode():
        for sizes, mix, src, _ in feed:
            audio, aux = model(mix)
            per_batch.append([float(t.crit_t(estims=audio, input_sizes=sizes, target_attr=src))] +
                             [float(t.crit_m(estims=a, idx=k, input_sizes=sizes, target_attr=src)) for k, a in enumerate(aux)])
    want = tr.ref_epoch_means(per_batch, 2)
    print("averaged", t.last_valid, "hand loop", want, "raw", t.last_valid_raw)
    assert t.last_valid == want
    # the raw result: a run without the EMA
    plain = make_trainer(corpus, tmp_path / "plain", max_epoch=2, start_scheduling=0)
    plain.run()
    assert t.last_valid_raw == plain.last_valid and t.last_valid_raw != t.last_valid
    # the scheduler and `best` received the averaged one
    assert t.scheduler.best == t.last_valid[0] and t.best == t.last_valid[0] and ck["valid_loss"] == t.last_valid[0]
    assert plain.scheduler.best == plain.last_valid[0] != t.scheduler.best
    valid = [ln for ln in lines if ln.startswith("[VALID]")]
    assert len(valid) == 2 and valid[0].endswith("| raw") and valid[1].endswith("| ema")
    assert f"Loss_t = {t.last_valid_raw[0]:.4f}" in valid[0] and f"Loss_t = {t.last_valid[0]:.4f}" in valid[1]
    # both passes saw the same batches, and the feed moved on once: its state is the plain run's
    assert t.valid_feed.state_dict() == plain.valid_feed.state_dict()


def test_resume_continues_bit_for_bit(golden, tmp_path):
    """Dropout on.  A: three epochs straight.  B: two epochs, every object dropped, one more from the directory."""
    corpus, _, _ = corpus_and_keys(golden)
    assert VARIANTS["tiny"].dropout > 0
    a = make_trainer(corpus, tmp_path / "a", None, max_epoch=4, ema_decay=DECAY)
    a.run()
    b = make_trainer(corpus, tmp_path / "b", None, max_epoch=3, ema_decay=DECAY)
    b.run()
    del b
    b = make_trainer(corpus, tmp_path / "b", None, max_epoch=4, ema_decay=DECAY)
    b.run()
    assert b.start_epoch == 3 and a.global_step == b.global_step == 6
    assert _same_final(_final(a), _final(b))
    ea, eb = a.opt.ema_state_dict(), b.opt.ema_state_dict()
    for k in ea:
        assert er.same(ea[k], eb[k]), k
    assert a.last_valid == b.last_valid and a.last_train == b.last_train
    assert any(not er.same(ea[k], a.model.state_dict()[k]) for k in ea)


def test_resume_from_a_file_without_the_ema(golden, tmp_path):
    corpus, _, _ = corpus_and_keys(golden)
    plain = make_trainer(corpus, tmp_path / "ck", max_epoch=2)
    plain.run()
    assert "ema_state_dict" not in torch.load(plain.last_checkpoint, map_location="cpu")
    lines = []
    t = make_trainer(corpus, tmp_path / "ck", max_epoch=3, ema_decay=DECAY, log=lines.append)
    t.opt.load_ema_state_dict({k: v + 1.0 for k, v in t.opt.ema_state_dict().items()})      # anything but the weights about to be loaded
    assert t.load_latest() == 2
    assert any("ema_state_dict" in ln and "starts again" in ln for ln in lines), lines
    got = t.opt.ema_state_dict()
    for k, p in plain.model.named_parameters():
        assert er.same(got[k], p), k


def test_checkpoint_layout(golden, tmp_path):
    corpus, _, _ = corpus_and_keys(golden)
    t = make_trainer(corpus, tmp_path / "on", max_epoch=2, ema_decay=DECAY, ema_warmup=4.0)
    t.run()
    ck = torch.load(t.last_checkpoint, map_location="cpu")
    assert set(ck) == set(T.CHECKPOINT_KEYS) | {T.RUN_STATE_KEY, "ema_state_dict"}
    rs = ck[T.RUN_STATE_KEY]
    assert set(rs) == {"global_step", "plateau", "train_feed", "valid_feed", "best", "seed", "ema"} and rs["ema"] == {"decay": DECAY, "warmup": 4.0}
    msd, esd = ck["model_state_dict"], ck["ema_state_dict"]
    assert list(esd) == list(msd)
    names = {k for k, _ in t.model.named_parameters()}
    differ = 0
    for k in msd:
        assert esd[k].shape == msd[k].shape and esd[k].dtype == msd[k].dtype, k
        if k in names:
            differ += int(not tr.same_bits(esd[k], msd[k]))
        else:
            assert tr.same_bits(esd[k], msd[k]), k                           # buffers: the model's own
    assert differ > 0 and len(names) < len(msd)
    assert "ema_state_dict" not in str(ck["optimizer_state_dict"].keys())
    # the EMA off: the file and the run state are what they were
    off = make_trainer(corpus, tmp_path / "off", max_epoch=2)
    off.run()
    ck = torch.load(off.last_checkpoint, map_location="cpu")
    assert set(ck) == set(T.CHECKPOINT_KEYS) | {T.RUN_STATE_KEY}
    assert set(ck[T.RUN_STATE_KEY]) == {"global_step", "plateau", "train_feed", "valid_feed", "best", "seed"}


def test_tools_train_and_separate_with_the_ema(golden, tmp_path):
    """tools/train_from_scp.py --ema-decay as a child process, then ``python -m sepreformer_amd.infer --ema`` on its checkpoint and on one
    written without the EMA."""
    _, keys, arrays = corpus_and_keys(golden)
    scp = {}
    for role in ("s1", "s2", "mix"):
        lines = []
        for k in keys:
            wav = str(tmp_path / f"{role}_{k}.wav")
            tr.write_wav16(wav, arrays[f"{role}/{k}"])
            lines.append(f"{k} {wav}")
        scp[role] = str(tmp_path / f"{role}.scp")
        with open(scp[role], "w") as f:
            f.write("\n".join(lines) + "\n")
    ck = str(tmp_path / "ck")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_from_scp.py"), "--form", "wsj0", "--scp", f"s1={scp['s1']}", f"s2={scp['s2']}",
           "--model", "tiny", "--precision", "bf16x3", "--batch", "2", "--max-len", "2000", "--valid-scp", f"mix={scp['mix']}", f"s1={scp['s1']}",
           f"s2={scp['s2']}", "--checkpoint-dir", ck, "--warmup-steps", "3", "--test-scp", f"mix={scp['mix']}", f"s1={scp['s1']}", f"s2={scp['s2']}",
           "--test-epochs", "1"]
    run = subprocess.run(cmd + ["--epochs", "2", "--ema-decay", "0.99"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert os.listdir(ck) == ["epoch.0001.pth"] and "[VALID] Epoch  1" in run.stdout and "[TEST] Epoch  1: SISNRi = " in run.stdout
    path = os.path.join(ck, "epoch.0001.pth")
    saved = torch.load(path, map_location="cpu")
    assert "ema_state_dict" in saved and saved[T.RUN_STATE_KEY]["ema"] == {"decay": 0.99, "warmup": 10.0}
    wav = str(tmp_path / "clip.wav")
    tr.write_wav16(wav, arrays[f"mix/{keys[0]}"][:4000])
    infer = [sys.executable, "-m", "sepreformer_amd.infer", "--model", "tiny", "--ema", wav, "--checkpoint"]
    done = subprocess.run(infer + [path], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert done.returncode == 0, done.stdout + done.stderr
    written = [wav[:-4] + s for s in ("_in.wav", "_out_0.wav", "_out_1.wav")]
    assert done.stdout.split() == written and all(os.path.getsize(w) > 44 for w in written)
    # a file without the key: the ValueError's message, a non-zero status, nothing written
    for w in written:
        os.remove(w)
    bare = str(tmp_path / "bare.pth")
    torch.save({k: v for k, v in saved.items() if k != "ema_state_dict"}, bare)
    failed = subprocess.run(infer + [bare], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert failed.returncode != 0 and "holds no ema_state_dict" in failed.stderr and bare in failed.stderr, failed.stdout + failed.stderr
    assert not any(os.path.exists(w) for w in written)
