"""``sepr_global_block_fwd``: the EGA gate inside the GCFN kernel against the two launches it replaces - bit for bit.

A frame's value must not depend on which path computed it (the batch-pipeline and batch-1 goldens compare launch forms with each other), so
every comparison here is ``torch.equal``, of the gate output ``y_mid`` and of the block output ``y``, between the entry with SEPR_GB_FUSE on
and off and against ``sepr_ega_fwd`` + ``sepr_gcfn_fwd``.  The switch is a latched knob: flipped with the environment + ``sepr_knobs_reload``.
"""
import ctypes as C
import os

import pytest
import torch

from sepreformer_amd import lib as L
from sepreformer_amd.config import VARIANTS
from sepreformer_amd.model import Model
from sepreformer_amd.synth import synth_mixture

pytestmark = pytest.mark.gpu
BASE = "SepReformer_Base_WSJ0"
_model = {}


def base_model():
    if "m" not in _model:
        _model["m"] = Model.from_config(VARIANTS[BASE], init_seed=0, precision="bf16x3").load_synthetic_(0).eval().to("cuda")
    return _model["m"]


class fuse_switch:
    """SEPR_GB_FUSE for the duration of a block, re-latched on the way in and out."""

    def __init__(self, on):
        self.val = "1" if on else "0"

    def __enter__(self):
        self.old = os.environ.get("SEPR_GB_FUSE")
        os.environ["SEPR_GB_FUSE"] = self.val
        L.load().sepr_knobs_reload()
        assert L.load().sepr_knob(L.KNOB_GB_FUSE) == int(self.val)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("SEPR_GB_FUSE", None)
        else:
            os.environ["SEPR_GB_FUSE"] = self.old
        L.load().sepr_knobs_reload()


def entry(eng, x, gw, n, T, Tp):
    """(y_mid, y) of one call; both buffers start as NaN so a row nobody wrote cannot compare equal."""
    cfg = eng.cfg
    mid = torch.full_like(x, float("nan"))
    y = torch.full_like(x, float("nan"))
    L.check(eng.lib.sepr_global_block_fwd(x.data_ptr(), mid.data_ptr(), y.data_ptr(), n, T, Tp, cfg.feat, cfg.heads, C.byref(gw[0]), C.byref(gw[1]),
                                          gw[2] or None, *eng._wsargs, eng._st), "sepr_global_block_fwd")
    torch.cuda.synchronize()
    return mid, y


def first_diff(a, b):
    d = (a != b) | (a.isnan() != b.isnan())
    idx = d.reshape(-1, a.shape[-1]).nonzero()
    return None if idx.numel() == 0 else (int(idx[0, 0]), int(idx[0, 1]), int(d.sum()))


# (n, T, Tp): every pooling factor of the Base model (16, 8, 4, 2); M = n*T just above the 17000-row small-launch threshold; T not a multiple of
# the 126-frame tile, so tiles straddle sequence boundaries and the last tile is partial; T == Tp takes the fallback; the last is bench scale
CASES = [(24, 800, 50), (17, 1040, 130), (15, 1200, 300), (18, 1000, 500), (21, 810, 405), (30, 600, 600), (32, 8000, 500)]


@pytest.mark.parametrize("n,T,Tp", CASES)
def test_global_block_entry_bit_identical(n, T, Tp):
    m = base_model()
    eng = m.engine()
    F = eng.cfg.feat
    assert F == 128 and n * T >= 17000
    eng.prepare(n, 4 * T, T)
    c = eng.cfg
    eng._wsargs = eng._workspace(max(eng.lib.sepr_workspace_bytes(op, n, T, Tp, F, c.enc_channels, c.num_spks) for op in (L.OP_EGA, L.OP_GCFN)))
    gw = eng.pk.enc_stages[0]["g"][1]
    assert gw[2], "the permuted gate pack is built for the Base model"
    x = (torch.randn(n, T, F, generator=torch.Generator().manual_seed(T + n)) * 1.5).cuda()
    with fuse_switch(False):
        mid0, y0 = entry(eng, x, gw, n, T, Tp)
        mid_ref = eng.ega(x, gw[0], n, T, Tp)
        y_ref = eng.gcfn(mid_ref, gw[1], n, T)
        torch.cuda.synchronize()
    with fuse_switch(True):
        mid1, y1 = entry(eng, x, gw, n, T, Tp)
    assert torch.isfinite(mid1).all() and torch.isfinite(y1).all()
    assert torch.equal(mid0, mid_ref) and torch.equal(y0, y_ref)
    print(f"n={n} T={T} Tp={Tp}: first differing (row, channel, count) y_mid {first_diff(mid1, mid0)}  y {first_diff(y1, y0)}")
    assert torch.equal(mid1, mid0), first_diff(mid1, mid0)
    assert torch.equal(y1, y0), first_diff(y1, y0)


@pytest.mark.parametrize("B", [32, 16])
def test_model_forward_bit_identical(B):
    m = base_model()
    x = (synth_mixture(B, 32000, seed=11) * 4).cuda()
    outs = []
    for on in (False, True):
        with fuse_switch(on), torch.no_grad():
            audio, aux = m(x)
            torch.cuda.synchronize()
            outs.append(([a.clone() for a in audio], [[t.clone() for t in a] for a in aux]))
    (a0, x0), (a1, x1) = outs
    for s in range(len(a0)):
        assert torch.equal(a0[s], a1[s]), ("audio", s, first_diff(a1[s], a0[s]))
    for i in range(len(x0)):
        for s in range(len(x0[i])):
            assert torch.equal(x0[i][s], x1[i][s]), (f"aux_{i}", s, first_diff(x1[i][s], x0[i][s]))
