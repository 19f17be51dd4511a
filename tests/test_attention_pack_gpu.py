"""The packed-K form of the dk = 16 bf16x3 attention (``relattn_x3p_kernel``, SEPR_ATTN_PACK) through ``sepr_ega_fwd``.

Every case is an ``ega`` case of tests/branch_ref.py driven as tests/test_branch_parity_gpu.py::run_block drives it, precision bf16x3.  With
the switch on, every family of every case must be finite and agree with the float64 reference on the branch to the project's own bar
``br.bar(floor_db, floor_x3_db)`` (from the reference alone, 6 dB margin).  The figure with the switch off is recorded beside it
(``attn_pack.<variant>.<shape>.<family>.on/.off`` in parity_report.json) as information: the packed product carries the fourth term
lo.lo, so it should read about equal or higher (measured: -0.13 to +0.47 dB).  The switch is a latched knob: flipped with the
environment + ``sepr_knobs_reload``.

Shapes (the smallest at which this kernel can go wrong): tiny (F 64, 4 heads, dk 16, maxlen 40) T' = 1, 15, 16, 17 - a wave with one
active query, the 16-query tile edge; 63, 64, 65 - the 64-query workgroup edge, the 64-key tile edge, the key-bound pass, relative
positions beyond +-maxlen on both sides; n 3, pool 2, T' 130 - three key tiles, the clamp, the pooled path, sequence indexing; Base width
(F 128, 8 heads) T' = 65, 129 - eight heads and the pre-split position table (``pe_k_planes``).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import branch_ref as br                                                      # noqa: E402
import test_gpu_parity as tgp                                               # noqa: E402
from sepreformer_amd import lib as L                                        # noqa: E402

pytestmark = pytest.mark.gpu
PRECISION = "bf16x3"
CASES = {
    "tiny": [br.Case("ega", br.ROW_FAMILIES, n=2, fac=1, Tp=Tp) for Tp in (1, 15, 16, 17, 63, 64, 65)]
    + [br.Case("ega", br.ROW_FAMILIES, n=3, fac=2, Tp=130)],
    br.BASE: [br.Case("ega", br.ROW_FAMILIES, n=2, fac=1, Tp=Tp) for Tp in (65, 129)],
}
DETERMINISM = [("tiny", 65), (br.BASE, 129)]
GOLDEN_OFF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_pack_off_tiny.npz")


class pack_switch:
    """SEPR_ATTN_PACK for the duration of a block, re-latched on the way in and out."""

    def __init__(self, val):
        self.val = str(int(val))

    def __enter__(self):
        self.old = os.environ.get("SEPR_ATTN_PACK")
        os.environ["SEPR_ATTN_PACK"] = self.val
        L.load().sepr_knobs_reload()
        assert L.load().sepr_knob(L.KNOB_ATTN_PACK) == int(self.val)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("SEPR_ATTN_PACK", None)
        else:
            os.environ["SEPR_ATTN_PACK"] = self.old
        L.load().sepr_knobs_reload()


def engine(variant):
    m, _ = tgp.gpu_model(variant, PRECISION)
    eng = m.engine()
    eng.prepare(8, 2400, 2400)
    assert m.cfg.feat // m.cfg.heads == 16, "the packed kernel is the dk = 16 one"
    return m, eng


def run_ega(eng, case, x, knob):
    """``sepr_ega_fwd`` of one case with the switch at ``knob``, as run_block drives the "ega" kind."""
    s = case.shape
    with pack_switch(knob):
        y = eng.ega(x, eng.pk.enc_stages[0]["g"][0][0], s["n"], s["Tp"] * s["fac"], s["Tp"])
        torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("variant", list(CASES))
def test_attention_pack_branch(variant):
    m, eng = engine(variant)
    bad = []
    for case in CASES[variant]:
        shape = "_".join(f"{k}{v}" for k, v in case.shape.items())
        for fam in case.families:
            r = br.floors(case, variant, fam, want_x3=True)
            need = br.bar(r["floor_db"], r["floor_x3_db"])
            x = r["inp"]["x"].cuda()
            x32 = r["x64"].float()
            db = {}
            for tag, knob in (("on", 1), ("off", 0)):
                y = run_ega(eng, case, x, knob).float().cpu()
                finite = bool(torch.isfinite(y).all()) and y.shape == r["y64"].shape
                db[tag] = br.branch_db(y, x32, r["y64"], r["x64"]) if finite else -999.0
                tgp.REPORT[f"attn_pack.{variant}.{shape}.{fam}.{tag}"] = round(db[tag], 2)
            print(f"attn_pack.{variant}.{shape}.{fam}: on {db['on']:.2f} dB  off {db['off']:.2f} dB  bar {need:.2f} "
                  f"(floor {r['floor_db']:.2f}, x3 floor {r['floor_x3_db']:.2f})")
            if db["on"] == -999.0:
                bad.append(f"{variant}.{shape}.{fam}: non-finite or misshapen output")
            elif not db["on"] >= need:
                bad.append(f"{variant}.{shape}.{fam}: {db['on']:.1f} dB < bar {need:.1f}")
    tgp.record(f"attn_pack.{variant}.failures", len(bad))                  # one write of everything gathered above
    assert not bad, f"{len(bad)} below the bar: " + "; ".join(bad[:60])


@pytest.mark.parametrize("variant,Tp", DETERMINISM)
def test_attention_pack_deterministic(variant, Tp):
    """Two runs of the packed kernel on one input are bit-identical (the packed-add incident of DESIGN.md section 10 showed as run-to-run
    differences in exactly this kernel's bias path)."""
    m, eng = engine(variant)
    case = next(c for c in CASES[variant] if c.shape["Tp"] == Tp)
    x = br.make_inputs(case, m.cfg, "randn")["x"].cuda()
    a = run_ega(eng, case, x, 1).clone()
    b = run_ega(eng, case, x, 1)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), int((a != b).sum())


def test_attention_pack_off_is_the_old_kernel():
    """SEPR_ATTN_PACK=0 gives, bit for bit, what the library gave before the packed kernel existed: the stored output of that library
    (tests/golden/make_attn_pack_golden.py) for tiny, n 2, T' 65, randn.  That relattn_x3_kernel's device code is unchanged for every shape is
    shown by the disassembly comparison in profiles/attn_pack_device_code.txt; this is the run-time end of it (the dispatch).  The fixture holds
    the whole ``sepr_ega_fwd`` output: a change to any other kernel of that entry that moves a bit needs the fixture made again."""
    m, eng = engine("tiny")
    case = next(c for c in CASES["tiny"] if c.shape["Tp"] == 65)
    x = br.make_inputs(case, m.cfg, "randn")["x"]
    g = np.load(GOLDEN_OFF)
    assert np.array_equal(g["x"], x.numpy()), "the fixture was made for another input"
    y = run_ega(eng, case, x.cuda(), 0).cpu()
    want = torch.from_numpy(g["y"])
    assert torch.equal(y, want), int((y != want).sum())
    y_on = run_ega(eng, case, x.cuda(), 1).cpu()
    assert not torch.equal(y_on, want), "the switch changed nothing: the packed kernel did not run"
