"""Device backward judged on the part it computes, in float64, on hard inputs (measure, bar, families, ``BWD_CASES``: tests/branch_ref.py;
the proof that this bar rejects defects planted in the backward: tests/test_branch_parity_bwd_cpu.py).

Every case goes through the TrainEngine calls tests/test_train_gpu.py drives it with (``block_fwd`` / ``block_bwd``, the down / split / fuse
pairs; dropout 0, gradient buffer zeroed before each).  ``dx`` of the four residual blocks is judged on ``dx - dy``, every parameter
gradient of the block (EGA: ``pe_k`` too) on its own, each against ``bar = min(80 dB, floor_db - 6 dB)`` (bf16x3: also
``floor_x3_db - 6 dB``) with both floors from float64 / float32 autograd over the oracle on that very case.  A tensor whose float64
gradient is nothing (structural zeros; what ``zeros`` makes exactly zero) is judged on magnitude, ``max|g| <= 1e-3 x scale``; with
``dy = zeros`` every gradient and ``dx`` must be exactly 0 (stale partials, 0 x inf, a finisher adding into an unzeroed buffer).
Everything must be finite.

Plain ``bf16`` runs the same cases with finiteness and the ``dy = zeros`` exactness required and every figure recorded, without a dB
bar: what one bf16 MFMA per product should reach on the branch gradient does not follow from the split argument; the recorded figures
are what a bar can be set from.

Every figure goes through record() of tests/test_gpu_parity.py into its parity_report.json as
``branch_bwd.<variant>.<precision>.<case>.<x family>.<dy family>.<tensor>`` with ``....floor_db`` (and ``....floor_x3_db``) beside it.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import branch_ref as br                                                      # noqa: E402
import test_gpu_parity as tgp                                               # noqa: E402
import test_train_gpu as ttg                                                # noqa: E402

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp32", "bf16x3"]
RECORDED_ONLY = "bf16"                                                      # no dB bar (module docstring)


class Judge:
    """Measures every tensor of every (case, x family, dy family) of one test and fails at the end with all of them."""

    def __init__(self, variant, precision):
        self.variant, self.precision, self.bad, self.worst = variant, precision, [], {}
        self.barred = precision != RECORDED_ONLY

    def check(self, case, xf, df, r, got_of):
        """``got_of(name)``: the device tensor of ``name`` (a ``dx`` name or a state-dict key) as a float32 host tensor."""
        cfg = ttg.VARIANTS[self.variant]
        pre = br.param_prefixes(case, cfg)
        for n, rule in r["rule"].items():
            short = n if n in r["dx64"] else ("pe_k" if n == br.PE_K else n[len(next(p for p in pre if n.startswith(p))):])
            name = f"branch_bwd.{self.variant}.{self.precision}.{case.tag}.{xf}.{df}.{short}"
            want = r["dx64"][n] if n in r["dx64"] else r["g64"][n]
            got = got_of(n)
            if got.shape != want.shape:
                self.bad.append(f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}")
                continue
            if not torch.isfinite(got).all():
                tgp.REPORT[name] = -999.0
                self.bad.append(f"{name}: non-finite values")
                continue
            if rule == "zero":                                        # dy = zeros: exactly 0, whatever the precision
                top = float(got.abs().max())
                tgp.REPORT[name + ".max_abs"] = top
                if top != 0.0:
                    self.bad.append(f"{name}: max|.| {top:.3e} with dy = 0")
                continue
            if rule == "magnitude":
                rel = float(got.abs().max()) / (r["scale"] + 1e-300)
                tgp.REPORT[name + ".zero_rel"] = float(f"{rel:.3e}")
                if self.barred and not rel <= br.MAG_TOL:
                    self.bad.append(f"{name}: max|g| is {rel:.2e} of the block's largest gradient, the float64 gradient is ~0")
                continue
            x3 = r["floor_x3_db"][n] if self.precision == "bf16x3" else None
            db = br.measure_bwd(r, n, got)
            tgp.REPORT[name] = round(db, 2)
            tgp.REPORT[name + ".floor_db"] = round(r["floor_db"][n], 2)
            if x3 is not None:
                tgp.REPORT[name + ".floor_x3_db"] = round(x3, 2)
            if not self.barred:
                continue
            need = br.bar(r["floor_db"][n], x3)
            key = br.BWD_KIND[case.kind]
            if key not in self.worst or db - need < self.worst[key][0]:
                self.worst[key] = (db - need, name, db, need)
            if not db >= need:
                self.bad.append(f"{name}: {db:.1f} dB < bar {need:.1f} (floor {r['floor_db'][n]:.1f}" + (f", x3 floor {x3:.1f})" if x3 is not None else ")"))

    def done(self, what):
        for kind, (_, name, db, need) in sorted(self.worst.items()):
            print(f"closest to its bar: {name} {db:.1f} dB (bar {need:.1f})")
            tgp.REPORT[f"branch_bwd.{self.variant}.{self.precision}.{what}.{kind}.least_spare_db"] = round(db - need, 2)
        tgp.record(f"branch_bwd.{self.variant}.{self.precision}.{what}.failures", len(self.bad))      # one write of everything gathered above
        assert not self.bad, f"{len(self.bad)} failed: " + "; ".join(self.bad[:60])


def run_bwd(cfg, sdd, tp, eng, case, r):
    """Forward + backward of one case on the device, as tests/test_train_gpu.py drives the kind -> {dx name: device tensor}."""
    k, s = br.BWD_KIND[case.kind], case.shape
    S = cfg.num_spks
    d = {n_: t.cuda() for n_, t in r["inp"].items()}
    dy = r["dy"].cuda()
    bn = {"cla": br.E0 + ".l_block_1.block.cla.BN.", "down": br.E0 + ".downconv.BN."}.get(k)
    keep = {n_: sdd[bn + n_].clone() for n_ in ("running_mean", "running_var")} if bn else {}     # shared device state: put back below
    if k == "gcfn":
        _, rec = eng.block_fwd("gcfn", d["x"], tp.gcfn[0], s["n"], s["T"])
        out = {"dx": eng.block_bwd(rec, dy)}
    elif k == "cla":
        _, rec = eng.block_fwd("cla", d["x"], tp.cla[0], s["n"], s["T"])
        out = {"dx": eng.block_bwd(rec, dy)}
    elif k == "ega":
        _, rec = eng.block_fwd("ega", d["x"], tp.ega[0], s["n"], s["Tp"] * s["fac"], s["Tp"])
        out = {"dx": eng.block_bwd(rec, dy)}
    elif k == "spkattn":
        _, rec = eng.block_fwd("spk", d["x"], tp.spk[0], s["B"] * S, s["T"])
        out = {"dx": eng.block_bwd(rec, dy)}
    elif k == "down":
        _, cx, To = eng.down_fwd(d["x"], tp.down[0], s["n"], s["T"])
        assert To == dy.shape[1]
        out = {"dx": eng.down_bwd(d["x"], cx, tp.down[0], dy, s["n"], s["T"])}
    elif k == "split":
        _, cx = eng.split_fwd(d["x"], tp.splits[0], s["B"], s["T"])
        dx = torch.empty_like(d["x"])
        eng.split_bwd(d["x"], cx, tp.splits[0], dy, dx, False, s["B"], s["T"])
        out = {"dx": dx}
    elif k == "fuse":
        eng.fuse_fwd(d["lo"], d["sk"], tp.fuse[0], s["B"] * S, s["T"])
        dlo, dsk = eng.fuse_bwd(d["lo"], d["sk"], tp.fuse[0], dy, s["B"] * S, s["T"])
        out = {"dlo": dlo, "dskip": dsk}
    else:
        raise KeyError(case.kind)
    torch.cuda.synchronize()
    for n_, v in keep.items():
        sdd[bn + n_].copy_(v)
    return out


def _run(variant, precision, cases, what):
    cfg, sd, sdd, gb, tp, eng = ttg.setup(variant, precision)
    judge = Judge(variant, precision)
    for case in cases:
        for xf, df in case.families:
            r = br.floors_bwd(case, variant, xf, df, want_x3=(precision == "bf16x3"))       # host references: cached across the precisions
            gb.flat.zero_()
            dxs = run_bwd(cfg, sdd, tp, eng, case, r)
            judge.check(case, xf, df, r, lambda n: (dxs[n] if n in dxs else gb.view(n)).detach().float().cpu())
    gb.flat.zero_()
    judge.done(what)


@pytest.mark.parametrize("precision", PRECISIONS + [RECORDED_ONLY])
@pytest.mark.parametrize("variant", br.GPU_VARIANTS)
def test_branch_bwd_blocks(variant, precision):
    """The shapes of the training tests x every x family (dy = randn) and the hard dy families (x = randn, plus100)."""
    _run(variant, precision, br.BWD_CASES, "blocks")


@pytest.mark.parametrize("precision", PRECISIONS + [RECORDED_ONLY])
@pytest.mark.parametrize("variant", br.GPU_VARIANTS)
def test_branch_bwd_several_tiles(variant, precision):
    """GCFN 8193 rows, CLA n2 T2100, EGA pool 8 T' 300: randn and the three families with the lowest floors."""
    _run(variant, precision, br.BWD_LARGE_CASES, "several_tiles")
