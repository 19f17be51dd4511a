"""The branch-parity bar of the BACKWARD has teeth: proof from the reference side only (no device).  tests/branch_ref.py holds the
measure (``dx - dy`` for the residual blocks, every parameter gradient on its own), the bar and ``BWD_CASES``;
tests/test_branch_parity_bwd_gpu.py runs the same cases on the device.

  * every (case, x family, dy family): the float64 backward is finite, ``floor_db`` (float32 autograd against float64 autograd) and
    ``floor_x3_db`` (the split products, forward and backward) are finite for every tensor judged on agreement, and above 40 dB on
    ``dx - dy``; tensors judged on magnitude are ~0 in float32 autograd too;
  * ``_MMx3`` (the split product as an autograd Function) leaves the forward figures of the existing cases bit-identical, and its backward
    is the split product of the gradient;
  * every backward mutant (the oracle's exact forward with ONE defect in the gradient) is bit-identical to plain autograd with its defect
    off, and misses the fp32 bar of at least one listed (case, families, tensor) by >= 6 dB with it on;
  * the same mutants measured the old way (``agreement_db`` on whole ``dx`` / on the gradient, randn, float32 oracle, Base width, the
    shapes of tests/test_train_gpu.py) stand beside the new figures in profiles/branch_parity_bwd_mutants.json (rewritten with
    SEPR_WRITE_PROFILES=1, checked against this run otherwise).
"""
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import branch_ref as br                                                      # noqa: E402
from oracle import sepreformer_oracle as orc                                 # noqa: E402
from sepreformer_amd.config import VARIANTS                                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "branch_parity_bwd_mutants.json")
REQUIRED_MUTANTS = {"ln_bwd_xhat_term_lost", "ln_bwd_eps_1e-6", "softmax_bwd_no_rowsum", "bn_bwd_stats_constant", "dwconv_bwd_halo_lost",
                    "upsample_bwd_last_lost", "avgpool_bwd_wrong_count", "pe_k_grad_clamped_dropped", "wgrad_last_row_lost"}


def test_bwd_case_list_is_whole():
    """The shapes tests/test_train_gpu.py names, every x family against dy = randn, the four hard dy families against randn / plus100,
    one several-tile shape per residual block on WORST_FLOORS; no family removed."""
    tags = {c.tag for c in br.BWD_CASES}
    assert tags == {"gcfn_train.n2_T37", "gcfn_train.n3_T300", "gcfn_train.n1_T1", "cla_train.n2_T24", "cla_train.n2_T150", "cla_train.n3_T700",
                    "ega_train.n2_fac1_Tp25", "ega_train.n2_fac4_Tp30", "ega_train.n2_fac2_Tp130", "ega_train.n2_fac16_Tp9",
                    "spkattn_train.B3_T33", "down_train.n2_T40", "down_train.n2_T41", "down_train.n2_T6", "split.B3_T129", "fuse.B2_T24"}
    assert {c.tag for c in br.BWD_LARGE_CASES} == {"gcfn_train.n3_T2731", "cla_train.n2_T2100", "ega_train.n2_fac8_Tp300"}
    assert 3 * 2731 == 8193 and 130 > VARIANTS["tiny"].maxlen
    pairs = set(br.BWD_PAIRS)
    assert len(pairs) == len(br.BWD_PAIRS) == len(br.ROW_FAMILIES) + 8
    assert {(xf, "randn") for xf in br.ROW_FAMILIES} <= pairs
    assert {(xf, df) for xf in ("randn", "plus100") for df in ("row_range", "silent_rows", "loud", "zeros")} <= pairs
    assert all(c.families == br.BWD_PAIRS for c in br.BWD_CASES)
    assert all(c.families == [(xf, "randn") for xf in br.WORST_FLOORS] for c in br.BWD_LARGE_CASES)
    assert not br.REMOVED_FAMILIES
    import test_train_gpu as ttg
    assert br.STRUCTURAL_ZERO == ttg.STRUCTURAL_ZERO
    # dy has a seed of its own: it is not the x of the same family
    case, cfg = br.BWD_CASES[0], VARIANTS["tiny"]
    assert not torch.equal(br.make_dy(case, cfg, "randn"), br.make_inputs(case, cfg, "randn")["x"])
    assert float(br.make_dy(case, cfg, "zeros").abs().max()) == 0.0


def test_reference_bwd_is_autograd_over_the_oracle():
    """reference_bwd against the lines tests/test_train_gpu.py::test_ega_train writes out (float32): same dx, same gradients, pe_k among them."""
    from oracle import train_oracle as tor
    cfg = VARIANTS["tiny"]
    case = next(c for c in br.BWD_CASES if c.tag == "ega_train.n2_fac2_Tp130")
    inp, dy = br.make_inputs(case, cfg, "randn"), br.make_dy(case, cfg, "randn")
    dx, res, grads = br.reference_bwd(case, "tiny", torch.float32, inp, dy)
    sdl = tor.leaf_state(br.state("tiny"))
    xl = inp["x"].permute(0, 2, 1).clone().requires_grad_(True)
    p = br.E0 + ".g_block_1.block.ega"
    orc.ega(sdl, p, xl, orc.rel_pos_k(sdl, 130, cfg.maxlen), cfg.heads).backward(dy)
    assert torch.equal(dx["dx"], xl.grad.permute(0, 2, 1)) and torch.equal(res, dy)
    want = {k: v.grad for k, v in sdl.items() if (k.startswith(p + ".") or k == br.PE_K) and v.requires_grad and v.grad is not None}
    assert set(grads) == set(want) and br.PE_K in grads
    assert all(torch.equal(grads[k], want[k]) for k in want)
    assert br.reference_bwd(br.BWD_CASES[-1], "tiny", torch.float64, br.make_inputs(br.BWD_CASES[-1], cfg, "randn"),
                            br.make_dy(br.BWD_CASES[-1], cfg, "randn"))[1] is None          # fuse: no residual


@pytest.mark.parametrize("tag", ["ega.n2_fac4_Tp130", "gcfn.n2_T37"])
def test_mm_x3_function_keeps_the_forward_figures(tag, monkeypatch):
    """The existing floors() of two cases with ``_mm_x3`` as the autograd Function and as the plain split product: the same bits."""
    case = next(c for c in br.BLOCK_CASES if c.tag == tag)
    for fam in ("randn", "plus100"):
        r = br.floors(case, "tiny", fam)
        y_fn, _ = br.reference_x3(case, "tiny", r["inp"])
        with monkeypatch.context() as mp:
            mp.setattr(br, "_mm_x3", br._mm_x3_raw)
            y_raw, _ = br.reference_x3(case, "tiny", r["inp"])
        assert torch.equal(y_fn, y_raw)
        assert br.branch_db(y_raw, r["x64"], r["y64"], r["x64"]) == r["floor_x3_db"]


def test_mm_x3_backward_is_the_split_product_of_the_gradient():
    g = torch.Generator().manual_seed(5)
    for sa, sb in (((3, 7, 16), (16, 24)), ((2, 4, 9, 8), (2, 4, 8, 9)), ((9, 8, 8), (9, 8, 9))):   # Linear, q k^T, the positional product
        a = torch.randn(*sa, generator=g, dtype=torch.float64).requires_grad_(True)
        b = torch.randn(*sb, generator=g, dtype=torch.float64).requires_grad_(True)
        dc = torch.randn(*torch.matmul(a, b).shape, generator=g, dtype=torch.float64)
        br._mm_x3(a, b).backward(dc)
        assert torch.equal(a.grad, br._mm_x3_raw(dc, b.detach().transpose(-1, -2)).sum_to_size(a.shape))
        assert torch.equal(b.grad, br._mm_x3_raw(a.detach().transpose(-1, -2), dc).sum_to_size(b.shape))
        a2, b2 = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
        torch.matmul(a2, b2).backward(dc)
        # 2^-15.4 per product (module docstring of branch_ref) is 93 dB; differentiating _mm_x3_raw itself reads ~50 dB (bf16-rounded gradient)
        assert orc.agreement_db(a.grad, a2.grad) > 85.0 and orc.agreement_db(b.grad, b2.grad) > 85.0


@pytest.mark.parametrize("case", br.BWD_CASES + br.BWD_LARGE_CASES, ids=repr)
def test_bwd_floors_are_finite(case):
    for xf, df in case.families:
        r = br.floors_bwd(case, "tiny", xf, df)
        assert r["finite"], (case, xf, df)
        assert set(r["rule"]) == set(r["dx64"]) | set(r["g64"])
        for n, rule in r["rule"].items():
            where = (case, xf, df, n)
            if df == "zeros":
                assert rule == "zero" and float((r["dx64"].get(n, r["g64"].get(n))).abs().max()) == 0.0, where    # exactly 0 in the reference too
            elif rule == "magnitude":
                assert r["g32_max"][n] <= br.MAG_TOL * r["scale"], where
            else:
                f, f3 = r["floor_db"][n], r["floor_x3_db"][n]
                assert math.isfinite(f) and math.isfinite(f3), where + (f, f3)
                if n in r["dx64"]:
                    assert f > 40.0 and f3 > 40.0, where + (f, f3)
        if df != "zeros":
            assert all(r["rule"][n] == "db" for n in r["dx64"]), (case, xf, df)


# ----------------------------------------------------------------------------------------------------------------------
# mutants
# ----------------------------------------------------------------------------------------------------------------------
def test_mutant_list_is_whole():
    assert set(br.bwd_mutants()) >= REQUIRED_MUTANTS
    kinds = {c.kind for c in br.BWD_CASES}
    assert all(m["kinds"] <= kinds for m in br.bwd_mutants().values())


def _bwd(case, variant, dtype, r, ctx=None):
    if ctx is None:
        return br.reference_bwd(case, variant, dtype, r["inp"], r["dy"])
    with ctx():
        return br.reference_bwd(case, variant, dtype, r["inp"], r["dy"])


# the case each Function is compared with plain autograd on (T 300 > 128 for the halo, fac 2 for upsample / pool, Tp 130 for the clamp)
OFF_CASE = {"bn_bwd_stats_constant": "cla_train.n2_T150", "dwconv_bwd_halo_lost": "gcfn_train.n3_T300"}


@pytest.mark.parametrize("name", list(br.bwd_mutants()))
def test_function_with_defect_off_is_plain_autograd(name):
    m = br.bwd_mutants()[name]
    tag = OFF_CASE.get(name, "ega_train.n2_fac2_Tp130")
    case = next(c for c in br.BWD_CASES if c.tag == tag)
    assert case.kind in m["kinds"]
    for dtype in (torch.float64, torch.float32):
        r = br.floors_bwd(case, "tiny", "randn", "randn", want_x3=False)
        dx, _, g = _bwd(case, "tiny", dtype, r)
        dx_f, _, g_f = _bwd(case, "tiny", dtype, r, m["off"])
        assert all(torch.equal(dx[k], dx_f[k]) for k in dx), name
        assert set(g) == set(g_f) and all(torch.equal(g[k], g_f[k]) for k in g), name
        dx_m, _, g_m = _bwd(case, "tiny", dtype, r, m["ctx"])          # ... and the defect does change something there
        assert not (all(torch.equal(dx[k], dx_m[k]) for k in dx) and all(torch.equal(g[k], g_m[k]) for k in g)), name


def _short(n):
    return n if "." not in n else ".".join(n.split(".")[-2:])


def _survey(m):
    """Every listed (case, x family, dy family, tensor) at tiny width the mutant can touch -> its figure against the clean float64 backward."""
    rows = []
    for case in br.BWD_CASES:
        if case.kind not in m["kinds"]:
            continue
        for xf, df in case.families:
            r = br.floors_bwd(case, "tiny", xf, df)
            if df == "zeros":
                continue
            dx_m, _, g_m = _bwd(case, "tiny", torch.float64, r, m["ctx"])
            for n, v in list(dx_m.items()) + list(g_m.items()):
                if r["rule"][n] != "db":
                    continue
                rows.append({"case": case.tag, "x": xf, "dy": df, "tensor": _short(n), "mutant_db": br.measure_bwd(r, n, v),
                             "bar_fp32_db": br.bar(r["floor_db"][n]), "bar_bf16x3_db": br.bar(r["floor_db"][n], r["floor_x3_db"][n])})
    return rows


# Base width, randn, float32, at the shape tests/test_train_gpu.py runs the block at: where each mutant's old-way figures are taken
# (the clamp of pe_k is reached at tiny width only - Base has maxlen 2000 - so that mutant's old way is test_ega_train[tiny] at Tp 130)
OLD_VARIANT = {"pe_k_grad_clamped_dropped": "tiny"}
OLD_WAY = {"ln_bwd_xhat_term_lost": "gcfn_train.n3_T300", "ln_bwd_eps_1e-6": "gcfn_train.n3_T300", "softmax_bwd_no_rowsum": "ega_train.n2_fac2_Tp130",
           "bn_bwd_stats_constant": "cla_train.n2_T150", "dwconv_bwd_halo_lost": "gcfn_train.n3_T300", "upsample_bwd_last_lost": "ega_train.n2_fac2_Tp130",
           "avgpool_bwd_wrong_count": "ega_train.n2_fac2_Tp130", "pe_k_grad_clamped_dropped": "ega_train.n2_fac2_Tp130",
           "wgrad_last_row_lost": "cla_train.n3_T700"}


def _old_way(name, m):
    """What test_gcfn_train / test_cla_train / test_ega_train measure: agreement_db on whole dx and on every gradient that is not a
    structural zero, float32 autograd, randn x and dy; the lowest of them decides whether the 80 dB bar passes."""
    case = next(c for c in br.BWD_CASES if c.tag == OLD_WAY[name])
    variant = OLD_VARIANT.get(name, br.BASE)
    cfg = VARIANTS[variant]
    r = {"inp": br.make_inputs(case, cfg, "randn"), "dy": br.make_dy(case, cfg, "randn")}
    dx, _, g = _bwd(case, variant, torch.float32, r)
    dx_m, _, g_m = _bwd(case, variant, torch.float32, r, m["ctx"])
    db = lambda a, b: 999.0 if torch.equal(a, b) else orc.agreement_db(a, b)      # noqa: E731  (999 = untouched by the defect)
    fig = {"dx": db(dx_m["dx"], dx["dx"])}
    fig.update({_short(k): db(g_m[k], g[k]) for k in g if not k.endswith(br.STRUCTURAL_ZERO)})
    low = min(fig, key=fig.get)
    # the same case the new way (float64, the branch)
    d64, _, g64 = _bwd(case, variant, torch.float64, r)
    m64, _, _ = _bwd(case, variant, torch.float64, r, m["ctx"])
    if torch.equal(m64["dx"], d64["dx"]):
        m64["dx"] = None
    return {"variant": variant, "case": case.tag, "x": "randn", "dy": "randn", "agreement_on_whole_dx_db": fig["dx"], "lowest_tensor": low,
            "lowest_agreement_db": fig[low], "passes_old_80_db_bar": bool(fig[low] >= br.MIN_DB),
            "branch_db_on_dx_at_this_case": 999.0 if m64["dx"] is None else br.branch_db(m64["dx"], r["dy"].double(), d64["dx"], r["dy"].double())}


_results = {}


@pytest.mark.parametrize("name", list(br.bwd_mutants()))
def test_bwd_mutant_is_rejected(name):
    m = br.bwd_mutants()[name]
    rows = _survey(m)
    assert rows, name
    best = max(rows, key=lambda r: r["bar_fp32_db"] - r["mutant_db"])
    best3 = max(rows, key=lambda r: r["bar_bf16x3_db"] - r["mutant_db"])
    old = _old_way(name, m)
    rd = lambda v: round(float(v), 1)                                       # noqa: E731
    keys = ("case", "x", "dy", "tensor")
    _results[name] = {
        "new": dict({k: best[k] for k in keys}, variant="tiny", mutant_db=rd(best["mutant_db"]), bar_fp32_db=rd(best["bar_fp32_db"]),
                    spare_db=rd(best["bar_fp32_db"] - best["mutant_db"])),
        "new_bf16x3": dict({k: best3[k] for k in keys}, variant="tiny", mutant_db=rd(best3["mutant_db"]), bar_bf16x3_db=rd(best3["bar_bf16x3_db"]),
                           spare_db=rd(best3["bar_bf16x3_db"] - best3["mutant_db"])),
        "figures_that_reject_it": sum(1 for r in rows if r["bar_fp32_db"] - r["mutant_db"] >= br.MARGIN_DB), "figures_tried": len(rows),
        "old": {k: (rd(v) if isinstance(v, float) else v) for k, v in old.items()},
    }
    print(name, json.dumps(_results[name]))
    assert best["bar_fp32_db"] - best["mutant_db"] >= br.MARGIN_DB, f"{name}: no listed figure sees it with 6 dB to spare (best {best})"
    assert best3["bar_bf16x3_db"] - best3["mutant_db"] >= br.MARGIN_DB, f"{name}: invisible under the bf16x3 bar (best {best3})"


def test_bwd_mutant_record():
    """profiles/branch_parity_bwd_mutants.json is this run's result (SEPR_WRITE_PROFILES=1 rewrites it): every mutant rejected with >= 6 dB
    to spare, and it says which of them the 80 dB bar on whole tensors, randn, let through."""
    names = list(br.bwd_mutants())
    for n in names:
        if n not in _results:                                               # run on its own: measure here
            test_bwd_mutant_is_rejected(n)
    if os.environ.get("SEPR_WRITE_PROFILES") == "1":
        doc = {"what": "the oracle's forward with one defect planted in the backward, against clean float64 autograd: 'new' = the listed "
                       "(case, x family, dy family, tensor) at tiny width that sees it best (dx on the branch dx - dy, a parameter gradient on its "
                       "own) against that figure's bar min(80, floor - 6); 'old' = agreement on whole dx and on every gradient, randn, float32 "
                       "autograd, Base width, at the shape the training tests use (tests/test_branch_parity_bwd_cpu.py)",
               "passed_by_the_old_80_db_bar": sorted(n for n in names if _results[n]["old"]["passes_old_80_db_bar"]),
               "mutants": _results}
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(PROFILE) as f:
        doc = json.load(f)
    rec = doc["mutants"]
    assert set(rec) == set(names) >= REQUIRED_MUTANTS
    for n in names:
        assert rec[n]["new"]["spare_db"] >= br.MARGIN_DB, n
        assert abs(rec[n]["new"]["spare_db"] - _results[n]["new"]["spare_db"]) <= 1.0, n
        assert abs(rec[n]["old"]["lowest_agreement_db"] - _results[n]["old"]["lowest_agreement_db"]) <= 1.0, n
        assert rec[n]["old"]["passes_old_80_db_bar"] == _results[n]["old"]["passes_old_80_db_bar"], n
    assert doc["passed_by_the_old_80_db_bar"] == sorted(n for n in names if rec[n]["old"]["passes_old_80_db_bar"])
    assert "ln_bwd_eps_1e-6" in doc["passed_by_the_old_80_db_bar"]          # randn never reaches the eps: only `quiet` shows it
