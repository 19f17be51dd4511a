"""The bars the training criteria are held to on hard inputs have teeth: proof from the reference side only (no device).
tests/criterion_ref.py holds the cases, the float64 reference, the float32 floor, the restatement of the device's algorithm, the rules and
the mutants; tests/test_criterion_hard_gpu.py runs the same cases on the device.

  * every (case, kind): float64 autograd over the oracle is finite; the restatement without a mutant passes every rule it is judged by
    (row figures, exact zeros, permutation, losses); every bar is >= 55 dB except on ``dc100`` (float32 means at |mean| = 100);
  * every family does what it was built for (a clamped term, alpha < 0, raw scales on both sides of 1e-2, a target energy about eps, ...);
  * every mutant of the restatement is rejected: a listed row figure misses its bar by >= 6 dB, or an exact-zero row is not zero, or a
    permutation differs;
  * the same mutants measured as tests/test_train_gpu.py::test_criteria_backward measures (its inputs, uniform upstream gradient, whole
    tensors, 80 / 60 dB) stand beside the new figures in profiles/criterion_hard_mutants.json (rewritten with SEPR_WRITE_PROFILES=1,
    checked against this run otherwise).
"""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criterion_ref as cr                                                   # noqa: E402
from oracle.sepreformer_oracle import agreement_db                           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "criterion_hard_mutants.json")
REQUIRED_MUTANTS = {"time_no_clamp", "time_gl0", "time_no_sign", "time_no_et_term", "time_no_mean", "mag_scale_gate_open", "mag_no_scale_path",
                    "mag_no_demean", "mag_pad_minus_mean", "mag_ola_drops_last_frame", "mag_no_sqrt_floor", "mag_identity_perm", "mag_gl0"}
# what the inputs of test_criteria_backward cannot show (this run's measurement must say the same)
OLD_BARS_LET_THROUGH = {"time_no_et_term", "time_gl0", "mag_scale_gate_open", "mag_gl0"}


def test_case_list_is_whole():
    tags = {c.tag for c in cr.CASES}
    assert len(tags) == len(cr.CASES) == 2 * 12 + 13 * 3 + 1
    for T in (400, 4097):
        assert {c.family for c in cr.CASES if (c.S, c.B, c.T) == (2, 3, T)} == set(cr.FAMILIES)
    for S in (1, 2, 3):
        for T in (400, 512, 513, 4096, 4097):
            assert {"plain", "anti", "half_clamped"} <= {c.family for c in cr.CASES if (c.S, c.B, c.T) == (S, 3, T)}, (S, T)
    assert "S2_B65_T512.plain" in tags
    assert len(cr.FAMILIES) == 12 and set(cr.MUTANTS["time"]) | set(cr.MUTANTS["mag"]) >= REQUIRED_MUTANTS
    for c in cr.CASES:
        assert torch.equal(c.weights(), torch.linspace(0.5, 2.0, c.B))
        est, src = c.tensors()
        assert est.shape == src.shape == (c.S, c.B, c.T) and est.dtype == torch.float32
    # the frame geometry the shapes were chosen for: one frame after padding, exactly one, two, and a second moment chunk of one sample
    frames = lambda T: ((T + 127) // 128 * 128 - 512) // 128 + 1             # noqa: E731
    assert [frames(T) for T in cr.T_EDGES] == [1, 1, 2, 29, 30] and 4097 - cr.PIT_CHUNK == 1


def _case(tag):
    return next(c for c in cr.CASES if c.tag == tag)


@pytest.mark.parametrize("T", [400, 4097])
def test_families_do_what_they_were_built_for(T):
    """Each property is read from the float64 reference or the inputs, never from the restatement."""
    t = lambda f, k: cr.floors(_case(f"S2_B3_T{T}.{f}"), k)                   # noqa: E731
    # the swap makes the permutation (1, 0)
    assert t("plain", "time")["perm64"].tolist() == [[1, 0]] * 3 and t("plain", "mag")["perm64"].tolist() == [[1, 0]] * 3
    # clamped terms: exact zeros in the float64 gradient
    assert bool(t("close60", "time")["zero"].all()) and (t("close60", "time")["loss64"] == -60.0).all()
    assert t("half_clamped", "time")["zero"].tolist() == [[True] * 3, [False] * 3]
    assert not t("close60", "mag")["zero"].any() and not t("half_clamped", "mag")["zero"].any()
    # silent rows
    for f in ("silent_est", "silent_tgt"):
        z = t(f, "time")["zero"]
        assert int(z.sum()) == 1 and float(t(f, "time")["loss64"][0]) >= cr.EPS_DOMINATED_DB
    assert bool(t("silent_est", "time")["zero"][0, 0]) and bool(t("silent_tgt", "time")["zero"][1, 0])
    assert bool(t("silent_est", "mag")["zero"][0, 0])
    # alpha < 0 for estimate 0 against its target; the magnitude loss's scale clamp active there
    c = _case(f"S2_B3_T{T}.anti")
    raw = cr.raw_scale(c)
    for k in ("time", "mag"):
        p = cr.floors(c, k)["perm64"]
        assert all(float(raw[0, int(p[b, 0]), b]) < -0.5 for b in range(3)), k
    # raw scales on both sides of 1e-2, none near it
    c = _case(f"S2_B3_T{T}.scale_edge")
    raw, p = cr.raw_scale(c), cr.floors(c, "mag")["perm64"]
    v = [float(raw[0, int(p[b, 0]), b]) for b in range(3)]
    assert min(v) < cr.SCALE_MIN < max(v) and all(abs(x - cr.SCALE_MIN) > cr.SCALE_EDGE_MARGIN for x in v), v
    # two equal estimates: the identity wins the tie
    c = _case(f"S2_B3_T{T}.tie")
    assert torch.equal(c.tensors()[0][0], c.tensors()[0][1])
    assert t("tie", "time")["perm64"].tolist() == [[0, 1]] * 3 and t("tie", "mag")["perm64"].tolist() == [[0, 1]] * 3
    # |t~|^2 of target 0 within a decade of the time loss's eps
    _, src = _case(f"S2_B3_T{T}.target_near_eps").tensors()
    tt = (src[0].double() - src[0].double().mean(-1, keepdim=True)).pow(2).sum(-1)
    assert ((tt > 0.1 * cr.EPS["time"]) & (tt < 20.0 * cr.EPS["time"])).all(), tt


@pytest.mark.parametrize("case", cr.CASES, ids=repr)
def test_reference_is_finite_and_the_restatement_meets_its_bars(case):
    for kind in cr.KINDS:
        r = cr.floors(case, kind)
        assert r["finite"], (case, kind)
        assert torch.equal(r["perm32"], r["perm64"]), (case, kind)
        live = ~r["zero"]
        if bool(live.any()):
            assert torch.isfinite(r["floor_db"][live]).all() and torch.isfinite(r["floor_dev_db"][live]).all(), (case, kind)
            if case.family != "dc100":
                assert float(r["bar"][live].min()) >= cr.FLOOR_OF_BARS_DB, (case, kind, r["bar"])
            assert float(r["bar"][live].max()) <= cr.MIN_DB
        loss, perm, grad = r["restated"]
        bad, _ = cr.judge(case, kind, loss, perm, grad)
        assert not bad, bad
        # float32 autograd passes the same rules: the bars ask nothing of the device that float32 arithmetic does not reach on the host
        bad32, _ = cr.judge(case, kind, r["loss32"], r["perm32"], r["g32"])
        assert not bad32, bad32


# ----------------------------------------------------------------------------------------------------------------------
# mutants
# ----------------------------------------------------------------------------------------------------------------------
def _survey(kind, name):
    """Every listed case under the mutant -> the row figures with their bars, the exact-zero rows it breaks, the permutations it changes."""
    rows, zeros, perms, nonfinite = [], [], [], []
    for case in cr.CASES:
        r = cr.floors(case, kind)
        _, perm, grad = cr.restated(case, kind, name)
        if not torch.equal(perm, r["perm64"]):
            perms.append(case.tag)
        for s in range(case.S):
            for b in range(case.B):
                where = f"{case.tag}.dest{s}.b{b}"
                if not torch.isfinite(grad[s, b]).all():
                    nonfinite.append(where)
                elif bool(r["zero"][s, b]):
                    if float(grad[s, b].abs().max()) != 0.0:
                        zeros.append(where)
                else:
                    rows.append({"figure": where, "family": case.family, "mutant_db": agreement_db(grad[s, b], r["g64"][s, b]),
                                 "bar_db": float(r["bar"][s, b])})
    return rows, zeros, perms, nonfinite


_results = {}


@pytest.mark.parametrize("name", cr.TIME_MUTANTS + cr.MAG_MUTANTS)
def test_mutant_is_rejected(name):
    kind = "time" if name in cr.TIME_MUTANTS else "mag"
    rows, zeros, perms, nonfinite = _survey(kind, name)
    best = max(rows, key=lambda r: r["bar_db"] - r["mutant_db"])
    spare = best["bar_db"] - best["mutant_db"]
    seen_by = sorted({r["family"] for r in rows if r["bar_db"] - r["mutant_db"] >= cr.MARGIN_DB})
    old = cr.old_way(kind, name)
    rd = lambda v: round(float(v), 1)                                       # noqa: E731
    _results[name] = {
        "new": {"figure": best["figure"], "mutant_db": rd(best["mutant_db"]), "bar_db": rd(best["bar_db"]), "spare_db": rd(spare)},
        "row_figures_that_reject_it": sum(1 for r in rows if r["bar_db"] - r["mutant_db"] >= cr.MARGIN_DB), "row_figures_tried": len(rows),
        "families_whose_figures_reject_it": seen_by,
        "exact_zero_rows_broken": len(zeros), "permutations_changed_in_cases": len(perms), "non_finite_rows": len(nonfinite),
        "rejected_by": [k for k, v in (("row_figure", spare >= cr.MARGIN_DB), ("exact_zero", zeros), ("permutation", perms)) if v],
        "rejected": bool(spare >= cr.MARGIN_DB or zeros or perms),
        "old": {k: (rd(v) if isinstance(v, float) else v) for k, v in old.items()},
    }
    print(name, json.dumps(_results[name]))
    assert spare >= cr.MARGIN_DB or zeros or perms, f"{name}: no listed figure, exact zero or permutation sees it (best {best})"


def test_unmutated_restatement_passes_the_old_bars():
    for kind in cr.KINDS:
        old = cr.old_way(kind, None)
        assert old["passes_old_bars"], (kind, old)


def test_mutant_record():
    """profiles/criterion_hard_mutants.json is this run's result (SEPR_WRITE_PROFILES=1 rewrites it): every mutant rejected, and it says
    which of them the inputs and bars of test_criteria_backward let through."""
    names = cr.TIME_MUTANTS + cr.MAG_MUTANTS
    for n in names:
        if n not in _results:                                               # run on its own: measure here
            test_mutant_is_rejected(n)
    if os.environ.get("SEPR_WRITE_PROFILES") == "1":
        doc = {"what": "the device's criterion algorithm restated in torch (tests/criterion_ref.py) with one planted defect, against float64 autograd "
                       "over the oracle: 'new' = the listed gradient row d est[s, b] that sees it best against that row's bar "
                       "min(80, float32 floor - 6, restated floor - 6), with the exact-zero rows it breaks and the cases whose permutation it changes; "
                       "'old' = the same mutant on the inputs of tests/test_train_gpu.py::test_criteria_backward, uniform upstream gradient, mean loss "
                       "(100 / 90 dB) and every d est_s as one tensor (80 dB time, 60 dB mag): the figure closest to (or furthest under) its bar",
               "passed_by_the_old_bars": sorted(n for n in names if _results[n]["old"]["passes_old_bars"]),
               "mutants": _results}
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(PROFILE) as f:
        doc = json.load(f)
    rec = doc["mutants"]
    assert set(rec) == set(names) >= REQUIRED_MUTANTS
    for n in names:
        assert rec[n]["rejected"] and _results[n]["rejected"], n
        for k in ("exact_zero_rows_broken", "permutations_changed_in_cases"):
            assert rec[n][k] == _results[n][k], (n, k)
        assert abs(rec[n]["new"]["spare_db"] - _results[n]["new"]["spare_db"]) <= 1.0, n
        assert abs(rec[n]["old"]["lowest_agreement_db"] - _results[n]["old"]["lowest_agreement_db"]) <= 1.0, n
        assert rec[n]["old"]["passes_old_bars"] == _results[n]["old"]["passes_old_bars"], n
    assert doc["passed_by_the_old_bars"] == sorted(n for n in names if rec[n]["old"]["passes_old_bars"])
    assert OLD_BARS_LET_THROUGH <= set(doc["passed_by_the_old_bars"])
