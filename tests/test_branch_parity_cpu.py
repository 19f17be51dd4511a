"""The branch-parity bar has teeth: proof from the reference side only (no device).  See tests/branch_ref.py for the measure, the bar
and the shared case list; tests/test_branch_parity_gpu.py runs the same cases on the device.

  * every (case, family) of the shared list: the float64 oracle is finite, ``floor_db`` (float32 oracle vs float64) and ``floor_x3_db``
    (bf16 hi+lo products) are finite - zeros, constant rows and silence included;
  * every mutant (the oracle with one planted defect) misses the fp32 bar of at least one listed (case, family) by >= 6 dB, i.e. the
    device test would fail if a kernel had that defect;
  * the same mutants measured the way the block tests did until now (``agreement_db`` on ``y``, randn, float32 oracle) stand next to
    the new figures in profiles/branch_parity_mutants.json (rewritten with SEPR_WRITE_PROFILES=1, checked against this run otherwise).

Base width is used only where it is the point (pooled length above maxlen = 2000, and the old-way figures at the shapes of the existing
tests); everything else runs at tiny width (maxlen 40), where the same code paths of the oracle are exercised in milliseconds.
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
PROFILE = os.path.join(ROOT, "profiles", "branch_parity_mutants.json")


def test_family_lists_are_whole():
    """The issue's nine row families plus constant / one-hot rows, five waveform families plus plain speech; at most one family in ten
    may be removed (with its reason, in branch_ref.REMOVED_FAMILIES) because float64 cannot evaluate it - none was."""
    assert set(br.ROW_FAMILIES) | set(br.REMOVED_FAMILIES) >= {"randn", "plus10", "plus100", "loud", "quiet", "zeros", "silent_rows", "outlier",
                                                              "row_range", "constant_rows", "one_hot_rows"}
    assert set(br.WAVE_FAMILIES) | set(br.REMOVED_FAMILIES) >= {"silent_utt", "silent_half", "dc", "clipped", "level_1e-5"}
    total = len(br.ROW_FAMILIES) + len(br.WAVE_FAMILIES) + len(br.REMOVED_FAMILIES)
    assert len(br.REMOVED_FAMILIES) * 10 <= total
    assert set(br.WORST_FLOORS) <= set(br.ROW_FAMILIES)
    fam = br.input_families((2, 30, 16), 3)
    assert list(fam) == br.ROW_FAMILIES and all(torch.equal(fam[k], br.input_families((2, 30, 16), 3)[k]) for k in fam)
    assert float(fam["constant_rows"][:, ::7].var(-1, unbiased=False).max()) == 0.0
    assert int((fam["one_hot_rows"] != 0).sum(-1).max()) == 1
    wav = br.wave_families(3, 800, 3)
    assert list(wav) == br.WAVE_FAMILIES and float(wav["silent_utt"][1].abs().max()) == 0.0 and float(wav["clipped"].abs().max()) == 1.0
    # the shapes the device file must run are in the shared list
    tags = {c.tag for c in br.ALL_CASES}
    assert {"gcfn.n2_T37", "gcfn.n3_T300", "cla.n2_T24", "cla.n2_T150", "cla.n1_T500", "down.n2_T40", "down.n2_T41", "down.n2_T6",
            "ega.n1_fac1_Tp2100", "ega.n1_fac2_Tp2050"} <= tags
    assert {c.shape["fac"] for c in br.BLOCK_CASES if c.kind == "ega"} == {1, 2, 4, 8, 16}


def test_attention_restatement_is_the_oracle():
    """The attention the two attention mutants are built on, with both defects off, is oracle.mha bit for bit."""
    sd, cfg = br.state("tiny"), VARIANTS["tiny"]
    x = br.input_families((2, 50, cfg.feat), 1)["randn"]
    p = br.E0 + ".g_block_1.block.ega.block.self_attn"
    pos = orc.rel_pos_k(sd, 50, cfg.maxlen)
    assert torch.equal(br._mha_variant()(sd, p, x, pos, cfg.heads), orc.mha(sd, p, x, pos, cfg.heads))
    assert torch.equal(br.oracle64(orc.gcfn, sd, br.E0 + ".g_block_1.block.gcfn", x),
                       orc.gcfn(br.sd64(sd), br.E0 + ".g_block_1.block.gcfn", x.double()))


@pytest.mark.parametrize("case", br.cases_for("tiny"), ids=repr)
def test_floors_are_finite(case):
    for fam in case.families:
        r = br.floors(case, "tiny", fam)
        assert r["finite"], (case, fam)
        assert math.isfinite(r["floor_db"]) and math.isfinite(r["floor_x3_db"]), (case, fam, r["floor_db"], r["floor_x3_db"])
        assert r["floor_db"] > 40.0 and r["floor_x3_db"] > 40.0, (case, fam, r["floor_db"], r["floor_x3_db"])   # a float32 oracle this far off is a broken case


# the way the block tests measured until now, at the shapes of the existing tests (Base width, randn): where each mutant's old figure is taken
OLD_WAY = {"clamp_neg_off_by_one": (br.BASE, "ega.n1_fac2_Tp2050"), "clamp_both_off_by_one": (br.BASE, "ega.n1_fac1_Tp2100"),
           "ragged_last_key_masked": (br.BASE, "ega.n2_fac4_Tp130"), "dwconv_halo_tap_lost": (br.BASE, "gcfn.n3_T300")}


def _mutant_out(m, case, variant, inp, dtype):
    with m["ctx"]():
        return br.reference(case, variant, br.state(variant, dtype), inp)


def _survey(name, m):
    """Every listed (variant, case, family) the mutant can touch -> its branch agreement with the clean float64 oracle and the bars."""
    rows = []
    by_tag = {c.tag: c for c in br.ALL_CASES}
    todo = [("tiny", c) for c in br.cases_for("tiny") if c.kind in m["kinds"]]
    if name in OLD_WAY:
        todo.append((OLD_WAY[name][0], by_tag[OLD_WAY[name][1]]))          # Base width: one shape per mutant of the issue's table, randn only
    for variant, case in todo:
        for fam in (["randn"] if variant == br.BASE else case.families):
            r = br.floors(case, variant, fam, want_x3=(variant != br.BASE))
            ym, xm = _mutant_out(m, case, variant, r["inp"], torch.float64)
            db = br.branch_db(ym, xm, r["y64"], r["x64"])
            x3 = r["floor_x3_db"]
            rows.append({"variant": variant, "case": case.tag, "family": fam, "mutant_branch_db": db, "bar_fp32_db": br.bar(r["floor_db"]),
                         "bar_bf16x3_db": None if x3 is None else br.bar(r["floor_db"], x3)})
    return rows


def _old_way(name, m, best):
    by_tag = {c.tag: c for c in br.ALL_CASES}
    variant, tag = OLD_WAY.get(name, (best["variant"], best["case"]))
    case = by_tag[tag]
    fam = "randn" if "randn" in case.families else case.families[0]
    inp = br.make_inputs(case, VARIANTS[variant], fam)
    y, _ = br.reference(case, variant, br.state(variant), inp)
    ym, _ = _mutant_out(m, case, variant, inp, torch.float32)
    return {"variant": variant, "case": tag, "family": fam, "agreement_on_y_db": orc.agreement_db(ym, y)}


_results = {}


@pytest.mark.parametrize("name", list(br.mutants()))
def test_mutant_is_rejected(name):
    m = br.mutants()[name]
    rows = _survey(name, m)
    assert rows, name
    best = max(rows, key=lambda r: r["bar_fp32_db"] - r["mutant_branch_db"])
    spare = best["bar_fp32_db"] - best["mutant_branch_db"]
    x3rows = [r for r in rows if r["bar_bf16x3_db"] is not None]
    best3 = max(x3rows, key=lambda r: r["bar_bf16x3_db"] - r["mutant_branch_db"])
    old = _old_way(name, m, best)
    same = [r for r in rows if (r["variant"], r["case"], r["family"]) == (old["variant"], old["case"], old["family"])][0]
    rd = lambda v: round(float(v), 1)                                       # noqa: E731
    _results[name] = {
        "new": {"variant": best["variant"], "case": best["case"], "family": best["family"], "mutant_branch_db": rd(best["mutant_branch_db"]),
                "bar_fp32_db": rd(best["bar_fp32_db"]), "spare_db": rd(spare)},
        "new_bf16x3": {"variant": best3["variant"], "case": best3["case"], "family": best3["family"], "mutant_branch_db": rd(best3["mutant_branch_db"]),
                       "bar_bf16x3_db": rd(best3["bar_bf16x3_db"]), "spare_db": rd(best3["bar_bf16x3_db"] - best3["mutant_branch_db"])},
        "cases_that_reject_it": sum(1 for r in rows if r["bar_fp32_db"] - r["mutant_branch_db"] >= br.MARGIN_DB), "cases_tried": len(rows),
        "old": dict(old, agreement_on_y_db=rd(old["agreement_on_y_db"]), passes_old_80_db_bar=bool(old["agreement_on_y_db"] >= br.MIN_DB),
                    branch_db_at_this_case=rd(same["mutant_branch_db"]), bar_fp32_db_at_this_case=rd(same["bar_fp32_db"])),
    }
    print(name, json.dumps(_results[name]))
    assert spare >= br.MARGIN_DB, f"{name}: no listed case sees it with 6 dB to spare (best {best})"
    assert best3["bar_bf16x3_db"] - best3["mutant_branch_db"] >= br.MARGIN_DB, f"{name}: invisible under the bf16x3 bar (best {best3})"


def test_mutant_record():
    """profiles/branch_parity_mutants.json is this run's result (SEPR_WRITE_PROFILES=1 rewrites it): every mutant rejected with >= 6 dB to
    spare, and the one-sided clamp at T' = 2050 among those the old measurement let through."""
    names = list(br.mutants())
    for n in names:
        if n not in _results:                                               # run on its own: measure here
            test_mutant_is_rejected(n)
    if os.environ.get("SEPR_WRITE_PROFILES") == "1":
        doc = {"what": "oracle with one planted defect against the clean oracle: 'new' = branch agreement in float64 on the listed case that "
                       "sees it best, against that case's bar min(80, floor - 6); 'old' = agreement on y, randn, float32 oracle, at the shape "
                       "the block tests used (tests/test_branch_parity_cpu.py)",
               "mutants": _results}
        with open(PROFILE, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(PROFILE) as f:
        rec = json.load(f)["mutants"]
    assert set(rec) == set(names)
    for n in names:
        assert rec[n]["new"]["spare_db"] >= br.MARGIN_DB, n
        assert abs(rec[n]["new"]["spare_db"] - _results[n]["new"]["spare_db"]) <= 1.0, n
        assert abs(rec[n]["old"]["agreement_on_y_db"] - _results[n]["old"]["agreement_on_y_db"]) <= 1.0, n
    assert rec["clamp_neg_off_by_one"]["old"]["case"] == "ega.n1_fac2_Tp2050" and rec["clamp_neg_off_by_one"]["old"]["passes_old_80_db_bar"]
