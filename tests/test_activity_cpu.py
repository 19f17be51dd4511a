"""Frame activity and the colouring-based assignment without a device: the restatement's own error bound, ``colour``
against enumeration, ``frame_classes`` against a per-sample brute force, and what the entries refuse before any HIP call."""
import math
import os
import random
import re

import numpy as np
import pytest

import activity_ref as ref
from sepreformer_amd import conversation as cv
from sepreformer_amd import lib as L
from test_conversation_cpu import host_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("frame,T", [(32, 31), (160, 1000), (256, 4100), (4096, 8191)])
def test_frame_energy_restatement_is_within_its_bound(frame, T):
    """``frame`` additions of non-negative exact terms: every partial sum is at most the true sum times (1 + 2^-53)^k, so the result lies
    within ``frame * 2^-52`` relative of the exact sum (``math.fsum`` of the exact squares, correctly rounded)."""
    rng = np.random.default_rng(frame + T)
    x = (rng.normal(size=(3, T)) * 10.0 ** rng.uniform(-20, 3, size=(3, T))).astype(np.float32)
    got = ref.frame_energy_ref(x, frame)
    nF = -(-T // frame)
    assert got.shape == (3, nF)
    for r in range(3):
        for f in range(nF):
            want = math.fsum((x[r, f * frame:(f + 1) * frame].astype(np.float64) ** 2).tolist())
            assert abs(got[r, f] - want) <= frame * 2.0 ** -52 * want, (r, f, got[r, f], want)


def _check_colour(v, begin, length, C):
    want, best, second = ref.colour_brute(v, begin, length, C)
    got = cv.colour(v, begin, length, C)
    if want is None:
        assert got is None
        return None
    assert best - second > 1e-9 * max(1.0, abs(best)), (best, second)      # the restatement's own gap: the maximiser is beyond doubt
    assert np.array_equal(got, want), (got, want)
    return got


@pytest.mark.parametrize("C", [2, 3])
def test_colour_equals_enumeration_on_planned_conversations(C):
    corpus = host_corpus()
    seen = 0
    for seed in range(12):
        conv = cv.plan_conversation(corpus, random.Random(seed), seconds=14.0, speakers=3, max_active=2, overlap=(0.2, 0.8), p_overlap=0.7)
        G = min(9, len(conv.utt))
        by_time = np.argsort(conv.place, kind="stable")[:G]                # a table that is NOT in time order: sorted by (track, place)
        by_time = np.sort(by_time)
        begin, length = conv.place[by_time], conv.len[by_time]
        v = np.random.default_rng(seed).normal(size=(G, C)) * 10.0
        seen += _check_colour(v, begin, length, C) is not None
    assert seen >= 6


def test_colour_on_hand_made_sets():
    v = np.array([[3.0, 1.0], [2.0, 5.0], [4.0, 0.5]])
    # a chain 0 - 1 - 2: two colourings, (0, 1, 0) = 12 and (1, 0, 1) = 3.5
    assert _check_colour(v, [0, 5, 12], [8, 10, 6], 2).tolist() == [0, 1, 0]
    # segments that only abut are not adjacent: each takes its best channel
    assert _check_colour(v, [0, 8, 18], [8, 10, 6], 2).tolist() == [0, 1, 0]
    assert cv.colour(np.array([[1.0, 9.0], [1.0, 9.0]]), [0, 8], [8, 4], 2).tolist() == [1, 1]
    # G = 1
    assert _check_colour(np.array([[1.0, 2.0, 0.0]]), [7], [3], 3).tolist() == [1]
    # a clique of C + 1 segments: no colouring
    for C in (2, 3):
        G = C + 1
        assert cv.colour(np.ones((G, C)), list(range(G)), [10] * G, C) is None
        assert ref.colour_brute(np.ones((G, C)), list(range(G)), [10] * G, C)[0] is None
    # ... also behind a valid beginning
    assert cv.colour(np.ones((4, 2)), [0, 20, 21, 22], [5, 9, 9, 9], 2) is None
    # the exact tie of two identical columns: the lexicographically first colouring wins, in (begin, index) order - not in table order
    tie = np.array([[2.0, 2.0], [1.0, 1.0], [3.0, 3.0]])
    got = cv.colour(tie, [10, 0, 12], [5, 11, 6], 2)                       # time order: 1, 0, 2; 1 - 0 and 0 - 2 adjacent
    want, best, second = ref.colour_brute(tie, [10, 0, 12], [5, 11, 6], 2)
    assert best == 6.0 and got.tolist() == want.tolist() == [1, 0, 0]
    # equal begins are ordered by table index
    assert _check_colour(np.array([[0.0, 1.0], [0.0, 3.0]]), [4, 4], [2, 2], 2).tolist() == [0, 1]
    # a table in another order than time, three channels, two talkers overlapping a third
    v3 = np.array([[1.0, 7.0, 2.0], [6.0, 6.5, 0.0], [0.0, 8.0, 1.0], [5.0, 4.0, 3.0]])
    _check_colour(v3, [30, 0, 10, 25], [10, 28, 18, 12], 3)


def test_colour_handles_a_long_conversation_without_enumeration():
    corpus = host_corpus()
    conv = cv.plan_conversation(corpus, random.Random(5), seconds=600.0, speakers=3, max_active=2)
    G = len(conv.utt)
    assert G > 150
    v = np.random.default_rng(0).normal(size=(G, 2))
    a = cv.colour(v, conv.place, conv.len, 2)
    b, e = conv.place.astype(np.int64), conv.place.astype(np.int64) + conv.len
    assert a is not None and set(a.tolist()) <= {0, 1}
    for g in range(G):
        for h in range(g + 1, G):
            if max(b[g], b[h]) < min(e[g], e[h]):
                assert a[g] != a[h]


@pytest.mark.parametrize("collar", [0, 1, 7, 1000])
def test_frame_classes_equal_the_per_sample_brute_force(collar):
    n, frame, C = 203, 8, 2                                               # 26 frames, the last of 3 samples
    # spans that start / end on a frame boundary, one sample either side of one, at the ends of the recording, and abutting
    begin = np.array([0, 16, 41, 63, 88, 120, 160, 199])
    length = np.array([8, 9, 7, 10, 8, 17, 25, 4])
    coloured = np.array([0, 1, 0, 1, -1, 0, 1, 0])
    got = cv.frame_classes((begin, length), coloured, n, C, frame, collar)
    assert got.dtype == np.uint8 and got.shape == (C, 26)
    assert np.array_equal(got, ref.frame_classes_brute(begin, length, coloured, n, C, frame, collar))
    if collar == 0:
        assert not (got == 3).any()                                      # a collar of 0 widens nothing
        assert got[0, 0] == 0 and got[1, 0] == 1 and got[0, 1] == 2 and got[1, 2] == 0 and got[1, 3] == 0 and got[1, 4] == 2
    if collar == 1000:
        assert not (got == 2).any()                                      # the collar reaches past 0 and past n: nothing is quiet


def test_frame_classes_hand_case():
    # one span of channel 0 on [8, 16) of 40 samples, frames of 8, a collar of 3: frame 1 own, frames 0 and 2 collar, the rest quiet; for channel 1
    # the widened span is cross
    got = cv.frame_classes(([8], [8]), [0], 40, 2, 8, 3)
    assert got.tolist() == [[3, 0, 3, 2, 2], [1, 1, 1, 2, 2]]
    got = cv.frame_classes(([9], [6]), [1], 40, 2, 8, 0)
    assert got.tolist() == [[2, 1, 2, 2, 2], [2, 0, 2, 2, 2]]


def test_idle_figures():
    s = np.zeros((2, 4, 4))
    s[0, 0] = [10, 8, 5.0, 5.0]
    s[0, 1] = [4, 1, 1e-4, 1.0]
    s[0, 2] = [6, 2, 0.5, 0.0]
    out = cv.idle_figures(s)
    assert abs(out["leak_db"][0] + 40.0) < 1e-9 and np.isnan(out["quiet_db"][0]) and out["false_alarm"][0] == 0.3 and abs(out["miss"][0] - 0.2) < 1e-15
    assert all(np.isnan(out[k][1]) for k in out)


def test_score_without_spans_is_unchanged_and_with_spans_adds_the_colouring():
    rng = np.random.default_rng(1)
    G, C = 7, 2
    v, v_mix = rng.normal(size=(G, C)) * 5, rng.normal(size=G)
    conv_of, track = np.array([0, 0, 0, 0, 1, 1, 1]), np.array([0, 1, 2, 0, 0, 1, 0])
    S_of, ov = [3, 2], rng.uniform(0, 1, size=G)
    plain = cv.score(v, v_mix, conv_of, track, S_of, C, overlap=ov)
    assert sorted(plain) == sorted(["best", "assigned", "utt", "cons", "switch", "assignment", "sisnri_utt", "sisnri_cons", "switch_rate", "n", "overlap",
                                    "bins"])
    assert all(sorted(b) == ["n", "sisnri_cons", "sisnri_utt"] for b in plain["bins"].values())
    assert sorted(cv.score(v, v_mix, conv_of, track, S_of, C)) == sorted(k for k in plain if k not in ("overlap", "bins"))
    begin, length = np.array([0, 5, 12, 30, 0, 6, 20]), np.array([8, 10, 6, 5, 8, 10, 4])
    full = cv.score(v, v_mix, conv_of, track, S_of, C, overlap=ov, spans=(begin, length))
    for k in plain:
        if k != "bins":
            np.testing.assert_equal(full[k], plain[k])
    assert sorted(set(full) - set(plain)) == ["coloured", "graph", "graph_switch_rate", "sisnri_graph"]
    assert np.isnan(plain["cons"][:4]).all() and (full["coloured"] >= 0).all()          # S = 3 > C = 2: no cons, but a colouring
    for r in (0, 1):
        idx = conv_of == r
        assert np.array_equal(full["coloured"][idx], ref.colour_brute(v[idx], begin[idx], length[idx], C)[0])
    g = np.arange(G)
    assert np.array_equal(full["graph"], v[g, full["coloured"]] - v_mix)
    assert full["sisnri_graph"] == float(full["graph"].mean()) and full["graph_switch_rate"] == float((full["best"] != full["coloured"]).mean())
    assert all("sisnri_graph" in b for b in full["bins"].values())
    # a conversation without a colouring: -1 and NaN, left out of the means
    none = cv.score(v, v_mix, conv_of, track, S_of, C, spans=(np.array([0, 1, 2, 30, 0, 6, 20]), np.array([9, 9, 9, 5, 8, 10, 4])))
    assert (none["coloured"][:4] == -1).all() and np.isnan(none["graph"][:4]).all() and np.isfinite(none["sisnri_graph"])


def test_entries_are_declared_bound_and_refuse_before_any_device_call():
    hdr = open(os.path.join(ROOT, "include", "sepr.h")).read()
    names = ("sepr_frame_energy_fwd", "sepr_frame_activity_bytes", "sepr_frame_activity_fwd", "sepr_frame_class_sums_bytes", "sepr_frame_class_sums_fwd")
    for name in names:
        assert re.search(r"^(int|long long) " + name + r"\(", hdr, re.M) and name in L.SIGNATURES
    for name in names[1::2]:
        assert re.search(r"^long long " + name + r"\(", hdr, re.M) and L.SIGNATURES[name][0] is L._ll
    assert int(re.search(r"#define SEPR_VERSION (\d+)", hdr).group(1)) == 413 == L.ABI_VERSION
    mk = open(os.path.join(ROOT, "sepreformer_amd", "csrc", "Makefile")).read()
    assert "sepr_activity.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)
    lib = L.load()
    p = 0x10000                                                   # a well-aligned address that is never dereferenced: every call below is refused
    nan, inf = float("nan"), float("inf")

    egood = dict(x=p, rows=3, T=1000, ld=1000, frame=160, e=p)

    def energy(**kw):
        a = {**egood, **kw}
        return lib.sepr_frame_energy_fwd(a["x"], a["rows"], a["T"], a["ld"], a["frame"], a["e"], None)

    for kw in [dict(x=None), dict(e=None), dict(rows=0), dict(rows=65536), dict(T=0), dict(T=(1 << 36) + 1, ld=1 << 37), dict(ld=999), dict(frame=28),
               dict(frame=0), dict(frame=4100), dict(frame=162), dict(frame=-160), dict(x=p + 2), dict(e=p + 4)]:
        assert energy(**kw) == L.SEPR_EINVAL, kw

    agood = dict(e=p, rows=2, nF=50, ratio=1e-4, floor=1e-12, hang=10, active=p, level=p, ws=p, ws_bytes=1 << 20)

    def activity(**kw):
        a = {**agood, **kw}
        return lib.sepr_frame_activity_fwd(a["e"], a["rows"], a["nF"], a["ratio"], a["floor"], a["hang"], a["active"], a["level"], a["ws"],
                                           a["ws_bytes"], None)

    for kw in [dict(e=None), dict(active=None), dict(level=None), dict(rows=0), dict(rows=65536), dict(nF=0), dict(nF=(1 << 30) + 1), dict(hang=-1),
               dict(ratio=-1.0), dict(ratio=nan), dict(ratio=inf), dict(floor=-1.0), dict(floor=nan), dict(floor=inf), dict(e=p + 4),
               dict(level=p + 4)]:
        assert activity(**kw) == L.SEPR_EINVAL, kw
    need = lib.sepr_frame_activity_bytes(2, 50)
    assert need >= 2 * 51 * 4 and need % 256 == 0 and lib.sepr_frame_activity_bytes(8, 1 << 30) >= 8 * 4 * (1 << 30)
    assert [lib.sepr_frame_activity_bytes(*a) for a in ((0, 50), (65536, 50), (2, 0), (2, (1 << 30) + 1))] == [0, 0, 0, 0]
    assert activity(ws_bytes=need - 1) == L.SEPR_EWORKSPACE and activity(ws=None) == L.SEPR_EWORKSPACE

    cgood = dict(e_est=p, e_mix=p, active=p, cls=p, C=2, nF=50, out=p, ws=p, ws_bytes=1 << 20)

    def sums(**kw):
        a = {**cgood, **kw}
        return lib.sepr_frame_class_sums_fwd(a["e_est"], a["e_mix"], a["active"], a["cls"], a["C"], a["nF"], a["out"], a["ws"], a["ws_bytes"], None)

    for kw in [dict(e_est=None), dict(e_mix=None), dict(active=None), dict(cls=None), dict(out=None), dict(C=0), dict(C=9), dict(nF=0),
               dict(nF=(1 << 30) + 1), dict(e_est=p + 4), dict(e_mix=p + 4), dict(out=p + 4)]:
        assert sums(**kw) == L.SEPR_EINVAL, kw
    need = lib.sepr_frame_class_sums_bytes(2, 50)
    assert need >= 2 * 4 * 4 * 4 * 8 and need % 256 == 0
    assert [lib.sepr_frame_class_sums_bytes(*a) for a in ((0, 50), (9, 50), (2, 0), (2, (1 << 30) + 1))] == [0, 0, 0, 0]
    assert sums(ws_bytes=need - 1) == L.SEPR_EWORKSPACE and sums(ws=None) == L.SEPR_EWORKSPACE


def test_host_wrappers_have_no_cpu_path():
    import torch
    from sepreformer_amd import activity as act
    assert act.frame_samples(8000, 20) == 160 and act.frame_samples(16000, 20) == 320 and act.frame_samples(8000, 20.1) == 160
    assert act.frame_samples(8000, 20.3) == 164 and act.hang_frames(20, 200) == 10 and act.hang_frames(20, 0) == 0
    with pytest.raises(ValueError):
        act.frame_samples(8000, 1)
    with pytest.raises(ValueError, match="HIP device"):
        act.frame_energy(torch.zeros(2, 400), 160)
    with pytest.raises(ValueError, match="HIP device"):
        act.activity_of(torch.zeros(2, 4, dtype=torch.float64))
    mask = np.array([[0, 1, 1, 0, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], dtype=np.uint8)
    assert act.segments(mask, 160, 790) == [[(160, 480), (640, 790)], [], [(0, 790)]]
    assert "not measured optima" in act.channel_activity.__doc__


def test_activity_csv(tmp_path):
    import csv
    from sepreformer_amd import activity as act
    path = str(tmp_path / "a.csv")
    act.write_activity_csv(path, [[(160, 480), (640, 790)], [], [(0, 790)]], 8000)
    rows = list(csv.reader(open(path), quotechar="|"))
    assert rows == [["0", "0.02", "0.06"], ["0", "0.08", "0.09875"], ["2", "0.0", "0.09875"]]
