"""Frame activity on the device: the three entries bit for bit against the numpy restatement (tests/activity_ref.py),
a planted leak through the scoring loop, and the loop and the command line end to end on the smallest model."""
import csv
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import activity_ref as ref                                                   # noqa: E402
from test_conversation_gpu import synthetic_corpus                           # noqa: E402

from sepreformer_amd import activity as act                                  # noqa: E402
from sepreformer_amd import conversation as cv                               # noqa: E402
from sepreformer_amd import infer, longform                                  # noqa: E402
from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd.config import VARIANTS                                  # noqa: E402
from sepreformer_amd.model import Model                                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits64(t):
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).cpu().contiguous().view(torch.int64)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ---- frame energy -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [32, 160, 256, 4096])
def test_frame_energy_is_the_restatement_bit_for_bit(frame):
    """Rows that are views of a wider buffer, NaN behind ``T``, before the first sample and in guard rows above and below: on a 16-byte aligned
    layout (one load per four samples) and on an odd one (element by element).  Magnitudes from 1e-20 to 1e3."""
    rng = np.random.default_rng(frame)
    for T in (1, 31, 160, 4100, 8191):
        for rows in (1, 3, 9):
            x = (rng.normal(size=(rows, T)) * 10.0 ** rng.uniform(-20, 3, size=(rows, T))).astype(np.float32)
            x[0, :min(T, 3)] = [1e3, -1e-20, 0.0][:min(T, 3)]
            want = ref.frame_energy_ref(x, frame)
            for ld, off in ((T + 12 - T % 4, 4), (T + 7 + T % 2, 3)):        # ld a multiple of 4 with an aligned start; an odd ld, an odd start
                buf = torch.full((rows + 2, ld), float("nan"), device=DEV)
                view = buf[1:rows + 1, off:off + T]
                view.copy_(torch.from_numpy(x))
                got = act.frame_energy(view, frame)
                assert got.dtype == torch.float64 and got.shape == want.shape and got.device.type == "cuda"
                assert torch.equal(bits64(got), bits64(want)), (T, rows, ld, off)
                if rows > 1:
                    assert view.data_ptr() == buf.data_ptr() + 4 * (ld + off) and not view.is_contiguous()      # read in place, not repacked
            assert torch.equal(bits64(act.frame_energy(torch.from_numpy(x).to(DEV), frame)), bits64(want))      # contiguous rows, again


def test_frame_energy_of_recordings_on_frame_boundaries():
    """Zeros behind a recording change no bit: two recordings laid out on frame boundaries in one buffer give the frames each gives alone -
    what ``score_conversations`` relies on."""
    rng = np.random.default_rng(1)
    a, b = rng.normal(size=(2, 1000)).astype(np.float32), rng.normal(size=(2, 333)).astype(np.float32)
    pad = torch.zeros(2, 7 * 160 + 3 * 160, device=DEV)
    pad[:, :1000] = torch.from_numpy(a).to(DEV)
    pad[:, 1120:1120 + 333] = torch.from_numpy(b).to(DEV)
    got = act.frame_energy(pad, 160)
    assert torch.equal(bits64(got[:, :7]), bits64(ref.frame_energy_ref(a, 160))) and torch.equal(bits64(got[:, 7:]), bits64(ref.frame_energy_ref(b, 160)))


# ---- frame activity ---------------------------------------------------------------------------------------------------------------------
def activity_rows(nF, rng, ratio):
    """Energies of magnitudes well off the threshold, and the rows the header names: all zero, one loud frame at either end, a frame planted exactly
    at the threshold, a NaN frame."""
    pick = lambda: rng.choice([1.0, 3e-2, 1e-6, 0.0], size=nF) * rng.uniform(0.5, 0.9, size=nF)
    rows, planted = [pick(), np.zeros(nF)], []
    lo = np.full(nF, 1e-9)
    lo[0] = 2.0
    rows.append(lo)
    hi = np.full(nF, 1e-9)
    hi[-1] = 2.0
    rows.append(hi)
    if nF > 2:
        p = pick()
        p[nF // 2] = 0.95                                           # the level
        p[1] = p[nF // 2] * ratio                                   # exactly the threshold: not active
        rows.append(p)
        planted.append((len(rows) - 1, 1))
        q = pick()
        q[nF // 3], q[0] = np.nan, 0.93
        rows.append(q)
        rows.append(np.full(nF, np.nan))                            # every frame NaN: level -inf, the floor decides, nothing active
    neg = -pick()                                                   # energies are not negative, but a table is not trusted: the maximum of
    neg[0] = -0.0                                                   # negative values and -0.0 is +0.0, whatever the order
    rows.append(neg)
    return np.stack(rows), planted


@pytest.mark.parametrize("nF", [1, 5, 300])
def test_frame_activity_equals_the_restatement_in_every_byte(nF):
    rng = np.random.default_rng(nF)
    ratio_db = -40.0
    ratio = 10.0 ** (ratio_db / 10.0)
    e, planted = activity_rows(nF, rng, ratio)
    ed = torch.from_numpy(e).to(DEV)
    for hang in sorted({0, 1, max(0, nF - 1), nF + 5}):
        want, level, thr = ref.activity_ref(e, ratio, 1e-12, hang, planted=planted)
        active, lv = act.activity_of(ed, ratio_db=ratio_db, floor=1e-12, hang=hang)
        assert active.dtype == torch.uint8 and active.shape == e.shape
        assert np.array_equal(active.cpu().numpy(), want), (nF, hang)
        assert torch.equal(bits64(lv), bits64(level))
        for r, f in planted:
            assert e[r, f] == thr[r] and (hang > 0 or want[r, f] == 0)
    assert not want[1].any() and lv[1].item() == 0.0 and math.copysign(1.0, lv[-1].item()) == 1.0      # the all-zero row; a -0.0 maximum is +0.0
    if nF == 300:
        want0 = ref.activity_ref(e, ratio, 1e-12, 0, planted=planted)[0]
        assert want0[2].tolist() == [1] + [0] * 299 and want0[3].tolist() == [0] * 299 + [1] and not want0[6].any()
        want1 = ref.activity_ref(e, ratio, 1e-12, 1, planted=planted)[0]
        assert want1[2, :3].tolist() == [1, 1, 0] and want1[3, -3:].tolist() == [0, 1, 1]
        assert ref.activity_ref(e, ratio, 1e-12, 299, planted=planted)[0][2].all()


def guarded(nbytes):
    """A workspace of ``nbytes`` between two guards of 256 bytes of 0xA5."""
    buf = torch.full((nbytes + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + 256


def guards_intact(buf):
    return bool((buf[:256] == 0xA5).all()) and bool((buf[-256:] == 0xA5).all())


def test_frame_activity_workspace_lies_between_guards():
    rng = np.random.default_rng(9)
    e, planted = activity_rows(300, rng, 1e-4)
    rows, nF = e.shape
    lib = L.load()
    need = int(lib.sepr_frame_activity_bytes(rows, nF))
    buf, ws = guarded(need)
    ed = torch.from_numpy(e).to(DEV)
    out = torch.full((rows * nF + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    level = torch.empty(rows, dtype=torch.float64, device=DEV)
    assert lib.sepr_frame_activity_fwd(ed.data_ptr(), rows, nF, 1e-4, 1e-12, 3, out.data_ptr() + 256, level.data_ptr(), ws, need, stream()) == L.SEPR_OK
    torch.cuda.synchronize()
    assert guards_intact(buf) and guards_intact(out)
    want = ref.activity_ref(e, 1e-4, 1e-12, 3, planted=planted)[0]
    assert np.array_equal(out[256:-256].cpu().numpy().reshape(rows, nF), want)
    assert lib.sepr_frame_activity_fwd(ed.data_ptr(), rows, nF, 1e-4, 1e-12, 3, out.data_ptr() + 256, level.data_ptr(), ws, need - 1,
                                       stream()) == L.SEPR_EWORKSPACE


# ---- class sums -------------------------------------------------------------------------------------------------------------------------
def class_problem(C, nF, seed, empty=False):
    rng = np.random.default_rng(seed)
    e_est = rng.uniform(0, 1, size=(C, nF)) * 10.0 ** rng.uniform(-12, 3, size=(C, nF))
    e_mix = rng.uniform(0, 1, size=nF) * 10.0 ** rng.uniform(-12, 3, size=nF)
    active = rng.integers(0, 2, size=(C, nF)).astype(np.uint8) * rng.integers(1, 256, size=(C, nF)).astype(np.uint8)      # any non-zero byte is active
    cls = rng.integers(0, 256, size=(C, nF)).astype(np.uint8)                    # high bits set: only cls & 3 counts
    if empty:
        cls = (cls & 0xFC) | 1                                                   # class 1 alone: three empty classes
    return e_est, e_mix, active, cls


def run_class_sums(tensors, C, nF):
    lib = L.load()
    need = int(lib.sepr_frame_class_sums_bytes(C, nF))
    buf, ws = guarded(need)
    out = torch.full((C * 16 + 64,), float("nan"), dtype=torch.float64, device=DEV)
    call = lambda: lib.sepr_frame_class_sums_fwd(*(t.data_ptr() for t in tensors), C, nF, out.data_ptr() + 256, ws, need, stream())
    return call, out, buf


@pytest.mark.parametrize("C,nF,empty", [(1, 1, False), (2, 255, False), (8, 257, False), (2, 1030, False), (8, 1030, True), (1, 257, True)])
def test_class_sums_are_the_restatement_bit_for_bit(C, nF, empty):
    prob = class_problem(C, nF, seed=C * 10000 + nF, empty=empty)
    want, want_part = ref.class_sums_ref(*prob)
    tensors = [torch.from_numpy(a).to(DEV) for a in prob]
    call, out, buf = run_class_sums(tensors, C, nF)
    assert call() == L.SEPR_OK
    torch.cuda.synchronize()
    got = out[32:32 + C * 16].clone()
    assert guards_intact(buf) and bool(torch.isnan(out[:32]).all()) and bool(torch.isnan(out[32 + C * 16:]).all())
    assert torch.equal(bits64(got), bits64(want.reshape(-1)))
    part = buf[256:256 + C * 64 * 8].clone().view(torch.float64)
    assert torch.equal(bits64(part), bits64(want_part.reshape(-1)))              # the wave sums, stage by stage
    counts = got.view(C, 4, 4)[..., :2].cpu().numpy()
    masked = prob[3] & 3
    assert np.array_equal(counts[..., 0], np.stack([(masked == k).sum(1) for k in range(4)], axis=1))
    assert np.array_equal(counts[..., 1], np.stack([((masked == k) & (prob[2] != 0)).sum(1) for k in range(4)], axis=1))
    assert counts[..., 0].sum() == C * nF and (not empty or (counts[:, [0, 2, 3], 0] == 0).all())
    assert call() == L.SEPR_OK                                                   # two calls give equal bits
    torch.cuda.synchronize()
    assert torch.equal(bits64(out[32:32 + C * 16]), bits64(got))
    via = act.frame_class_sums(*tensors)                                         # the wrapper
    assert torch.equal(bits64(via.reshape(-1)), bits64(got))


def test_class_sums_replay_from_a_graph_after_the_tables_were_rewritten():
    C, nF = 2, 257
    first, second = class_problem(C, nF, seed=1), class_problem(C, nF, seed=2)
    tensors = [torch.from_numpy(a).to(DEV) for a in first]
    call, out, buf = run_class_sums(tensors, C, nF)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert call() == L.SEPR_OK
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call() == L.SEPR_OK
    for t, a in zip(tensors, second):
        t.copy_(torch.from_numpy(a))
    graph.replay()
    torch.cuda.synchronize()
    want = ref.class_sums_ref(*second)[0]
    assert torch.equal(bits64(out[32:32 + C * 16]), bits64(want.reshape(-1))) and guards_intact(buf)
    assert not np.array_equal(want, ref.class_sums_ref(*first)[0])


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
LAMBDA = 0.01
# (utt, start, place, len, track) on 26000 samples: A and B overlap, C and D overlap, E stands alone; gaps between the three groups
HAND = [(0, 0, 0, 4000, 0), (3, 0, 3000, 4000, 1), (1, 0, 9000, 4000, 2), (4, 0, 12000, 3000, 0), (2, 0, 20000, 2600, 1)]
HIDDEN = {0: 0, 3000: 1, 9000: 0, 12000: 1, 20000: 0}                          # place -> channel


def planted(swap=None):
    corpus, _ = synthetic_corpus("float32")
    f = np.float32(1.0)
    conv = cv.make_conversation("hand", 26000, 3, [(u, s, p, n, f, f, t) for u, s, p, n, t in HAND])
    rd = cv.render(corpus, [conv])
    tr = rd.tracks_of(0)
    hidden = np.array([HIDDEN[int(p)] for p in conv.place])
    est = torch.zeros(2, conv.n, device=DEV)
    for c in range(2):
        for g in range(len(conv.utt)):
            a, b = int(conv.place[g]), int(conv.place[g] + conv.len[g])
            seg = tr[int(conv.track[g]), a:b]
            est[c, a:b] += seg if hidden[g] == c else LAMBDA * seg
    if swap is not None:
        a, b = swap
        est[:, a:b] = est[[1, 0], a:b]
    return corpus, conv, rd, est, hidden


def test_a_planted_leak_is_measured():
    """``est_c`` = the segments coloured ``c`` plus 0.01 times the others.  On the cross frames of a channel the mixture holds only the other
    channel's talker and the estimate is 0.01 times it: the pooled leak is 20 log10(0.01) = -40 dB within 1e-4 dB - the float32 rounding of
    ``est`` moves an energy ratio by under 1e-6 relative (4.3e-6 dB), two decades below.  No bed: the quiet frames hold no mixture energy."""
    corpus, conv, rd, est, hidden = planted()
    kw = dict(idle=True, ratio_db=-30.0, hang_ms=40.0, collar_seconds=0.25)
    got = infer.score_conversations(corpus, [conv], rd, [list(est)], 2, **kw)
    assert got["coloured"].tolist() == hidden.tolist() and got["graph_switch_rate"] == 0.0 and np.isnan(got["sisnri_cons"])
    assert conv.place.tolist() == [0, 12000, 3000, 20000, 9000]                  # sorted by (track, place): A, D, B, E, C
    assert np.all(got["graph"][[0, 1, 2, 4]] > 25.0)                           # (E stands alone: the mixture is E there, nothing to improve)
    frame, collar, hang = 160, 2000, 2
    assert (got["frames"]["frame"], got["frames"]["collar"], got["frames"]["hang"]) == (frame, collar, hang)
    x = est.cpu().numpy()
    e_est, e_mix = ref.frame_energy_ref(x, frame), ref.frame_energy_ref(rd.mixture(0).cpu().numpy(), frame)[0]
    active = ref.activity_ref(e_est, 10.0 ** -3.0, 1e-12, hang)[0]
    cls = ref.frame_classes_brute(conv.place, conv.len, hidden, conv.n, 2, frame, collar)
    sums = ref.class_sums_ref(e_est, e_mix, active, cls)[0]
    assert torch.equal(bits64(got["class_sums"][0]), bits64(sums))
    n_idle, a_idle = sums[:, 1, 0] + sums[:, 2, 0], sums[:, 1, 1] + sums[:, 2, 1]
    assert (sums[:, 1, 0] > 5).all() and (sums[:, 2, 0] > 5).all() and (sums[:, 0, 0] > 40).all()
    assert np.array_equal(got["false_alarm"][0], a_idle / n_idle) and np.array_equal(got["miss"][0], (sums[:, 0, 0] - sums[:, 0, 1]) / sums[:, 0, 0])
    assert got["pooled"]["false_alarm"] == a_idle.sum() / n_idle.sum() and got["pooled"]["miss"] == 0.0
    print(f"planted leak: pooled {got['pooled']['leak_db']:.7f} dB, per channel {got['leak_db'][0].tolist()}, false alarm {got['pooled']['false_alarm']:.4f}")
    assert abs(got["pooled"]["leak_db"] - 20.0 * math.log10(LAMBDA)) < 1e-4
    assert np.all(np.abs(got["leak_db"][0] - 20.0 * math.log10(LAMBDA)) < 1e-4)
    assert np.isnan(got["pooled"]["quiet_db"]) and np.isnan(got["quiet_db"]).all()
    assert got["class_frames"].shape == (1, 2, 4) and np.array_equal(got["class_frames"][0], sums[..., 0])


def test_a_planted_swap_over_one_utterance_is_counted():
    """The two estimate rows exchanged over B's span: B's best channel is now A's, the colouring still has to tell them apart - one segment of
    five has ``best != coloured``."""
    corpus, conv, rd, est, hidden = planted(swap=(3000, 7000))
    got = infer.score_conversations(corpus, [conv], rd, [list(est)], 2, idle=True)
    assert got["coloured"][0] != got["coloured"][2]                       # sorted by (track, place): A is row 0, B row 2
    assert got["best"][0] == got["best"][2] == 0 and got["graph_switch_rate"] == 0.2
    assert got["coloured"][[1, 3, 4]].tolist() == hidden[[1, 3, 4]].tolist()


@pytest.fixture(scope="module")
def tiny():
    return Model.from_config(VARIANTS["tiny"], init_seed=0).load_synthetic_(0).eval().to(DEV)


PARENT_KEYS = ["best", "assigned", "utt", "cons", "switch", "assignment", "sisnri_utt", "sisnri_cons", "switch_rate", "n", "overlap", "bins", "v", "v_mix",
               "conversations"]


def test_evaluate_conversations_with_idle_end_to_end(tiny, tmp_path):
    """Three talkers on the model's two channels: ``sisnri_cons`` is NaN, ``sisnri_graph`` is not.  Every figure equals ``score`` and the
    restatement applied to the loop's own tensors, for both methods; the csv files parse; ``idle=False`` is the dict it always was."""
    corpus, _ = synthetic_corpus("both")
    convs = [cv.plan_conversation(corpus, random.Random(21 + i), seconds=2.0 + 0.27 * i, speakers=3, max_active=2, pause=(0.0, 0.3)) for i in (0, 1)]
    assert all(c.S == 3 for c in convs) and convs[1].n % 160 != 0
    kw = dict(chunk_seconds=0.5, overlap_seconds=0.125)
    conv_of = np.concatenate([np.full(len(c.utt), r) for r, c in enumerate(convs)])
    track, ov = np.concatenate([c.track for c in convs]), np.concatenate([cv.overlap_fraction(c) for c in convs])
    spans = (np.concatenate([c.place for c in convs]), np.concatenate([c.len for c in convs]))
    plain = infer.evaluate_conversations(tiny, corpus, convs, method="long", **kw)
    assert list(plain) == PARENT_KEYS and sorted(plain["bins"]["0"]) == ["n", "sisnri_cons", "sisnri_utt"]
    np.testing.assert_equal({k: plain[k] for k in PARENT_KEYS[:12]}, cv.score(plain["v"], plain["v_mix"], conv_of, track, [3, 3], 2, overlap=ov))
    rd = cv.render(corpus, convs)
    ests = longform.separate_long(tiny, [rd.mixture(r) for r in range(2)], **kw)
    for method in ("long", "bank"):
        seg_csv, idle_csv = str(tmp_path / f"seg_{method}.csv"), str(tmp_path / f"idle_{method}.csv")
        got = infer.evaluate_conversations(tiny, corpus, convs, method=method, slots=4, idle=True, csv_path=seg_csv, idle_csv_path=idle_csv, **kw)
        assert np.isnan(got["sisnri_cons"]) and np.isfinite(got["sisnri_graph"]) and (got["coloured"] >= 0).all()
        want = cv.score(got["v"], got["v_mix"], conv_of, track, [3, 3], 2, overlap=ov, spans=spans)
        np.testing.assert_equal({k: got[k] for k in want}, want)
        if method == "long":
            same = [k for k in PARENT_KEYS if k != "bins"]                       # what idle=False returns is unchanged; the bins gain one key
            np.testing.assert_equal({k: got[k] for k in same}, {k: plain[k] for k in same})
            np.testing.assert_equal({b: {k: x for k, x in d.items() if k != "sisnri_graph"} for b, d in got["bins"].items()}, plain["bins"])
        fr = got["frames"]
        frame, e = fr["frame"], fr["e"].cpu().numpy()
        assert frame == 160 and fr["offset"].tolist() == [0] + np.cumsum([-(-c.n // 160) for c in convs]).tolist()
        sums = np.zeros((2, 2, 4, 4))
        g = 0
        for r, c in enumerate(convs):
            fa, fb = fr["offset"][r], fr["offset"][r + 1]
            assert torch.equal(bits64(e[2, fa:fb]), bits64(ref.frame_energy_ref(rd.mixture(r).cpu().numpy(), frame)[0]))
            if method == "long":
                assert torch.equal(bits64(e[:2, fa:fb]), bits64(ref.frame_energy_ref(torch.stack(list(ests[r])).cpu().numpy(), frame)))
            active = fr["active"][r].cpu().numpy()
            assert np.array_equal(active, ref.activity_ref(e[:2, fa:fb], 10.0 ** (-40.0 / 10.0), 1e-12, fr["hang"])[0])
            cls = fr["classes"][r].cpu().numpy()
            G = len(c.utt)
            assert np.array_equal(cls, ref.frame_classes_brute(c.place, c.len, got["coloured"][g:g + G], c.n, 2, frame, fr["collar"]))
            sums[r] = ref.class_sums_ref(e[:2, fa:fb], e[2, fa:fb], active, cls)[0]
            g += G
        assert torch.equal(bits64(got["class_sums"]), bits64(sums)) and np.array_equal(got["class_frames"], sums[..., 0])
        for key, val in cv.idle_figures(sums).items():
            np.testing.assert_equal(got[key], val)
        np.testing.assert_equal(got["pooled"], {k: float(v) for k, v in cv.idle_figures(sums.reshape(-1, 4, 4).sum(0)).items()})
        rows = list(csv.reader(open(seg_csv, newline=""), quotechar="|"))
        assert len(rows) == got["n"] and all(len(r) == 12 for r in rows)
        rows = list(csv.reader(open(idle_csv, newline=""), quotechar="|"))
        assert len(rows) == 4 and [r[:3] for r in rows] == [[convs[i // 2].key, str(i // 2), str(i % 2)] for i in range(4)]
        for i, row in enumerate(rows):
            assert [int(x) for x in row[3:7]] == got["class_frames"][i // 2, i % 2].tolist()
            np.testing.assert_equal([float(x) for x in row[7:]], [float(got[k][i // 2, i % 2]) for k in ("leak_db", "quiet_db", "false_alarm", "miss")])


def test_the_command_line_writes_the_runs_of_channel_activity(tiny, tmp_path, monkeypatch, capsys):
    """``python -m sepreformer_amd.infer FILE --activity-csv OUT`` on its three paths - whole file, ``--chunk-seconds``, ``--slots`` - writes the runs
    of ``segments(channel_activity(tracks))`` of the tracks that path separates."""
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.normal(0, 0.1, 4000), np.zeros(4000), rng.normal(0, 0.1, 4001)]).astype(np.float32)
    wav = str(tmp_path / "talk.wav")
    infer.write_wav(wav, x, 8000)
    paths = {"whole": ([], lambda: infer.separate_file(tiny, wav)[0]),
             "long": (["--chunk-seconds", "0.5", "--overlap-seconds", "0.125"],
                      lambda: infer.separate_long_file(tiny, wav, chunk_seconds=0.5, overlap_seconds=0.125)[0]),
             "bank": (["--slots", "2", "--chunk-seconds", "0.5", "--overlap-seconds", "0.125"],
                      lambda: infer.separate_many_files(tiny, [wav], slots=2, chunk_seconds=0.5, overlap_seconds=0.125)[0][0])}
    for name, (flags, direct) in paths.items():
        out = str(tmp_path / f"{name}.csv")
        monkeypatch.setattr(sys, "argv", ["infer", wav, "--model", "tiny", "--device", DEV, "--activity-csv", out, "--activity-ratio-db", "-35",
                                          "--activity-hang-ms", "60"] + flags)
        infer._main()
        assert out in capsys.readouterr().out.split("\n")
        tracks = torch.from_numpy(direct()).to(DEV)
        active, _, _ = act.channel_activity(tracks, fs=8000, ratio_db=-35.0, hang_ms=60.0)
        runs = act.segments(active, 160, tracks.shape[1])
        got = [(int(c), float(b), float(e)) for c, b, e in csv.reader(open(out, newline=""), quotechar="|")]
        assert got == [(c, b / 8000.0, e / 8000.0) for c, rs in enumerate(runs) for b, e in rs] and len(got) >= 1, name
        assert all(e <= 12001 / 8000.0 for _, _, e in got)
