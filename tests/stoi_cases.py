"""Inputs shared by tests/test_stoi_cpu.py and tests/test_stoi_gpu.py: references cut from tests/golden/sample_WSJ.wav with inserted
pauses, estimates built as tests/test_bss_eval_gpu.py::_speech_case builds them (a filtered copy with leakage, a noisy copy), the plain
mixture, and the float64 restatement's values for them (computed once per process and never modified).

Pauses: two stretches per reference scaled by 1e-4, so that the silent-frame removal really removes frames.  A stretch is 0.25 s where
the utterance is long enough to keep 30 spectral frames beside it; the 0.75 s and 0.5 s utterances of the ragged batch take 0.1 s and
0.05 s stretches (two 0.25 s stretches would leave them 21 and 2 frames, i.e. "too short", which has a case of its own).
"""
import functools
import os

import numpy as np

import stoi_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))

# name -> (fs, S, lengths, wav offset of the first reference of each utterance)
CASES = {
    "ragged_8k": (8000, 2, (4000, 6000, 8000), (1000, 9000, 21000)),
    "three_8k": (8000, 3, (8000,), (3000,)),
    "long_10k": (10000, 2, (42000,), (500,)),          # 297 segments: more than the 256 threads of the segment walk
    "one_16k": (16000, 2, (12000,), (30000,)),
}
SPACING = 9000         # the references of one utterance start this many samples apart in the recording (wrapping around)


@functools.lru_cache(maxsize=None)
def wav():
    from scipy.io import wavfile
    sr, d = wavfile.read(os.path.join(HERE, "golden", "sample_WSJ.wav"))
    assert sr == 8000 and d.dtype == np.int16
    return d.astype(np.float64) / 32768.0


def _pause_len(n, fs):
    sec = n / fs
    return int(round((0.25 if sec >= 1.0 else 0.1 if sec >= 0.75 else 0.05) * fs))


def _reference(start, n, fs, which):
    x = np.take(wav(), np.arange(start, start + n), mode="wrap").copy()
    p = _pause_len(n, fs)
    for c in ((0.22 + 0.05 * which) * n, (0.68 - 0.04 * which) * n):      # two stretches, at different places per reference
        a = int(c) - p // 2
        x[a:a + p] *= 1e-4
    return x


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(fs, S, lengths, T, src [S][B][T], est [S][B][T], mix [B][T]) float32; samples beyond an utterance's length are noise, which a
    correct implementation never reads."""
    fs, S, lengths, offsets = CASES[name]
    B, T = len(lengths), max(lengths)
    rng = np.random.default_rng(sum(map(ord, name)))
    src = 0.05 * rng.standard_normal((S, B, T))
    est = 0.05 * rng.standard_normal((S, B, T))
    mix = 0.05 * rng.standard_normal((B, T))
    for b, (n, off) in enumerate(zip(lengths, offsets)):
        s = np.stack([_reference(off + i * SPACING, n, fs, i) for i in range(S)])
        e = [0.7 * np.convolve(s[1], [1.0, 0.4, -0.2])[:n] + 0.05 * s[0] + 1e-3 * rng.standard_normal(n),
             1.3 * s[0] + 0.1 * s[1] + 3e-3 * rng.standard_normal(n)]
        if S == 3:
            e.append(0.9 * s[2] + 0.2 * s[0] + 1e-2 * rng.standard_normal(n))
        src[:, b, :n], est[:, b, :n], mix[b, :n] = s, np.stack(e), s.sum(0)
    f32 = lambda a: np.ascontiguousarray(a.astype(np.float32))             # noqa: E731
    return {"fs": fs, "S": S, "lengths": list(lengths), "T": T, "src": f32(src), "est": f32(est), "mix": f32(mix)}


@functools.lru_cache(maxsize=None)
def expected(name, round_taps=False, round_signals=False):
    """The restatement on build(name): per utterance b and reference i, ref.evaluate against the S estimates and the mixture.
    -> dict(stoi [B][S][S], estoi [B][S][S], stoi_mix [B][S], estoi_mix [B][S], kept [B][S], frames [B][S], margin [B][S], short [B][S])"""
    c = build(name)
    S, B = c["S"], len(c["lengths"])
    out = {"stoi": np.empty((B, S, S)), "estoi": np.empty((B, S, S)), "stoi_mix": np.empty((B, S)), "estoi_mix": np.empty((B, S)),
           "kept": np.empty((B, S), np.int64), "frames": np.empty((B, S), np.int64), "margin": np.empty((B, S)),
           "short": np.empty((B, S), bool)}
    for b, n in enumerate(c["lengths"]):
        for i in range(S):
            r = ref.evaluate(c["src"][i, b, :n], [c["est"][j, b, :n] for j in range(S)] + [c["mix"][b, :n]], c["fs"],
                             round_taps=round_taps, round_signals=round_signals)
            out["stoi"][b, i], out["estoi"][b, i] = r["stoi"][:S], r["estoi"][:S]
            out["stoi_mix"][b, i], out["estoi_mix"][b, i] = r["stoi"][S], r["estoi"][S]
            for k in ("kept", "frames", "margin", "short"):
                out[k][b, i] = r[k]
    for v in out.values():
        v.setflags(write=False)
    return out


def delta(name):
    """The largest change of the restatement's own values on build(name) when the converter's taps and the 10 kHz signals are rounded to
    float32, as the device design rounds them."""
    a, b = expected(name), expected(name, True, True)
    return max(float(np.max(np.abs(a[k] - b[k]))) for k in ("stoi", "estoi", "stoi_mix", "estoi_mix"))
