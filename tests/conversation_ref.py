"""Restatement of the conversation render and the segment-wise SI-SNR, written from include/sepr.h (it shares no code with
``sepreformer_amd``): a float32 numpy loop in the stated order, the per-pair term of the oracle's SI-SNR in float64 on the slices, and an
invariant checker for schedules.  A conversation here is anything with the attributes ``n, S, utt, start, place, len, norm, gain, track``."""
from __future__ import annotations

import numpy as np
import torch

from oracle.criterion_oracle import _sisnr

EPS = 1e-15


def sample_values(a: np.ndarray) -> np.ndarray:
    """float32 sample values of a stored utterance: an int16 sample is ``int16 / 32768`` (exact)."""
    return a.astype(np.float32) / np.float32(32768.0) if a.dtype == np.int16 else a.astype(np.float32)


def render_ref(arrays, convs, S_max=None):
    """-> (mix float32 [total], tracks float32 [S_max, total], out_off).  ``arrays``: the utterances in corpus storage order."""
    S_max = S_max or max(c.S for c in convs)
    out_off = np.concatenate([[0], np.cumsum([c.n for c in convs])]).astype(np.int64)
    total = int(out_off[-1])
    tracks = np.zeros((S_max, total), dtype=np.float32)           # +0.0 where no segment covers a sample
    for r, c in enumerate(convs):
        for g in range(len(c.utt)):
            x = sample_values(arrays[int(c.utt[g])])[int(c.start[g]):int(c.start[g]) + int(c.len[g])]
            assert x.shape[0] == int(c.len[g]), "the segment reads past its utterance"
            a = x * np.float32(c.norm[g])                         # two separately rounded float32 multiplies
            o = int(out_off[r]) + int(c.place[g])
            tracks[int(c.track[g]), o:o + int(c.len[g])] = a * np.float32(c.gain[g])
    mix = np.zeros(total, dtype=np.float32)
    for s in range(S_max):                                        # ((0 + track 0) + track 1) + ...
        mix = mix + tracks[s]
    return mix, tracks, out_off


def sisnr_ref(est, ref, mix, rows, begin, length, eps=EPS, dtype=torch.float64):
    """-> (v [G, C], v_mix [G]) float64 through the oracle's ``_sisnr`` on the slices (numpy in, numpy out)."""
    G, C = len(rows), est.shape[0]
    v, vm = np.zeros((G, C)), np.zeros(G)
    for g in range(G):
        sl = slice(int(begin[g]), int(begin[g]) + int(length[g]))
        r = torch.from_numpy(np.ascontiguousarray(ref[int(rows[g]), sl])).to(dtype)
        for c in range(C):
            v[g, c] = float(_sisnr(torch.from_numpy(np.ascontiguousarray(est[c, sl])).to(dtype)[None], r[None], eps)[0])
        vm[g] = float(_sisnr(torch.from_numpy(np.ascontiguousarray(mix[sl])).to(dtype)[None], r[None], eps)[0])
    return v, vm


def sisnr_longdouble(a, r, eps=EPS):
    """The header's definition in numpy ``longdouble``: one pair, one value."""
    a, r = a.astype(np.longdouble), r.astype(np.longdouble)
    eps = np.longdouble(eps)
    at, rt = a - a.sum() / len(a), r - r.sum() / len(r)
    s_rr, s_ar = (rt * rt).sum(), (at * rt).sum()
    alpha = s_ar / (s_rr + eps)
    d = at - alpha * rt
    return float(20 * np.log10(eps + abs(alpha) * np.sqrt(s_rr) / (np.sqrt((d * d).sum()) + eps)))


def correlation(a, r):
    """|rho| of the centred pair in float64 (0 for a silent side)."""
    a, r = a.astype(np.float64), r.astype(np.float64)
    at, rt = a - a.mean(), r - r.mean()
    den = np.sqrt((at * at).sum() * (rt * rt).sum())
    return 0.0 if den == 0 else float(abs((at * rt).sum()) / den)


def tol_db(n: int) -> float:
    """The derived tolerance of DESIGN.md section 5h: (n + 16) u bounds any summation order's relative error on a sum of squares, 8.69 = 20 / ln 10
    turns a relative error into dB, 100 covers both norms on both sides and the cancellation in s_ar (at most 1 / |rho| <= 34)."""
    return 1e-12 + 8.69 * 100 * (n + 16) * 2.0 ** -53


LENGTHS = (1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 5000)
FAMILIES = ("noise", "swapped", "dc", "silent_ref", "silent_est")


def _at_snr(rng, r, snr_db):
    """``r + k * noise`` with the noise centred and made orthogonal to the centred ``r`` and ``k`` chosen so that the SI-SNR is ``snr_db`` (up
    to the float32 rounding of the sum): the case's conditioning is set by its label, not by the draw."""
    r64 = r.astype(np.float64)
    rt = r64 - r64.mean()
    z = rng.normal(0, 1, size=r.shape[0])
    z = z - z.mean()
    z = z - (z @ rt) / (rt @ rt) * rt
    k = np.sqrt((rt @ rt) / (z @ z)) * 10.0 ** (-snr_db / 20.0)
    return (r64 + k * z).astype(np.float32)


def sisnr_problem(C: int, seed: int = 0):
    """One call's worth of segment SI-SNR cases for ``C`` channels and ``S = C`` reference rows: every length of ``LENGTHS`` under every family of
    ``FAMILIES``, each segment on a stretch of its own of rows of ``ld > T`` floats, no ``begin`` a multiple of 4.

    * ``noise``: channel ``c`` is the scored reference plus noise at the c-th of +50, +20, -20 dB - channel 0 is the best;
    * ``swapped``: the same at 0, +35, -10 dB - another channel than 0 is the best;
    * ``dc``: reference and channels have mean 0.5 and deviation 1e-3 (+30, +10, 0 dB), on which sums of raw moments lose about six digits;
    * ``silent_ref`` / ``silent_est``: a reference segment of zeros / channel 0 of zeros: -300 dB.

    A single sample is silent once centred, whatever it holds: length 1 runs under every family and gives -300.  Two centred samples are always
    perfectly correlated or anti-correlated: the residual is rounding alone and the value, above +200 dB, is set by ``eps`` and the last bit of
    ``alpha`` - no bound on relative errors applies - so length 2 runs under the two silent families only, and its ``silent_est`` has every
    channel and the mixture silent.
    -> dict(est [C, ld], ref [C, ld], mix [ld], rows, begin, length, family (per segment), T, ld)."""
    rng = np.random.default_rng(seed)
    S = C
    snrs = {"noise": (50.0, 20.0, -20.0), "swapped": (0.0, 35.0, -10.0), "dc": (30.0, 10.0, 0.0)}
    segs, pos = [], 0
    for n in LENGTHS:
        for fam in FAMILIES:
            if n == 2 and not fam.startswith("silent"):
                continue
            b = pos + 1 + len(segs) % 3
            b += 1 if b % 4 == 0 else 0
            segs.append((fam, b, n))
            pos = b + n + 2
    T = pos + 3
    ld = T + 12
    ref = rng.normal(0, 0.1, size=(S, ld)).astype(np.float32)
    est = rng.normal(0, 0.1, size=(C, ld)).astype(np.float32)
    ref[:, T:] = np.nan                                             # the padding of a row is never read
    est[:, T:] = np.nan
    rows, begin, length, family = [], [], [], []
    for g, (fam, b, n) in enumerate(segs):
        row = g % S
        sl = slice(b, b + n)
        if fam == "dc":
            ref[:, sl] = (0.5 + 1e-3 * rng.normal(0, 1, size=(S, n))).astype(np.float32)
        if fam == "silent_ref":
            ref[row, sl] = 0.0
        elif n >= 3:
            for c in range(C):
                est[c, sl] = _at_snr(rng, ref[row, sl], snrs.get(fam, snrs["noise"])[c])
        if fam == "silent_est":
            est[slice(None) if n == 2 else 0, sl] = 0.0
        rows.append(row), begin.append(b), length.append(n), family.append(fam)
    mix = np.zeros(ld, dtype=np.float32)
    for s in range(S):
        mix = mix + ref[s]
    for fam, b, n in segs:
        if n == 2 and fam == "silent_est":
            mix[b:b + n] = 0.0
    return dict(est=est, ref=ref, mix=mix, rows=np.array(rows, np.int32), begin=np.array(begin, np.int32), length=np.array(length, np.int32),
                family=family, T=T, ld=ld)


def check_schedule(c, max_active=None, lengths=None):
    """Assert the invariants of a schedule: sorted by (track, place), inside [0, n), n a multiple of 4, the segments of one track
    disjoint, at most ``max_active`` tracks active at any sample, and - with the corpus ``lengths`` - every read inside its utterance."""
    G = len(c.utt)
    assert G >= 1 and c.n % 4 == 0 and c.n >= 4 and 1 <= c.S <= 8
    for f, dt in (("utt", np.int32), ("start", np.int32), ("place", np.int32), ("len", np.int32), ("norm", np.float32), ("gain", np.float32),
                  ("track", np.int32)):
        col = getattr(c, f)
        assert col.dtype == dt and col.shape == (G,), f
    key = [(int(t), int(p)) for t, p in zip(c.track, c.place)]
    assert key == sorted(key)
    assert c.len.min() >= 1 and c.place.min() >= 0 and int((c.place.astype(np.int64) + c.len).max()) <= c.n
    assert c.track.min() >= 0 and c.track.max() < c.S and c.start.min() >= 0
    for g in range(1, G):
        if c.track[g] == c.track[g - 1]:
            assert int(c.place[g - 1]) + int(c.len[g - 1]) <= int(c.place[g]), g
    if lengths is not None:
        assert np.all(c.start.astype(np.int64) + c.len <= np.asarray(lengths)[c.utt])
    if max_active is not None:
        active = np.zeros(c.n + 1, dtype=np.int64)
        np.add.at(active, c.place, 1)
        np.add.at(active, c.place.astype(np.int64) + c.len, -1)
        assert int(np.cumsum(active).max()) <= max_active
