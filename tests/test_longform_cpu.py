"""Long-form separation without a device: the geometry, the float64 restatement of the stitching (tests/longform_ref.py)
on planted chunk permutations and gains, the gain-carry rules, and the C-ABI argument checks of sepr_stitch_fwd."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_ref as ref                                                   # noqa: E402

from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import longform                                         # noqa: E402


@pytest.mark.parametrize("W,O", [(32000, 8000), (64, 32), (64, 4), (48, 12)])
def test_geometry(W, O):
    H = W - O
    for T in list(range(1, 3 * W)) if W < 100 else [1, W - 1, W, W + 1, W + H, W + H + 1, 73600, 28_800_000]:
        nc = ref.num_chunks(T, W, O)
        assert nc == longform.num_chunks(T, W, O)
        if T <= W:
            assert nc == 1
            continue
        assert (nc - 1) * H + W >= T > (nc - 2) * H + W               # the last window reaches T, one fewer would not
        for k in range(nc - 1):                                          # every overlap [(k+1)H, kH + W) lies inside [0, T)
            assert 0 <= (k + 1) * H and k * H + W <= T
    w_in, w_out = ref.crossfade_f32(O)
    assert w_in.dtype == np.float32 and np.all(w_in + w_out == np.float32(1.0))
    assert np.all(np.diff(w_in) >= 0) and 0 < w_in[0] < 0.05 and 0.95 < w_in[-1] <= 1 and np.all(w_out >= 0)


def test_sepreformer_recording_geometry():
    """The reference's sample (9.2 s at 8 kHz) is 3 windows at 4 s / 1 s; an hour is 1200."""
    assert ref.num_chunks(73600, 32000, 8000) == 3
    assert ref.num_chunks(3600 * 8000, 32000, 8000) == 1200
    assert list(ref.chunk_offsets([73600, 100, 32001], 32000, 8000)) == [0, 3, 4, 6]


def _sources(S, T, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((S, T))
    for s in range(S):
        w = rng.standard_normal(T)
        y = np.zeros(T)
        a = 1.5 - 0.3 * s
        for t in range(T):
            y[t] = w[t] + (a * y[t - 1] - 0.7 * y[t - 2] if t >= 2 else 0.0)
        out[s] = y / np.abs(y).max()
    return out


def _planted(src, W, O, seed, match_gain):
    """Cut the true sources into windows; permute every window's sources at random and (match_gain) scale them by random
    nonzero gains of either sign.  -> chunks [Nc, S, W]."""
    S, T = src.shape
    rng = np.random.default_rng(seed)
    cuts = np.stack([ref.cut(src[s], W, O) for s in range(S)], axis=1)   # [Nc, S, W]
    out = np.empty_like(cuts)
    for k in range(cuts.shape[0]):
        p = rng.permutation(S)
        g = rng.uniform(0.3, 3.0, S) * rng.choice([-1.0, 1.0], S) if match_gain else np.ones(S)
        for s in range(S):
            out[k, p[s]] = g[s] * cuts[k, s]
    return out


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("match_gain", [False, True])
def test_planted_recovery(S, match_gain):
    W, O = 256, 64
    T = 2000                                                             # 9 windows, the last one padded
    src = _sources(S, T, seed=S)
    chunks = _planted(src, W, O, seed=10 + S, match_gain=match_gain)
    y, perm, gain = ref.stitch(chunks, T, O, match_gain)
    assert y.shape == (S, T)
    # one global permutation (and, with match_gain, one global gain per track) maps the output onto the sources
    best = None
    for p in itertools.permutations(range(S)):
        ok = True
        for s in range(S):
            tgt = src[p[s]]
            g = y[s] @ tgt / (tgt @ tgt)
            if not match_gain and abs(abs(g) - 1.0) > 1e-12:
                ok = False
            if np.abs(y[s] - g * tgt).max() > 1e-12:
                ok = False
        if ok:
            best = p
    assert best is not None
    if not match_gain:                                                   # without gain matching the signs stay as planted
        assert np.all(gain == 1.0)


def test_planted_recovery_many_windows_and_padding():
    W, O, S = 64, 16, 2
    T = W + 56 * (W - O) + 5                                             # 58 windows, 5 samples into the last
    src = _sources(S, T, seed=7)
    chunks = _planted(src, W, O, seed=8, match_gain=True)
    assert chunks.shape[0] == 58
    y, _, _ = ref.stitch(chunks, T, O, True)
    g = [y[s] @ src[s] / (src[s] @ src[s]) for s in range(S)]
    if abs(g[0]) < 0.1:
        g = [y[s] @ src[1 - s] / (src[1 - s] @ src[1 - s]) for s in range(S)]
        src = src[::-1]
    for s in range(S):
        assert np.abs(y[s] - g[s] * src[s]).max() <= 1e-12


def test_single_window_is_the_window():
    rng = np.random.default_rng(0)
    chunks = rng.standard_normal((1, 2, 64))
    y, perm, gain = ref.stitch(chunks, 50, 16, True)
    assert np.array_equal(y, chunks[0, :, :50]) and list(perm[0]) == [0, 1] and np.all(gain == 1)


def test_gain_carry_rules():
    O = 100
    rng = np.random.default_rng(1)
    a = rng.standard_normal((2, O))
    # matched pair well correlated: the least-squares ratio, sign included
    b = np.stack([-2.0 * a[0], 0.5 * a[1]])
    C, Ea, Eb = a @ b.T, (a * a).sum(1), (b * b).sum(1)
    pi, ratio = ref.choose(C, Ea, Eb, O, True)
    assert pi == (0, 1) and np.allclose(ratio, [-0.5, 2.0], rtol=1e-14)
    pi, ratio = ref.choose(C, Ea, Eb, O, False)
    assert np.all(ratio == 1.0)
    # silent incoming source: carried
    b0 = np.stack([np.zeros(O), 0.5 * a[1]])
    C, Ea, Eb = a @ b0.T, (a * a).sum(1), (b0 * b0).sum(1)
    _, ratio = ref.choose(C, Ea, Eb, O, True)
    assert ratio[0] == 1.0 and abs(ratio[1] - 2.0) < 1e-12
    # below the silence floor (mean square 1e-12 per sample) but otherwise perfectly correlated: carried
    b1 = np.stack([1e-6 * a[0] / np.sqrt((a[0] ** 2).mean()), 0.5 * a[1]])
    C, Ea, Eb = a @ b1.T, (a * a).sum(1), (b1 * b1).sum(1)
    _, ratio = ref.choose(C, Ea, Eb, O, True)
    assert ratio[0] == 1.0
    # normalised correlation below rho_min (0.5): carried; above it: not
    for mix, carried in ((0.3, True), (0.7, False)):
        n = a[1] - (a[1] @ a[0]) / (a[0] @ a[0]) * a[0]                  # orthogonal to a[0]
        n *= np.linalg.norm(a[0]) / np.linalg.norm(n)
        b2 = np.stack([mix * a[0] + np.sqrt(1 - mix * mix) * n, 0.5 * a[1]])
        C, Ea, Eb = a @ b2.T, (a * a).sum(1), (b2 * b2).sum(1)
        pi, ratio = ref.choose(C, Ea, Eb, O, True)
        if pi == (0, 1):
            assert (ratio[0] == 1.0) == carried, (mix, ratio)
    # all silent: every score ties at 0 -> the identity
    z = np.zeros((3, 3))
    pi, ratio = ref.choose(z, np.zeros(3), np.zeros(3), O, True)
    assert pi == (0, 1, 2) and np.all(ratio == 1.0)


def test_carried_gain_propagates_through_silence():
    """A track silent on one boundary keeps its gain and is re-aligned on the next."""
    W, O, S = 64, 16, 2
    T = W + 2 * (W - O)
    src = _sources(S, T, seed=3)
    src[0, W - O:W + 10] = 0.0                                           # source 0 silent over the first overlap
    chunks = _planted(src, W, O, seed=4, match_gain=False)
    chunks[1] *= 3.0
    chunks[2] *= 6.0
    perm, gain = ref.plan(chunks, O, True)
    assert gain.shape == (3, 2) and np.isfinite(gain).all()
    silent = [s for s in range(S) if np.abs(chunks[0, perm[0, s], W - O:]).max() == 0][0]
    assert gain[1, silent] == 1.0                                         # silent on boundary 0: carried
    assert abs(gain[1, 1 - silent] - 1 / 3) < 1e-12                       # the other track: aligned
    assert abs(gain[2, silent] - 0.5) < 1e-12                                     # aligned again on boundary 1, from the carried gain
    assert abs(gain[2, 1 - silent] - 1 / 6) < 1e-12


# ---- C ABI: every argument check comes before any HIP call ------------------------------------------------------------
def _call(S=2, W=64, O=16, lengths=(100,), offsets=None, R=None, ws_bytes=None, ptr=4096, y=4096, null=None):
    lib = L.load()
    R = len(lengths) if R is None else R
    if offsets is None:
        offsets = list(ref.chunk_offsets(lengths, W, O)) if 2 * O <= W and O > 0 and W - O > 0 else [0] * (len(lengths) + 1)
    coff = (C.c_int * len(offsets))(*[int(v) for v in offsets])
    lens = (C.c_int * len(lengths))(*lengths)
    total = int(offsets[-1])
    if ws_bytes is None:
        ws_bytes = lib.sepr_stitch_workspace(R, total, S) if 2 <= S <= 3 else 1 << 20
    args = dict(chunks=ptr, coff=coff, lens=lens, y=y, perm=4096, gain=4096, ws=4096)
    if null:
        args[null] = None
    return lib.sepr_stitch_fwd(args["chunks"], args["coff"], args["lens"], R, S, W, O, 1, args["y"], args["perm"], args["gain"],
                               args["ws"], ws_bytes, None)


def test_abi_workspace():
    lib = L.load()
    for S in (2, 3):
        ns = S * S + 2 * S
        assert lib.sepr_stitch_workspace(1, 1, S) == 256 * 3
        assert lib.sepr_stitch_workspace(5, 1200, S) == -(-1200 * ns * 8 // 256) * 256 + 256 + 256
    assert lib.sepr_stitch_workspace(1, 1, 1) == 0 and lib.sepr_stitch_workspace(1, 1, 4) == 0
    assert lib.sepr_stitch_workspace(0, 1, 2) == 0 and lib.sepr_stitch_workspace(3, 2, 2) == 0


def test_abi_argument_checks():
    E = L.SEPR_EINVAL
    for name in ("chunks", "coff", "lens", "y", "perm", "gain"):
        assert _call(null=name) == E, name
    assert _call(S=1) == E and _call(S=4) == E
    assert _call(W=66, O=16) == E                                        # W % 4
    assert _call(W=64, O=18) == E                                        # O % 4
    assert _call(W=64, O=0, offsets=[0, 1], lengths=(50,)) == E          # O = 0
    assert _call(W=64, O=36, offsets=[0, 3], lengths=(100,)) == E        # O > W / 2
    assert _call(ptr=4100) == E and _call(y=4104) == E                    # not 16-byte aligned
    assert _call(lengths=(100, 50), offsets=[0, 2, 1]) == E              # non-monotone offsets
    assert _call(lengths=(100,), offsets=[1, 3]) == E                    # offsets must start at 0
    assert _call(lengths=(100,), offsets=[0, 3]) == E                    # Nc inconsistent with the length (2 expected)
    assert _call(lengths=(64,), offsets=[0, 2]) == E                     # T <= W is one window
    assert _call(lengths=(0,), offsets=[0, 1]) == E                      # empty recording
    assert _call(R=0, lengths=(100,), offsets=[0]) == E
    assert _call(ws_bytes=100) == L.SEPR_EWORKSPACE
    assert _call(null="ws") == L.SEPR_EWORKSPACE


def test_python_geometry_checks():
    longform.check_geometry(32000, 8000)
    for W, O in ((32002, 8000), (32000, 8002), (32000, 0), (32000, 16004), (12, 4)):
        with pytest.raises(ValueError):
            longform.check_geometry(W, O)
    offs, rows, n = longform.out_layout([73600, 100], 32000, 8000, 2)
    assert offs == [0, 2 * (3 * 24000 + 8000)] and rows == [3 * 24000 + 8000, 32000] and n == 2 * (4 * 24000 + 2 * 8000)
