"""BSS-eval SDR (PIT_SDRi) without a device: the float64 restatement of mir_eval's bss_eval_sources (tests/bss_eval_ref.py)
against a third formulation and known answers, the C-ABI argument checks of sepr_bss_eval_fwd, and the no-CPU-path rule."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bss_eval_ref as ref                                                  # noqa: E402

from sepreformer_amd import criterion as crit                               # noqa: E402
from sepreformer_amd import lib as L                                        # noqa: E402


def _speechlike(S, n, seed, tail=0):
    """S decorrelated AR(2)-filtered noise sources of n samples (the last `tail` zero)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((S, n))
    for s in range(S):
        w = rng.standard_normal(n - tail)
        y = np.zeros(n - tail)
        a1, a2 = 1.6 - 0.2 * s, -0.8
        for t in range(n - tail):
            y[t] = w[t] + (a1 * y[t - 1] if t >= 1 else 0.0) + (a2 * y[t - 2] if t >= 2 else 0.0)
        out[s, : n - tail] = y / np.abs(y).max()
    return out


def _lstsq_crit(refs, e, flen=ref.FLEN):
    """Third formulation: dense least squares on the explicit (L+F-1) x (S F) shift matrix.  -> sdr [S], sir [S], sar."""
    S, n = refs.shape
    N = n + flen - 1
    A = np.zeros((N, S * flen))
    for i in range(S):
        for a in range(flen):
            A[a:a + n, i * flen + a] = refs[i]
    ep = np.concatenate([e, np.zeros(flen - 1)])

    def proj(cols):
        c = np.linalg.lstsq(A[:, cols], ep, rcond=None)[0]
        return A[:, cols] @ c

    p_all = proj(slice(None))
    sdr, sir = np.empty(S), np.empty(S)
    for j in range(S):
        p_j = proj(slice(j * flen, (j + 1) * flen))
        sdr[j] = 10 * np.log10(np.sum(p_j ** 2) / np.sum((ep - p_j) ** 2))
        sir[j] = 10 * np.log10(np.sum(p_j ** 2) / np.sum((p_all - p_j) ** 2))
    sar = 10 * np.log10(np.sum(p_all ** 2) / np.sum((ep - p_all) ** 2))
    return sdr, sir, sar


def test_restatement_agrees_with_dense_least_squares():
    refs = _speechlike(2, 1600, 0)
    rng = np.random.default_rng(1)
    ests = np.stack([0.8 * refs[1] + 0.2 * refs[0] + 0.05 * rng.standard_normal(1600),
                     np.convolve(refs[0], [1.0, -0.3, 0.1])[:1600] + 0.1 * refs[1] + 0.02 * rng.standard_normal(1600)])
    sdr, sir, sar, perm = ref.bss_eval_sources(refs, ests)
    assert list(perm) == [1, 0]
    for k in range(2):
        want_sdr, want_sir, want_sar = _lstsq_crit(refs, ests[perm[k]])
        assert abs(sdr[k] - want_sdr[k]) < 1e-8, (sdr[k], want_sdr[k])
        assert abs(sir[k] - want_sir[k]) < 1e-8, (sir[k], want_sir[k])
        assert abs(sar[k] - want_sar) < 1e-8, (sar[k], want_sar)


def test_known_answers():
    refs = _speechlike(2, 1600, 2, tail=512)
    # an estimate equal to its reference: SDR >= 100 dB or +inf, never NaN
    sdr, sir, sar, perm = ref.bss_eval_sources(refs, refs.copy())
    assert list(perm) == [0, 1] and not np.isnan(sdr).any() and (sdr >= 100).all()
    # an FIR of <= 512 taps applied to a reference that ends in 512 zeros lies in the span of its delays
    h = np.random.default_rng(3).standard_normal(300) * np.exp(-np.arange(300) / 40.0)
    ests = np.stack([np.convolve(refs[0], h)[:1600], refs[1]])
    sdr, _, _, perm = ref.bss_eval_sources(refs, ests)
    assert list(perm) == [0, 1] and (sdr >= 100).all(), sdr


def test_scale_invariance_swap_and_duplicated_mixture():
    refs = _speechlike(2, 1600, 4)
    rng = np.random.default_rng(5)
    ests = np.stack([refs[0] + 0.3 * refs[1] + 0.05 * rng.standard_normal(1600), refs[1] - 0.2 * refs[0] + 0.1 * rng.standard_normal(1600)])
    sdr, sir, sar, perm = ref.bss_eval_sources(refs, ests)
    sdr2, sir2, sar2, perm2 = ref.bss_eval_sources(refs, ests * np.array([[3.7], [0.01]]))
    assert np.abs(sdr - sdr2).max() < 1e-9 and list(perm) == list(perm2) == [0, 1]
    sdr3, sir3, sar3, perm3 = ref.bss_eval_sources(refs, ests[::-1].copy())
    assert list(perm3) == [1, 0]
    assert np.abs(sdr3 - sdr).max() < 1e-9 and np.abs(sir3 - sir).max() < 1e-9 and np.abs(sar3 - sar).max() < 1e-9
    mix = refs.sum(0)
    _, _, _, pm = ref.bss_eval_sources(refs, np.stack([mix, mix]))
    assert list(pm) == [0, 1]


def test_silent_source_is_an_error():
    refs = _speechlike(2, 1600, 6)
    with pytest.raises(ValueError):
        ref.bss_eval_sources(refs, np.stack([refs[0], np.zeros(1600)]))


def _call(S=2, B=1, T=2048, lengths=None, mix=1, sdr_mix=1, ws_bytes=None):
    lib = L.load()
    lens = (C.c_int * B)(*(lengths or [T] * B))
    if ws_bytes is None:
        ws_bytes = lib.sepr_bss_eval_workspace(S, B, T) if 2 <= S <= 3 else 1 << 20
    p = 4096                                                                  # never dereferenced: every check comes first
    return lib.sepr_bss_eval_fwd(p, p, mix, lens, S, B, T, p, p, p, p, sdr_mix, p, p, ws_bytes, None)


def test_abi_argument_checks():
    lib = L.load()
    assert L.ABI_VERSION == 413
    assert lib.sepr_bss_eval_workspace(4, 1, 4096) == 0 and lib.sepr_bss_eval_workspace(2, 1, 1000) == 0
    assert lib.sepr_bss_eval_workspace(2, 1, 32000) > (2 * 512) ** 2 * 8
    assert _call(S=4, T=4096) == L.SEPR_EINVAL
    assert _call(S=1) == L.SEPR_EINVAL
    assert _call(S=2, lengths=[2 * 512 - 1]) == L.SEPR_EINVAL                 # L < S * 512
    assert _call(S=3, T=1535) == L.SEPR_EINVAL                                 # T < S * 512
    assert _call(S=2, lengths=[2049]) == L.SEPR_EINVAL                         # L > T
    assert _call(mix=None, sdr_mix=4096) == L.SEPR_EINVAL
    assert _call(ws_bytes=1024) == L.SEPR_EWORKSPACE


def test_no_cpu_path():
    x = torch.randn(2, 1, 2048)
    with pytest.raises(RuntimeError, match="HIP device"):
        crit.PIT_SDRi("cpu", 0)(estims=[x[0], x[1]], mixture=x.sum(0), input_sizes=torch.tensor([2048]), target_attr=[x[1], x[0]])
    with pytest.raises(RuntimeError, match="HIP device"):
        crit.bss_eval_sources(x[:, 0], x[:, 0])
    assert repr(crit.PIT_SDRi("cpu", 0)) == "<PIT_SDRi(device=device(type='cpu'), dump=0)>"
