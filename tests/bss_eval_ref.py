"""Float64 restatement of mir_eval 0.7 ``bss_eval_sources`` (compute_permutation=True) in its EXPLICIT form - test
infrastructure, never imported by the package.

Follows ``mir_eval.separation``: ``_project`` (FFT correlations, Toeplitz Gram, ``np.linalg.solve``, projection by
``fftconvolve``), ``_bss_decomp_mtifilt`` (s_true, e_spat, e_interf, e_artif), ``_bss_source_crit`` (energy ratios,
``_safe_db``) and the permutation choice (first maximiser of the mean SIR in ``itertools.permutations`` order).  The device
uses the closed form of the same projections (sepreformer_amd/csrc/sepr_bsseval.hip), so agreement checks two independent
formulations.  ``pit_sdri`` restates ``PIT_SDRi.__call__`` (utils/implements/criterions.py:274-289) for one utterance.
"""
from __future__ import annotations

import itertools

import numpy as np
from scipy.linalg import toeplitz
from scipy.signal import fftconvolve

FLEN = 512


def _safe_db(num, den):
    if den == 0:
        return np.inf
    return 10 * np.log10(num / den)


def _project(reference_sources, estimated_source, flen):
    nsrc, nsampl = reference_sources.shape
    reference_sources = np.hstack((reference_sources, np.zeros((nsrc, flen - 1))))
    estimated_source = np.hstack((estimated_source, np.zeros(flen - 1)))
    n_fft = int(2 ** np.ceil(np.log2(nsampl + flen - 1.0)))
    sf = np.fft.fft(reference_sources, n=n_fft, axis=1)
    sef = np.fft.fft(estimated_source, n=n_fft)
    G = np.zeros((nsrc * flen, nsrc * flen))
    for i in range(nsrc):
        for j in range(nsrc):
            ssf = np.real(np.fft.ifft(sf[i] * np.conj(sf[j])))
            ss = toeplitz(np.hstack((ssf[0], ssf[-1:-flen:-1])), r=ssf[:flen])
            G[i * flen:(i + 1) * flen, j * flen:(j + 1) * flen] = ss
            G[j * flen:(j + 1) * flen, i * flen:(i + 1) * flen] = ss.T
    D = np.zeros(nsrc * flen)
    for i in range(nsrc):
        ssef = np.real(np.fft.ifft(sf[i] * np.conj(sef)))
        D[i * flen:(i + 1) * flen] = np.hstack((ssef[0], ssef[-1:-flen:-1]))
    C = np.linalg.solve(G, D).reshape(flen, nsrc, order="F")
    sproj = np.zeros(nsampl + flen - 1)
    for i in range(nsrc):
        sproj += fftconvolve(C[:, i], reference_sources[i])[:nsampl + flen - 1]
    return sproj


def _bss_decomp_mtifilt(reference_sources, estimated_source, j, flen):
    nsampl = estimated_source.size
    s_true = np.hstack((reference_sources[j], np.zeros(flen - 1)))
    e_spat = _project(reference_sources[j, np.newaxis, :], estimated_source, flen) - s_true
    e_interf = _project(reference_sources, estimated_source, flen) - s_true - e_spat
    e_artif = -s_true - e_spat - e_interf
    e_artif[:nsampl] += estimated_source
    return s_true, e_spat, e_interf, e_artif


def _bss_source_crit(s_true, e_spat, e_interf, e_artif):
    s_filt = s_true + e_spat
    sdr = _safe_db(np.sum(s_filt ** 2), np.sum((e_interf + e_artif) ** 2))
    sir = _safe_db(np.sum(s_filt ** 2), np.sum(e_interf ** 2))
    sar = _safe_db(np.sum((s_filt + e_interf) ** 2), np.sum(e_artif ** 2))
    return sdr, sir, sar


def validate(reference_sources, estimated_sources):
    if reference_sources.shape != estimated_sources.shape:
        raise ValueError("shapes differ")
    if np.any(np.all(reference_sources == 0, axis=1)):
        raise ValueError("All the reference sources should be non-silent (not all-zeros)")
    if np.any(np.all(estimated_sources == 0, axis=1)):
        raise ValueError("All the estimated sources should be non-silent (not all-zeros)")


def bss_eval_sources(reference_sources, estimated_sources, flen=FLEN):
    """[S,T] float arrays -> (sdr [S], sir [S], sar [S], perm [S]) indexed by reference, as mir_eval returns them."""
    ref = np.atleast_2d(np.asarray(reference_sources, dtype=np.float64))
    est = np.atleast_2d(np.asarray(estimated_sources, dtype=np.float64))
    validate(ref, est)
    nsrc = est.shape[0]
    sdr, sir, sar = (np.empty((nsrc, nsrc)) for _ in range(3))
    for jest in range(nsrc):
        for jtrue in range(nsrc):
            sdr[jest, jtrue], sir[jest, jtrue], sar[jest, jtrue] = _bss_source_crit(*_bss_decomp_mtifilt(ref, est[jest], jtrue, flen))
    perms = list(itertools.permutations(list(range(nsrc))))
    mean_sir = np.empty(len(perms))
    dum = np.arange(nsrc)
    for i, perm in enumerate(perms):
        mean_sir[i] = np.mean(sir[perm, dum])
    popt = perms[np.argmax(mean_sir)]
    idx = (popt, dum)
    return sdr[idx], sir[idx], sar[idx], np.asarray(popt)


def pit_sdri(targets, estims, mixture):
    """PIT_SDRi.__call__ for one utterance: targets / estims [S,T], mixture [T] -> (sum of SDRi, SDRi [S]) (num_utts = 1).
    The mixture is repeated S times (the reference concatenates it twice, i.e. S = 2)."""
    targets, estims = np.asarray(targets, np.float64), np.asarray(estims, np.float64)
    inp = np.stack([np.asarray(mixture, np.float64)] * targets.shape[0])
    out = bss_eval_sources(targets, estims)[0]
    inn = bss_eval_sources(targets, inp)[0]
    return np.sum(out - inn) / 1, out - inn
