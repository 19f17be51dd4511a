"""STOI / ESTOI without a device: the measure's 10 kHz converter table (resample.plan_oct) against scipy's resample_poly, properties of the
float64 restatement (tests/stoi_ref.py) on real speech, the conditions the device test's inputs must meet (tests/stoi_cases.py), the new
exports, the C-ABI argument checks of sepr_stoi_fwd, and the no-CPU-path rule."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy.signal import resample_poly

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as rr                                                    # noqa: E402
import stoi_cases as sc                                                      # noqa: E402
import stoi_ref as ref                                                       # noqa: E402

from sepreformer_amd import criterion as crit                                # noqa: E402
from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import resample as rs                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fs", [8000, 16000])
def test_plan_oct_table_is_resample_poly(fs, monkeypatch):
    """plan_oct's float32 table, pushed through the float64 restatement of the resample kernel, against resample_poly with the window
    of the definition.  Bound: each tap carries a relative rounding of at most 2^-24, so an output differs by at most
    2^-24 max_p sum_j |tap[p][j]| max|x| (plus float64 summation noise, 1e-13 max|x|)."""
    p = rs.plan_oct(fs, 10000)
    L_, M_ = ref.ratio(fs)
    h, Lh = ref.oct_filter(L_, M_)
    assert (p.L, p.M) == (L_, M_) and p.K % 2 == 0 and p.Hh == (p.K - 2) // 2 and p.taps.dtype == np.float32 and p.taps.shape == (p.L, p.K)
    if fs == 8000:
        assert (p.L, p.M, Lh, p.K) == (5, 4, 182, 74)
    assert np.count_nonzero(p.taps) <= 2 * Lh + 1 and abs(float(p.taps.astype(np.float64).sum()) - p.L) < 1e-5      # every tap of L h once
    monkeypatch.setattr(rr, "geometry", lambda a, b: (p.L, p.M, p.K, p.Hh, None))
    monkeypatch.setattr(rr, "taps", lambda a, b: p.taps)
    x = sc.wav()[2000:2000 + 7001].astype(np.float32)                          # odd length: the last output sits past the last input
    got = rr.resample(x, fs, 10000)
    want = resample_poly(x.astype(np.float64), L_, M_, window=h)
    assert got.shape == want.shape == (rs.out_len(len(x), p.L, p.M),)
    bound = (2.0 ** -24 * np.abs(p.taps.astype(np.float64)).sum(axis=1).max() + 1e-13) * np.abs(x).max()
    err = float(np.abs(got - want).max())
    print(f"plan_oct {fs}: max |y - resample_poly| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)


def test_restatement_properties_on_speech():
    x = sc.wav()[4000:4000 + 32000]
    assert abs(ref.stoi(x, x, 8000) - 1.0) < 1e-9 and abs(ref.stoi(x, x, 8000, extended=True) - 1.0) < 1e-9
    rng = np.random.default_rng(0)
    noise = rng.standard_normal(len(x)) * np.sqrt(np.mean(x * x))
    for ext in (False, True):
        vals = [ref.stoi(x, x + noise * 10 ** (-snr / 20), 8000, extended=ext) for snr in (20, 10, 0)]
        assert 1.0 > vals[0] > vals[1] > vals[2] > 0.0, (ext, vals)
    out = ref.evaluate(x[:2000], [x[:2000]], 8000)                              # 2500 samples at 10 kHz: 18 frames
    assert out["short"] and out["stoi"][0] == out["estoi"][0] == 1e-5 and ref.stoi(x[:2000], x[:2000], 8000) == 1e-5
    lo, hi = ref.band_edges()
    assert lo[0] == crit.STOI_BIN0 and hi[-1] == crit.STOI_BIN0 + crit.STOI_NBIN and lo[1:] == hi[:-1]


def test_device_tables_are_the_definitions_window_and_dft():
    """criterion.stoi_tables against np.hanning and np.fft.rfft on a random frame."""
    tab = crit.stoi_tables("cpu").numpy()
    assert tab.dtype == np.float64 and tab.shape == (256 + 2 * 256 * 212,)
    assert np.array_equal(tab[:256], ref.W)
    tw = tab[256:].reshape(256, 212, 2)
    f = np.random.default_rng(1).standard_normal(256)
    X = np.fft.rfft(f, n=512)[7:219]
    assert np.abs(f @ tw[:, :, 0] - X.real).max() < 1e-12 and np.abs(f @ tw[:, :, 1] + X.imag).max() < 1e-12


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_device_test_inputs_meet_their_conditions(name):
    """The inputs of tests/test_stoi_gpu.py: frames really are removed, no utterance is too short, and no frame lies within 0.01 dB of
    the keep / remove threshold (a frame that close might legitimately flip on another summation order)."""
    e = sc.expected(name)
    assert (e["kept"] < e["frames"]).all(), (e["kept"], e["frames"])
    assert not e["short"].any() and (e["kept"] - 1 >= 30).all()
    assert (e["margin"] >= 0.01).all(), e["margin"]
    for k in ("stoi", "estoi", "stoi_mix", "estoi_mix"):
        assert np.isfinite(e[k]).all() and (np.abs(e[k]) <= 1.0 + 1e-9).all()
    if name == "long_10k":
        assert (e["kept"] - 30 > 256).all()                                     # more segments than one pass of the device's walk


def test_header_and_binding_list_the_new_exports():
    hdr = open(os.path.join(ROOT, "include", "sepr.h")).read()
    declared = set(re.findall(r"\b(sepr_[a-z0-9_]+)\s*\(", hdr))
    assert {"sepr_stoi_fwd", "sepr_stoi_workspace"} <= declared and {"sepr_stoi_fwd", "sepr_stoi_workspace"} <= set(L.SIGNATURES)
    assert "DESIGN.md section 5f" in hdr
    lib = L.load()                                                             # a stale library fails here, on the missing symbol
    assert hasattr(lib, "sepr_stoi_fwd") and hasattr(lib, "sepr_stoi_workspace")
    assert L.ABI_VERSION == 413 and lib.sepr_version() == 413
    assert len(L.SIGNATURES["sepr_stoi_fwd"][1]) == 17
    mk = open(os.path.join(ROOT, "sepreformer_amd", "csrc", "Makefile")).read()
    assert "sepr_stoi.hip" in mk


def _call(S=2, B=1, T=4096, ref_p=4096, mix=4096, stoi_mix=4096, estoi_mix=4096, tables=4096, ws=4096, ws_bytes=None):
    lib = L.load()
    if ws_bytes is None:
        ws_bytes = lib.sepr_stoi_workspace(S, B, T) or 1 << 20
    p = 4096                                                                  # never dereferenced: every check comes first
    return lib.sepr_stoi_fwd(ref_p, p, mix, p, S, B, T, tables, p, p, stoi_mix, estoi_mix, p, p, ws, ws_bytes, None)


def test_abi_argument_checks():
    lib = L.load()
    assert lib.sepr_stoi_workspace(4, 1, 4096) == 0 and lib.sepr_stoi_workspace(1, 1, 4096) == 0
    assert lib.sepr_stoi_workspace(2, 0, 4096) == 0 and lib.sepr_stoi_workspace(2, 1, 255) == 0
    assert lib.sepr_stoi_workspace(2, 65535 // 8 + 1, 4096) == 0 and lib.sepr_stoi_workspace(2, 65535 // 8, 256) > 0
    frames = (40000 - 256) // 128 + 1
    assert lib.sepr_stoi_workspace(2, 1, 40000) >= 2 * 4 * 15 * frames * 8
    assert lib.sepr_stoi_workspace(2, 2, 40000) < 2 * lib.sepr_stoi_workspace(2, 1, 40000) + 4096
    assert _call(S=4) == L.SEPR_EINVAL and _call(S=1) == L.SEPR_EINVAL
    assert _call(B=0) == L.SEPR_EINVAL and _call(T=255) == L.SEPR_EINVAL
    assert _call(ref_p=None) == L.SEPR_EINVAL and _call(tables=None) == L.SEPR_EINVAL
    assert _call(mix=None) == L.SEPR_EINVAL                                     # outputs for a mixture that is not there
    assert _call(stoi_mix=None) == L.SEPR_EINVAL and _call(estoi_mix=None) == L.SEPR_EINVAL
    assert _call(ws_bytes=1024) == L.SEPR_EWORKSPACE and _call(ws=None) == L.SEPR_EWORKSPACE


def test_no_cpu_path_and_pit_rule():
    x = torch.randn(2, 1, 4096)
    with pytest.raises(RuntimeError, match="HIP device"):
        crit.stoi(x, x)
    with pytest.raises(RuntimeError, match="HIP device"):
        crit.PIT_STOI("cpu")(estims=[x[0], x[1]], mixture=x.sum(0), input_sizes=torch.tensor([4096]), target_attr=[x[1], x[0]])
    assert repr(crit.PIT_STOI("cpu", True)) == "<PIT_STOI(device=device(type='cpu'), extended=True, fs=8000)>"
    # the permutation rule, against the restatement's: first maximiser of the mean, values indexed by reference; a tie takes the identity
    v = np.array([[[0.2, 0.9], [0.8, 0.1]], [[0.5, 0.5], [0.5, 0.5]], [[0.9, 0.1], [0.3, 0.4]]])
    vm = np.array([[0.3, 0.4], [0.1, 0.2], [0.5, 0.1]])
    perm, chosen, imp = crit.stoi_pit(v, vm)
    for b in range(3):
        p, c, i = ref.pit(v[b], vm[b])
        assert list(perm[b]) == p and np.array_equal(chosen[b], c) and np.array_equal(imp[b], i)
    assert perm.tolist() == [[1, 0], [0, 1], [0, 1]]
    v3 = np.random.default_rng(2).random((4, 3, 3))
    perm, chosen, imp = crit.stoi_pit(v3, np.zeros((4, 3)))
    for b in range(4):
        assert list(perm[b]) == ref.pit(v3[b], np.zeros(3))[0]
