"""The image-source room simulator without a device: properties of the numpy restatement
(tests/rirsim_ref.py) that do not need the kernel - the direct path alone, reciprocity, the prefix property - the pulse table,
``eyring_beta``, ``RoomSampler``, every validation error, and the argument checks of ``sepr_rir_ism_fwd``."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rirsim_ref as ref                                                     # noqa: E402

from sepreformer_amd import lib as L_                                        # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402

FSC = 8000.0 / 343.0
ROOM = [5.0, 4.0, 3.0, 1.1, 1.3, 1.2, 3.7, 2.9, 1.6]


def test_beta_zero_is_the_direct_pulse_alone():
    """With ``beta = 0`` every image but the source itself has weight ``bpow[n >= 1] = 0``: the sums are the interpolated pulse of the
    direct path, 81 taps around ``floor(tau0)``."""
    for room, N in ((ROOM, 400), ([5.0, 4.0, 3.0, 2.0, 2.0, 1.5, 2.1, 2.0, 1.5], 300), (ROOM, 70)):
        acc, images = ref.ism_acc(room + [0.0], FSC, N)
        want = ref.direct_pulse(room, FSC, N)
        assert np.array_equal(acc, want) and images > 1
        d = math.dist(room[3:6], room[6:9])
        i0 = int(math.floor(d * FSC))
        nz = np.nonzero(acc)[0]
        assert nz.min() >= max(0, i0 - rv.ISM_HW) and nz.max() <= min(N - 1, i0 + rv.ISM_HW)
        if N > i0 + 1:
            assert ref.peak_index(acc) in (i0, i0 + 1)
    # the pulse of a source 0.1 m from the microphone starts before t = 0 and is clipped there
    acc, _ = ref.ism_acc([5.0, 4.0, 3.0, 2.0, 2.0, 1.5, 2.1, 2.0, 1.5, 0.0], FSC, 300)
    assert acc[0] != 0 and not acc[2 + rv.ISM_HW + 1:].any()


def test_reciprocity_is_exact():
    """Exchanging source and microphone negates or keeps every image offset exactly (include/sepr.h writes the offsets so), so the squared
    offsets, the distances and the integer sums are the same bits."""
    for beta, N in ((0.5, 600), (0.9, 400)):
        a, na = ref.ism_acc(ROOM + [beta], FSC, N)
        b, nb = ref.ism_acc(ROOM[:3] + ROOM[6:9] + ROOM[3:6] + [beta], FSC, N)
        assert na == nb and np.array_equal(a, b) and np.abs(a).max() > 2 ** 40


def test_a_shorter_response_is_a_prefix():
    """An image belongs to the response iff its pulse starts at or before the last sample, so the sums of ``N' < N`` samples are the first
    ``N'`` of the sums of ``N``: tests/test_rirsim_gpu.py computes each room once, at its longest."""
    room = ROOM + [0.7]
    long, _ = ref.ism_acc(room, FSC, 517)
    for n in (1, 40, 81, 255, 256, 257):
        short, _ = ref.ism_acc(room, FSC, n)
        assert np.array_equal(short, long[:n]), n


def test_reference_table_rows():
    """A 5 x 4 x 3 m room at nominal 0.15 s: some 10^4 images, the peak is the direct path - the sample nearest ``tau0`` (71.8 here) -
    the sums stay far inside int64 and float64's integers, and the realised decay runs longer than Eyring's nominal value."""
    src, mic = [1.1, 1.3, 1.2], [3.7, 2.9, 1.6]
    tau0 = math.dist(src, mic) * FSC
    beta = rv.eyring_beta((5.0, 4.0, 3.0), 0.15)
    acc, images = ref.ism_acc([5.0, 4.0, 3.0] + src + mic + [beta], FSC, 1200)
    assert ref.peak_index(acc) == int(round(tau0)) == 72 and images > 5000
    assert 2 ** 40 < np.abs(acc).max() < 2 ** 46
    h = ref.rir_from_acc(acc, True)
    assert h.dtype == np.float32 and np.abs(h).max() == 1.0
    rt = rv.schroeder_rt60(acc.astype(np.float64), 8000)
    assert 0.15 < rt < 0.35                                                  # longer than Eyring's nominal value: documented, not gated finer


def test_ism_lut_is_the_formula():
    lut = rv.ism_lut()
    assert lut.shape == (rv.ISM_Q + 1, rv.ISM_TW) == (33, 81) and lut.dtype == np.float64 and lut.flags["C_CONTIGUOUS"]
    for k in (0, 1, 7, 16, 31, 32):
        for j in (0, 1, 39, 40, 41, 79, 80):
            x = (j - rv.ISM_HW) - k / rv.ISM_Q
            want = 0.0 if abs(x) > rv.ISM_HW + 1 else (1.0 if x == 0 else math.sin(math.pi * x) / (math.pi * x)) * 0.5 * (
                1.0 + math.cos(math.pi * x / (rv.ISM_HW + 1)))
            assert abs(lut[k, j] - want) < 1e-15, (k, j)
    assert lut[0, rv.ISM_HW] == 1.0 and np.abs(np.delete(lut[0], rv.ISM_HW)).max() < 1e-15     # sin(float64(pi) j), not 0
    assert np.allclose(lut[rv.ISM_Q, 1:], lut[0, :-1], atol=1e-3)          # one whole step later: the neighbouring tap, under a shifted window
    assert np.array_equal(lut, rv.ism_lut())


def test_eyring_beta_is_the_formula():
    for room, rt60, c in (((5.0, 4.0, 3.0), 0.3, 343.0), ((9.0, 7.5, 3.5), 0.6, 340.0), ((1.5, 1.5, 1.5), 0.2, 343.0)):
        V = room[0] * room[1] * room[2]
        S = 2 * (room[0] * room[1] + room[1] * room[2] + room[0] * room[2])
        alpha = 1 - math.exp(-24 * math.log(10) * V / (c * S * rt60))
        assert rv.eyring_beta(room, rt60, c) == pytest.approx(math.sqrt(1 - alpha), rel=1e-14)
        assert 0 < rv.eyring_beta(room, rt60, c) < 1
    assert rv.eyring_beta((5, 4, 3), 0.6) > rv.eyring_beta((5, 4, 3), 0.2)
    with pytest.raises(ValueError):
        rv.eyring_beta((5, 4, 3), 0.0)


def test_room_sampler():
    sampler = rv.RoomSampler()
    a, b, c = sampler.draw(40, seed=3), sampler.draw(40, seed=3), sampler.draw(40, seed=(3, 1))
    assert a.shape == (40, 10) and a.dtype == np.float64 and isinstance(a, np.ndarray)
    assert np.array_equal(a, b) and np.array_equal(a.rt60, b.rt60) and not np.array_equal(a, c)
    assert np.array_equal(sampler.draw(40, seed=(3, 1)), c)
    rv.validate_rooms(a)
    L, s, m = np.asarray(a[:, 0:3]), np.asarray(a[:, 3:6]), np.asarray(a[:, 6:9])
    for ax, (lo, hi) in enumerate(((5, 10), (5, 10), (3, 4))):
        assert (L[:, ax] >= lo).all() and (L[:, ax] <= hi).all()
    assert (a.rt60 >= 0.2).all() and (a.rt60 <= 0.6).all() and a.rt60.shape == (40,)
    for p in (s, m):
        assert (p[:, :2] >= 0.5).all() and (L[:, :2] - p[:, :2] >= 0.5).all()
        assert (p[:, 2] >= 0.9).all() and (p[:, 2] <= 1.8).all()
    dist = np.sqrt(((s - m) ** 2).sum(1))
    assert (dist >= 0.66 - 1e-12).all() and (dist <= 2.0 + 1e-12).all()
    for r in range(40):
        assert a[r, 9] == rv.eyring_beta(L[r], a.rt60[r])
    # every range is settable
    small = rv.RoomSampler(dims=((2, 3), (2, 3), (2.5, 2.5)), rt60=0.1, distance=(0.3, 0.5), height=(1.0, 1.2), margin=0.2, c=340.0).draw(5, seed=0)
    assert (np.asarray(small[:, :2]) <= 3).all() and (small.rt60 == 0.1).all() and (np.asarray(small[:, 2]) == 2.5).all()
    rv.validate_rooms(small)
    for kw in (dict(dims=((1.0, 2.0), (5, 10), (3, 4))), dict(rt60=(0.0, 0.3)), dict(distance=(0.05, 1.0)), dict(margin=0.05), dict(margin=2.5),
               dict(height=(0.9, 3.5)), dict(c=0.0), dict(dims=((5, 10), (5, 10)))):
        with pytest.raises(ValueError):
            rv.RoomSampler(**kw)
    with pytest.raises(ValueError):
        sampler.draw(0, seed=0)
    assert rv.parse_rooms("64") == (64, 0.2, 0.6) and rv.parse_rooms("8:0.3:0.5") == (8, 0.3, 0.5)
    with pytest.raises(ValueError):
        rv.parse_rooms("0")


def test_every_validation_error_is_raised():
    ok = np.array([ROOM + [0.5]])
    rv.validate_rooms(ok)

    def bad(col, val):
        t = ok.copy()
        t[0, col] = val
        return t

    for rooms, match in ((bad(0, 1.4), "dimension"), (bad(2, 1.0), "dimension"), (bad(3, 0.05), "source"), (bad(4, 3.95), "source"),
                         (bad(5, 3.5), "source"), (bad(6, 0.0), "microphone"), (bad(8, 2.95), "microphone"), (bad(9, 1.0), "beta"),
                         (bad(9, -0.1), "beta"), (bad(1, float("nan")), "non-finite"), (bad(9, float("inf")), "non-finite"),
                         (np.zeros((0, 10)), r"\[R >= 1, 10\]"), (np.zeros((2, 9)), r"\[R >= 1, 10\]"), (np.zeros(10), r"\[R >= 1, 10\]")):
        with pytest.raises(ValueError, match=match):
            rv.RirBank.simulate(rooms, 8000, length=100)
    close = ok.copy()
    close[0, 3:6] = close[0, 6:9] + [0.05, 0.0, 0.0]
    with pytest.raises(ValueError, match="source and microphone"):
        rv.RirBank.simulate(close, 8000, length=100)
    for length in (0, -1, 16385):
        with pytest.raises(ValueError, match="samples"):
            rv.RirBank.simulate(ok, 8000, length=length)
    with pytest.raises(ValueError, match="length is required"):
        rv.RirBank.simulate(ok, 8000)
    with pytest.raises(ValueError, match="reflection orders"):               # sqrt(3) (N + HW + 1) / fsc / Lmin + 3 >= 1024
        rv.RirBank.simulate(np.array([[1.5, 1.5, 1.5, 0.4, 0.5, 0.6, 1.1, 0.9, 1.0, 0.5]]), 4000, length=16384)
    with pytest.raises(ValueError, match="normalise"):
        rv.RirBank.simulate(ok, 8000, length=100, normalise="energy")
    with pytest.raises(ValueError, match="fs >= 1"):
        rv.RirBank.simulate(ok, 8000, length=100, c=0.0)


def test_simulate_has_no_cpu_path():
    rooms = rv.RoomSampler().draw(2, seed=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rv.RirBank.simulate(rooms, 8000, device=None)                        # the default length comes from the rooms' rt60
    with pytest.raises(RuntimeError, match="no CPU path"):
        rv.RirBank.simulate(rooms, 8000, length=64, device="cpu")
    with pytest.raises(ValueError, match="RirBank.simulate"):
        rv.RirBank.from_arrays([np.ones(4, np.float32)], 8000).resimulate(rooms)


def test_c_abi_argument_checks():
    """``sepr_rir_ism_fwd`` is exported and every check comes before any HIP call: testable without a device."""
    lib = L_.load()
    assert "sepr_rir_ism_fwd" in L_.SIGNATURES and hasattr(lib, "sepr_rir_ism_fwd")
    p = 0x1000                                                               # never dereferenced: the checks reject the call first
    E = L_.SEPR_EINVAL

    def sim(rooms=p, R=2, N=100, fsc=FSC, lut=p, acc=p, rir=p, peak=p, normalise=1):
        return lib.sepr_rir_ism_fwd(rooms, R, N, C.c_double(fsc), lut, acc, rir, peak, normalise, None)

    for kw in (dict(rooms=None), dict(lut=None), dict(acc=None), dict(rir=None), dict(peak=None), dict(R=0), dict(R=-1), dict(R=65536),
               dict(N=0), dict(N=-5), dict(N=16385), dict(normalise=2), dict(normalise=-1), dict(fsc=0.0), dict(fsc=-1.0),
               dict(fsc=float("nan")), dict(fsc=float("inf")), dict(N=16384, fsc=4000.0 / 343.0), dict(rooms=p + 4), dict(lut=p + 4),
               dict(acc=p + 4), dict(rir=p + 2), dict(peak=p + 1)):
        assert sim(**kw) == E, kw
