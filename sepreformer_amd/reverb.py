"""Room impulse responses for the dynamic-mixing feed.

The reference's one reverberant variant reads every source's reverberant twin from disk (``models/SepReformer_Large_DM_WHAMR/dataset.py``),
so an utterance meets one room for ever.  Here a bank of impulse responses lives on the device beside the corpus (``RirBank``), the
planners of ``datafeed`` draw one per source and example, and the mixing launch convolves (``sepr_dynmix_reverb_fwd``): the mixture takes
the whole response, the target the direct path of the same response, so the two stay aligned in time.

    bank = RirBank.from_scp("rirs.scp", fs=8000, device="cuda:0")            # measured responses, or
    bank = RirBank.from_arrays(synthetic_rirs(64, 8000), 8000, device="cuda:0")
    planner = functools.partial(plan_whamr, rirs=bank)                       # target="direct" by default
    feed = DynamicMixFeed(corpus, planner, batch=16, max_len=32000, rirs=bank, fixed_length=True)
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

MAX_TAPS = 16384                                        # samples of the longest impulse response sepr_dynmix_reverb_fwd takes


class RirBank:
    """``R >= 1`` float32 impulse responses of 1 .. 16384 samples, back to back in one buffer with an int64 table ``offsets [R + 1]`` of
    cumulative sample counts; names and lengths on the host.  ``device=None`` keeps the host layout only (inspectable and usable by the
    planners, not by a launch)."""

    def __init__(self, names: Sequence[str], arrays: Sequence[np.ndarray], fs: int, device=None):
        self.names: List[str] = [str(n) for n in names]
        if not self.names:
            raise ValueError("an empty RIR bank")
        if len(set(self.names)) != len(self.names):
            raise ValueError("duplicate RIR names")
        for nm, h in zip(self.names, arrays):
            if h.ndim != 1 or h.dtype != np.float32:
                raise ValueError(f"RIR {nm}: expected a 1-D float32 array, got {h.dtype} {h.shape}")
            if h.shape[0] < 1:
                raise ValueError(f"RIR {nm}: an empty impulse response")
            if h.shape[0] > MAX_TAPS:
                raise ValueError(f"RIR {nm}: {h.shape[0]} samples, the mixing kernel takes at most {MAX_TAPS}")
            if not np.isfinite(h).all():
                raise ValueError(f"RIR {nm}: a non-finite sample")
            if not h.any():
                raise ValueError(f"RIR {nm}: an all-zero impulse response")
        self.fs = int(fs)
        self.index: Dict[str, int] = {k: i for i, k in enumerate(self.names)}
        self.lengths = np.array([int(h.shape[0]) for h in arrays], dtype=np.int64)
        self.offsets_host = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.total = int(self.offsets_host[-1])
        self.host = np.ascontiguousarray(np.concatenate(list(arrays)), dtype=np.float32)
        self._direct = self.direct_taps()
        self.device = None if device is None else torch.device(device)
        self.buf = self.offsets = None
        if self.device is not None:
            if self.device.type != "cuda" or not torch.cuda.is_available():
                raise RuntimeError("an RirBank lives on the HIP device (there is no CPU path); device=None keeps the host layout only")
            self.buf = torch.from_numpy(self.host).to(self.device)
            self.offsets = torch.from_numpy(self.offsets_host).to(self.device)

    # ---- construction ------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, arrays: Union[Dict[str, np.ndarray], Sequence[np.ndarray]], fs: int, device=None,
                    normalise: Optional[str] = "peak") -> "RirBank":
        """``arrays``: name -> 1-D float array, or a sequence of them (named "0", "1", ...).  ``normalise="peak"`` stores
        ``float32(h64 / max|h64|)``, ``None`` stores ``h`` as given."""
        if normalise not in ("peak", None):
            raise ValueError(f"normalise = {normalise!r}: 'peak' or None")
        if not isinstance(arrays, dict):
            arrays = {str(i): a for i, a in enumerate(arrays)}
        names, out = [], []
        for name, a in arrays.items():
            a = np.asarray(a)
            if a.ndim != 1 or a.dtype.kind != "f":
                raise ValueError(f"RIR {name}: expected a 1-D floating-point array, got {a.dtype} {a.shape}")
            if a.shape[0] < 1:
                raise ValueError(f"RIR {name}: an empty impulse response")
            h64 = a.astype(np.float64)
            if not np.isfinite(h64).all():
                raise ValueError(f"RIR {name}: a non-finite sample")
            if normalise == "peak":
                peak = float(np.max(np.abs(h64)))
                if peak == 0.0:
                    raise ValueError(f"RIR {name}: an all-zero impulse response")
                h64 = h64 / peak
            names.append(name)
            out.append(h64.astype(np.float32))
        return cls(names, out, fs, device=device)

    @classmethod
    def from_scp(cls, path: str, fs: int, device=None, resample: bool = False) -> "RirBank":
        """A ``key path`` list of wav files (read with ``infer.load_audio``), peak-normalised.  A file at another rate than ``fs`` raises
        unless ``resample`` is set, which converts it on the device (``resample.resample``)."""
        from .datafeed import parse_scp
        from .infer import load_audio
        arrays: Dict[str, np.ndarray] = {}
        other: Dict[int, List[str]] = {}
        for key, wav in parse_scp(path).items():
            x, sr = load_audio(wav)
            if sr != int(fs):
                if not resample:
                    raise RuntimeError(f"{wav}: sampling rate {sr} != bank rate {fs} (pass resample=True to convert it)")
                other.setdefault(sr, []).append(key)
            arrays[key] = x
        for sr, names in other.items():
            from .resample import resample as _resample
            ys = _resample([torch.from_numpy(arrays[nm]) for nm in names], sr, int(fs), device=device)
            for nm, y in zip(names, ys):
                arrays[nm] = y.cpu().numpy()
        return cls.from_arrays(arrays, fs, device=device, normalise="peak")

    # ---- what the planners read --------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return len(self.names)

    def rir(self, r: int) -> np.ndarray:
        return self.host[self.offsets_host[r]:self.offsets_host[r + 1]]

    def direct_taps(self, early_ms: float = 0.0) -> np.ndarray:
        """int32 [R]: the taps up to and including the direct path - the FIRST maximum of ``|h_r|`` - plus ``early_ms`` of early
        reflections: ``min(len_r, argmax|h_r| + 1 + round(early_ms fs / 1000))``."""
        extra = int(round(float(early_ms) * self.fs / 1000.0))
        out = [min(int(n), max(1, int(np.argmax(np.abs(self.rir(r)))) + 1 + extra)) for r, n in enumerate(self.lengths)]
        return np.array(out, dtype=np.int32)

    def _bank_args(self):
        return (self.buf.data_ptr(), self.total, self.offsets.data_ptr(), len(self.names))

    # ---- simulated rooms --------------------------------------------------------------------------
    @classmethod
    def simulate(cls, rooms, fs: int, length: Optional[int] = None, device=None, normalise: Optional[str] = "peak",
                 c: float = 343.0) -> "RirBank":
        """A bank of ``R`` shoebox-room responses simulated on the device by the image-source method (``sepr_rir_ism_fwd``): one launch, then
        one device-to-host copy that fills ``host``, ``lengths``, ``offsets`` and ``_direct``, so the planners and ``direct_taps()`` work as
        for any bank.  ``rooms``: float64 ``[R, 10]`` rows ``Lx Ly Lz sx sy sz mx my mz beta`` (``validate_rooms``), e.g. from
        ``RoomSampler.draw``.  All responses have one length: ``length``, or - when ``rooms`` carries its nominal ``rt60`` values, as a
        sampler's draw does - ``min(16384, ceil(fs max rt60))``.  ``normalise``: ``"peak"`` as ``from_arrays``, ``None`` keeps the physical
        scale ``1 / (4 pi d)``.

        ``_direct`` of a simulated bank is ``min(N, peak_idx + 1 + ISM_HW)``: the direct path is a band-limited pulse of ``2 ISM_HW + 1`` taps
        centred near the peak, so the default target (``target="direct"``) holds the WHOLE direct pulse, not its rising half.
        ``direct_taps(early_ms)`` keeps its generic meaning (up to and including the peak) for any explicit request."""
        if normalise not in ("peak", None):
            raise ValueError(f"normalise = {normalise!r}: 'peak' or None")
        table = validate_rooms(rooms)
        R = table.shape[0]
        if length is None:
            rt60 = getattr(rooms, "rt60", None)
            if rt60 is None:
                raise ValueError("length is required: these rooms carry no nominal rt60 values (RoomSampler.draw attaches them)")
            length = min(MAX_TAPS, int(math.ceil(int(fs) * float(np.max(rt60)))))
        N = int(length)
        fsc = _check_ism_size(table, int(fs), N, float(c))
        if device is None or torch.device(device).type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("an RirBank lives on the HIP device (there is no CPU path); rooms are simulated on the device only")
        self = cls.__new__(cls)
        self.names = [str(i) for i in range(R)]
        self.fs = int(fs)
        self.index = {k: i for i, k in enumerate(self.names)}
        self.lengths = np.full(R, N, dtype=np.int64)
        self.offsets_host = (np.arange(R + 1, dtype=np.int64) * N)
        self.total = R * N
        self.device = torch.device(device)
        # [R N float32 | R int32] in one allocation: the responses (buf) and the peak indices leave the device in one copy
        out = torch.zeros(R * N + R, dtype=torch.int32, device=self.device)
        self.buf = out[:R * N].view(torch.float32)
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self._sim = {"fsc": fsc, "c": float(c), "normalise": 1 if normalise == "peak" else 0, "N": N, "out": out,
                     "lut": torch.from_numpy(ism_lut()).to(self.device),
                     "rooms": torch.empty(R, 10, dtype=torch.float64, device=self.device),
                     "acc": torch.empty(R, N, dtype=torch.int64, device=self.device)}
        self.host = np.zeros(R * N, dtype=np.float32)
        self._direct = np.ones(R, dtype=np.int32)
        self._run_ism(table)
        return self

    def resimulate(self, rooms, c: Optional[float] = None) -> "RirBank":
        """Simulate ``rooms`` (as many as the bank holds) into this bank IN PLACE: ``buf.data_ptr()``, ``offsets``, ``R`` and ``N`` stay, so
        every pointer a feed or a captured launch holds remains valid; ``host`` and ``_direct`` are refreshed."""
        sim = getattr(self, "_sim", None)
        if sim is None:
            raise ValueError("resimulate needs a bank made by RirBank.simulate")
        table = validate_rooms(rooms)
        if table.shape[0] != len(self.names):
            raise ValueError(f"{table.shape[0]} rooms for a bank of {len(self.names)} responses")
        if c is not None:
            sim["c"] = float(c)
        sim["fsc"] = _check_ism_size(table, self.fs, sim["N"], sim["c"])
        self._run_ism(table)
        return self

    def _run_ism(self, table: np.ndarray) -> None:
        from . import lib as L_
        sim, R, N = self._sim, len(self.names), self._sim["N"]
        out = sim["out"]
        with torch.cuda.device(self.device):
            sim["rooms"].copy_(torch.from_numpy(table))
            # on the current stream: a mixing launch already queued there reads the old responses, one queued after this the new ones
            L_.check(L_.load().sepr_rir_ism_fwd(sim["rooms"].data_ptr(), R, N, sim["fsc"], sim["lut"].data_ptr(), sim["acc"].data_ptr(),
                                                self.buf.data_ptr(), out.data_ptr() + 4 * R * N, sim["normalise"],
                                                torch.cuda.current_stream(self.device).cuda_stream), "sepr_rir_ism_fwd")
            got = out.cpu().numpy()                                              # the one device-to-host copy
        host = np.ascontiguousarray(got[:R * N]).view(np.float32)
        peak = got[R * N:].astype(np.int64)
        if not np.isfinite(host).all():
            raise ValueError("a simulated response holds a non-finite sample")
        zero = [r for r in range(R) if not host[r * N:(r + 1) * N].any()]
        if zero:
            raise ValueError(f"room {zero[0]}: an all-zero impulse response ({N} samples end before the direct path arrives)")
        self.host = host
        self.peak_idx = peak.astype(np.int32)
        self._direct = np.minimum(N, peak + 1 + ISM_HW).astype(np.int32)
        self.rooms = table


# ---- image-source rooms -----------------------------------------------------------------------------
ISM_HW, ISM_Q, ISM_FB = 40, 32, 48
ISM_TW = 2 * ISM_HW + 1
ROOM_MIN_DIM, ROOM_MIN_GAP = 1.5, 0.1                   # metres: smallest room dimension; source / microphone to a wall and to each other
ISM_MAX_ORDER = 1024                                    # entries of the kernel's table of powers of beta


def ism_lut() -> np.ndarray:
    """float64 ``[Q + 1, TW]``: ``lut[k][j] = sinc(x) 0.5 (1 + cos(pi x / (HW + 1)))`` with ``x = (j - HW) - k / Q``, zero for
    ``|x| > HW + 1`` - a Hann-windowed sinc pulse at 33 fractional positions.  Built on the host and uploaded: the device and any
    restatement read the same bits."""
    j = np.arange(ISM_TW, dtype=np.float64)[None, :] - float(ISM_HW)
    k = np.arange(ISM_Q + 1, dtype=np.float64)[:, None] / float(ISM_Q)
    x = j - k
    out = np.sinc(x) * 0.5 * (1.0 + np.cos(np.pi * x / float(ISM_HW + 1)))
    out[np.abs(x) > float(ISM_HW + 1)] = 0.0
    return np.ascontiguousarray(out, dtype=np.float64)


def eyring_beta(room: Sequence[float], rt60: float, c: float = 343.0) -> float:
    """The wall reflection coefficient that gives a shoebox ``room = (Lx, Ly, Lz)`` the NOMINAL reverberation time ``rt60`` by Eyring's
    formula: ``alpha = 1 - exp(-24 ln10 V / (c S rt60))``, ``beta = sqrt(1 - alpha)``.  Image-source decays of a shoebox run longer than
    Eyring predicts (section 5e-4 records how much): ``rt60`` names the room, it is not measured from the response."""
    lx, ly, lz = (float(v) for v in room)
    if not (lx > 0 and ly > 0 and lz > 0 and rt60 > 0 and c > 0):
        raise ValueError("room dimensions, rt60 and c are positive")
    V, S = lx * ly * lz, 2.0 * (lx * ly + ly * lz + lx * lz)
    alpha = 1.0 - math.exp(-24.0 * math.log(10.0) * V / (c * S * rt60))
    return math.sqrt(1.0 - alpha)


class Rooms(np.ndarray):
    """A float64 ``[count, 10]`` room table that remembers the nominal ``rt60`` of every row (``RirBank.simulate`` takes its default length
    from it)."""
    rt60: Optional[np.ndarray] = None

    def __array_finalize__(self, obj):
        self.rt60 = getattr(obj, "rt60", None)


def validate_rooms(rooms) -> np.ndarray:
    """``rooms`` as a contiguous float64 ``[R, 10]`` array ``Lx Ly Lz sx sy sz mx my mz beta``, or ``ValueError``: R >= 1, finite values,
    every dimension >= 1.5 m, source and microphone >= 0.1 m from every wall and from each other, 0 <= beta < 1."""
    t = np.ascontiguousarray(np.asarray(rooms, dtype=np.float64))
    if t.ndim != 2 or t.shape[1] != 10 or t.shape[0] < 1:
        raise ValueError(f"rooms: expected a [R >= 1, 10] array, got {t.shape}")
    if not np.isfinite(t).all():
        raise ValueError("rooms: a non-finite value")
    L, s, m, beta = t[:, 0:3], t[:, 3:6], t[:, 6:9], t[:, 9]
    for r in range(t.shape[0]):
        if (L[r] < ROOM_MIN_DIM).any():
            raise ValueError(f"room {r}: a dimension below {ROOM_MIN_DIM} m")
        for what, p in (("source", s[r]), ("microphone", m[r])):
            if (p < ROOM_MIN_GAP).any() or (L[r] - p < ROOM_MIN_GAP).any():
                raise ValueError(f"room {r}: the {what} is closer than {ROOM_MIN_GAP} m to a wall (or outside the room)")
        if math.sqrt(float(np.sum((s[r] - m[r]) ** 2))) < ROOM_MIN_GAP:
            raise ValueError(f"room {r}: source and microphone are closer than {ROOM_MIN_GAP} m")
        if not (0.0 <= beta[r] < 1.0):
            raise ValueError(f"room {r}: beta = {beta[r]!r}, expected 0 <= beta < 1")
    return np.array(t, dtype=np.float64)                # a plain array of our own


def _check_ism_size(table: np.ndarray, fs: int, N: int, c: float) -> float:
    """``fsc = fs / c`` after the size checks of ``sepr_rir_ism_fwd``."""
    if fs < 1 or not (c > 0.0):
        raise ValueError("fs >= 1 and c > 0")
    if not (1 <= N <= MAX_TAPS):
        raise ValueError(f"length = {N}: 1 .. {MAX_TAPS} samples")
    fsc = float(fs) / float(c)
    # the entry bounds its table for the smallest dimension of the contract, so a table that passes for these rooms and not for a 1.5 m
    # room is refused here with the same words
    for lmin in (float(table[:, 0:3].min()), ROOM_MIN_DIM):
        if not (math.sqrt(3.0) * (N + ISM_HW + 1) / fsc / lmin + 3.0 < ISM_MAX_ORDER):
            raise ValueError(f"{N} samples at fs / c = {fsc:.3f} per metre reach reflection orders beyond {ISM_MAX_ORDER} in a room of "
                             f"{lmin} m: shorten the response")
    return fsc


class RoomSampler:
    """Random shoebox rooms for ``RirBank.simulate``.  The ranges are this project's own defaults, in the style of the rooms WHAMR was rendered
    from, not a copy of them; every one is settable.  ``dims``: (lo, hi) metres per axis; ``rt60``: nominal seconds (``eyring_beta`` turns it
    into the reflection coefficient); ``distance``: source to microphone, metres; ``height``: of source and of microphone, metres;
    ``margin``: metres kept between either and the four side walls (and, capped at what ``height`` leaves, floor and ceiling)."""

    def __init__(self, dims=((5.0, 10.0), (5.0, 10.0), (3.0, 4.0)), rt60=(0.2, 0.6), distance=(0.66, 2.0), height=(0.9, 1.8),
                 margin: float = 0.5, c: float = 343.0):
        self.dims = tuple(_range(d) for d in dims)
        self.rt60, self.distance, self.height = _range(rt60), _range(distance), _range(height)
        self.margin, self.c = float(margin), float(c)
        if len(self.dims) != 3 or any(not (ROOM_MIN_DIM <= lo <= hi) for lo, hi in self.dims):
            raise ValueError(f"dims = {dims!r}: three (lo, hi) ranges of at least {ROOM_MIN_DIM} m")
        if not (0.0 < self.rt60[0] <= self.rt60[1]):
            raise ValueError(f"rt60 = {rt60!r}: positive seconds")
        if not (ROOM_MIN_GAP <= self.distance[0] <= self.distance[1]):
            raise ValueError(f"distance = {distance!r}: at least {ROOM_MIN_GAP} m")
        if not (ROOM_MIN_GAP <= self.margin and 2.0 * self.margin < min(self.dims[0][0], self.dims[1][0])):
            raise ValueError(f"margin = {margin!r}: at least {ROOM_MIN_GAP} m and less than half the smallest floor dimension")
        if not (ROOM_MIN_GAP <= self.height[0] <= self.height[1] <= self.dims[2][0] - ROOM_MIN_GAP):
            raise ValueError(f"height = {height!r}: inside the lowest room, {ROOM_MIN_GAP} m from floor and ceiling")
        if not self.c > 0.0:
            raise ValueError("c > 0")

    def draw(self, count: int, seed) -> Rooms:
        """``count`` rooms as a float64 ``[count, 10]`` table (``.rt60``: the nominal values), from ``numpy.random.default_rng(seed)``.  Draws
        per room: Lx, Ly, Lz, rt60, the microphone (x, y, height), then - rejection sampling - a distance, an azimuth and a source height
        until the source keeps the margin and the source-to-microphone distance lies in ``distance``."""
        if count < 1:
            raise ValueError("count >= 1")
        rng = np.random.default_rng(seed)
        out, rts = np.zeros((int(count), 10), dtype=np.float64), np.zeros(int(count), dtype=np.float64)
        for r in range(int(count)):
            L = [float(rng.uniform(lo, hi)) for lo, hi in self.dims]
            rt = float(rng.uniform(*self.rt60))
            mic = [float(rng.uniform(self.margin, L[0] - self.margin)), float(rng.uniform(self.margin, L[1] - self.margin)),
                   float(rng.uniform(*self.height))]
            for _ in range(10000):
                dist, az, hz = float(rng.uniform(*self.distance)), float(rng.uniform(0.0, 2.0 * math.pi)), float(rng.uniform(*self.height))
                dz = hz - mic[2]
                if abs(dz) > dist:
                    continue
                rho = math.sqrt(dist * dist - dz * dz)
                src = [mic[0] + rho * math.cos(az), mic[1] + rho * math.sin(az), hz]
                if all(self.margin <= src[a] <= L[a] - self.margin for a in range(2)):
                    break
            else:
                raise ValueError("no source position found: the distance range does not fit the rooms")
            out[r] = L + src + mic + [eyring_beta(L, rt, self.c)]
            rts[r] = rt
        rooms = out.view(Rooms)
        rooms.rt60 = rts
        return rooms


def parse_rooms(text: str) -> Tuple[int, float, float]:
    """``"COUNT"`` or ``"COUNT:RT60LO:RT60HI"`` (``"COUNT:RT60"`` for one value) -> (count, lo, hi); without a range, ``RoomSampler``'s."""
    if ":" not in text:
        count = int(text)
        if count < 1:
            raise ValueError(f"{text!r}: COUNT >= 1")
        return count, 0.2, 0.6
    return parse_synthetic(text)


def schroeder_rt60(h: np.ndarray, fs: int, lo_db: float = -5.0, hi_db: float = -25.0) -> float:
    """The decay time of a response by Schroeder's backward integration: the time the energy decay curve takes from ``lo_db`` to ``hi_db``,
    extrapolated to 60 dB.  NaN when the response does not decay that far."""
    e = np.cumsum(np.asarray(h, dtype=np.float64)[::-1] ** 2)[::-1]
    if e[0] <= 0.0:
        return float("nan")
    with np.errstate(divide="ignore"):
        db = 10.0 * np.log10(e / e[0])
    a, b = np.nonzero(db <= lo_db)[0], np.nonzero(db <= hi_db)[0]
    if not len(a) or not len(b) or b[0] <= a[0]:
        return float("nan")
    return float(60.0 / (lo_db - hi_db) * (b[0] - a[0]) / fs)


def _range(v) -> Tuple[float, float]:
    lo, hi = (v, v) if np.isscalar(v) else v
    return float(lo), float(hi)


def synthetic_rirs(count: int, fs: int, rt60=(0.2, 0.8), drr_db=(0.0, 10.0), seed: int = 0) -> List[np.ndarray]:
    """``count`` synthetic impulse responses (float32) for tests, benches and users without a measured bank: a unit direct path
    ``h[d] = 1`` after an integer delay ``d`` in ``[0, 0.005 fs]``, followed by a Gaussian tail ``sigma g[j] 10^(-3 (j - d) / (rt60 fs))``
    (-60 dB at ``rt60`` seconds), ``sigma`` set so that the tail's EXPECTED energy is ``10^(-drr_db / 10)`` of the direct path's; the
    length is ``min(16384, d + ceil(rt60 fs))``.  ``rt60`` and ``drr_db`` are a value or a ``(lo, hi)`` range drawn uniformly.  Draws per
    response, from ``numpy.random.default_rng(seed)``: rt60, drr, d, the tail."""
    if count < 1:
        raise ValueError("count >= 1")
    rng = np.random.default_rng(seed)
    (r0, r1), (d0, d1) = _range(rt60), _range(drr_db)
    if not (0.0 < r0 <= r1):
        raise ValueError(f"rt60 = {rt60!r}: positive seconds")
    out = []
    for _ in range(int(count)):
        rt, drr = float(rng.uniform(r0, r1)), float(rng.uniform(d0, d1))
        d = int(rng.integers(0, int(0.005 * fs) + 1))
        n = min(MAX_TAPS, d + int(math.ceil(rt * fs)))
        n = max(n, d + 1)
        h = np.zeros(n, dtype=np.float64)
        h[d] = 1.0
        if n > d + 1:
            env = 10.0 ** (-3.0 * np.arange(1, n - d, dtype=np.float64) / (rt * fs))
            sigma = math.sqrt(10.0 ** (-drr / 10.0) / float(np.sum(env * env)))
            h[d + 1:] = sigma * env * rng.standard_normal(n - d - 1)
        out.append(h.astype(np.float32))
    return out


def parse_synthetic(text: str) -> Tuple[int, float, float]:
    """``"COUNT:RT60LO:RT60HI"`` (``"COUNT:RT60"`` for one value) -> (count, lo, hi)."""
    tok = text.split(":")
    if len(tok) not in (2, 3):
        raise ValueError(f"{text!r}: expected COUNT:RT60LO:RT60HI")
    count, lo = int(tok[0]), float(tok[1])
    hi = float(tok[2]) if len(tok) == 3 else lo
    if count < 1 or not (0.0 < lo <= hi):
        raise ValueError(f"{text!r}: COUNT >= 1 and 0 < RT60LO <= RT60HI")
    return count, lo, hi
