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
