"""Sample-rate conversion on the device: recordings at any rate in, the model's rate out (and back).

The reference loads every file with ``librosa.load(path, sr=fs)`` (``engine.py:155``), which resamples on the host.  Here the
conversion is one HIP launch (``csrc/sepr_resample.hip``): rational ratio ``L / M``, Kaiser-windowed sinc, one tap row per
output phase, float64 accumulation of exact products, one rounding to float32.  The definitions are in DESIGN.md section 5d
and include/sepr.h; tests/resample_ref.py restates them in float64.  The filter is this project's own: it does not reproduce
soxr (librosa's default converter) sample for sample.

``plan`` is host arithmetic (numpy float64) and needs no device; ``resample`` runs on the HIP device only.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, NamedTuple, Sequence, Tuple, Union

import numpy as np
import torch

from . import lib as L_

ZEROS = 64          # zero crossings of the sinc per side
ROLLOFF = 0.945     # cut-off as a fraction of the lower Nyquist frequency
BETA = 12.0         # Kaiser window parameter
MAX_CONVERTERS = 16                     # converters one launch takes: sepr_dynmix_speed_fwd, sepr_streambank_convert (csrc/sepr_polyphase.h)
SPAN_TILE, SPAN_BYTES = 256, 64 * 1024  # sepr_resample_fwd's and sepr_streambank_convert's tile of outputs and the LDS its input span must fit


class Plan(NamedTuple):
    L: int              # fs_out / gcd
    M: int              # fs_in / gcd
    K: int              # taps per phase, 2 Hh + 2
    Hh: int             # ceil(ZEROS / s), s = min(1, L / M)
    taps: np.ndarray    # float32 [L][K]


def geometry(fs_in: int, fs_out: int) -> Tuple[int, int, int, int]:
    """``(L, M, K, Hh)`` of the converter ``fs_in -> fs_out``: ``plan`` without the table."""
    fs_in, fs_out = int(fs_in), int(fs_out)
    if fs_in < 1 or fs_out < 1:
        raise ValueError(f"sampling rates must be positive, got {fs_in} -> {fs_out}")
    g = math.gcd(fs_in, fs_out)
    L, M = fs_out // g, fs_in // g
    Hh = -((-ZEROS * max(L, M)) // L)               # ceil(Z / s) in integers: Z max(1, M / L)
    return L, M, 2 * Hh + 2, Hh


def span_fits(L: int, M: int, K: int, tile: int = SPAN_TILE, lds_bytes: int = SPAN_BYTES) -> bool:
    """Whether the input span of a tile of ``tile`` outputs, ``(tile - 1) M / L + K + 1`` doubles with the tap row of an ``L = 1``
    converter beside it, fits ``lds_bytes``: the ratio limit of ``sepr_resample_fwd`` and ``sepr_streambank_convert``."""
    return ((tile - 1) * M // L + K + 1 + (K if L == 1 else 0)) * 8 <= lds_bytes


def plan(fs_in: int, fs_out: int) -> Plan:
    """``(L, M, K, Hh, taps)`` of the converter ``fs_in -> fs_out``: ``taps[p][j] = rolloff s sinc(rolloff u) kaiser(u / Z)`` at
    ``u = (p / L + Hh - j) s``, zero for ``|u| >= Z``; float64 arithmetic rounded once to float32."""
    L, M, K, Hh = geometry(fs_in, fs_out)
    s = min(1.0, L / M)
    p = np.arange(L, dtype=np.float64)[:, None]
    j = np.arange(K, dtype=np.float64)[None, :]
    u = (p / L + Hh - j) * s
    inside = np.abs(u) < ZEROS
    w = np.i0(BETA * np.sqrt(np.where(inside, 1.0 - (u / ZEROS) ** 2, 0.0))) / np.i0(BETA)
    taps = np.where(inside, ROLLOFF * s * np.sinc(ROLLOFF * u) * w, 0.0)
    return Plan(L, M, K, Hh, taps.astype(np.float32))


def plan_oct(fs_in: int, fs_out: int = 10000) -> Plan:
    """The converter STOI prescribes (pystoi's ``resample_oct``), in the ``[L][K]`` phase layout of ``plan``: half
    length ``Lh = ceil((60 - 8) / (28.714 fc / 10))`` at ``fc = 1 / (2 max(L, M))``, ``h[t] = kaiser(2 Lh + 1, 0.1102 (60 - 8.7))[t]
    2 L fc sinc(2 fc t)`` normalised to unit sum, applied as ``scipy.signal.resample_poly(x, L, M, window=h)``: a centred filter of gain
    ``L``.  Output ``n`` at ``n M = b L + p`` is ``sum_r L h[p + L r] x[b - r]``, so ``taps[p][j] = L h[p + L (Hh - j)]`` with
    ``Hh = floor(Lh / L)`` and ``K = 2 Hh + 2`` (zero where ``|p + L (Hh - j)| > Lh``); float64 arithmetic rounded once to float32.
    ``sepr_resample_fwd`` runs it like any other plan."""
    L, M, _, _ = geometry(fs_in, fs_out)                # the ratio; the half length is this filter's own
    fc = 1.0 / (2 * max(L, M))
    Lh = int(math.ceil((60 - 8) / (28.714 * fc / 10)))
    t = np.arange(-Lh, Lh + 1, dtype=np.float64)
    h = np.kaiser(2 * Lh + 1, 0.1102 * (60 - 8.7)) * (2 * L * fc * np.sinc(2 * fc * t))
    h = L * (h / np.sum(h))
    Hh = Lh // L
    K = 2 * Hh + 2
    pos = np.arange(L, dtype=np.int64)[:, None] + L * (Hh - np.arange(K, dtype=np.int64))[None, :]      # p + L (Hh - j)
    inside = np.abs(pos) <= Lh
    taps = np.where(inside, h[np.clip(pos + Lh, 0, 2 * Lh)], 0.0)
    return Plan(L, M, K, Hh, taps.astype(np.float32))


def out_len(T: int, L: int, M: int) -> int:
    """``ceil(T L / M)``: the length ``librosa.resample`` gives."""
    return -((-int(T) * L) // M)


def device_table(p: Plan) -> np.ndarray:
    """The table in the kernel's layout: float32 ``[K][L]``, column ``q`` = the tap row of phase ``(q M) mod L`` - output ``n``
    reads column ``n mod L``, so consecutive lanes read consecutive floats."""
    q = (np.arange(p.L, dtype=np.int64) * p.M) % p.L
    return np.ascontiguousarray(p.taps[q].T)


def converter_args(tables: Sequence[Tuple[Plan, torch.Tensor]]):
    """``(conv_taps, conv_L, conv_M, conv_K, NC)`` of a launch that takes a converter set (include/sepr.h) from ``(plan, device table)``
    pairs: ctypes arrays, of one element when the set is empty."""
    NC = len(tables)
    if NC > MAX_CONVERTERS:
        raise ValueError(f"{NC} converters: one launch takes {MAX_CONVERTERS}")
    ints = [(C.c_int * max(NC, 1))(*[getattr(p, f) for p, _ in tables]) for f in ("L", "M", "K")]
    return ((C.c_void_p * max(NC, 1))(*[t.data_ptr() for _, t in tables]), *ints, NC)


_tables: Dict[Tuple[int, int, str, bool], Tuple[Plan, torch.Tensor]] = {}


def _table(fs_in: int, fs_out: int, dev: torch.device, oct: bool = False) -> Tuple[Plan, torch.Tensor]:
    key = (int(fs_in), int(fs_out), str(dev), oct)
    if key not in _tables:
        p = plan_oct(fs_in, fs_out) if oct else plan(fs_in, fs_out)
        _tables[key] = (p, torch.from_numpy(device_table(p)).to(dev))
    return _tables[key]


def _as_list(x) -> Tuple[List[torch.Tensor], int]:
    """-> (1-D tensors, form): form 1 = a 1-D tensor, 2 = a [1, T] tensor, 0 = a sequence."""
    if isinstance(x, torch.Tensor):
        if x.dim() == 1:
            return [x], 1
        if x.dim() == 2 and x.shape[0] == 1:
            return [x[0]], 2
        raise ValueError("a tensor must be [T] or [1, T]; pass several recordings as a sequence of 1-D tensors")
    xs = list(x)
    for v in xs:
        if not isinstance(v, torch.Tensor) or v.dim() != 1:
            raise ValueError("every recording of the sequence must be a 1-D tensor")
    return xs, 0


@torch.no_grad()
def resample(x: Union[torch.Tensor, Sequence[torch.Tensor]], fs_in: int, fs_out: int, device=None):
    """Convert recordings from ``fs_in`` to ``fs_out`` on the device.

    ``x``: a 1-D tensor, a ``[1, T]`` tensor, or a sequence of 1-D tensors of any lengths (each at least one sample).  Returns
    float32 device tensors of ``ceil(T fs_out / fs_in)`` samples in the same form (a list for a sequence); all recordings of a
    call share one launch, and a recording's result does not depend on the others.  ``fs_in == fs_out`` returns ``x`` itself.
    Tensors already on a HIP device stay there; CPU tensors are copied to ``device`` (default ``cuda:0``) - without a HIP
    device this raises: there is no CPU path."""
    if int(fs_in) == int(fs_out):
        return x
    xs, form = _as_list(x)
    if not xs:
        return []
    dev = next((v.device for v in xs if v.device.type == "cuda"), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("resample runs on the HIP device only (there is no CPU path)")
        dev = torch.device(device if device is not None else "cuda:0")
    if dev.type != "cuda":
        raise RuntimeError("resample runs on the HIP device only (there is no CPU path)")
    for v in xs:
        if v.shape[0] < 1:
            raise ValueError("every recording must hold at least one sample")
    p, table = _table(fs_in, fs_out, dev)
    parts = _convert(xs, p, table, dev)
    if form == 1:
        return parts[0]
    if form == 2:
        return parts[0][None]
    return parts


@torch.no_grad()
def resample_oct(xs: Sequence[torch.Tensor], fs_in: int, fs_out: int = 10000) -> List[torch.Tensor]:
    """1-D device tensors through the ``plan_oct`` converter (STOI's 10 kHz conversion), all in one launch -> a list of float32 device
    tensors of ``ceil(T fs_out / fs_in)`` samples.  ``fs_in == fs_out`` returns the tensors themselves."""
    xs = list(xs)
    if int(fs_in) == int(fs_out) or not xs:
        return xs
    dev = xs[0].device
    if dev.type != "cuda":
        raise RuntimeError("resample runs on the HIP device only (there is no CPU path)")
    p, table = _table(fs_in, fs_out, dev, oct=True)
    return _convert(xs, p, table, dev)


def _convert(xs: List[torch.Tensor], p: Plan, table: torch.Tensor, dev: torch.device) -> List[torch.Tensor]:
    """One ``sepr_resample_fwd`` launch over the 1-D tensors ``xs`` with the plan's table."""
    lib = L_.load()
    xs = [v.to(device=dev, dtype=torch.float32) for v in xs]
    R = len(xs)
    if lib.sepr_resample_workspace(R) == 0:
        raise ValueError(f"{R} recordings in one call: more than the kernel's grid takes")
    lens = [int(v.shape[0]) for v in xs]
    outs = [out_len(T, p.L, p.M) for T in lens]
    xin = xs[0].contiguous() if R == 1 else torch.cat(xs)
    y = torch.empty(sum(outs), dtype=torch.float32, device=dev)
    ioff = (C.c_longlong * (R + 1))(0, *np.cumsum(lens).tolist())
    ooff = (C.c_longlong * (R + 1))(0, *np.cumsum(outs).tolist())
    ws = torch.empty(lib.sepr_resample_workspace(R), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        L_.check(lib.sepr_resample_fwd(xin.data_ptr(), ioff, y.data_ptr(), ooff, R, table.data_ptr(), p.L, p.M, p.K, ws.data_ptr(),
                                       ws.numel(), stream.cuda_stream), "sepr_resample_fwd")
        # the offsets are pageable host memory that the call's copies read when they run: they must outlive the copies
        stream.synchronize()
    return [y[int(ooff[r]):int(ooff[r + 1])] for r in range(R)]
