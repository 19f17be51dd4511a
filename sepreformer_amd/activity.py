"""Frame activity of separated tracks on the device (contracts in include/sepr.h).

A separator gives ``C`` tracks and nothing that says when each carries speech; the test loop of the long-form paths never looks at what a
channel emits while none of its talkers speaks.  This module is the measure both need:

    active, level, e = channel_activity(torch.stack(est))       # uint8 [C, nF], float64 [C], float64 [C, nF] - all on the device
    runs = segments(active, frame_samples(), T)                  # per channel [(begin_sample, end_sample), ...] after ONE copy of the mask
    write_activity_csv("meeting.csv", runs, fs=8000)

* ``frame_energy`` is one ``sepr_frame_energy_fwd`` launch for all rows: the energy of every frame in float64, in a stated order;
* ``activity_of`` is ``sepr_frame_activity_fwd``: a frame is raw-active when its energy lies above ``max(floor, level * ratio)``, ``level`` the
  loudest frame of the row, and active when a raw-active frame lies within ``hang`` frames;
* ``frame_class_sums`` is ``sepr_frame_class_sums_fwd``: per channel and class of frames, how many there are, how many are active, and the
  energies of the channel and of the mixture in them - what ``infer.evaluate_conversations(idle=True)`` reduces to its leak figures.

There is no CPU path: like every entry of the product, these run on the HIP device or raise.
"""
from __future__ import annotations

import csv
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import lib as L_


def frame_samples(fs: int = 8000, frame_ms: float = 20.0) -> int:
    """The frame of ``channel_activity``: ``round(frame_ms * fs / 1000)`` samples rounded to the nearest multiple of 4, a half upwards (the
    kernel takes 32..4096)."""
    frame = (int(round(float(frame_ms) * int(fs) / 1000.0)) + 2) // 4 * 4
    if not 32 <= frame <= 4096:
        raise ValueError(f"frame_ms = {frame_ms} at {fs} Hz is {frame} samples: the frame kernel takes a multiple of 4 in 32..4096")
    return frame


def hang_frames(frame_ms: float = 20.0, hang_ms: float = 200.0) -> int:
    """``round(hang_ms / frame_ms)`` frames, at least 0."""
    return max(0, int(round(float(hang_ms) / float(frame_ms))))


def frame_energy(x: torch.Tensor, frame: int) -> torch.Tensor:
    """One ``sepr_frame_energy_fwd`` launch: ``x`` float32 ``[rows, T]`` (or ``[T]``) on the device, with any common row stride - a view of a
    wider buffer is read in place -> float64 ``[rows, ceil(T / frame)]`` on the device, the sum of squares of every frame (the last may be
    partial).  Nothing is copied to the host."""
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or x.dtype != torch.float32 or x.device.type != "cuda" or x.shape[1] < 1:
        raise ValueError("x must be a float32 [rows, T] tensor on the HIP device (there is no CPU path)")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    rows, T = int(x.shape[0]), int(x.shape[1])
    ld = int(x.stride(0)) if rows > 1 else T
    nF = -(-T // int(frame))
    e = torch.empty(rows, nF, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        L_.check(L_.load().sepr_frame_energy_fwd(x.data_ptr(), rows, T, ld, int(frame), e.data_ptr(),
                                                 torch.cuda.current_stream(x.device).cuda_stream), "sepr_frame_energy_fwd")
    return e


def activity_of(e: torch.Tensor, ratio_db: float = -40.0, floor: float = 1e-12, hang: int = 10) -> Tuple[torch.Tensor, torch.Tensor]:
    """``sepr_frame_activity_fwd`` on frame energies ``e`` float64 ``[rows, nF]`` -> ``(active uint8 [rows, nF], level float64 [rows])`` on the
    device.  The threshold ratio ``10 ** (ratio_db / 10)`` is computed here, once, and passed as a double."""
    if e.dim() != 2 or e.dtype != torch.float64 or e.device.type != "cuda":
        raise ValueError("e must be a float64 [rows, nF] tensor on the HIP device (there is no CPU path)")
    e = e.contiguous()
    rows, nF = int(e.shape[0]), int(e.shape[1])
    lib = L_.load()
    active = torch.empty(rows, nF, dtype=torch.uint8, device=e.device)
    level = torch.empty(rows, dtype=torch.float64, device=e.device)
    ws = torch.empty(max(1, int(lib.sepr_frame_activity_bytes(rows, nF))), dtype=torch.uint8, device=e.device)
    with torch.cuda.device(e.device):
        L_.check(lib.sepr_frame_activity_fwd(e.data_ptr(), rows, nF, 10.0 ** (float(ratio_db) / 10.0), float(floor), int(hang), active.data_ptr(),
                                             level.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(e.device).cuda_stream),
                 "sepr_frame_activity_fwd")
    return active, level


def channel_activity(x: torch.Tensor, fs: int = 8000, frame_ms: float = 20.0, ratio_db: float = -40.0, floor: float = 1e-12,
                     hang_ms: float = 200.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """When does each row of ``x`` (float32 ``[rows, T]`` on the device) carry signal?  -> ``(active uint8 [rows, nF], level float64 [rows],
    e float64 [rows, nF])``, all on the device: ``frame_energy`` over frames of ``frame_samples(fs, frame_ms)`` samples, then ``activity_of``
    with ``hang = hang_frames(frame_ms, hang_ms)``.  A frame is active when a frame within ``hang`` frames of it holds more energy than
    ``max(floor, level * 10 ** (ratio_db / 10))``, ``level`` being the energy of the row's loudest frame.

    The defaults - 40 dB below the loudest frame, an absolute floor of 1e-12, 200 ms of hang-over - are conventions for a caller to change,
    not measured optima: nothing here was tuned against labelled speech."""
    e = frame_energy(x, frame_samples(fs, frame_ms))
    active, level = activity_of(e, ratio_db=ratio_db, floor=floor, hang=hang_frames(frame_ms, hang_ms))
    return active, level, e


def frame_class_sums(e_est: torch.Tensor, e_mix: torch.Tensor, active: torch.Tensor, cls: torch.Tensor, out: torch.Tensor = None
                     ) -> torch.Tensor:
    """``sepr_frame_class_sums_fwd``: ``e_est`` float64 ``[C, nF]``, ``e_mix`` float64 ``[nF]``, ``active`` and ``cls`` uint8 ``[C, nF]`` on
    the device -> float64 ``[C, 4, 4]`` on the device (into ``out`` when given): per channel and class (``cls & 3``) the number of frames,
    the number of active frames, the sum of ``e_est`` and the sum of ``e_mix``."""
    C, nF = int(e_est.shape[0]), int(e_est.shape[1])
    dev = e_est.device
    for t, dt, shape in ((e_est, torch.float64, (C, nF)), (e_mix, torch.float64, (nF,)), (active, torch.uint8, (C, nF)), (cls, torch.uint8, (C, nF))):
        if t.dtype != dt or tuple(t.shape) != shape or t.device != dev or dev.type != "cuda":
            raise ValueError(f"expected a {dt} {shape} tensor on the HIP device (there is no CPU path)")
    e_est, e_mix, active, cls = e_est.contiguous(), e_mix.contiguous(), active.contiguous(), cls.contiguous()
    if out is None:
        out = torch.empty(C, 4, 4, dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or tuple(out.shape) != (C, 4, 4) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous float64 {(C, 4, 4)} tensor on {dev}")
    lib = L_.load()
    ws = torch.empty(max(1, int(lib.sepr_frame_class_sums_bytes(C, nF))), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L_.check(lib.sepr_frame_class_sums_fwd(e_est.data_ptr(), e_mix.data_ptr(), active.data_ptr(), cls.data_ptr(), C, nF, out.data_ptr(),
                                               ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
                 "sepr_frame_class_sums_fwd")
    return out


def segments(active, frame: int, T: int) -> List[List[Tuple[int, int]]]:
    """Per row of the mask ``active`` (``[rows, nF]``, a device tensor or an array) the runs of active frames as ``(begin_sample,
    end_sample)``, the end clipped to ``T``.  A device mask is copied to the host once."""
    a = (active.detach().cpu().numpy() if isinstance(active, torch.Tensor) else np.asarray(active)) != 0
    if a.ndim == 1:
        a = a[None]
    frame, T = int(frame), int(T)
    out = []
    for row in a:
        edge = np.diff(np.concatenate([[0], row.astype(np.int8), [0]]))
        out.append([(int(b) * frame, min(int(e) * frame, T)) for b, e in zip(np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0])])
    return out


def write_activity_csv(path: str, runs: Sequence[Sequence[Tuple[int, int]]], fs: int) -> None:
    """One row per run of ``segments``: channel, begin in seconds, end in seconds - in the csv dialect of the test loops."""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh, quotechar="|", quoting=csv.QUOTE_MINIMAL)
        for c, rs in enumerate(runs):
            for b, e in rs:
                w.writerow([c, b / float(fs), e / float(fs)])
