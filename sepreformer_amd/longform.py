"""Long-form separation: overlapping windows of the training length, batched through the separator, stitched on the device.

The models are trained on 4 s crops; a recording minutes long run as one forward leaves that regime (relative positions clamp at
``maxlen``, GroupNorm and global attention span the whole file) and runs at batch 1.  ``separate_long`` cuts each recording into
windows of ``W`` samples overlapping by ``O`` (hop ``H = W - O``), runs the windows through ``model(x)`` in batches, and puts the
outputs back together with ``sepr_stitch_fwd`` (csrc/sepr_stitch.hip): per boundary, the speaker permutation that best matches
the overlapping estimates (the sign is free: the models are trained scale-invariant), optionally a least-squares gain, and a
sin^2 crossfade.  The definitions are in DESIGN.md section 5c and include/sepr.h; tests/longform_ref.py restates them in float64.

A recording of at most ``W`` samples is one window and takes the ``separate`` path unchanged (bit-identical to it).  The
windows of one recording are never batched with another recording's, so what a recording gets does not depend on what else
is in the call.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import lib as L


def num_chunks(T: int, W: int, O: int) -> int:
    """Windows of a recording of ``T`` samples: 1 for ``T <= W``, else ``1 + ceil((T - W) / H)``."""
    H = W - O
    return 1 if T <= W else 1 + -(-(T - W) // H)


def check_geometry(W: int, O: int, stride: int = 4, kernel: int = 16) -> None:
    """Raise ``ValueError`` unless ``W`` / ``O`` are multiples of the encoder stride (and of 4), ``0 < O <= W / 2`` and
    ``W >= kernel``."""
    for name, v in (("chunk length", W), ("overlap", O)):
        if v % stride or v % 4:
            raise ValueError(f"{name} {v} samples is not a multiple of the encoder stride {stride} (and of 4)")
    if not 0 < O <= W // 2:
        raise ValueError(f"overlap {O} must satisfy 0 < overlap <= chunk / 2 = {W // 2} samples")
    if W < kernel:
        raise ValueError(f"chunk length {W} is shorter than the encoder kernel {kernel}")


def out_layout(lengths: Sequence[int], W: int, O: int, S: int) -> Tuple[List[int], List[int], int]:
    """(offset of each recording's [S, row] block in ``y``, row length of each recording, total floats of ``y``)."""
    H = W - O
    offs, rows, k = [], [], 0
    for r, T in enumerate(lengths):
        nc = num_chunks(T, W, O)
        offs.append(S * (k * H + r * O))
        rows.append(nc * H + O)
        k += nc
    return offs, rows, S * (k * H + len(lengths) * O)


def stitch(chunks: torch.Tensor, lengths: Sequence[int], O: int, match_gain: bool = False
           ) -> Tuple[List[torch.Tensor], torch.Tensor, torch.Tensor]:
    """One ``sepr_stitch_fwd`` call.  ``chunks`` [total_chunks, S, W] float32 on the device, the windows of recording r in
    order after those of recordings 0 .. r-1.  -> (per recording a [S, T_r] view of the packed output, perm [total, S] int32,
    gain [total, S] float32)."""
    if chunks.device.type != "cuda":
        raise RuntimeError("stitch runs on the HIP device only (there is no CPU path)")
    if chunks.dim() != 3 or chunks.dtype != torch.float32:
        raise ValueError("chunks must be a [total_chunks, S, W] float32 tensor")
    chunks = chunks.contiguous()
    total, S, W = chunks.shape
    R = len(lengths)
    nc = [num_chunks(int(T), W, O) for T in lengths]
    if sum(nc) != total:
        raise ValueError(f"{total} chunks given, the lengths need {sum(nc)}")
    offs, rows, ny = out_layout(lengths, W, O, S)
    lib = L.load()
    dev = chunks.device
    y = torch.empty(ny, dtype=torch.float32, device=dev)
    perm = torch.empty(total, S, dtype=torch.int32, device=dev)
    gain = torch.empty(total, S, dtype=torch.float32, device=dev)
    ws = torch.empty(max(1, lib.sepr_stitch_workspace(R, total, S)), dtype=torch.uint8, device=dev)
    coff = (C.c_int * (R + 1))(0, *[sum(nc[:r + 1]) for r in range(R)])
    lens = (C.c_int * R)(*[int(T) for T in lengths])
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        L.check(lib.sepr_stitch_fwd(chunks.data_ptr(), coff, lens, R, S, W, O, int(bool(match_gain)), y.data_ptr(),
                                    perm.data_ptr(), gain.data_ptr(), ws.data_ptr(), ws.numel(), st), "sepr_stitch_fwd")
        # coff / lens are pageable host memory that the call's copies read when they run: they must outlive the copies
        torch.cuda.current_stream(dev).synchronize()
    outs = [y[o:o + S * row].view(S, row)[:, :int(T)] for o, row, T in zip(offs, rows, lengths)]
    return outs, perm, gain


def _as_list(mixtures) -> Tuple[List[torch.Tensor], bool]:
    if isinstance(mixtures, torch.Tensor):
        if mixtures.dim() == 2 and mixtures.shape[0] == 1:
            return [mixtures[0]], True
        if mixtures.dim() == 1:
            return [mixtures], True
        raise ValueError("a tensor mixture must be [T] or [1, T]; pass several recordings as a sequence of 1-D tensors")
    xs = list(mixtures)
    for x in xs:
        if not isinstance(x, torch.Tensor) or x.dim() != 1:
            raise ValueError("every recording of the sequence must be a 1-D tensor")
    return xs, False


@torch.no_grad()
def separate_long(model, mixtures: Union[torch.Tensor, Sequence[torch.Tensor]], chunk_seconds: float = 4.0,
                  overlap_seconds: float = 1.0, fs: int = 8000, batch: int = 32, match_gain: bool = False,
                  return_plan: bool = False):
    """Separate recordings of any length by overlapping windows.

    ``mixtures``: a 1-D tensor, a ``[1, T]`` tensor, or a sequence of 1-D tensors of any lengths.  Returns, for a single
    tensor, ``num_spks`` tensors ``[T]``; for a sequence, one such list per recording - all on the model's device (the model
    is put in ``eval()``).  Window ``W = chunk_seconds * fs`` and overlap ``O = overlap_seconds * fs`` samples must be
    multiples of the encoder stride, ``0 < O <= W / 2``, ``W >= `` the encoder kernel.  A recording of at most ``W`` samples
    is ``separate(model, x)`` itself.  Longer ones: windows ``[kH, kH + W)``, the last zero-padded, through ``model(x)`` in
    batches of at most ``batch`` windows of that recording (main outputs only), then one ``sepr_stitch_fwd`` call over all
    of them.  ``match_gain`` also aligns the gain of each speaker track across boundaries (least squares on the overlap).

    ``return_plan=True`` returns ``(outputs, plan)``; ``plan``: ``stitched`` (indices of the recordings that were windowed),
    ``chunks`` [total, S, W] (the separator's window outputs), ``perm`` [total, S], ``gain`` [total, S], ``lengths``,
    ``W``, ``O``; the windows of ``stitched[q]`` come after those of ``stitched[:q]``."""
    from .infer import separate
    xs, single = _as_list(mixtures)
    cfg = model.cfg
    W, O = int(round(chunk_seconds * fs)), int(round(overlap_seconds * fs))
    check_geometry(W, O, cfg.enc_stride, cfg.enc_kernel)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    H, S = W - O, model.num_spks
    dev = next(model.parameters()).device
    model.eval()
    outs: List[Optional[List[torch.Tensor]]] = [None] * len(xs)
    long_idx = [r for r, x in enumerate(xs) if x.shape[-1] > W]
    for r, x in enumerate(xs):
        if x.shape[-1] <= W:
            outs[r] = [e[0] for e in separate(model, x[None])]
    plan: Dict[str, object] = {"stitched": long_idx, "W": W, "O": O, "lengths": [int(xs[r].shape[-1]) for r in long_idx]}
    if long_idx:
        lengths = plan["lengths"]
        ncs = [num_chunks(T, W, O) for T in lengths]
        buf = torch.empty(sum(ncs), S, W, dtype=torch.float32, device=dev)
        aux = model.compute_aux
        model.compute_aux = False                  # main outputs only: the auxiliary heads are not stitched
        try:
            k = 0
            for r, nc in zip(long_idx, ncs):
                x = xs[r].to(device=dev, dtype=torch.float32)
                xp = torch.zeros((nc - 1) * H + W, dtype=torch.float32, device=dev)
                xp[:x.shape[-1]] = x
                win = xp.unfold(0, W, H)               # [nc, W] strided view
                for b0 in range(0, nc, batch):
                    b1 = min(nc, b0 + batch)
                    audio, _ = model(win[b0:b1].contiguous())
                    for s in range(S):
                        buf[k + b0:k + b1, s].copy_(audio[s][..., :W])
                k += nc
        finally:
            model.compute_aux = aux
        ys, perm, gain = stitch(buf, lengths, O, match_gain)
        for r, y in zip(long_idx, ys):
            outs[r] = [y[s] for s in range(S)]
        plan.update(chunks=buf, perm=perm, gain=gain)
    result = outs[0] if single else outs
    return (result, plan) if return_plan else result
