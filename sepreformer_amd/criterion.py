"""Device-side permutation-invariant SI-SNR criteria behind the reference's criterion call surface.

Mirrors ``utils/implements/criterions.py`` of the reference:

* ``PIT_SISNR_time(device, num_spks, scale_inv)(estims=..., input_sizes=..., target_attr=...)`` -> scalar loss
  (reference :180-217, called by ``engine.py:70,103``);
* ``PIT_SISNRi(device, num_spks, scale_inv)(estims=..., mixture=..., input_sizes=..., target_attr=..., eps=...)``
  -> ``(mean summed improvement, per-speaker improvements)`` (reference :220-260, called by ``engine.py:131``).
* ``PIT_SDRi(device, dump)(estims=..., mixture=..., input_sizes=..., target_attr=...)`` -> ``(sum of SDRi / num_utts, SDRi per
  reference)`` (reference :264-289, called by ``engine.py:133``) on ``bss_eval_sources``, mir_eval's BSS-eval in float64 on the
  device (``csrc/sepr_bsseval.hip`` through ``sepr_bss_eval_fwd``; the CPU restatement is ``tests/bss_eval_ref.py``).
* ``PIT_STOI(device, extended)`` with the same call surface -> the STOI / ESTOI improvement over the mixture (beyond the reference;
  ``csrc/sepr_stoi.hip`` through ``sepr_stoi_fwd``; the CPU restatement is ``tests/stoi_ref.py``).

``estims`` / ``target_attr`` are lists of ``[B,T]`` tensors (or one ``[S,B,T]`` tensor) on the HIP device.  The
arithmetic is one pass over the waveforms in ``csrc/sepr_criterion.hip`` through ``sepr_pit_sisnr_fwd``; there is no
CPU implementation here (the CPU restatement is ``oracle/criterion_oracle.py``, test infrastructure).

Training: when an estimate requires grad, ``PIT_SISNR_time`` / ``PIT_SISNR_mag`` return an
autograd-connected scalar; their backward is ``sepr_pit_sisnr_bwd`` / ``sepr_pit_sisnr_mag_bwd`` (closed form from the same
moments; the STFT adjoint is one more projection with the transposed DFT kernel), the permutation chosen in the forward
is held fixed, as ``torch.min`` does in the reference.

Beyond the reference: ``PIT_SASDR_time`` / ``PIT_SASDR_mag``, the source-aggregated, soft-thresholded SDR with the
siblings' call surface, defined - value and gradient - when a target is silent throughout (``sepr_pit_sasdr_fwd/_bwd``,
``sepr_pit_sasdr_mag_fwd/_bwd``; the CPU restatement is ``tests/sasdr_ref.py``).
"""
from __future__ import annotations

from typing import List, Sequence, Union

import torch

from . import lib as L

_TensorList = Union[torch.Tensor, Sequence[torch.Tensor]]


def _needs_grad(x: _TensorList) -> bool:
    if not torch.is_grad_enabled():
        return False
    return x.requires_grad if isinstance(x, torch.Tensor) else any(t.requires_grad for t in x)


def _stack_g(x: _TensorList) -> torch.Tensor:
    """Stack keeping the autograd graph (the training criteria differentiate through this)."""
    t = x if isinstance(x, torch.Tensor) else torch.stack(list(x), dim=0)
    return t.to(torch.float32).contiguous()


def _pit_time_bytes(lib, S: int, B: int, T: int) -> int:
    return lib.sepr_workspace_bytes(L.OP_PIT, B, T, 0, 0, 0, S)


def _pit_time_bwd_bytes(lib, S: int, B: int, T: int, *_) -> int:
    """Workspace of ``sepr_pit_sisnr_bwd`` / ``sepr_pit_sasdr_bwd``.  Mirrors ``PitWs(..., bwd = true)`` of csrc/sepr_criterion.hip: the forward's
    partial moments, then four float32 coefficients per (utterance, source), and room for the alignment of the two."""
    return _pit_time_bytes(lib, S, B, T) + 16 * B * S + 512


def _mag_bwd_bytes(lib, S: int, B: int, T: int, frame_len: int, frame_shift: int, *_) -> int:
    return lib.sepr_pit_sisnr_mag_bwd_workspace(S, B, T, frame_len, frame_shift)


def _pit_function(name: str, doc: str, forward, perm_key: str, bwd_entry: str, bwd_bytes):
    """The autograd Function of one training criterion: ``apply(est, tgt, *consts)`` -> per-utterance loss ``[B]``, with ``consts`` the
    criterion's constant tensors (the DFT kernels) followed by its scalars.  ``forward(est, tgt, *consts)`` is the functional wrapper's dict,
    whose ``perm_key`` is held fixed in the backward; the backward is the C entry ``bwd_entry(est, tgt, perm, gl, S, B, T, *consts, dest, ws,
    ws_bytes, stream)`` on a workspace of ``bwd_bytes(lib, S, B, T, *scalars)`` bytes."""

    def fwd(ctx, est, tgt, *consts):
        out = forward(est, tgt, *consts)
        ctx.save_for_backward(est, tgt, out[perm_key], *(c for c in consts if isinstance(c, torch.Tensor)))
        ctx.scalars = tuple(c for c in consts if not isinstance(c, torch.Tensor))
        return out["loss"]

    def bwd(ctx, gl):
        est, tgt, perm, *tensors = ctx.saved_tensors
        S, B, T = est.shape
        lib = L.load()
        with torch.cuda.device(est.device):
            ws = torch.empty(bwd_bytes(lib, S, B, T, *ctx.scalars), dtype=torch.uint8, device=est.device)
            dest = torch.empty_like(est)
            glc = gl.detach().to(torch.float32).contiguous()
            L.check(getattr(lib, bwd_entry)(est.data_ptr(), tgt.data_ptr(), perm.data_ptr(), glc.data_ptr(), S, B, T,
                                            *(t.data_ptr() for t in tensors), *ctx.scalars, dest.data_ptr(), ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream(est.device).cuda_stream), bwd_entry)
        return (dest,) + (None,) * (1 + len(tensors) + len(ctx.scalars))

    return type(name, (torch.autograd.Function,), {"__doc__": doc, "__module__": __name__, "forward": staticmethod(fwd),
                                                   "backward": staticmethod(bwd)})


_PitTimeFn = _pit_function(
    "_PitTimeFn", "sum_b w_b * loss_b of PIT_SISNR_time with d/d est from sepr_pit_sisnr_bwd (criterions.py:191-217): apply(est, tgt, eps, clamp_min).",
    lambda est, tgt, eps, clamp_min: pit_sisnr(est, tgt, eps_loss=eps, clamp_min=clamp_min), "loss_perm", "sepr_pit_sisnr_bwd", _pit_time_bwd_bytes)
_PitMagFn = _pit_function(
    "_PitMagFn", "Per-utterance PIT_SISNR_mag loss with d/d est from sepr_pit_sisnr_mag_bwd (criterions.py:148-176): "
    "apply(est, tgt, dft, dft_t, frame_len, frame_shift, eps).",
    lambda est, tgt, dft, dft_t, *c: pit_sisnr_mag(est, tgt, dft, *c), "perm", "sepr_pit_sisnr_mag_bwd", _mag_bwd_bytes)
_SaSdrTimeFn = _pit_function(
    "_SaSdrTimeFn", "Per-utterance PIT_SASDR_time loss with d/d est from sepr_pit_sasdr_bwd (DESIGN.md section 5e-7): apply(est, tgt, eps, snr_max).",
    lambda est, tgt, eps, snr_max: pit_sasdr(est, tgt, eps=eps, snr_max=snr_max), "perm", "sepr_pit_sasdr_bwd", _pit_time_bwd_bytes)
_SaSdrMagFn = _pit_function(
    "_SaSdrMagFn", "Per-utterance PIT_SASDR_mag loss with d/d est from sepr_pit_sasdr_mag_bwd (DESIGN.md section 5e-7): "
    "apply(est, tgt, dft, dft_t, frame_len, frame_shift, eps, snr_max).",
    lambda est, tgt, dft, dft_t, *c: pit_sasdr_mag(est, tgt, dft, *c), "perm", "sepr_pit_sasdr_mag_bwd", _mag_bwd_bytes)


def _stack(x: _TensorList, what: str) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.stack(list(x), dim=0)
    if t.dim() != 3:
        raise RuntimeError(f"{what}: expected num_spks tensors of shape [batch, samples]")
    if not t.is_cuda:
        raise RuntimeError(f"{what} is not on the HIP device (no CPU fallback exists)")
    return t.detach().to(torch.float32).contiguous()


def _pit_call(entry: str, what: str, estims: _TensorList, targets: _TensorList, nbytes, consts: tuple, takes_mix: bool = False, mixture=None):
    """One forward entry over ``[S,B,T]`` estimates / targets: ``entry(est, tgt, [mix,] S, B, T, *consts, loss, perm, [sisnri, sisnri_perm,]
    ws, ws_bytes, stream)`` on a workspace of ``nbytes(lib, S, B, T)`` bytes (0: the problem is not supported); the bracketed arguments are those
    of an entry that ``takes_mix``, null without a ``mixture`` ``[B,T]``.  Returns ``(loss [B], perm [B,S], sisnri, sisnri_perm)``,
    the last two ``None`` without a mixture."""
    est, tgt = _stack(estims, "estims"), _stack(targets, "target_attr")
    if est.shape != tgt.shape:
        raise RuntimeError(f"estims {tuple(est.shape)} and targets {tuple(tgt.shape)} differ")
    S, B, T = est.shape
    dev = est.device
    mix = None
    if mixture is not None:
        mix = mixture.detach().to(torch.float32).contiguous()
        if tuple(mix.shape) != (B, T) or mix.device != dev:
            raise RuntimeError("mixture must be [batch, samples] on the same device as the estimates")
    ptr = lambda t: None if t is None else t.data_ptr()
    lib = L.load()
    with torch.cuda.device(dev):
        n = nbytes(lib, S, B, T)
        if n == 0:
            raise RuntimeError(f"unsupported {what} problem: num_spks={S}, batch={B}, samples={T}")
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        perm = torch.empty(B, S, dtype=torch.int32, device=dev)
        sisnri = torch.empty(B, S, dtype=torch.float32, device=dev) if mix is not None else None
        sisnri_perm = torch.empty(B, S, dtype=torch.int32, device=dev) if mix is not None else None
        L.check(getattr(lib, entry)(est.data_ptr(), tgt.data_ptr(), *((ptr(mix),) if takes_mix else ()), S, B, T, *consts, loss.data_ptr(),
                                    perm.data_ptr(), *((ptr(sisnri), ptr(sisnri_perm)) if takes_mix else ()), ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream(dev).cuda_stream), entry)
    return loss, perm, sisnri, sisnri_perm


def pit_sisnr(estims: _TensorList, targets: _TensorList, mixture: torch.Tensor = None, eps_loss: float = 1.0e-8,
              eps_i: float = 1.0e-15, clamp_min: float = -30.0):
    """One launch pair over ``[S,B,T]`` estimates / targets.  Returns a dict with ``loss`` ``[B]`` (PIT_SISNR_time per
    utterance), ``loss_perm`` ``[B,S]`` and, when ``mixture`` is given, ``sisnri`` ``[B,S]`` / ``sisnri_perm`` ``[B,S]``."""
    loss, loss_perm, sisnri, sisnri_perm = _pit_call("sepr_pit_sisnr_fwd", "PIT", estims, targets, _pit_time_bytes,
                                                     (eps_loss, eps_i, clamp_min), takes_mix=True, mixture=mixture)
    return {"loss": loss, "loss_perm": loss_perm, "sisnri": sisnri, "sisnri_perm": sisnri_perm}


def stft_kernel(frame_len: int, frame_hop: int, window: str = "hann") -> torch.Tensor:
    """The reference's conv-STFT kernel (``STFTBase._init_kernel``, criterions.py:43-61) as a ``[frame_len + 2 (padded to
    a multiple of 4), frame_len]`` matrix: windowed, scaled real DFT rows, then imaginary rows, then zero rows.  A
    constant of the criterion (built on the host once, like the reference does in ``__post_init__``)."""
    if window != "hann":
        raise NotImplementedError("only the 'hann' window is configured by the reference")
    N = frame_len
    W = torch.hann_window(frame_len)
    if N // 4 == frame_hop:
        W = (2 / 3) ** 0.5 * W
    elif N // 2 == frame_hop:
        W = W ** 0.5
    S = 0.5 * (N * N / frame_hop) ** 0.5
    K = torch.fft.rfft(torch.eye(N) / S, dim=1)[:frame_len]                 # [N, N/2+1]
    K = torch.stack((torch.real(K), torch.imag(K)), dim=2)                  # [N, N/2+1, 2]
    K = torch.transpose(K, 0, 2) * W                                         # [2, N/2+1, N]
    K = torch.reshape(K, (N + 2, frame_len))
    pad = (-(N + 2)) % 4
    return torch.cat([K, torch.zeros(pad, frame_len)], 0).to(torch.float32).contiguous()


def _mag_bytes(frame_len: int, frame_shift: int):
    return lambda lib, S, B, T: lib.sepr_pit_sisnr_mag_workspace(S, B, T, frame_len, frame_shift)


def pit_sisnr_mag(estims: _TensorList, targets: _TensorList, dft: torch.Tensor, frame_len: int, frame_shift: int,
                  eps: float = 1.0e-12):
    """Per-utterance PIT_SISNR_mag loss ``[B]`` and its permutation ``[B,S]`` (one moment pass, one f32-MFMA STFT
    projection over all 2S waveforms, one pair-sum pass)."""
    loss, perm, _, _ = _pit_call("sepr_pit_sisnr_mag_fwd", "PIT_SISNR_mag", estims, targets, _mag_bytes(frame_len, frame_shift),
                                 (dft.data_ptr(), frame_len, frame_shift, eps))
    return {"loss": loss, "perm": perm}


def pit_sasdr(estims: _TensorList, targets: _TensorList, eps: float = 1.0e-8, snr_max: float = 30.0):
    """Source-aggregated, soft-thresholded SDR over ``[S,B,T]`` estimates / targets: ``loss`` ``[B]`` =
    ``min_p 10 log10((E_p + tau D + eps) / (D + eps))`` and ``perm`` ``[B,S]``, the first minimiser of ``E_p``.  Defined for silent targets.
    ``sepr_pit_sasdr_fwd``: the moment pass of ``pit_sisnr`` and one finalising launch."""
    loss, perm, _, _ = _pit_call("sepr_pit_sasdr_fwd", "PIT", estims, targets, _pit_time_bytes, (eps, snr_max))
    return {"loss": loss, "perm": perm}


def pit_sasdr_mag(estims: _TensorList, targets: _TensorList, dft: torch.Tensor, frame_len: int, frame_shift: int,
                  eps: float = 1.0e-12, snr_max: float = 30.0):
    """``pit_sasdr`` on the STFT magnitudes of the zero-mean signals (the projection and the pair sums of ``pit_sisnr_mag`` with unit
    target scales): ``loss`` ``[B]`` and ``perm`` ``[B,S]``.  ``sepr_pit_sasdr_mag_fwd``."""
    loss, perm, _, _ = _pit_call("sepr_pit_sasdr_mag_fwd", "PIT_SASDR_mag", estims, targets, _mag_bytes(frame_len, frame_shift),
                                 (dft.data_ptr(), frame_len, frame_shift, eps, snr_max))
    return {"loss": loss, "perm": perm}


class _Base:
    def __init__(self, device, num_spks: int, scale_inv: bool = True):
        if not scale_inv:
            raise NotImplementedError("only the scale-invariant form is built (scale_inv: true in every shipped config)")
        self.device, self.num_spks, self.scale_inv = torch.device(device), num_spks, scale_inv

    def __repr__(self):
        return f"<{type(self).__name__}(device={self.device!r}, num_spks={self.num_spks!r}, scale_inv={self.scale_inv!r})>"

    def _check(self, estims):
        n = estims.shape[0] if isinstance(estims, torch.Tensor) else len(estims)
        if n != self.num_spks:
            raise RuntimeError(f"expected {self.num_spks} estimates, got {n}")


class PIT_SISNR_time(_Base):
    def __call__(self, **kwargs) -> torch.Tensor:
        estims, targets = kwargs["estims"], kwargs["target_attr"]
        self._check(estims)
        if _needs_grad(estims):                                                   # training: autograd-connected (engine.py:70,75)
            loss = _PitTimeFn.apply(_stack_g(estims), _stack(targets, "target_attr"), 1.0e-8, -30.0)
            return torch.sum(loss) / kwargs["input_sizes"].shape[0]
        out = pit_sisnr(estims, targets)
        return torch.sum(out["loss"]) / kwargs["input_sizes"].shape[0]           # reference :216-217


class PIT_SISNRi(_Base):
    def __call__(self, **kwargs):
        estims, targets = kwargs["estims"], kwargs["target_attr"]
        self._check(estims)
        out = pit_sisnr(estims, targets, mixture=kwargs["mixture"], eps_i=kwargs["eps"])
        per = out["sisnri"]
        mean = torch.sum(per) / kwargs["input_sizes"].shape[0]                    # reference :255-257
        return mean, (per[0] if per.shape[0] == 1 else per)


class PIT_SISNR_mag:
    """``PIT_SISNR_mag(device, frame_length, frame_shift, window, num_stages, num_spks, scale_inv, mel_opt)`` of the
    reference (criterions.py:117-176): ``__call__(estims=..., idx=..., input_sizes=..., target_attr=...)`` -> scalar loss.
    ``idx`` selects one of ``num_stages`` identical STFT layers in the reference; there is one kernel matrix here."""

    def __init__(self, device, frame_length: int, frame_shift: int, window: str, num_stages: int, num_spks: int,
                 scale_inv: bool = True, mel_opt: bool = False):
        if not scale_inv or mel_opt:
            raise NotImplementedError("only scale_inv=True, mel_opt=False (what every shipped config uses) is built")
        self.device = torch.device(device)
        self.frame_length, self.frame_shift, self.window = frame_length, frame_shift, window
        self.num_stages, self.num_spks, self.scale_inv, self.mel_opt = num_stages, num_spks, scale_inv, mel_opt
        self._dft = stft_kernel(frame_length, frame_shift, window)
        ldd = (frame_length + 2 + 31) // 32 * 32                                   # K of the adjoint projection (include/sepr.h)
        self._dft_t = torch.zeros(frame_length, ldd)
        self._dft_t[:, : frame_length + 2] = self._dft[: frame_length + 2].t()
        if self.device.type == "cuda":
            self._dft = self._dft.to(self.device)
            self._dft_t = self._dft_t.to(self.device).contiguous()

    def __repr__(self):
        return (f"<PIT_SISNR_mag(device={self.device!r}, frame_length={self.frame_length}, frame_shift={self.frame_shift}, "
                f"window={self.window!r}, num_stages={self.num_stages}, num_spks={self.num_spks}, scale_inv=True, mel_opt=False)>")

    def __call__(self, **kwargs) -> torch.Tensor:
        estims, targets = kwargs["estims"], kwargs["target_attr"]
        if not 0 <= int(kwargs["idx"]) < self.num_stages:
            raise IndexError("idx out of range")                                    # self.stft[idx] in the reference
        n = estims.shape[0] if isinstance(estims, torch.Tensor) else len(estims)
        if n != self.num_spks:
            raise RuntimeError(f"expected {self.num_spks} estimates, got {n}")
        if self._dft.device.type != "cuda":
            raise RuntimeError("PIT_SISNR_mag was built for a non-HIP device (no CPU fallback exists)")
        if _needs_grad(estims):                                                     # training (engine.py:68,75)
            loss = _PitMagFn.apply(_stack_g(estims), _stack(targets, "target_attr"), self._dft, self._dft_t, self.frame_length,
                                   self.frame_shift, 1.0e-12)
            return torch.sum(loss) / kwargs["input_sizes"].shape[0]
        out = pit_sisnr_mag(estims, targets, self._dft, self.frame_length, self.frame_shift)
        return torch.sum(out["loss"]) / kwargs["input_sizes"].shape[0]             # reference :175-176


class PIT_SASDR_time:
    """``PIT_SASDR_time(device, num_spks, snr_max=30.0)`` with the call surface of ``PIT_SISNR_time``: the source-aggregated,
    soft-thresholded SDR, the criterion for windows in which a talker is silent.  Returns
    ``num_spks * mean_b loss[b]``: a loop that divides the criterion by ``num_spks`` (``trainer.mix_loss``) then reads dB per utterance, and
    a fully active example weighs what the sum of its per-source terms weighs in the SI-SNR form."""

    def __init__(self, device, num_spks: int, snr_max: float = 30.0):
        self.device, self.num_spks, self.snr_max = torch.device(device), num_spks, float(snr_max)

    def __repr__(self):
        return f"<{type(self).__name__}(device={self.device!r}, num_spks={self.num_spks!r}, snr_max={self.snr_max!r})>"

    def __call__(self, **kwargs) -> torch.Tensor:
        estims, targets = kwargs["estims"], kwargs["target_attr"]
        n = estims.shape[0] if isinstance(estims, torch.Tensor) else len(estims)
        if n != self.num_spks:
            raise RuntimeError(f"expected {self.num_spks} estimates, got {n}")
        if _needs_grad(estims):
            loss = _SaSdrTimeFn.apply(_stack_g(estims), _stack(targets, "target_attr"), 1.0e-8, self.snr_max)
        else:
            loss = pit_sasdr(estims, targets, snr_max=self.snr_max)["loss"]
        return self.num_spks * torch.sum(loss) / kwargs["input_sizes"].shape[0]


class PIT_SASDR_mag(PIT_SISNR_mag):
    """``PIT_SASDR_mag(device, frame_length, frame_shift, window, num_stages, num_spks, snr_max=30.0)`` with the call surface of
    ``PIT_SISNR_mag`` (whose STFT kernel and eps = 1e-12 it keeps): ``PIT_SASDR_time``'s expression on STFT magnitudes, target scale 1."""

    def __init__(self, device, frame_length: int, frame_shift: int, window: str, num_stages: int, num_spks: int, snr_max: float = 30.0):
        super().__init__(device, frame_length, frame_shift, window, num_stages, num_spks)
        self.snr_max = float(snr_max)

    def __repr__(self):
        return (f"<PIT_SASDR_mag(device={self.device!r}, frame_length={self.frame_length}, frame_shift={self.frame_shift}, "
                f"window={self.window!r}, num_stages={self.num_stages}, num_spks={self.num_spks}, snr_max={self.snr_max!r})>")

    def __call__(self, **kwargs) -> torch.Tensor:
        estims, targets = kwargs["estims"], kwargs["target_attr"]
        if not 0 <= int(kwargs["idx"]) < self.num_stages:
            raise IndexError("idx out of range")
        n = estims.shape[0] if isinstance(estims, torch.Tensor) else len(estims)
        if n != self.num_spks:
            raise RuntimeError(f"expected {self.num_spks} estimates, got {n}")
        if self._dft.device.type != "cuda":
            raise RuntimeError("PIT_SASDR_mag was built for a non-HIP device (no CPU fallback exists)")
        if _needs_grad(estims):
            loss = _SaSdrMagFn.apply(_stack_g(estims), _stack(targets, "target_attr"), self._dft, self._dft_t, self.frame_length,
                                     self.frame_shift, 1.0e-12, self.snr_max)
        else:
            loss = pit_sasdr_mag(estims, targets, self._dft, self.frame_length, self.frame_shift, snr_max=self.snr_max)["loss"]
        return self.num_spks * torch.sum(loss) / kwargs["input_sizes"].shape[0]


# ---- Graph-PIT ------------------------------------------------------------------------------------
GRAPH_MAX_CHANNELS, GRAPH_MAX_ROWS = 3, 8


class GraphPIT:
    """``GraphPIT(device, channels, rows, batch, samples, snr_max=30.0)``: the targets of a conversation window for a separator of ``channels``
    outputs, from the window's ``rows`` target rows - one per utterance heard in it (``sepr_graph_pit_assign`` / ``sepr_graph_pit_assemble``,
    include/sepr.h; the CPU restatement is ``tests/graphpit_ref.py``).  Rows that overlap in time may not share a channel; among the colourings
    of that graph the one with the lowest source-aggregated error against the estimates is taken, and each channel's target is the sum of its
    rows.

    The object owns static device tensors, so both launches replay from a captured graph: ``spans`` int32 ``[B, U, 2]`` and ``adj`` int32
    ``[B, U]`` (the tables ``load`` rewrites), ``col`` int32 ``[B, U]``, ``value`` float64 ``[B]``, ``status`` int32 ``[B]`` (1: the graph of
    that example has no colouring with ``channels`` colours - ``col`` is 0, ``value`` NaN) and the ``channels`` assembled targets ``[B, T]``.

    ``graph(estims, rows)`` returns those target tensors.  They are targets: nothing is differentiated through them.  The loss is the existing
    ``PIT_SASDR_time`` / ``PIT_SASDR_mag`` on ``(estims, graph(estims, rows))`` - their permutation search includes the identity.  The SI-SNR
    pair is refused (``check_pair``): an assembled channel is often silent, where those criteria have no usable gradient."""

    SLOTS = 4               # pinned staging buffers in flight
    EPS = 1.0e-8            # PIT_SASDR_time's

    def __init__(self, device, channels: int, rows: int, batch: int, samples: int, snr_max: float = 30.0):
        C_, U, B, T = int(channels), int(rows), int(batch), int(samples)
        if not (1 <= C_ <= GRAPH_MAX_CHANNELS and 1 <= U <= GRAPH_MAX_ROWS and B >= 1 and T >= 4 and T % 4 == 0):
            raise ValueError(f"GraphPIT: 1..{GRAPH_MAX_CHANNELS} channels, 1..{GRAPH_MAX_ROWS} rows, batch >= 1 and a positive multiple of 4 "
                             f"samples, got {(C_, U, B, T)}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GraphPIT runs on the HIP device (there is no CPU path)")
        self.channels, self.rows, self.batch, self.samples, self.snr_max = C_, U, B, T, float(snr_max)
        nbytes = int(L.load().sepr_graph_pit_bytes(C_, U, B))
        if nbytes == 0:
            raise RuntimeError(f"unsupported Graph-PIT problem: channels={C_}, rows={U}, batch={B}")
        dev = self.device
        self._table = torch.zeros(3 * B * U, dtype=torch.int32, device=dev)      # spans, then adj: one copy re-targets both launches
        self.spans = self._table[:2 * B * U].view(B, U, 2)
        self.adj = self._table[2 * B * U:].view(B, U)
        self.col = torch.zeros(B, U, dtype=torch.int32, device=dev)
        self.value = torch.zeros(B, dtype=torch.float64, device=dev)
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)
        self.targets = [torch.zeros(B, T, dtype=torch.float32, device=dev) for _ in range(C_)]
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._stage: List[torch.Tensor] = []
        self._events: list = []
        self._slot = 0

    def __repr__(self):
        return (f"<GraphPIT(device={self.device!r}, channels={self.channels}, rows={self.rows}, batch={self.batch}, samples={self.samples}, "
                f"snr_max={self.snr_max!r})>")

    @staticmethod
    def check_pair(*criteria) -> None:
        """Refuse the SI-SNR criteria as the loss on assembled targets."""
        for c in criteria:
            if isinstance(c, (PIT_SISNR_time, PIT_SISNRi)) or type(c) is PIT_SISNR_mag:
                raise ValueError(f"{type(c).__name__} on Graph-PIT targets: an assembled channel is often silent, where the SI-SNR criteria give "
                                 "a zero or unbounded gradient - use PIT_SASDR_time / PIT_SASDR_mag")

    def load(self, spans, adj) -> None:
        """The tables of the next call, from host arrays (``spans`` ``[B, U, 2]``, ``adj`` ``[B, U]``, any integer type): written into a pinned
        staging buffer, then one asynchronous copy on the current stream.  Nothing waits for the device."""
        import numpy as np
        B, U = self.batch, self.rows
        sp, ad = np.asarray(spans), np.asarray(adj)
        if sp.shape != (B, U, 2) or ad.shape != (B, U):
            raise ValueError(f"GraphPIT.load: spans {(B, U, 2)} and adj {(B, U)}, got {sp.shape} and {ad.shape}")
        if not self._stage:
            self._stage = [torch.empty(3 * B * U, dtype=torch.int32).pin_memory() for _ in range(self.SLOTS)]
            self._events = [None] * self.SLOTS
        k = self._slot
        self._slot = (k + 1) % self.SLOTS
        if self._events[k] is not None:
            self._events[k].synchronize()               # the copy that last read this staging buffer has run (SLOTS batches ago)
        host = self._stage[k].numpy()
        host[:2 * B * U] = sp.astype(np.int64).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32).ravel()
        host[2 * B * U:] = (ad.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).ravel()
        self._table.copy_(self._stage[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._events[k] = ev

    def _pointers(self, tensors, count: int, what: str):
        ts = list(tensors) if not isinstance(tensors, torch.Tensor) else list(tensors.unbind(0))
        if len(ts) != count:
            raise RuntimeError(f"expected {count} {what}, got {len(ts)}")
        keep = []
        for t in ts:
            t = t.detach()
            if t.device != self.device or tuple(t.shape) != (self.batch, self.samples):
                raise RuntimeError(f"{what}: [{self.batch}, {self.samples}] tensors on {self.device}, got {tuple(t.shape)} on {t.device}")
            keep.append(t.to(torch.float32).contiguous())
        import ctypes
        return (ctypes.c_void_p * count)(*[t.data_ptr() for t in keep]), keep

    def assign(self, estims, rows) -> None:
        """``col``, ``value`` and ``status`` of the batch in ``rows`` against ``estims`` under the loaded tables."""
        lib = L.load()
        ep, ek = self._pointers(estims, self.channels, "estimates")
        rp, rk = self._pointers(rows, self.rows, "target rows")
        with torch.cuda.device(self.device):
            L.check(lib.sepr_graph_pit_assign(ep, rp, self.spans.data_ptr(), self.adj.data_ptr(), self.channels, self.rows, self.batch,
                                              self.samples, self.EPS, self.snr_max, self.col.data_ptr(), self.value.data_ptr(),
                                              self.status.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                              torch.cuda.current_stream(self.device).cuda_stream), "sepr_graph_pit_assign")

    def assemble(self, rows) -> List[torch.Tensor]:
        """The channels' targets from ``rows`` under ``col``: written into ``self.targets`` and returned."""
        import ctypes
        lib = L.load()
        rp, rk = self._pointers(rows, self.rows, "target rows")
        op = (ctypes.c_void_p * self.channels)(*[t.data_ptr() for t in self.targets])
        with torch.cuda.device(self.device):
            L.check(lib.sepr_graph_pit_assemble(rp, self.spans.data_ptr(), self.col.data_ptr(), self.channels, self.rows, self.batch,
                                                self.samples, op, torch.cuda.current_stream(self.device).cuda_stream),
                    "sepr_graph_pit_assemble")
        return self.targets

    def __call__(self, estims, rows) -> List[torch.Tensor]:
        with torch.no_grad():
            self.assign(estims, rows)
            return self.assemble(rows)


# ---- BSS-eval SDR (PIT_SDRi, criterions.py:264-289) ----------------------------------------------------------------------
BSS_FLEN = 512                    # mir_eval's distortion-filter length
BSS_WS_CAP = 1 << 30               # one call's workspace stays under 1 GiB: larger batches are split


def _bss_stack(x: _TensorList, what: str) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.stack(list(x), dim=0)
    if not t.is_cuda:
        raise RuntimeError(f"{what} is not on the HIP device (no CPU fallback exists)")
    return t.detach().to(torch.float32)


def bss_eval(references: torch.Tensor, estimates: torch.Tensor, mixture: torch.Tensor = None, lengths=None):
    """Batched BSS-eval on the device: references / estimates ``[S,B,T]``, mixture ``[B,T]`` or None, lengths ``[B]`` valid
    samples (default T).  Returns a dict of numpy arrays ``sdr, sir, sar`` (float64) and ``perm`` (int64) ``[B,S]`` indexed by
    reference, ``sdr_mix`` ``[B,S]`` when a mixture is given, and ``status`` ``[B]`` (0 ok, 1 silent source, 2 factorisation
    failed).  ``csrc/sepr_bsseval.hip`` through ``sepr_bss_eval_fwd``."""
    import numpy as np
    ref, est = _bss_stack(references, "reference_sources"), _bss_stack(estimates, "estimated_sources")
    if ref.dim() != 3 or ref.shape != est.shape:
        raise ValueError(f"reference {tuple(ref.shape)} and estimated {tuple(est.shape)} sources must both be [S,B,T]")
    S, B, T = ref.shape
    dev = ref.device
    if est.device != dev:
        raise RuntimeError("estimates and references are on different devices")
    if not 2 <= S <= 3:
        raise ValueError(f"num_spks={S}: the device BSS-eval supports 2 or 3 sources")
    mix = None
    if mixture is not None:
        mix = _bss_stack(mixture, "mixture")
        if tuple(mix.shape) != (B, T) or mix.device != dev:
            raise RuntimeError("mixture must be [batch, samples] on the same device as the estimates")
    lens = [T] * B if lengths is None else [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if len(lens) != B:
        raise ValueError(f"{len(lens)} lengths for a batch of {B}")
    for b, n in enumerate(lens):
        if not S * BSS_FLEN <= n <= T:
            raise ValueError(f"utterance {b}: valid length {n} outside [{S * BSS_FLEN}, {T}] (BSS-eval needs at least "
                             f"num_spks * {BSS_FLEN} samples)")
    lib = L.load()
    out = {k: np.empty((B, S), np.float64) for k in ("sdr", "sir", "sar")}
    out["perm"] = np.empty((B, S), np.int64)
    out["status"] = np.empty(B, np.int64)
    if mix is not None:
        out["sdr_mix"] = np.empty((B, S), np.float64)
    per_utt = lib.sepr_bss_eval_workspace(S, 1, T)
    step = max(1, min(B, BSS_WS_CAP // max(per_utt, 1)))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        for b0 in range(0, B, step):
            n = min(step, B - b0)
            e, r = est[:, b0:b0 + n].contiguous(), ref[:, b0:b0 + n].contiguous()
            m = None if mix is None else mix[b0:b0 + n].contiguous()
            nbytes = lib.sepr_bss_eval_workspace(S, n, T)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            sdr, sir, sar = (torch.empty(n, S, dtype=torch.float64, device=dev) for _ in range(3))
            perm = torch.empty(n, S, dtype=torch.int32, device=dev)
            status = torch.empty(n, dtype=torch.int32, device=dev)
            sdr_mix = None if m is None else torch.empty(n, S, dtype=torch.float64, device=dev)
            lens_c = (L._i * n)(*lens[b0:b0 + n])
            L.check(lib.sepr_bss_eval_fwd(e.data_ptr(), r.data_ptr(), None if m is None else m.data_ptr(), lens_c, S, n, T,
                                          sdr.data_ptr(), sir.data_ptr(), sar.data_ptr(), perm.data_ptr(),
                                          None if sdr_mix is None else sdr_mix.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                          ws.numel(), stream.cuda_stream), "sepr_bss_eval_fwd")
            for k, v in (("sdr", sdr), ("sir", sir), ("sar", sar), ("perm", perm), ("status", status), ("sdr_mix", sdr_mix)):
                if v is not None:
                    out[k][b0:b0 + n] = v.cpu().numpy()
    return out


def _bss_raise(status) -> None:
    for b, s in enumerate(status.tolist()):
        if s == 1:
            raise ValueError(f"utterance {b}: a reference, estimated or mixture source is silent (all zeros); BSS-eval is "
                             "undefined for it (mir_eval.separation.validate raises the same)")
        if s == 2:
            raise RuntimeError(f"utterance {b}: the Gram matrix of the delayed references is not positive definite "
                               "(Cholesky pivot <= 0)")


def bss_eval_sources(reference_sources, estimated_sources, input_sizes=None):
    """``mir_eval.separation.bss_eval_sources(reference_sources, estimated_sources)`` (mir_eval 0.7, compute_permutation=True)
    on the HIP device.  ``[S,T]`` tensors give ``(sdr [S], sir [S], sar [S], perm [S])`` numpy arrays as mir_eval does;
    ``[S,B,T]`` tensors give the same with a leading batch dimension, ``input_sizes`` ``[B]`` the valid length of each
    utterance.  Values are indexed by REFERENCE k: ``sdr[k]`` belongs to estimate ``perm[k]`` (``PIT_SISNRi`` indexes by
    estimate instead).  A silent source raises ValueError, a failed factorisation RuntimeError."""
    ref = reference_sources if isinstance(reference_sources, torch.Tensor) else torch.stack(list(reference_sources))
    est = estimated_sources if isinstance(estimated_sources, torch.Tensor) else torch.stack(list(estimated_sources))
    if ref.dim() not in (2, 3) or ref.shape != est.shape:
        raise ValueError(f"reference {tuple(ref.shape)} and estimated {tuple(est.shape)} sources must both be [S,T] or [S,B,T]")
    flat = ref.dim() == 2
    if flat:
        ref, est = ref[:, None], est[:, None]
    out = bss_eval(ref, est, lengths=input_sizes)
    _bss_raise(out["status"])
    res = tuple(out[k] for k in ("sdr", "sir", "sar", "perm"))
    return tuple(r[0] for r in res) if flat else res


class PIT_SDRi:
    """``PIT_SDRi(device, dump)`` of the reference (criterions.py:264-289, configs.yaml ``PIT_SDRi: {dump: 0}``):
    ``__call__(estims=, mixture=, input_sizes=, target_attr=)`` -> ``(sum of SDRi / num_utts, SDRi per reference)`` with
    SDRi = SDR(estimates) - SDR(mixture repeated num_spks times), BSS-eval on the device (``bss_eval`` above).  The reference
    concatenates the mixture exactly twice (so num_spks = 3 raises there); here it is repeated num_spks times.  The mixture's
    correlations are formed once, not once per repetition.  SDRi is indexed by reference, as mir_eval returns it."""

    def __init__(self, device, dump: int = 0):
        self.device, self.dump = torch.device(device), dump

    def __repr__(self):
        return f"<PIT_SDRi(device={self.device!r}, dump={self.dump!r})>"

    def __call__(self, **kwargs):
        import numpy as np
        if self.device.type != "cuda":
            raise RuntimeError("PIT_SDRi was built for a non-HIP device (no CPU fallback exists)")
        est = _bss_stack(kwargs["estims"], "estims").to(self.device)
        tgt = _bss_stack([t.to(self.device) for t in kwargs["target_attr"]] if not isinstance(kwargs["target_attr"], torch.Tensor)
                         else kwargs["target_attr"].to(self.device), "target_attr")
        mix = kwargs["mixture"].to(self.device)
        input_sizes = kwargs["input_sizes"]
        B = est.shape[1]
        lengths = input_sizes.reshape(-1).tolist() if input_sizes.numel() == B else None
        out = bss_eval(tgt, est, mixture=mix.reshape(B, -1), lengths=lengths)
        _bss_raise(out["status"])
        sdri = out["sdr"] - out["sdr_mix"]
        num_utts = input_sizes.shape[0]
        return np.sum(sdri) / num_utts, (sdri[0] if B == 1 else sdri)


# ---- STOI / ESTOI (beyond the reference, which reports SI-SNRi and SDRi only) --------------------------------
STOI_FS = 10000                    # the rate the measure is defined at
STOI_FRAME, STOI_BIN0, STOI_NBIN = 256, 7, 212
STOI_WS_CAP = 1 << 30              # one call's workspace stays under 1 GiB: larger batches are split
_stoi_tables = {}


def stoi_tables(device) -> torch.Tensor:
    """The constants ``sepr_stoi_fwd`` reads (include/sepr.h), float64 on ``device``: the window ``hanning(258)[1:-1]`` and the twiddle
    pairs ``(cos, sin)(2 pi ((7 + k) t mod 512) / 512)`` for t < 256, k < 212 - the argument is reduced in integers first."""
    import numpy as np
    key = str(device)
    if key not in _stoi_tables:
        t = np.arange(STOI_FRAME, dtype=np.int64)[:, None]
        k = STOI_BIN0 + np.arange(STOI_NBIN, dtype=np.int64)[None, :]
        ang = 2.0 * np.pi * ((k * t) % 512).astype(np.float64) / 512.0
        tab = np.concatenate([np.hanning(STOI_FRAME + 2)[1:-1], np.stack([np.cos(ang), np.sin(ang)], axis=2).ravel()])
        _stoi_tables[key] = torch.from_numpy(tab).to(device)
    return _stoi_tables[key]


def stoi(references: torch.Tensor, estimates: torch.Tensor, mixture: torch.Tensor = None, lengths=None, fs: int = 8000):
    """STOI and ESTOI of every (reference, estimate) pair on the device: references / estimates ``[S,B,T]``, mixture ``[B,T]`` or None,
    lengths ``[B]`` valid samples (default T), all sampled at ``fs``.  Signals at another rate than 10 kHz go through the measure's own
    converter first (``resample.plan_oct``, one ``sepr_resample_fwd`` launch), then ``sepr_stoi_fwd`` (``csrc/sepr_stoi.hip``).  Returns a
    dict of device tensors: ``stoi``, ``estoi`` float64 ``[B,S,S]`` (entry (i, j): reference i against estimate j), ``stoi_mix``,
    ``estoi_mix`` float64 ``[B,S]`` when a mixture is given, ``kept`` int32 ``[B,S]`` (frames of reference i that are not silent) and
    ``status`` int32 ``[B,S]`` (bit 0: fewer than 30 frames left, the values of that reference are 1e-5)."""
    from .resample import out_len, plan_oct, resample_oct
    ref, est = _bss_stack(references, "references"), _bss_stack(estimates, "estimates")
    if ref.dim() != 3 or ref.shape != est.shape:
        raise ValueError(f"references {tuple(ref.shape)} and estimates {tuple(est.shape)} must both be [S,B,T]")
    S, B, T = ref.shape
    dev = ref.device
    if est.device != dev:
        raise RuntimeError("estimates and references are on different devices")
    if not 2 <= S <= 3:
        raise ValueError(f"num_spks={S}: the device STOI supports 2 or 3 sources")
    mix = None
    if mixture is not None:
        mix = _bss_stack(mixture, "mixture")
        if tuple(mix.shape) != (B, T) or mix.device != dev:
            raise RuntimeError("mixture must be [batch, samples] on the same device as the estimates")
    lens = [T] * B if lengths is None else [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if len(lens) != B:
        raise ValueError(f"{len(lens)} lengths for a batch of {B}")
    for b, n in enumerate(lens):
        if not 1 <= n <= T:
            raise ValueError(f"utterance {b}: valid length {n} outside [1, {T}]")
    fs = int(fs)
    sig = torch.cat([ref.permute(1, 0, 2), est.permute(1, 0, 2)] + ([] if mix is None else [mix[:, None]]), dim=1)   # [B][2S(+1)][T]
    Q = sig.shape[1]
    if fs != STOI_FS:                                   # the 10 kHz signals, ragged, then back into one zero-padded block
        p = plan_oct(fs, STOI_FS)
        lens10 = [out_len(n, p.L, p.M) for n in lens]
        T10 = max(max(lens10), STOI_FRAME)
        parts = resample_oct([sig[b, q, :lens[b]].contiguous() for b in range(B) for q in range(Q)], fs, STOI_FS)
        if min(lens10) == T10:
            sig = torch.stack(parts).view(B, Q, T10)
        else:
            sig = torch.zeros(B, Q, T10, dtype=torch.float32, device=dev)
            for b in range(B):
                for q in range(Q):
                    sig[b, q, :lens10[b]] = parts[b * Q + q]
        lens, T = lens10, T10
    elif T < STOI_FRAME:
        sig = torch.nn.functional.pad(sig, (0, STOI_FRAME - T))
        T = STOI_FRAME
    lib = L.load()
    tab = stoi_tables(dev)
    out = {"stoi": torch.empty(B, S, S, dtype=torch.float64, device=dev), "estoi": torch.empty(B, S, S, dtype=torch.float64, device=dev),
           "kept": torch.empty(B, S, dtype=torch.int32, device=dev), "status": torch.empty(B, S, dtype=torch.int32, device=dev)}
    if mix is not None:
        out["stoi_mix"] = torch.empty(B, S, dtype=torch.float64, device=dev)
        out["estoi_mix"] = torch.empty(B, S, dtype=torch.float64, device=dev)
    per_utt = lib.sepr_stoi_workspace(S, 1, T)
    if per_utt == 0:
        raise ValueError(f"unsupported STOI problem: num_spks={S}, samples={T}")
    step = max(1, min(B, STOI_WS_CAP // per_utt, 65535 // (S * (S + 2))))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        for b0 in range(0, B, step):
            n = min(step, B - b0)
            r, e = sig[b0:b0 + n, :S].contiguous(), sig[b0:b0 + n, S:2 * S].contiguous()
            m = None if mix is None else sig[b0:b0 + n, 2 * S].contiguous()
            ws = torch.empty(lib.sepr_stoi_workspace(S, n, T), dtype=torch.uint8, device=dev)
            o = {k: v[b0:b0 + n] for k, v in out.items()}                       # leading-dimension slices are contiguous views
            L.check(lib.sepr_stoi_fwd(r.data_ptr(), e.data_ptr(), None if m is None else m.data_ptr(), lens_d[b0:b0 + n].data_ptr(), S, n, T,
                                      tab.data_ptr(), o["stoi"].data_ptr(), o["estoi"].data_ptr(),
                                      None if m is None else o["stoi_mix"].data_ptr(), None if m is None else o["estoi_mix"].data_ptr(),
                                      o["kept"].data_ptr(), o["status"].data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream),
                    "sepr_stoi_fwd")
    return out


def stoi_pit(values, values_mix):
    """values ``[B,S,S]`` (reference i, estimate j) and values_mix ``[B,S]`` as numpy float64 -> ``(perm [B,S], chosen [B,S], improvement
    [B,S])`` indexed by reference: per utterance the first maximiser of the mean over ``itertools.permutations``."""
    import itertools
    import numpy as np
    B, S, _ = values.shape
    perms = list(itertools.permutations(range(S)))
    k = np.arange(S)
    perm = np.empty((B, S), np.int64)
    for b in range(B):
        perm[b] = perms[int(np.argmax([np.mean(values[b, k, list(p)]) for p in perms]))]
    chosen = np.take_along_axis(values, perm[:, :, None], axis=2)[:, :, 0]
    return perm, chosen, chosen - values_mix


class PIT_STOI:
    """``PIT_STOI(device, extended=False, fs=8000)`` with the criteria's call surface: ``__call__(estims=, mixture=, input_sizes=,
    target_attr=)`` -> ``(sum of the improvements / num_utts, improvement per reference)`` with improvement = STOI (ESTOI when
    ``extended``) of the chosen estimate minus that of the mixture, on the device (``stoi`` above).  The permutation is the first
    maximiser of the mean value over ``itertools.permutations``; values are indexed by reference, as ``PIT_SDRi`` indexes them.  The
    last call's permutation and values stay in ``perm`` / ``values``.  Evaluation only: there is no backward."""

    def __init__(self, device, extended: bool = False, fs: int = 8000):
        self.device, self.extended, self.fs = torch.device(device), bool(extended), int(fs)
        self.perm = self.values = None

    def __repr__(self):
        return f"<PIT_STOI(device={self.device!r}, extended={self.extended!r}, fs={self.fs!r})>"

    def __call__(self, **kwargs):
        import numpy as np
        if self.device.type != "cuda":
            raise RuntimeError("PIT_STOI was built for a non-HIP device (no CPU fallback exists)")
        est = _bss_stack(kwargs["estims"], "estims").to(self.device)
        tgt = _bss_stack([t.to(self.device) for t in kwargs["target_attr"]] if not isinstance(kwargs["target_attr"], torch.Tensor)
                         else kwargs["target_attr"].to(self.device), "target_attr")
        mix = kwargs["mixture"].to(self.device)
        input_sizes = kwargs["input_sizes"]
        B = est.shape[1]
        lengths = input_sizes.reshape(-1).tolist() if input_sizes.numel() == B else None
        out = stoi(tgt, est, mixture=mix.reshape(B, -1), lengths=lengths, fs=self.fs)
        key = "estoi" if self.extended else "stoi"
        self.perm, self.values, imp = stoi_pit(out[key].cpu().numpy(), out[key + "_mix"].cpu().numpy())
        return np.sum(imp) / input_sizes.shape[0], (imp[0] if B == 1 else imp)
