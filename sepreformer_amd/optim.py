"""The optimizer step of the reference loop as three launches: ``clip_grad_norm_`` + ``torch.optim.AdamW.step``
(``engine.py:76-77``) over the training path's flat gradient buffer (``include/sepr.h`` sepr_adamw_step).

    opt = FlatAdamW(model, lr=1e-4, weight_decay=1e-2)
    loss.backward()
    grad_norm = opt.step(max_norm=5.0)          # device scalar: the total norm BEFORE clipping (what clip_grad_norm_ returns)

Why: torch reaches Base's 1 312 parameter tensors through ``multi_tensor_apply`` - 37 launches for the update, 12 for the norms, 37
for the clip scaling, 1.8 ms per step - although the training path already keeps every gradient in ONE buffer.  Here the norm is one
pass over that buffer and the update one launch over a (tensor, first element) block table.

Same arithmetic as ``torch.optim.AdamW`` (decoupled weight decay, bias corrections from the device-side step counter); the
gradients are NOT scaled in place (the clip coefficient is applied inside the update).  ``param_groups[0]["lr"]`` may be changed by
a scheduler: the value is mirrored into a device scalar before each step, so a captured step (``train_step.CapturedTrainStep``)
picks it up without a re-capture.  State (``exp_avg`` / ``exp_avg_sq`` / ``step``) is exposed per parameter as views of the flat
buffers, so ``state_dict()`` has ``torch.optim.AdamW``'s layout.  No CPU path.

``ema_decay=d`` (with ``skip_nonfinite=True``) keeps an exponential moving average of the parameters inside the update launch
(``sepr_adamw_step_ema``): the kernel folds the parameter value it has just stored into a flat fp32 buffer,
``e += (1 - d_t) (p - e)`` with ``d_t = min(d, (1 + t) / (ema_warmup + t))``.  ``averaged()`` exchanges parameters and averages in
place (``sepr_adamw_swap``) for the length of a ``with`` block, so every inference path runs on the averaged weights without a second
model; ``ema_state_dict()`` / ``load_ema_state_dict()`` carry the buffer under the model's ``state_dict`` names.  BatchNorm running
statistics are buffers, not parameters: the averaged model uses the current ones.  ``state_dict()`` does not mention the EMA.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, Optional

import torch

from . import lib as L


class FlatAdamW(torch.optim.Optimizer):
    fused_clip = True          # train_step.CapturedTrainStep: step(max_norm=...) does the clipping itself

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 skip_nonfinite: bool = False, ema_decay: Optional[float] = None, ema_warmup: float = 10.0):
        if ema_decay is not None:
            # the EMA entry is the guarded step: an average that has taken in one poisoned iterate never recovers
            if not skip_nonfinite:
                raise ValueError("FlatAdamW: ema_decay needs skip_nonfinite=True (the EMA is kept by the guarded step)")
            if not 0.0 <= float(ema_decay) < 1.0:
                raise ValueError("FlatAdamW: ema_decay must lie in [0, 1)")
        params = [p for p in model.parameters() if p.requires_grad]
        if not params:
            raise ValueError("no trainable parameters")
        if len(params) != sum(1 for _ in model.parameters()):
            # the norm pass runs over the WHOLE flat gradient buffer, which holds the gradient of every parameter of the model
            raise ValueError("FlatAdamW clips over the model's whole flat gradient buffer: every parameter must be trainable")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or lr < 0.0 or eps < 0.0 or weight_decay < 0.0:
            raise ValueError("invalid AdamW hyper-parameters")
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("FlatAdamW needs the parameters on the HIP device (no CPU path exists)")
        for p in params:
            if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous() or p.data_ptr() % 16:
                raise ValueError("FlatAdamW: every parameter must be a contiguous, 16-byte aligned fp32 tensor on one device")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, capturable=True))
        self._model, self._dev, self._lib = model, dev, L.load()
        # skip_nonfinite: sepr_adamw_step_guarded - a non-finite total gradient norm skips the step (scal[5] = 1) instead of poisoning
        # the weights; with finite gradients the arithmetic is the unguarded entry's, bit for bit
        self.skip_nonfinite = bool(skip_nonfinite)
        self._entry = self._lib.sepr_adamw_step_guarded if self.skip_nonfinite else self._lib.sepr_adamw_step
        self._ledger: Optional[torch.Tensor] = None           # attach_ledger: float64 run ledger every step is folded into
        self._parts: Optional[torch.Tensor] = None
        self._params = params
        blk = self._lib.sepr_adamw_block_elems()
        # moments: 64-element aligned slots, like the gradient buffer
        soff, off = [], 0
        for p in params:
            soff.append(off)
            off += (p.numel() + 63) // 64 * 64
        self._exp_avg = torch.zeros(off, dtype=torch.float32, device=dev)
        self._exp_avg_sq = torch.zeros(off, dtype=torch.float32, device=dev)
        self._step = torch.zeros(1, dtype=torch.float64, device=dev)
        self._lr = torch.full((1,), float(lr), dtype=torch.float32, device=dev)
        self._lr_host = float(lr)
        self._scal = torch.zeros(8, dtype=torch.float32, device=dev)
        self._ws = torch.zeros(self._lib.sepr_adamw_workspace(), dtype=torch.uint8, device=dev)
        blocks = []
        for i, p in enumerate(params):
            blocks.extend((i, e) for e in range(0, p.numel(), blk))
        self._t_params = torch.tensor([p.data_ptr() for p in params], dtype=torch.int64, device=dev)
        self._t_soff = torch.tensor(soff, dtype=torch.int64, device=dev)
        self._t_numel = torch.tensor([p.numel() for p in params], dtype=torch.int32, device=dev)
        self._t_blocks = torch.tensor(blocks, dtype=torch.int32, device=dev).contiguous()
        self._nblocks = len(blocks)
        self._soff = soff
        self._t_goff: Optional[torch.Tensor] = None           # built from the first gradients (their offsets in the flat buffer)
        self._goff_host: Optional[list] = None
        self._ptrs = [p.data_ptr() for p in params]
        self._expose_state()
        # weight EMA: a third flat buffer in the moments' layout, folded by the update launch itself
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = float(ema_warmup)
        self._ema: Optional[torch.Tensor] = None
        self._averaged = False                                # inside averaged(): the parameters hold the EMA, the buffer the raw weights
        if self.ema_decay is not None:
            self._ema = torch.zeros(off, dtype=torch.float32, device=dev)
            self.reset_ema()

    # ---- torch.optim.Optimizer plumbing ---------------------------------------------------------------------------------
    def _expose_state(self):
        for p, so in zip(self._params, self._soff):
            n = p.numel()
            self.state[p] = {"step": self._step[0], "exp_avg": self._exp_avg[so:so + n].view(p.shape),
                             "exp_avg_sq": self._exp_avg_sq[so:so + n].view(p.shape)}

    def load_state_dict(self, state_dict):
        """Accepts a ``torch.optim.AdamW`` / ``FlatAdamW`` state dict: the moments are copied INTO the flat buffers."""
        if len(state_dict.get("param_groups", [])) != 1:
            raise ValueError("FlatAdamW has ONE parameter group (one set of hyper-parameters for the whole flat buffer)")
        super().load_state_dict(state_dict)
        for grp in self.param_groups:           # a torch.optim.AdamW checkpoint carries capturable=False: the step here is always capturable
            grp["capturable"] = True
        steps = []
        for p, so in zip(self._params, self._soff):
            st = self.state.get(p, {})
            if "exp_avg" in st:
                n = p.numel()
                self._exp_avg[so:so + n].copy_(st["exp_avg"].reshape(-1).to(self._dev, torch.float32))
                self._exp_avg_sq[so:so + n].copy_(st["exp_avg_sq"].reshape(-1).to(self._dev, torch.float32))
                steps.append(float(st["step"]))
        if steps:
            if max(steps) != min(steps):
                raise ValueError("FlatAdamW keeps ONE step counter: the loaded per-parameter steps differ")
            self._step.fill_(steps[0])
        self._lr_host = None
        self._expose_state()

    def add_param_group(self, param_group):
        """One group only: the update reads ``param_groups[0]``'s hyper-parameters for every tensor of the flat buffer."""
        if getattr(self, "param_groups", None):
            raise ValueError("FlatAdamW supports a single parameter group (per-group lr / weight decay would be silently ignored)")
        super().add_param_group(param_group)

    def refresh(self):
        """Mirror the (scheduler-updated) learning rate into the device scalar.  Called by ``step`` outside a capture and by
        ``CapturedTrainStep`` before each replay."""
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_host:
            self._lr.fill_(lr)
            self._lr_host = lr

    # ---- the step -----------------------------------------------------------------------------------------------------------
    def _grad_base(self) -> torch.Tensor:
        flat = self._model.__dict__.get("_grad_flat")
        g0 = self._params[0].grad
        if flat is None or g0 is None:
            raise RuntimeError("FlatAdamW.step: no gradients of the HIP training path to apply (call loss.backward() on model(x) first)")
        if self._goff_host is None:
            lo, hi = flat.data_ptr(), flat.data_ptr() + 4 * flat.numel()
            offs = []
            for p in self._params:
                g = p.grad
                if g is None or g.dtype != torch.float32 or not g.is_contiguous() or not (lo <= g.data_ptr() and g.data_ptr() + 4 * g.numel() <= hi):
                    raise RuntimeError("FlatAdamW: a parameter's .grad is not a slice of the model's flat gradient buffer")
                if (g.data_ptr() - lo) % 16:
                    raise RuntimeError("FlatAdamW: a gradient slice of the flat buffer is not 16-byte aligned")
                offs.append((g.data_ptr() - lo) // 4)
            self._goff_host = offs
            self._t_goff = torch.tensor(offs, dtype=torch.int64, device=self._dev)
        else:   # cheap per-step check that the layout has not moved (first and last slice)
            lo = flat.data_ptr()
            gl = self._params[-1].grad
            if g0.data_ptr() - lo != 4 * self._goff_host[0] or gl is None or gl.data_ptr() - lo != 4 * self._goff_host[-1]:
                raise RuntimeError("FlatAdamW: the gradients are no longer slices of the flat gradient buffer in the recorded layout")
        return flat

    def validate(self) -> None:
        """Full check of what ``step`` only spot-checks (first / last tensor): every parameter still lives where the tables say and every
        ``.grad`` is the recorded slice of the model's flat gradient buffer.  ``CapturedTrainStep`` calls it once before capturing."""
        if [p.data_ptr() for p in self._params] != self._ptrs:
            raise RuntimeError("FlatAdamW: a parameter moved after the optimizer was built; build a new optimizer")
        flat = self._model.__dict__.get("_grad_flat")
        if flat is None or self._goff_host is None:
            return
        lo = flat.data_ptr()
        for p, off in zip(self._params, self._goff_host):
            if p.grad is None or p.grad.data_ptr() - lo != 4 * off:
                raise RuntimeError("FlatAdamW: a gradient is no longer the recorded slice of the flat gradient buffer")

    @torch.no_grad()
    def step(self, closure=None, max_norm: Optional[float] = None):
        """One AdamW update; ``max_norm``: clip the total gradient norm first (``clip_grad_norm_`` semantics, norm type 2).  Returns
        the total gradient norm before clipping as a device scalar (``None`` without ``max_norm``)."""
        if closure is not None:
            raise ValueError("FlatAdamW does not take a closure")
        if [p.data_ptr() for p in (self._params[0], self._params[-1])] != [self._ptrs[0], self._ptrs[-1]]:
            raise RuntimeError("FlatAdamW: the parameters moved (model.to(...) after the optimizer was built); build a new optimizer")
        if self._averaged:
            raise RuntimeError("FlatAdamW.step inside averaged(): the parameters hold the averaged weights there, not the trajectory")
        flat = self._grad_base()
        g = self.param_groups[0]
        if not torch.cuda.is_current_stream_capturing():
            self.refresh()
        t = self._tables()
        with torch.cuda.device(self._dev):
            st = torch.cuda.current_stream(self._dev).cuda_stream
            head = (C.byref(t), flat.data_ptr(), flat.numel(), self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(), self._step.data_ptr(),
                    self._lr.data_ptr(), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                    float(max_norm) if max_norm else 0.0)
            tail = (self._scal.data_ptr(), self._ws.data_ptr(), self._ws.numel(), st)
            if self._ema is not None:
                L.check(self._lib.sepr_adamw_step_ema(*head, self._ema.data_ptr(), self.ema_decay, self.ema_warmup, *tail), "sepr_adamw_step_ema")
            else:
                L.check(self._entry(*head, *tail), "sepr_adamw_step_guarded" if self.skip_nonfinite else "sepr_adamw_step")
            if self._ledger is not None:
                # here and nowhere else: an eager step and a captured one (the launch is then part of the optimizer graph) both pass
                # through this line, so the ledger sees every optimizer step exactly once
                L.check(self._lib.sepr_run_ledger_update(self._parts.data_ptr(), self._parts.numel(), self._scal.data_ptr(),
                                                         self._ledger.data_ptr(), self._ledger.numel(), st), "sepr_run_ledger_update")
        return self._scal[0] if max_norm else None

    def _tables(self) -> L.AdamWTables:
        goff = self._t_goff if self._t_goff is not None else self._t_soff      # sepr_adamw_swap does not read the gradient offsets
        return L.AdamWTables(params=self._t_params.data_ptr(), grad_off=goff.data_ptr(), state_off=self._t_soff.data_ptr(),
                             numel=self._t_numel.data_ptr(), blocks=self._t_blocks.data_ptr(), ntensors=len(self._params),
                             nblocks=self._nblocks)

    # ---- the weight EMA ------------------------------------------------------------------------------------------------------
    def _need_ema(self) -> torch.Tensor:
        if self._ema is None:
            raise RuntimeError("FlatAdamW was built without ema_decay: there is no averaged copy of the weights")
        return self._ema

    def _names(self) -> Dict[int, str]:
        return {id(p): n for n, p in self._model.named_parameters()}

    @torch.no_grad()
    def reset_ema(self) -> None:
        """The averages start (again) at the current parameters."""
        ema = self._need_ema()
        if self._averaged:
            raise RuntimeError("FlatAdamW.reset_ema inside averaged()")
        for p, so in zip(self._params, self._soff):
            ema[so:so + p.numel()].copy_(p.detach().reshape(-1))

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """``{parameter name: compact CPU copy of its average}`` under the model's ``state_dict`` names."""
        ema = self._need_ema()
        if self._averaged:
            raise RuntimeError("FlatAdamW.ema_state_dict inside averaged(): the buffer holds the raw weights there")
        names = self._names()
        return {names[id(p)]: ema[so:so + p.numel()].view(p.shape).detach().cpu().clone() for p, so in zip(self._params, self._soff)}

    @torch.no_grad()
    def load_ema_state_dict(self, sd) -> None:
        """Takes what ``ema_state_dict`` returns (further keys, a model's buffers for instance, are ignored)."""
        ema = self._need_ema()
        if self._averaged:
            raise RuntimeError("FlatAdamW.load_ema_state_dict inside averaged()")
        names = self._names()
        for p, so in zip(self._params, self._soff):
            name = names[id(p)]
            if name not in sd:
                raise KeyError(f"load_ema_state_dict: no entry for parameter {name}")
            v = sd[name]
            if tuple(v.shape) != tuple(p.shape):
                raise ValueError(f"load_ema_state_dict: {name} has shape {tuple(v.shape)}, the parameter {tuple(p.shape)}")
            ema[so:so + p.numel()].copy_(v.reshape(-1).to(self._dev, torch.float32))

    def _swap(self) -> None:
        t = self._tables()
        with torch.cuda.device(self._dev):
            L.check(self._lib.sepr_adamw_swap(C.byref(t), self._ema.data_ptr(), torch.cuda.current_stream(self._dev).cuda_stream),
                    "sepr_adamw_swap")
        self._model.invalidate_packed()                       # the packed weight forms were derived from the other set

    @contextlib.contextmanager
    def averaged(self):
        """Inside the block the model's parameters ARE the averaged weights (and the EMA buffer holds the raw ones): one in-place, bitwise
        exchange on entry and one on exit, each followed by ``model.invalidate_packed()``.  No nesting, no ``step`` inside."""
        self._need_ema()
        if self._averaged:
            raise RuntimeError("FlatAdamW.averaged() does not nest")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FlatAdamW.averaged() inside a graph capture")
        if [p.data_ptr() for p in self._params] != self._ptrs:
            raise RuntimeError("FlatAdamW: a parameter moved after the optimizer was built; build a new optimizer")
        self._swap()
        self._averaged = True
        try:
            yield self
        finally:
            self._averaged = False
            self._swap()

    def attach_ledger(self, ledger: Optional[torch.Tensor], parts: Optional[torch.Tensor] = None) -> None:
        """From now on every ``step`` ends with one ``sepr_run_ledger_update`` launch that folds ``parts`` (the step's loss scalars, fp32,
        written by the caller before ``step``) and this optimizer's ``scal`` into ``ledger`` (float64, ``lib.ledger_doubles(len(parts))``
        long).  A step captured into a graph keeps the two tensors it was captured with.  ``None`` detaches."""
        if ledger is None:
            self._ledger = self._parts = None
            return
        if parts is None or parts.dtype != torch.float32 or parts.dim() != 1 or not parts.is_contiguous() or parts.device != self._dev:
            raise ValueError("parts: a contiguous 1-D fp32 tensor on the optimizer's device")
        if not 1 <= parts.numel() <= L.LEDGER_MAX_PARTS:
            raise ValueError(f"1 .. {L.LEDGER_MAX_PARTS} loss parts")
        if ledger.dtype != torch.float64 or not ledger.is_contiguous() or ledger.device != self._dev or ledger.numel() != L.ledger_doubles(parts.numel()):
            raise ValueError(f"ledger: a contiguous float64 tensor of {L.ledger_doubles(parts.numel())} elements on the optimizer's device")
        self._ledger, self._parts = ledger, parts

    @property
    def skipped(self) -> torch.Tensor:
        """Device scalar: 1 when the last guarded ``step`` was skipped for a non-finite gradient norm, else 0."""
        return self._scal[5]

    @property
    def clip_coef(self) -> torch.Tensor:
        """Device scalar: the clip coefficient of the last ``step(max_norm=...)`` that was applied.  A guarded step that was skipped
        (``skipped`` = 1) writes the norm and the skip flag only: this scalar then still holds the step before's."""
        return self._scal[1]
