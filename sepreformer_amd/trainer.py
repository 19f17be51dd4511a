"""The reference's training run (``Engine.run`` / ``_train`` / ``_validate`` in ``models/*/engine.py``, the checkpoint pair of
``utils/util_engine.py``, the warm-up of ``utils/implements/schedulers.py``) around the captured step.

    train = DynamicMixFeed(corpus, plan_wsj0, batch=16, max_len=32000, seed=0, fixed_length=True)
    valid = DynamicMixFeed(valid_corpus, plan_direct, batch=16, max_len=32000, seed=0, drop_last=False)
    Trainer(model, train, valid, "checkpoints/", lr=1e-3, seed=0).run()

``Trainer`` owns the model, a ``FlatAdamW(skip_nonfinite=True)``, the two feeds, the criteria and an optional test iterable.  A
steady-state step costs no host synchronisation: the loss parts and the optimizer's scalars are folded into a float64 ledger on
the device (``include/sepr.h`` sepr_run_ledger_update, launched from ``FlatAdamW.step``), which the host looks at once per log interval
(an asynchronous copy into pinned memory: the queue is not drained) and reads once per epoch.  The loss mix ``alpha(epoch)`` lives in two device scalars the captured graph reads, so an epoch boundary is a
``fill_`` and no re-capture.  A step whose gradient norm is not finite is skipped on the device and counted.

A checkpoint (``epoch.NNNN.pth``: the reference's five keys plus ``sepr_run_state``) and fresh Python objects continue the
trajectory bit for bit: the dropout words of global step ``i`` are a pure function of ``(run seed, i)`` (``seed_word`` /
``salt_word``), the feeds' generator states travel in the file, and the first batch of a (re)start is the example batch of the
capture - a real batch, a real step, counted.

``ema_decay=d`` keeps an exponential moving average of the weights inside the optimizer's update launch (``FlatAdamW(ema_decay=d)``,
DESIGN.md section 5g-2).  ``validate_with`` says which weights validation, the plateau schedule, ``best`` and the test loop see:
``"ema"`` (the default; the passes run inside ``opt.averaged()``), ``"raw"``, or ``"both"`` (two ``[VALID]`` lines, the averaged
result decides).  The checkpoint then carries ``ema_state_dict`` - the keys of ``model_state_dict``, parameters from the average,
buffers from the model - which ``infer.load_checkpoint_weights(..., ema=True)`` or a plain ``load_state_dict`` takes on its own.  The
EMA never touches the raw trajectory, and the decay schedule has no state: its ``t`` is the optimizer's step counter.

Two deliberate differences from the reference: every epoch is saved by default (``save="all"``; the reference saves the epochs that
beat the loss the run STARTED from), and non-finite steps are skipped instead of poisoning the weights.

Out of scope: data-parallel runs (the feeds' ``rank`` / ``world`` and ``model.grad_sync`` are passed through untouched and not
tested here; with the EMA on, every rank would apply the same update to its own buffer, so the buffers would agree - untested
too), TensorBoard, the MAC summary, and ``mvn`` (refused; every shipped config has it false).
"""
from __future__ import annotations

import os
import re
import time
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import torch

from . import lib as L

CHECKPOINT_KEYS = ("epoch", "model_state_dict", "optimizer_state_dict", "train_loss", "valid_loss")      # util_engine.py:98-105
RUN_STATE_KEY = "sepr_run_state"
EMA_KEY = "ema_state_dict"
_NAME = re.compile(r"^epoch\.(\d+)\.pth$")
_M64 = (1 << 64) - 1


# ---- host-only pieces (tests/test_trainer_cpu.py) ----------------------------------------------------------------------------------
def alpha(epoch: int) -> float:
    """``engine.py:72``: the weight of the magnitude losses, 0.4 until epoch 100, then times 0.8 every five epochs."""
    return 0.4 * 0.8 ** (1 + (epoch - 101) // 5) if epoch > 100 else 0.4


def warmup_lr(base_lr: float, i: int, warmup_steps: int) -> float:
    """``engine.py:61`` + ``schedulers.py:20-23``: the learning rate before the ``i``-th batch (1-based) of epoch 1."""
    return base_lr * (float(i) / float(warmup_steps) if i < warmup_steps else 1.0)


def batch_lr(current: float, base_lr: float, epoch: int, i: int, warmup_steps: int) -> float:
    """The learning rate the ``i``-th batch of ``epoch`` runs at: the warm-up steps only in epoch 1 (``engine.py:61``); every other epoch,
    and so an epoch 1 that ended before ``warmup_steps``, leaves the rate where it is."""
    return warmup_lr(base_lr, i, warmup_steps) if epoch == 1 else current


def _mix64(z: int) -> int:
    """splitmix64's finaliser."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def seed_word(seed: int) -> int:
    """The by-value dropout seed every capture of a run freezes: a constant of the run."""
    return _mix64(_mix64(int(seed) & _M64) ^ 0x5EED) & 0x3FFFFFFFFFFFFFFF


def salt_word(seed: int, step: int) -> int:
    """The dropout salt of global step ``step`` (1-based): a counter-based hash of ``(run seed, step)``, no state."""
    return _mix64(_mix64(int(seed) & _M64) ^ _mix64(int(step) & _M64)) & 0x7FFFFFFFFFFFFFFF


def ema_decay_at(t: int, decay: float, warmup: float = 10.0) -> float:
    """The EMA decay of optimizer step ``t`` (1-based, the optimizer's own counter after its increment), as the prepare kernel of
    ``sepr_adamw_step_ema`` forms it in double: ``decay``, ramped in as ``(1 + t) / (warmup + t)`` while that is smaller; ``warmup <= 0``
    turns the ramp off."""
    if warmup <= 0:
        return float(decay)
    return min(float(decay), (1.0 + float(t)) / (float(warmup) + float(t)))


def checkpoint_name(epoch: int) -> str:
    return f"epoch.{epoch:04}.pth"                      # util_engine.py:106


def list_checkpoints(directory: str) -> List[Tuple[int, str]]:
    """``(epoch, path)`` of every ``epoch.NNNN.pth`` in ``directory``, ascending."""
    if not os.path.isdir(directory):
        return []
    found = [(int(m.group(1)), os.path.join(directory, f)) for f in os.listdir(directory) for m in [_NAME.match(f)] if m]
    return sorted(found)


def latest_checkpoint(directory: str) -> Optional[str]:
    """``util_engine.py:31-38``: the file with the highest ``NNNN``; ``None`` for an empty (or missing) directory."""
    found = list_checkpoints(directory)
    return found[-1][1] if found else None


def should_save(save: str, valid_loss: float, best: float) -> bool:
    if save not in ("all", "best"):
        raise ValueError("save: 'all' or 'best'")
    return save == "all" or valid_loss < best


def prune_checkpoints(directory: str, keep_last: Optional[int]) -> List[str]:
    """Remove all but the ``keep_last`` highest-numbered checkpoints; returns what was removed."""
    if not keep_last:
        return []
    gone = [p for _, p in list_checkpoints(directory)[:-int(keep_last)]]
    for p in gone:
        os.remove(p)
    return gone


def write_checkpoint(directory: str, epoch: int, model_sd: dict, optimizer_sd: dict, train_loss: float, valid_loss: float,
                     run_state: dict, keep_last: Optional[int] = None, extra: Optional[dict] = None) -> str:
    """The reference's five keys plus ``sepr_run_state``, inside ONE file: the reference's loader parses every file name of the
    directory as ``epoch.<int>.``, so nothing else may lie there - the file is written beside the directory and moved in.
    ``extra``: further top-level keys (``ema_state_dict``); none of the six may be replaced."""
    body = {"epoch": int(epoch), "model_state_dict": model_sd, "optimizer_state_dict": optimizer_sd, "train_loss": float(train_loss),
            "valid_loss": float(valid_loss), RUN_STATE_KEY: run_state}
    if extra:
        clash = set(extra) & set(body)
        if clash:
            raise ValueError(f"write_checkpoint: extra may not replace {sorted(clash)}")
        body.update(extra)
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, checkpoint_name(epoch))
    tmp = os.path.join(os.path.dirname(os.path.abspath(directory)), "." + os.path.basename(os.path.abspath(directory)) + "." + checkpoint_name(epoch) + ".tmp")
    torch.save(body, tmp)
    os.replace(tmp, path)
    prune_checkpoints(directory, keep_last)
    return path


def read_checkpoint(path: str) -> dict:
    return torch.load(path, map_location="cpu")


def plateau_step(scheduler, epoch: int, start_scheduling: int, valid_loss: float) -> bool:
    """``engine.py:201``: the plateau scheduler sees the validation time loss only after ``start_scheduling``."""
    if epoch > start_scheduling:
        scheduler.step(valid_loss)
        return True
    return False


def epoch_means(part_sums: Sequence[float], steps: float, num_spks: int) -> Tuple[float, float]:
    """``engine.py:82-83`` from the ledger's float64 sums: ``(T_Loss, F_Loss)``, each divided by ``num_spks`` (``:69,71``)."""
    if steps <= 0:
        return float("nan"), float("nan")
    t = float(part_sums[0]) / num_spks
    f = [float(s) / num_spks for s in part_sums[1:]]
    return t / steps, sum(f) / len(f) / steps


def mix_loss(l_time: torch.Tensor, l_mag: Sequence[torch.Tensor], w_time: torch.Tensor, w_freq: torch.Tensor, num_spks: int) -> torch.Tensor:
    """``engine.py:73-74`` with the two weights as tensors: ``(w_time * l_time + w_freq * mean_i(l_mag_i)) / num_spks``.  The one
    statement of the expression: the captured graph and a check outside it evaluate the same operations in the same order."""
    acc = l_mag[0]
    for m in l_mag[1:]:
        acc = acc + m
    return (w_time * l_time + w_freq * (acc / len(l_mag))) / num_spks


CRITERIA = ("sisnr", "sasdr", "graph_sasdr")


def check_criterion(criterion: str, absent: float, rows: Optional[int] = None) -> None:
    """What ``Trainer`` refuses: an unknown criterion, the SI-SNR criteria on a feed that makes windows with a silent talker or target rows
    (``rows``: the training feed's ``.rows``, ``None`` for a feed of sources), and Graph-PIT on a feed without rows."""
    if criterion == "graph_sisnr":
        raise ValueError("Graph-PIT is built on the SA-SDR pair only: an assembled channel is often silent, where the SI-SNR criteria give a zero "
                         "or unbounded gradient - use criterion='graph_sasdr'")
    if criterion not in CRITERIA:
        raise ValueError(f"criterion: one of {CRITERIA}, got {criterion!r}")
    if criterion == "graph_sasdr" and rows is None:
        raise ValueError("criterion='graph_sasdr' needs a training feed of target rows (convfeed.ConversationWindowFeed: it has .rows)")
    if criterion != "graph_sasdr" and rows is not None:
        raise ValueError(f"the training feed makes {rows} target rows per window, not one source per channel: train it with "
                         "criterion='graph_sasdr'")
    if criterion == "sisnr" and float(absent or 0.0) > 0.0:
        raise ValueError(f"the training feed has absent = {absent}: on a silent target the SI-SNR criteria give the estimate a zero gradient "
                         "(time form: alpha = 0) or one that grows like 1 / |estimate| (magnitude form); train it with criterion='sasdr'")


def check_resume_criterion(criterion: str, run_state: Optional[dict], path: str = "the checkpoint") -> None:
    """A checkpoint of a run with another criterion than ``"sisnr"`` records it in ``sepr_run_state`` (a missing key, or no run state at all,
    means ``"sisnr"``); the losses of the two are different scales, so a run continues with the one it began with."""
    was = (run_state or {}).get("criterion", "sisnr")
    if was != criterion:
        raise ValueError(f"{path} was trained with criterion={was!r}, this run asks for {criterion!r}: best, the plateau schedule and the "
                         "loss curves would mix two scales - resume with the same criterion or start in a fresh directory")


class Ledger:
    """Host view of one read of the device ledger (``lib.LEDGER_SLOTS``)."""

    def __init__(self, values: Sequence[float], nparts: int):
        s = L.LEDGER_SLOTS
        v = [float(x) for x in values]
        self.values, self.nparts = v, nparts
        self.steps, self.skipped, self.nonfinite = v[s["steps"]], v[s["skipped"]], v[s["nonfinite"]]
        self.gnorm_sum, self.gnorm_max, self.clipped = v[s["gnorm_sum"]], v[s["gnorm_max"]], v[s["clipped"]]
        self.part_sum = v[s["part_sum"]:s["part_sum"] + nparts]
        self.last = v[s["part_sum"] + nparts:s["part_sum"] + 2 * nparts]


# ---- the run ------------------------------------------------------------------------------------------------------------------------
class Trainer:
    def __init__(self, model, train_feed, valid_feed, checkpoint_dir: str, lr: float = 1.0e-3, weight_decay: float = 1.0e-2,
                 seed: int = 0, max_epoch: int = 200, clip_norm: Optional[float] = 5.0, start_scheduling: int = 50,
                 test_epochs: Sequence[int] = (100, 120, 150, 170), warmup_steps: int = 1000, factor: float = 0.8, patience: int = 2,
                 min_lr: float = 1.0e-10, mvn: bool = False, save: str = "all", keep_last: Optional[int] = None, log_every: int = 50,
                 max_skipped: int = 10, test_utterances: Optional[Callable[[], Iterable]] = None, log: Callable[[str], None] = print,
                 ema_decay: Optional[float] = None, ema_warmup: float = 10.0, validate_with: str = "ema", criterion: str = "sisnr",
                 snr_max: float = 30.0):
        """``train_feed``: a ``DynamicMixFeed`` with ``fixed_length=True``; ``valid_feed``: one over ``plan_direct`` (``drop_last=False``
        keeps the trailing partial batch, as the reference's validation loader does).  ``test_utterances``: a callable returning the
        iterable ``infer.evaluate_utterances`` takes, run at ``test_epochs``.  The other arguments are the reference's ``engine`` /
        ``optimizer`` / ``scheduler`` settings; the defaults are the values its four ``configs.yaml`` share.  ``ema_decay`` / ``ema_warmup``:
        the weight EMA of ``FlatAdamW``; ``validate_with`` (``"raw"``, ``"ema"``, ``"both"``) is ignored while it is off.  ``criterion``:
        ``"sisnr"`` (the reference's ``PIT_SISNR_time`` / ``PIT_SISNR_mag``) or ``"sasdr"`` (``PIT_SASDR_time`` / ``PIT_SASDR_mag`` with
        ``snr_max``), for training and validation alike; a training feed with ``absent > 0`` needs ``"sasdr"``.
        ``"graph_sasdr"`` (section 5e-8): the SA-SDR pair on the targets a ``criterion.GraphPIT`` assembles from the target rows of a
        ``convfeed.ConversationWindowFeed``; a validation feed without ``.rows`` is scored by the plain SA-SDR pair."""
        if mvn:
            raise ValueError("mvn: true is not supported (every shipped configuration has it false)")
        if not getattr(train_feed, "fixed_length", False):
            raise ValueError("the training feed must be built with fixed_length=True (the captured step has one shape)")
        should_save(save, 0.0, 0.0)
        if validate_with not in ("raw", "ema", "both"):
            raise ValueError("validate_with: 'raw', 'ema' or 'both'")
        if warmup_steps < 1 or log_every < 1:
            raise ValueError("warmup_steps >= 1 and log_every >= 1")
        check_criterion(criterion, getattr(train_feed, "absent", 0.0), getattr(train_feed, "rows", None))
        from .criterion import GraphPIT, PIT_SASDR_mag, PIT_SASDR_time, PIT_SISNR_mag, PIT_SISNR_time
        from .optim import FlatAdamW
        self.model, self.train_feed, self.valid_feed, self.dir = model, train_feed, valid_feed, checkpoint_dir
        self.cfg = model.cfg
        self.dev = next(model.parameters()).device
        self.base_lr, self.seed = float(lr), int(seed)
        self.max_epoch, self.clip_norm, self.start_scheduling, self.test_epochs = int(max_epoch), clip_norm, int(start_scheduling), tuple(test_epochs)
        self.warmup_steps, self.save_mode, self.keep_last = int(warmup_steps), save, keep_last
        self.log_every, self.max_skipped, self.test_utterances, self.log = int(log_every), int(max_skipped), test_utterances, log
        self.opt = FlatAdamW(model, lr=lr, weight_decay=weight_decay, skip_nonfinite=True, ema_decay=ema_decay, ema_warmup=ema_warmup)
        self.ema = ema_decay is not None
        self.validate_with = validate_with if self.ema else "raw"
        self.last_valid_raw: Optional[Tuple[float, float, int]] = None          # validate_with="both": the raw weights' result of the last epoch
        self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.opt, mode="min", factor=factor, patience=patience, min_lr=min_lr)
        S, R = self.cfg.num_spks, self.cfg.num_stages
        self.criterion, self.snr_max = criterion, float(snr_max)
        if criterion in ("sasdr", "graph_sasdr"):
            self.crit_t = PIT_SASDR_time(self.dev, S, self.snr_max)
            self.crit_m = PIT_SASDR_mag(self.dev, 512, 128, "hann", R, S, self.snr_max)
        else:
            self.crit_t = PIT_SISNR_time(self.dev, S, True)
            self.crit_m = PIT_SISNR_mag(self.dev, 512, 128, "hann", R, S, True, False)
        self.nparts = 1 + R
        self.parts = torch.zeros(self.nparts, dtype=torch.float32, device=self.dev)
        self.ledger = torch.zeros(L.ledger_doubles(self.nparts), dtype=torch.float64, device=self.dev)
        self.vparts, self.vledger = torch.zeros_like(self.parts), torch.zeros_like(self.ledger)
        self.w_time = torch.full((), 1.0 - alpha(1), dtype=torch.float32, device=self.dev)
        self.w_freq = torch.full((), alpha(1), dtype=torch.float32, device=self.dev)
        self.opt.attach_ledger(self.ledger, self.parts)
        B, T = train_feed.batch, train_feed.max_len
        self._sizes = torch.full((B,), T)                # fixed-length rows: the padding is part of the example
        self._x = torch.zeros(B, T, device=self.dev)
        # Graph-PIT: the step's targets are the feed's rows, and the criteria see what the GraphPIT assembles from them inside the captured step
        self.graph = GraphPIT(self.dev, S, train_feed.rows, B, T, self.snr_max) if criterion == "graph_sasdr" else None
        self._vgraph = None                              # the validation feed's, built on its first batch of rows
        self._targets = [torch.zeros(B, T, device=self.dev) for _ in range(S if self.graph is None else train_feed.rows)]
        self.step = None                                 # CapturedTrainStep, built on the first batch of a (re)start
        self._snap: Optional[torch.Tensor] = None        # pinned host copy of the ledger for the log interval's look
        self.global_step, self.best, self.start_epoch = 0, float("inf"), 1
        self.last_checkpoint: Optional[str] = None

    # ---- loss ---------------------------------------------------------------------------------------------------------------------
    def set_alpha(self, a: float) -> None:
        """The loss mix of the coming steps: two ``fill_``s on the scalars the captured graph reads."""
        self.w_time.fill_(1.0 - a)
        self.w_freq.fill_(a)

    def _loss_fn(self, audio, aux, *targets):
        tg = list(targets) if self.graph is None else self.graph(audio, list(targets))
        l_time = self.crit_t(estims=audio, input_sizes=self._sizes, target_attr=tg).reshape(())
        l_mag = [self.crit_m(estims=a, idx=i, input_sizes=self._sizes, target_attr=tg).reshape(()) for i, a in enumerate(aux)]
        with torch.no_grad():
            self.parts.copy_(torch.stack([l_time.detach()] + [m.detach() for m in l_mag]))
        return mix_loss(l_time, l_mag, self.w_time, self.w_freq, self.cfg.num_spks)

    def _salt(self) -> int:
        return salt_word(self.seed, self.global_step + 1)

    def _seed(self) -> int:
        return seed_word(self.seed)

    def _build_step(self):
        """The captured step of this (re)start, from the batch in ``_x`` / ``_targets``: its one eager warm-up step is a real training step.  The
        model draws the run's constant seed word while a step exists (``release`` takes the hook off again)."""
        from .train_step import CapturedTrainStep
        self.model.dropout_seed_fn = self._seed           # the dropout words of global step i: a pure function of (run seed, i)
        self.step = CapturedTrainStep(self.model, self._loss_fn, self.opt, self._x, self._targets, max_norm=self.clip_norm, warmup=1,
                                      salt_fn=self._salt)
        self.model.invalidate_packed()                    # the warm-up step wrote the weights behind the version counters; only replays invalidate

    def read_ledger(self, valid: bool = False) -> Ledger:
        """One device-to-host copy (synchronises)."""
        return Ledger((self.vledger if valid else self.ledger).cpu().tolist(), self.nparts)

    # ---- epochs -------------------------------------------------------------------------------------------------------------------
    def _check_skipped(self, led: Ledger, seen: float) -> float:
        if led.skipped > seen:
            self.log(f"[SKIP] {int(led.skipped - seen)} step(s) with a non-finite gradient norm skipped up to global step {self.global_step}")
        if led.skipped > self.max_skipped:
            raise RuntimeError(f"{int(led.skipped)} steps of this epoch had a non-finite gradient norm (max_skipped = {self.max_skipped}); "
                               f"last good checkpoint: {self.last_checkpoint or 'none'}")
        return led.skipped

    def train_epoch(self, epoch: int) -> Tuple[float, float, int]:
        """``_train`` (``engine.py:50-83``): one epoch of the training feed -> ``(T_Loss, F_Loss, num_batch)``."""
        self.model.train()
        self.set_alpha(alpha(epoch))
        self.ledger.zero_()
        group = self.opt.param_groups[0]
        i, seen = 0, 0.0
        pending = None                                   # (event, batch, global step, lr) of a ledger snapshot on its way to the host
        if self._snap is None:
            self._snap = torch.zeros(self.ledger.numel(), dtype=torch.float64).pin_memory()

        def report(ev, at, gstep, lr):
            nonlocal seen
            ev.synchronize()
            led = Ledger(self._snap.tolist(), self.nparts)
            seen = self._check_skipped(led, seen)
            t, f = epoch_means(led.part_sum, led.steps, self.cfg.num_spks)
            self.log(f"epoch {epoch} batch {at} (global step {gstep}): T_Loss {t:.4f}  F_Loss {f:.4f}  "
                     f"grad norm max {led.gnorm_max:.3f}  clipped {int(led.clipped)}  lr {lr:.3e}")

        for plan in self.train_feed.plans():
            i += 1
            group["lr"] = batch_lr(group["lr"], self.base_lr, epoch, i, self.warmup_steps)
            if self.graph is not None:
                self.graph.load(plan.spans, plan.adj)     # the tables the step's two Graph-PIT launches read
            if self.step is None:
                self.train_feed.write(plan, self._x, self._targets)
                self._build_step()
            else:
                self.train_feed.write(plan, self.step.x, self.step.targets)
                self.step(self.step.x, self.step.targets)
            self.global_step += 1
            if pending is not None and pending[0].query():
                report(*pending)
                pending = None
            if i % self.log_every == 0:
                # the log interval's look at the ledger must not drain the queue (a drained queue costs the launch latency of a whole
                # step's graph): an asynchronous copy into pinned memory and an event; the line is printed once the copy has landed,
                # a step or two later, while the device works on
                if pending is not None:
                    report(*pending)
                self._snap.copy_(self.ledger, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.dev))
                pending = (ev, i, self.global_step, group["lr"])
        if pending is not None:
            report(*pending)
        led = self.read_ledger()
        self._check_skipped(led, seen)
        t, f = epoch_means(led.part_sum, led.steps, self.cfg.num_spks)
        return t, f, i

    def validate(self, weights: Optional[str] = None) -> Tuple[float, float, int]:
        """``_validate`` (``engine.py:86-110``): one pass over the validation feed -> the same three values.  The batch means are
        averaged, so a trailing partial batch weighs as much as a full one.  ``weights``: ``"raw"`` or ``"ema"``; the default is what
        ``validate_with`` says (``"both"`` counts as ``"ema"`` here: ``run`` makes the second pass)."""
        if weights is None:
            weights = "raw" if self.validate_with == "raw" else "ema"
        if weights == "ema":
            with self.opt.averaged():
                return self._validate()
        return self._validate()

    def _validate(self) -> Tuple[float, float, int]:
        lib = L.load()
        self.model.eval()
        nb = 0
        with torch.inference_mode():
            self.vledger.zero_()
            rows = getattr(self.valid_feed, "rows", None) if self.graph is not None else None
            for sizes, mix, src, _ in self.valid_feed:
                audio, aux = self.model(mix)
                if rows is not None:                      # a feed of rows: the targets its own GraphPIT assembles against these estimates
                    if self._vgraph is None:
                        from .criterion import GraphPIT
                        self._vgraph = GraphPIT(self.dev, self.cfg.num_spks, rows, int(mix.shape[0]), int(mix.shape[1]), self.snr_max)
                    plan = self.valid_feed.last_plan
                    self._vgraph.load(plan.spans, plan.adj)
                    src = self._vgraph(audio, src)
                l_time = self.crit_t(estims=audio, input_sizes=sizes, target_attr=src).reshape(())
                l_mag = [self.crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=src).reshape(()) for i, a in enumerate(aux)]
                self.vparts.copy_(torch.stack([l_time] + l_mag))
                with torch.cuda.device(self.dev):
                    L.check(lib.sepr_run_ledger_update(self.vparts.data_ptr(), self.nparts, None, self.vledger.data_ptr(), self.vledger.numel(),
                                                       torch.cuda.current_stream(self.dev).cuda_stream), "sepr_run_ledger_update")
                nb += 1
        led = self.read_ledger(valid=True)
        t, f = epoch_means(led.part_sum, led.steps, self.cfg.num_spks)
        return t, f, nb

    def test(self) -> Optional[Tuple[float, float, int]]:
        if self.test_utterances is None:
            return None
        from .infer import evaluate_utterances
        self.model.eval()
        if self.validate_with != "raw":                    # "ema" and "both": the shipped weights are the averaged ones
            with self.opt.averaged():
                return evaluate_utterances(self.model, self.test_utterances())
        return evaluate_utterances(self.model, self.test_utterances())

    # ---- checkpoints --------------------------------------------------------------------------------------------------------------
    def run_state(self) -> dict:
        rs = {"global_step": int(self.global_step), "plateau": self.scheduler.state_dict(), "train_feed": self.train_feed.state_dict(),
              "valid_feed": self.valid_feed.state_dict(), "best": float(self.best), "seed": int(self.seed)}
        if self.criterion != "sisnr":                     # a missing key means "sisnr": the layout of a run with the reference's criteria is unchanged
            rs["criterion"] = self.criterion
        if self.ema:
            rs["ema"] = {"decay": float(self.opt.ema_decay), "warmup": float(self.opt.ema_warmup)}
        return rs

    def save(self, epoch: int, train_loss: float, valid_loss: float) -> Optional[str]:
        """Every epoch (``save="all"``) or the epochs that beat the best so far (``"best"``); ``keep_last`` prunes older files."""
        keep = should_save(self.save_mode, valid_loss, self.best)
        self.best = min(self.best, valid_loss)
        if not keep:
            return None
        cpu = lambda v: v.detach().cpu().clone() if torch.is_tensor(v) else v      # noqa: E731  (compact copies, not views of the flat buffers)
        osd = self.opt.state_dict()
        osd = {"state": {k: {n: cpu(v) for n, v in st.items()} for k, st in osd["state"].items()}, "param_groups": osd["param_groups"]}
        msd = {k: cpu(v) for k, v in self.model.state_dict().items()}
        extra = None
        if self.ema:
            # the keys of model_state_dict: parameters from the average, buffers (BatchNorm statistics) from the model - loadable on its own
            esd = self.opt.ema_state_dict()
            extra = {EMA_KEY: {k: esd.get(k, v) for k, v in msd.items()}}
        self.last_checkpoint = write_checkpoint(self.dir, epoch, msd, osd, train_loss, valid_loss, self.run_state(), self.keep_last, extra)
        return self.last_checkpoint

    def load_latest(self) -> int:
        """``util_engine.py:12-47``: load the latest checkpoint of the directory, if there is one -> the epoch to start at.  A file in the
        reference's five-key layout (no ``sepr_run_state``) continues with fresh feeds and the optimizer's own step count."""
        path = latest_checkpoint(self.dir)
        if path is None:
            self.start_epoch = 1
            return 1
        ck = read_checkpoint(path)
        self.model.load_state_dict(ck["model_state_dict"], strict=False)
        self.model.invalidate_packed()
        self.opt.load_state_dict(ck["optimizer_state_dict"])
        rs = ck.get(RUN_STATE_KEY)
        check_resume_criterion(self.criterion, rs, path)
        if rs is not None:
            self.seed, self.global_step, self.best = int(rs["seed"]), int(rs["global_step"]), float(rs["best"])
            self.scheduler.load_state_dict(rs["plateau"])
            self.train_feed.load_state_dict(rs["train_feed"])
            self.valid_feed.load_state_dict(rs["valid_feed"])
        else:
            self.global_step = int(float(self.opt._step.item()))
        if self.ema:
            if EMA_KEY in ck:
                self.opt.load_ema_state_dict(ck[EMA_KEY])
            else:
                self.opt.reset_ema()
                self.log(f"{path} carries no {EMA_KEY}: the weight EMA starts again at the loaded weights")
        self.last_checkpoint = path
        self.start_epoch = int(ck["epoch"]) + 1
        self.log(f"loaded {path}: resuming at epoch {self.start_epoch}, global step {self.global_step}")
        return self.start_epoch

    # ---- Engine.run ---------------------------------------------------------------------------------------------------------------
    def run(self) -> None:
        start = self.load_latest()
        t0 = time.time()
        init_t = init_f = 0.0
        if start > 1:
            keep = self.valid_feed.state_dict()          # the initial validation is a report, not part of the trajectory
            init_t, init_f, _ = self.validate()
            self.valid_feed.load_state_dict(keep)
        self.log(f"[INIT] Epoch {start:2d}: Loss_t = {init_t:.4f} dB | Loss_f = {init_f:.4f} dB | Speed = ({time.time() - t0:.2f}s)")
        try:
            for epoch in range(start, self.max_epoch):
                t0 = time.time()
                tr_t, tr_f, tr_n = self.train_epoch(epoch)
                t1 = time.time()
                raw = None
                if self.validate_with == "both":
                    # the same batches for both passes: the raw pass is put back out of the feed's state, so the feed moves on once per epoch
                    keep = self.valid_feed.state_dict()
                    raw = self.validate("raw")
                    self.valid_feed.load_state_dict(keep)
                    t_raw = time.time()
                va_t, va_f, va_n = self.validate()
                t2 = time.time()
                plateau_step(self.scheduler, epoch, self.start_scheduling, va_t)      # with the EMA on ("ema", "both"): the averaged weights' loss
                self.log(f"[TRAIN] Epoch {epoch:2d}: Loss_t = {tr_t:.4f} dB | Loss_f = {tr_f:.4f} dB | Speed = ({t1 - t0:.2f}s/{tr_n:d})")
                if raw is not None:
                    self.log(f"[VALID] Epoch {epoch:2d}: Loss_t = {raw[0]:.4f} dB | Loss_f = {raw[1]:.4f} dB | Speed = ({t_raw - t1:.2f}s/{raw[2]:d}) | raw")
                    self.log(f"[VALID] Epoch {epoch:2d}: Loss_t = {va_t:.4f} dB | Loss_f = {va_f:.4f} dB | Speed = ({t2 - t_raw:.2f}s/{va_n:d}) | ema")
                    self.last_valid_raw = raw
                else:
                    self.log(f"[VALID] Epoch {epoch:2d}: Loss_t = {va_t:.4f} dB | Loss_f = {va_f:.4f} dB | Speed = ({t2 - t1:.2f}s/{va_n:d})")
                if epoch in self.test_epochs and self.test_utterances is not None:
                    t3 = time.time()
                    sisnri, sdri, n = self.test()
                    self.log(f"[TEST] Epoch {epoch:2d}: SISNRi = {sisnri:.4f} dB | SDRi = {sdri:.4f} dB | Speed = ({time.time() - t3:.2f}s/{n:d})")
                self.save(epoch, tr_t, va_t)
                self.last_train, self.last_valid = (tr_t, tr_f, tr_n), (va_t, va_f, va_n)
        finally:
            self.release()

    def release(self) -> None:
        """Drop the captured step and take the seed hook off the model: it draws from its own generator again, and no reference to this
        object stays behind on it."""
        if self.step is not None:
            self.step.release()
            self.step = None
        self.model.__dict__.pop("dropout_seed_fn", None)
