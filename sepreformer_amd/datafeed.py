"""Training batches from a device-resident corpus with dynamic mixing.

The reference builds every training example of its ``*_DM_*`` variants on the host (``models/SepReformer_Large_DM_*/dataset.py``:
``_dynamic_mixing`` picks a second utterance, RMS-normalises it to the first, draws gains and - WHAM / WHAMR - a noise file, crops
and sums, in librosa + numpy inside ``DataLoader`` workers).  Here the whole corpus lives in HBM (``Corpus``), the random choices of
a batch are a small table made on the host (``plan_*``, the reference's own draws from a ``random.Random`` in the reference's order)
and ONE launch (``csrc/sepr_dynmix.hip``) gathers, scales, sums and zero-pads the batch (``DynamicMixFeed``).  The host touches no
sample.

    corpus = Corpus.from_scp({"s1": "tr_s1.scp", "s2": "tr_s2.scp"}, fs=8000, device="cuda:0")
    feed = DynamicMixFeed(corpus, plan_wsj0, batch=16, max_len=32000, seed=0, fixed_length=True)
    step = CapturedTrainStep(model, loss_fn, opt, x, targets)
    for _ in range(steps):
        feed.next_into(step.x, step.targets)
        loss, grad_norm = step(step.x, step.targets)

What is exact: a PCM16 sample is ``int16 / 32768`` (what ``librosa.load`` returns for such a file), its sum of squares an int64, the
two multiplies and the sum of the terms the reference's float32 operations in the reference's order.  The one thing that is not the
reference's bit for bit is the RMS: numpy takes it from a pairwise float32 sum, this module from the exact integer sum (a few ulp).

Speed perturbation: ``plan_wsj0`` / ``plan_wham`` / ``plan_whamr`` take ``speeds=`` (integer percentages, e.g.
``range(95, 106)``) and draw one per source; a perturbed term is the stored utterance passed through ``resample.plan(p, 100)``, converted
inside the mixing launch (``sepr_dynmix_speed_fwd``) on the cropped span only.

Reverberation: the same three planners take ``rirs=`` (a ``reverb.RirBank``) and draw one impulse response per
source; a reverberant term is the stored utterance convolved with the first ``taps`` samples of that response inside the mixing launch
(``sepr_dynmix_reverb_fwd``) - the whole response in the mixture, by default its direct path in the target.

Both: with ``speed_reverb=True`` the three planners take ``speeds=`` and ``rirs=`` together; a term that carries both is
the PERTURBED utterance under the response - the talker speaks faster or slower, then the room answers - made inside the one launch
(``sepr_dynmix_speed_reverb_fwd``).

Turn-taking: the three planners take ``turns=Turns(overlap=(lo, hi), ramp=RL)`` - alone or with any of the above - and give
every source a turn ``[on, off)`` of the example, so that the talkers overlap for a drawn fraction of their turns instead of the whole crop; the gate
acts on the talker inside the launch (``sepr_dynmix_turns_fwd``), before the room, which therefore rings on after the talker stops.  With
``absent=P`` beside ``turns`` one talker of an example, with probability P, is silent throughout - the empty turn, a ``+0.0`` target row - which the
trainer's ``criterion="sasdr"`` can score.

Shuffling: the reference shuffles through ``DataLoader(shuffle=True)`` (torch's generator); this feed takes the epoch's key order
from the caller (``keys=``), and by default draws a permutation from its own ``random.Random`` before every epoch.
"""
from __future__ import annotations

import ctypes as C
import math
import random
from typing import Callable, Dict, Iterator, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import lib as L_
from . import resample as R_
from .reverb import RirBank

# (utterance index, start sample, norm factor, gain), plus the speed in percent when the planner was given speeds, or plus
# (speed, RIR index or -1, taps) when it was given an RIR bank - the speed 100 unless it was given both (speed_reverb=True) - or plus
# (speed, RIR index or -1, taps, on, off) when it was given turns: the turn [on, off) in output samples of the example
Term = Union[Tuple[int, int, np.float32, np.float32], Tuple[int, int, np.float32, np.float32, int],
             Tuple[int, int, np.float32, np.float32, int, int, int], Tuple[int, int, np.float32, np.float32, int, int, int, int, int]]
_ONE = np.float32(1.0)
TURN_FAR = 1 << 30                                     # (-TURN_FAR, TURN_FAR) is the open turn: the gate is 1 wherever it can be evaluated
MAX_TURN_RAMP = 4096                                   # the longest ramp table sepr_dynmix_turns_fwd takes


class Example(NamedTuple):
    key: str
    n: int                      # output samples (a multiple of 4)
    mix: Tuple[Term, ...]       # M mixture terms, summed in this order
    tgt: Tuple[Term, ...]       # S target terms


class _PlanFields(NamedTuple):
    keys: List[str]
    n: np.ndarray               # int32 [B], descending
    utt: np.ndarray             # int32 [B, M + S]: the M mixture terms, then the S target terms
    start: np.ndarray           # int32 [B, M + S]
    norm: np.ndarray            # float32 [B, M + S]
    gain: np.ndarray            # float32 [B, M + S]
    M: int
    S: int
    speed: Optional[np.ndarray] = None      # int32 [B, M + S] percent (100 = as recorded), None: planned without speeds
    rir: Optional[np.ndarray] = None        # int32 [B, M + S] index into the RIR bank (-1 = none), None: planned without RIRs
    taps: Optional[np.ndarray] = None       # int32 [B, M + S] leading samples of that RIR the term is convolved with


class BatchPlan(_PlanFields):
    """The tuple above and, beside it, the turn columns of a plan with turns: ``on`` and ``off``, int32 ``[B, M + S]``,
    the term's turn ``[on, off)`` in output samples of the example; ``None``: planned without turns.  They are keyword arguments and
    attributes, not fields of the tuple - its eleven fields, their order and their defaults are what a plan without turns has always had,
    and code that builds or unpacks one by position keeps working.  ``_replace`` and ``_asdict`` take and keep them.  Whatever goes through
    the bare tuple does NOT: ``BatchPlan(*plan)``, ``_make``, unpacking, ``==`` and ``hash`` see the eleven fields only, so a plan rebuilt by
    position has lost its turns and would take the entry without them - carry ``on=plan.on, off=plan.off`` along, or use ``_replace``."""
    on: Optional[np.ndarray] = None
    off: Optional[np.ndarray] = None

    def __new__(cls, *args, on: Optional[np.ndarray] = None, off: Optional[np.ndarray] = None, **kw):
        self = super().__new__(cls, *args, **kw)
        if (on is None) != (off is None):
            raise ValueError("a plan with turns carries both columns, on and off")
        self.on, self.off = on, off
        return self

    def _replace(self, **kw):
        on, off = kw.pop("on", self.on), kw.pop("off", self.off)
        return BatchPlan(*super()._replace(**kw), on=on, off=off)

    def _asdict(self):
        return {**super()._asdict(), "on": self.on, "off": self.off}


def parse_scp(path: str) -> Dict[str, str]:
    """The reference's ``key path`` lists (``utils/util_dataset.py::parse_scps``): two tokens per line, no duplicate key."""
    out: Dict[str, str] = {}
    with open(path) as f:
        for line in f:
            tok = line.strip().split()
            if not tok:
                continue
            if len(tok) != 2:
                raise RuntimeError(f"{path}: expected 'key path', got {line!r}")
            if tok[0] in out:
                raise ValueError(f"{path}: duplicate key {tok[0]!r}")
            out[tok[0]] = tok[1]
    return out


class Corpus:
    """Utterances resident on the device: one int16 buffer (PCM16 files as they are on disk), one float32 buffer (everything else),
    an int64 table ``offsets [N + 1]`` of cumulative element counts on the device, names and lengths on the host.  Storage order:
    the int16 utterances first, then the float32 ones, each group in the order given; ``index[name]`` is the utterance's number.

    ``device=None`` keeps the layout on the host only (inspectable, not usable by a feed): the energies come from the device
    (``sepr_corpus_energy``, once at load) or from the caller (``set_energies``, e.g. kept from an earlier load)."""

    def __init__(self, names16, arrays16, names32, arrays32, device=None, fs: Optional[int] = None):
        self.names: List[str] = list(names16) + list(names32)
        if not self.names:
            raise ValueError("an empty corpus")
        if len(set(self.names)) != len(self.names):
            raise ValueError("duplicate utterance names")
        self.n16, self.fs = len(names16), fs
        self.index: Dict[str, int] = {k: i for i, k in enumerate(self.names)}
        self.lengths = np.array([int(a.shape[0]) for a in list(arrays16) + list(arrays32)], dtype=np.int64)
        if int(self.lengths.min()) < 1:
            raise ValueError("every utterance must hold at least one sample")
        self.offsets_host = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.total16 = int(self.offsets_host[self.n16])
        self.total32 = int(self.offsets_host[-1]) - self.total16
        self.roles: Dict[str, List[str]] = {}            # from_scp: role -> keys in file order
        self.ss16: Optional[np.ndarray] = None           # int64 [n16] sum of squares of the raw int16 values
        self.ss32: Optional[np.ndarray] = None           # float64 [N - n16]
        self._rms: Optional[np.ndarray] = None
        self.device = None if device is None else torch.device(device)
        self.buf16 = self.buf32 = self.offsets = None
        self._host = (list(arrays16), list(arrays32))
        if self.device is not None:
            self._upload()

    # ---- construction ------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, arrays: Dict[str, np.ndarray], device=None, fs: Optional[int] = None) -> "Corpus":
        """``arrays``: name -> 1-D int16 or float32 array."""
        n16, a16, n32, a32 = [], [], [], []
        for name, a in arrays.items():
            a = np.asarray(a)
            if a.ndim != 1 or a.dtype not in (np.int16, np.float32):
                raise ValueError(f"{name}: expected a 1-D int16 or float32 array, got {a.dtype} {a.shape}")
            (n16 if a.dtype == np.int16 else n32).append(name)
            (a16 if a.dtype == np.int16 else a32).append(np.ascontiguousarray(a))
        return cls(n16, a16, n32, a32, device=device, fs=fs)

    @classmethod
    def from_scp(cls, scps: Union[Dict[str, str], Sequence[str]], fs: int, device=None, resample: bool = False) -> "Corpus":
        """Read the reference's ``key path`` lists.  ``scps``: role -> scp file (a sequence gets the roles "0", "1", ...); the
        utterance of ``key`` in ``role`` is named ``f"{role}/{key}"`` and ``corpus.roles[role]`` lists the keys in file order (what
        ``random.choice`` draws from).  Files are read with ``infer.load_audio``; one whose samples are all ``k / 32768`` with ``k`` an
        int16 - every PCM16 file, for which ``librosa.load`` returns exactly that - is stored as int16, anything else as float32.  A
        file at another rate than ``fs`` raises unless ``resample`` is set, which converts it on the device (``resample.resample``;
        the result is float32)."""
        from .infer import load_audio
        if not isinstance(scps, dict):
            scps = {str(i): p for i, p in enumerate(scps)}
        arrays: Dict[str, np.ndarray] = {}
        roles: Dict[str, List[str]] = {}
        other: Dict[int, List[str]] = {}
        for role, scp in scps.items():
            table = parse_scp(scp)
            roles[role] = list(table)
            for key, path in table.items():
                x, sr = load_audio(path)
                name = f"{role}/{key}"
                if sr != int(fs):
                    if not resample:
                        raise RuntimeError(f"{path}: sampling rate {sr} != corpus rate {fs} (pass resample=True to convert it)")
                    other.setdefault(sr, []).append(name)
                    arrays[name] = x
                    continue
                k = x * np.float32(32768.0)
                pcm = np.clip(k, -32768.0, 32767.0).astype(np.int16)
                arrays[name] = pcm if np.array_equal(pcm.astype(np.float32), k) else x
        for sr, names in other.items():
            from .resample import resample as _resample
            ys = _resample([torch.from_numpy(arrays[nm]) for nm in names], sr, int(fs), device=device)
            for nm, y in zip(names, ys):
                arrays[nm] = y.cpu().numpy()
        out = cls.from_arrays(arrays, device=device, fs=int(fs))
        out.roles = roles
        return out

    def _upload(self) -> None:
        dev = self.device
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("a Corpus lives on the HIP device (there is no CPU path); device=None keeps the host layout only")
        a16, a32 = self._host

        def put(arrs, total, dtype, quantum):
            if not arrs:
                return None
            buf = torch.zeros((total + quantum - 1) // quantum * quantum, dtype=dtype, device=dev)      # allocated to a 16-byte multiple
            pos, group, held = 0, [], 0
            for a in arrs + [None]:
                if a is not None:
                    group.append(a)
                    held += a.shape[0]
                if group and (a is None or held >= (1 << 24)):
                    buf[pos:pos + held].copy_(torch.from_numpy(np.concatenate(group)))
                    pos, group, held = pos + held, [], 0
            return buf

        self.buf16 = put(a16, self.total16, torch.int16, 8)
        self.buf32 = put(a32, self.total32, torch.float32, 4)
        self.offsets = torch.from_numpy(self.offsets_host).to(dev)
        self._host = ([], [])
        lib = L_.load()
        N, n16 = len(self.names), self.n16
        ss16 = torch.zeros(max(n16, 1), dtype=torch.int64, device=dev)
        ss32 = torch.zeros(max(N - n16, 1), dtype=torch.float64, device=dev)
        ws = torch.empty(lib.sepr_corpus_energy_workspace(N), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            L_.check(lib.sepr_corpus_energy(*self._corpus_args(), ss16.data_ptr(), ss32.data_ptr(), ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream(dev).cuda_stream), "sepr_corpus_energy")
        self.set_energies(ss16[:n16].cpu().numpy(), ss32[:N - n16].cpu().numpy())      # the N energies, copied to the host once

    def _corpus_args(self):
        return (self.buf16.data_ptr() if self.buf16 is not None else None, self.total16,
                self.buf32.data_ptr() if self.buf32 is not None else None, self.total32, self.offsets.data_ptr(), self.n16, len(self.names))

    def set_energies(self, ss16: np.ndarray, ss32: np.ndarray) -> None:
        ss16, ss32 = np.asarray(ss16, dtype=np.int64), np.asarray(ss32, dtype=np.float64)
        if ss16.shape != (self.n16,) or ss32.shape != (len(self.names) - self.n16,):
            raise ValueError("one energy per utterance of each storage format")
        self.ss16, self.ss32 = ss16, ss32
        n = self.lengths.astype(np.float64)
        ms = np.concatenate([ss16.astype(np.float64) / (32768.0 ** 2 * n[:self.n16]), ss32 / n[self.n16:]])
        self._rms = np.sqrt(ms).astype(np.float32)

    @property
    def rms(self) -> np.ndarray:
        """float32 [N]: ``float32(sqrt(ss / (32768^2 n)))`` (int16) / ``float32(sqrt(ss / n))`` (float32), in float64 until the end."""
        if self._rms is None:
            raise RuntimeError("the corpus has no energies: they are computed on the HIP device at load (or given with set_energies)")
        return self._rms

    def __len__(self) -> int:
        return len(self.names)

    def lookup(self, role: str, key: str) -> int:
        return self.index[f"{role}/{key}"]


# ---- planners: the reference's draws, in the reference's order ----------------------------------------------------------------
def wsj0_distinct_speakers(key: str, key_random: str) -> bool:
    """``dataset.py:97-99`` of the WSJ0 variant: neither speaker id (first three letters of the 2nd / 4th ``_`` field) matches."""
    a, b = key.split('_'), key_random.split('_')
    return a[1][:3] != b[3][:3] and a[3][:3] != b[1][:3]


def _gain(rng: random.Random, lo: float, hi: float) -> np.float32:
    """``pow(10, -random.uniform(lo, hi) / 20)``; numpy multiplies a float32 array by the float32 value of a Python float."""
    return np.float32(pow(10, -rng.uniform(lo, hi) / 20))


def _norm(ref_rms: np.float32, cur_rms: np.float32) -> np.float32:
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(ref_rms) / np.float32(cur_rms)            # float32 divide, as ``ref_rms / curr_rms`` of two np.float32


def speed_ratio(speed: int) -> Tuple[int, int]:
    """``(L, M)`` of the converter of a speed in percent: ``L / M = 100 / speed`` in lowest terms (``resample.plan(speed, 100)``)."""
    speed = int(speed)
    if speed < 1:
        raise ValueError(f"a speed is a positive integer percentage, got {speed}")
    g = math.gcd(speed, 100)
    return 100 // g, speed // g


def parse_speeds(text: str) -> List[int]:
    """``"95:105"`` (an inclusive range) or ``"95,100,105"`` (a list) -> the speeds in percent."""
    if ":" in text:
        lo, hi = (int(v) for v in text.split(":"))
        out = list(range(lo, hi + 1))
    else:
        out = [int(v) for v in text.split(",") if v.strip()]
    if not out or min(out) < 1:
        raise ValueError(f"--speeds {text!r}: expected LO:HI or a comma list of positive integer percentages")
    return out


def perturbed_len(T: int, speed: int) -> int:
    """Samples of an utterance of ``T`` samples at ``speed`` percent: ``ceil(T L / M)``."""
    return int(T) if int(speed) == 100 else R_.out_len(T, *speed_ratio(speed))


def _draw_speeds(rng: random.Random, speeds: Optional[Sequence[int]], count: int) -> Optional[List[int]]:
    """One ``rng.choice(speeds)`` per source, in source order; no draw without speeds."""
    if speeds is None:
        return None
    return [int(rng.choice(speeds)) for _ in range(count)]


def _draw_rirs(rng: random.Random, rirs: Optional[RirBank], speeds, count: int, speed_reverb: bool = False) -> Optional[List[int]]:
    """One ``rng.randrange(len(rirs))`` per source, in source order; no draw without a bank.  With speeds it takes ``speed_reverb``."""
    if rirs is None:
        return None
    if speeds is not None and not speed_reverb:
        raise ValueError("speeds and rirs in one plan: pass one of them, or speed_reverb=True to perturb each source and then reverberate it")
    return [rng.randrange(len(rirs)) for _ in range(count)]


def _mix_rv(rirs: RirBank, rv: Sequence[int]) -> List[Tuple[int, int]]:
    """The mixture's (rir, taps) of the sources: the whole impulse response."""
    return [(r, int(rirs.lengths[r])) for r in rv]


def _target_rv(rirs: RirBank, rv: Sequence[int], target: Union[str, int]) -> List[Tuple[int, int]]:
    """The targets' (rir, taps): ``"direct"`` = the direct path of the same response (``rirs.direct_taps()``), ``"dry"`` = no response,
    ``"full"`` = the mixture's term, an integer = that many taps, clipped to the response's length."""
    if target == "direct":
        return [(r, int(rirs._direct[r])) for r in rv]
    if target == "dry":
        return [(-1, 1) for _ in rv]
    if target == "full":
        return _mix_rv(rirs, rv)
    if isinstance(target, (int, np.integer)) and not isinstance(target, bool) and int(target) >= 1:
        return [(r, min(int(target), int(rirs.lengths[r]))) for r in rv]
    raise ValueError(f"target = {target!r}: 'direct', 'dry', 'full' or a tap count >= 1")


def _same_device(a: Optional[torch.device], b: Optional[torch.device]) -> bool:
    """``cuda`` and ``cuda:<current>`` name one device."""
    if a is None or b is None or a.type != b.type:
        return False
    idx = lambda d: d.index if d.index is not None else (torch.cuda.current_device() if d.type == "cuda" else 0)      # noqa: E731
    return idx(a) == idx(b)


class Turns(NamedTuple):
    """What a planner is given to make partially overlapped talkers: ``overlap = (lo, hi)`` in [0, 1], the range the
    example's overlap ``rho`` is drawn from (1 = everybody talks throughout, today's mixture; 0 = back-to-back turns), and ``ramp``, the samples
    of the raised-cosine fade at either end of a turn (0 = a hard gate)."""
    overlap: Tuple[float, float] = (0.0, 1.0)
    ramp: int = 80


def parse_turns(text: str, ramp: int = 80) -> Turns:
    """``"0:1"`` (LO:HI) or ``"0.5"`` (one value) -> ``Turns``."""
    lo, _, hi = text.partition(":")
    return _check_turns(Turns((float(lo), float(hi if hi else lo)), int(ramp)))


def _check_turns(turns: Turns) -> Turns:
    lo, hi = (float(v) for v in turns.overlap)
    if not (0.0 <= lo <= hi <= 1.0):
        raise ValueError(f"turns: overlap = {turns.overlap!r}, expected 0 <= lo <= hi <= 1")
    if isinstance(turns.ramp, bool) or not isinstance(turns.ramp, (int, np.integer)) or not (0 <= int(turns.ramp) <= MAX_TURN_RAMP):
        raise ValueError(f"turns: ramp = {turns.ramp!r}, expected an integer in 0 .. {MAX_TURN_RAMP}")
    return turns


def turn_ramp(RL: int) -> np.ndarray:
    """The gate's table (include/sepr.h): float32 ``[RL]``, ``float32(0.5 - 0.5 cos(pi (i + 0.5) / RL))`` formed in float64."""
    RL = int(RL)
    if not (0 <= RL <= MAX_TURN_RAMP):
        raise ValueError(f"a ramp of {RL} samples: 0 .. {MAX_TURN_RAMP}")
    i = np.arange(RL, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / max(RL, 1))).astype(np.float32)


def _check_absent(absent: float, turns: Optional[Turns]) -> float:
    if isinstance(absent, bool) or not isinstance(absent, (int, float)) or not (0.0 <= float(absent) <= 1.0):
        raise ValueError(f"absent = {absent!r}, expected a probability in [0, 1]")
    if float(absent) > 0.0 and turns is None:
        raise ValueError("absent > 0 silences a talker by giving it the empty turn: it needs turns=Turns(...)")
    return float(absent)


def _lay_turns(order: Sequence[int], rho: float, n: int, out: List[Tuple[int, int]]) -> None:
    """The talkers of ``order`` laid over ``[0, n)`` with overlap ``rho`` (the rule of ``_draw_turns``); one talker alone gets the open turn."""
    k = len(order)
    if k == 1:
        out[order[0]] = (-TURN_FAR, TURN_FAR)
        return
    d = min(n, math.ceil(n / (k - (k - 1) * rho)))
    h = (n - d) // (k - 1)
    for s, who in enumerate(order):
        on, off = s * h, s * h + d
        out[who] = (-TURN_FAR if on <= 0 else on, TURN_FAR if off >= n or s == k - 1 else off)


def _draw_turns(rng: random.Random, turns: Optional[Turns], S: int, n: int, absent: float = 0.0) -> Optional[List[Tuple[int, int]]]:
    """The sources' turns of an example of ``n`` samples, in source order; no draw without ``turns``.  Two draws, after every other draw of the
    example: ``rho = rng.uniform(lo, hi)``, then the order of the talkers, ``rng.sample(range(S), S)``.  Every turn is
    ``d = min(n, ceil(n / (S - (S - 1) rho)))`` samples long and the s-th talker's begins at ``s h``, ``h = (n - d) // (S - 1)``: together they
    cover ``[0, n)``, neighbours overlap by ``d - h``, every source is active for at least ``n / S`` samples.  A turn that begins at or before
    sample 0 began before the window (``on = -TURN_FAR``: no fade-in, the history kept), one that reaches ``n`` - and the last talker's - goes on
    after it (``off = TURN_FAR``).  ``absent > 0``: two more draws after those two, ``rng.random() < absent`` and
    ``who = rng.randrange(S)`` - both made whatever the first says, so an example consumes the generator alike either way; when the first
    holds, talker ``who`` is silent throughout (the empty turn ``(TURN_FAR, TURN_FAR)``) and the other ``S - 1``, in their drawn order and with
    the same ``rho``, are laid over ``[0, n)`` by the same rule.  ``absent = 0`` draws nothing more."""
    absent = _check_absent(absent, turns)
    if turns is None:
        return None
    _check_turns(turns)
    rho = rng.uniform(float(turns.overlap[0]), float(turns.overlap[1]))
    order = rng.sample(range(S), S)
    out: List[Tuple[int, int]] = [(0, 0)] * S
    if absent > 0.0:
        gone, who = rng.random() < absent, rng.randrange(S)
        if gone:
            out[who] = _EMPTY
            order = [w for w in order if w != who]
    _lay_turns(order, rho, n, out)
    return out


_EMPTY = (TURN_FAR, TURN_FAR)                          # the turn of a talker who is silent throughout: on = off, nothing lies inside it
_OPEN = (-TURN_FAR, TURN_FAR)                          # the turn of a term that is not gated inside a plan with turns (the noise)
_NO_RIR = (-1, 1)                                      # a term that is not reverberated inside a plan with RIRs (the noise)


def _terms(utts, starts, norms, gains, sp, rv=None, tn=None) -> Tuple[Term, ...]:
    if tn is not None:
        k = len(tn)
        return tuple((u, s, nf, g, p, r, t, on, off)
                     for u, s, nf, g, p, (r, t), (on, off) in zip(utts, starts, norms, gains, sp or [100] * k, rv or [_NO_RIR] * k, tn))
    if rv is not None:
        return tuple((u, s, nf, g, p, r, k) for u, s, nf, g, p, (r, k) in zip(utts, starts, norms, gains, sp or [100] * len(rv), rv))
    if sp is None:
        return tuple((u, s, nf, g) for u, s, nf, g in zip(utts, starts, norms, gains))
    return tuple((u, s, nf, g, p) for u, s, nf, g, p in zip(utts, starts, norms, gains, sp))


def plan_wsj0(corpus: Corpus, rng: random.Random, key: str, max_len: int, srcs: Sequence[str] = ("s1", "s2"),
              accept: Callable[[str, str], bool] = wsj0_distinct_speakers, crop: bool = True,
              speeds: Optional[Sequence[int]] = None, rirs: Optional[RirBank] = None, target: Union[str, int] = "direct",
              speed_reverb: bool = False, turns: Optional[Turns] = None, absent: float = 0.0) -> Example:
    """``SepReformer_Large_DM_WSJ0/dataset.py:84-139``.  ``crop=False`` is the reference's "test" partition (no ``max_len`` crop).
    ``speeds``: directly after the draw that orders the two sources, one ``rng.choice(speeds)`` per source; the perturbed lengths
    replace the stored ones, the norm factors keep the stored utterances' RMS (section 5e-2).  ``rirs``: at that same position, one
    ``rng.randrange(len(rirs))`` per source; the mixture terms take the whole impulse response, the target terms what ``target`` says
    (``_target_rv``); lengths and norm factors stay the stored utterances' (section 5e-3).  Both take ``speed_reverb=True``: the speeds are
    drawn first, then the responses; every later draw uses the perturbed lengths; a source term is the perturbed utterance under the
    whole response and its target the same speed under what ``target`` says (section 5e-5).  ``turns``: after every other draw of the example,
    the two draws of ``_draw_turns``; each source's mixture term and its target carry the source's turn (section 5e-6).  ``absent``: the
    probability that one talker, drawn by ``_draw_turns`` after those, is silent throughout - its target and its mixture term carry the empty
    turn (section 5e-7); it needs ``turns``."""
    keys = corpus.roles[srcs[0]]
    while True:
        key_random = rng.choice(keys)
        if accept(key, key_random):
            break
    i1, i2 = (0, 1) if rng.random() > 0.5 else (1, 0)
    sp = _draw_speeds(rng, speeds, 2)
    rv = _draw_rirs(rng, rirs, speeds, 2, speed_reverb)
    utts = [corpus.lookup(srcs[i1], key), corpus.lookup(srcs[i2], key_random)]
    ref = corpus.rms[utts[0]]
    norms = [_norm(ref, corpus.rms[u]) for u in utts]
    gains = [_gain(rng, -5, 5) for _ in utts]
    lens = [perturbed_len(corpus.lengths[u], p) for u, p in zip(utts, sp or (100, 100))]
    min_len = min(lens)
    starts = [rng.randint(0, ln - min_len) for ln in lens]
    n = min_len - min_len % 4
    if crop and n > max_len:
        st = rng.randint(0, n - max_len)
        starts, n = [s + st for s in starts], max_len
    tn = _draw_turns(rng, turns, 2, n, absent)
    if rv is not None:
        return Example(key, n, _terms(utts, starts, norms, gains, sp, _mix_rv(rirs, rv), tn),
                       _terms(utts, starts, norms, gains, sp, _target_rv(rirs, rv, target), tn))
    terms = _terms(utts, starts, norms, gains, sp, None, tn)
    return Example(key, n, terms, terms)


def plan_wham(corpus: Corpus, rng: random.Random, key: str, max_len: int, srcs: Sequence[str] = ("s1", "s2"), noise: str = "noise",
              speeds: Optional[Sequence[int]] = None, rirs: Optional[RirBank] = None, target: Union[str, int] = "direct",
              speed_reverb: bool = False, turns: Optional[Turns] = None, absent: float = 0.0) -> Example:
    """``SepReformer_Large_DM_WHAM/dataset.py``: no speaker rule, the noise of ``key`` normalised to the first source with a gain of
    its own from U(-5, 5) dB, everything cropped to ``min(max_len, lengths)`` at independent random indices.  ``speeds``: as in
    ``plan_wsj0``; the noise is not perturbed.  ``rirs`` / ``target`` / ``speed_reverb``: as in ``plan_wsj0``; the noise is not
    reverberated.  ``turns`` / ``absent``: as in ``plan_wsj0``; the noise keeps the open turn."""
    key_random = rng.choice(corpus.roles[srcs[0]])
    i1, i2 = (0, 1) if rng.random() > 0.5 else (1, 0)
    sp = _draw_speeds(rng, speeds, 2)
    rv = _draw_rirs(rng, rirs, speeds, 2, speed_reverb)
    utts = [corpus.lookup(srcs[i1], key), corpus.lookup(srcs[i2], key_random)]
    ref = corpus.rms[utts[0]]
    norms = [_norm(ref, corpus.rms[u]) for u in utts]
    gains = [_gain(rng, -5, 5) for _ in utts]
    un = corpus.lookup(noise, key)
    norms.append(_norm(ref, corpus.rms[un]))
    gains.append(_gain(rng, -5, 5))
    utts.append(un)
    if sp is not None:
        sp.append(100)
    lens = [perturbed_len(corpus.lengths[u], p) for u, p in zip(utts, sp or (100, 100, 100))]
    min_len = min([max_len] + lens)
    starts = [rng.randint(0, ln - min_len) for ln in lens]
    n = min_len - min_len % 4
    tn = _draw_turns(rng, turns, 2, n, absent)
    tm = None if tn is None else tn + [_OPEN]
    if rv is not None:
        return Example(key, n, _terms(utts, starts, norms, gains, sp, _mix_rv(rirs, rv) + [_NO_RIR], tm),
                       _terms(utts[:2], starts, norms, gains, sp, _target_rv(rirs, rv, target), tn))
    terms = _terms(utts, starts, norms, gains, sp, None, tm)
    return Example(key, n, terms, terms[:2])


def plan_whamr(corpus: Corpus, rng: random.Random, key: str, max_len: int, srcs: Sequence[str] = ("s1", "s2"),
               reverb: Sequence[str] = ("s1_reverb", "s2_reverb"), noise: str = "noise", speeds: Optional[Sequence[int]] = None,
               rirs: Optional[RirBank] = None, target: Union[str, int] = "direct", speed_reverb: bool = False,
               turns: Optional[Turns] = None, absent: float = 0.0) -> Example:
    """``SepReformer_Large_DM_WHAMR/dataset.py:87-154``: the mixture is the two reverberant twins plus the noise (gains U(-3, 3) dB,
    noise U(-6, 3) dB), the targets are the anechoic sources with their twins' norm factor, gain and crop index.  ``speeds``: as in
    ``plan_wsj0``; a dry source and its reverberant twin share one speed, the noise is not perturbed.  ``rirs`` / ``target``: as in
    ``plan_wsj0``; the mixture is then the DRY sources reverberated in the launch plus the noise, and the ``reverb`` roles are never
    looked up - a corpus without pre-rendered twins serves.  ``speed_reverb=True`` with both: the dry sources perturbed and then
    reverberated in the launch (playing a pre-rendered twin faster, the other order, is ``speeds=`` alone).  ``turns`` / ``absent``: as in ``plan_wsj0``; the noise
    keeps the open turn.  With ``rirs`` the room rings on after a talker stops; without, a pre-rendered twin is gated as recorded, tail and all."""
    key_random = rng.choice(corpus.roles[srcs[0]])
    i1, i2 = (0, 1) if rng.random() > 0.5 else (1, 0)
    sp = _draw_speeds(rng, speeds, 2)
    rv = _draw_rirs(rng, rirs, speeds, 2, speed_reverb)
    dry = [corpus.lookup(srcs[i1], key), corpus.lookup(srcs[i2], key_random)]
    wet = dry if rv is not None else [corpus.lookup(reverb[i1], key), corpus.lookup(reverb[i2], key_random)]
    for d, w in zip(dry, wet):
        if corpus.lengths[d] != corpus.lengths[w]:
            raise ValueError(f"{corpus.names[d]} and {corpus.names[w]} differ in length (the reference stacks them)")
    ref = corpus.rms[dry[0]]
    norms = [_norm(ref, corpus.rms[u]) for u in dry]
    gains = [_gain(rng, -3, 3) for _ in dry]
    un = corpus.lookup(noise, key)
    nnorm, ngain = _norm(ref, corpus.rms[un]), _gain(rng, -6, 3)
    lens = [perturbed_len(corpus.lengths[u], p) for u, p in zip(dry, sp or (100, 100))]
    min_len = min([max_len] + lens + [int(corpus.lengths[un])])
    starts = [rng.randint(0, ln - min_len) for ln in lens]
    nstart = rng.randint(0, int(corpus.lengths[un]) - min_len)
    n = min_len - min_len % 4
    tn = _draw_turns(rng, turns, 2, n, absent)
    tm = None if tn is None else tn + [_OPEN]
    if rv is not None:
        return Example(key, n, _terms(dry + [un], starts + [nstart], norms + [nnorm], gains + [ngain], None if sp is None else sp + [100],
                                      _mix_rv(rirs, rv) + [_NO_RIR], tm),
                       _terms(dry, starts, norms, gains, sp, _target_rv(rirs, rv, target), tn))
    mix = _terms(wet + [un], starts + [nstart], norms + [nnorm], gains + [ngain], None if sp is None else sp + [100], None, tm)
    tgt = _terms(dry, starts, norms, gains, sp, None, tn)
    return Example(key, n, mix, tgt)


def plan_direct(corpus: Corpus, rng: random.Random, key: str, max_len: int, srcs: Sequence[str] = ("s1", "s2"), mix: str = "mix",
                crop: bool = True, speeds: Optional[Sequence[int]] = None, rirs: Optional[RirBank] = None) -> Example:
    """``_direct_load``: the fixed mixture file and its sources, norm and gain 1, the ``% 4`` truncation and the ``max_len`` crop.
    The mixture is one term; the kernel takes ``M >= S`` terms, so it is followed by terms of gain 0, which add exactly nothing.
    A fixed mixture cannot be perturbed or reverberated: ``speeds`` and ``rirs`` raise."""
    if speeds is not None:
        raise ValueError("plan_direct loads a fixed mixture file: it takes no speeds")
    if rirs is not None:
        raise ValueError("plan_direct loads a fixed mixture file: it takes no rirs")
    um = corpus.lookup(mix, key)
    n = int(corpus.lengths[um])
    n -= n % 4
    start = 0
    if crop and n > max_len:
        start, n = rng.randint(0, n - max_len), max_len
    tgt = tuple((corpus.lookup(r, key), start, _ONE, _ONE) for r in srcs)
    mixt = ((um, start, _ONE, _ONE),) + tuple((um, start, _ONE, np.float32(0.0)) for _ in srcs[1:])
    return Example(key, n, mixt, tgt)


def collate_plan(corpus: Corpus, examples: Sequence[Example], rirs: Optional[RirBank] = None, speed_reverb: bool = False,
                 turns: bool = False) -> BatchPlan:
    """Order the examples by length, longest first (``_collate``'s stable ``sorted(..., reverse=True)``), check every term against its
    utterance - at its speed - and, for a reverberant term, against the bank ``rirs``, and lay the table out as the kernel reads it.
    ``speed_reverb``: terms may carry a speed and a response; a plan with responses then has ``speed``, ``rir`` and ``taps`` all set, whatever
    speeds were drawn (so the batches of one feed share one table layout and one entry).  A term that carries a turn (a 9-tuple) gives the plan
    its ``on`` and ``off`` columns, a term without one the open turn; ``turns``: the plan has the columns whatever its terms carry.  In such a
    plan a term's speed and response count only where they are set (a speed other than 100, a response index >= 0)."""
    egs = sorted(examples, key=lambda e: e.n, reverse=True)
    M, S = len(egs[0].mix), len(egs[0].tgt)
    if not (2 <= S <= 3 and S <= M <= S + 1):
        raise ValueError(f"{M} mixture terms and {S} target terms: the kernel takes S in 2..3 and M in S..S+1")
    B = len(egs)
    utt, start = np.zeros((B, M + S), np.int32), np.zeros((B, M + S), np.int32)
    norm, gain = np.zeros((B, M + S), np.float32), np.zeros((B, M + S), np.float32)
    speed = np.full((B, M + S), 100, np.int32)
    rir, taps = np.full((B, M + S), -1, np.int32), np.ones((B, M + S), np.int32)
    on, off = np.full((B, M + S), -TURN_FAR, np.int32), np.full((B, M + S), TURN_FAR, np.int32)
    any_speed = any_rir = False
    any_turn = bool(turns)
    for b, e in enumerate(egs):
        if len(e.mix) != M or len(e.tgt) != S:
            raise ValueError("every example of a batch needs the same number of terms")
        if e.n < 1:
            raise ValueError(f"{e.key}: an example of {e.n} samples")
        for j, term in enumerate(e.mix + e.tgt):
            u, s, nf, g = term[:4]
            p = int(term[4]) if len(term) > 4 else 100
            any_speed |= len(term) == 5 or p != 100
            if len(term) > 7:
                any_turn = True
                on[b, j], off[b, j] = max(-TURN_FAR, min(TURN_FAR, int(term[7]))), max(-TURN_FAR, min(TURN_FAR, int(term[8])))
            if len(term) > 5 and (len(term) == 7 or int(term[5]) >= 0):
                any_rir = True
                r, k = int(term[5]), int(term[6])
                if rirs is None:
                    raise ValueError(f"{e.key}: term {j} carries an RIR, collate_plan was given no bank (rirs=)")
                if not (-1 <= r < len(rirs)) or (r >= 0 and not (1 <= k <= int(rirs.lengths[r]))):
                    raise ValueError(f"{e.key}: term {j} takes {k} taps of RIR {r}; the bank holds {len(rirs)}"
                                     + (f", this one {int(rirs.lengths[r])} samples" if 0 <= r < len(rirs) else ""))
                rir[b, j], taps[b, j] = r, k
            if not (0 <= u < len(corpus)) or p < 1 or s < 0 or s + e.n > perturbed_len(corpus.lengths[u], p):
                raise ValueError(f"{e.key}: term {j} reads [{s}, {s + e.n}) of utterance {u}" + (f" at {p} % speed" if p != 100 else ""))
            utt[b, j], start[b, j], norm[b, j], gain[b, j], speed[b, j] = u, s, nf, g, p
    if any_speed and any_rir and not speed_reverb:
        raise ValueError("a plan with speeds and RIRs takes speed_reverb=True (each source perturbed, then reverberated)")
    any_speed |= any_rir and speed_reverb
    return BatchPlan([e.key for e in egs], np.array([e.n for e in egs], np.int32), utt, start, norm, gain, M, S, speed if any_speed else None,
                     rir if any_rir else None, taps if any_rir else None, on=on if any_turn else None, off=off if any_turn else None)


def table_layout(B: int, NT: int, speeds: bool = False, rirs: bool = False, turns: bool = False) -> Dict[str, Tuple[int, int]]:
    """The device table of a plan, the one place that says where its blocks lie: name -> (first int32 word, words), in memory order
    ``utt | start | norm | gain | n``, then ``conv`` for a plan with speeds, then ``rir | taps`` for one with RIRs.  A plan with turns has one
    layout whatever else it carries - its one entry reads every column: ``... | conv | rir | taps | on | off``."""
    speeds, rirs = speeds or turns, rirs or turns
    names = ("utt", "start", "norm", "gain", "n") + (("conv",) if speeds else ()) + (("rir", "taps") if rirs else ()) + (("on", "off") if turns else ())
    words = [B if name == "n" else B * NT for name in names]
    return {name: (sum(words[:k]), words[k]) for k, name in enumerate(names)}


def _table_words(B: int, NT: int, speeds: bool = False, rirs: bool = False, turns: bool = False) -> int:
    return sum(words for _, words in table_layout(B, NT, speeds, rirs, turns).values())


def _plan_layout(plan: BatchPlan) -> Tuple[int, int, bool, bool, bool]:
    """The arguments of ``table_layout`` for ``plan``."""
    return (*plan.utt.shape, plan.speed is not None, plan.rir is not None, plan.on is not None)


def ramp_table(dev, RL: int) -> torch.Tensor:
    """``turn_ramp(RL)`` on ``dev``: the gate's table as ``mix_batch`` takes it (``ramp=``).  One host-to-device copy - a feed makes it once, when
    it is built; make it before a graph capture, not inside one."""
    return torch.from_numpy(turn_ramp(RL)).to(dev)


def plan_speeds(plan: BatchPlan) -> List[int]:
    """The distinct speeds other than 100 of a plan, ascending: the default converter set of ``pack_table`` and ``mix_batch``."""
    return [] if plan.speed is None else sorted({int(p) for p in plan.speed.ravel()} - {100})


_converters: Dict[Tuple[str, Tuple[int, ...]], tuple] = {}


def _converter_args(dev: torch.device, speeds: Sequence[int]):
    """The converter arguments of ``sepr_dynmix_speed_fwd`` for ``speeds`` (converter k = ``resample.plan(speeds[k], 100)``): the tables
    are built once per (device, speed) and stay on the device (``resample._table``), the host arrays once per (device, set)."""
    key = (str(dev), tuple(int(p) for p in speeds))
    if key not in _converters:
        _converters[key] = R_.converter_args([R_._table(p, 100, dev) for p in key[1]])
    return _converters[key]


def mix_batch(corpus: Corpus, plan: BatchPlan, Tmax: Optional[int] = None, mix: Optional[torch.Tensor] = None,
              src: Optional[Sequence[torch.Tensor]] = None, table: Optional[torch.Tensor] = None,
              speeds: Optional[Sequence[int]] = None, rirs: Optional[RirBank] = None,
              ramp: Union[int, torch.Tensor, None] = None):
    """One ``sepr_dynmix_fwd`` launch for ``plan`` on the corpus's device (current stream) -> ``(mix [B, Tmax], [src_s [B, Tmax]])``;
    a plan that carries speeds goes through ``sepr_dynmix_speed_fwd``, one that carries RIRs through ``sepr_dynmix_reverb_fwd`` with the
    bank ``rirs``, which must be on the corpus's device, one that carries both through ``sepr_dynmix_speed_reverb_fwd``.  ``table``: an int32 device tensor that already holds the plan in
    the kernel's layout (``DynamicMixFeed`` stages it through pinned memory); without it the plan is copied from pageable memory.
    ``speeds``: the converter set the table's index block refers to (``pack_table``); default: the plan's own speeds.  A captured launch
    keeps the set it was captured with, so a table rewritten between replays must be packed against that set.  A plan that carries turns
    (``plan.on``) always goes through ``sepr_dynmix_turns_fwd``, whatever else it carries, with the gate's table ``ramp`` (required for such a
    plan): the device tensor ``ramp_table(device, RL)``, or the length ``RL`` itself (0 = a hard gate), which uploads the table in this call -
    one pageable copy per call, so a captured launch and a loop pass the tensor."""
    dev = corpus.device
    if dev is None:
        raise RuntimeError("the corpus is not on the HIP device (there is no CPU path)")
    B, NT = plan.utt.shape
    Tmax = int(Tmax if Tmax is not None else -(-int(plan.n.max()) // 4) * 4)
    if Tmax % 4 or int(plan.n.max()) > Tmax:
        raise ValueError(f"Tmax = {Tmax} must be a multiple of 4 and hold the longest example ({int(plan.n.max())})")
    if plan.rir is not None:
        if rirs is None:
            raise ValueError("the plan carries RIRs: pass the bank (rirs=)")
        if not _same_device(rirs.device, dev):
            raise ValueError(f"the RIR bank is on {rirs.device}, the corpus on {dev}")
    if plan.on is not None:
        if isinstance(ramp, (int, np.integer)) and not isinstance(ramp, bool) and 0 <= int(ramp) <= MAX_TURN_RAMP:
            ramp = ramp_table(dev, int(ramp))
        if not isinstance(ramp, torch.Tensor) or ramp.dtype != torch.float32 or ramp.dim() != 1 or ramp.numel() > MAX_TURN_RAMP \
                or not ramp.is_contiguous() or not _same_device(ramp.device, dev):
            raise ValueError(f"the plan carries turns: pass the gate's ramp (ramp_table(device, RL), or RL = 0 .. {MAX_TURN_RAMP}), got {ramp!r}")
    if table is None:
        table = torch.from_numpy(pack_table(plan, speeds)).to(dev)
    if table.numel() < _table_words(*_plan_layout(plan)):
        raise ValueError("the device table is shorter than the plan's layout")
    if mix is None:
        mix = torch.empty(B, Tmax, dtype=torch.float32, device=dev)
    if src is None:
        block = torch.empty(plan.S, B, Tmax, dtype=torch.float32, device=dev)
        src = [block[s] for s in range(plan.S)]
    for t in [mix] + list(src):
        if tuple(t.shape) != (B, Tmax) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"outputs must be contiguous float32 [{B}, {Tmax}] tensors on {dev}")
    if len(src) != plan.S:
        raise ValueError(f"{plan.S} target rows expected")
    at = {name: table.data_ptr() + 4 * first for name, (first, _) in table_layout(*_plan_layout(plan)).items()}
    rows = (C.c_void_p * plan.S)(*[t.data_ptr() for t in src])
    entry, cols, own = "sepr_dynmix_fwd", (), ()        # the entry, the table columns of its form, the form's own arguments
    if plan.on is not None:
        entry, cols = "sepr_dynmix_turns_fwd", (at["conv"], at["rir"], at["taps"], at["on"], at["off"])
        own = (*_converter_args(dev, plan_speeds(plan) if speeds is None else speeds),
               *(rirs._bank_args() if plan.rir is not None else (None, 0, None, 0)), ramp.data_ptr() if ramp.numel() else None, ramp.numel())
    elif plan.rir is not None and plan.speed is not None:
        entry, cols = "sepr_dynmix_speed_reverb_fwd", (at["conv"], at["rir"], at["taps"])
        own = (*_converter_args(dev, plan_speeds(plan) if speeds is None else speeds), *rirs._bank_args())
    elif plan.rir is not None:
        entry, cols, own = "sepr_dynmix_reverb_fwd", (at["rir"], at["taps"]), rirs._bank_args()
    elif plan.speed is not None:
        entry, cols, own = "sepr_dynmix_speed_fwd", (at["conv"],), _converter_args(dev, plan_speeds(plan) if speeds is None else speeds)
    with torch.cuda.device(dev):
        L_.check(getattr(L_.load(), entry)(*corpus._corpus_args(), at["utt"], at["start"], at["norm"], at["gain"], *cols, at["n"], B, plan.M, plan.S,
                                           Tmax, mix.data_ptr(), rows, *own, torch.cuda.current_stream(dev).cuda_stream), entry)
    return mix, list(src)


def pack_table(plan: BatchPlan, speeds: Optional[Sequence[int]] = None) -> np.ndarray:
    """The plan as one int32 array in the order of ``table_layout`` (``norm`` and ``gain`` as their bits).  The ``conv`` block of a plan that
    carries speeds: -1 for a term at 100 %, else the position of the term's speed in ``speeds`` (default ``plan_speeds(plan)``).  A plan with turns
    has every column: ``conv`` and ``rir`` are -1 and ``taps`` 1 where it carries no speeds or no RIRs."""
    blocks = {"utt": plan.utt, "start": plan.start, "norm": plan.norm.view(np.int32), "gain": plan.gain.view(np.int32), "n": plan.n,
              "rir": plan.rir, "taps": plan.taps, "on": plan.on, "off": plan.off}
    if plan.on is not None:
        blocks["conv"] = np.full_like(plan.utt, -1)
        if plan.rir is None:
            blocks["rir"], blocks["taps"] = np.full_like(plan.utt, -1), np.ones_like(plan.utt)
    if plan.speed is not None:
        order = [int(p) for p in (plan_speeds(plan) if speeds is None else speeds)]
        index = {**{p: k for k, p in enumerate(order)}, 100: -1}
        missing = sorted({int(p) for p in plan.speed.ravel()} - set(index))
        if missing:
            raise ValueError(f"speeds {missing} of the plan are not in the converter set {order}")
        blocks["conv"] = np.array([index[int(p)] for p in plan.speed.ravel()], np.int32)
    layout = table_layout(*_plan_layout(plan))
    return np.concatenate([blocks[name].ravel().astype(np.int32, copy=False) for name in layout])


class FeedOrder:
    """The host-only half of a feed: the ``random.Random`` that permutes the keys and makes the planners' draws, the epoch counter, the
    shard and the batch boundaries.  It needs no device, and it is what a checkpoint keeps of a feed (``state_dict``): written at an
    epoch boundary, a fresh object that loads it yields the next epoch's key order and the same planner draws.  (The simulated-rooms
    bank follows from ``(seed, epoch)``, so the epoch counter covers it.)"""

    def __init__(self, default_keys: Optional[Sequence[str]], batch: int, seed=0, keys: Optional[Sequence[str]] = None,
                 rank: int = 0, world: int = 1, drop_last: bool = True, fixed_length: bool = False):
        from .dist import shard_range
        shard_range(1, rank, world)                     # validates rank / world
        if batch < 1:
            raise ValueError("batch >= 1")
        if fixed_length and not drop_last:
            raise ValueError("drop_last=False yields a smaller last batch: variable-length mode only (fixed_length rows feed static tensors)")
        self.batch, self.seed, self.rank, self.world, self.drop_last = int(batch), seed, rank, world, bool(drop_last)
        self.rng = random.Random(seed)
        self.epoch = 0
        self.keys = None if keys is None else list(keys)
        self.default_keys = None if default_keys is None else list(default_keys)
        if self.keys is None and self.default_keys is None:
            raise ValueError("the corpus has no roles (it was not read from scp lists): pass keys=")

    def epoch_order(self) -> List[str]:
        if self.keys is not None:
            order = list(self.keys)
        else:
            order = list(self.default_keys)
            self.rng.shuffle(order)
        from .dist import shard_range
        lo, hi = shard_range(len(order), self.rank, self.world)
        return order[lo:hi]

    def batches(self, order: Sequence[str]) -> List[List[str]]:
        """The epoch's batches of keys: full ones, then - with ``drop_last=False`` - the remainder as a last, smaller one."""
        full = len(order) - len(order) % self.batch
        out = [list(order[i:i + self.batch]) for i in range(0, full, self.batch)]
        if not self.drop_last and full < len(order):
            out.append(list(order[full:]))
        return out

    def state_dict(self) -> dict:
        return {"rng": self.rng.getstate(), "epoch": int(self.epoch), "seed": self.seed}

    def load_state_dict(self, state: dict) -> None:
        version, words, gauss = state["rng"]
        self.rng.setstate((int(version), tuple(int(w) for w in words), gauss))      # (a list after a round trip through a file)
        self.epoch = int(state["epoch"])


class DynamicMixFeed:
    """``for input_sizes, mixture, src, key in feed`` - the reference's ``_collate`` tuple (``input_sizes`` float32 on the host,
    ``mixture [B, T]`` and the ``S`` tensors ``src[s] [B, T]`` on the device, the keys), one epoch per iteration.

    ``planner(corpus, rng, key, max_len) -> Example`` is one of ``plan_wsj0`` / ``plan_wham`` / ``plan_whamr`` / ``plan_direct`` (bind
    other role names, or ``speeds=range(95, 106)`` for speed perturbation, with ``functools.partial``; for reverberation bind ``rirs=bank`` and
    pass the same bank as the feed's ``rirs=``; for both bind ``speed_reverb=True`` as well - the feed reads the flag from the
    ``functools.partial`` and passes it to ``collate_plan``; a planner wrapped otherwise says it with the feed's ``speed_reverb=``; for turn-taking
    bind ``turns=Turns(...)``, which the feed reads the same way - or takes as its own ``turns=`` - for the gate's ramp table; ``absent=P`` bound beside it is kept as ``feed.absent``).  Per batch: plan on the host, write the table into a pinned staging buffer, one
    asynchronous copy into the static device table, one launch - all on the current stream, nothing waits for the device.
    ``keys``: the epoch's key order, used as given every epoch; default: the keys of the corpus's first role, permuted with the
    feed's ``random.Random(seed)`` before each epoch (the same generator then makes the examples' draws).  ``rank`` / ``world``:
    this rank's contiguous shard of the key order (``dist.shard_range``).  A trailing partial batch is dropped; ``drop_last=False``
    yields it as a last, smaller batch (the reference's validation loader) - variable-length mode only: static tensors have one
    shape, so with ``fixed_length`` it is refused.  ``state_dict()`` / ``load_state_dict()``: the generator's state and the epoch
    counter (``FeedOrder``, which holds the feed's host-only state), for a checkpoint written between epochs.
    ``fixed_length``: every row is ``max_len`` samples, shorter examples zero-padded - constant shapes, which a
    ``CapturedTrainStep`` needs; ``next_into(x, targets)`` then writes the next batch straight into the step's static tensors.
    ``rooms`` (a ``reverb.RoomSampler``, with ``rirs=RirBank.simulate(...)``): every ``rooms_every``-th epoch, the first included, begins by
    re-simulating the bank in place from ``rooms.draw(len(rirs), seed=(seed, epoch))``, so an utterance does not meet
    the same room in every epoch; ``rooms=None`` changes nothing."""

    SLOTS = 4               # pinned staging buffers in flight

    def __init__(self, corpus: Corpus, planner: Callable[..., Example], batch: int, max_len: int, seed: int = 0,
                 keys: Optional[Sequence[str]] = None, fixed_length: bool = False, rank: int = 0, world: int = 1,
                 rirs: Optional[RirBank] = None, rooms=None, rooms_every: int = 1, speed_reverb: Optional[bool] = None,
                 drop_last: bool = True, turns: Optional[Turns] = None):
        if corpus.device is None:
            raise RuntimeError("DynamicMixFeed needs a corpus on the HIP device (there is no CPU path)")
        if rirs is not None and not _same_device(rirs.device, corpus.device):
            raise ValueError(f"the RIR bank is on {rirs.device}, the corpus on {corpus.device}")
        if batch < 1 or max_len < 4:
            raise ValueError("batch >= 1 and max_len >= 4")
        if fixed_length and max_len % 4:
            raise ValueError("fixed_length needs max_len to be a multiple of 4")
        self.order = FeedOrder(list(next(iter(corpus.roles.values()))) if corpus.roles else None, batch, seed, keys, rank, world, drop_last,
                               fixed_length=fixed_length)     # (refuses drop_last=False with fixed_length)
        self.corpus, self.planner, self.batch, self.max_len = corpus, planner, int(batch), int(max_len)
        self.fixed_length, self.rank, self.world, self.rirs = bool(fixed_length), rank, world, rirs
        if rooms is not None:
            if rirs is None or getattr(rirs, "_sim", None) is None:
                raise ValueError("rooms= redraws a simulated bank: pass rirs=RirBank.simulate(...)")
            if int(rooms_every) < 1:
                raise ValueError("rooms_every >= 1")
            if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or int(seed) < 0:
                raise ValueError("rooms= needs a non-negative integer seed (the rooms of an epoch are drawn from (seed, epoch))")
        self.rooms, self.rooms_every, self.seed = rooms, int(rooms_every), seed
        if speed_reverb is None:                        # the flag the user bound on the planner
            speed_reverb = (getattr(planner, "keywords", None) or {}).get("speed_reverb", False)
        self.speed_reverb = bool(speed_reverb)
        if turns is None:                               # the turns the user bound on the planner, read as speed_reverb is
            turns = (getattr(planner, "keywords", None) or {}).get("turns")
        self.turns = None if turns is None else _check_turns(turns)
        # the probability of a silent talker the user bound on the planner (section 5e-7): what a trainer asks before it picks a criterion
        self.absent = _check_absent((getattr(planner, "keywords", None) or {}).get("absent", 0.0), self.turns)
        self._ramp = None if self.turns is None else ramp_table(corpus.device, int(self.turns.ramp))      # once per feed and device
        self._table = None
        self._speeds: List[int] = []                    # the converter set: every speed a plan has used, in order of first use
        self._stage: List[torch.Tensor] = []
        self._events: List[Optional[torch.cuda.Event]] = []
        self._slot = 0
        self._epoch: Optional[Iterator[BatchPlan]] = None
        self.last_plan: Optional[BatchPlan] = None

    # ---- host side ---------------------------------------------------------------------------------------------------------
    rng = property(lambda self: self.order.rng)
    keys = property(lambda self: self.order.keys)
    epoch = property(lambda self: self.order.epoch, lambda self, v: setattr(self.order, "epoch", int(v)))

    def epoch_order(self) -> List[str]:
        return self.order.epoch_order()

    def state_dict(self) -> dict:
        """What a checkpoint written between epochs keeps of the feed (``FeedOrder.state_dict``)."""
        return self.order.state_dict()

    def load_state_dict(self, state: dict) -> None:
        self.order.load_state_dict(state)
        self._epoch = None                              # a batch iterator in flight belonged to the state that was replaced

    def _begin_epoch(self) -> None:
        """With ``rooms=``: before the first plan of every ``rooms_every``-th epoch the bank is re-simulated in place from
        ``rooms.draw(len(bank), seed=(seed, epoch))`` - numpy's generator, so the planners' ``random.Random`` makes the draws it would make
        without ``rooms``.  The epoch's plans then read the new ``_direct``; the launches of the epoch before are already queued."""
        epoch, self.epoch = self.epoch, self.epoch + 1
        if self.rooms is not None and epoch % self.rooms_every == 0:
            self.rirs.resimulate(self.rooms.draw(len(self.rirs), seed=(int(self.seed), epoch)))

    def plans(self) -> Iterator[BatchPlan]:
        """The batch plans of one epoch (host only - except with ``rooms=``, where the epoch begins by simulating its rooms on the device)."""
        self._begin_epoch()
        order = self.epoch_order()
        for keys in self.order.batches(order):
            yield collate_plan(self.corpus, [self.planner(self.corpus, self.rng, k, self.max_len) for k in keys], self.rirs, self.speed_reverb,
                               self.turns is not None)

    # ---- device side -------------------------------------------------------------------------------------------------------
    def _launch(self, plan: BatchPlan, mix=None, src=None):
        dev = self.corpus.device
        words = _table_words(*_plan_layout(plan))
        self._speeds += [p for p in plan_speeds(plan) if p not in self._speeds]
        if self._table is None or self._table.numel() != words:
            self._table = torch.empty(words, dtype=torch.int32, device=dev)
            self._stage = [torch.empty(words, dtype=torch.int32).pin_memory() for _ in range(self.SLOTS)]
            self._events = [None] * self.SLOTS
        k = self._slot
        self._slot = (k + 1) % self.SLOTS
        if self._events[k] is not None:
            self._events[k].synchronize()               # the copy that last read this staging buffer has run (SLOTS batches ago)
        self._stage[k].numpy()[:] = pack_table(plan, self._speeds)
        self._table.copy_(self._stage[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self._events[k] = ev
        self.last_plan = plan
        return mix_batch(self.corpus, plan, self.max_len if self.fixed_length else None, mix, src, table=self._table, speeds=self._speeds,
                         rirs=self.rirs, ramp=self._ramp)

    def __iter__(self):
        for plan in self.plans():
            mix, src = self._launch(plan)
            yield torch.from_numpy(plan.n.astype(np.float32)), mix, src, plan.keys

    def next_plan(self) -> BatchPlan:
        """The next batch plan, running on into the next epoch when one ends."""
        for _ in range(2):
            if self._epoch is None:
                self._epoch = self.plans()
            plan = next(self._epoch, None)
            if plan is not None:
                return plan
            self._epoch = None
        raise ValueError(f"an epoch of this shard holds fewer than {self.batch} keys")

    def write(self, plan: BatchPlan, x: torch.Tensor, targets: Sequence[torch.Tensor]) -> None:
        """Write the batch of ``plan`` (one of ``plans()``) into ``x`` and ``targets``: what ``next_into`` does with the plan it drew, for a
        loop that walks exactly one epoch (``trainer.Trainer``)."""
        if not self.fixed_length:
            raise ValueError("write needs fixed_length=True (static tensors have one shape)")
        self._launch(plan, x, list(targets)[:plan.S])

    def next_into(self, x: torch.Tensor, targets: Sequence[torch.Tensor]) -> BatchPlan:
        """Write the next batch into ``x [B, max_len]`` and ``targets`` (``S`` tensors ``[B, max_len]``), e.g. ``step.x`` and
        ``step.targets`` of a ``CapturedTrainStep``.  Returns the plan (``plan.n``: the lengths, ``plan.keys``)."""
        if not self.fixed_length:
            raise ValueError("next_into needs fixed_length=True (static tensors have one shape)")
        plan = self.next_plan()
        self._launch(plan, x, list(targets)[:plan.S])
        return plan
