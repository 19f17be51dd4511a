#!/usr/bin/env python3
"""Dynamic-mixing feed beside the training step it feeds (sepreformer_amd/datafeed.py).

  1. device time of one ``sepr_dynmix_fwd`` launch: hipEvents around each of 100 launches after warm-up (median, min, max), B = 16 and
     32 x 4 s, in the WSJ0 form (2 terms) and the WHAMR form (5 terms), on a synthetic PCM16 corpus resident on the device;
  2. in the same process: a ``CapturedTrainStep`` loop (Base, bf16, batch 16, the reference's loss, FlatAdamW) on a fixed batch against
     the same loop fed by ``DynamicMixFeed.next_into`` - alternating, three runs each, ms per step;
  3. the reference-form numpy mixing (decode, RMS, scale, crop, sum) from RAM-resident int16 arrays on a 16-thread pool, in utt/s
     (reported only).

Conditions of section 5e: the WHAMR-form launch at B = 16 takes at most 1 % of the fixed-batch step time of THIS run; the mean of the
fed runs exceeds the mean of the fixed runs by at most the larger within-setting spread (max - min) of this run.

``--speeds 95:105`` measures speed perturbation instead (section 5e-2), in one child process with the settings alternating: the plain
launch against the launch with every source term perturbed (WSJ0 form, S = 2, B = 16 and 32 x 4 s), and the bf16 training step fed
without and with speeds; the step without speeds of that same run is the yardstick.

``--rirs 64:0.6`` measures reverberation by convolution instead (section 5e-3), in one child process with the settings alternating: the
plain WHAMR-form launch (5 terms) against the reverberant form (3 mixture terms, the two sources under a whole impulse response, and 2
direct-path targets) at RT60 = 0.3, 0.6 and 1.0 s, B = 16 and 32 x 4 s; and the bf16 training step fed plainly and fed with
reverberation from COUNT synthetic responses of RT60 seconds; the plainly fed step of that same run is the yardstick.

``--room-rirs 64:0.2:0.6`` measures simulating a bank of shoebox rooms on the device instead (section 5e-4), in one child process: the
hipEvent time of one ``sepr_rir_ism_fwd`` call for COUNT rooms, the numpy restatement's CPU time for one room, the realised decay of a few
responses beside the nominal RT60, and the bf16 training step fed from a fixed simulated bank against the same feed re-simulating its
rooms every epoch (three steps here), alternating.  Condition: one simulation takes less than one training step of the same run.

``--turns LO:HI`` measures turn-taking (section 5e-6) on top of whatever ``--speeds`` and ``--rirs`` say, in one child process with the settings
alternating: the launch of the plan without turns through the entry it has today beside the launch of the same planner with
``turns=Turns((LO, HI))`` through ``sepr_dynmix_turns_fwd``, and the bf16 training step fed without and with turns.  ``--turns 1:1`` is the new
entry at full overlap - the cost of the gate's code - and ``--turns 0:1`` what sparse overlap saves through the skipped tiles and chunks.

``--speeds 95:105 --rirs 64:0.6`` together measure both in one source (section 5e-5), in one child process with the settings alternating:
the combined launch (each source perturbed, then under a whole response of RT60 seconds; direct-path targets at the same speed) beside the
reverb-only and the speed-only launch of the same plan shapes (WHAMR form, B = 16 and 32 x 4 s), and the bf16 training step fed with
reverberation alone and with both; the reverb-fed step of that same run is the yardstick.

Every step runs in a child process of its own under ``timeout -k 10 <s>``; the first step that fails ends the run.

    python tools/dynmix_bench.py [--out profiles/dynmix_timing.json]
    python tools/dynmix_bench.py --speeds 95:105 [--out profiles/dynmix_speed.json]
    python tools/dynmix_bench.py --rirs 64:0.6 [--out profiles/dynmix_reverb.json]
    python tools/dynmix_bench.py --room-rirs 64:0.2:0.6 [--out profiles/rir_ism.json]
    python tools/dynmix_bench.py --speeds 95:105 --rirs 64:0.6 [--out profiles/dynmix_speed_reverb.json]
    python tools/dynmix_bench.py [--speeds 95:105] [--rirs 64:0.6] --turns 0:1
"""
import argparse
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, T4S = 8000, 32000
NKEYS = 48
STEPS = [("device", 780), ("host", 300)]
LOOP_STEPS, LOOP_RUNS = 20, 3
ROLES = ("s1", "s2", "s1_reverb", "s2_reverb", "noise")


def _stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "mean": sum(v) / len(v)}


def synth_corpus_arrays():
    """name -> int16 array: NKEYS keys x 5 roles of 4.5 - 8 s (pseudo-random PCM16; the kernel's time does not depend on the values)."""
    import numpy as np
    rng = np.random.default_rng(0)
    keys = [f"k{i:03d}a_0.{i:04d}_k{i:03d}b_-0.{i:04d}" for i in range(NKEYS)]
    arrays = {}
    for i, k in enumerate(keys):
        n = int(rng.integers(36000, 64000))
        for r in ROLES:
            m = n if r != "noise" else int(rng.integers(36000, 64000))
            arrays[f"{r}/{k}"] = rng.integers(-6000, 6000, size=m, dtype=np.int16)
    return keys, arrays


def step_device():
    import functools
    import numpy as np
    import torch
    from sepreformer_amd import datafeed as df
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.train_step import CapturedTrainStep
    dev = torch.device("cuda:0")
    keys, arrays = synth_corpus_arrays()
    corpus = df.Corpus.from_arrays(arrays, device=dev, fs=FS)
    corpus.roles = {r: list(keys) for r in ROLES}
    forms = {"wsj0": functools.partial(df.plan_wsj0, accept=lambda a, b: True), "whamr": df.plan_whamr}
    kernel = []
    for form, planner in forms.items():
        for B in (16, 32):
            rng = random.Random(B)
            plan = df.collate_plan(corpus, [planner(corpus, rng, keys[i % NKEYS], T4S) for i in range(B)])
            table = torch.from_numpy(df.pack_table(plan)).to(dev)
            mix = torch.empty(B, T4S, device=dev)
            src = [torch.empty(B, T4S, device=dev) for _ in range(plan.S)]
            ms = []
            for i in range(20 + 100):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                df.mix_batch(corpus, plan, T4S, mix, src, table=table)
                e1.record()
                torch.cuda.synchronize()
                if i >= 20:
                    ms.append(e0.elapsed_time(e1))
            # and back to back, without an event pair per launch
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                df.mix_batch(corpus, plan, T4S, mix, src, table=table)
            e1.record()
            torch.cuda.synchronize()
            terms = plan.M + (0 if form == "wsj0" else plan.S)
            nbytes = int(plan.n.sum()) * 2 * terms + B * T4S * 4 * (1 + plan.S)
            med = _stats(ms)["median"]
            kernel.append({"form": form, "B": B, "samples": T4S, "terms_read": terms, "device_ms": _stats(ms), "launches": 100,
                           "back_to_back_ms_per_launch": e0.elapsed_time(e1) / 100, "algorithmic_bytes": nbytes,
                           "GBs_at_median": nbytes / (med * 1e-3) / 1e9})
    # ---- the training step: fixed batch against fed, same process, alternating
    B = 16
    cfg = VARIANTS["SepReformer_Base_WSJ0"]
    torch.manual_seed(0)
    model = Model.from_config(cfg, init_seed=0, precision="bf16").load_synthetic_(0).to(dev).train()
    crit_t = PIT_SISNR_time(dev, cfg.num_spks, True)
    crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, cfg.num_spks, True, False)
    sizes = torch.full((B,), T4S)
    opt = FlatAdamW(model, lr=1.0e-4, weight_decay=1.0e-2)

    def loss_fn(audio, aux, *tg):
        tg = list(tg)
        l_time = crit_t(estims=audio, input_sizes=sizes, target_attr=tg)
        l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=tg) for i, a in enumerate(aux)]
        return (0.6 * l_time + 0.4 * sum(l_mag) / len(l_mag)) / cfg.num_spks

    feed = df.DynamicMixFeed(corpus, df.plan_whamr, batch=B, max_len=T4S, seed=0, fixed_length=True)
    x = torch.zeros(B, T4S, device=dev)
    tg = [torch.zeros(B, T4S, device=dev) for _ in range(2)]
    feed.next_into(x, tg)
    step = CapturedTrainStep(model, loss_fn, opt, x, tg, max_norm=5.0, warmup=2)
    fx, ftg = step.x.clone(), [t.clone() for t in step.targets]

    def loop(fed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(LOOP_STEPS):
            if fed:
                feed.next_into(step.x, step.targets)
                loss, _ = step(step.x, step.targets)
            else:
                loss, _ = step(fx, ftg)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / LOOP_STEPS, float(loss.detach())

    loop(False), loop(True)                                                   # warm both paths
    fixed, fedr, losses = [], [], []
    for _ in range(LOOP_RUNS):
        ms, _ = loop(False)
        fixed.append(ms)
        ms, ls = loop(True)
        fedr.append(ms)
        losses.append(ls)
    # host cost of planning + staging one batch on its own
    t0 = time.perf_counter()
    for _ in range(50):
        feed.next_plan()
    plan_ms = (time.perf_counter() - t0) * 1e3 / 50
    step.release()
    assert all(np.isfinite(v) for v in losses)
    return {"device": torch.cuda.get_device_name(0), "kernel": kernel,
            "loop": {"model": "SepReformer_Base_WSJ0 bf16, batch 16 x 4 s, CapturedTrainStep + FlatAdamW, the reference's loss", "steps_per_run": LOOP_STEPS,
                     "fixed_ms_per_step": fixed, "fed_ms_per_step": fedr, "fed_form": "whamr", "fed_last_losses": losses,
                     "host_plan_ms_per_batch": plan_ms}}


def step_speed(speeds):
    """Plain launch against perturbed launch, and the training step fed without and with speeds; everything alternating."""
    import functools
    import numpy as np
    import torch
    from sepreformer_amd import datafeed as df
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.train_step import CapturedTrainStep
    dev = torch.device("cuda:0")
    keys, arrays = synth_corpus_arrays()
    corpus = df.Corpus.from_arrays(arrays, device=dev, fs=FS)
    corpus.roles = {r: list(keys) for r in ROLES}
    speeds = df.parse_speeds(speeds)
    every = [p for p in speeds if p != 100]                                   # "every source term perturbed": 100 % left out of the draw
    plain = functools.partial(df.plan_wsj0, accept=lambda a, b: True)
    kernel = []
    for B in (16, 32):
        sets = {}
        for name, planner in (("plain", plain), ("perturbed", functools.partial(plain, speeds=every))):
            rng = random.Random(B)
            plan = df.collate_plan(corpus, [planner(corpus, rng, keys[i % NKEYS], T4S) for i in range(B)])
            table = torch.from_numpy(df.pack_table(plan, every)).to(dev)
            sets[name] = (plan, table, torch.empty(B, T4S, device=dev), [torch.empty(B, T4S, device=dev) for _ in range(plan.S)], [])
        for i in range(20 + 100):
            for plan, table, mix, src, ms in sets.values():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                df.mix_batch(corpus, plan, T4S, mix, src, table=table, speeds=every)
                e1.record()
                torch.cuda.synchronize()
                if i >= 20:
                    ms.append(e0.elapsed_time(e1))
        plan = sets["perturbed"][0]
        taps = sum(int(n) * int(df.R_.plan(int(p), 100).K) for n, row in zip(plan.n, plan.speed[:, :plan.M]) for p in row)
        kernel.append({"form": "wsj0", "B": B, "samples": T4S, "S": plan.S, "plain_device_ms": _stats(sets["plain"][4]),
                       "perturbed_device_ms": _stats(sets["perturbed"][4]), "launches": 100, "perturbed_terms": int((plan.speed[:, :plan.M] != 100).sum()),
                       "f64_fma": taps, "Gfma_per_s_at_median": taps / (_stats(sets["perturbed"][4])["median"] * 1e-3) / 1e9})
    B = 16
    cfg = VARIANTS["SepReformer_Base_WSJ0"]
    torch.manual_seed(0)
    model = Model.from_config(cfg, init_seed=0, precision="bf16").load_synthetic_(0).to(dev).train()
    crit_t = PIT_SISNR_time(dev, cfg.num_spks, True)
    crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, cfg.num_spks, True, False)
    sizes = torch.full((B,), T4S)
    opt = FlatAdamW(model, lr=1.0e-4, weight_decay=1.0e-2)

    def loss_fn(audio, aux, *tg):
        tg = list(tg)
        l_time = crit_t(estims=audio, input_sizes=sizes, target_attr=tg)
        l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=tg) for i, a in enumerate(aux)]
        return (0.6 * l_time + 0.4 * sum(l_mag) / len(l_mag)) / cfg.num_spks

    feeds = {"plain": df.DynamicMixFeed(corpus, plain, batch=B, max_len=T4S, seed=0, fixed_length=True),
             "speeds": df.DynamicMixFeed(corpus, functools.partial(plain, speeds=speeds), batch=B, max_len=T4S, seed=0, fixed_length=True)}
    x = torch.zeros(B, T4S, device=dev)
    tg = [torch.zeros(B, T4S, device=dev) for _ in range(2)]
    feeds["plain"].next_into(x, tg)
    step = CapturedTrainStep(model, loss_fn, opt, x, tg, max_norm=5.0, warmup=2)

    def loop(feed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(LOOP_STEPS):
            feed.next_into(step.x, step.targets)
            loss, _ = step(step.x, step.targets)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / LOOP_STEPS, float(loss.detach())

    for f in feeds.values():
        loop(f)                                                               # warm both paths
    runs = {name: [] for name in feeds}
    losses = []
    for _ in range(LOOP_RUNS):
        for name, f in feeds.items():
            ms, ls = loop(f)
            runs[name].append(ms)
            losses.append(ls)
    plan_ms = {}
    for name, f in feeds.items():
        t0 = time.perf_counter()
        for _ in range(50):
            f.next_plan()
        plan_ms[name] = (time.perf_counter() - t0) * 1e3 / 50
    step.release()
    assert all(np.isfinite(v) for v in losses)
    return {"device": torch.cuda.get_device_name(0), "speeds": speeds, "kernel": kernel,
            "loop": {"model": "SepReformer_Base_WSJ0 bf16, batch 16 x 4 s, CapturedTrainStep + FlatAdamW, the reference's loss, fed in the WSJ0 form",
                     "steps_per_run": LOOP_STEPS, "plain_ms_per_step": runs["plain"], "speeds_ms_per_step": runs["speeds"],
                     "host_plan_ms_per_batch": plan_ms}}


def step_reverb(spec):
    """Plain WHAMR-form launch against the reverberant launch at three RT60s, and the training step fed plainly and with reverberation;
    everything alternating."""
    import functools
    import numpy as np
    import torch
    from sepreformer_amd import datafeed as df
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.reverb import RirBank, parse_synthetic, synthetic_rirs
    from sepreformer_amd.train_step import CapturedTrainStep
    count, rt_lo, rt_hi = parse_synthetic(spec)
    dev = torch.device("cuda:0")
    keys, arrays = synth_corpus_arrays()
    corpus = df.Corpus.from_arrays(arrays, device=dev, fs=FS)
    corpus.roles = {r: list(keys) for r in ROLES}
    banks = {rt: RirBank.from_arrays(synthetic_rirs(count, FS, rt60=rt, seed=0), FS, device=dev) for rt in (0.3, 0.6, 1.0)}
    kernel = []
    for B in (16, 32):
        sets = {}
        for name, bank in [("plain", None)] + [(f"rt60_{rt}", b) for rt, b in banks.items()]:
            planner = df.plan_whamr if bank is None else functools.partial(df.plan_whamr, rirs=bank)
            rng = random.Random(B)
            plan = df.collate_plan(corpus, [planner(corpus, rng, keys[i % NKEYS], T4S) for i in range(B)], rirs=bank)
            table = torch.from_numpy(df.pack_table(plan)).to(dev)
            sets[name] = (plan, bank, table, torch.empty(B, T4S, device=dev), [torch.empty(B, T4S, device=dev) for _ in range(plan.S)], [])
        for i in range(20 + 100):
            for plan, bank, table, mix, src, ms in sets.values():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                df.mix_batch(corpus, plan, T4S, mix, src, table=table, rirs=bank)
                e1.record()
                torch.cuda.synchronize()
                if i >= 20:
                    ms.append(e0.elapsed_time(e1))
        rec = {"form": "whamr", "B": B, "samples": T4S, "S": 2, "launches": 100, "plain_device_ms": _stats(sets["plain"][5])}
        for rt in banks:
            plan, ms = sets[f"rt60_{rt}"][0], sets[f"rt60_{rt}"][5]
            fma = int(sum(int(n) * int(k) for n, rr, kk in zip(plan.n, plan.rir, plan.taps) for r, k in zip(rr, kk) if r >= 0))
            rec[f"rt60_{rt}"] = {"device_ms": _stats(ms), "f64_fma": fma, "Gfma_per_s_at_median": fma / (_stats(ms)["median"] * 1e-3) / 1e9,
                                 "mixture_taps_mean": float(plan.taps[:, :2].mean()), "target_taps_mean": float(plan.taps[:, 3:].mean())}
        kernel.append(rec)
    B = 16
    cfg = VARIANTS["SepReformer_Base_WSJ0"]
    torch.manual_seed(0)
    model = Model.from_config(cfg, init_seed=0, precision="bf16").load_synthetic_(0).to(dev).train()
    crit_t = PIT_SISNR_time(dev, cfg.num_spks, True)
    crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, cfg.num_spks, True, False)
    sizes = torch.full((B,), T4S)
    opt = FlatAdamW(model, lr=1.0e-4, weight_decay=1.0e-2)

    def loss_fn(audio, aux, *tg):
        tg = list(tg)
        l_time = crit_t(estims=audio, input_sizes=sizes, target_attr=tg)
        l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=tg) for i, a in enumerate(aux)]
        return (0.6 * l_time + 0.4 * sum(l_mag) / len(l_mag)) / cfg.num_spks

    bank = RirBank.from_arrays(synthetic_rirs(count, FS, rt60=(rt_lo, rt_hi), seed=1), FS, device=dev)
    feeds = {"plain": df.DynamicMixFeed(corpus, df.plan_whamr, batch=B, max_len=T4S, seed=0, fixed_length=True),
             "reverb": df.DynamicMixFeed(corpus, functools.partial(df.plan_whamr, rirs=bank), batch=B, max_len=T4S, seed=0, fixed_length=True,
                                         rirs=bank)}
    x = torch.zeros(B, T4S, device=dev)
    tg = [torch.zeros(B, T4S, device=dev) for _ in range(2)]
    feeds["plain"].next_into(x, tg)
    step = CapturedTrainStep(model, loss_fn, opt, x, tg, max_norm=5.0, warmup=2)

    def loop(feed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(LOOP_STEPS):
            feed.next_into(step.x, step.targets)
            loss, _ = step(step.x, step.targets)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / LOOP_STEPS, float(loss.detach())

    for f in feeds.values():
        loop(f)                                                               # warm both paths
    runs = {name: [] for name in feeds}
    losses = []
    for _ in range(LOOP_RUNS):
        for name, f in feeds.items():
            ms, ls = loop(f)
            runs[name].append(ms)
            losses.append(ls)
    plan_ms = {}
    for name, f in feeds.items():
        t0 = time.perf_counter()
        for _ in range(50):
            f.next_plan()
        plan_ms[name] = (time.perf_counter() - t0) * 1e3 / 50
    step.release()
    assert all(np.isfinite(v) for v in losses)
    return {"device": torch.cuda.get_device_name(0), "rirs": {"count": count, "rt60": [rt_lo, rt_hi], "samples": [int(bank.lengths.min()), int(bank.lengths.max())]},
            "kernel": kernel,
            "loop": {"model": "SepReformer_Base_WSJ0 bf16, batch 16 x 4 s, CapturedTrainStep + FlatAdamW, the reference's loss, fed in the WHAMR form",
                     "steps_per_run": LOOP_STEPS, "plain_ms_per_step": runs["plain"], "reverb_ms_per_step": runs["reverb"],
                     "host_plan_ms_per_batch": plan_ms}}


def _fed_loops(corpus, feeds):
    """The bf16 training step (Base, batch 16 x 4 s, CapturedTrainStep + FlatAdamW, the reference's loss) fed by each of ``feeds`` in turn:
    LOOP_RUNS runs of LOOP_STEPS steps per feed, alternating, after one warming run each.  -> ({name: [ms per step]}, {name: host ms per plan})."""
    import numpy as np
    import torch
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.train_step import CapturedTrainStep
    dev, B = corpus.device, 16
    cfg = VARIANTS["SepReformer_Base_WSJ0"]
    torch.manual_seed(0)
    model = Model.from_config(cfg, init_seed=0, precision="bf16").load_synthetic_(0).to(dev).train()
    crit_t = PIT_SISNR_time(dev, cfg.num_spks, True)
    crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, cfg.num_spks, True, False)
    sizes = torch.full((B,), T4S)
    opt = FlatAdamW(model, lr=1.0e-4, weight_decay=1.0e-2)

    def loss_fn(audio, aux, *tg):
        tg = list(tg)
        l_time = crit_t(estims=audio, input_sizes=sizes, target_attr=tg)
        l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=tg) for i, a in enumerate(aux)]
        return (0.6 * l_time + 0.4 * sum(l_mag) / len(l_mag)) / cfg.num_spks

    x = torch.zeros(B, T4S, device=dev)
    tg = [torch.zeros(B, T4S, device=dev) for _ in range(2)]
    next(iter(feeds.values())).next_into(x, tg)
    step = CapturedTrainStep(model, loss_fn, opt, x, tg, max_norm=5.0, warmup=2)

    def loop(feed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(LOOP_STEPS):
            feed.next_into(step.x, step.targets)
            loss, _ = step(step.x, step.targets)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / LOOP_STEPS, float(loss.detach())

    for f in feeds.values():
        loop(f)                                                               # warm every path
    runs = {name: [] for name in feeds}
    losses = []
    for _ in range(LOOP_RUNS):
        for name, f in feeds.items():
            ms, ls = loop(f)
            runs[name].append(ms)
            losses.append(ls)
    plan_ms = {}
    for name, f in feeds.items():
        t0 = time.perf_counter()
        for _ in range(50):
            f.next_plan()
        plan_ms[name] = (time.perf_counter() - t0) * 1e3 / 50
    step.release()
    assert all(np.isfinite(v) for v in losses)
    return runs, plan_ms


def step_speed_reverb(speeds, spec):
    """The combined launch beside the reverb-only and the speed-only launch of the same plan shapes, and the training step fed with
    reverberation alone and with both; everything alternating."""
    import functools
    import numpy as np
    import torch
    from sepreformer_amd import datafeed as df
    from sepreformer_amd.reverb import RirBank, parse_synthetic, synthetic_rirs
    count, rt_lo, rt_hi = parse_synthetic(spec)
    dev = torch.device("cuda:0")
    keys, arrays = synth_corpus_arrays()
    corpus = df.Corpus.from_arrays(arrays, device=dev, fs=FS)
    corpus.roles = {r: list(keys) for r in ROLES}
    speeds = df.parse_speeds(speeds)
    every = [p for p in speeds if p != 100]                                   # "every source perturbed": 100 % left out of the draw
    bank = RirBank.from_arrays(synthetic_rirs(count, FS, rt60=rt_hi, seed=0), FS, device=dev)
    planners = {"reverb": functools.partial(df.plan_whamr, rirs=bank), "speed": functools.partial(df.plan_whamr, speeds=every),
                "both": functools.partial(df.plan_whamr, speeds=every, rirs=bank, speed_reverb=True)}
    DS_TILE, DR_CHUNK = 2048, 1024
    kernel = []
    for B in (16, 32):
        sets = {}
        for name, planner in planners.items():
            rng = random.Random(B)
            use = None if name == "speed" else bank
            plan = df.collate_plan(corpus, [planner(corpus, rng, keys[i % NKEYS], T4S) for i in range(B)], rirs=use, speed_reverb=name == "both")
            table = torch.from_numpy(df.pack_table(plan, every)).to(dev)
            sets[name] = (plan, use, table, torch.empty(B, T4S, device=dev), [torch.empty(B, T4S, device=dev) for _ in range(plan.S)], [])
        # the reverb-only and the speed-only plan again, through the COMBINED entry (all speeds 100 / all responses -1): the same bits from the
        # new kernel's code for those terms, which says what the conversions cost beside the FIR loop inside one kernel
        for name, extra in (("reverb", dict(speed=np.full_like(sets["reverb"][0].utt, 100))),
                            ("speed", dict(rir=np.full_like(sets["speed"][0].utt, -1), taps=np.ones_like(sets["speed"][0].utt)))):
            plan = sets[name][0]._replace(**extra)
            table = torch.from_numpy(df.pack_table(plan, every)).to(dev)
            sets[name + "_through_combined_entry"] = (plan, bank, table, torch.empty(B, T4S, device=dev),
                                                      [torch.empty(B, T4S, device=dev) for _ in range(plan.S)], [])
        for i in range(20 + 100):
            for plan, use, table, mix, src, ms in sets.values():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                df.mix_batch(corpus, plan, T4S, mix, src, table=table, rirs=use, speeds=every)
                e1.record()
                torch.cuda.synchronize()
                if i >= 20:
                    ms.append(e0.elapsed_time(e1))
        rec = {"form": "whamr", "B": B, "samples": T4S, "S": 2, "launches": 100}
        for name, (plan, use, _, _, _, ms) in sets.items():
            fir = conv = 0
            for n, row_p, row_r, row_k in zip(plan.n, plan.speed if plan.speed is not None else [[100] * 5] * B,
                                              plan.rir if plan.rir is not None else [[-1] * 5] * B, plan.taps if plan.taps is not None else [[1] * 5] * B):
                for p, r, k in zip(row_p, row_r, row_k):
                    K = int(df.R_.plan(int(p), 100).K) if p != 100 else 0
                    if r >= 0:
                        fir += int(n) * int(k)
                    if p != 100 and r < 0:
                        conv += int(n) * K
                    if p != 100 and r >= 0:                                     # per tile and chunk: the 2048 + kc - 1 perturbed samples it reaches
                        for t0 in range(0, int(n), DS_TILE):
                            for k0 in range(0, int(k), DR_CHUNK):
                                conv += (min(DS_TILE, int(n) - t0) + min(DR_CHUNK, int(k) - k0) - 1) * K
            med = _stats(ms)["median"]
            rec[name] = {"device_ms": _stats(ms), "fir_f64_fma": fir, "conversion_f64_fma_upper": conv,
                         "Gfma_per_s_at_median": (fir + conv) / (med * 1e-3) / 1e9,
                         "mixture_taps_mean": float(plan.taps[:, :2].mean()) if plan.taps is not None else None}
        for name in ("reverb", "speed"):                                      # the two entries agree bit for bit where they must
            a, b = sets[name], sets[name + "_through_combined_entry"]
            rec[name + "_through_combined_entry"]["equals_" + name + "_entry"] = bool(torch.equal(a[3], b[3]) and
                                                                                      all(torch.equal(x, y) for x, y in zip(a[4], b[4])))
        kernel.append(rec)
    loop_bank = RirBank.from_arrays(synthetic_rirs(count, FS, rt60=(rt_lo, rt_hi), seed=1), FS, device=dev)
    feeds = {"reverb": df.DynamicMixFeed(corpus, functools.partial(df.plan_whamr, rirs=loop_bank), batch=16, max_len=T4S, seed=0, fixed_length=True,
                                         rirs=loop_bank),
             "both": df.DynamicMixFeed(corpus, functools.partial(df.plan_whamr, speeds=speeds, rirs=loop_bank, speed_reverb=True), batch=16,
                                       max_len=T4S, seed=0, fixed_length=True, rirs=loop_bank)}
    runs, plan_ms = _fed_loops(corpus, feeds)
    return {"device": torch.cuda.get_device_name(0), "speeds": speeds,
            "rirs": {"count": count, "rt60": [rt_lo, rt_hi], "samples": [int(loop_bank.lengths.min()), int(loop_bank.lengths.max())]}, "kernel": kernel,
            "loop": {"model": "SepReformer_Base_WSJ0 bf16, batch 16 x 4 s, CapturedTrainStep + FlatAdamW, the reference's loss, fed in the WHAMR form",
                     "steps_per_run": LOOP_STEPS, "reverb_ms_per_step": runs["reverb"], "both_ms_per_step": runs["both"],
                     "host_plan_ms_per_batch": plan_ms}}


def step_turns(turns, speeds, spec):
    """The launch of a plan without turns, through the entry it has without them, beside the launch of the same planner with turns through the
    new entry, and the training step fed without and with turns; everything alternating.  The corpus, the planners, the banks, the batches and the
    generators' seeds are those of the step that measures the same ``--speeds`` / ``--rirs`` without ``--turns``, so its figures are the yardstick."""
    import functools
    import torch
    from sepreformer_amd import datafeed as df
    from sepreformer_amd.reverb import RirBank, parse_synthetic, synthetic_rirs
    dev = torch.device("cuda:0")
    keys, arrays = synth_corpus_arrays()
    corpus = df.Corpus.from_arrays(arrays, device=dev, fs=FS)
    corpus.roles = {r: list(keys) for r in ROLES}
    tn = df.parse_turns(turns)
    bank = loop_bank = None
    base, loop_base = {}, {}
    if speeds:
        speeds = df.parse_speeds(speeds)
        base["speeds"] = [p for p in speeds if p != 100]                         # "every source perturbed": 100 % left out of the draw
        loop_base["speeds"] = speeds
    if spec:
        count, rt_lo, rt_hi = parse_synthetic(spec)
        bank = RirBank.from_arrays(synthetic_rirs(count, FS, rt60=rt_hi, seed=0), FS, device=dev)
        loop_bank = RirBank.from_arrays(synthetic_rirs(count, FS, rt60=(rt_lo, rt_hi), seed=1), FS, device=dev)
        base.update(rirs=bank, speed_reverb=bool(speeds))
        loop_base.update(rirs=loop_bank, speed_reverb=bool(speeds))
    every = base.get("speeds", [])
    ramp = df.ramp_table(dev, tn.ramp)
    planners = {"base": functools.partial(df.plan_whamr, **base), "turns": functools.partial(df.plan_whamr, turns=tn, **base)}
    DS_TILE = 2048
    kernel = []
    for B in (16, 32):
        sets = {}
        for name, planner in planners.items():
            rng = random.Random(B)
            plan = df.collate_plan(corpus, [planner(corpus, rng, keys[i % NKEYS], T4S) for i in range(B)], rirs=bank, speed_reverb=bool(speeds and spec))
            table = torch.from_numpy(df.pack_table(plan, every)).to(dev)
            sets[name] = (plan, table, torch.empty(B, T4S, device=dev), [torch.empty(B, T4S, device=dev) for _ in range(plan.S)], [])
        for i in range(20 + 100):
            for plan, table, mix, src, ms in sets.values():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                df.mix_batch(corpus, plan, T4S, mix, src, table=table, rirs=bank, speeds=every, ramp=ramp)
                e1.record()
                torch.cuda.synchronize()
                if i >= 20:
                    ms.append(e0.elapsed_time(e1))
        plan = sets["turns"][0]
        tiles = silent = 0                                                       # source terms' tiles, and those the skip rule takes whole
        for b in range(B):
            for j in list(range(2)) + list(range(plan.M, plan.M + plan.S)):
                K = int(plan.taps[b, j]) if plan.rir is not None and plan.rir[b, j] >= 0 else 1
                for t0 in range(0, int(plan.n[b]), DS_TILE):
                    tiles += 1
                    silent += t0 >= int(plan.off[b, j]) + K - 1 or min(t0 + DS_TILE, int(plan.n[b])) <= int(plan.on[b, j])
        active = [(min(int(f), int(n)) - max(int(o), 0)) / int(n) for o, f, n in zip(plan.on[:, :2].ravel(), plan.off[:, :2].ravel(), plan.n.repeat(2))]
        kernel.append({"form": "whamr", "B": B, "samples": T4S, "S": 2, "launches": 100, "base": {"device_ms": _stats(sets["base"][4])},
                       "turns": {"device_ms": _stats(sets["turns"][4]), "source_tiles": tiles, "source_tiles_skipped_whole": int(silent),
                                 "mean_active_fraction_of_a_source": sum(active) / len(active)}})
    feeds = {name: df.DynamicMixFeed(corpus, functools.partial(df.plan_whamr, **kw), batch=16, max_len=T4S, seed=0, fixed_length=True, rirs=loop_bank)
             for name, kw in (("base", loop_base), ("turns", dict(loop_base, turns=tn)))}
    runs, plan_ms = _fed_loops(corpus, feeds)
    return {"device": torch.cuda.get_device_name(0), "turns": {"overlap": list(tn.overlap), "ramp": tn.ramp}, "speeds": speeds or None, "rirs": spec or None,
            "kernel": kernel,
            "loop": {"model": "SepReformer_Base_WSJ0 bf16, batch 16 x 4 s, CapturedTrainStep + FlatAdamW, the reference's loss, fed in the WHAMR form",
                     "steps_per_run": LOOP_STEPS, "base_ms_per_step": runs["base"], "turns_ms_per_step": runs["turns"], "host_plan_ms_per_batch": plan_ms}}


def step_rooms(spec):
    """Simulating a bank of shoebox rooms on the device (section 5e-4): hipEvent time of one ``sepr_rir_ism_fwd`` call for COUNT rooms,
    the numpy restatement's CPU time for ONE of them (and that the two agree exactly), the realised decay of a few responses beside the
    nominal rt60, and the bf16 training step fed from a fixed simulated bank against the same feed with ``rooms_every=1``, alternating."""
    import functools
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rirsim_ref
    from sepreformer_amd import datafeed as df
    from sepreformer_amd import lib as L_
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.reverb import RirBank, RoomSampler, parse_rooms, schroeder_rt60
    from sepreformer_amd.train_step import CapturedTrainStep
    count, rt_lo, rt_hi = parse_rooms(spec)
    dev = torch.device("cuda:0")
    sampler = RoomSampler(rt60=(rt_lo, rt_hi))
    rooms = sampler.draw(count, seed=0)
    bank = RirBank.simulate(rooms, FS, device=dev)
    N, sim = int(bank.lengths[0]), bank._sim
    lib = L_.load()
    ms = []
    for i in range(5 + 20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L_.check(lib.sepr_rir_ism_fwd(sim["rooms"].data_ptr(), count, N, sim["fsc"], sim["lut"].data_ptr(), sim["acc"].data_ptr(), bank.buf.data_ptr(),
                                      sim["out"].data_ptr() + 4 * count * N, sim["normalise"], torch.cuda.current_stream().cuda_stream), "sepr_rir_ism_fwd")
        e1.record()
        torch.cuda.synchronize()
        if i >= 5:
            ms.append(e0.elapsed_time(e1))
    wall = []
    for i in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bank.resimulate(sampler.draw(count, seed=(0, i)))
        wall.append((time.perf_counter() - t0) * 1e3)
    bank.resimulate(rooms)
    t0 = time.perf_counter()
    acc0, images0 = rirsim_ref.ism_acc(np.asarray(rooms[0]), sim["fsc"], N)
    cpu_s = time.perf_counter() - t0
    exact = bool(np.array_equal(sim["acc"][0].cpu().numpy(), acc0))
    # realised decay: a few rooms simulated long enough for the -25 dB point, whatever their rt60
    few = min(count, 6)
    long_n = min(16384, int(np.ceil(2.5 * FS * rt_hi)))
    longer = RirBank.simulate(rooms[:few], FS, length=long_n, device=dev, normalise=None)
    decay = [{"room_m": [round(float(v), 3) for v in rooms[r, :3]], "beta": float(rooms[r, 9]), "nominal_rt60_s": float(rooms.rt60[r]),
              "schroeder_T20_s": schroeder_rt60(longer.rir(r), FS), "peak_idx": int(longer.peak_idx[r])} for r in range(few)]
    del longer

    keys, arrays = synth_corpus_arrays()
    corpus = df.Corpus.from_arrays(arrays, device=dev, fs=FS)
    corpus.roles = {r: list(keys) for r in ROLES}
    B = 16
    cfg = VARIANTS["SepReformer_Base_WSJ0"]
    torch.manual_seed(0)
    model = Model.from_config(cfg, init_seed=0, precision="bf16").load_synthetic_(0).to(dev).train()
    crit_t = PIT_SISNR_time(dev, cfg.num_spks, True)
    crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, cfg.num_spks, True, False)
    sizes = torch.full((B,), T4S)
    opt = FlatAdamW(model, lr=1.0e-4, weight_decay=1.0e-2)

    def loss_fn(audio, aux, *tg):
        tg = list(tg)
        l_time = crit_t(estims=audio, input_sizes=sizes, target_attr=tg)
        l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=tg) for i, a in enumerate(aux)]
        return (0.6 * l_time + 0.4 * sum(l_mag) / len(l_mag)) / cfg.num_spks

    redrawn = RirBank.simulate(rooms, FS, device=dev)
    feeds = {"fixed": df.DynamicMixFeed(corpus, functools.partial(df.plan_whamr, rirs=bank), batch=B, max_len=T4S, seed=0, fixed_length=True, rirs=bank),
             "rooms": df.DynamicMixFeed(corpus, functools.partial(df.plan_whamr, rirs=redrawn), batch=B, max_len=T4S, seed=0, fixed_length=True,
                                        rirs=redrawn, rooms=sampler, rooms_every=1)}
    x = torch.zeros(B, T4S, device=dev)
    tg = [torch.zeros(B, T4S, device=dev) for _ in range(2)]
    feeds["fixed"].next_into(x, tg)
    step = CapturedTrainStep(model, loss_fn, opt, x, tg, max_norm=5.0, warmup=2)

    def loop(feed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(LOOP_STEPS):
            feed.next_into(step.x, step.targets)
            loss, _ = step(step.x, step.targets)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / LOOP_STEPS, float(loss.detach())

    for f in feeds.values():
        loop(f)                                                               # warm both paths
    runs = {name: [] for name in feeds}
    losses = []
    for _ in range(LOOP_RUNS):
        for name, f in feeds.items():
            e_before = f.epoch
            ms_step, ls = loop(f)
            runs[name].append(ms_step)
            losses.append(ls)
            if name == "rooms":
                epochs_per_run = f.epoch - e_before
    step.release()
    assert all(np.isfinite(v) for v in losses)
    return {"device": torch.cuda.get_device_name(0),
            "rooms": {"count": count, "rt60_nominal": [rt_lo, rt_hi], "samples": N, "fs": FS, "sampler": "RoomSampler defaults",
                      "images_room0": images0},
            "simulate": {"device_ms": _stats(ms), "launches": 20, "resimulate_wall_ms": _stats(wall),
                         "restatement_cpu_s_one_room": cpu_s, "restatement_equals_device_sums": exact},
            "decay": decay,
            "loop": {"model": "SepReformer_Base_WSJ0 bf16, batch 16 x 4 s, CapturedTrainStep + FlatAdamW, the reference's loss, fed in the WHAMR form "
                              "from a simulated bank", "steps_per_run": LOOP_STEPS, "steps_per_epoch": NKEYS // B,
                     "resimulations_per_run_rooms": epochs_per_run, "fixed_ms_per_step": runs["fixed"], "rooms_ms_per_step": runs["rooms"]}}


def step_host():
    """The reference's per-example work in numpy from RAM-resident arrays (no disk, no decoding of a file): WHAMR form."""
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    keys, arrays = synth_corpus_arrays()

    def load(name):
        return arrays[name].astype(np.float32) / np.float32(32768.0)

    def example(i):
        rng = random.Random(i)
        key, other = keys[i % NKEYS], rng.choice(keys)
        dry = [load(f"s1/{key}"), load(f"s2/{other}")]
        wet = [load(f"s1_reverb/{key}"), load(f"s2_reverb/{other}")]
        ref = np.sqrt(np.mean(np.square(dry[0])))
        lens = [T4S]
        for d, w in zip(dry, wet):
            nf = ref / np.sqrt(np.mean(np.square(d)))
            d *= nf
            w *= nf
            g = pow(10, -rng.uniform(-3, 3) / 20)
            d *= np.float32(g)
            w *= np.float32(g)
            lens.append(len(d))
        noise = load(f"noise/{key}")
        noise *= ref / np.sqrt(np.mean(np.square(noise)))
        noise = noise * pow(10, -rng.uniform(-6, 3) / 20)
        n = min(lens + [len(noise)])
        out = []
        for d, w in zip(dry, wet):
            s = rng.randint(0, len(d) - n)
            out.append((w[s:s + n], d[s:s + n]))
        s = rng.randint(0, len(noise) - n)
        mix = out[0][0] + out[1][0] + noise[s:s + n]
        return mix, [o[1] for o in out]

    N = 512
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(example, range(32)))
        t0 = time.perf_counter()
        list(pool.map(example, range(N)))
        dt = time.perf_counter() - t0
    return {"host_numpy": {"threads": 16, "examples": N, "utt_per_s": N / dt, "form": "whamr, from RAM-resident int16 arrays, no collate"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--speeds", default=None, metavar="LO:HI", help="measure speed perturbation (an inclusive range or a comma list of percentages)")
    ap.add_argument("--rirs", default=None, metavar="COUNT:RT60", help="measure reverberation by convolution (COUNT synthetic impulse responses of RT60 s)")
    ap.add_argument("--room-rirs", default=None, metavar="COUNT[:RT60LO:RT60HI]", help="measure simulating COUNT shoebox rooms on the device (image-source method)")
    ap.add_argument("--turns", default=None, metavar="LO:HI", help="measure turn-taking with the overlap drawn from [LO, HI], on top of --speeds and --rirs")
    args = ap.parse_args()
    both = bool(args.speeds and args.rirs)                                   # the two together: section 5e-5
    if args.turns and args.room_rirs:
        ap.error("--turns composes with --speeds and --rirs")
    if sum(bool(v) for v in (args.speeds, args.rirs, args.room_rirs)) > (2 if both and not args.room_rirs else 1):
        ap.error("--speeds, --rirs and --room-rirs are measured in runs of their own (--speeds with --rirs measures both in one source)")
    if args.step:
        rec = {"device": step_device, "host": step_host, "speed": lambda: step_speed(args.speeds), "reverb": lambda: step_reverb(args.rirs),
               "rooms": lambda: step_rooms(args.room_rirs), "both": lambda: step_speed_reverb(args.speeds, args.rirs),
               "turns": lambda: step_turns(args.turns, args.speeds, args.rirs)}[args.step]()
        print("__RESULT__" + json.dumps(rec))
        return
    rec, failed = {}, None
    for name, limit in ([("turns", 600)] if args.turns else [("both", 600)] if both else [("speed", 600)] if args.speeds else [("reverb", 600)] if args.rirs else [("rooms", 600)] if args.room_rirs else STEPS):
        cmd = (["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name] + (["--speeds", args.speeds] if args.speeds else [])
               + (["--rirs", args.rirs] if args.rirs else []) + (["--room-rirs", args.room_rirs] if args.room_rirs else []) + (["--turns", args.turns] if args.turns else []))
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("__RESULT__")]
        if r.returncode != 0 or not lines:
            failed = {"step": name, "returncode": r.returncode, "stderr_tail": r.stderr[-1500:]}
            print(json.dumps(failed), file=sys.stderr)
            break                                                          # nothing more runs on the device after a failure
        rec.update(json.loads(lines[-1][len("__RESULT__"):]))
        print(name, "done", flush=True)
    if not failed and args.turns:
        lp = rec["loop"]
        a, b = lp["base_ms_per_step"], lp["turns_ms_per_step"]
        mean = lambda v: sum(v) / len(v)                                    # noqa: E731
        k = next(r for r in rec["kernel"] if r["B"] == 16)
        rec["summary"] = {"base_launch_ms_median": k["base"]["device_ms"]["median"], "turns_launch_ms_median": k["turns"]["device_ms"]["median"],
                          "turns_launch_over_base": k["turns"]["device_ms"]["median"] / k["base"]["device_ms"]["median"],
                          "base_step_ms_mean": mean(a), "turns_step_ms_mean": mean(b), "difference_ms": mean(b) - mean(a),
                          "base_step_spread_ms": max(a) - min(a), "turns_step_spread_ms": max(b) - min(b)}
    elif not failed and both:
        lp = rec["loop"]
        a, b = lp["reverb_ms_per_step"], lp["both_ms_per_step"]
        mean = lambda v: sum(v) / len(v)                                    # noqa: E731
        k = next(r for r in rec["kernel"] if r["B"] == 16)
        spread = max(max(a) - min(a), max(b) - min(b))
        med = {name: k[name]["device_ms"]["median"] for name in k if isinstance(k[name], dict)}
        rec["summary"] = {"launch_ms_median": med, "both_minus_reverb_launch_ms": med["both"] - med["reverb"],
                          "both_minus_reverb_through_combined_entry_ms": med["both"] - med["reverb_through_combined_entry"],
                          "conversion_fma_upper_over_fir_fma": k["both"]["conversion_f64_fma_upper"] / k["both"]["fir_f64_fma"],
                          "launch_excess_over_reverb": med["both"] / med["reverb"] - 1.0,
                          "reverb_step_ms_mean": mean(a), "both_step_ms_mean": mean(b), "difference_ms": mean(b) - mean(a),
                          "reverb_step_spread_ms": max(a) - min(a), "both_step_spread_ms": max(b) - min(b),
                          "both_exceeds_reverb_by_more_than_the_larger_spread": mean(b) - mean(a) > spread}
    elif not failed and args.speeds:
        lp = rec["loop"]
        a, b = lp["plain_ms_per_step"], lp["speeds_ms_per_step"]
        mean = lambda v: sum(v) / len(v)                                    # noqa: E731
        k = next(r for r in rec["kernel"] if r["B"] == 16)
        rec["summary"] = {"plain_launch_ms_median": k["plain_device_ms"]["median"], "perturbed_launch_ms_median": k["perturbed_device_ms"]["median"],
                          "plain_step_ms_mean": mean(a), "speeds_step_ms_mean": mean(b), "difference_ms": mean(b) - mean(a),
                          "plain_step_spread_ms": max(a) - min(a), "speeds_step_spread_ms": max(b) - min(b),
                          "perturbed_launch_share_of_plain_step": k["perturbed_device_ms"]["median"] / mean(a)}
    elif not failed and args.rirs:
        lp = rec["loop"]
        a, b = lp["plain_ms_per_step"], lp["reverb_ms_per_step"]
        mean = lambda v: sum(v) / len(v)                                    # noqa: E731
        k = next(r for r in rec["kernel"] if r["B"] == 16)
        spread = max(max(a) - min(a), max(b) - min(b))
        rec["summary"] = {"plain_launch_ms_median": k["plain_device_ms"]["median"],
                          "reverb_launch_ms_median": {rt: k[rt]["device_ms"]["median"] for rt in k if rt.startswith("rt60_")},
                          "plain_step_ms_mean": mean(a), "reverb_step_ms_mean": mean(b), "difference_ms": mean(b) - mean(a),
                          "plain_step_spread_ms": max(a) - min(a), "reverb_step_spread_ms": max(b) - min(b),
                          "reverb_exceeds_plain_by_more_than_the_larger_spread": mean(b) - mean(a) > spread}
    elif not failed and args.room_rirs:
        lp = rec["loop"]
        a, b = lp["fixed_ms_per_step"], lp["rooms_ms_per_step"]
        mean = lambda v: sum(v) / len(v)                                    # noqa: E731
        sim_ms = rec["simulate"]["device_ms"]["median"]
        rec["summary"] = {"simulate_ms_median": sim_ms, "fixed_step_ms_mean": mean(a), "rooms_step_ms_mean": mean(b), "difference_ms": mean(b) - mean(a),
                          "fixed_step_spread_ms": max(a) - min(a), "rooms_step_spread_ms": max(b) - min(b),
                          "condition_one_simulation_under_one_step": {"simulate_ms": sim_ms, "step_ms": mean(a), "met": sim_ms < mean(a)}}
    elif not failed:
        lp = rec["loop"]
        fixed, fed = lp["fixed_ms_per_step"], lp["fed_ms_per_step"]
        mean = lambda v: sum(v) / len(v)                                    # noqa: E731
        k = next(r for r in rec["kernel"] if r["form"] == "whamr" and r["B"] == 16)
        spread = max(max(fixed) - min(fixed), max(fed) - min(fed))
        rec["conditions"] = {
            "launch_at_most_1pct_of_step": {"launch_ms_median": k["device_ms"]["median"], "fixed_step_ms_mean": mean(fixed),
                                            "fraction": k["device_ms"]["median"] / mean(fixed), "met": k["device_ms"]["median"] <= 0.01 * mean(fixed)},
            "fed_vs_fixed": {"fixed_mean_ms": mean(fixed), "fed_mean_ms": mean(fed), "difference_ms": mean(fed) - mean(fixed),
                             "larger_within_setting_spread_ms": spread, "met": mean(fed) - mean(fixed) <= spread},
            "utt_per_s": {"step_fixed": 16 / mean(fixed) * 1e3, "step_fed": 16 / mean(fed) * 1e3, "host_numpy_16_threads": rec["host_numpy"]["utt_per_s"]}}
    if failed:
        rec["failed"] = failed
    line = json.dumps(rec)
    print(line)
    if args.out and not failed:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
