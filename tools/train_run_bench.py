#!/usr/bin/env python3
"""What the epoch loop (sepreformer_amd/trainer.py) costs over the bare captured step, on a synthetic corpus,
batch 16 x 4 s, bf16, per model (default: SepReformer_Base_WSJ0 and SepReformer_Large_DM_WSJ0):

  (a) the bare loop of ``tools/train_from_scp.py --steps``, built as that tool builds it - a model and a captured step of its own, an
      unguarded ``FlatAdamW`` with no ledger, the fixed 0.6 / 0.4 loss: ``next_into`` + ``step``, one synchronisation at the end, STEPS
      steps, RUNS times, alternating with (b) in the same process;
  (b) a ``Trainer.train_epoch`` of the same STEPS steps, log interval at its default;
  (c) ``Trainer.validate`` over VALID utterances, in utt/s;
  (d) the device time of the ledger launch and of the guarded against the unguarded optimizer step, from a
      ``rocprofv3 --kernel-trace --stats`` run of its own over ten eager steps of Base per entry (``--no-trace`` skips it).

Pass condition: median(b) >= median(a) - (max(a) - min(a)), in utt/s - the margin is the yardstick's own spread in this call.
Every part runs in a child process of its own under ``timeout -k 10 <s>``; the first that fails ends the run.

``--ema-decay D`` measures the weight EMA instead, per model: (a) is ``Trainer.train_epoch`` without the EMA - the
loop above's (b) - and (b) the same epoch of a ``Trainer(ema_decay=D)``, alternating in one process under the same pass condition; then one
validation pass on the raw weights against one under ``FlatAdamW.averaged()`` (two exchanges and two re-packs apart), the exchange pair
alone, ``torch._foreach_lerp_`` over the parameter list (the route the fused update replaces), and the hipEvent time of each Trainer's two
captured graphs replayed on their own: the optimizer graph holds everything the EMA adds to a step.  Its kernel trace holds the update kernel
with and without the EMA and the exchange kernel.  ``--ema-first`` builds and runs the Trainer with the EMA first; ``--ema-control`` builds both
without it, which shows what two instances of one loop differ by.

    python tools/train_run_bench.py [--models SepReformer_Base_WSJ0] [--steps 200] [--runs 5] [--out profiles/train_run.json]
    python tools/train_run_bench.py --ema-decay 0.999 --models SepReformer_Base_WSJ0 --out profiles/ema.json
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, T4S, B = 8000, 32000, 16
ROLES = ("s1", "s2", "mix")


def _stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "mean": sum(v) / len(v)}


def synth_corpus(nkeys, dev, seed=0):
    """``nkeys`` keys x (s1, s2, mix) of 4.5 - 8 s of pseudo-random PCM16: the loop's time does not depend on the values."""
    import numpy as np
    from sepreformer_amd import datafeed as df
    rng = np.random.default_rng(seed)
    keys = [f"k{i:04d}a_0.{i:04d}_k{i:04d}b_-0.{i:04d}" for i in range(nkeys)]
    arrays = {}
    for k in keys:
        n = int(rng.integers(36000, 64000))
        for r in ROLES:
            arrays[f"{r}/{k}"] = rng.integers(-6000, 6000, size=n, dtype=np.int16)
    corpus = df.Corpus.from_arrays(arrays, device=dev, fs=FS)
    corpus.roles = {r: list(keys) for r in ROLES}
    return corpus, keys


def child_loop(model_name, steps, runs, nvalid):
    import functools
    import torch
    from sepreformer_amd import datafeed as df
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.model import Model
    from sepreformer_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    corpus, keys = synth_corpus(48, dev)
    order = (keys * (steps * B // len(keys) + 1))[:steps * B]                         # one epoch = STEPS batches
    vcorpus, vkeys = synth_corpus(nvalid, dev, seed=1)
    planner = functools.partial(df.plan_wsj0, accept=lambda a, b: True)
    feed = df.DynamicMixFeed(corpus, planner, batch=B, max_len=T4S, seed=0, fixed_length=True, keys=order)
    valid = df.DynamicMixFeed(vcorpus, df.plan_direct, batch=B, max_len=T4S, seed=0, keys=vkeys, drop_last=False)
    cfg = VARIANTS[model_name]
    model = Model.from_config(cfg, init_seed=0, precision="bf16").load_synthetic_(0).to(dev).train()
    ck = tempfile.mkdtemp(prefix="train_run_bench_")
    trainer = Trainer(model, feed, valid, ck, lr=1.0e-4, seed=0, log=lambda s: None)
    # (a) is built the way tools/train_from_scp.py --steps builds it: a model, a feed and a captured step of its own, an UNGUARDED FlatAdamW with no
    # ledger, the plain 0.6 / 0.4 loss - so (b) - (a) holds everything the loop adds: the norm pass the guard always runs (here it runs anyway:
    # max_norm), the guarded kernels, the parts copy, the ledger launch, the per-batch schedule and the ledger read-backs
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.train_step import CapturedTrainStep
    bare_model = Model.from_config(cfg, init_seed=0, precision="bf16").load_synthetic_(0).to(dev).train()
    bare_feed = df.DynamicMixFeed(corpus, planner, batch=B, max_len=T4S, seed=0, fixed_length=True, keys=order)
    crit_t = PIT_SISNR_time(dev, cfg.num_spks, True)
    crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, cfg.num_spks, True, False)
    sizes = torch.full((B,), T4S)
    bare_opt = FlatAdamW(bare_model, lr=1.0e-4, weight_decay=1.0e-2)

    def loss_fn(audio, aux, *tg):
        tg = list(tg)
        l_time = crit_t(estims=audio, input_sizes=sizes, target_attr=tg)
        l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=tg) for i, a in enumerate(aux)]
        return (0.6 * l_time + 0.4 * sum(l_mag) / len(l_mag)) / cfg.num_spks

    x = torch.zeros(B, T4S, device=dev)
    tgs = [torch.zeros(B, T4S, device=dev) for _ in range(cfg.num_spks)]
    bare_feed.next_into(x, tgs)
    step = CapturedTrainStep(bare_model, loss_fn, bare_opt, x, tgs, max_norm=5.0)
    plan_s, read_s = [0.0], [0.0]
    try:
        trainer.train_epoch(2)                                                        # builds the Trainer's captured step; warms its loop

        def bare():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                bare_feed.next_into(step.x, step.targets)
                loss, _ = step(step.x, step.targets)
            float(loss.detach())
            return steps * B / (time.perf_counter() - t0)

        def looped():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.train_epoch(2)
            return steps * B / (time.perf_counter() - t0)

        bare()
        a, b = [], []
        for _ in range(runs):
            a.append(bare())
            b.append(looped())
            print(f"{model_name}: run {len(a)} / {runs}: bare {a[-1]:.1f} utt/s, Trainer {b[-1]:.1f} utt/s", file=sys.stderr, flush=True)      # a long run must not fall silent
        # attribution, should (b) fall short: host time of planning a batch and of one ledger read-back
        t0 = time.perf_counter()
        for _ in range(50):
            feed.next_plan()
        plan_s[0] = (time.perf_counter() - t0) / 50
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            trainer.read_ledger()
        read_s[0] = (time.perf_counter() - t0) / 20
        trainer.validate()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, nb = trainer.validate()
        torch.cuda.synchronize()
        v = nvalid / (time.perf_counter() - t0)
    finally:
        trainer.release()
        step.release()
        shutil.rmtree(ck, ignore_errors=True)
    sa, sb = _stats(a), _stats(b)
    return {"model": model_name, "device": torch.cuda.get_device_name(0), "batch": B, "samples": T4S, "precision": "bf16", "steps_per_run": steps,
            "runs": runs, "log_every": trainer.log_every,
            "a_is": "tools/train_from_scp.py --steps: own model and captured step, unguarded FlatAdamW, no ledger, fixed 0.6 / 0.4 loss",
            "b_is": "Trainer.train_epoch: guarded FlatAdamW, ledger launch, parts copy, weight scalars, schedule, ledger read-backs", "a_bare_utt_s": a, "b_trainer_utt_s": b, "a": sa, "b": sb,
            "pass": sb["median"] >= sa["median"] - (sa["max"] - sa["min"]), "valid_utterances": nvalid, "valid_batches": nb, "c_valid_utt_s": v,
            "host_plan_ms_per_batch": plan_s[0] * 1e3, "ledger_read_ms": read_s[0] * 1e3}


def child_ema_loop(model_name, steps, runs, nvalid, decay, control=False, ema_first=False):
    """(a) Trainer.train_epoch without the EMA, (b) with it: two Trainers of their own in one process, alternating.  ``control``: (b) is built
    without the EMA too - what two instances of the SAME loop differ by in one process, beside which a shortfall of (b) is read.  ``ema_first``: the Trainer with the EMA is built first and runs first in every
    pair (the control shows the instance built second running slower)."""
    import functools
    import torch
    from sepreformer_amd import datafeed as df
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.model import Model
    from sepreformer_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    corpus, keys = synth_corpus(48, dev)
    order = (keys * (steps * B // len(keys) + 1))[:steps * B]
    vcorpus, vkeys = synth_corpus(nvalid, dev, seed=1)
    planner = functools.partial(df.plan_wsj0, accept=lambda a, b: True)
    cfg = VARIANTS[model_name]
    trainers, dirs = [], []
    for d in ((decay, None) if ema_first else (None, None if control else decay)):
        feed = df.DynamicMixFeed(corpus, planner, batch=B, max_len=T4S, seed=0, fixed_length=True, keys=order)
        valid = df.DynamicMixFeed(vcorpus, df.plan_direct, batch=B, max_len=T4S, seed=0, keys=vkeys, drop_last=False)
        model = Model.from_config(cfg, init_seed=0, precision="bf16").load_synthetic_(0).to(dev).train()
        dirs.append(tempfile.mkdtemp(prefix="train_run_bench_"))
        trainers.append(Trainer(model, feed, valid, dirs[-1], lr=1.0e-4, seed=0, log=lambda s: None, ema_decay=d))
    plain, ema = reversed(trainers) if ema_first else trainers

    def epoch(t):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.train_epoch(2)
        return steps * B / (time.perf_counter() - t0)

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    try:
        for t in trainers:                                                            # builds the captured steps; warms both loops
            epoch(t)
        a, b = [], []
        for _ in range(runs):
            for t in trainers:
                (a if t is plain else b).append(epoch(t))
            print(f"{model_name}: run {len(a)} / {runs}: without {a[-1]:.1f} utt/s, with the EMA {b[-1]:.1f} utt/s", file=sys.stderr, flush=True)
        # attribution: hipEvent time of each Trainer's two captured graphs on their own (forward + backward; norm + prepare + update + ledger),
        # so a gap between the loops can be told apart: the optimizer graph holds everything the EMA adds to a step
        def graph_ms(g, n):
            g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                g.replay()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / n
        graphs = {}
        for _ in range(2):                                                            # twice, alternating: the second pass is the one kept
            for name, t in (("a", plain), ("b", ema)):
                graphs[name] = {"main_graph_ms": graph_ms(t.step.g_main, 30), "optimizer_graph_us": 1e3 * graph_ms(t.step.g_opt, 200)}
        params = [p.detach() for p in ema.model.parameters()]
        if control:
            sa, sb = _stats(a), _stats(b)
            return {"model": model_name, "control": "both Trainers WITHOUT the EMA: two instances of one loop", "steps_per_run": steps, "runs": runs,
                    "a_without_utt_s": a, "b_without_utt_s": b, "a": sa, "b": sb, "step_ms_a": 1e3 * B / sa["median"], "step_ms_b": 1e3 * B / sb["median"],
                    "graphs": graphs}
        v_raw = timed(lambda: ema.validate("raw"), 2)
        v_ema = timed(lambda: ema.validate("ema"), 2)

        def swap_pair():
            with ema.opt.averaged():
                pass
        swap_s = timed(swap_pair, 20)
        ema.model.invalidate_packed()
        shadow = [p.clone() for p in params]
        lerp_s = timed(lambda: torch._foreach_lerp_(shadow, params, 1.0 - decay), 50)
    finally:
        for t in trainers:
            t.release()
        for d in dirs:
            shutil.rmtree(d, ignore_errors=True)
    sa, sb = _stats(a), _stats(b)
    return {"model": model_name, "device": torch.cuda.get_device_name(0), "batch": B, "samples": T4S, "precision": "bf16", "steps_per_run": steps,
            "runs": runs, "ema_decay": decay, "order": "the Trainer with the EMA built first, first in every pair" if ema_first else
            "the Trainer without the EMA built first, first in every pair", "parameters": sum(p.numel() for p in params), "parameter_tensors": len(params),
            "a_is": "Trainer.train_epoch, EMA off (sepr_adamw_step_guarded: the parent commit's code path)",
            "b_is": "Trainer.train_epoch, ema_decay on (sepr_adamw_step_ema in the optimizer graph)", "a_without_utt_s": a, "b_with_utt_s": b,
            "a": sa, "b": sb, "pass": sb["median"] >= sa["median"] - (sa["max"] - sa["min"]),
            "step_ms_without": 1e3 * B / sa["median"], "step_ms_with": 1e3 * B / sb["median"], "graphs": graphs,
            "graphs_is": "hipEvent time per replay of each Trainer's captured graphs on their own: 30 of the main graph, 200 of the optimizer graph",
            "valid_utterances": nvalid, "validate_raw_s": v_raw, "validate_averaged_s": v_ema, "averaged_overhead_ms": (v_ema - v_raw) * 1e3,
            "swap_pair_ms": swap_s * 1e3, "foreach_lerp_ms": lerp_s * 1e3,
            "foreach_lerp_is": "torch._foreach_lerp_(shadow list, parameter list, 1 - d): host-timed mean of 50 calls, queue drained at both ends"}


def child_trace(ema_decay=None):
    """Ten eager steps of Base under each optimizer entry, ledger attached: what the kernel trace then attributes.  With ``ema_decay``: the
    guarded entry against the EMA entry, and one ``averaged()`` block for the exchange kernel."""
    import torch
    from sepreformer_amd import lib as L
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.criterion import PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.synth import synth_mixture
    dev = torch.device("cuda:0")
    crit = PIT_SISNR_time(dev, 2, True)
    s1, s2 = synth_mixture(2, 4000, seed=1).to(dev), synth_mixture(2, 4000, seed=2).to(dev)
    sizes = torch.full((2,), 4000)
    for guarded in ((True, False) if ema_decay is None else (None, True)):
        model = Model.from_config(VARIANTS["SepReformer_Base_WSJ0"], init_seed=0, precision="bf16").load_synthetic_(0).to(dev).train()
        opt = FlatAdamW(model, lr=1.0e-4, skip_nonfinite=guarded is not False, ema_decay=ema_decay if guarded is None else None)
        parts = torch.zeros(5, dtype=torch.float32, device=dev)
        opt.attach_ledger(torch.zeros(L.ledger_doubles(5), dtype=torch.float64, device=dev), parts)
        for _ in range(10):
            opt.zero_grad(set_to_none=True)
            audio, _ = model(s1 + s2)
            (crit(estims=audio, input_sizes=sizes, target_attr=[s1, s2]) / 2).backward()
            opt.step(max_norm=5.0)
        if guarded is None:
            with opt.averaged():
                pass
        torch.cuda.synchronize()
    return {"ok": True}


def run_trace(ema_decay=None):
    if shutil.which("rocprofv3") is None:
        return {"skipped": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="train_run_trace_")
    try:
        subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "t", "--",
                        sys.executable, os.path.abspath(__file__), "--child", "trace"] + ([] if ema_decay is None else ["--ema-decay", str(ema_decay)]), check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=out)
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        rows = list(csv.DictReader(open(files[0])))
        # the two templates are <GUARD, EMA>
        pick = {"ledger": "run_ledger_kernel", "update_guarded": "opt_adamw_kernel<true, false>", "update_unguarded": "opt_adamw_kernel<false, false>",
                "prep_guarded": "opt_prep_kernel<true, false>", "prep_unguarded": "opt_prep_kernel<false, false>", "norm": "opt_sqsum_kernel"}
        if ema_decay is not None:
            pick = {"update_guarded": "opt_adamw_kernel<true, false>", "update_ema": "opt_adamw_kernel<true, true>", "prep_guarded": "opt_prep_kernel<true, false>",
                    "prep_ema": "opt_prep_kernel<true, true>", "swap": "opt_swap_kernel", "norm": "opt_sqsum_kernel"}
        return {"model": "SepReformer_Base_WSJ0 (14.7 M parameters), 10 eager steps per entry",
                **{name: {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
                   for name, sub in pick.items() for r in rows if sub in r["Name"]}}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["SepReformer_Base_WSJ0", "SepReformer_Large_DM_WSJ0"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--valid", type=int, default=500)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per child")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D", help="measure the weight EMA: Trainer.train_epoch without it against with it")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit to record when the tool runs from a tree without its .git (default: git rev-parse --short HEAD)")
    ap.add_argument("--ema-control", action="store_true", help="with --ema-decay: build BOTH Trainers without the EMA (what two instances of the same loop "
                    "differ by in one process); no trace")
    ap.add_argument("--ema-first", action="store_true", help="with --ema-decay: build and run the Trainer with the EMA first (default: second)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-model", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "loop":
        r = child_loop(args.child_model, args.steps, args.runs, args.valid) if args.ema_decay is None else \
            child_ema_loop(args.child_model, args.steps, args.runs, args.valid, args.ema_decay, args.ema_control, args.ema_first)
        print("RESULT " + json.dumps(r), flush=True)
        return
    if args.child == "trace":
        print("RESULT " + json.dumps(child_trace(args.ema_decay)), flush=True)
        return
    git = lambda *a: subprocess.run(["git", "-C", ROOT, *a], capture_output=True, text=True).stdout.strip()      # noqa: E731
    commit = args.commit or git("rev-parse", "--short", "HEAD") or None
    result = {"tool": "tools/train_run_bench.py", "commit": commit, "loops": []}
    if not args.commit and commit and git("status", "--porcelain", "--untracked-files=no"):
        result["commit"] = commit + " + uncommitted changes"
    for name in args.models:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "loop", "--child-model", name,
               "--steps", str(args.steps), "--runs", str(args.runs), "--valid", str(args.valid)]
        if args.ema_decay is not None:
            cmd += ["--ema-decay", str(args.ema_decay)] + (["--ema-control"] if args.ema_control else []) + (["--ema-first"] if args.ema_first else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)                    # the child's progress lines go straight to stderr
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"{name}: child ended with status {p.returncode}\n{p.stdout[-2000:]}")
        r = json.loads(line[-1][7:])
        result["loops"].append(r)
        if args.ema_control:
            print(f"{name}: control, both without the EMA: (a) {r['a']['median']:.2f} utt/s [{r['a']['min']:.2f} .. {r['a']['max']:.2f}]  "
                  f"(b) {r['b']['median']:.2f} utt/s [{r['b']['min']:.2f} .. {r['b']['max']:.2f}]", flush=True)
            continue
        if args.ema_decay is not None:
            print(f"{name}: (a) without {r['a']['median']:.1f} utt/s [{r['a']['min']:.1f} .. {r['a']['max']:.1f}]  (b) with the EMA {r['b']['median']:.1f} utt/s "
                  f"[{r['b']['min']:.1f} .. {r['b']['max']:.1f}]  pass {r['pass']}  averaged() around a validation pass {r['averaged_overhead_ms']:.2f} ms  "
                  f"exchange pair {r['swap_pair_ms']:.3f} ms  _foreach_lerp_ {r['foreach_lerp_ms']:.3f} ms  graphs {json.dumps(r['graphs'])}", flush=True)
            continue
        print(f"{name}: (a) bare {r['a']['median']:.1f} utt/s [{r['a']['min']:.1f} .. {r['a']['max']:.1f}]  (b) Trainer {r['b']['median']:.1f} utt/s "
              f"[{r['b']['min']:.1f} .. {r['b']['max']:.1f}]  pass {r['pass']}  (c) validation {r['c_valid_utt_s']:.1f} utt/s", flush=True)
    if not args.no_trace and not args.ema_control:
        result["kernel_trace"] = run_trace(args.ema_decay)
        print("kernel trace:", json.dumps(result["kernel_trace"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
