#!/usr/bin/env python3
"""Graph-PIT and the conversation-window feed beside the training step they feed.

  1. ``kernels``: hipEvent time of ``sepr_graph_pit_assign`` + ``sepr_graph_pit_assemble`` (one ``GraphPIT`` call) at B = 16, T = 32000, U = 8,
     C = 2 on the tables of real window plans, and of each entry alone; and of the window render (``ConversationWindowFeed.write``: the table
     copy, the one render launch, the row copies) without rooms and with rooms and a noise bed, at B = 16 x 4 s;
  2. ``loop``: the bf16 training step (Base, batch 16 x 4 s, ``CapturedTrainStep`` + ``FlatAdamW``, the SA-SDR pair) fed by a ``Turns`` feed with
     ``criterion="sasdr"`` beside the step with Graph-PIT inside, fed by conversation windows in rooms over a bed - the same tree, alternating,
     three rounds of 20 steps, ms per step.  The two steps differ in more than Graph-PIT (the feed's launch, 7 target rows instead of 2), so the
     figure bounds what the new path costs end to end; the sasdr step's own spread across rounds is recorded beside it.

No bar is set: the figures are recorded.  Every step runs in a child process of its own under ``timeout -k 10 <s>``; the first that fails ends the run.

    python tools/graphpit_bench.py [--out profiles/graph_pit.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, T4S, B = 8000, 32000, 16
STEPS = [("kernels", 300), ("loop", 600)]
LOOP_STEPS, LOOP_RUNS = 20, 3
NSPK, NUTT = 12, 4


def _stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "mean": sum(v) / len(v)}


def speaker_of(name):
    role, _, key = name.partition("/")
    return role + key[:5]


def synth_corpus(dev):
    """12 speakers x 4 utterances of 2 - 6 s in each of the two talker roles - the same keys in both, as the mixing planners expect - and 8 noise
    utterances (pseudo-random PCM16; no kernel's time depends on the values)."""
    import numpy as np
    from sepreformer_amd import datafeed as df
    rng = np.random.default_rng(0)
    arrays, roles = {}, {"s1": [], "s2": [], "noise": []}
    for role in ("s1", "s2"):
        for j in range(NSPK):
            for i in range(NUTT):
                key = f"sp{j:03d}u{i}"
                arrays[f"{role}/{key}"] = rng.integers(-6000, 6000, size=int(rng.integers(16000, 48000)), dtype=np.int16)
                roles[role].append(key)
    for i in range(8):
        arrays[f"noise/n{i}"] = rng.integers(-1500, 1500, size=int(rng.integers(36000, 64000)), dtype=np.int16)
        roles["noise"].append(f"n{i}")
    corpus = df.Corpus.from_arrays(arrays, device=dev, fs=FS)
    corpus.roles = roles
    return corpus


def window_feed(corpus, bank=None, noise=False, seed=0):
    import functools
    from sepreformer_amd.conversation import plan_conversation
    from sepreformer_amd.convfeed import ConversationWindowFeed
    planner = functools.partial(plan_conversation, speakers=3, max_active=2, speaker_of=speaker_of, **({"noise": "noise"} if noise else {}))
    return ConversationWindowFeed(corpus, batch=B, max_len=T4S, channels=2, conversations=8, seconds=120.0, planner=planner, seed=seed, rirs=bank)


def _event_ms(fn, n=50, warm=5):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return _stats(out)


def step_kernels():
    import torch
    from sepreformer_amd.criterion import GraphPIT
    from sepreformer_amd.reverb import RirBank, synthetic_rirs
    dev = torch.device("cuda:0")
    corpus = synth_corpus(dev)
    bank = RirBank.from_arrays(synthetic_rirs(64, FS, rt60=(0.2, 0.6), seed=1), FS, device=dev)
    res = {}
    for name, feed in (("dry", window_feed(corpus)), ("rooms_and_bed", window_feed(corpus, bank, noise=True))):
        x = torch.zeros(B, T4S, device=dev)
        rows = [torch.zeros(B, T4S, device=dev) for _ in range(feed.rows)]
        plans = [feed.next_plan() for _ in range(8)]
        k = [0]

        def write():
            feed.write(plans[k[0] % len(plans)], x, rows)
            k[0] += 1

        res[f"window_write_{name}_ms"] = _event_ms(write)
        res[f"window_{name}"] = {"rows": feed.rows, "dropped": feed.dropped, "segments_per_batch": _stats([float(sum(len(w.conv.utt) for w in p.windows)) for p in plans]),
                                 "rows_used_per_window": _stats([float(w.used) for p in plans for w in p.windows])}
        t0 = time.perf_counter()
        for _ in range(20):
            feed.next_plan()
        res[f"window_plan_host_ms_{name}"] = (time.perf_counter() - t0) * 1e3 / 20
        if name == "dry":
            g = GraphPIT(dev, 2, feed.rows, B, T4S)
            g.load(plans[0].spans, plans[0].adj)
            feed.write(plans[0], x, rows)
            est = [x * 0.5, x * 0.5 + 0.01]
            res["graph_pit_call_ms"] = _event_ms(lambda: g(est, rows))
            res["graph_pit_assign_ms"] = _event_ms(lambda: g.assign(est, rows))
            res["graph_pit_assemble_ms"] = _event_ms(lambda: g.assemble(rows))
            torch.cuda.synchronize()
            res["graph_pit_status"] = g.status.tolist()
    return res


def step_loop():
    import functools
    import numpy as np
    import torch
    from sepreformer_amd import datafeed as df
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.criterion import GraphPIT, PIT_SASDR_mag, PIT_SASDR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.reverb import RirBank, synthetic_rirs
    from sepreformer_amd.train_step import CapturedTrainStep
    dev = torch.device("cuda:0")
    corpus = synth_corpus(dev)
    bank = RirBank.from_arrays(synthetic_rirs(64, FS, rt60=(0.2, 0.6), seed=1), FS, device=dev)
    cfg = VARIANTS["SepReformer_Base_WSJ0"]
    sizes = torch.full((B,), T4S)
    crit_t = PIT_SASDR_time(dev, cfg.num_spks)
    crit_m = PIT_SASDR_mag(dev, 512, 128, "hann", cfg.num_stages, cfg.num_spks)
    keys = list(corpus.roles["s1"])

    def make(graph_rows):
        torch.manual_seed(0)
        model = Model.from_config(cfg, init_seed=0, precision="bf16").load_synthetic_(0).to(dev).train()
        opt = FlatAdamW(model, lr=1.0e-4, weight_decay=1.0e-2)
        graph = GraphPIT(dev, cfg.num_spks, graph_rows, B, T4S) if graph_rows else None

        def loss_fn(audio, aux, *tg):
            tg = list(tg) if graph is None else graph(audio, list(tg))
            l_time = crit_t(estims=audio, input_sizes=sizes, target_attr=tg)
            l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=tg) for i, a in enumerate(aux)]
            return (0.6 * l_time + 0.4 * sum(l_mag) / len(l_mag)) / cfg.num_spks
        return model, opt, graph, loss_fn

    # the yardstick: criterion="sasdr" on a Turns feed (two sources drawn per example from the same corpus, any pair accepted)
    turns_feed = df.DynamicMixFeed(corpus, functools.partial(df.plan_wsj0, turns=df.Turns((0.0, 0.5), 80), accept=lambda a, b: True), batch=B,
                                   max_len=T4S, seed=0, fixed_length=True, keys=keys)
    wfeed = window_feed(corpus, bank, noise=True)
    steps = {}
    for name, feed, rows in (("sasdr_turns", turns_feed, 0), ("graph_sasdr_windows", wfeed, wfeed.rows)):
        model, opt, graph, loss_fn = make(rows)
        x = torch.zeros(B, T4S, device=dev)
        tg = [torch.zeros(B, T4S, device=dev) for _ in range(rows or cfg.num_spks)]
        plan = feed.next_into(x, tg)
        if graph is not None:
            graph.load(plan.spans, plan.adj)
        steps[name] = (CapturedTrainStep(model, loss_fn, opt, x, tg, max_norm=5.0, warmup=2), feed, graph)

    def loop(name):
        step, feed, graph = steps[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(LOOP_STEPS):
            plan = feed.next_into(step.x, step.targets)
            if graph is not None:
                graph.load(plan.spans, plan.adj)
            loss, _ = step(step.x, step.targets)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / LOOP_STEPS, float(loss.detach())

    for name in steps:
        loop(name)                                                            # warm every path
    runs, losses = {name: [] for name in steps}, {name: [] for name in steps}
    for _ in range(LOOP_RUNS):
        for name in steps:
            ms, ls = loop(name)
            runs[name].append(ms)
            losses[name].append(ls)
    status = steps["graph_sasdr_windows"][2].status.tolist()
    for step, _, _ in steps.values():
        step.release()
    assert all(np.isfinite(v) for vs in losses.values() for v in vs), losses
    a, g = runs["sasdr_turns"], runs["graph_sasdr_windows"]
    return {"model": "SepReformer_Base_WSJ0 bf16, batch 16 x 4 s, CapturedTrainStep + FlatAdamW, the SA-SDR pair, 0.6 / 0.4", "steps_per_run": LOOP_STEPS,
            "ms_per_step": runs, "last_losses": losses, "sasdr_turns_spread_ms": max(a) - min(a),
            "graph_minus_sasdr_ms": sum(g) / len(g) - sum(a) / len(a), "graph_over_sasdr": (sum(g) / len(g)) / (sum(a) / len(a)),
            "window_rows": wfeed.rows, "windows_dropped": wfeed.dropped, "graph_status_last_batch": status}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_pit.json"))
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps({"kernels": step_kernels, "loop": step_loop}[args.step]()), flush=True)
        return
    res = {"what": "python tools/graphpit_bench.py on one MI355X: hipEvents over 50 calls after warm-up; the loop alternates the two steps, three rounds "
                   "of 20 steps each in one process"}
    for name, limit in STEPS:
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.exit(f"step {name} failed (exit {p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        res[name] = json.loads(line[-1][7:])
        print(name, json.dumps(res[name]), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
