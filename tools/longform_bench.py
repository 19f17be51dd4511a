#!/usr/bin/env python3
"""Long-form separation throughput (sepreformer_amd/longform.py): seconds of audio separated per second
of wall time by ``separate_long`` on Base (bf16x3, batch 32, 4 s windows, 1 s overlap) at 60 s, 10 min and 60 min of synthetic
mixture, the hipEvent device time of the stitch launches alone, and for comparison the whole-file ``separate`` at 20 s and
60 s only (its behaviour on longer input is not probed).

Every step runs in a child process of its own under ``timeout -k 10 <s>``; the first step that fails ends the run.

    python tools/longform_bench.py [--out profiles/longform_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 8000
# (step name, seconds of audio, time limit of the step in s)
STEPS = [("long", 60, 240), ("long", 600, 300), ("long", 3600, 420), ("whole", 20, 180), ("whole", 60, 240)]


def _model():
    import torch  # noqa: F401
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.model import Model
    return Model.from_config(VARIANTS["SepReformer_Base_WSJ0"], init_seed=0, precision="bf16x3").load_synthetic_(0).eval().to("cuda:0")


def _mixture(seconds):
    import torch
    from sepreformer_amd.synth import synth_mixture
    n = seconds * FS
    piece = synth_mixture(1, min(n, 600 * FS), seed=3)[0]                 # a 10-minute pattern repeated (synthesis is CPU-bound)
    return torch.cat([piece] * (-(-n // piece.numel())))[:n]


def step_long(seconds):
    import torch
    from sepreformer_amd import longform
    m = _model()
    x = _mixture(seconds)
    longform.separate_long(m, x[:60 * FS])                                 # warm-up: engine, workspace, both batch shapes
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, plan = longform.separate_long(m, x, return_plan=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert all(bool(torch.isfinite(o).all()) for o in out)
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        longform.stitch(plan["chunks"], plan["lengths"], plan["O"], False)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    nc = plan["chunks"].shape[0]
    return {"mode": "separate_long", "audio_s": seconds, "chunks": int(nc), "wall_s": wall, "audio_s_per_s": seconds / wall,
            "stitch_device_ms_median": sorted(times)[len(times) // 2], "stitch_device_ms_min": min(times),
            "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}


def step_whole(seconds):
    import torch
    from sepreformer_amd import infer
    m = _model()
    x = _mixture(seconds)[None]
    infer.separate(m, x)                                                   # warm-up at the same shape
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = infer.separate(m, x)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert all(bool(torch.isfinite(o).all()) for o in out)
    return {"mode": "separate (whole file)", "audio_s": seconds, "wall_s": wall, "audio_s_per_s": seconds / wall,
            "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--seconds", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        rec = step_long(args.seconds) if args.step == "long" else step_whole(args.seconds)
        import torch
        rec["device"] = torch.cuda.get_device_name(0)
        print("__RESULT__" + json.dumps(rec))
        return
    runs, failed = [], None
    for name, seconds, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--seconds", str(seconds)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("__RESULT__")]
        if r.returncode != 0 or not lines:
            failed = {"step": name, "audio_s": seconds, "returncode": r.returncode, "stderr_tail": r.stderr[-1500:]}
            print(json.dumps(failed), file=sys.stderr)
            break                                                          # nothing more runs on the device after a failure
        runs.append(json.loads(lines[-1][len("__RESULT__"):]))
        print(json.dumps(runs[-1]), flush=True)
    rec = {"device": runs[0]["device"] if runs else None,
           "what": "Base bf16x3, synthetic weights; separate_long: 4 s windows, 1 s overlap, batch 32, no gain matching",
           "runs": runs}
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
