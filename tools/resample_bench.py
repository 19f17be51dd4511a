#!/usr/bin/env python3
"""Sample-rate conversion time (sepreformer_amd/resample.py) beside what it feeds: 60 s, 10 min and 60 min of
48 kHz -> 8 kHz and 44.1 kHz -> 8 kHz (one track in) and 8 kHz -> 44.1 kHz (two tracks out), each with hipEvents around
``resample`` (warm-up, then several repetitions: median, min, max) and as host wall time of the call; ``separate_long`` (Base,
bf16x3, batch 32, 4 s windows) on the same length of audio in the same run; ``scipy.signal.resample_poly`` on the host with the
same prototype filter (single-threaded: a 16-way thread split of the signal measured no gain, the filter loop holds the GIL).

The condition of section 5d: input + output conversion take at most 5 % of the ``separate_long`` time of the same recording.

Every step runs in a child process of its own under ``timeout -k 10 <s>``; the first step that fails ends the run.

    python tools/resample_bench.py [--out profiles/resample_timing.json] [--no-host]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FS = 8000
LENGTHS = [60, 600, 3600]
JOBS = [("in_48k", 48000, 8000, 1), ("in_44k1", 44100, 8000, 1), ("out_44k1", 8000, 44100, 2)]      # name, fs_in, fs_out, tracks
REPS, WARM = 7, 2
PEAK_F64_TFLOPS, PEAK_HBM_TBS = 78.6, 8.0                                  # MI355X data sheet: vector float64, HBM3E
STEPS = [("resample", 420), ("long", 600), ("host", 900)]                   # step, time limit in s


def _stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def step_resample():
    import torch
    from sepreformer_amd import resample as rs
    out = []
    for name, fs_in, fs_out, tracks in JOBS:
        p = rs.plan(fs_in, fs_out)
        for seconds in LENGTHS:
            g = torch.Generator(device="cuda:0").manual_seed(seconds)
            xs = [torch.randn(seconds * fs_in, device="cuda:0", generator=g) for _ in range(tracks)]
            arg = xs[0] if tracks == 1 else xs
            dev_ms, wall_ms = [], []
            for i in range(WARM + REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                y = rs.resample(arg, fs_in, fs_out)
                e1.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if i >= WARM:
                    dev_ms.append(e0.elapsed_time(e1))
                    wall_ms.append((t1 - t0) * 1e3)
            ys = [y] if tracks == 1 else y
            assert all(bool(torch.isfinite(v).all()) for v in ys)
            n_out = sum(int(v.shape[0]) for v in ys)
            med = _stats(dev_ms)["median"] * 1e-3
            fma = n_out * p.K
            nbytes = 4 * (tracks * seconds * fs_in + n_out)
            out.append({"job": name, "fs_in": fs_in, "fs_out": fs_out, "tracks": tracks, "audio_s": seconds, "L": p.L, "M": p.M, "K": p.K,
                        "outputs": n_out, "device_ms": _stats(dev_ms), "wall_ms": _stats(wall_ms), "reps": REPS,
                        "gfma_per_s": fma / med / 1e9, "fraction_of_f64_vector_peak": 2 * fma / med / (PEAK_F64_TFLOPS * 1e12),
                        "hbm_GBs": nbytes / med / 1e9, "fraction_of_hbm_peak": nbytes / med / (PEAK_HBM_TBS * 1e12)})
            del xs, arg, y, ys
            torch.cuda.empty_cache()
    return {"conversions": out, "device": torch.cuda.get_device_name(0)}


def step_long():
    import torch
    from longform_bench import _mixture, _model
    from sepreformer_amd import longform
    m = _model()
    longform.separate_long(m, _mixture(60))                                # warm-up: engine, workspace, both batch shapes
    torch.cuda.synchronize()
    out = []
    for seconds in LENGTHS:
        x = _mixture(seconds).to("cuda:0")
        walls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = longform.separate_long(m, x)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        assert all(bool(torch.isfinite(o).all()) for o in y)
        out.append({"audio_s": seconds, "wall_s": _stats(walls), "reps": 3})
    return {"separate_long": out}


def step_host():
    import numpy as np
    from scipy.signal import resample_poly
    from sepreformer_amd import resample as rs
    out = []
    for name, fs_in, fs_out, tracks in JOBS:
        p = rs.plan(fs_in, fs_out)
        h = np.zeros(2 * (p.Hh + 1) * p.L + 1)
        for ph in range(p.L):
            h[(p.Hh + 1) * p.L + ph + (p.Hh - np.arange(p.K)) * p.L] = p.taps[ph].astype(np.float64) / p.L
        for seconds in LENGTHS:
            x = np.random.default_rng(seconds).standard_normal(seconds * fs_in).astype(np.float32)
            t0 = time.perf_counter()
            for _ in range(tracks):
                resample_poly(x, p.L, p.M, window=h)
            out.append({"job": name, "audio_s": seconds, "tracks": tracks, "wall_s": time.perf_counter() - t0})
    return {"host_resample_poly": out, "host_threads": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the scipy comparison (minutes of host time)")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        rec = {"resample": step_resample, "long": step_long, "host": step_host}[args.step]()
        print("__RESULT__" + json.dumps(rec))
        return
    rec, failed = {}, None
    for name, limit in STEPS:
        if name == "host" and args.no_host:
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("__RESULT__")]
        if r.returncode != 0 or not lines:
            failed = {"step": name, "returncode": r.returncode, "stderr_tail": r.stderr[-1500:]}
            print(json.dumps(failed), file=sys.stderr)
            break                                                          # nothing more runs on the device after a failure
        rec.update(json.loads(lines[-1][len("__RESULT__"):]))
        print(name, "done", flush=True)
    if not failed:
        conv = {(c["job"], c["audio_s"]): c for c in rec["conversions"]}
        cond = []
        for sl in rec["separate_long"]:
            s = sl["audio_s"]
            for jin in ("in_48k", "in_44k1"):
                ms = conv[(jin, s)]["wall_ms"]["median"] + conv[("out_44k1", s)]["wall_ms"]["median"]
                dms = conv[(jin, s)]["device_ms"]["median"] + conv[("out_44k1", s)]["device_ms"]["median"]
                cond.append({"audio_s": s, "input": jin, "output": "out_44k1", "conversion_wall_ms": ms, "conversion_device_ms": dms,
                             "separate_long_wall_ms": sl["wall_s"]["median"] * 1e3,
                             "fraction_wall": ms / (sl["wall_s"]["median"] * 1e3), "fraction_device": dms / (sl["wall_s"]["median"] * 1e3)})
        rec["condition_at_most_0.05"] = cond
        try:
            import kres
            rec["kernel_resources"] = kres.resources(os.path.join(ROOT, "sepreformer_amd", "_native", "libsepr_hip.so"), "resample_kernel")
        except Exception as e:                                             # the figures above do not depend on it
            rec["kernel_resources"] = repr(e)
    rec["what"] = ("resample: hipEvents and host wall around one call, noise input; separate_long: Base bf16x3, synthetic weights, 4 s windows, "
                   "1 s overlap, batch 32; host: scipy.signal.resample_poly with the same prototype filter")
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
