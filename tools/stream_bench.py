#!/usr/bin/env python3
"""The stream bank measured (sepreformer_amd/streambank.py) -> profiles/stream_bank.json.

(a) Throughput on a corpus: a seeded synthetic corpus of 200 recordings of 10 - 30 s, Base, bf16x3, 4 s windows, 1 s overlap;
    ``separate_long(model, list)`` (the baseline: windows of one recording per forward) against ``separate_many(model, list,
    slots=32)`` (one window of 32 recordings per forward); five runs of each, alternating in one process, in seconds of audio per
    second of wall time.  Pass condition: median(bank) >= median(baseline) + (max - min of baseline) - the margin is the baseline's
    own spread in this call.
(b) Live cost: for A in {1, 8, 32} streams, the hipEvent device time per hop of the gather launch, the forward and the step launch,
    each against the same run's forward.  There is no bar: the ratio is written down.
    With ``--rate N`` / ``--out-rate N`` every stream is pushed at N Hz / returned at N Hz and converted inside the hop (DESIGN.md
    section 5c-3); the input-convert launch and the output-convert launch (with the history carry) are timed beside the others.
    Condition: both together take at most 5 % of the same hop's forward (median over the hops of one pass).

Each part runs in a child process of its own under ``timeout -k 10 <s>``; the first part that fails ends the run.

    python tools/stream_bench.py [--out profiles/stream_bank.json] [--rate N] [--out-rate N] [--parts corpus,live]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, NREC, RUNS, SLOTS = 8000, 200, 5, 32
PARTS = [("corpus", 900), ("live", 300)]                                  # (part, time limit in s)


def _model():
    import torch  # noqa: F401
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.model import Model
    return Model.from_config(VARIANTS["SepReformer_Base_WSJ0"], init_seed=0, precision="bf16x3").load_synthetic_(0).eval().to("cuda:0")


def _corpus():
    import numpy as np
    from sepreformer_amd.synth import synth_mixture
    rng = np.random.default_rng(2024)
    lengths = [int(v) for v in rng.integers(10 * FS, 30 * FS + 1, NREC)]
    pool = synth_mixture(1, 120 * FS, seed=17)[0]                          # synthesis is CPU-bound: recordings are crops of one pool
    starts = [int(v) for v in rng.integers(0, pool.numel() - 30 * FS, NREC)]
    return [pool[s:s + n].clone() for s, n in zip(starts, lengths)]


def _stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "runs": v}


def part_corpus():
    import torch
    from sepreformer_amd import longform, streambank
    m = _model()
    xs = [x.to("cuda:0") for x in _corpus()]                               # on the device for both: the copy is not what is compared
    audio = sum(x.numel() for x in xs) / FS
    longform.separate_long(m, xs[:8])                                      # warm-up: engine, workspaces, the batch shapes of both
    streambank.separate_many(m, xs[:40], slots=SLOTS)
    torch.cuda.synchronize()
    rate = {"separate_long": [], "separate_many": []}
    for _ in range(RUNS):
        for name, fn in (("separate_long", lambda: longform.separate_long(m, xs)),
                         ("separate_many", lambda: streambank.separate_many(m, xs, slots=SLOTS))):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            rate[name].append(audio / (time.perf_counter() - t0))
            assert len(out) == NREC and all(bool(torch.isfinite(o).all()) for o in out[0])
            del out
    a, b = _stats(rate["separate_long"]), _stats(rate["separate_many"])
    return {"recordings": NREC, "audio_s": audio, "slots": SLOTS, "unit": "audio seconds per second",
            "baseline_separate_long": a, "bank_separate_many": b,
            "condition": "median(bank) >= median(baseline) + (max - min of baseline)",
            "pass": "yes" if b["median"] >= a["median"] + (a["max"] - a["min"]) else "no"}


def part_live(rate=None, out_rate=None):
    import torch
    from sepreformer_amd import streambank
    from sepreformer_amd.synth import synth_mixture
    m = _model()
    hops, rows = 12, []
    fin = rate or FS
    for A in (1, 8, 32):
        bank = streambank.StreamBank(m, slots=A, max_rate=max(fin, out_rate or FS, 48000))
        L, M, K, Hh = streambank.geometry(fin, FS)

        def upto(n):                                                       # input samples that make n model-rate samples computable
            return n if fin == FS else (n - 1) * M // L + Hh + 2

        x = synth_mixture(1, upto(bank.W + (hops + 2) * bank.H), seed=A)[0].to("cuda:0")
        sids = [bank.open(fs_in=rate, fs_out=out_rate) for _ in range(A)]
        for sid in sids:
            bank.push(sid, x[:upto(bank.W)])
        for h in range(hops + 2):
            bank.profile = h >= 2                                          # two hops of warm-up (k = 0 has no boundary)
            assert len(bank.step()) == A
            for sid in sids:
                bank.push(sid, x[upto(bank.W + h * bank.H):upto(bank.W + (h + 1) * bank.H)])
        torch.cuda.synchronize()
        ms = [[e[i].elapsed_time(e[i + 1]) for i in range(5)] for e in bank.hop_events]
        med = [sorted(c)[len(c) // 2] for c in zip(*ms)]
        share = sorted((c[0] + c[4]) / c[2] for c in ms)
        rows.append({"A": A, "hops": len(ms), "convert_in_ms": med[0], "gather_ms": med[1], "forward_ms": med[2], "step_ms": med[3],
                     "convert_out_ms": med[4], "gather_over_forward": med[1] / med[2], "step_over_forward": med[3] / med[2],
                     "convert_over_forward": share[len(share) // 2], "convert_over_forward_max": share[-1]})
    out = {"unit": "median hipEvent device ms per hop", "rate_in": fin, "rate_out": out_rate or FS, "rows": rows}
    if fin != FS or (out_rate or FS) != FS:
        out["condition"] = "input plus output conversion (with the carry) at most 5 % of the same hop's forward, median over the hops"
        out["pass"] = "yes" if all(r["convert_over_forward"] <= 0.05 for r in rows) else "no"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bank.json"))
    ap.add_argument("--rate", type=int, default=None, help="live part: push every stream at this rate (default: the model's)")
    ap.add_argument("--out-rate", type=int, default=None, help="live part: return every stream at this rate (default: the model's)")
    ap.add_argument("--parts", default="corpus,live", help="which parts to run")
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part:
        fn = {"corpus": part_corpus, "live": lambda: part_live(args.rate, args.out_rate)}[args.part]
        print("RESULT " + json.dumps(fn()), flush=True)
        return 0
    result = {"model": "SepReformer_Base_WSJ0", "precision": "bf16x3", "chunk_seconds": 4.0, "overlap_seconds": 1.0}
    rates = [f"--{k}={v}" for k, v in (("rate", args.rate), ("out-rate", args.out_rate)) if v]
    for part, limit in PARTS:
        if part not in args.parts.split(","):
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part] + rates,
                           cwd=ROOT, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{part}: exit status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return 1
        result[part] = json.loads(line[-1][7:])
        print(part, json.dumps(result[part]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
