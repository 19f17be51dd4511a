#!/usr/bin/env python3
"""Device time of STOI / ESTOI (csrc/sepr_stoi.hip, one sepr_stoi_fwd call over the S estimates AND the mixture of every reference, both
measures), hipEvent-timed on 10 kHz input, the 8 kHz -> 10 kHz conversion of the same signals timed separately, against the CPU float64
restatement (tests/stoi_ref.py) per utterance on the same host.

    python tools/stoi_bench.py [--out profiles/stoi_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sepreformer_amd import criterion as crit     # noqa: E402
from sepreformer_amd import lib as L              # noqa: E402
from sepreformer_amd import resample as rs        # noqa: E402
from sepreformer_amd.synth import synth_sources   # noqa: E402


def _signals(B, T, S):
    src = np.concatenate([synth_sources(B, T, seed=1 + k) for k in range((S + 1) // 2)], axis=1)[:, :S]      # [B,S,T]
    src = torch.from_numpy(src).contiguous().to("cuda:0")
    g = torch.Generator().manual_seed(2)
    est = (src.roll(1, 1) * 0.9 + 0.05 * src + 0.01 * torch.randn(src.shape, generator=g).to("cuda:0")).contiguous()
    return src, est, src.sum(1).contiguous()


def _timed(call, reps, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}


def device_ms(B, T, S=2, reps=10, warmup=3):
    """T samples at 10 kHz per signal: the sepr_stoi_fwd call alone."""
    src, est, mix = _signals(B, T, S)
    lib = L.load()
    tab = crit.stoi_tables("cuda:0")
    ws = torch.empty(lib.sepr_stoi_workspace(S, B, T), dtype=torch.uint8, device="cuda:0")
    o = [torch.empty(B, S, S, dtype=torch.float64, device="cuda:0") for _ in range(2)] + \
        [torch.empty(B, S, dtype=torch.float64, device="cuda:0") for _ in range(2)] + \
        [torch.empty(B, S, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda:0")
    st = torch.cuda.current_stream()

    def call():
        L.check(lib.sepr_stoi_fwd(src.data_ptr(), est.data_ptr(), mix.data_ptr(), lens.data_ptr(), S, B, T, tab.data_ptr(), o[0].data_ptr(),
                                  o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), o[5].data_ptr(), ws.data_ptr(),
                                  ws.numel(), st.cuda_stream), "sepr_stoi_fwd")
    rec = {"B": B, "T_10k": T, "S": S, **_timed(call, reps, warmup), "workspace_MB": ws.numel() / 1e6,
           "stoi_mean": float(o[0].mean()), "estoi_mean": float(o[1].mean()), "kept_mean": float(o[4].double().mean())}
    assert int(o[5].abs().sum()) == 0
    return rec


def convert_ms(B, T8, S=2, reps=10, warmup=3):
    """The 8 kHz -> 10 kHz conversion of the 2 S + 1 signals per utterance (one sepr_resample_fwd launch, host wall time included)."""
    src, est, mix = _signals(B, T8, S)
    xs = [v for t in (src, est) for row in t for v in row] + list(mix)
    return {"B": B, "T_8k": T8, "signals": len(xs), **_timed(lambda: rs.resample_oct(xs, 8000, 10000), reps, warmup)}


def whole_call_wall_ms(B, T8, S=2, reps=5):
    """criterion.stoi end to end on 8 kHz input (conversion, packing, the kernels, no copy back), host wall time."""
    src, est, mix = _signals(B, T8, S)
    a, b = src.permute(1, 0, 2).contiguous(), est.permute(1, 0, 2).contiguous()
    crit.stoi(a, b, mixture=mix, fs=8000)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        crit.stoi(a, b, mixture=mix, fs=8000)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"B": B, "T_8k": T8, "median_ms": float(np.median(ts)), "min_ms": float(np.min(ts))}


def cpu_s_per_utt(T8, S=2):
    import stoi_ref as ref
    src = synth_sources(1, T8, seed=1)[0].astype(np.float64)
    est = src[::-1] * 0.9 + 0.05 * src
    t0 = time.perf_counter()
    for i in range(S):                                     # per reference: the S estimates and the mixture, both measures
        ref.evaluate(src[i], list(est) + [src.sum(0)], 8000)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0),
           "what": "sepr_stoi_fwd: STOI and ESTOI of S references against S estimates + mixture, float64, 10 kHz input",
           "runs": [device_ms(32, 40000), device_ms(1, 40000), device_ms(8, 40000, S=3)],
           "convert_8k_to_10k": [convert_ms(32, 32000), convert_ms(1, 32000)],
           "criterion_stoi_wall": [whole_call_wall_ms(32, 32000), whole_call_wall_ms(1, 32000)],
           "cpu_restatement_s_per_utt_4s": cpu_s_per_utt(32000), "cpu_threads": torch.get_num_threads()}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
