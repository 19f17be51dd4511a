#!/usr/bin/env python3
"""Device time of the BSS-eval metric behind PIT_SDRi (csrc/sepr_bsseval.hip, one sepr_bss_eval_fwd call over the
estimates AND the mixture), hipEvent-timed, against the CPU float64 restatement of mir_eval's bss_eval_sources
(tests/bss_eval_ref.py) per utterance on the same host.

    python tools/bss_bench.py [--out profiles/bss_eval_timing.json]
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
from sepreformer_amd.synth import synth_sources   # noqa: E402


def device_ms(B, T, S=2, reps=10, warmup=3):
    src = np.concatenate([synth_sources(B, T, seed=1 + k) for k in range((S + 1) // 2)], axis=1)[:, :S]     # [B,S,T]
    src = torch.from_numpy(src).permute(1, 0, 2).contiguous().to("cuda:0")                                  # [S,B,T]
    assert tuple(src.shape) == (S, B, T)
    g = torch.Generator().manual_seed(2)
    est = (src.roll(1, 0) * 0.9 + 0.05 * src + 0.01 * torch.randn(src.shape, generator=g).to("cuda:0")).contiguous()
    mix = src.sum(0).contiguous()
    lib = L.load()
    ws = torch.empty(lib.sepr_bss_eval_workspace(S, B, T), dtype=torch.uint8, device="cuda:0")
    outs = [torch.empty(B, S, dtype=torch.float64, device="cuda:0") for _ in range(4)]
    perm = torch.empty(B, S, dtype=torch.int32, device="cuda:0")
    status = torch.empty(B, dtype=torch.int32, device="cuda:0")
    lens = (L._i * B)(*([T] * B))
    st = torch.cuda.current_stream()

    def call():
        L.check(lib.sepr_bss_eval_fwd(est.data_ptr(), src.data_ptr(), mix.data_ptr(), lens, S, B, T, outs[0].data_ptr(),
                                      outs[1].data_ptr(), outs[2].data_ptr(), perm.data_ptr(), outs[3].data_ptr(),
                                      status.data_ptr(), ws.data_ptr(), ws.numel(), st.cuda_stream), "sepr_bss_eval_fwd")
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
    assert int(status.abs().sum()) == 0
    return {"B": B, "T": T, "S": S, "median_ms": float(np.median(times)), "min_ms": float(np.min(times)),
            "workspace_MB": ws.numel() / 1e6, "sdr_mean_dB": float(outs[0].mean())}


def cpu_s_per_utt(T, S=2):
    import bss_eval_ref as ref
    src = synth_sources(1, T, seed=1)[0].astype(np.float64)
    est = src[::-1] * 0.9 + 0.05 * src
    t0 = time.perf_counter()
    ref.pit_sdri(src, est, src.sum(0))                     # two bss_eval_sources calls, as PIT_SDRi makes
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0), "what": "sepr_bss_eval_fwd: estimates + mixture, float64",
           "runs": [device_ms(32, 32000), device_ms(1, 32000), device_ms(8, 32000, S=3)],
           "cpu_restatement_s_per_utt_4s": cpu_s_per_utt(32000), "cpu_threads": torch.get_num_threads()}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
