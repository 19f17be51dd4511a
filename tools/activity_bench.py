#!/usr/bin/env python3
"""Device time of the frame-activity launches of ``infer.evaluate_conversations(idle=True)`` (csrc/sepr_activity.hip)
on four 10-minute two-channel conversations, hipEvent-timed, medians of 50 after warm-up: the one ``sepr_frame_energy_fwd`` launch over the
frame-aligned scratch buffer (with its achieved bytes per second: the kernel reads every row once), the four ``sepr_frame_activity_fwd`` and
the four ``sepr_frame_class_sums_fwd`` calls, and beside them, in the same run, the four ``sepr_segment_sisnr_fwd`` calls of the same
evaluation.  Every call goes straight to the library on buffers made beforehand, so the figures are device time, not the wrappers' allocations.

    python tools/activity_bench.py [--out profiles/activity.json]
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sepreformer_amd import activity as act       # noqa: E402
from sepreformer_amd import conversation as cv    # noqa: E402
from sepreformer_amd import datafeed as df        # noqa: E402
from sepreformer_amd import lib as L              # noqa: E402

DEV = "cuda:0"


def timed(call, reps=50, warmup=5):
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
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--count", type=int, default=4)
    args = ap.parse_args()
    fs, C, frame, hang = 8000, 2, act.frame_samples(8000, 20.0), act.hang_frames(20.0, 200.0)
    rng = np.random.default_rng(0)
    corpus = df.Corpus.from_arrays({f"u{i:02d}": rng.normal(0, 0.05, size=int(rng.integers(2 * fs, 6 * fs))).astype(np.float32) for i in range(40)},
                                   device=DEV, fs=fs)
    convs = [cv.plan_conversation(corpus, random.Random(i), seconds=60.0 * args.minutes, speakers=2) for i in range(args.count)]
    rd = cv.render(corpus, convs)
    g = torch.Generator().manual_seed(1)
    est_all = (rd.tracks[:C] + 0.01 * torch.randn(C, rd.table.total, generator=g).to(DEV)).contiguous()
    lib, st = L.load(), torch.cuda.current_stream(DEV).cuda_stream

    offset = np.concatenate([[0], np.cumsum([-(-c.n // frame) for c in convs])]).astype(np.int64)
    pad = torch.zeros(C + 1, int(offset[-1]) * frame, dtype=torch.float32, device=DEV)
    for r, c in enumerate(convs):
        a, p = int(rd.out_off[r]), int(offset[r]) * frame
        pad[:C, p:p + c.n].copy_(est_all[:, a:a + c.n])
        pad[C, p:p + c.n].copy_(rd.mixture(r))
    rows, T = int(pad.shape[0]), int(pad.shape[1])
    e = torch.empty(rows, T // frame, dtype=torch.float64, device=DEV)
    energy = lambda: L.check(lib.sepr_frame_energy_fwd(pad.data_ptr(), rows, T, T, frame, e.data_ptr(), st), "sepr_frame_energy_fwd")
    energy()

    per = []                                                       # per conversation: the buffers of its activity, class-sums and SI-SNR calls
    for r, c in enumerate(convs):
        fa, fb = int(offset[r]), int(offset[r + 1])
        nF = fb - fa
        e_est, e_mix = e[:C, fa:fb].contiguous(), e[C, fa:fb].contiguous()
        active = torch.empty(C, nF, dtype=torch.uint8, device=DEV)
        level = torch.empty(C, dtype=torch.float64, device=DEV)
        ws_a = torch.empty(int(lib.sepr_frame_activity_bytes(C, nF)), dtype=torch.uint8, device=DEV)
        coloured = np.asarray(c.track, dtype=np.int64) % C
        cls = torch.from_numpy(cv.frame_classes((c.place, c.len), coloured, c.n, C, frame, int(0.25 * fs))).to(DEV)
        sums = torch.empty(C, 4, 4, dtype=torch.float64, device=DEV)
        ws_c = torch.empty(int(lib.sepr_frame_class_sums_bytes(C, nF)), dtype=torch.uint8, device=DEV)
        G = len(c.utt)
        seg = torch.from_numpy(np.stack([c.track, c.place, c.len]).astype(np.int32)).to(DEV)
        v, vm = torch.empty(G, C, dtype=torch.float64, device=DEV), torch.empty(G, dtype=torch.float64, device=DEV)
        ws_s = torch.empty(int(lib.sepr_segment_sisnr_bytes(G, C)), dtype=torch.uint8, device=DEV)
        a = int(rd.out_off[r])
        per.append(dict(nF=nF, G=G, n=int(c.n), e_est=e_est, e_mix=e_mix, active=active, level=level, ws_a=ws_a, cls=cls, sums=sums, ws_c=ws_c,
                        seg=seg, v=v, vm=vm, ws_s=ws_s, est=est_all[:, a:], ref=rd.tracks[:, a:], mix=rd.mix[a:]))

    def activity():
        for p in per:
            L.check(lib.sepr_frame_activity_fwd(p["e_est"].data_ptr(), C, p["nF"], 1e-4, 1e-12, hang, p["active"].data_ptr(), p["level"].data_ptr(),
                                                p["ws_a"].data_ptr(), p["ws_a"].numel(), st), "sepr_frame_activity_fwd")

    def class_sums():
        for p in per:
            L.check(lib.sepr_frame_class_sums_fwd(p["e_est"].data_ptr(), p["e_mix"].data_ptr(), p["active"].data_ptr(), p["cls"].data_ptr(), C,
                                                  p["nF"], p["sums"].data_ptr(), p["ws_c"].data_ptr(), p["ws_c"].numel(), st),
                    "sepr_frame_class_sums_fwd")

    def sisnr():
        for p in per:
            L.check(lib.sepr_segment_sisnr_fwd(p["est"].data_ptr(), p["ref"].data_ptr(), p["mix"].data_ptr(), p["seg"][0].data_ptr(),
                                               p["seg"][1].data_ptr(), p["seg"][2].data_ptr(), p["G"], C, 2, p["n"], rd.table.total, 1e-15,
                                               p["v"].data_ptr(), p["vm"].data_ptr(), p["ws_s"].data_ptr(), p["ws_s"].numel(), st),
                    "sepr_segment_sisnr_fwd")

    activity()
    rec = {"device": torch.cuda.get_device_name(0), "conversations": len(convs), "minutes": args.minutes, "channels": C, "frame": frame,
           "frames": int(offset[-1]), "segments": int(sum(p["G"] for p in per)), "reps": 50}
    for name, call in (("frame_energy", energy), ("frame_activity_x4", activity), ("frame_class_sums_x4", class_sums), ("segment_sisnr_x4", sisnr)):
        med, low = timed(call)
        rec[name] = {"median_ms": med, "min_ms": low}
    nbytes = rows * T * 4
    rec["frame_energy"].update(bytes_read=nbytes, GB_per_s=nbytes / (rec["frame_energy"]["median_ms"] * 1e-3) / 1e9)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
