#!/usr/bin/env python3
"""Device time of the training criteria's eight entries (csrc/sepr_criterion.hip): the four ``sepr_pit_sasdr_*`` beside
their SI-SNR siblings ``sepr_pit_sisnr_*``, which share the moment pass and the STFT projection with them.

hipEvents around every launch, B = 16 x 32 000 samples, S = 2, the magnitude forms at 512 / 128; after a warm-up the entries run in turn, one
launch each per round, 100 rounds, so that clock and cache states are shared alike; the median, minimum and maximum of each entry in
microseconds.  ``--other-lib PATH``: all eight entries of a second build of the library (an earlier commit's) in the same rotation, and per entry
whether this build's median lies within the other build's own min - max band (``within_other_band``).

    python tools/criterion_bench.py [--other-lib sepreformer_amd/_native/libsepr_hip_<tag>.so] [--out profiles/sasdr.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, B, T, N, HOP = 2, 16, 32000, 512, 128
SIBLINGS = ("sepr_pit_sisnr_fwd", "sepr_pit_sisnr_bwd", "sepr_pit_sisnr_mag_fwd", "sepr_pit_sisnr_mag_bwd")
ENTRIES = SIBLINGS + tuple(n.replace("sisnr", "sasdr") for n in SIBLINGS)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from sepreformer_amd import lib as L
    from sepreformer_amd.criterion import PIT_SISNR_mag, _pit_time_bwd_bytes
    dev = torch.device("cuda:0")
    lib = L.load()
    g = torch.Generator().manual_seed(0)
    tgt = (0.1 * torch.randn(S, B, T, generator=g)).to(dev)
    est = (tgt.flip(0) + 0.03 * torch.randn(S, B, T, generator=g).to(dev)).contiguous()
    tgt[0, ::4] = 0.0                                                        # every fourth window has a silent talker
    gl = torch.full((B,), 1.0 / B, device=dev)
    crit = PIT_SISNR_mag(dev, N, HOP, "hann", 1, S, True, False)
    dft, dft_t = crit._dft, crit._dft_t
    loss, perm = torch.empty(B, device=dev), torch.empty(B, S, dtype=torch.int32, device=dev)
    dest = torch.empty_like(est)
    ws = torch.empty(max(_pit_time_bwd_bytes(lib, S, B, T), lib.sepr_pit_sisnr_mag_bwd_workspace(S, B, T, N, HOP)), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    e, t, p, w, n = est.data_ptr(), tgt.data_ptr(), perm.data_ptr(), ws.data_ptr(), ws.numel()

    def entries(h):
        return {
            "sepr_pit_sisnr_fwd": lambda: h.sepr_pit_sisnr_fwd(e, t, None, S, B, T, 1e-8, 1e-15, -30.0, loss.data_ptr(), p, None, None, w, n, st),
            "sepr_pit_sisnr_bwd": lambda: h.sepr_pit_sisnr_bwd(e, t, p, gl.data_ptr(), S, B, T, 1e-8, -30.0, dest.data_ptr(), w, n, st),
            "sepr_pit_sisnr_mag_fwd": lambda: h.sepr_pit_sisnr_mag_fwd(e, t, S, B, T, dft.data_ptr(), N, HOP, 1e-12, loss.data_ptr(), p, w, n, st),
            "sepr_pit_sisnr_mag_bwd": lambda: h.sepr_pit_sisnr_mag_bwd(e, t, p, gl.data_ptr(), S, B, T, dft.data_ptr(), dft_t.data_ptr(), N, HOP,
                                                                                    1e-12, dest.data_ptr(), w, n, st),
            "sepr_pit_sasdr_fwd": lambda: h.sepr_pit_sasdr_fwd(e, t, S, B, T, 1e-8, 30.0, loss.data_ptr(), p, w, n, st),
            "sepr_pit_sasdr_bwd": lambda: h.sepr_pit_sasdr_bwd(e, t, p, gl.data_ptr(), S, B, T, 1e-8, 30.0, dest.data_ptr(), w, n, st),
            "sepr_pit_sasdr_mag_fwd": lambda: h.sepr_pit_sasdr_mag_fwd(e, t, S, B, T, dft.data_ptr(), N, HOP, 1e-12, 30.0, loss.data_ptr(), p, w, n, st),
            "sepr_pit_sasdr_mag_bwd": lambda: h.sepr_pit_sasdr_mag_bwd(e, t, p, gl.data_ptr(), S, B, T, dft.data_ptr(), dft_t.data_ptr(), N, HOP,
                                                                                    1e-12, 30.0, dest.data_ptr(), w, n, st),
        }

    runs = {("this", k): f for k, f in entries(lib).items()}
    if args.other_lib:
        other = C.CDLL(os.path.abspath(args.other_lib))
        for name in ENTRIES:
            fn = getattr(other, name)
            fn.restype, fn.argtypes = L.SIGNATURES[name]
        runs.update({("other", k): f for k, f in entries(other).items()})
    with torch.cuda.device(dev):
        for f in runs.values():                                              # every forward before its backward: perm is valid
            for _ in range(args.warmup):
                L.check(f(), "warm-up")
        torch.cuda.synchronize()
        events = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, f in runs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = f()
                b.record()
                L.check(rc, k[1])
                events[k].append((a, b))
        torch.cuda.synchronize()
    res = {"shape": {"S": S, "B": B, "T": T, "frame_len": N, "frame_shift": HOP}, "rounds": args.rounds, "unit": "us", "device": torch.cuda.get_device_name(0),
           "build": L.build_info(), "entries": {}}
    for (which, name), ev in events.items():
        us = [1000.0 * a.elapsed_time(b) for a, b in ev]
        res["entries"][f"{name}@{which}"] = {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}
    base = "other" if args.other_lib else "this"
    res["difference_us"] = {n.replace("sisnr", "sasdr"): round(res["entries"][n.replace("sisnr", "sasdr") + "@this"]["median"] - res["entries"][f"{n}@{base}"]["median"], 2)
                            for n in SIBLINGS}
    res["difference_against"] = f"the SI-SNR entries of the {'other' if args.other_lib else 'same'} library"
    if args.other_lib:
        res["within_other_band"] = {n: res["entries"][f"{n}@other"]["min"] <= res["entries"][f"{n}@this"]["median"] <= res["entries"][f"{n}@other"]["max"]
                                    for n in ENTRIES}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
