#!/usr/bin/env python3
"""Rendering and scoring conversations on the device (sepreformer_amd/conversation.py), on a synthetic PCM16 corpus.

  1. device time of one ``sepr_conversation_render`` launch - COUNT conversations of MINUTES minutes on two tracks, mixture and tracks -
     with hipEvents around each of 50 launches after warm-up (median, min, max); the same render as torch operations on the device (one
     slice-add per segment into zeroed rows, event-timed likewise) and as the numpy restatement on the host (wall clock, three runs);
  2. device time of one ``sepr_segment_sisnr_fwd`` call over the segments of one conversation against two channels (tracks plus noise),
     beside the float64 torch restatement of the same values on the device (one slice at a time);
  3. one ``infer.evaluate_conversations`` call (Base, synthetic weights, ``method="long"``) against ``separate_long`` alone on the same
     mixtures, alternating, three runs each, wall clock around a device synchronise: the share of the call spent outside the separator.

The bytes a render has to move - 4 bytes written per output sample and row, 2 read per source sample - over the launch time is reported as
a share of the HBM peak of 8 TB/s.  Nothing is asserted: the numbers go to the json file and DESIGN.md quotes them.

    python tools/conversation_bench.py [--count 4] [--minutes 2] [--out profiles/conversation.json]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS = 8000
HBM_PEAK = 8.0e12


def _stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "mean": sum(v) / len(v)}


def synth_corpus(dev):
    """40 utterances of 3 - 8 s for each of 8 speakers in the two WSJ0 roles (pseudo-random PCM16: the kernels' time does not depend on the values)."""
    import numpy as np
    from sepreformer_amd import datafeed as df
    rng = np.random.default_rng(0)
    arrays, keys = {}, []
    for i in range(40):
        a, b = f"{i % 8:03d}", f"{(i + 3) % 8:03d}"
        keys.append(f"k{i:03d}_{a}a{i:04d}_0.5_{b}b{i:04d}_-0.5")
        for role in ("s1", "s2"):
            arrays[f"{role}/{keys[-1]}"] = rng.integers(-6000, 6000, size=int(rng.integers(24000, 64000)), dtype=np.int16)
    corpus = df.Corpus.from_arrays(arrays, device=dev, fs=FS)
    corpus.roles = {"s1": list(keys), "s2": list(keys)}
    return corpus, [arrays[nm] for nm in corpus.names]


def _events(fn, warm=10, reps=50):
    import torch
    ms = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    return _stats(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--count", type=int, default=4)
    ap.add_argument("--minutes", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conversation.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("conversation_bench needs the HIP device: nothing is measured without it")
    import conversation_ref as ref
    from sepreformer_amd import conversation as cv
    from sepreformer_amd import infer, longform
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.model import Model
    dev = torch.device("cuda:0")
    corpus, utts = synth_corpus(dev)
    convs = [cv.plan_conversation(corpus, random.Random(i), seconds=60.0 * args.minutes) for i in range(args.count)]
    table = cv.ConvTable(convs, dev)
    mix = torch.empty(table.total, device=dev)
    tracks = torch.empty(table.S_max, table.total, device=dev)
    out = {"count": args.count, "minutes": args.minutes, "samples": table.total, "segments": table.G, "tracks": table.S_max}

    # 1. render
    out["render_ms"] = _events(lambda: cv.render_into(corpus, table, mix, tracks))
    out["render_mix_only_ms"] = _events(lambda: cv.render_into(corpus, table, mix, None))
    src = int(sum(int(c.len.sum()) for c in convs))
    moved = 4 * table.total * (1 + table.S_max) + 2 * src
    out["render_bytes"] = moved
    out["render_share_of_hbm_peak"] = moved / (out["render_ms"]["median"] * 1e-3) / HBM_PEAK
    f16 = corpus.buf16.to(torch.float32) * (1.0 / 32768.0)          # the torch restatement reads converted samples: conversion not timed
    offs = corpus.offsets_host

    def torch_render():
        tracks.zero_()
        for r, c in enumerate(convs):
            o = int(table.out_off_host[r])
            for g in range(len(c.utt)):
                a = int(offs[c.utt[g]]) + int(c.start[g])
                tracks[int(c.track[g]), o + int(c.place[g]):o + int(c.place[g]) + int(c.len[g])] = \
                    (f16[a:a + int(c.len[g])] * float(c.norm[g])) * float(c.gain[g])
        torch.add(tracks[0], tracks[1], out=mix)

    out["render_torch_ops_ms"] = _events(torch_render, warm=2, reps=10)
    cv.render_into(corpus, table, mix, tracks)
    torch.cuda.synchronize()
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want_mix, _, _ = ref.render_ref(utts, convs)
        host.append((time.perf_counter() - t0) * 1e3)
    out["render_numpy_ms"] = _stats(host)
    out["render_equals_numpy"] = bool(np.array_equal(mix.cpu().numpy().view(np.int32), want_mix.view(np.int32)))

    # 2. the metric, on the first conversation
    rd = cv.Rendered(convs, table, mix, tracks)
    c0 = convs[0]
    est = (rd.tracks_of(0) + 0.01 * torch.randn(c0.S, c0.n, device=dev)).contiguous()
    tr, mx = rd.tracks_of(0).contiguous(), rd.mixture(0)
    out["sisnr_segments"] = len(c0.utt)
    out["sisnr_ms"] = _events(lambda: cv.segment_sisnr(est, tr, mx, c0.track, c0.place, c0.len))

    def torch_sisnr():
        vals = []
        for g in range(len(c0.utt)):
            sl = slice(int(c0.place[g]), int(c0.place[g]) + int(c0.len[g]))
            r = tr[int(c0.track[g]), sl].double()
            r = r - r.mean()
            for a in (est[0, sl], est[1, sl], mx[sl]):
                a = a.double()
                a = a - a.mean()
                al = (a * r).sum() / ((r * r).sum() + 1e-15)
                vals.append(20 * torch.log10(1e-15 + (al * r).norm() / ((a - al * r).norm() + 1e-15)))
        return torch.stack(vals)

    out["sisnr_torch_ops_ms"] = _events(torch_sisnr, warm=2, reps=10)
    v, vm = cv.segment_sisnr(est, tr, mx, c0.track, c0.place, c0.len)
    want = torch_sisnr().view(-1, 3)
    out["sisnr_max_abs_diff_db"] = float(torch.max((torch.cat([v, vm[:, None]], 1) - want).abs()))

    # 3. the loop around the separator
    model = Model.from_config(VARIANTS["SepReformer_Base_WSJ0"], init_seed=0).load_synthetic_(0).eval().to(dev)
    mixes = [rd.mixture(r).clone() for r in range(len(convs))]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    full = lambda: infer.evaluate_conversations(model, corpus, convs, method="long")
    sep = lambda: longform.separate_long(model, mixes)
    wall(sep)                                                        # warm-up of every shape
    wall(full)
    t_full, t_sep = [], []
    for _ in range(3):
        t_sep.append(wall(sep))
        t_full.append(wall(full))
    out["evaluate_s"], out["separate_long_s"] = _stats(t_full), _stats(t_sep)
    out["share_outside_separator"] = 1.0 - out["separate_long_s"]["median"] / out["evaluate_s"]["median"]
    res = full()
    out["synthetic_weights_scores"] = {k: res[k] for k in ("sisnri_utt", "sisnri_cons", "switch_rate", "n")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
