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

With ``--rirs COUNT:RT60[,RT60...]`` the talkers sit in rooms (section 5h-2) and the bench measures ``sepr_conversation_render_rooms`` instead
(``--noise`` lays a noise bed under every conversation), on the same schedule beside the dry launch above:

  a. the rooms launch with synthetic banks of COUNT responses at each RT60 (the first one listed is used below);
  b. the rooms launch with every segment's ``rir = -1``: what the new skeleton costs over the dry one;
  c. the rooms launch on a schedule that is mostly silence (``p_overlap = 0``, ``pause = (2, 2)``) with the active share of (track, sample) pairs of
     both schedules: the time should fall roughly with it;
  d. the same render as float64 torch operations on the device - per segment an FFT convolution and a slice-add - and its largest difference;
  e. one ``evaluate_conversations(..., rirs=bank)`` call beside ``separate_long`` alone on the same mixtures.

The float64 FMAs the definition asks for - samples times taps, summed over the segments - over the launch time is reported against the device's
vector FP64 peak, and the LDS bytes those FMAs read (a group of 64 FMAs reads eight staged samples and eight taps: 2 bytes per FMA) against the
LDS read rate.

    python tools/conversation_bench.py --count 4 --minutes 10 --rirs 64:0.6,0.3,1.0 [--noise] --out profiles/conversation_rooms.json
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
FP64_FMA_PEAK = 78.6e12 / 2             # vector FP64 FMAs per second
LDS_READ_PEAK = 150e12                  # bytes per second, every CU streaming wide reads
LDS_BYTES_PER_FMA = 2.0                 # the rooms kernel: 16 doubles per group of 64 FMAs


def _stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "mean": sum(v) / len(v)}


def synth_corpus(dev, noise=False):
    """40 utterances of 3 - 8 s for each of 8 speakers in the two WSJ0 roles (pseudo-random PCM16: the kernels' time does not depend on the values);
    ``noise``: four of 20 - 40 s more in a role ``noise``."""
    import numpy as np
    from sepreformer_amd import datafeed as df
    rng = np.random.default_rng(0)
    arrays, keys = {}, []
    for i in range(40):
        a, b = f"{i % 8:03d}", f"{(i + 3) % 8:03d}"
        keys.append(f"k{i:03d}_{a}a{i:04d}_0.5_{b}b{i:04d}_-0.5")
        for role in ("s1", "s2"):
            arrays[f"{role}/{keys[-1]}"] = rng.integers(-6000, 6000, size=int(rng.integers(24000, 64000)), dtype=np.int16)
    beds = [f"n{i}" for i in range(4)] if noise else []
    for k in beds:
        arrays[f"noise/{k}"] = rng.integers(-2000, 2000, size=int(rng.integers(160000, 320000)), dtype=np.int16)
    corpus = df.Corpus.from_arrays(arrays, device=dev, fs=FS)
    corpus.roles = {"s1": list(keys), "s2": list(keys), **({"noise": beds} if noise else {})}
    return corpus, [arrays[nm] for nm in corpus.names]


def rooms_bench(args, corpus, dev, out):
    """The measurements a - e of the module's docstring, into ``out``."""
    import numpy as np
    import torch
    from sepreformer_amd import conversation as cv
    from sepreformer_amd import infer, longform, reverb
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.model import Model
    count, _, rts = args.rirs.partition(":")
    rts = [float(v) for v in rts.split(",")]
    noise = "noise" if args.noise else None
    seconds = 60.0 * args.minutes

    def bank_of(rt):
        return reverb.RirBank.from_arrays(reverb.synthetic_rirs(int(count), FS, rt60=rt, seed=0), FS, device=dev)

    def buffers(convs):
        table = cv.ConvTable(convs, dev)
        return table, torch.empty(table.total, device=dev), torch.empty(table.S_max, table.total, device=dev)

    def work(convs):
        """(float64 FMAs the definition asks for, share of (talker track, sample) pairs under a support)"""
        fma = sum(int((c.len.astype(np.int64) * (1 if c.taps is None else c.taps)).sum()) for c in convs)
        live = 0
        for c in convs:
            taps = np.ones(len(c.utt), np.int64) if c.taps is None else c.taps.astype(np.int64)
            for s in range(c.S):
                k = c.track == s
                lo, hi = c.place[k].astype(np.int64), np.minimum(c.n, c.place[k].astype(np.int64) + c.len[k] + taps[k] - 1)
                live += int(np.maximum(0, hi - np.maximum(lo, np.concatenate([[0], np.maximum.accumulate(hi)[:-1]]))).sum())
        return fma, live / float(sum(c.S * c.n for c in convs))

    res = {"rirs": args.rirs, "noise": bool(args.noise)}
    first = None
    for rt in rts:                                                   # a. one bank per RT60, the same draws otherwise
        bank = bank_of(rt)
        convs = [cv.plan_conversation(corpus, random.Random(i), seconds=seconds, rirs=bank, noise=noise) for i in range(args.count)]
        table, mix, tracks = buffers(convs)
        ms = _events(lambda: cv.render_into(corpus, table, mix, tracks, rirs=bank))
        fma, live = work(convs)
        rate = fma / (ms["median"] * 1e-3)
        res[f"rooms_rt60_{rt}"] = {"ms": ms, "mix_only_ms": _events(lambda: cv.render_into(corpus, table, mix, None, rirs=bank)),
                                   "taps": [int(bank.lengths.min()), int(bank.lengths.max())], "segments": table.G, "fp64_fma": fma,
                                   "active_share": live, "fma_per_s": rate, "share_of_fp64_peak": rate / FP64_FMA_PEAK,
                                   "lds_read_bytes_per_s": LDS_BYTES_PER_FMA * rate, "share_of_lds_read_rate": LDS_BYTES_PER_FMA * rate / LDS_READ_PEAK}
        if first is None:
            first = (bank, convs, table, mix, tracks)
    bank, convs, table, mix, tracks = first
    # b. the skeleton alone: the dry schedule through the rooms entry
    plain = [cv.plan_conversation(corpus, random.Random(i), seconds=seconds) for i in range(args.count)]
    none = [c._replace(rir=np.full(len(c.utt), -1, np.int32), taps=np.ones(len(c.utt), np.int32), direct=np.ones(len(c.utt), np.int32)) for c in plain]
    tb, mx, tr = buffers(none)
    res["rooms_entry_without_responses_ms"] = _events(lambda: cv.render_into(corpus, tb, mx, tr))
    # c. mostly silence
    sparse = [cv.plan_conversation(corpus, random.Random(i), seconds=seconds, p_overlap=0.0, pause=(2.0, 2.0), rirs=bank, noise=noise)
              for i in range(args.count)]
    tb, mx, tr = buffers(sparse)
    fma, live = work(sparse)
    res["rooms_sparse"] = {"ms": _events(lambda: cv.render_into(corpus, tb, mx, tr, rirs=bank)), "active_share": live, "fp64_fma": fma,
                           "segments": tb.G}
    del tb, mx, tr
    # d. float64 torch operations: per segment an FFT convolution, rounded to float32, scaled, slice-added
    f32 = corpus.buf16.to(torch.float32) * (1.0 / 32768.0)
    offs = corpus.offsets_host
    wet = torch.empty_like(tracks)
    ref_mix = torch.empty_like(mix)

    def conv(x, h):
        m = x.shape[0] + h.shape[0] - 1
        nfft = 1 << (m - 1).bit_length()
        return torch.fft.irfft(torch.fft.rfft(x.double(), nfft) * torch.fft.rfft(h.double(), nfft), nfft)[:m].float()

    def torch_rooms():
        wet.zero_()
        for r, c in enumerate(convs):
            o = int(table.out_off_host[r])
            for g in range(len(c.utt)):
                a = int(offs[c.utt[g]]) + int(c.start[g])
                x = f32[a:a + int(c.len[g])]
                p = o + int(c.place[g])
                if c.rir[g] < 0:
                    wet[int(c.track[g]), p:p + x.shape[0]] += (x * float(c.norm[g])) * float(c.gain[g])
                    continue
                h = bank.buf[int(bank.offsets_host[c.rir[g]]):int(bank.offsets_host[c.rir[g]]) + int(c.taps[g])]
                y = (conv(x, h) * float(c.norm[g])) * float(c.gain[g])
                m = min(y.shape[0], o + c.n - p)
                wet[int(c.track[g]), p:p + m] += y[:m]
        torch.sum(wet, 0, out=ref_mix)

    res["rooms_torch_fp64_fft_ms"] = _events(torch_rooms, warm=1, reps=3)
    cv.render_into(corpus, table, mix, tracks, rirs=bank)
    res["rooms_max_abs_diff_to_torch"] = float((mix - ref_mix).abs().max())
    res["rooms_max_abs"] = float(mix.abs().max())
    del wet, ref_mix, f32
    # e. the loop around the separator
    model = Model.from_config(VARIANTS["SepReformer_Base_WSJ0"], init_seed=0).load_synthetic_(0).eval().to(dev)
    rd = cv.Rendered(convs, table, mix, tracks)
    mixes = [rd.mixture(r).clone() for r in range(len(convs))]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    full = lambda: infer.evaluate_conversations(model, corpus, convs, method="long", rirs=bank)
    sep = lambda: longform.separate_long(model, mixes)
    wall(sep)
    wall(full)
    t_full, t_sep = [], []
    for _ in range(3):
        t_sep.append(wall(sep))
        t_full.append(wall(full))
    res["evaluate_s"], res["separate_long_s"] = _stats(t_full), _stats(t_sep)
    res["share_outside_separator"] = 1.0 - res["separate_long_s"]["median"] / res["evaluate_s"]["median"]
    out["rooms"] = res


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
    ap.add_argument("--rirs", default=None, metavar="COUNT:RT60[,RT60...]", help="measure the rooms launch instead: synthetic banks of COUNT responses")
    ap.add_argument("--noise", action="store_true", help="with --rirs: a noise bed under every conversation")
    args = ap.parse_args()
    if args.noise and not args.rirs:
        ap.error("--noise needs --rirs")
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
    corpus, utts = synth_corpus(dev, noise=args.noise)
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
    if args.rirs:                                                    # the dry launch above is the yardstick; the rest is the rooms'
        rooms_bench(args, corpus, dev, out)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return
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
