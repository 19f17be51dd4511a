#!/usr/bin/env python3
"""What every exported size entry returned BEFORE the workspace layouts were stated once (docs/HISTORY.md, "workspace layouts").

    git worktree add /tmp/parent <parent commit> && make -C /tmp/parent/sepreformer_amd/csrc
    cp /tmp/parent/sepreformer_amd/_native/libsepr_hip.so sepreformer_amd/_native/libsepr_hip_parent.so      # tools/README.md
    SEPR_LIB_VARIANT=parent python tests/golden/make_workspace_sizes.py

Calls the size entries of the PARENT commit's library (never the tree under test: the script refuses to run without
``SEPR_LIB_VARIANT``) over a grid of shapes and writes ``workspace_sizes.json``: per entry a list of ``[arg, ..., bytes]`` rows.
``tests/test_workspace_sizes_cpu.py`` asserts that the product library returns the same value for every row.  No device is needed.

The grid: the widths (F, N, H) of the tiny, Base and Large configurations, S in {2, 3}, the shapes (n, T, Tp) below - single rows,
sizes that are no multiple of any tile, the benchmark's batch of 32 four-second utterances - and per entry the shapes it refuses
(n = 0, S = 4, T below its minimum), for which it returns 0.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from sepreformer_amd import lib as L  # noqa: E402

WIDTHS = ((64, 64, 4), (128, 256, 8), (256, 256, 8))                     # (F, N, H): tiny, Base, Large
SPKS = (2, 3)
SHAPES = ((1, 1, 1), (1, 8, 1), (3, 1201, 0), (4, 1000, 250), (32, 8000, 500), (64, 8000, 500))   # (n, T, Tp); the last two: bench.py, B and B * S
REFUSED = ((0, 1000, 250), (4, 0, 0))                                    # n = 0, T = 0
OUT_SHAPES = ((4, 997, 1000), (4, 997, 250), (64, 7997, 8000), (64, 7997, 2000))     # TOP_OUT: (sequences, L, Tsrc), main and auxiliary heads
FRONT_SHAPES = ((2, 4000, 1000), (3, 4801, 1200), (32, 32000, 8000), (2, 15, 8))     # TOP_FRONT: (B, samples, Lp); the last below one filter


def cases():
    """name -> list of argument tuples."""
    c = {k: [] for k in ("sepr_workspace_bytes", "sepr_train_ctx_bytes", "sepr_train_ws_bytes", "sepr_linear_wgrad_workspace",
                         "sepr_pit_sisnr_mag_workspace", "sepr_pit_sisnr_mag_bwd_workspace", "sepr_bss_eval_workspace",
                         "sepr_stoi_workspace", "sepr_stitch_workspace", "sepr_resample_workspace", "sepr_corpus_energy_workspace",
                         "sepr_adamw_workspace")}
    for F, N, H in WIDTHS:
        for S in SPKS + (4,):
            for n, T, Tp in SHAPES + REFUSED:
                if S == 4 and (n, T, Tp) != (4, 1000, 250):
                    continue
                for op in range(8):                      # lib.OP_ENCODER .. lib.OP_PIT
                    c["sepr_workspace_bytes"].append((op, n, T, Tp, F, N, S))
                for top in range(12):                    # lib.TOP_GCFN .. lib.TOP_GCFN_FUSED16
                    shapes = [(n, T, Tp)]
                    if top in (L.TOP_EGA, L.TOP_EGA_X3) and Tp == 0 and T > 0:
                        shapes = [(n, T, T)]             # the sizing run divides by Tp: unpooled attention instead

                    if top == L.TOP_OUT and n == 4:
                        shapes += list(OUT_SHAPES)
                    if top == L.TOP_FRONT and n == 4:
                        shapes += list(FRONT_SHAPES)
                    for n_, T_, Tp_ in shapes:
                        c["sepr_train_ctx_bytes"].append((top, n_, T_, Tp_, F, N, S, H))
                        for K in ((0, 5, 65) if top in (L.TOP_CLA, L.TOP_DOWN) else (0,)):
                            c["sepr_train_ws_bytes"].append((top, n_, T_, Tp_, F, N, S, H, K))
        for M in (0, 1, 8, 3603, 4000, 512000):
            for n_, k_ in ((6 * F, F), (F, 3 * F), (N, 16), (2 * F * 3, F * 3)):
                c["sepr_linear_wgrad_workspace"].append((M, n_, k_))
    for S in (1, 2, 3, 4):
        for B in (0, 1, 5, 32):
            for T in (1, 37, 3001, 8000, 32000):
                c["sepr_pit_sisnr_mag_workspace"].append((S, B, T, 512, 128))
                c["sepr_pit_sisnr_mag_bwd_workspace"].append((S, B, T, 512, 128))
                c["sepr_bss_eval_workspace"].append((S, B, T))
                c["sepr_stoi_workspace"].append((S, B, T))
        c["sepr_pit_sisnr_mag_workspace"] += [(S, 4, 8000, 500, 128), (S, 4, 8000, 512, 130), (S, 4, 8000, 256, 64)]
        c["sepr_pit_sisnr_mag_bwd_workspace"] += [(S, 4, 8000, 500, 128), (S, 4, 8000, 512, 130), (S, 4, 8000, 256, 64)]
        for R, total in ((0, 0), (1, 1), (3, 7), (8, 40), (8, 7), (256, 5000)):
            c["sepr_stitch_workspace"].append((R, total, S))
    c["sepr_resample_workspace"] = [(R,) for R in (0, 1, 3, 64, 4096, 1 << 20)]
    c["sepr_corpus_energy_workspace"] = [(N,) for N in (0, 1, 100, 10000, 1 << 20)]
    c["sepr_adamw_workspace"] = [()]
    return c


def main():
    if not os.environ.get("SEPR_LIB_VARIANT"):
        raise SystemExit("set SEPR_LIB_VARIANT=parent: the golden values come from the parent commit's library, not from the tree under test")
    lib = L.load()
    out = {}
    for name, rows in cases().items():
        fn = getattr(lib, name)
        out[name] = [list(a) + [int(fn(*a))] for a in rows]
    path = os.path.join(HERE, "workspace_sizes.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": [\n' + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in v) + "\n ]"
                                   for k, v in out.items()) + "\n}\n")
    print(f"{path}: {sum(len(v) for v in out.values())} rows from {L.LIB_PATH}")


if __name__ == "__main__":
    main()
