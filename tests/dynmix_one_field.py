"""Plans that tell a complete "same term" comparison of the mixing kernels from one that forgets a field: S = 2,
M = 2, one example per field the form compares; example k copies both targets from their mixture terms and then changes field k alone.
Shared by tests/test_dynmix_gpu.py, test_dynmix_speed_gpu.py and test_dynmix_reverb_gpu.py, which compare the launch with their numpy
restatements bit for bit."""
import numpy as np
import torch

TMAX = 2052                                                                  # for the tiled forms one full tile of 2048 and one of 4


def plans(df, base, other):
    """``base[field]``: the values of the two mixture terms, ``other[field]``: the values of the two targets in the example that changes
    ``field``; the fields are ``BatchPlan``'s arrays, in its order.  -> (the plan whose targets ARE the mixture terms in every example,
    the plan whose example k differs from it in field k of both targets), every example ``TMAX`` samples long."""
    B = len(base)
    same = {f: np.tile(np.array(list(v) * 2, np.float32 if f in ("norm", "gain") else np.int32), (B, 1)) for f, v in base.items()}
    changed = {f: a.copy() for f, a in same.items()}
    for k, f in enumerate(base):
        changed[f][k, 2:] = other[f]
        assert not np.any(changed[f][k, 2:] == same[f][k, 2:]), f

    def plan(c):
        return df.BatchPlan([str(k) for k in range(B)], np.full(B, TMAX, np.int32), c["utt"], c["start"], c["norm"], c["gain"], 2, 2,
                            c.get("speed"), c.get("rir"), c.get("taps"))

    return plan(same), plan(changed)


def check(launch, restate, same, changed):
    """``restate(plan) -> (mix, src [S, B, T])`` on the CPU, ``launch(plan) -> (mix, [src_s])`` on the device.  By the restatement alone
    every changed target differs from its mixture term in at least one sample (so that a comparison which forgets the field shows);
    the launch equals the restatement bit for bit."""
    _, kept = restate(same)
    wm, ws = restate(changed)
    for k in range(ws.shape[1]):
        for s in range(ws.shape[0]):
            assert not torch.equal(ws[s, k], kept[s, k]), f"example {k}, target {s}: the changed field does not change the output"
    mix, src = launch(changed)
    torch.cuda.synchronize()
    assert torch.equal(mix.cpu(), wm)
    for k in range(ws.shape[1]):
        assert torch.equal(torch.stack(src).cpu()[:, k], ws[:, k]), f"example {k} (the field changed alone is number {k})"
