"""Restatements for the epoch loop's tests (sepreformer_amd/trainer.py): the reference's expressions written
out again, independent of the module under test, and the host-side twins of what the device ledger accumulates."""
import math

import numpy as np
import torch


def ref_alpha(epoch):
    """engine.py:72, as written there."""
    return 0.4 * 0.8**(1+(epoch-101)//5) if epoch > 100 else 0.4


def lambda_lr_rates(base_lr, warmup_steps, batches):
    """The learning rate each batch of epoch 1 runs at in the reference: LambdaLR with the warm-up lambda of schedulers.py:20-23 on a
    dummy CPU optimizer, stepped once before each batch (engine.py:61)."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base_lr)

    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda step: float(step) / float(warmup_steps) if step < warmup_steps else 1.0)
    out = []
    for _ in range(batches):
        opt.step()
        sched.step()
        out.append(opt.param_groups[0]["lr"])
    return out


class HostLedger:
    """What sepr_run_ledger_update accumulates, on the host: float64 sums of the same fp32 values in the same order."""

    def __init__(self, nparts):
        self.nparts = nparts
        self.steps = self.skipped = self.nonfinite = self.clipped = 0.0
        self.gnorm_sum, self.gnorm_max = 0.0, 0.0
        self.part_sum, self.last = [0.0] * nparts, [0.0] * nparts

    def update(self, parts, gnorm=None, clip=None, skipped=False):
        if skipped:
            self.skipped += 1.0
            return
        self.steps += 1.0
        if any(not math.isfinite(v) for v in parts):
            self.nonfinite += 1.0
        for i, v in enumerate(parts):
            self.part_sum[i] += float(v)
            self.last[i] = float(v)
        if gnorm is not None:
            self.gnorm_sum += float(gnorm)
            self.gnorm_max = max(self.gnorm_max, float(gnorm))
            if float(clip) < 1.0:
                self.clipped += 1.0

    def values(self):
        return [self.steps, self.skipped, self.nonfinite, self.gnorm_sum, self.gnorm_max, self.clipped] + self.part_sum + self.last


def ref_epoch_means(per_batch_parts, num_spks):
    """engine.py:69,71,82-83: running sums of ``item() / num_spks`` per batch, the mean over stages, the mean over batches."""
    num_stages = len(per_batch_parts[0]) - 1
    tot_time, tot_freq, nb = 0, [0 for _ in range(num_stages)], 0
    for parts in per_batch_parts:
        nb += 1
        for idx in range(num_stages):
            tot_freq[idx] += parts[1 + idx] / num_spks
        tot_time += parts[0] / num_spks
    f = sum(tot_freq) / len(tot_freq)
    return tot_time / nb, f / nb, nb


def bits(t):
    """A tensor's bytes, for bitwise comparisons that must also hold for NaN."""
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b""


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bits(a) == bits(b)


def write_wav16(path, pcm, fs=8000):
    """A PCM16 mono wav file from an int16 array (the standard library's writer)."""
    import wave
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.asarray(pcm, dtype="<i2").tobytes())
