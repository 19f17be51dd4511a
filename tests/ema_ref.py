"""Restatement of the weight EMA (sepreformer_amd/optim.py) for its tests, independent of the module under
test: the decay schedule in Python floats (doubles, as the prepare kernel forms it) and one EMA step in numpy float32 with every
operation rounded - the kernel does not contract, so its result is this one bit for bit."""
import numpy as np


def decay_at(t, decay, warmup):
    """The decay of optimizer step ``t`` (1-based): ``decay``, ramped in as ``(1 + t) / (warmup + t)`` while that is smaller."""
    if warmup <= 0:
        return float(decay)
    return min(float(decay), (1.0 + float(t)) / (float(warmup) + float(t)))


def one_minus(t, decay, warmup):
    """What the prepare kernel leaves in scal[6]."""
    return np.float32(1.0 - decay_at(t, decay, warmup))


def ema_step(e, p, t, decay, warmup):
    """``e + (1 - d_t) * (p - e)`` in float32: a subtraction, a multiplication and an addition, each rounded."""
    e, p = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32)
    w = one_minus(t, decay, warmup)
    diff = (p - e).astype(np.float32)
    prod = (w * diff).astype(np.float32)
    return (e + prod).astype(np.float32)


def bits(a):
    """int32 view of a float32 array or tensor, for bitwise comparisons."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(-1).view(np.int32)


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))
