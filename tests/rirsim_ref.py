"""numpy restatement of the image-source room simulator, written from the definition in include/sepr.h
(``sepr_rir_ism_fwd``), by brute force: the FULL cube of image indices ``(k, p)`` per axis - no shell, no tiles, no intervals - the
per-image arithmetic exactly as defined (numpy rounds every float64 operation separately), and ``np.add.at`` into int64.  Integer sums do
not depend on the order, so the device's sums must equal these bit for bit.

The reference project has no room simulator; this restatement is the yardstick.
"""
import numpy as np

from sepreformer_amd.reverb import ISM_FB, ISM_HW, ISM_Q, ISM_TW, ism_lut

FOURPI = 4.0 * np.pi
SCALE = float(2 ** ISM_FB)


def axis_images(L, s, m, dmax):
    """(offset float64 [E], reflections int64 [E]) of every image index of one axis whose offset can lie within ``dmax``, and then some."""
    K = int(np.floor((dmax + s + m) / (2.0 * L))) + 2
    k = np.arange(-K, K + 1, dtype=np.int64)
    kf = k.astype(np.float64) * (2.0 * L)
    c0, c1 = s - m, -(s + m)
    off = np.concatenate([kf + c0, kf + c1])
    n = np.concatenate([np.abs(2 * k), np.abs(2 * k - 1)])
    return off, n


def ism_acc(room, fsc, N, lut=None, chunk=20000):
    """int64 [N] fixed-point sums of one room (``Lx Ly Lz sx sy sz mx my mz beta``), and the number of images that belong to it."""
    lut = ism_lut() if lut is None else lut
    room = np.asarray(room, dtype=np.float64)
    L, s, m, beta = room[0:3], room[3:6], room[6:9], float(room[9])
    fsc = float(fsc)
    dmax = (N + ISM_HW + 1) / fsc
    (ox, nx), (oy, ny), (oz, nz) = (axis_images(float(L[a]), float(s[a]), float(m[a]), dmax) for a in range(3))
    bpow = [1.0]
    for _ in range(int(nx.max() + ny.max() + nz.max())):
        bpow.append(bpow[-1] * beta)                                         # a sequential product, not pow
    bpow = np.array(bpow, dtype=np.float64)
    q = (ox * ox)[:, None] + (oy * oy)[None, :]
    d = np.sqrt(q[:, :, None] + (oz * oz)[None, None, :])
    tau = d * fsc
    i0 = np.floor(tau)
    keep = i0 - ISM_HW <= N - 1
    n = (nx[:, None, None] + ny[None, :, None] + nz[None, None, :])[keep]
    d, tau, i0 = d[keep], tau[keep], i0[keep]
    acc = np.zeros(N, dtype=np.int64)
    j = np.arange(ISM_TW, dtype=np.int64)
    for lo in range(0, d.shape[0], chunk):
        sl = slice(lo, lo + chunk)
        a = bpow[n[sl]] / (FOURPI * d[sl])
        f = tau[sl] - i0[sl]
        fq = f * float(ISM_Q)
        kf = np.floor(fq)
        w = fq - kf
        k = kf.astype(np.int64)
        v = lut[k] + w[:, None] * (lut[k + 1] - lut[k])
        c = np.rint((a[:, None] * v) * SCALE).astype(np.int64)               # half to even
        t = i0[sl].astype(np.int64)[:, None] - ISM_HW + j[None, :]
        ok = (t >= 0) & (t < N)
        np.add.at(acc, t[ok], c[ok])
    return acc, int(d.shape[0])


def peak_index(acc):
    """The first index of the maximum of ``|h|``."""
    return int(np.argmax(np.abs(acc)))


def rir_from_acc(acc, normalise):
    """float32 [N]: ``float32(h / max|h|)`` (an all-zero response stays zero) or ``float32(h)`` with ``h = acc / 2^48``."""
    h = acc.astype(np.float64) / SCALE
    if not normalise:
        return h.astype(np.float32)
    peak = float(np.max(np.abs(h)))
    if peak == 0.0:
        return np.zeros(acc.shape[0], dtype=np.float32)
    return (h / peak).astype(np.float32)


def direct_pulse(room, fsc, N, lut=None):
    """int64 [N]: the interpolated pulse of the direct path alone, tap by tap in scalar arithmetic."""
    lut = ism_lut() if lut is None else lut
    room = [float(v) for v in room]
    dx, dy, dz = (np.float64(room[3 + a]) - np.float64(room[6 + a]) for a in range(3))
    d = np.sqrt((dx * dx + dy * dy) + dz * dz)
    tau = d * np.float64(fsc)
    i0 = np.floor(tau)
    a = np.float64(1.0) / (np.float64(FOURPI) * d)
    fq = (tau - i0) * np.float64(ISM_Q)
    k = int(np.floor(fq))
    w = fq - np.floor(fq)
    acc = np.zeros(N, dtype=np.int64)
    if i0 - ISM_HW > N - 1:
        return acc
    for j in range(ISM_TW):
        t = int(i0) - ISM_HW + j
        if 0 <= t < N:
            v = lut[k][j] + w * (lut[k + 1][j] - lut[k][j])
            acc[t] += int(np.rint((a * v) * np.float64(SCALE)))
    return acc
