"""The image-source room simulator on the device: ``sepr_rir_ism_fwd`` against the brute-force numpy restatement
(tests/rirsim_ref.py) - the int64 sums exactly, the float32 responses bit for bit under both normalisations - run to run, under
reciprocity, through ``RirBank.simulate`` / ``resimulate`` into the mixing launch, and through ``DynamicMixFeed(rooms=...)``.

Shapes: the kernel's tile is W = 256 output samples, so N runs over {1, 40, 81, W - 1, W, W + 1, 2 W + 5}; a response of N' < N samples is a
prefix of the sums of N (tests/test_rirsim_cpu.py), so every room is restated once, at N = 517, and shared.  The 1.5 m cube at N = 517
holds some 10^4 images with reflection orders past 40 and spreads its columns over six of the eight column splits of a tile."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_ref as dr                                                      # noqa: E402
import dynmix_reverb_ref as mixref                                           # noqa: E402
import rirsim_ref as ref                                                     # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L_                                        # noqa: E402
from sepreformer_amd import reverb as rv                                     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = 256                                                                      # RS_W of sepr_rirsim.hip
NMAX = 2 * W + 5
NS = [1, 40, 81, W - 1, W, W + 1, NMAX]
GEOMETRY = ([5.0, 4.0, 3.0, 1.1, 1.3, 1.2, 3.7, 2.9, 1.6],                   # three rooms of different sizes ...
            [1.5, 1.5, 1.5, 0.4, 0.5, 0.6, 1.1, 0.9, 1.0],                   # ... the smallest cube the contract allows: many images, high orders
            [7.3, 6.1, 3.4, 6.0, 1.0, 2.9, 5.1, 1.7, 1.1])
BETAS = (0.0, 0.5, 0.95)
CLOSE = [5.0, 4.0, 3.0, 2.0, 2.0, 1.5, 2.1, 2.0, 1.5]                        # the source 0.1 m from the microphone: the pulse starts before t = 0
G = 64                                                                       # guard elements around every output


@functools.lru_cache(maxsize=None)
def restated(room, fs, N=NMAX):
    """The shared, read-only restatement of one room (a tuple of ten floats)."""
    acc, images = ref.ism_acc(list(room), fs / 343.0, N)
    acc.setflags(write=False)
    return acc, images


def device_ism(rooms, fs, N, normalise):
    """One call of the entry with guarded outputs -> (acc int64 [R, N], rir float32 [R, N], peak_idx int32 [R])."""
    rooms = np.ascontiguousarray(rooms, dtype=np.float64)
    R = rooms.shape[0]
    d_rooms = torch.from_numpy(rooms).to(DEV)
    lut = torch.from_numpy(rv.ism_lut()).to(DEV)
    acc = torch.full((R * N + 2 * G,), -77, dtype=torch.int64, device=DEV)
    rir = torch.full((R * N + 2 * G,), 123.0, dtype=torch.float32, device=DEV)
    peak = torch.full((R + 2 * G,), -5, dtype=torch.int32, device=DEV)
    L_.check(L_.load().sepr_rir_ism_fwd(d_rooms.data_ptr(), R, N, fs / 343.0, lut.data_ptr(), acc[G:].data_ptr(), rir[G:].data_ptr(),
                                        peak[G:].data_ptr(), normalise, torch.cuda.current_stream().cuda_stream), "sepr_rir_ism_fwd")
    torch.cuda.synchronize()
    for t, fill in ((acc, -77), (rir, 123.0), (peak, -5)):
        assert bool((t[:G] == fill).all()) and bool((t[-G:] == fill).all())
    return acc[G:-G].view(R, N).cpu().numpy(), rir[G:-G].view(R, N).cpu().numpy(), peak[G:-G].cpu().numpy()


def check(rooms, fs, N):
    """acc exactly, rir bit for bit under both normalisations, peak_idx - every room of the table against its restatement."""
    for normalise in (1, 0):
        acc, rir, peak = device_ism(rooms, fs, N, normalise)
        for r, room in enumerate(rooms):
            want, _ = restated(tuple(room), fs)
            want = want[:N]
            diff = np.nonzero(acc[r] != want)[0]
            assert diff.size == 0, (fs, N, r, diff[:5], acc[r][diff[:5]], want[diff[:5]])
            assert np.array_equal(rir[r].view(np.int32), ref.rir_from_acc(want, normalise).view(np.int32)), (fs, N, r, normalise)
            assert peak[r] == ref.peak_index(want), (fs, N, r)


@pytest.mark.parametrize("N", NS)
def test_sums_and_responses_bit_equal(N):
    """R = 3 rooms at fs 8000, every room under every beta of {0, 0.5, 0.95} (three tables, the betas rotated)."""
    for shift in range(3):
        rooms = [GEOMETRY[g] + [BETAS[(g + shift) % 3]] for g in range(3)]
        check(rooms, 8000, N)
    if N == NMAX:
        images = [restated(tuple(GEOMETRY[g] + [0.95]), 8000)[1] for g in range(3)]
        assert images[1] > 10000 and max(images) == images[1]
        assert np.abs(restated(tuple(GEOMETRY[1] + [0.95]), 8000)[0]).max() > 2 ** 40


def test_close_source_and_16_kHz():
    """The pulse of a source 0.1 m from the microphone is clipped at t < 0; one table at fs 16000; R = 1 and R = 4."""
    check([CLOSE + [0.5]], 8000, 300)
    acc, _ = restated(tuple(CLOSE + [0.5]), 8000)
    assert acc[0] != 0 and ref.peak_index(acc) == 2
    check([GEOMETRY[0] + [0.5], GEOMETRY[1] + [0.95], GEOMETRY[2] + [0.0], CLOSE + [0.95]], 16000, NMAX)


def test_two_launches_give_equal_bits():
    rooms = [GEOMETRY[g] + [0.95] for g in range(3)]
    a, b = device_ism(rooms, 8000, NMAX, 1), device_ism(rooms, 8000, NMAX, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    single = device_ism(rooms[1:2], 8000, NMAX, 1)                           # a room does not depend on its neighbours in the table
    assert np.array_equal(single[0][0], a[0][1]) and np.array_equal(single[1][0], a[1][1])


def test_reciprocity_on_the_device():
    rooms = [GEOMETRY[g] + [0.9] for g in range(3)]
    swapped = [r[:3] + r[6:9] + r[3:6] + r[9:] for r in rooms]
    a, b = device_ism(rooms, 8000, NMAX, 0), device_ism(swapped, 8000, NMAX, 0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)) and np.array_equal(a[2], b[2])
    assert np.abs(a[0]).max() > 2 ** 40


def small_corpus():
    rng = np.random.default_rng(11)
    arrays = {"u0": rng.integers(-20000, 20000, size=3000, dtype=np.int16), "u1": rng.normal(0, 0.1, size=2600).astype(np.float32)}
    corpus = df.Corpus.from_arrays(arrays, device=DEV)
    return corpus, [arrays[nm] for nm in corpus.names]


def test_simulate_and_resimulate():
    """``RirBank.simulate``: host layout, ``peak_idx`` and ``_direct`` from the one copy.  ``resimulate``: the same pointers, new contents;
    a plan made afterwards mixes bit-equal to tests/dynmix_reverb_ref.py over the new ``bank.host``."""
    N = 300
    first = np.array([GEOMETRY[g] + [0.5] for g in range(3)])
    second = np.array([GEOMETRY[(g + 1) % 3] + [0.95] for g in range(3)])
    bank = rv.RirBank.simulate(first, 8000, length=N, device=DEV)
    assert len(bank) == 3 and (bank.lengths == N).all() and np.array_equal(bank.offsets_host, [0, N, 2 * N, 3 * N]) and bank.total == 3 * N
    assert np.array_equal(bank.offsets.cpu().numpy(), bank.offsets_host)
    ptr, off_ptr = bank.buf.data_ptr(), bank.offsets.data_ptr()
    for rooms in (first, second):
        if rooms is second:
            before = bank.host.copy()
            assert bank.resimulate(second) is bank
            assert bank.buf.data_ptr() == ptr and bank.offsets.data_ptr() == off_ptr and len(bank) == 3 and (bank.lengths == N).all()
            assert not np.array_equal(bank.host, before)
        for r in range(3):
            want = restated(tuple(rooms[r]), 8000)[0][:N]
            assert np.array_equal(bank.rir(r).view(np.int32), ref.rir_from_acc(want, True).view(np.int32))
            assert bank.peak_idx[r] == ref.peak_index(want)
            assert bank._direct[r] == min(N, ref.peak_index(want) + 1 + rv.ISM_HW)      # the whole direct pulse
            assert bank.direct_taps()[r] == ref.peak_index(want) + 1                   # the generic meaning is unchanged
        assert np.array_equal(bank.buf.cpu().numpy(), bank.host)
    short = rv.RirBank.simulate(first[:1], 8000, length=90, device=DEV)     # the direct pulse (peak at 72) runs past the end: clipped
    assert short.peak_idx[0] == 72 and short._direct[0] == 90
    raw = rv.RirBank.simulate(first, 8000, length=N, device=DEV, normalise=None)
    assert np.array_equal(raw.rir(0).view(np.int32), ref.rir_from_acc(restated(tuple(first[0]), 8000)[0][:N], False).view(np.int32))
    with pytest.raises(ValueError, match="rooms for a bank"):
        bank.resimulate(first[:2])
    with pytest.raises(ValueError, match="all-zero"):                        # one sample ends before any direct path arrives
        rv.RirBank.simulate(first, 8000, length=1, device=DEV)
    # a plan made after resimulate: the mixture under the whole response, the targets under the direct pulse
    corpus, utts = small_corpus()
    ns = np.array([2052, 1000], np.int32)
    utt = np.array([[0, 1, 0, 1], [1, 0, 1, 0]], np.int32)
    start = np.array([[7, 0, 7, 0], [1600, 2000, 1600, 2000]], np.int32)
    rng = np.random.default_rng(2)
    norm, gain = rng.uniform(0.5, 2.0, size=(2, 2)).astype(np.float32), rng.uniform(0.5, 1.5, size=(2, 2)).astype(np.float32)
    norm, gain = np.concatenate([norm, norm], 1), np.concatenate([gain, gain], 1)
    rir = np.array([[0, 1, 0, 1], [2, 0, 2, 0]], np.int32)
    taps = np.where(np.arange(4)[None, :] < 2, N, bank._direct[rir]).astype(np.int32)
    plan = df.BatchPlan(["a", "b"], ns, utt, start, norm, gain, 2, 2, None, rir, taps)
    mix, src = df.mix_batch(corpus, plan, 2052, rirs=bank)
    hs = [bank.rir(r) for r in range(3)]
    wm, ws = mixref.batch(utts, hs, plan.n, plan.utt, plan.start, plan.norm, plan.gain, plan.rir, plan.taps, 2, 2, 2052)
    assert torch.equal(mix.cpu(), torch.from_numpy(wm)) and torch.equal(torch.stack(src).cpu(), torch.from_numpy(ws))


def test_feed_redraws_the_rooms(golden):
    """``DynamicMixFeed(rooms=sampler)``: the bank differs between epochs, is identical for equal (seed, epoch) - and equals the restatement
    of ``sampler.draw(R, seed=(seed, epoch))`` - and the planner's generator ends an epoch in the state of a feed without ``rooms``."""
    g = golden("dynmix")
    arrays, roles = dr.fixture_corpus(g)
    arrays = {nm: a for nm, a in arrays.items() if "_reverb/" not in nm}
    corpus = df.Corpus.from_arrays(arrays, device=DEV, fs=8000)
    corpus.roles = {r: k for r, k in roles.items() if not r.endswith("_reverb")}
    utts = [arrays[nm] for nm in corpus.names]
    sampler = rv.RoomSampler(rt60=(0.1, 0.2))
    R, N, B, T, SEED = 3, 256, 4, 2000, 5

    def feed(rooms, every=1):
        bank = rv.RirBank.simulate(sampler.draw(R, seed=99), 8000, length=N, device=DEV)
        return df.DynamicMixFeed(corpus, functools.partial(df.plan_whamr, rirs=bank), batch=B, max_len=T, seed=SEED, rirs=bank,
                                 fixed_length=True, rooms=rooms, rooms_every=every), bank

    (f1, b1), (f2, b2), (f0, b0), (fe, be) = feed(sampler), feed(sampler), feed(None), feed(sampler, 2)
    assert sampler.draw(R, seed=99).rt60.max() <= 0.2
    start = b0.host.copy()
    hosts = []
    for epoch in range(2):
        ptr = b1.buf.data_ptr()
        batches = list(f1)                                                   # one batch per epoch of four keys
        assert len(batches) == 1 and b1.buf.data_ptr() == ptr
        _, mix, src, _ = batches[0]
        plan = f1.last_plan
        hosts.append(b1.host.copy())
        want = sampler.draw(R, seed=(SEED, epoch))
        for r in range(R):
            acc, _ = ref.ism_acc(np.asarray(want[r]), 8000 / 343.0, N)
            assert np.array_equal(b1.rir(r).view(np.int32), ref.rir_from_acc(acc, True).view(np.int32)), (epoch, r)
        assert np.array_equal(plan.taps[:, 3:], b1._direct[plan.rir[:, 3:]]) and (plan.taps[:, :2] == N).all()
        wm, ws = mixref.batch(utts, [b1.rir(r) for r in range(R)], plan.n, plan.utt, plan.start, plan.norm, plan.gain, plan.rir, plan.taps,
                              plan.M, plan.S, T)
        assert torch.equal(mix.cpu(), torch.from_numpy(wm)) and torch.equal(torch.stack(src).cpu(), torch.from_numpy(ws))
        list(f2), list(f0), list(fe)
        assert np.array_equal(b2.host, b1.host)                              # equal (seed, epoch): identical banks
        assert np.array_equal(b0.host, start)                                # rooms=None: nothing changes
        assert f0.rng.getstate() == f1.rng.getstate() == f2.rng.getstate()   # the planner's generator is not touched
        assert f0.last_plan.keys == plan.keys and np.array_equal(f0.last_plan.rir, plan.rir) and np.array_equal(f0.last_plan.start, plan.start)
        assert np.array_equal(be.host, hosts[0])                             # rooms_every = 2: epoch 1 keeps the rooms of epoch 0
    assert not np.array_equal(hosts[0], hosts[1]) and not np.array_equal(hosts[0], start)
    list(fe)
    assert not np.array_equal(be.host, hosts[0])                             # epoch 2 redraws
    with pytest.raises(ValueError, match="simulate"):
        df.DynamicMixFeed(corpus, df.plan_whamr, batch=B, max_len=T, rooms=sampler)
    with pytest.raises(ValueError, match="simulate"):
        df.DynamicMixFeed(corpus, df.plan_whamr, batch=B, max_len=T, rooms=sampler, rirs=rv.RirBank.from_arrays([np.ones(4, np.float32)], 8000, device=DEV))
    with pytest.raises(ValueError, match="rooms_every"):
        df.DynamicMixFeed(corpus, df.plan_whamr, batch=B, max_len=T, rooms=sampler, rirs=b1, rooms_every=0)
