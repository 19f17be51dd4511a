"""Dynamic mixing without a device: the planners' draw order against the reference's recorded runs, the numpy
restatement (tests/dynmix_ref.py) against the reference's recorded outputs, the energies, ``Corpus.from_scp``, the C-ABI argument
checks of the new entries, and what ``datafeed.py`` may import."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_ref as ref                                                     # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import infer                                            # noqa: E402
from sepreformer_amd import lib as L_                                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANNERS = {"wsj0": df.plan_wsj0, "wham": df.plan_wham, "whamr": df.plan_whamr, "direct": df.plan_direct}


def host_corpus(g):
    """The fixture's corpus as a host-only ``Corpus`` with the restatement's energies."""
    arrays, roles = ref.fixture_corpus(g)
    c = df.Corpus.from_arrays(arrays, device=None, fs=8000)
    c.roles = roles
    c.set_energies(np.array([ref.energy(arrays[nm]) for nm in c.names], dtype=np.int64), np.zeros(0))
    return c, [arrays[nm] for nm in c.names]


def run_planner(g, tag, corpus):
    rng = random.Random(int(g[f"{tag}.seed"]))
    egs, digests = [], []
    for key in [str(k) for k in g["keys"]]:
        egs.append(PLANNERS[tag](corpus, rng, key, int(g["max_len"])))
        digests.append(ref.state_digest(rng.getstate()))
    return egs, digests


@pytest.mark.parametrize("tag", ["wsj0", "wham", "whamr", "direct"])
def test_planner_draw_order(golden, tag):
    """With the fixture's seed each planner yields the reference's lengths and keys, and the generator's state after EVERY example
    equals the reference's: the same number and kind of draws, the WSJ0 re-draw loop included."""
    g = golden("dynmix")
    corpus, _ = host_corpus(g)
    egs, digests = run_planner(g, tag, corpus)
    assert [e.n for e in egs] == g[f"{tag}.n_in"].tolist()
    assert digests == [str(d) for d in g[f"{tag}.digests"]]
    plan = df.collate_plan(corpus, egs)
    assert plan.keys == [str(k) for k in g[f"{tag}.keys_out"]]
    assert np.array_equal(plan.n.astype(np.float32), g[f"{tag}.input_sizes"]) and g[f"{tag}.input_sizes"].dtype == np.float32
    assert (plan.M, plan.S) == {"wsj0": (2, 2), "wham": (3, 2), "whamr": (3, 2), "direct": (2, 2)}[tag]


def test_wsj0_speaker_rule_rejects_draws(golden):
    """The fixture's keys make the reference's rule reject some partners, so the re-draw loop is really exercised."""
    keys = [str(k) for k in golden("dynmix")["keys"]]
    verdicts = [df.wsj0_distinct_speakers(a, b) for a in keys for b in keys]
    assert not all(verdicts) and any(verdicts)
    assert not df.wsj0_distinct_speakers(keys[0], keys[1]) and df.wsj0_distinct_speakers(keys[0], keys[0])


@pytest.mark.parametrize("tag", ["wsj0", "wham", "whamr", "direct"])
def test_restatement_against_reference(golden, tag):
    """Every example: lengths equal; every sample of ``_direct_load`` and of any term whose norm factor is exactly 1 bit-equal; every
    mixture and source >= 120 dB.  The only permitted difference is the RMS - numpy's pairwise float32 sum against the exact integer
    sum: a few float32 ulp on ref_rms, curr_rms and their ratio, <= ~4e-7 relative = -128 dB; 120 dB leaves 8 dB over that."""
    g = golden("dynmix")
    corpus, utts = host_corpus(g)
    egs, _ = run_planner(g, tag, corpus)
    plan = df.collate_plan(corpus, egs)
    T = g[f"{tag}.mixture"].shape[1]
    mix, src = ref.mix_batch(utts, plan.n, plan.utt, plan.start, plan.norm, plan.gain, plan.M, plan.S, T)
    want_mix, want_src = g[f"{tag}.mixture"], g[f"{tag}.src"]
    assert mix.shape == want_mix.shape and src.shape == want_src.shape
    exact = 0
    for b in range(len(plan.n)):
        n = int(plan.n[b])
        assert not want_mix[b, n:].any() and not mix[b, n:].any() and not src[:, b, n:].any()
        db = [ref.agreement_db(mix[b], want_mix[b])] + [ref.agreement_db(src[s, b], want_src[s, b]) for s in range(plan.S)]
        print(f"{tag} example {b}: n {n}, agreement {['%.1f' % d for d in db]} dB")
        assert min(db) >= 120.0, (tag, b, db)
        if tag == "direct":
            assert np.array_equal(mix[b], want_mix[b]) and np.array_equal(src[:, b], want_src[:, b])
            exact += 1 + plan.S
        else:
            for s in range(plan.S):
                if plan.norm[b, plan.M + s] == np.float32(1.0):
                    assert np.array_equal(src[s, b], want_src[s, b]), (tag, b, s)
                    exact += 1
    assert exact >= len(plan.n)                 # the first source of every example has norm factor ref / ref = 1


def test_energies(golden):
    arrays, _ = ref.fixture_corpus(golden("dynmix"))
    for nm, x in arrays.items():
        assert ref.energy(x) == int(np.sum(x.astype(np.int64) ** 2)), nm
    x = np.array([-32768] * 5 + [7], dtype=np.int16)
    assert ref.energy(x) == 5 * 2 ** 30 + 49
    c = df.Corpus.from_arrays({"a": x}, device=None)
    with pytest.raises(RuntimeError, match="energies"):
        c.rms
    c.set_energies(np.array([ref.energy(x)]), np.zeros(0))
    assert c.rms.dtype == np.float32 and c.rms[0] == ref.rms(x)


def test_corpus_from_scp(tmp_path):
    """PCM16 files stay int16 (and equal the file's samples), names / roles / offsets are right, a rate mismatch raises."""
    rng = np.random.default_rng(0)
    want, scps = {}, {}
    for role in ("s1", "s2"):
        lines = []
        for i, key in enumerate(("k0_a_b_c", "k1_a_b_c", "k2_a_b_c")):
            x = rng.uniform(-0.9, 0.9, size=900 + 37 * i + (5 if role == "s2" else 0))
            path = str(tmp_path / f"{role}_{key}.wav")
            infer.write_wav(path, x, 8000)
            want[f"{role}/{key}"] = np.clip(np.rint(x * 32767.0), -32768, 32767).astype(np.int16)
            lines.append(f"{key} {path}\n")
        scps[role] = str(tmp_path / f"{role}.scp")
        open(scps[role], "w").writelines(lines)
    from scipy.io import wavfile
    fpath = str(tmp_path / "float.wav")
    wavfile.write(fpath, 8000, rng.uniform(-0.5, 0.5, size=333).astype(np.float32))
    scps["noise"] = str(tmp_path / "noise.scp")
    open(scps["noise"], "w").write(f"k0_a_b_c {fpath}\n")
    c = df.Corpus.from_scp(scps, fs=8000, device=None)
    assert c.n16 == 6 and len(c) == 7 and c.names[:6] == list(want) and c.names[6] == "noise/k0_a_b_c"
    assert c.roles == {"s1": ["k0_a_b_c", "k1_a_b_c", "k2_a_b_c"], "s2": ["k0_a_b_c", "k1_a_b_c", "k2_a_b_c"], "noise": ["k0_a_b_c"]}
    assert c.lengths.tolist() == [len(v) for v in want.values()] + [333]
    assert c.offsets_host.tolist() == np.concatenate([[0], np.cumsum(c.lengths)]).tolist()
    assert (c.total16, c.total32) == (sum(len(v) for v in want.values()), 333)
    a16, a32 = c._host
    assert all(a.dtype == np.int16 and np.array_equal(a, w) for a, w in zip(a16, want.values()))
    assert a32[0].dtype == np.float32 and c.lookup("s2", "k1_a_b_c") == 4
    with pytest.raises(RuntimeError, match="sampling rate"):
        df.Corpus.from_scp(scps, fs=16000, device=None)
    with pytest.raises(RuntimeError, match="HIP device"):
        df.DynamicMixFeed(c, df.plan_wsj0, batch=2, max_len=400)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            df.Corpus.from_scp(scps, fs=8000, device="cuda:0")


def test_collate_plan_validates_terms(golden):
    g = golden("dynmix")
    corpus, _ = host_corpus(g)
    egs, _ = run_planner(g, "wsj0", corpus)
    u, s, nf, gn = egs[0].mix[0]
    bad = egs[0]._replace(mix=((u, int(corpus.lengths[u]) - egs[0].n + 1, nf, gn),) + egs[0].mix[1:])
    with pytest.raises(ValueError, match="reads"):
        df.collate_plan(corpus, [bad] + egs[1:])
    with pytest.raises(ValueError, match="terms"):
        df.collate_plan(corpus, [egs[0]._replace(mix=egs[0].mix[:1])])


def test_c_abi_argument_checks():
    """Every check comes before any HIP call: testable without a device."""
    lib = L_.load()
    assert lib.sepr_corpus_energy_workspace(0) == 0 and lib.sepr_corpus_energy_workspace(-3) == 0
    assert lib.sepr_corpus_energy_workspace(5) >= 5 * 8 * 8
    p = 0x1000                                                               # never dereferenced: the checks reject the call first
    rows2, rows3 = (C.c_void_p * 2)(p, p), (C.c_void_p * 3)(p, p, p)

    def mix(buf16=p, t16=100, buf32=None, t32=0, off=p, n16=3, N=3, tu=p, ts=p, tn=p, tg=p, n=p, B=2, M=2, S=2, T=64, out=p, rows=rows2):
        return lib.sepr_dynmix_fwd(buf16, t16, buf32, t32, off, n16, N, tu, ts, tn, tg, n, B, M, S, T, out, rows, None)

    E = L_.SEPR_EINVAL
    for kw in (dict(off=None), dict(tu=None), dict(ts=None), dict(tn=None), dict(tg=None), dict(n=None), dict(out=None), dict(rows=None),
               dict(rows=(C.c_void_p * 2)(p, None)), dict(buf16=None), dict(B=0), dict(B=-1), dict(S=1), dict(S=4, rows=rows3),
               dict(M=1), dict(M=4), dict(S=3, M=2, rows=rows3), dict(S=3, M=5, rows=rows3), dict(T=0), dict(T=62), dict(T=66),
               dict(out=p + 4), dict(buf16=p + 2), dict(N=0, n16=0), dict(n16=4), dict(N=4), dict(t16=0)):
        assert mix(**kw) == E, kw
    assert lib.sepr_corpus_energy(None, 100, None, 0, p, 3, 3, p, None, p, 1 << 20, None) == E
    assert lib.sepr_corpus_energy(p, 100, None, 0, None, 3, 3, p, None, p, 1 << 20, None) == E
    assert lib.sepr_corpus_energy(p, 100, None, 0, p, 3, 3, None, None, p, 1 << 20, None) == E
    assert lib.sepr_corpus_energy(p, 100, None, 0, p, 3, 4, p, None, p, 1 << 20, None) == E          # a float32 utterance without a buffer
    assert lib.sepr_corpus_energy(p, 100, None, 0, p, 3, 3, p, None, p, 8, None) == L_.SEPR_EWORKSPACE
    assert lib.sepr_corpus_energy(p, 100, None, 0, p, 3, 3, p, None, None, 0, None) == L_.SEPR_EWORKSPACE


def test_datafeed_imports_nothing_from_oracle_or_tests():
    src = open(os.path.join(ROOT, "sepreformer_amd", "datafeed.py")).read()
    for word in ("import oracle", "from oracle", "import tests", "from tests", "dynmix_ref"):
        assert word not in src, word
