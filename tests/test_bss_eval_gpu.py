"""Device BSS-eval (csrc/sepr_bsseval.hip) against the explicit float64 restatement of mir_eval's bss_eval_sources
(tests/bss_eval_ref.py): permutations identical, SDR / SIR / SAR / mixture SDR within 1e-6 dB up to 60 dB and 1e-3 dB up to
100 dB; PIT_SDRi and the full test loop of the reference's engine."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bss_eval_ref as ref                                                  # noqa: E402

from sepreformer_amd import criterion as crit                               # noqa: E402
from sepreformer_amd import infer                                           # noqa: E402

DEV = "cuda:0"


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    for g, w in zip(got.ravel(), want.ravel()):
        if abs(w) <= 60:
            assert abs(g - w) <= 1e-6, (what, g, w)
        elif abs(w) <= 100:
            assert abs(g - w) <= 1e-3, (what, g, w)
        else:
            assert g > 100 or (w < 0 and g < -100), (what, g, w)


def _check(src, est, mix, lengths=None):
    """src / est [S,B,T] float32 numpy, mix [B,T]; device vs restatement per utterance over its valid length."""
    S, B, T = src.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)        # noqa: E731
    out = crit.bss_eval(t(src), t(est), mixture=t(mix), lengths=lengths)
    assert (out["status"] == 0).all()
    for b in range(B):
        n = T if lengths is None else lengths[b]
        sdr, sir, sar, perm = ref.bss_eval_sources(src[:, b, :n], est[:, b, :n])
        assert list(out["perm"][b]) == list(perm), (b, out["perm"][b], perm)
        _close(out["sdr"][b], sdr, "sdr")
        _close(out["sir"][b], sir, "sir")
        _close(out["sar"][b], sar, "sar")
        sdr_m = ref.bss_eval_sources(src[:, b, :n], np.stack([mix[b, :n]] * S))[0]
        _close(out["sdr_mix"][b], sdr_m, "sdr_mix")
    return out


def _speech_case():
    """Two disjoint 3 s references cut from a real 8 kHz utterance; estimates from gains, a short FIR, cross-talk and noise."""
    x = np.load(os.path.join(os.path.dirname(__file__), "golden", "e2e_base_sample_wav.npz"))["x"][0].astype(np.float64)
    n = 24000
    s = np.stack([x[1000:1000 + n], x[40000:40000 + n]])
    rng = np.random.default_rng(0)
    e0 = 0.7 * np.convolve(s[1], [1.0, 0.4, -0.2])[:n] + 0.05 * s[0] + 1e-3 * rng.standard_normal(n)
    e1 = 1.3 * s[0] + 0.1 * s[1] + 3e-3 * rng.standard_normal(n)
    est = np.stack([e0, e1]).astype(np.float32)[:, None]
    src = s.astype(np.float32)[:, None]
    return src, est, (src[0] + src[1])


@pytest.mark.gpu
def test_bss_eval_matches_restatement_on_golden_batches(golden):
    g = golden("criterion")
    _check(g["s2.src"], g["s2.est"], g["s2.mix"])
    _check(g["s3.src"], g["s3.est"], g["s3.mix"])                           # S = 3 at 3001 samples, the minimum is 1536


@pytest.mark.gpu
def test_bss_eval_real_speech_and_ragged_lengths(golden):
    src, est, mix = _speech_case()
    out = _check(src, est, mix)
    assert list(out["perm"][0]) == [1, 0]
    g = golden("criterion")
    _check(g["s2.src"][:, :4], g["s2.est"][:, :4], g["s2.mix"][:4], lengths=[8000, 1024, 5003, 2047])


@pytest.mark.gpu
def test_bss_eval_sources_surface_deterministic_and_silent():
    src, est, mix = _speech_case()
    r, e = torch.from_numpy(src[:, 0]).to(DEV), torch.from_numpy(est[:, 0]).to(DEV)
    a = crit.bss_eval_sources(r, e)
    b = crit.bss_eval_sources(r, e)
    assert all(x.shape == (2,) for x in a)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)                                         # bit-identical run to run
    want = ref.bss_eval_sources(src[:, 0], est[:, 0])
    assert list(a[3]) == list(want[3])
    _close(a[0], want[0], "sdr")
    with pytest.raises(ValueError, match="utterance 0"):
        crit.bss_eval_sources(r, torch.stack([e[0], torch.zeros_like(e[1])]))
    with pytest.raises(ValueError):
        crit.bss_eval_sources(torch.stack([r[0], torch.zeros_like(r[1])]), e)


@pytest.mark.gpu
def test_pit_sdri_matches_reference_call(golden):
    g = golden("criterion")
    for b in range(2):
        src, est, mix = g["s2.src"][:, b], g["s2.est"][:, b], g["s2.mix"][b]
        c = crit.PIT_SDRi(DEV, 0)
        tot, per = c(estims=[torch.from_numpy(est[s][None]).to(DEV) for s in range(2)], mixture=torch.from_numpy(mix[None]),
                     input_sizes=torch.tensor([mix.shape[-1]]), target_attr=[torch.from_numpy(src[s][None]) for s in range(2)])
        want_tot, want_per = ref.pit_sdri(src, est, mix)
        assert per.shape == (2,)
        _close(per, want_per, "sdri")
        assert abs(tot.item() - want_tot) <= 2e-6


@pytest.mark.gpu
def test_evaluate_utterances_full_test_loop(tmp_path):
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.model import Model
    from sepreformer_amd.synth import synth_sources
    model = Model.from_config(VARIANTS["tiny"], init_seed=0).load_synthetic_(0).eval().to(DEV)
    srcs = torch.from_numpy(synth_sources(3, 2001, seed=5))                         # [3, 2, 2001]
    utts = [(srcs[b].sum(0, keepdim=True), [srcs[b, 0:1], srcs[b, 1:2]], f"utt{b}.wav") for b in range(3)]
    m_si, m_sdr, n = infer.evaluate_utterances(model, utts, sisnr_csv_path=str(tmp_path / "si.csv"),
                                               sdr_csv_path=str(tmp_path / "sdr.csv"), wav_dir=str(tmp_path / "wav"))
    assert n == 3
    for name in ("si.csv", "sdr.csv"):
        rows = open(tmp_path / name).read().strip().split("\n")
        assert len(rows) == 3 and rows[0].startswith("utt0,") and len(rows[0].split(",")) == 3
    assert sorted(os.listdir(tmp_path / "wav"))[0] == "utt00_mixture.wav"
    m_si_only, n2 = infer.test_utterances(model, utts)
    assert n2 == 3 and m_si == m_si_only
    want = []
    for mix, src, _ in utts:
        est = np.stack([e[0].cpu().numpy() for e in infer.separate(model, mix)])
        want.append(ref.pit_sdri(torch.cat(src).numpy(), est, mix[0].numpy())[0] / 2)
    assert abs(m_sdr - float(np.mean(want))) < 1e-6, (m_sdr, want)
