"""Device STOI / ESTOI (csrc/sepr_stoi.hip through criterion.stoi) against the float64 restatement (tests/stoi_ref.py) on the inputs of
tests/stoi_cases.py: references from a real utterance with inserted pauses, so that frames really are removed (asserted), and no frame
within 0.01 dB of the keep / remove threshold (asserted), so that `kept` must equal the restatement's.

Tolerance.  The device design rounds twice where the definition stays in float64: the converter's taps and the 10 kHz signals are
float32.  DELTA is the largest change of the restatement's own values on these inputs when exactly those two roundings are applied to
it, measured on the CPU (stoi_cases.delta): ragged_8k 1.73e-8, three_8k 8.45e-9, one_16k 3.98e-9, long_10k 0 (no conversion, and the
inputs are float32 already).  TOL = 100 DELTA: two orders of margin for the different transform formulation and summation orders.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stoi_cases as sc                                                      # noqa: E402
import stoi_ref as ref                                                       # noqa: E402

from sepreformer_amd import criterion as crit                                # noqa: E402
from sepreformer_amd import infer                                            # noqa: E402

DEV = "cuda:0"
DELTA = 1.73e-8
TOL = 100 * DELTA
KEYS = ("stoi", "estoi", "stoi_mix", "estoi_mix")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(name, utts=None):
    c = sc.build(name)
    u = slice(None) if utts is None else utts
    out = crit.stoi(_dev(c["src"][:, u]), _dev(c["est"][:, u]), mixture=_dev(c["mix"][u]), lengths=c["lengths"][u], fs=c["fs"])
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged_8k", "three_8k", "long_10k", "one_16k"])
def test_stoi_matches_restatement(name):
    want = sc.expected(name)
    assert (want["kept"] < want["frames"]).all() and (want["margin"] >= 0.01).all() and not want["short"].any()
    out = _run(name)
    S, B = sc.build(name)["S"], len(sc.build(name)["lengths"])
    assert out["stoi"].shape == out["estoi"].shape == (B, S, S) and out["stoi"].dtype == torch.float64
    assert out["stoi_mix"].shape == out["estoi_mix"].shape == out["kept"].shape == out["status"].shape == (B, S)
    assert np.array_equal(out["kept"].cpu().numpy(), want["kept"]), (out["kept"], want["kept"])
    assert int(out["status"].abs().sum()) == 0
    for k in KEYS:
        err = float(np.abs(out[k].cpu().numpy() - want[k]).max())
        print(f"{name} {k}: max |device - restatement| = {err:.3e} (TOL {TOL:.3e})")
    for k in KEYS:
        assert np.abs(out[k].cpu().numpy() - want[k]).max() <= TOL, k


@pytest.mark.gpu
def test_stoi_without_mixture_and_bitwise_repeatable_and_batch_independent():
    c = sc.build("ragged_8k")
    a, b = _run("ragged_8k"), _run("ragged_8k")
    for k in a:
        assert torch.equal(a[k], b[k]), k                                       # bit-identical run to run
    for u in range(3):
        one = _run("ragged_8k", slice(u, u + 1))                                # T = 8000 as in the batch, its own length
        for k in a:
            assert torch.equal(one[k][0], a[k][u]), (u, k)
    n = c["lengths"][0]                                                         # and at its own padded length
    one = crit.stoi(_dev(c["src"][:, :1, :n]), _dev(c["est"][:, :1, :n]), mixture=_dev(c["mix"][:1, :n]), fs=8000)
    for k in a:
        assert torch.equal(one[k][0], a[k][0]), k
    nomix = crit.stoi(_dev(c["src"]), _dev(c["est"]), lengths=c["lengths"], fs=8000)
    assert set(nomix) == {"stoi", "estoi", "kept", "status"}
    assert torch.equal(nomix["stoi"], a["stoi"]) and torch.equal(nomix["estoi"], a["estoi"])


@pytest.mark.gpu
def test_too_short_and_silent_utterances_beside_neighbours():
    c = sc.build("ragged_8k")
    want = sc.expected("ragged_8k")
    src, est, mix = c["src"].copy(), c["est"].copy(), c["mix"].copy()
    full = _run("ragged_8k")
    out = crit.stoi(_dev(src), _dev(est), mixture=_dev(mix), lengths=[4000, 2000, 8000], fs=8000)     # 2500 samples at 10 kHz: 18 frames
    st = out["status"].cpu().numpy()
    assert st.tolist() == [[0, 0], [1, 1], [0, 0]]
    for k in KEYS:
        v = out[k].cpu().numpy()
        assert (v[1] == 1e-5).all(), (k, v[1])
        assert np.array_equal(v[[0, 2]], full[k].cpu().numpy()[[0, 2]]), k      # the neighbours are not disturbed
    short = ref.evaluate(src[0, 1, :2000], [est[0, 1, :2000]], 8000)
    assert short["short"] and out["kept"].cpu().numpy()[1, 0] == short["kept"]
    # an all-zero reference: every frame has the same energy, all are kept, every band value is 0 and so is every correlation
    src[1, 2] = 0.0
    out = crit.stoi(_dev(src), _dev(est), mixture=_dev(mix), lengths=c["lengths"], fs=8000)
    z = ref.evaluate(src[1, 2, :8000], [est[0, 2, :8000], est[1, 2, :8000], mix[2, :8000]], 8000)
    assert not z["short"] and z["kept"] == z["frames"] == 77
    assert out["status"].cpu().numpy().tolist() == [[0, 0], [0, 0], [0, 0]] and out["kept"].cpu().numpy()[2, 1] == 77
    for k in KEYS:
        v = out[k].cpu().numpy()
        assert np.isfinite(v).all(), k
    assert np.abs(out["stoi"].cpu().numpy()[2, 1] - z["stoi"][:2]).max() <= TOL and np.abs(out["estoi"].cpu().numpy()[2, 1] - z["estoi"][:2]).max() <= TOL
    assert abs(out["stoi_mix"].cpu().numpy()[2, 1] - z["stoi"][2]) <= TOL
    assert np.abs(out["stoi"].cpu().numpy()[2, 0] - want["stoi"][2, 0]).max() <= TOL   # the other reference of that utterance


@pytest.mark.gpu
@pytest.mark.parametrize("name,extended", [("ragged_8k", False), ("ragged_8k", True), ("three_8k", False), ("three_8k", True)])
def test_pit_stoi_matches_restatement(name, extended):
    c, want = sc.build(name), sc.expected(name)
    key = "estoi" if extended else "stoi"
    S, B = c["S"], len(c["lengths"])
    pit = crit.PIT_STOI(DEV, extended=extended, fs=c["fs"])
    tot, per = pit(estims=[_dev(c["est"][s]) for s in range(S)], mixture=torch.from_numpy(c["mix"]),
                   input_sizes=torch.tensor(c["lengths"]), target_attr=[torch.from_numpy(c["src"][s]) for s in range(S)])
    per = np.asarray(per).reshape(B, S)
    total = 0.0
    for b in range(B):
        perm, chosen, imp = ref.pit(want[key][b], want[key + "_mix"][b])
        assert list(pit.perm[b]) == perm, (b, pit.perm[b], perm)
        assert np.abs(pit.values[b] - chosen).max() <= TOL and np.abs(per[b] - imp).max() <= 2 * TOL
        total += imp.sum()
    assert abs(float(tot) - total / B) <= 2 * TOL * S
    assert any(list(p) != list(range(S)) for p in pit.perm)                     # the estimates are built swapped: not the identity


@pytest.mark.gpu
def test_evaluate_utterances_all_rows_and_unchanged_loop(tmp_path):
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.model import Model
    model = Model.from_config(VARIANTS["tiny"], init_seed=0).load_synthetic_(0).eval().to(DEV)
    c = sc.build("ragged_8k")
    utts = []
    for b, n in enumerate((4000, 6000, 5000)):
        s = [torch.from_numpy(c["src"][i, b:b + 1, :n].copy()) for i in range(2)]
        utts.append((s[0] + s[1], s, f"utt{b}.wav"))
    res = infer.evaluate_utterances_all(model, utts, sisnr_csv_path=str(tmp_path / "si.csv"), sdr_csv_path=str(tmp_path / "sdr.csv"),
                                        stoi_csv_path=str(tmp_path / "stoi.csv"), estoi_csv_path=str(tmp_path / "estoi.csv"))
    assert set(res) == {"sisnri", "sdri", "stoi", "estoi", "stoi_i", "estoi_i", "n"} and res["n"] == 3
    m_si, m_sdr, n = infer.evaluate_utterances(model, utts, sisnr_csv_path=str(tmp_path / "si2.csv"), sdr_csv_path=str(tmp_path / "sdr2.csv"))
    assert (res["sisnri"], res["sdri"], res["n"]) == (m_si, m_sdr, n)           # bitwise: the same loop
    for name in ("si", "sdr"):
        assert open(tmp_path / f"{name}.csv").read() == open(tmp_path / f"{name}2.csv").read()
    means = {k: 0.0 for k in ("stoi", "estoi", "stoi_i", "estoi_i")}
    rows = {k: open(tmp_path / f"{k}.csv").read().strip().split("\n") for k in ("stoi", "estoi")}
    for u, (mix, src, key) in enumerate(utts):
        est = torch.stack([e[0] for e in infer.separate(model, mix)])[:, None]
        out = crit.stoi(torch.cat(src)[:, None].to(DEV), est, mixture=mix.to(DEV), fs=8000)
        for k in ("stoi", "estoi"):
            _, val, imp = crit.stoi_pit(out[k].cpu().numpy(), out[k + "_mix"].cpu().numpy())
            row = rows[k][u].split(",")
            assert row[0] == f"utt{u}" and len(row) == 3 and [float(v) for v in row[1:]] == [float(v) for v in val[0]], (k, row, val)
            means[k] += val[0].sum() / 2 / 3
            means[k + "_i"] += imp[0].sum() / 2 / 3
    for k, v in means.items():
        assert abs(res[k] - v) <= 1e-12, (k, res[k], v)
