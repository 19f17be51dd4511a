"""Device blocks judged on the part they compute, in float64, on hard inputs (measure, bar, families, case list: tests/branch_ref.py;
the proof that this bar rejects planted defects: tests/test_branch_parity_cpu.py).

Every case goes through the engine call tests/test_gpu_parity.py::test_blocks uses for it (the training forwards as
tests/test_train_gpu.py drives them), every output must be finite and agree with the float64 oracle on the branch to
``bar = min(80 dB, floor_db - 6 dB)`` (bf16x3: also ``floor_x3_db - 6 dB``), both floors computed on the host from the oracle for that very
input.  Every figure goes through record() of tests/test_gpu_parity.py into its parity_report.json as ``branch.<variant>.<precision>.<kind>.<shape>.<family>`` with
``....floor_db`` (and ``....floor_x3_db``) beside it.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import branch_ref as br                                                      # noqa: E402
import test_gpu_parity as tgp                                               # noqa: E402
from sepreformer_amd import lib as L                                        # noqa: E402
from sepreformer_amd.config import VARIANTS                                 # noqa: E402

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp32", "bf16x3"]


class Judge:
    """Measures every (case, family) of one test and fails at the end with all of them, so one device run shows the whole picture."""

    def __init__(self, variant, precision):
        self.variant, self.precision, self.bad, self.worst = variant, precision, [], {}

    def check(self, case, family, got, ref=None, suffix=""):
        r = ref or br.floors(case, self.variant, family, want_x3=(self.precision == "bf16x3"))
        name = f"branch.{self.variant}.{self.precision}.{case.tag}.{family}{suffix}"
        got = got.detach().float().cpu()
        x3 = r["floor_x3_db"] if self.precision == "bf16x3" else None
        need = br.bar(r["floor_db"], x3)
        tgp.REPORT[name + ".floor_db"] = round(r["floor_db"], 2)
        if x3 is not None:
            tgp.REPORT[name + ".floor_x3_db"] = round(x3, 2)
        if got.shape != r["y64"].shape:
            self.bad.append(f"{name}: shape {tuple(got.shape)} != {tuple(r['y64'].shape)}")
            return None
        if not torch.isfinite(got).all():
            tgp.REPORT[name] = -999.0
            self.bad.append(f"{name}: non-finite output")
            return None
        x32 = None if r["x64"] is None else r["x64"].float()          # the residual input as the device received it
        db = br.branch_db(got, x32, r["y64"], r["x64"])
        tgp.REPORT[name] = round(db, 2)
        key = case.kind
        if key not in self.worst or db - need < self.worst[key][0]:
            self.worst[key] = (db - need, name, db, need)
        if not db >= need:
            self.bad.append(f"{name}: {db:.1f} dB < bar {need:.1f} (floor {r['floor_db']:.1f}" + (f", x3 floor {x3:.1f})" if x3 is not None else ")"))
        return db

    def done(self):
        for kind, (_, name, db, need) in sorted(self.worst.items()):
            print(f"closest to its bar: {name} {db:.1f} dB (bar {need:.1f})")
            tgp.REPORT[f"branch.{self.variant}.{self.precision}.{kind}.least_spare_db"] = round(db - need, 2)
        tgp.record(f"branch.{self.variant}.{self.precision}.failures", len(self.bad))      # one write of everything gathered above
        assert not self.bad, f"{len(self.bad)} below the bar: " + "; ".join(self.bad[:60])


def _encode(eng, cfg, wav_d):
    """The encoder launch of test_blocks: [B, L, N] channel-last frames and the GroupNorm statistics."""
    B, T = wav_d.shape
    L_ = cfg.frames(T)
    enc = torch.empty(B, L_, cfg.enc_channels, device="cuda")
    gn = torch.empty(B, 2, device="cuda")
    L.check(eng.lib.sepr_encoder_fwd(wav_d.data_ptr(), B, T, eng.pk.enc_w, cfg.enc_channels, cfg.enc_kernel, cfg.enc_stride, 1e-8,
                                     enc.data_ptr(), gn.data_ptr(), *eng._wsargs, eng._st), "enc")
    return enc, gn, L_


def run_block(m, eng, case, inp):
    """One case on the device through the engine call of test_blocks."""
    cfg, pk = m.cfg, eng.pk
    S, F = cfg.num_spks, cfg.feat
    k, s = case.kind, case.shape
    d = {n_: t.cuda() for n_, t in inp.items()}
    if k == "gcfn":
        return eng.gcfn(d["x"], pk.enc_stages[0]["g"][0][1], s["n"], s["T"])
    if k == "cla":
        return eng.cla(d["x"], pk.enc_stages[0]["l"][0][0], s["n"], s["T"])
    if k == "ega":
        return eng.ega(d["x"], pk.enc_stages[0]["g"][0][0], s["n"], s["Tp"] * s["fac"], s["Tp"])
    if k == "spkattn":
        return eng.spkattn(d["x"], pk.dec_stages[0]["spk"][0][0], s["B"] * S, s["T"])
    if k == "down":
        return eng.downconv(d["x"], pk.enc_stages[0]["down"], s["n"], s["T"])[0]
    if k == "split":
        return eng.spksplit(d["x"], pk.splits[0], s["B"], s["T"])
    if k == "fuse":
        return eng.fuse(d["lo"], d["sk"], pk.fuse[0], s["B"] * S, s["T"])
    enc, gn, L_ = _encode(eng, cfg, d["wav"])
    B = s["B"]
    if k == "encoder":
        return enc
    if k == "projector":
        Lp = cfg.padded_frames(L_)
        pj = torch.empty(B, Lp, F, device="cuda")
        L.check(eng.lib.sepr_projector_fwd(enc.data_ptr(), B, L_, Lp, cfg.enc_channels, F, gn.data_ptr(), pk.proj_g, pk.proj_b, pk.proj_w,
                                           pj.data_ptr(), eng._st), "proj")
        return pj
    if k == "head_main":
        Lp = cfg.padded_frames(L_)
        return eng.head(d["z"], pk.out_main, B * S, Lp, L_, None, None, B)
    if k == "head_aux":
        return eng.head(d["z"], pk.out_aux[1], B * S, s["Ts"], L_, eng._idx(s["Ts"], L_), enc, B)
    raise KeyError(k)


def _blocks(variant, precision, cases):
    m, _ = tgp.gpu_model(variant, precision)
    eng = m.engine()
    eng.prepare(8, 2400, 2400)
    judge = Judge(variant, precision)
    for case in cases:
        for fam in case.families:
            inp = br.make_inputs(case, m.cfg, fam)
            y = run_block(m, eng, case, inp)
            torch.cuda.synchronize()
            judge.check(case, fam, y)
    judge.done()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", br.GPU_VARIANTS)
def test_branch_blocks(variant, precision):
    """The edge shapes of test_blocks x every input family."""
    _blocks(variant, precision, br.cases_for(variant, br.BLOCK_CASES))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_branch_ega_crosses_maxlen(precision):
    """Base width, T' = 2100 (pool 1) and 2050 (pool 2) > maxlen = 2000: randn and the three families with the lowest floors."""
    assert VARIANTS[br.BASE].maxlen == 2000
    _blocks(br.BASE, precision, br.cases_for(br.BASE, br.MAXLEN_CASES))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", br.GPU_VARIANTS)
def test_branch_train_forward(variant, precision):
    """The training forward of the four residual blocks (sepr_*_train_fwd: another kernel instantiation than inference), driven as
    test_gcfn_train / test_cla_train / test_ega_train / test_spkattn_train drive it (dropout 0), one shape per block."""
    import test_train_gpu as ttg
    cfg, sd, sdd, gb, tp, eng = ttg.setup(variant, precision)
    judge = Judge(variant, precision)
    bn = br.E0 + ".l_block_1.block.cla.BN."
    for case in br.cases_for(variant, br.TRAIN_CASES):
        s = case.shape
        for fam in case.families:
            x = br.make_inputs(case, cfg, fam)["x"].cuda()
            if case.kind == "gcfn_train":
                y, _ = eng.block_fwd("gcfn", x, tp.gcfn[0], s["n"], s["T"])
            elif case.kind == "cla_train":
                keep = {k_: sdd[bn + k_].clone() for k_ in ("running_mean", "running_var")}      # shared device state: put back below
                y, _ = eng.block_fwd("cla", x, tp.cla[0], s["n"], s["T"])
                torch.cuda.synchronize()
                for k_, v in keep.items():
                    sdd[bn + k_].copy_(v)
            elif case.kind == "ega_train":
                y, _ = eng.block_fwd("ega", x, tp.ega[0], s["n"], s["Tp"] * s["fac"], s["Tp"])
            else:
                y, _ = eng.block_fwd("spk", x, tp.spk[0], s["B"] * cfg.num_spks, s["T"])
            torch.cuda.synchronize()
            judge.check(case, fam, y)
    judge.done()


def _stack(audio, aux, B, n):
    rows = [torch.stack([a.reshape(B, -1)[:, :n] for a in audio], 0)]
    rows += [torch.stack([a.reshape(B, -1)[:, :n] for a in st], 0) for st in aux]
    return torch.stack(rows, 0)                                       # [1 + R, S, B, n], as branch_ref.reference("e2e") stacks them


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", ["tiny", br.BASE])
def test_branch_end_to_end(variant, precision):
    """Model.forward on the waveform families (tiny; Base at 0.5 s) against the float64 oracle's model_forward, main and auxiliary
    outputs.  With one all-silent utterance in the batch: everything finite, the silent row judged on its own against float64, and the
    other rows bit-identical to the same batch with a normal utterance in that slot."""
    m, _ = tgp.gpu_model(variant, precision)
    judge = Judge(variant, precision)
    (case,) = br.cases_for(variant, br.E2E_CASES)
    B = case.shape["B"]
    outs = {}
    for fam in case.families:
        r = br.floors(case, variant, fam, want_x3=(precision == "bf16x3"))
        audio, aux = m(r["inp"]["wav"].cuda())
        torch.cuda.synchronize()
        outs[fam] = _stack([a.cpu() for a in audio], [[a.cpu() for a in st] for st in aux], B, r["y64"].shape[-1])
        judge.check(case, fam, outs[fam], r)
    # rows must not leak: the silent slot (utterance 1) changes nothing in utterance 0
    quiet_row, other = min(1, B - 1), 0
    assert torch.isfinite(outs["silent_utt"]).all()
    assert torch.equal(outs["silent_utt"][:, :, other], outs["speech"][:, :, other]), "a silent utterance changed another row of its batch"
    # the silent row alone (main head: what the biases make of silence; auxiliary heads: masked by a zero encoding, exactly 0)
    r = br.floors(case, variant, "silent_utt", want_x3=(precision == "bf16x3"))
    y64 = r["y64"][:, :, quiet_row]
    y32, _ = br.reference(case, variant, br.state(variant), r["inp"])
    row = {"y64": y64, "x64": None, "floor_db": br.branch_db(y32[:, :, quiet_row], None, y64, None), "floor_x3_db": None}
    if precision == "bf16x3":
        row["floor_x3_db"] = br.branch_db(br.reference_x3(case, variant, r["inp"])[0][:, :, quiet_row], None, y64, None)
    judge.check(case, "silent_utt", outs["silent_utt"][:, :, quiet_row], row, suffix=".silent_row")
    judge.done()
