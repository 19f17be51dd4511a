"""The device's training criteria judged forward and backward against float64 autograd on hard inputs and shape edges (cases, reference,
floors, rules: tests/criterion_ref.py; the proof that these bars reject planted defects: tests/test_criterion_hard_cpu.py).

Every case runs the forward through ``pit_sisnr`` / ``pit_sisnr_mag`` and the backward through ``_PitTimeFn`` / ``_PitMagFn`` with the upstream
gradient ``w = linspace(0.5, 2, B)``.  Every gradient row ``d est[s, b]`` must be finite and either agree with float64 to
``bar = min(80 dB, floor_db - 6 dB, floor_dev_db - 6 dB)`` or, where the float64 row is exactly 0, be exactly 0; the permutation must be
float64's; the losses are within the tolerances of tests/test_criterion.py.  Both floors come from the host (float32 autograd, the
restatement of the kernels' arithmetic); nothing here is set from what the device returns.  No case is skipped or exempted.

Every figure goes through record() of tests/test_gpu_parity.py into its parity_report.json as ``criterion_hard.<kind>.<case>.dest<s>.b<b>`` with
``.bar_db`` beside it, and ``criterion_hard.<kind>.S<S>.least_spare_db`` per test.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criterion_ref as cr                                                   # noqa: E402
import test_gpu_parity as tgp                                               # noqa: E402

pytestmark = pytest.mark.gpu


def run_case(case, kind, crit_mag):
    """-> (forward loss [B], forward permutation [B, S], the Function's loss [B], d (loss . w) / d est [S, B, T]) from the device."""
    from sepreformer_amd.criterion import _PitMagFn, _PitTimeFn, pit_sisnr, pit_sisnr_mag
    dev = torch.device("cuda:0")
    est, src = case.tensors()
    e, t, w = est.to(dev).requires_grad_(True), src.to(dev), case.weights().to(dev)
    if kind == "time":
        out = pit_sisnr(e.detach(), t, eps_loss=cr.EPS["time"], clamp_min=cr.CLAMP_MIN)
        loss, perm = out["loss"], out["loss_perm"]
        per = _PitTimeFn.apply(e, t, cr.EPS["time"], cr.CLAMP_MIN)
    else:
        out = pit_sisnr_mag(e.detach(), t, crit_mag._dft, cr.FRAME_LEN, cr.FRAME_HOP, cr.EPS["mag"])
        loss, perm = out["loss"], out["perm"]
        per = _PitMagFn.apply(e, t, crit_mag._dft, crit_mag._dft_t, cr.FRAME_LEN, cr.FRAME_HOP, cr.EPS["mag"])
    (per * w).sum().backward()
    torch.cuda.synchronize()
    return loss.cpu(), perm.cpu(), per.detach().cpu(), e.grad.cpu()


def call_surface(case, kind, crit, bad):
    """``PIT_SISNR_time`` / ``PIT_SISNR_mag`` as the training loop calls them, evaluation and training path: the mean over the batch."""
    dev = torch.device("cuda:0")
    est, src = case.tensors()
    r = cr.floors(case, kind)
    want, tol = float(r["loss64"].mean()), float(r["loss_tol"].max())
    sizes = torch.full((case.B,), case.T)
    kw = {"idx": 0} if kind == "mag" else {}
    tg = [t.to(dev) for t in src]
    for grad in (False, True):
        es = [e.to(dev).requires_grad_(grad) for e in est]
        out = crit(estims=es, input_sizes=sizes, target_attr=tg, **kw)
        got = float(out.detach())
        name = f"criterion_hard.{kind}.{case.tag}.mean" + (".train" if grad else ".eval")
        tgp.REPORT[name + "_err_db"] = float(f"{abs(got - want):.3e}")
        if out.requires_grad != grad or not abs(got - want) <= tol:
            bad.append(f"{name}: {got:.6f} vs {want:.6f} (tolerance {tol:.1e} dB), requires_grad {out.requires_grad}")


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("kind", cr.KINDS)
def test_criterion_hard(kind, S):
    from sepreformer_amd.criterion import PIT_SISNR_mag, PIT_SISNR_time
    dev = torch.device("cuda:0")
    crit_mag = PIT_SISNR_mag(dev, cr.FRAME_LEN, cr.FRAME_HOP, "hann", 1, S, True, False)
    bad, worst = [], None
    cases = cr.cases_for(S)
    assert cases
    for case in cases:
        loss, perm, per, grad = run_case(case, kind, crit_mag)
        if not torch.equal(loss, per):
            bad.append(f"{kind}.{case.tag}: the autograd Function's loss differs from the forward entry's")
        b, least = cr.judge(case, kind, loss, perm, grad, report=tgp.REPORT, prefix="criterion_hard.")
        bad += b
        if least is not None and (worst is None or least[0] < worst[0]):
            worst = least
    call_surface(cases[0], kind, crit_mag if kind == "mag" else PIT_SISNR_time(dev, S, True), bad)
    if worst is not None:
        print(f"closest to its bar: {worst[1]} {worst[2]:.1f} dB (bar {worst[3]:.1f})")
        tgp.REPORT[f"criterion_hard.{kind}.S{S}.least_spare_db"] = round(worst[0], 2)
    tgp.record(f"criterion_hard.{kind}.S{S}.failures", len(bad))            # one write of everything gathered above
    assert not bad, f"{len(bad)} failed: " + "; ".join(bad[:60])
