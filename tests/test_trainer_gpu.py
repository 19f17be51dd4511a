"""The epoch loop on the device (sepreformer_amd/trainer.py): the run ledger against float64 sums on the host, the
guarded optimizer step, the validation pass against a hand loop, a run cut between epochs and continued bit for bit, checkpoint
interchange with ``torch.optim.AdamW`` and the reference's five-key layout, and the tool.  The ``tiny`` variant on the four-key corpus of
tests/golden/dynmix.npz, batch 2, 2000 samples."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_ref as dr                                                      # noqa: E402
import trainer_ref as tr                                                     # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import trainer as T                                     # noqa: E402
from sepreformer_amd.config import VARIANTS                                  # noqa: E402
from sepreformer_amd.model import Model                                      # noqa: E402
from sepreformer_amd.optim import FlatAdamW                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, MAXLEN, LR, WARMUP = 2, 2000, 1.0e-3, 3


def corpus_and_keys(golden):
    g = golden("dynmix")
    arrays, roles = dr.fixture_corpus(g)
    c = df.Corpus.from_arrays(arrays, device=DEV, fs=8000)
    c.roles = roles
    return c, [str(k) for k in g["keys"]], arrays


def tiny(dropout=0.0):
    cfg = VARIANTS["tiny"] if dropout is None else dataclasses.replace(VARIANTS["tiny"], dropout=dropout)
    return Model.from_config(cfg, init_seed=0).load_synthetic_(0).to(DEV)


def feeds(corpus, train_keys=None, valid_keys=None):
    train = df.DynamicMixFeed(corpus, df.plan_wsj0, batch=B, max_len=MAXLEN, seed=3, fixed_length=True, keys=train_keys)
    valid = df.DynamicMixFeed(corpus, df.plan_direct, batch=B, max_len=MAXLEN, seed=4, keys=valid_keys, drop_last=False)
    return train, valid


def make_trainer(corpus, directory, dropout=0.0, train_keys=None, valid_keys=None, **kw):
    train, valid = feeds(corpus, train_keys, valid_keys)
    kw.setdefault("max_epoch", 3)
    kw.setdefault("log", lambda s: None)
    return T.Trainer(tiny(dropout), train, valid, str(directory), lr=LR, seed=11, warmup_steps=WARMUP, **kw)


def test_ledger_equals_float64_sums_on_the_host(golden, tmp_path):
    """One training epoch of four batches through Trainer (one eager warm-up step, three replays) against the same four steps made
    with the public pieces, read back with float() per step and summed in float64 in the same order: every slot is equal, since
    float64 sums of the same fp32 values in the same order have nothing to differ by."""
    corpus, keys, _ = corpus_and_keys(golden)
    lines = []
    t = make_trainer(corpus, tmp_path, train_keys=keys * 2, log_every=2, log=lines.append)
    got_means = t.train_epoch(1)
    got = t.read_ledger()
    assert t.global_step == 4 and got_means[2] == 4
    # one line per log interval, from a snapshot of the ledger taken after that batch (the copy is asynchronous: the line may come a step late)
    assert [ln.split(":")[0] for ln in lines] == ["epoch 1 batch 2 (global step 2)", "epoch 1 batch 4 (global step 4)"], lines
    assert f"T_Loss {got_means[0]:.4f}  F_Loss {got_means[1]:.4f}" in lines[1] and f"clipped {int(got.clipped)}" in lines[1]

    # the same steps, eagerly, one host read per value
    model = tiny().train()
    feed, _ = feeds(corpus, keys * 2)
    opt = FlatAdamW(model, lr=LR, weight_decay=1.0e-2, skip_nonfinite=True)
    w_time = torch.full((), 1.0 - T.alpha(1), dtype=torch.float32, device=DEV)
    w_freq = torch.full((), T.alpha(1), dtype=torch.float32, device=DEV)
    sizes = torch.full((B,), MAXLEN)
    x, tg = torch.zeros(B, MAXLEN, device=DEV), [torch.zeros(B, MAXLEN, device=DEV) for _ in range(2)]
    host, per_batch = tr.HostLedger(t.nparts), []
    for i in range(1, 5):
        opt.param_groups[0]["lr"] = tr.lambda_lr_rates(LR, WARMUP, i)[-1]
        feed.next_into(x, tg)
        opt.zero_grad(set_to_none=True)
        audio, aux = model(x)
        l_time = t.crit_t(estims=audio, input_sizes=sizes, target_attr=tg).reshape(())
        l_mag = [t.crit_m(estims=a, idx=k, input_sizes=sizes, target_attr=tg).reshape(()) for k, a in enumerate(aux)]
        loss = T.mix_loss(l_time, l_mag, w_time, w_freq, 2)
        loss.backward()
        gn = opt.step(max_norm=5.0)
        parts = [float(l_time)] + [float(m) for m in l_mag]
        per_batch.append(parts)
        host.update(parts, float(gn), float(opt.clip_coef), skipped=float(opt.skipped) != 0.0)
    print("ledger", got.values, "host", host.values())
    assert got.values == host.values()
    assert got.steps == 4 and got.skipped == 0 and got.nonfinite == 0 and got.gnorm_max > 0
    want_means = tr.ref_epoch_means(per_batch, 2)
    assert got_means == want_means, (got_means, want_means)
    assert float(t.step.loss) == float(loss)
    for (k, a), (_, b) in zip(t.model.state_dict().items(), model.state_dict().items()):
        assert tr.same_bits(a, b), k

    # the step's total loss is the one expression, evaluated outside the graph from the parts and the two weight scalars
    def outside():
        return T.mix_loss(t.parts[0], [t.parts[1 + k] for k in range(t.nparts - 1)], t.w_time, t.w_freq, 2)
    assert tr.same_bits(t.step.loss.reshape(()), outside().reshape(()))
    # a new alpha between two replays: two fill_s, the same graphs
    g_main, g_opt = t.step.g_main, t.step.g_opt
    old = (t.w_time.clone(), t.w_freq.clone())
    t.set_alpha(T.alpha(106))
    t.step(t.step.x, t.step.targets)
    assert t.step.g_main is g_main and t.step.g_opt is g_opt
    assert float(t.w_freq) == float(torch.tensor(T.alpha(106), dtype=torch.float32)) and float(t.w_time) == float(torch.tensor(1.0 - T.alpha(106), dtype=torch.float32))
    assert tr.same_bits(t.step.loss.reshape(()), outside().reshape(()))
    stale = T.mix_loss(t.parts[0], [t.parts[1 + k] for k in range(t.nparts - 1)], old[0], old[1], 2)
    assert float(stale) != float(t.step.loss)
    assert t.read_ledger().steps == 5
    assert t.model.__dict__.get("dropout_seed_fn") is not None
    t.release()
    assert "dropout_seed_fn" not in t.model.__dict__ and t.step is None      # nothing of the Trainer stays behind on the model


def _batch(seed=5):
    from sepreformer_amd.synth import synth_mixture
    s1, s2 = synth_mixture(B, MAXLEN, seed=seed).to(DEV), synth_mixture(B, MAXLEN, seed=seed + 1).to(DEV)
    return (s1 + s2).contiguous(), [s1.contiguous(), s2.contiguous()]


class _Eager:
    """An eager step of tiny on one fixed batch, the optimizer's step apart."""

    def __init__(self, skip_nonfinite, with_ledger=False):
        from sepreformer_amd.criterion import PIT_SISNR_time
        self.model = tiny().train()
        self.opt = FlatAdamW(self.model, lr=LR, weight_decay=1.0e-2, skip_nonfinite=skip_nonfinite)
        self.crit = PIT_SISNR_time(torch.device(DEV), 2, True)
        self.x, self.tg = _batch()
        self.sizes = torch.full((B,), MAXLEN)
        self.parts = torch.zeros(3, dtype=torch.float32, device=DEV)
        self.ledger = torch.zeros(L.ledger_doubles(3), dtype=torch.float64, device=DEV)
        if with_ledger:
            self.opt.attach_ledger(self.ledger, self.parts)

    def backward(self):
        self.opt.zero_grad(set_to_none=True)
        audio, _ = self.model(self.x)
        loss = self.crit(estims=audio, input_sizes=self.sizes, target_attr=self.tg) / 2
        loss.backward()
        with torch.no_grad():
            self.parts.fill_(float(loss))

    def snapshot(self):
        return ([p.detach().clone() for p in self.model.parameters()], self.opt._exp_avg.clone(), self.opt._exp_avg_sq.clone(), self.opt._step.clone())

    def poison(self, value):
        """One element of the flat gradient buffer overwritten between backward and step: arithmetic, not a fault."""
        g = next(iter(self.model.parameters())).grad
        flat = self.model.__dict__["_grad_flat"]
        assert flat.data_ptr() <= g.data_ptr() < flat.data_ptr() + 4 * flat.numel()
        g.view(-1)[0] = value


def _same(a, b):
    return all(tr.same_bits(p, q) for p, q in zip(a[0], b[0])) and all(tr.same_bits(p, q) for p, q in zip(a[1:], b[1:]))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_guard_skips_a_nonfinite_step(bad):
    run = _Eager(True, with_ledger=True)
    run.backward()
    run.opt.step(max_norm=5.0)
    before = run.snapshot()
    run.backward()
    run.poison(bad)
    run.opt.step(max_norm=5.0)
    assert float(run.opt._scal[5]) == 1.0 and float(run.opt.skipped) == 1.0
    assert _same(before, run.snapshot())                                     # parameters, both moments, the step counter
    led = T.Ledger(run.ledger.cpu().tolist(), 3)
    assert led.skipped == 1 and led.steps == 1 and float(run.opt._step) == 1.0
    run.backward()
    run.opt.step(max_norm=5.0)
    assert float(run.opt._scal[5]) == 0.0
    led = T.Ledger(run.ledger.cpu().tolist(), 3)
    assert led.skipped == 1 and led.steps == 2
    # a run that never saw the bad gradient
    clean = _Eager(True)
    for _ in range(2):
        clean.backward()
        clean.opt.step(max_norm=5.0)
    assert _same(clean.snapshot(), run.snapshot())


def test_unguarded_step_still_poisons():
    """skip_nonfinite=False is today's behaviour: the NaN coefficient reaches every parameter."""
    run = _Eager(False)
    run.backward()
    run.opt.step(max_norm=5.0)
    run.backward()
    run.poison(float("nan"))
    run.opt.step(max_norm=5.0)
    assert float(run.opt._step) == 2.0 and float(run.opt._scal[5]) == 0.0
    assert all(bool(torch.isnan(p).all()) for p in run.model.parameters())


@pytest.mark.parametrize("max_norm", [5.0, 0.05, None])
def test_guarded_equals_unguarded_on_finite_gradients(max_norm):
    a, b = _Eager(True), _Eager(False)
    for _ in range(3):
        for run in (a, b):
            run.backward()
            run.opt.step(max_norm=max_norm)
    assert float(a.opt._step) == 3.0 and _same(a.snapshot(), b.snapshot())
    if max_norm:
        assert float(a.opt._scal[0]) == float(b.opt._scal[0]) and float(a.opt.clip_coef) == float(b.opt.clip_coef)
        print("grad norm", float(a.opt._scal[0]), "clip", float(a.opt.clip_coef))


@pytest.mark.parametrize("nkeys", [3, 4])
def test_validate_equals_a_hand_loop(golden, tmp_path, nkeys):
    """3 keys at batch 2: one full batch and a trailing batch of ONE utterance, which weighs as much as the full one."""
    corpus, keys, _ = corpus_and_keys(golden)
    t = make_trainer(corpus, tmp_path, valid_keys=keys[:nkeys])
    before = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    got = t.validate()
    for k, v in t.model.state_dict().items():
        assert tr.same_bits(before[k], v), k
    _, feed = feeds(corpus, valid_keys=keys[:nkeys])
    model = t.model.eval()
    per_batch, sizes_seen = [], []
    with torch.inference_mode():
        for sizes, mix, src, _ in feed:
            audio, aux = model(mix)
            per_batch.append([float(t.crit_t(estims=audio, input_sizes=sizes, target_attr=src))] +
                             [float(t.crit_m(estims=a, idx=k, input_sizes=sizes, target_attr=src)) for k, a in enumerate(aux)])
            sizes_seen.append(mix.shape[0])
    assert sizes_seen == ([2, 1] if nkeys == 3 else [2, 2])
    want = tr.ref_epoch_means(per_batch, 2)
    print("validate", got, "hand loop", want)
    assert got == want
    led = t.read_ledger(valid=True)
    assert led.steps == 2 and led.gnorm_sum == 0 and led.skipped == 0 and led.last == per_batch[-1]


def test_feed_refuses_drop_last_false_with_fixed_length(golden):
    corpus, keys, _ = corpus_and_keys(golden)
    with pytest.raises(ValueError, match="drop_last"):
        df.DynamicMixFeed(corpus, df.plan_wsj0, batch=B, max_len=MAXLEN, fixed_length=True, drop_last=False)
    feed = df.DynamicMixFeed(corpus, df.plan_direct, batch=B, max_len=MAXLEN, keys=keys[:3], drop_last=False)
    assert [m.shape[0] for _, m, _, _ in feed] == [2, 1]


def test_validation_after_a_one_batch_epoch_sees_the_new_weights(golden, tmp_path):
    """An epoch of ONE batch is the eager warm-up step of the capture and no replay: the validation that follows must not answer from the
    weights packed by a validation before it."""
    corpus, keys, _ = corpus_and_keys(golden)
    t = make_trainer(corpus, tmp_path, train_keys=keys[:2], valid_keys=keys[:2])
    state = t.valid_feed.state_dict()
    before = t.validate()                                                    # packs the initial weights
    assert t.train_epoch(1)[2] == 1 and t.global_step == 1 and t.step.calls == 0
    t.valid_feed.load_state_dict(state)
    after = t.validate()
    t.model.invalidate_packed()
    t.valid_feed.load_state_dict(state)
    repacked = t.validate()
    print("before", before, "after", after, "repacked", repacked)
    assert after == repacked and after != before
    t.release()


def _final(t):
    return ({k: v.detach().clone() for k, v in t.model.state_dict().items()}, t.opt._exp_avg.clone(), t.opt._exp_avg_sq.clone(), t.opt._step.clone(),
            t.opt.param_groups[0]["lr"], t.last_train, t.last_valid, t.global_step)


@pytest.mark.parametrize("dropout", [0.0, None])
def test_resume_continues_bit_for_bit(golden, tmp_path, dropout):
    """A: two epochs straight.  B: one epoch, save, every object dropped, new model / optimizer / feeds / Trainer from the directory,
    one more epoch.  Fails on any stateful dropout stream and on any batch the restart consumes but does not count."""
    corpus, keys, _ = corpus_and_keys(golden)
    a = make_trainer(corpus, tmp_path / "a", dropout, max_epoch=3)
    a.run()
    fa = _final(a)
    b = make_trainer(corpus, tmp_path / "b", dropout, max_epoch=2)
    b.run()
    assert sorted(os.listdir(tmp_path / "b")) == ["epoch.0001.pth"] and b.global_step == 2
    del b
    b = make_trainer(corpus, tmp_path / "b", dropout, max_epoch=3)
    b.run()
    fb = _final(b)
    assert b.start_epoch == 2 and sorted(os.listdir(tmp_path / "b")) == ["epoch.0001.pth", "epoch.0002.pth"]
    assert fa[7] == fb[7] == 4                                               # the global step: the restart's first batch is counted
    assert fa[4] == fb[4] == T.warmup_lr(LR, 2, WARMUP)                                 # epoch 1 was shorter than the warm-up; epoch 2 left the rate alone
    print("train", fa[5], fb[5], "valid", fa[6], fb[6])
    assert fa[5] == fb[5] and fa[6] == fb[6]
    for k in fa[0]:
        assert tr.same_bits(fa[0][k], fb[0][k]), k
    assert tr.same_bits(fa[1], fb[1]) and tr.same_bits(fa[2], fb[2]) and tr.same_bits(fa[3], fb[3])
    if dropout is None:                                                      # the masks really were on: another run seed, another trajectory
        assert VARIANTS["tiny"].dropout > 0


def test_checkpoint_interchange(golden, tmp_path):
    corpus, keys, _ = corpus_and_keys(golden)
    t = make_trainer(corpus, tmp_path / "ours")
    tr_t, _, _ = t.train_epoch(1)
    va_t, _, _ = t.validate()
    path = t.save(1, tr_t, va_t)
    t.release()
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == set(T.CHECKPOINT_KEYS) | {T.RUN_STATE_KEY}
    assert set(ck[T.RUN_STATE_KEY]) == {"global_step", "plateau", "train_feed", "valid_feed", "best", "seed"}
    # ours -> torch.optim.AdamW
    m = tiny()
    m.load_state_dict(ck["model_state_dict"], strict=True)
    o = torch.optim.AdamW(m.parameters(), capturable=True)
    o.load_state_dict(ck["optimizer_state_dict"])
    for p, q in zip(m.parameters(), t.model.parameters()):
        assert tr.same_bits(o.state[p]["exp_avg"], t.opt.state[q]["exp_avg"]) and tr.same_bits(o.state[p]["exp_avg_sq"], t.opt.state[q]["exp_avg_sq"])
        assert float(o.state[p]["step"]) == float(t.opt._step) == 2.0
    # the reference's five-key layout, written from a torch AdamW -> Trainer
    os.makedirs(tmp_path / "theirs")
    torch.save({"epoch": 7, "model_state_dict": m.state_dict(), "optimizer_state_dict": o.state_dict(), "train_loss": 0.0, "valid_loss": 0.0},
               str(tmp_path / "theirs" / "epoch.0007.pth"))
    u = make_trainer(corpus, tmp_path / "theirs")
    assert u.load_latest() == 8 and u.start_epoch == 8 and u.global_step == 2
    assert tr.same_bits(u.opt._exp_avg, t.opt._exp_avg) and tr.same_bits(u.opt._exp_avg_sq, t.opt._exp_avg_sq) and float(u.opt._step) == 2.0
    for (k, a), (_, b) in zip(u.model.state_dict().items(), t.model.state_dict().items()):
        assert tr.same_bits(a, b), k
    # infer.py's checkpoint loading reads our file
    from sepreformer_amd.infer import load_checkpoint_weights
    fresh = Model.from_config(VARIANTS["tiny"], init_seed=1)
    res = load_checkpoint_weights(fresh, path)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, a), (_, b) in zip(fresh.state_dict().items(), t.model.state_dict().items()):
        assert tr.same_bits(a, b.cpu()), k


def test_tool_runs_epochs_and_resumes(golden, tmp_path):
    """tools/train_from_scp.py --epochs on scp lists written from the fixture corpus."""
    _, keys, arrays = corpus_and_keys(golden)
    scp = {}
    for role in ("s1", "s2", "mix"):
        lines = []
        for k in keys:
            wav = str(tmp_path / f"{role}_{k}.wav")
            tr.write_wav16(wav, arrays[f"{role}/{k}"])
            lines.append(f"{k} {wav}")
        scp[role] = str(tmp_path / f"{role}.scp")
        with open(scp[role], "w") as f:
            f.write("\n".join(lines) + "\n")
    ck = str(tmp_path / "ck")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_from_scp.py"), "--form", "wsj0", "--scp", f"s1={scp['s1']}", f"s2={scp['s2']}",
           "--model", "tiny", "--precision", "bf16x3", "--batch", "2", "--max-len", "2000", "--valid-scp", f"mix={scp['mix']}", f"s1={scp['s1']}",
           f"s2={scp['s2']}", "--checkpoint-dir", ck, "--warmup-steps", "3", "--test-scp", f"mix={scp['mix']}", f"s1={scp['s1']}", f"s2={scp['s2']}",
           "--test-epochs", "1"]
    first = subprocess.run(cmd + ["--epochs", "2"], capture_output=True, text=True, timeout=300)
    assert first.returncode == 0, first.stdout + first.stderr
    assert os.listdir(ck) == ["epoch.0001.pth"] and "[VALID] Epoch  1" in first.stdout
    assert "[TEST] Epoch  1: SISNRi = " in first.stdout and f"/{len(keys)})" in first.stdout.split("[TEST]")[1]      # the test loop ran over every file
    second = subprocess.run(cmd + ["--epochs", "3", "--resume"], capture_output=True, text=True, timeout=300)
    assert second.returncode == 0, second.stdout + second.stderr
    assert "[TEST]" not in second.stdout                                     # epoch 2 is not a test epoch
    assert "resuming at epoch 2" in second.stdout and "[TRAIN] Epoch  2" in second.stdout and "[TRAIN] Epoch  1" not in second.stdout
    assert sorted(os.listdir(ck)) == ["epoch.0001.pth", "epoch.0002.pth"]
