"""The epoch loop's host-only half (sepreformer_amd/trainer.py), without a device: the loss mix and the two
schedules against the reference's expressions, the checkpoint directory logic, the feeds' state, and the ledger's slot table."""
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dynmix_ref as dr                                                      # noqa: E402
import trainer_ref as tr                                                     # noqa: E402

from sepreformer_amd import datafeed as df                                   # noqa: E402
from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import trainer as T                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_alpha_is_the_reference_expression():
    for epoch in range(1, 201):
        assert T.alpha(epoch) == tr.ref_alpha(epoch), epoch
    assert T.alpha(100) == 0.4 and T.alpha(1) == 0.4
    assert all(T.alpha(e) == 0.4 * 0.8 for e in range(101, 106))
    assert T.alpha(106) == 0.4 * 0.8 ** 2
    assert abs(T.alpha(105) - 0.32) < 1e-15 and abs(T.alpha(106) - 0.256) < 1e-15


@pytest.mark.parametrize("warmup_steps", [1, 3, 1000])
def test_warmup_matches_lambda_lr(warmup_steps):
    """Epoch 1 of 7 batches: shorter than a warm-up of 1000, longer than one of 1 or 3.  Epoch 2 leaves the rate where epoch 1 left it."""
    base, batches = 1.0e-3, 7
    want = tr.lambda_lr_rates(base, warmup_steps, batches)
    lr, got = base, []
    for i in range(1, batches + 1):
        lr = T.batch_lr(lr, base, 1, i, warmup_steps)
        got.append(lr)
    assert got == want, (got, want)
    assert got == [T.warmup_lr(base, i, warmup_steps) for i in range(1, batches + 1)]
    assert got[-1] == (base if warmup_steps <= batches else base * batches / warmup_steps)
    for i in range(1, batches + 1):
        assert T.batch_lr(lr, base, 2, i, warmup_steps) == lr


def test_plateau_only_after_start_scheduling():
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1.0)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.8, patience=2, min_lr=1.0e-10)
    stepped = [T.plateau_step(sched, epoch, 3, 1.0) for epoch in range(1, 8)]          # a loss that never improves
    assert stepped == [False, False, False, True, True, True, True]
    # epochs 4 (sets the best), 5, 6 (two bad epochs: patience), 7 (the third): one reduction
    assert opt.param_groups[0]["lr"] == 0.8
    twin = torch.optim.SGD([p], lr=1.0)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(twin, mode="min", factor=0.8, patience=2, min_lr=1.0e-10)
    for _ in range(4):
        ref.step(1.0)
    assert twin.param_groups[0]["lr"] == opt.param_groups[0]["lr"]


def _write(directory, epoch, valid=0.0, keep_last=None, run_state=None):
    return T.write_checkpoint(str(directory), epoch, {"w": torch.zeros(2)}, {"state": {}, "param_groups": []}, 1.5, valid,
                              run_state if run_state is not None else {"global_step": 3 * epoch}, keep_last)


def test_checkpoint_directory_logic(tmp_path):
    d = tmp_path / "ck"
    assert T.latest_checkpoint(str(d)) is None                               # a directory that does not exist yet
    d.mkdir()
    assert T.latest_checkpoint(str(d)) is None and T.list_checkpoints(str(d)) == []       # empty -> start_epoch 1
    _write(d, 3)
    _write(d, 10)
    assert sorted(os.listdir(d)) == ["epoch.0003.pth", "epoch.0010.pth"]     # nothing else lies in the directory
    assert all(int(f.split(".")[1]) in (3, 10) for f in os.listdir(d))       # util_engine.py:37 parses every name
    latest = T.latest_checkpoint(str(d))
    assert os.path.basename(latest) == "epoch.0010.pth"
    ck = T.read_checkpoint(latest)
    assert ck["epoch"] + 1 == 11
    assert set(ck) == set(T.CHECKPOINT_KEYS) | {T.RUN_STATE_KEY} and len(ck) == 6
    assert T.CHECKPOINT_KEYS == ("epoch", "model_state_dict", "optimizer_state_dict", "train_loss", "valid_loss")
    assert ck["train_loss"] == 1.5 and ck[T.RUN_STATE_KEY] == {"global_step": 30}
    # keep_last prunes the older files
    for e in (11, 12, 13):
        _write(d, e, keep_last=2)
    assert sorted(os.listdir(d)) == ["epoch.0012.pth", "epoch.0013.pth"]
    assert T.prune_checkpoints(str(d), None) == [] and T.prune_checkpoints(str(d), 5) == []


def test_save_policy():
    assert T.should_save("all", 5.0, 1.0) and T.should_save("all", 0.5, 1.0)
    assert T.should_save("best", 0.5, 1.0) and not T.should_save("best", 1.0, 1.0) and not T.should_save("best", 2.0, 1.0)
    assert T.should_save("best", -3.0, float("inf"))
    with pytest.raises(ValueError):
        T.should_save("nth", 0.0, 0.0)


def _host_corpus(golden):
    g = golden("dynmix")
    arrays, roles = dr.fixture_corpus(g)
    c = df.Corpus.from_arrays(arrays, device=None, fs=8000)
    c.roles = roles
    c.set_energies(np.array([dr.energy(arrays[nm]) for nm in c.names], dtype=np.int64), np.zeros(0))
    return c, [str(k) for k in g["keys"]]


def test_feed_state_round_trip(golden, tmp_path):
    """state_dict -> a file -> a fresh object -> load_state_dict: the same next epoch order and the same planner draws."""
    corpus, keys = _host_corpus(golden)
    a = df.FeedOrder(keys, batch=2, seed=5)
    for _ in range(2):                                                       # two epochs of orders and draws
        a.epoch += 1
        for k in a.epoch_order():
            df.plan_wsj0(corpus, a.rng, k, 2000)
    path = str(tmp_path / "state.pth")
    torch.save({"feed": a.state_dict()}, path)
    b = df.FeedOrder(keys, batch=2, seed=99)
    b.load_state_dict(torch.load(path, map_location="cpu")["feed"])
    assert b.epoch == a.epoch == 2
    order_a, order_b = a.epoch_order(), b.epoch_order()
    assert order_a == order_b and sorted(order_a) == sorted(keys)
    for k in order_a:
        assert df.plan_wsj0(corpus, a.rng, k, 2000) == df.plan_wsj0(corpus, b.rng, k, 2000)
        assert df.plan_direct(corpus, a.rng, k, 2000) == df.plan_direct(corpus, b.rng, k, 2000)
    fresh = df.FeedOrder(keys, batch=2, seed=5)
    assert fresh.epoch == 0 and fresh.rng.getstate() == random.Random(5).getstate()


def test_drop_last_batch_boundaries():
    for n, want_keep, want_drop in ((3, [2, 1], [2]), (4, [2, 2], [2, 2]), (1, [1], [])):
        keys = [f"k{i}" for i in range(n)]
        keep = df.FeedOrder(keys, batch=2, keys=keys, drop_last=False)
        drop = df.FeedOrder(keys, batch=2, keys=keys)
        assert [len(b) for b in keep.batches(keep.epoch_order())] == want_keep
        assert [len(b) for b in drop.batches(drop.epoch_order())] == want_drop
        assert sum(keep.batches(keys), []) == keys
    assert df.FeedOrder(["a"], batch=2).drop_last is True


def test_drop_last_false_is_refused_with_fixed_length(golden):
    """Static tensors have one shape: the host-only half of the feed refuses the combination with a ValueError, and DynamicMixFeed hands its two
    flags to it.  The device check of DynamicMixFeed stays where it was: a host-only corpus is refused first, whatever else is asked."""
    keys = ["a", "b", "c"]
    with pytest.raises(ValueError, match="drop_last"):
        df.FeedOrder(keys, batch=2, drop_last=False, fixed_length=True)
    assert df.FeedOrder(keys, batch=2, drop_last=True, fixed_length=True).drop_last is True
    assert df.FeedOrder(keys, batch=2, drop_last=False, fixed_length=False).drop_last is False
    corpus, _ = _host_corpus(golden)
    with pytest.raises(RuntimeError, match="HIP device"):
        df.DynamicMixFeed(corpus, df.plan_direct, batch=2, max_len=2000, drop_last=False)


def test_ledger_slots_and_abi():
    hdr = open(os.path.join(ROOT, "include", "sepr.h")).read()
    enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"SEPR_LEDGER_([A-Z_]+) = (\d+)", hdr)}
    assert enum.pop("max_parts") == L.LEDGER_MAX_PARTS
    assert enum == L.LEDGER_SLOTS
    lib = L.load()
    for nparts in (1, 3, 5, L.LEDGER_MAX_PARTS):
        assert lib.sepr_run_ledger_doubles(nparts) == L.ledger_doubles(nparts) == 6 + 2 * nparts
    assert lib.sepr_run_ledger_doubles(0) == 0 and lib.sepr_run_ledger_doubles(L.LEDGER_MAX_PARTS + 1) == 0
    for name in ("sepr_adamw_step_guarded", "sepr_run_ledger_update", "sepr_run_ledger_doubles"):
        assert name in L.SIGNATURES and re.search(r"\b" + name + r"\s*\(", hdr), name
        assert L.SIGNATURES[name][0] is not L._sz                            # neither new entry returns size_t
    assert L.SIGNATURES["sepr_adamw_step_guarded"] == L.SIGNATURES["sepr_adamw_step"]
    assert int(re.search(r"#define SEPR_VERSION (\d+)", hdr).group(1)) == 413 == L.ABI_VERSION == lib.sepr_version()
    # argument validation happens before any launch
    assert lib.sepr_run_ledger_update(None, 3, None, None, 12, None) == L.SEPR_EINVAL
    led = Tled = T.Ledger(list(range(6 + 2 * 3)), 3)
    assert (led.steps, led.skipped, led.nonfinite, led.gnorm_sum, led.gnorm_max, led.clipped) == (0, 1, 2, 3, 4, 5)
    assert Tled.part_sum == [6, 7, 8] and Tled.last == [9, 10, 11]


def test_epoch_means_follow_the_reference():
    per_batch = [[-3.25, 1.5, 2.5], [-1.75, 0.5, 4.0], [2.0, -1.0, 0.25]]
    host = tr.HostLedger(3)
    for p in per_batch:
        host.update(p)
    got = T.epoch_means(host.part_sum, host.steps, 2)
    want = tr.ref_epoch_means(per_batch, 2)
    assert got == want[:2] and want[2] == 3


def test_dropout_words_are_stateless():
    assert T.seed_word(7) == T.seed_word(7) != T.seed_word(8)
    words = {T.salt_word(7, i) for i in range(1, 1001)}
    assert len(words) == 1000 and all(0 <= w < 2 ** 63 for w in words)
    assert T.salt_word(7, 5) != T.salt_word(8, 5)


def test_trainer_refuses_mvn_and_variable_length():
    class Feed:
        fixed_length = False
    with pytest.raises(ValueError, match="mvn"):
        T.Trainer(None, Feed(), Feed(), "x", mvn=True)
    with pytest.raises(ValueError, match="fixed_length"):
        T.Trainer(None, Feed(), Feed(), "x")
