"""The weight EMA's host-only half, without a device: the two new entries in the header and the binding, the
decay schedule against its restatement, the checkpoint's optional seventh key, and loading the averaged weights for inference."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_ref as er                                                         # noqa: E402

from sepreformer_amd import lib as L                                         # noqa: E402
from sepreformer_amd import trainer as T                                     # noqa: E402
from sepreformer_amd.config import VARIANTS                                  # noqa: E402
from sepreformer_amd.infer import load_checkpoint_weights                    # noqa: E402
from sepreformer_amd.model import Model                                      # noqa: E402
from sepreformer_amd.optim import FlatAdamW                                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(hdr, name):
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, name
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def test_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "sepr.h")).read()
    lib = L.load()
    for name in ("sepr_adamw_step_ema", "sepr_adamw_swap"):
        ret, _ = _declaration(hdr, name)
        assert ret == "int", (name, ret)
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is L._i, name
        assert hasattr(lib, name)
    _, guarded = _declaration(hdr, "sepr_adamw_step_guarded")
    _, ema = _declaration(hdr, "sepr_adamw_step_ema")
    assert len(ema) == len(guarded) + 3
    extra = [a for a in ema if a not in guarded]
    assert extra == ["float* ema", "double ema_decay", "double ema_warmup"] and ema.index("float* ema") + 3 == ema.index("float* scal")
    sg, se = L.SIGNATURES["sepr_adamw_step_guarded"][1], L.SIGNATURES["sepr_adamw_step_ema"][1]
    assert len(se) == len(sg) + 3 == len(ema)
    assert se[:12] == sg[:12] and se[12:15] == [L._fp, L._d, L._d] and se[15:] == sg[12:]
    assert len(L.SIGNATURES["sepr_adamw_swap"][1]) == 3 == len(_declaration(hdr, "sepr_adamw_swap")[1])
    assert int(re.search(r"#define SEPR_VERSION (\d+)", hdr).group(1)) == 413 == L.ABI_VERSION == lib.sepr_version()
    # argument validation happens before any launch
    assert lib.sepr_adamw_swap(None, None, None) == L.SEPR_EINVAL
    assert lib.sepr_adamw_step_ema(None, None, 0, None, None, None, None, 0.9, 0.999, 1e-8, 0.0, 0.0, None, 0.9, 10.0, None, None, 0, None) == L.SEPR_EINVAL


def test_decay_schedule():
    for decay, warmup in ((0.9, 10.0), (0.999, 10.0), (0.9999, 100.0), (0.9, 0.0), (0.0, 10.0)):
        for t in (1, 2, 10, 10 ** 6):
            assert T.ema_decay_at(t, decay, warmup) == er.decay_at(t, decay, warmup), (t, decay, warmup)
    assert T.ema_decay_at(1, 0.9, 10.0) == 2.0 / 11.0
    assert T.ema_decay_at(1, 0.9, 0.0) == 0.9 and T.ema_decay_at(7, 0.9, -1.0) == 0.9
    assert T.ema_decay_at(10 ** 6, 0.999, 10.0) == 0.999
    # the ramp rises towards the decay and never passes it
    ramp = [T.ema_decay_at(t, 0.999, 10.0) for t in range(1, 20001)]
    assert all(a <= b for a, b in zip(ramp, ramp[1:])) and ramp[-1] == 0.999 and ramp[0] < 0.2
    assert T.ema_decay_at(3, 0.9, 10.0) == T.ema_decay_at(3, 0.9)           # the default warm-up is 10


def _tiny_state(seed):
    return Model.from_config(VARIANTS["tiny"], init_seed=seed).state_dict()


def test_checkpoint_extra_key_and_ema_loading(tmp_path):
    raw, avg = _tiny_state(1), _tiny_state(2)
    osd = {"state": {}, "param_groups": []}
    seven = T.write_checkpoint(str(tmp_path / "seven"), 1, raw, osd, 1.5, 2.5, {"global_step": 3}, extra={"ema_state_dict": avg})
    six = T.write_checkpoint(str(tmp_path / "six"), 1, raw, osd, 1.5, 2.5, {"global_step": 3})
    ck7, ck6 = T.read_checkpoint(seven), T.read_checkpoint(six)
    assert set(ck6) == set(T.CHECKPOINT_KEYS) | {T.RUN_STATE_KEY} and len(ck6) == 6
    assert set(ck7) == set(ck6) | {"ema_state_dict"} and len(ck7) == 7
    assert ck7["epoch"] == 1 and ck7["valid_loss"] == 2.5 and ck7[T.RUN_STATE_KEY] == {"global_step": 3}
    with pytest.raises(ValueError):
        T.write_checkpoint(str(tmp_path / "bad"), 1, raw, osd, 1.5, 2.5, {}, extra={"epoch": 2})

    model = Model.from_config(VARIANTS["tiny"], init_seed=3)
    res = load_checkpoint_weights(model, seven, ema=True)
    assert not res.missing_keys and not res.unexpected_keys
    differ = 0
    for k, v in model.state_dict().items():
        assert er.same(v, avg[k]) if v.dtype == torch.float32 else torch.equal(v, avg[k]), k
        differ += int(v.dtype == torch.float32 and not er.same(v, raw[k]))
    assert differ > 0                                                        # the two sets really differ: ema=True did not load the raw weights
    load_checkpoint_weights(model, seven)                                    # the default stays the raw weights
    for k, v in model.state_dict().items():
        assert er.same(v, raw[k]) if v.dtype == torch.float32 else torch.equal(v, raw[k]), k
    with pytest.raises(ValueError, match=re.escape(six)):
        load_checkpoint_weights(model, six, ema=True)
    load_checkpoint_weights(model, six)                                      # ... and loads without ema


def test_ema_needs_the_guarded_step():
    """Refused before a parameter or a device is looked at."""
    with pytest.raises(ValueError, match="skip_nonfinite"):
        FlatAdamW(None, ema_decay=0.9, skip_nonfinite=False)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        FlatAdamW(None, ema_decay=0.9)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        FlatAdamW(None, ema_decay=1.0, skip_nonfinite=True)


def test_trainer_refuses_an_unknown_validate_with():
    class Feed:
        fixed_length = True
    with pytest.raises(ValueError, match="validate_with"):
        T.Trainer(None, Feed(), Feed(), "x", ema_decay=0.9, validate_with="averaged")
