"""The inference packer produces, byte for byte, what it produced before its weight forms were stated once: the CPU section of
tests/golden/pack_digests.json was recorded from the parent commit's ``pack.py`` (tests/golden/make_pack_digests.py) - one digest per block
struct over dtype, shape and bytes of every tensor it points at, null fields included, for F = 64 (S = 2 and 3), 128 and 256 in both
precisions and with each switch ``pack.py`` reads set to its non-default value.

And the promise of ``pack_gcfn_fused_batched``'s docstring: per block it is ``pack_gcfn_fused``."""
import importlib.util
import json
import os

import pytest
import torch

from sepreformer_amd import pack
from sepreformer_amd.config import VARIANTS
from sepreformer_amd.synth import synth_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_pack_digests", os.path.join(ROOT, "tests", "golden", "make_pack_digests.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(rec.PATH) as _f:
    GOLDEN = json.load(_f)


def row_id(r):
    return "-".join([r["variant"], r["precision"]] + [f"{k}={v}" for k, v in r["env"].items()])


def check_section(section: str, device: str, row):
    """``row`` of ``section`` against this tree's packer; a switch row is the plain row with its ``differs`` entries replaced."""
    want = row.get("digests")
    if want is None:
        plain = next(r for r in GOLDEN[section] if (r["variant"], r["precision"]) == (row["variant"], row["precision"]) and not r["env"])
        assert row["differs"] and set(row["differs"]) <= set(plain["digests"])
        want = {**plain["digests"], **row["differs"]}
    got = rec.digests_of(pack, row["variant"], row["precision"], device, row["env"])
    assert sorted(got) == sorted(want)
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, f"{row_id(row)}: {len(wrong)} of {len(want)} structs differ from the recording, first: {wrong[:8]}"


def test_recording_covers_every_switch_and_width():
    with open(pack.__file__) as f:
        named = rec.switches_named_in(f.read())
    rows = GOLDEN["cpu"]
    assert len(named) == 13 and named == sorted(rec.SWITCHES) == sorted(k for r in rows for k in r["env"])
    for r in rows:
        for k, v in r["env"].items():
            assert (v, r["variant"]) == rec.SWITCHES[k] and r["precision"] == "bf16x3"
    assert sorted((r["variant"], r["precision"]) for r in rows if not r["env"]) == sorted(rec.ROWS["cpu"])
    assert sorted({(VARIANTS[v].feat, VARIANTS[v].num_spks) for v, _ in rec.ROWS["cpu"]}) == [(64, 2), (64, 3), (128, 2), (256, 2)]


@pytest.mark.parametrize("row", GOLDEN["cpu"], ids=row_id)
def test_packed_model_equals_the_recorded_bytes(row):
    check_section("cpu", "cpu", row)


@pytest.mark.parametrize("variant", ["tiny", "tiny3", rec.BASE, rec.LARGE])
def test_batched_gcfn_pack_is_the_single_pack_per_block(variant):
    """All GCFN blocks of a model (F = 64, 128, 256; G = 30 .. 56) through ``pack_gcfn_fused_batched`` in one call: block for block the
    bytes of ``pack_gcfn_fused`` called on that block alone."""
    sd = synth_state_dict(VARIANTS[variant], rec.SEED)
    blocks = sorted(k[:-len(".net1.1.weight")] for k in sd if k.endswith(".net1.1.weight"))
    names = (".net1.1.weight", ".net1.1.bias", ".net1.0.weight", ".net1.0.bias", ".net2.2.weight", ".depthwise.weight", ".depthwise.bias")
    G, F = len(blocks), sd[blocks[0] + ".net1.0.weight"].shape[0]
    assert G > 1 and F == {"tiny": 64, "tiny3": 64, rec.BASE: 128, rec.LARGE: 256}[variant]
    args = [torch.stack([sd[b + n] for b in blocks], 0) for n in names]
    w1p, w2p = pack.pack_gcfn_fused_batched(*args)
    assert w1p.dtype == torch.uint8 and w1p.shape == (G, (3 * F // 32) * (4 * (F // 32) * 2048 + 4096))
    assert w2p.dtype == torch.bfloat16 and w2p.shape == (G, 3 * F // 32, F // 16, 2, 64, 8)
    for i, b in enumerate(blocks):
        s1, s2 = pack.pack_gcfn_fused(*[sd[b + n] for n in names])
        assert s1.dtype == torch.uint8 and s1.shape == (3 * F // 32, w1p.shape[1] // (3 * F // 32))
        assert torch.equal(w1p[i], s1.reshape(-1)) and torch.equal(w2p[i].view(torch.int16), s2.view(torch.int16)), b
    args[5] = args[5].reshape(G, 6 * F, 3)                                  # the [G,6F,3] form of the taps the device test hands in
    w1q, w2q = pack.pack_gcfn_fused_batched(*args)
    assert torch.equal(w1q, w1p) and torch.equal(w2q.view(torch.int16), w2p.view(torch.int16))
