"""Every exported size entry returns, value by value, what it returned before the workspace layouts were stated once: the rows of
tests/golden/workspace_sizes.json were recorded from the parent commit's library (tests/golden/make_workspace_sizes.py).  The internal
``*_ws`` functions are covered through ``sepr_train_ws_bytes``, which sums them.  No device is needed: a size entry launches nothing."""
import json
import os

import pytest

from sepreformer_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")) as _f:
    GOLDEN = json.load(_f)

ENTRIES = ["sepr_workspace_bytes", "sepr_train_ctx_bytes", "sepr_train_ws_bytes", "sepr_linear_wgrad_workspace", "sepr_pit_sisnr_mag_workspace",
           "sepr_pit_sisnr_mag_bwd_workspace", "sepr_bss_eval_workspace", "sepr_stoi_workspace", "sepr_stitch_workspace",
           "sepr_resample_workspace", "sepr_corpus_energy_workspace", "sepr_adamw_workspace"]


def test_golden_covers_every_size_entry():
    """Every symbol of the binding that returns a size_t is in the recording, with accepted and refused (0) shapes."""
    sized = sorted(k for k, (res, _) in L.SIGNATURES.items() if res is L._sz)
    assert sized == sorted(ENTRIES) == sorted(GOLDEN)
    for name in ENTRIES:
        if name != "sepr_adamw_workspace":      # (no argument, nothing to refuse)
            assert any(r[-1] == 0 for r in GOLDEN[name]) and any(r[-1] > 0 for r in GOLDEN[name]), name


@pytest.mark.parametrize("name", ENTRIES)
def test_sizes_equal_the_recorded_ones(name):
    assert not os.environ.get("SEPR_LIB_VARIANT"), "this test judges the product library"
    fn = getattr(L.load(), name)
    rows = GOLDEN[name]
    assert rows
    wrong = [(r[:-1], r[-1], int(fn(*r[:-1]))) for r in rows if int(fn(*r[:-1])) != r[-1]]
    assert not wrong, f"{name}: {len(wrong)} of {len(rows)} differ, first (args, recorded, now): {wrong[:5]}"
