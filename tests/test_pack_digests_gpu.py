"""tests/test_pack_digests_cpu.py on the device: the state dict is moved to the MI355X before packing, as ``Model`` does, and every block
struct of ``PackedModel`` must give the digest the parent commit's ``pack.py`` gave there (the device section of
tests/golden/pack_digests.json).  The fp64 folds reduce on the device, so this is where a differently ordered sum would show.  Plain torch
ops only: no kernel of the library runs."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pack_digests_cpu import GOLDEN, check_section, rec, row_id      # noqa: E402


def test_device_section_rows():
    assert [(r["variant"], r["precision"], r["env"]) for r in GOLDEN["device"]] == [(v, p, {}) for v, p in rec.ROWS["device"]]


@pytest.mark.gpu
@pytest.mark.parametrize("row", GOLDEN["device"], ids=row_id)
def test_packed_model_on_the_device_equals_the_recorded_bytes(row):
    check_section("device", "cuda:0", row)
