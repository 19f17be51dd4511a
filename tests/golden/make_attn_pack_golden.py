"""tests/golden/attn_pack_off_tiny.npz: what ``sepr_ega_fwd`` (tiny, bf16x3, n 2, T' 65, randn family) gave BEFORE the packed-K attention
kernel existed - the reference of tests/test_attention_pack_gpu.py::test_attention_pack_off_is_the_old_kernel.

It was written on an MI355X by a library built from the parent commit's csrc (a second library beside the product one, tools/README.md):

    SEPR_LIB_VARIANT=parent python tests/golden/make_attn_pack_golden.py [out.npz]

Run with the product library and SEPR_ATTN_PACK=0 it must reproduce the file bit for bit (``--check``).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import branch_ref as br                                                      # noqa: E402
from sepreformer_amd.config import VARIANTS                                 # noqa: E402
from sepreformer_amd.model import Model                                     # noqa: E402


def main(argv):
    check = "--check" in argv
    args = [a for a in argv if a != "--check"]
    out = args[0] if args else os.path.join(HERE, "attn_pack_off_tiny.npz")
    case = br.Case("ega", br.ROW_FAMILIES, n=2, fac=1, Tp=65)
    m = Model.from_config(VARIANTS["tiny"], init_seed=0, precision="bf16x3").load_synthetic_(0).eval().to("cuda")
    eng = m.engine()
    eng.prepare(8, 2400, 2400)
    x = br.make_inputs(case, m.cfg, "randn")["x"]
    y = eng.ega(x.cuda(), eng.pk.enc_stages[0]["g"][0][0], 2, 65, 65)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert np.isfinite(y).all()
    if check:
        g = np.load(out)
        same = np.array_equal(g["x"], x.numpy()) and np.array_equal(g["y"], y)
        print("attn_pack_off_tiny:", "reproduced bit for bit" if same else "DIFFERS")
        return 0 if same else 1
    np.savez(out, x=x.numpy(), y=y)
    print("wrote", out, y.shape)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
