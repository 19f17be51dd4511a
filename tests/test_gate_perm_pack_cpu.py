"""The row-permuted gate pack of the fused global block (``pack.py::pack_gate_fused_perm``) is ``pack_gate_fused`` with its rows moved:
un-permuting it gives that pack's tiles and biases exactly."""
import torch

from sepreformer_amd.pack import gate_perm_rows, pack_gate_fused, pack_gate_fused_perm


def rows_of(pack, F):
    """[F rows][K/32][plane][k group][8] bf16 bit patterns and [F] biases of a gate pack ([F/64 chunks][4 tiles | 4 KB constants] bytes)."""
    KS = F // 32
    nfrag = 4 * KS * 2 * 64 * 8 * 2
    w, b = [], []
    for c in range(F // 64):
        chunk = pack[c]
        t = chunk[:nfrag].view(torch.int16).reshape(4, KS, 2, 4, 16, 8)       # [tile][K step][plane][k group][row][8]
        w.append(t.permute(0, 4, 1, 2, 3, 5).reshape(64, KS, 2, 4, 8))
        cst = chunk[nfrag:].view(torch.float32)
        assert cst.numel() == 1024 and not cst[64:].any()
        b.append(cst[:64])
    return torch.cat(w, 0), torch.cat(b, 0)


def test_gate_perm_rows_is_a_permutation_in_fragment_order():
    rows = gate_perm_rows(128)
    assert sorted(rows.tolist()) == list(range(128))
    # lane group q of K step ks holds channels 32*ks + 8*q .. +7: rows 4q .. 4q+3 of tile 2*ks, then of tile 2*ks + 1
    for ks in range(4):
        for q in range(4):
            got = [int(rows[16 * (2 * ks + h) + 4 * q + r]) for h in range(2) for r in range(4)]
            assert got == list(range(32 * ks + 8 * q, 32 * ks + 8 * q + 8))


def test_unpermuting_gives_pack_gate_fused_exactly():
    F = 128
    g = torch.Generator().manual_seed(3)
    w = torch.randn(F, F, generator=g) * 0.2
    b = torch.randn(F, generator=g)
    gamma = 1.0 + 0.3 * torch.randn(F, generator=g)
    beta = 0.2 * torch.randn(F, generator=g)
    nat, perm = pack_gate_fused(w, b, gamma, beta), pack_gate_fused_perm(w, b, gamma, beta)
    assert nat.shape == perm.shape and nat.dtype == perm.dtype
    wn, bn = rows_of(nat, F)
    wp, bp = rows_of(perm, F)
    rows = gate_perm_rows(F)
    inv = torch.empty_like(rows)
    inv[rows] = torch.arange(F)
    assert torch.equal(wp[inv], wn) and torch.equal(bp[inv].view(torch.int32), bn.view(torch.int32))
    assert not torch.equal(wp, wn)
