"""The merged auxiliary-head decoder (``sepr_outlayer_basis_fwd`` per head + ONE ``sepr_aux_decoder_fwd``) against
the per-head ``sepr_outlayer_decoder_fwd`` path on the same synthetic weights.  Every accumulator of the merged kernel sees the operand
sequence of ``decoder_kernel`` and the overlap-add is the same, so every comparison is ``torch.equal``: no tolerance anywhere.

Head-level cases drive the two forms with random stage outputs and a random encoder output at the smallest shapes where the kernel can go
wrong (partial last tile, L < one tile, S = 3, B = 1, source lengths that are no power-of-two fraction of L); whole-forward cases flip the
engine's ``SEPR_AUX_MERGE`` switch (read once per engine, like ``SEPR_OVERLAP``) with one, two pipelines and under graph replay."""
import ctypes as C

import pytest
import torch

from sepreformer_amd import lib as L
from sepreformer_amd.config import VARIANTS
from sepreformer_amd.engine import SeparatorEngine
from sepreformer_amd.model import Model
from sepreformer_amd.synth import synth_mixture

BASE = "SepReformer_Base_WSJ0"
_models = {}


def gpu_model(variant):
    if variant not in _models:
        _models[variant] = Model.from_config(VARIANTS[variant], init_seed=0, precision="bf16x3").load_synthetic_(0).eval().to("cuda")
    return _models[variant]


def fresh_engine(m, monkeypatch, merge):
    """The model's engine re-created under SEPR_AUX_MERGE = merge, None = unset (the packed weights are cached, only the driver object is new)."""
    if merge is None:
        monkeypatch.delenv("SEPR_AUX_MERGE", raising=False)
    else:
        monkeypatch.setenv("SEPR_AUX_MERGE", merge)
    m._engine = None
    eng = m.engine()
    assert eng.aux_merge == (merge != "0") and eng._aux_merge_auto == (merge is None)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("variant,B,T,L_want,src_want", [
    ("tiny", 2, 1000, 247, [62, 124]),                    # 5 tiles with a partial last one; L differs from the padded length
    ("tiny3", 2, 1000, 247, [62, 124]),                   # the speaker loop and the [S, B, T] layout
    (BASE, 2, 2000, 497, [32, 64, 128, 256]),             # N = 256, four heads
    (BASE, 2, 200, 47, [3, 6, 12, 24]),                   # less than one tile, all-halo first tile, the float nearest_index map
    (BASE, 1, 2000, 497, [32, 64, 128, 256]),             # first and last utterance are the same one
])
def test_merged_heads_equal_per_head_decoders(variant, B, T, L_want, src_want):
    m = gpu_model(variant)
    eng, c = m.engine(), m.cfg
    L_ = c.frames(T)
    Lp = c.padded_frames(L_)
    R, S, nS = c.num_stages, c.num_spks, B * c.num_spks
    srcs = [(Lp >> R) << i for i in range(R)]
    assert L_ == L_want and srcs == src_want and eng._aux_merge_ok(L_, Lp)
    eng.prepare(B, L_, Lp)
    g = torch.Generator(device="cuda").manual_seed(11)
    enc = torch.randn(B, L_, c.enc_channels, device="cuda", generator=g)
    xs = [torch.randn(nS, t, c.feat, device="cuda", generator=g) for t in srcs]
    want = [eng.head(xs[i], eng.pk.out_aux[i], nS, srcs[i], L_, eng._idx(srcs[i], L_), enc, B) for i in range(R)]
    o2s = [eng.head_basis(xs[i], eng.pk.out_aux[i], nS, srcs[i], L_) for i in range(R)]
    got = eng.aux_decode(o2s, srcs, L_, enc, B)
    torch.cuda.synchronize()
    assert len(got) == R
    for i in range(R):
        assert got[i].shape == want[i].shape == (S, B, (L_ - 1) * c.enc_stride + c.enc_kernel)
        assert float(want[i].abs().max()) > 0.0
        assert torch.equal(got[i], want[i]), f"aux_{i}"


def count_merged_launches(monkeypatch):
    """Counts ``aux_decode`` calls of every engine (pipeline peers included): a list that grows by one per merged launch enqueued."""
    calls, plain = [], SeparatorEngine.aux_decode

    def counted(self, *a, **k):
        calls.append(self)
        return plain(self, *a, **k)

    monkeypatch.setattr(SeparatorEngine, "aux_decode", counted)
    return calls


def _whole_forward(m, monkeypatch, x, merge, calls, want_calls):
    """One Model forward under SEPR_AUX_MERGE = merge; the merged launch must have been enqueued exactly ``want_calls`` times (0 when off), so
    that on against off can never be the per-head path compared with itself."""
    eng = fresh_engine(m, monkeypatch, merge)
    L_ = m.cfg.frames(x.shape[1])
    assert eng._aux_merge_ok(L_, m.cfg.padded_frames(L_)) == (merge != "0")
    del calls[:]
    audio, aux = m(x)
    torch.cuda.synchronize()
    assert len(calls) == want_calls, (merge, len(calls))
    return [a.clone() for a in audio], [[t.clone() for t in a] for a in aux]


def _assert_same(a, b, R, S):
    assert len(a[1]) == len(b[1]) == R
    for s in range(S):
        assert torch.equal(a[0][s], b[0][s]), f"audio[{s}]"
        for i in range(R):
            assert torch.equal(a[1][i][s], b[1][i][s]), f"aux_{i}[{s}]"


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,pipelines", [(2, 4000, 1), (16, 2000, 2)])
def test_whole_base_forward_switch_on_equals_off(B, T, pipelines, monkeypatch):
    m = gpu_model(BASE)
    assert m.effective_pipelines(B) == pipelines
    x = synth_mixture(B, T, seed=3).cuda() * 4.0
    calls = count_merged_launches(monkeypatch)
    try:
        off = _whole_forward(m, monkeypatch, x, "0", calls, 0)
        on = _whole_forward(m, monkeypatch, x, "1", calls, pipelines)          # one merged launch per pipeline (peer engine)
        assert pipelines == 1 or (len(set(map(id, calls))) == pipelines and all(e.aux_merge for e in calls))
        auto = _whole_forward(m, monkeypatch, x, None, calls, 0)               # unset = auto: only where the merged grid fills the device
        eng, L4 = m.engine(), m.cfg.frames(32000)
        assert eng._cus >= 64 and not eng._aux_merge_pays(1, L4) and eng._aux_merge_pays(16, L4) and not eng._aux_merge_pays(B // pipelines, m.cfg.frames(T))
    finally:
        m._engine = None
    _assert_same(on, off, m.cfg.num_stages, m.cfg.num_spks)
    _assert_same(auto, off, m.cfg.num_stages, m.cfg.num_spks)


@pytest.mark.gpu
def test_whole_base_forward_graph_replay(monkeypatch):
    m = gpu_model(BASE)
    x = synth_mixture(2, 4000, seed=4).cuda() * 4.0
    calls = count_merged_launches(monkeypatch)
    try:
        off = _whole_forward(m, monkeypatch, x, "0", calls, 0)
        m.use_graphs = True
        on = _whole_forward(m, monkeypatch, x, "1", calls, 3)                  # two warm-up forwards + the captured one
        assert len(m.engine()._graphs) == 1
    finally:
        m.use_graphs = False
        m._engine = None
    _assert_same(on, off, m.cfg.num_stages, m.cfg.num_spks)


def test_aux_decoder_argument_checks():
    """Validation happens before any HIP call (no device needed): NH out of range, a null entry in a pointer array, N = 96, K != 16."""
    lib = L.load()
    fake = 0x1000                                          # never dereferenced: every call below is refused first

    def call(NH=2, null_at=None, N=64, K=16, S=2, stride=4):
        n = max(NH, 1)
        arrs = [(C.c_void_p * n)(*[fake] * n) for _ in range(4)]
        if null_at is not None:
            arrs[null_at][n - 1] = None
        return lib.sepr_aux_decoder_fwd(NH, *arrs, (C.c_int * n)(*[8] * n), fake, 2, S, 32, N, K, stride, None)

    assert call(NH=0) == L.SEPR_EINVAL
    assert call(NH=5) == L.SEPR_EINVAL
    for which in range(4):                                 # o2, idx, wdec, wav
        assert call(null_at=which) == L.SEPR_EINVAL
    assert call(N=96) == L.SEPR_EINVAL
    assert call(K=8) == L.SEPR_EINVAL
    assert call(K=32) == L.SEPR_EINVAL
    assert call(S=4) == L.SEPR_EINVAL
    assert call(stride=2) == L.SEPR_EINVAL
    assert lib.sepr_aux_decoder_fwd(2, None, None, None, None, None, fake, 2, 2, 32, 64, 16, 4, None) == L.SEPR_EINVAL
    assert lib.sepr_outlayer_basis_fwd(fake, 4, 40, 32, 64, 64, None, fake, None, 0, None) == L.SEPR_EINVAL
