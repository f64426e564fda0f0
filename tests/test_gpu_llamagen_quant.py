"""GPU: a LlamaGen backbone packed as e4m3 / MXFP4 (LlamaGenBackbone.enable_fused(weights=...)) against its "_as_bf16" twin, which holds the
same dequantised values at 16 bits on the same launch shapes.  Nothing here has a tolerance: the quantised kernels (G1q / G1wq, G1q4 / G1wq4)
rebuild the twin's MFMA operands bit for bit, so logits are compared bit for bit and decodes token for token."""
import pytest
import torch

import sjd_amd.backbones as BB
import sjd_amd.engine_batch as EB
import sjd_amd.launch_shapes as LS
import sjd_amd.ops as ops
import tests.test_gpu_llamagen_batch as B
from tests.helpers import make_llamagen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMATS = [("e4m3", "PackedQ8"), ("mxfp4", "PackedQ4")]


def _window(Bn, n, seed, vocab=16384):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, vocab, (Bn, n), generator=g).to(DEV), torch.arange(n)[None].repeat(Bn, 1).to(DEV), 0,
            torch.zeros(Bn, dtype=torch.int32, device=DEV))


def _same_head(a, b, rows):
    assert isinstance(a, ops.HeadOut) and isinstance(b, ops.HeadOut) and (a.col0, a.urow_off) == (b.col0, b.urow_off)
    assert a.part.data.shape == b.part.data.shape and torch.equal(a.part.data.view(torch.int32), b.part.data.view(torch.int32))
    sa, sb = a.row_norm[0][:, :rows].contiguous(), b.row_norm[0][:, :rows].contiguous()          # (the statistics of rows past the window are never written)
    assert torch.equal(sa.view(torch.int32), sb.view(torch.int32)) and a.row_norm[1:] == b.row_norm[1:]
    assert bool(torch.isfinite(a.part.data).all()) and float(a.part.data.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ a. one copy, every row count
@pytest.fixture(scope="module", params=FORMATS, ids=[f[0] for f in FORMATS])
def toy_pair(request):
    wt, cls = request.param
    out = []
    for w in (wt, wt + "_as_bf16"):
        m = make_llamagen(B.TOY_C2I, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
        m.enable_fused(ops, gemm="sjd", weights=w, max_rows=256)
        assert m.G1_CFG == LS.LLAMAGEN_QUANT_SETS[False, 256][0] and m.max_rows == 256
        m.setup_cache(batch=16, s_max=64)
        out.append(m)
    assert all(isinstance(x, getattr(ops, cls)) for d in out[0]._packed for x in d.values())
    assert all(isinstance(x, torch.Tensor) for d in out[1]._packed for x in d.values())
    return out


@pytest.mark.parametrize("rows", [16, 32, 64, 96, 128, 256])
def test_window_head_partials_equal_the_twins(toy_pair, rows, monkeypatch):
    """<= 32 rows, 33..64 (G1q / G1q4) and three, four and eight row tiles (G1wq / G1wq4) on the SAME packed copy"""
    seen, real = [], ops.skinny_gemm
    monkeypatch.setattr(ops, "skinny_gemm", lambda x, w, *a, **k: (seen.append((int(x.shape[0]), type(w).__name__)), real(x, w, *a, **k))[1])
    args = _window(rows // 16, 16, rows)
    with torch.no_grad():
        hq, ht = [m.forward_window(*args, head_partials=True) for m in toy_pair]
    torch.cuda.synchronize()
    _same_head(hq, ht, rows)
    kinds = {k for r, k in seen if r == rows}
    assert len(seen) == 2 * 4 * 2 and kinds == {type(toy_pair[0]._packed[0]["qkv"]).__name__, "Tensor"}          # every projection ran on G1 at the full row count


# ------------------------------------------------------------------------------------------------ b. teacher-forced loops, SJDBatchEngine
def _quantised(monkeypatch, weights):
    """tests.test_gpu_llamagen_batch builds its models with make_llamagen and packs them itself: hand it models whose enable_fused adds `weights`"""
    real = make_llamagen

    def make(*a, **k):
        m = real(*a, **k)
        packed = m.enable_fused
        m.enable_fused = lambda ops_, **kw: packed(ops_, weights=weights, **kw)
        return m
    monkeypatch.setattr(B, "make_llamagen", make)


def _decodes(monkeypatch):
    got, real = [], EB.SJDBatchEngine.decode_many

    def decode_many(self, *a, **k):
        assert getattr(self.backbone, "weights", None) is not None
        res = real(self, *a, **k)
        got.append([(list(seq), list(st.matched)) for seq, st in res])
        return res
    monkeypatch.setattr(EB.SJDBatchEngine, "decode_many", decode_many)
    return got


@pytest.mark.parametrize("n_prompts,n_slots,use_graph", [(3, 3, True), (3, 3, False), (8, 8, True), (5, 3, True)],
                         ids=["3-graph", "3-eager", "8-graph", "5-on-3-slots-refill"])
@pytest.mark.parametrize("weights", ["e4m3", "mxfp4"])
def test_teacher_forced_batch_tokens_equal_the_twins(monkeypatch, weights, n_prompts, n_slots, use_graph):
    """96 and 256 window rows per forward; every run also replays its logits into the CPU oracle (_tf_batch)"""
    got = _decodes(monkeypatch)
    for w in (weights, weights + "_as_bf16"):
        _quantised(monkeypatch, w)
        B._tf_batch(B.TOY_C2I, n_prompts, n_slots, use_graph=use_graph)
    q, t = got
    assert len(q) == n_prompts and q == t, "the quantised backbone and its twin accepted different tokens"
    assert len({tuple(s) for s, _ in q}) == n_prompts


@pytest.mark.parametrize("weights", ["e4m3", "mxfp4"])
def test_solver_generate_equals_the_twin(monkeypatch, weights):
    outs = []
    for w in (weights, weights + "_as_bf16"):
        _quantised(monkeypatch, w)
        outs.append(B._solver_many(True, None))          # five labels on five slots: 160 rows
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ c. GPT-3B width
def test_gpt_3b_width_forward_of_128_rows_equals_the_twin():
    """dim 3200, 32 heads of 100 stored 128 wide, intermediate 8704 (K = 3200, 4096 and 8704: 25, 32 and 68 granules), two layers, MXFP4"""
    import sjd_amd.synthetic as synthetic
    a = BB.LlamaGenArgs(dim=3200, n_layer=2, n_head=32, vocab_size=4096, block_size=576, model_type="c2i", cls_token_num=1, num_classes=1000)
    pair = []
    for w in ("mxfp4", "mxfp4_as_bf16"):
        with torch.device(DEV):
            m = BB.LlamaGenBackbone(a, attn=ops.HipWindowAttention(n_split=2)).to(torch.bfloat16).eval()
        synthetic.fill_state_dict_device(m, seed=5, embed_token_scale=0.5)
        m.enable_fused(ops, gemm="sjd", weights=w, max_rows=128, pad_head_dim=True, padded_batch=True)
        assert m.G1_CFG == LS.LLAMAGEN_QUANT_SETS[True, 128][0] and m._head_pad == 128
        m.setup_cache(batch=8, s_max=64)
        m.cache.k.fill_(7.0)
        m.cache.v.fill_(7.0)
        pair.append(m)
    mq, mt = pair
    assert isinstance(mq._packed[0]["o"], ops.PackedQ4) and mq._packed[0]["o"].K == 4096
    assert 0 < mq.compress_stats["rel_rms_error"] < 0.2 and mq.compress_stats["bytes_packed"] < 0.27 * mq.compress_stats["bytes_raw"]
    toks, pos, _, ks = _window(8, 16, 3, vocab=4096)
    with torch.no_grad():
        hq, ht = [m.forward_window(toks, pos, 0, ks, head_partials=True) for m in pair]
    torch.cuda.synchronize()
    _same_head(hq, ht, 128)
    for m in pair:
        for c in (m.cache.k, m.cache.v):
            assert not c[:, :, :, :16, 100:].any() and bool((c[:, :, :, 16:] == 7.0).all())          # the appended rows' pad columns; nothing else written
            assert float(c[:, :, :, :16, :100].float().abs().max()) > 0
    assert torch.equal(mq.cache.k.view(torch.int16), mt.cache.k.view(torch.int16)) and torch.equal(mq.cache.v.view(torch.int16), mt.cache.v.view(torch.int16))
