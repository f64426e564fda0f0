"""LlamaGenBackbone.enable_fused on the host: its refusals, the extended rotary table F2 reads, the gate|up packing order, and the
un-fused window forward left as it was."""
import pytest
import torch

import sjd_amd.backbones as BB
import sjd_amd.ops as ops
from oracle.attention_ref import OracleWindowAttention
from tests.helpers import make_llamagen

TINY = dict(dim=128, n_layer=2, n_head=2, vocab_size=16384, block_size=64, cls_token_num=1, model_type="c2i", num_classes=1000)


def test_enable_fused_refusals():
    with pytest.raises(ValueError, match="16-bit"):
        make_llamagen(TINY, 1, 0.25, None).enable_fused(ops, gemm="sjd")                          # fp32 weights
    gpt3b_like = dict(TINY, dim=200, n_head=2)                                                     # head_dim 100, as GPT-3B
    with pytest.raises(ValueError, match="head_dim 100"):
        make_llamagen(gpt3b_like, 1, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd")
    with pytest.raises(ValueError, match="gemm='sjd'"):
        make_llamagen(TINY, 1, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="torch")
    m = make_llamagen(TINY, 1, 0.25, None, dtype=torch.bfloat16)
    assert not getattr(m, "supports_head_partials", False)                                       # only once fused
    m.enable_fused(ops, gemm="sjd")
    assert m.supports_head_partials and "supports_head_partials" in m.__dict__


@pytest.mark.parametrize("model_type,cls,grid", [("c2i", 1, 16), ("t2i", 120, 32)])
def test_extended_rope_table(model_type, cls, grid):
    m = BB.LlamaGenBackbone(BB.LlamaGenArgs(dim=128, n_layer=1, n_head=2, block_size=grid * grid, cls_token_num=cls, model_type=model_type))
    n_real = cls + grid * grid
    for s_max in (n_real - 40, n_real, n_real + 77):
        m.setup_cache(batch=2, s_max=s_max)
        t = m._rope_ext
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (max(s_max, n_real), 32, 2) and t.shape[0] >= s_max
        assert torch.equal(t[:n_real], m.freqs)
        assert not t[:cls].any()                                           # condition rows: no rotation (zero cos / sin)
        assert torch.equal(t[n_real:], m.freqs[-1:].expand(t.shape[0] - n_real, -1, -1))
        pos = torch.arange(t.shape[0])
        assert torch.equal(t[pos], m.freqs[pos.clamp(max=m.freqs.shape[0] - 1)])      # = forward_embeds' clamp
    v0 = m.buffers_version
    m.setup_cache(batch=2, s_max=64)
    assert m.buffers_version == v0 + 1


def test_gate_up_concatenation_order():
    m = make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16)
    w1 = [l.feed_forward.w1.weight.detach().clone() for l in m.layers]
    w3 = [l.feed_forward.w3.weight.detach().clone() for l in m.layers]
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    v0 = getattr(m, "buffers_version", 0)
    m.enable_fused(ops, gemm="sjd")
    assert m.buffers_version == v0 + 1
    c = m.G1_CFG
    for li, layer in enumerate(m.layers):
        gu = m._fused[li]
        assert torch.equal(gu, torch.cat([w1[li], w3[li]]))                 # gate (w1) first, then up (w3)
        ff = layer.feed_forward
        assert ff.w1.weight.data_ptr() == gu.data_ptr() and torch.equal(ff.w3.weight, w3[li])
        g = layer.ffn_norm.weight.float()
        folded = (gu.float() * g[None, :]).to(gu.dtype)
        assert torch.equal(m._packed[li]["gate_up"], ops.pack_weight(folded, c["gate_up"][0], c["gate_up"][2]))
    for k, v in m.state_dict().items():                                      # the state dict is unchanged
        assert torch.equal(v, sd[k]), k


def test_forward_window_unfused_unchanged():
    m = make_llamagen(TINY, 5, 0.25, OracleWindowAttention())
    m.setup_cache(batch=2, s_max=96)
    toks = torch.randint(0, 16384, (2, 5), generator=torch.Generator().manual_seed(1))
    pos = (3 + torch.arange(5))[None].repeat(2, 1)
    ks = torch.zeros(2, dtype=torch.long)
    a = m.forward_window(toks, pos, 3, ks)
    k_a = m.cache.k.clone()
    m.setup_cache(batch=2, s_max=96)
    b = m.forward_embeds(m.tok_embeddings(toks), pos, 3, ks)
    assert torch.equal(a, b) and torch.equal(k_a, m.cache.k)
    c = m.forward_window(toks, pos, 3, ks, head_partials=True)              # un-fused: logits as before, whatever the flag
    assert torch.equal(a, c)
