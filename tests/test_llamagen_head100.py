"""LlamaGenBackbone.enable_fused(pad_head_dim=True) on the host: head_dim 100 (GPT-3B) stored 128 wide.

The refusal cases run on dim 200 / 2 heads, the smallest head_dim-100 model.  Everything that PACKS runs on dim 800 / 8 heads: kernel G1 and
ops.pack_weight take whole 32-column tiles and 16-wide k-steps, and at head_dim 100 the q|k|v projection's 300 * n_head columns and the hidden size
100 * n_head are such multiples only for head counts that are multiples of 8 -- dim 200 cannot be packed at all, with or without padding, and
enable_fused says so.
"""
import os
import re

import pytest
import torch

import sjd_amd._lib as L
import sjd_amd.backbones as BB
import sjd_amd.ops as ops
from tests.helpers import make_llamagen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(dim=128, n_layer=2, n_head=2, vocab_size=16384, block_size=64, cls_token_num=1, model_type="c2i", num_classes=1000)
GPT3B_LIKE = dict(TINY, dim=200, n_head=2)           # head_dim 100, as GPT-3B
TOY100 = dict(TINY, dim=800, n_head=8)               # head_dim 100 at the smallest width kernel G1 packs


def test_plain_call_still_refuses_and_names_the_argument():
    with pytest.raises(ValueError, match="head_dim 100") as e:
        make_llamagen(GPT3B_LIKE, 1, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd")
    assert "pad_head_dim" in str(e.value)
    with pytest.raises(ValueError, match="head_dim 100") as e:
        make_llamagen(TOY100, 1, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd")
    assert "pad_head_dim" in str(e.value)


def test_padded_refusals():
    with pytest.raises(ValueError, match="multiple of 32"):         # dim 200: no whole 32-column tiles (see the module docstring)
        make_llamagen(GPT3B_LIKE, 1, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd", pad_head_dim=True)
    for rows in (128, 256):                                          # the padded path ships windows of at most 64 rows
        with pytest.raises(ValueError, match="at most 64 rows"):
            make_llamagen(TOY100, 1, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd", max_rows=rows, pad_head_dim=True)
    with pytest.raises(ValueError, match="n_kv_head == n_head"):
        make_llamagen(dict(TOY100, n_kv_head=4), 1, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd", pad_head_dim=True)
    with pytest.raises(ValueError, match="head_dim 96"):              # the argument serves head_dim 100 only
        make_llamagen(dict(TINY, dim=768, n_head=8), 1, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd", pad_head_dim=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_padded_packing(dtype):
    m = make_llamagen(TOY100, 3, 0.25, None, dtype=dtype)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    wqkv = [l.attention.wqkv.weight.detach().clone() for l in m.layers]
    wo = [l.attention.wo.weight.detach().clone() for l in m.layers]
    v0 = getattr(m, "buffers_version", 0)
    m.enable_fused(ops, gemm="sjd", pad_head_dim=True)
    assert m.buffers_version == v0 + 1 and m.supports_head_partials and m.max_rows == 64
    c = m.G1_CFG
    assert c == BB.LlamaGenBackbone.G1_CFG_LLAMAGEN_3B
    H, D = 8, 100
    for li, layer in enumerate(m.layers):
        g = layer.attention_norm.weight.float()
        folded = (wqkv[li].float() * g[None, :]).to(dtype)                 # q|k|v at its TRUE size: N = 3 * 8 * 100 (F2 does the padding)
        assert folded.shape == (3 * H * D, H * D)
        assert torch.equal(m._packed[li]["qkv"], ops.pack_weight(folded, c["qkv"][0], c["qkv"][2]))
        wide = torch.zeros(H * D, H, 128, dtype=dtype)                      # wo with zero columns inserted at each head's pad positions
        wide[:, :, :D] = wo[li].view(H * D, H, D)
        wide = wide.view(H * D, H * 128)
        assert torch.equal(m._packed[li]["o"], ops.pack_weight(wide, c["o"][0], c["o"][2]))
        assert m._packed[li]["o"].numel() == H * D * H * 128
        assert not wide.view(H * D, H, 128)[:, :, D:].any() and torch.equal(wide.view(H * D, H, 128)[:, :, :D].reshape(H * D, H * D), wo[li])
    for k, v in m.state_dict().items():                                      # the state dict is unchanged
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("order", ["cache_first", "fused_first"])
def test_cache_is_128_wide_in_both_call_orders(order):
    m = make_llamagen(TOY100, 3, 0.25, None, dtype=torch.bfloat16)
    if order == "cache_first":
        m.setup_cache(batch=2, s_max=96)
        assert m.cache.k.shape == (2, 2, 8, 96, 100)
        v0 = m.buffers_version
        m.enable_fused(ops, gemm="sjd", pad_head_dim=True)
        assert m.buffers_version >= v0 + 2                                    # the packed weights AND the re-allocated cache
    else:
        m.enable_fused(ops, gemm="sjd", pad_head_dim=True)
        v0 = m.buffers_version
        m.setup_cache(batch=2, s_max=96)
        assert m.buffers_version == v0 + 1
    assert m.cache.k.shape == (2, 2, 8, 96, 128) and m.cache.v.shape == m.cache.k.shape and m.cache.k.dtype == torch.bfloat16
    assert not m.cache.k.any() and not m.cache.v.any()
    assert m._rope_ext.shape[1:] == (50, 2) and m._rope_ext.shape[0] >= 96 and m.freqs.shape[1:] == (50, 2)
    m.setup_cache(batch=4, s_max=128)                                         # a later cache of the padded model stays 128 wide
    assert m.cache.k.shape == (2, 4, 8, 128, 128)


@pytest.mark.parametrize("args", [TINY, dict(TINY, dim=256, n_head=2)], ids=["head_dim_64", "head_dim_128"])
def test_native_head_dims_are_unaffected(args):
    a = make_llamagen(args, 3, 0.25, None, dtype=torch.bfloat16)
    b = make_llamagen(args, 3, 0.25, None, dtype=torch.bfloat16)
    a.enable_fused(ops, gemm="sjd")
    b.enable_fused(ops, gemm="sjd", pad_head_dim=True)
    assert b._head_pad is None and a.G1_CFG == b.G1_CFG == BB.LlamaGenBackbone.G1_CFG_LLAMAGEN
    for pa, pb in zip(a._packed, b._packed):
        assert all(torch.equal(pa[k], pb[k]) for k in pa)
    assert torch.equal(a._packed_head, b._packed_head)
    b.setup_cache(batch=2, s_max=64)
    assert b.cache.k.shape[-1] == args["dim"] // 2


def test_mode_bits_header_and_lib_agree():
    hdr = open(os.path.join(ROOT, "include", "sjd_hip.h")).read()
    bit = lambda name: int(re.search(rf"#define {name} (0x[0-9a-f]+)", hdr).group(1), 16)
    assert L.F2_HEAD_PAD128 == bit("SJD_F2_HEAD_PAD128") == 0x400
    assert L.K1_HEAD_DIM_100 == bit("SJD_K1_HEAD_DIM_100") == 0x800
    assert len({L.F1_POST_NORM, L.F2_ROPE_TABLE, L.F2_HEAD_PAD128, L.K1_HEAD_DIM_100}) == 4
    assert not (L.F2_HEAD_PAD128 | L.K1_HEAD_DIM_100) & (0xff | (0xff << L.QKN_SHARDS_SHIFT))      # clear of the dtype code and the shard count


def test_example_and_bench_know_gpt_3b():
    import importlib.util
    spec = importlib.util.spec_from_file_location("llamagen_bench_tool", os.path.join(ROOT, "tools", "llamagen_bench.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.PRESETS["GPT-3B"] == (24, 32, 3200) and tool.CONFIG_3B == ("GPT-3B", "c2i", 384)
    a = tool._args(*tool.CONFIG_3B)
    assert a.dim // a.n_head == 100 and a.block_size == 576 and a.cls_token_num == 1
    src = open(os.path.join(ROOT, "examples", "llamagen_c2i.py")).read()
    assert "pad_head_dim=gpt.head_dim == 100" in src
