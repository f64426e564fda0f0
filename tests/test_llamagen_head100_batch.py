"""Several prompts per forward at head_dim 100 (GPT-3B), on the host: LlamaGenBackbone.enable_fused(pad_head_dim=True, padded_batch=True) packs the
padded model for windows of 128 / 256 rows on the sets swept at GPT-3B's shapes; the plain call keeps refusing and names the argument; so do
SJDBatchEngine's row checks.  Everything that packs runs on TOY100 (dim 800, 8 heads of 100: tests/test_llamagen_head100.py says why)."""
import importlib.util
import os

import pytest
import torch

import sjd_amd.backbones as BB
import sjd_amd.ops as ops
from sjd_amd.engine_batch import SJDBatchEngine
from tests.helpers import make_llamagen
from tests.test_llamagen_head100 import TINY, TOY100

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS = BB.LlamaGenBackbone
GPT3B_K = dict(qkv=3200, o=32 * 128, gate_up=3200, down=8704, head=3200)        # the reduction length of every projection of GPT-3B, heads stored 128 wide
GPT3B_MIN_KC = dict(qkv=400, o=512, gate_up=400, down=1088, head=400)           # the smallest chunk that leaves at most eight split-K planes


def _toy(dtype=torch.bfloat16, **kw):
    return make_llamagen(dict(TOY100, **kw), 3, 0.25, None, dtype=dtype)


@pytest.mark.parametrize("rows", [128, 256])
def test_plain_call_still_refuses_and_names_padded_batch(rows):
    with pytest.raises(ValueError, match="at most 64 rows") as e:
        _toy().enable_fused(ops, gemm="sjd", max_rows=rows, pad_head_dim=True)
    assert "padded_batch" in str(e.value)
    with pytest.raises(ValueError, match="at most 64 rows"):
        _toy().enable_fused(ops, gemm="sjd", max_rows=rows, pad_head_dim=True, padded_batch=False)


@pytest.mark.parametrize("rows", [128, 256])
def test_swept_sets_obey_the_rule(rows):
    cfg, head = getattr(CLS, f"G1_CFG_LLAMAGEN_3B_{rows}ROW"), getattr(CLS, f"HEAD_CFG_3B_{rows}ROW")
    assert set(cfg) == {"qkv", "o", "gate_up", "down"}
    for name, (kc, tiles, step_major) in list(cfg.items()) + [("head", head)]:
        assert tiles in CLS.G1_WIDE_TILES, name
        assert kc % 16 == 0 and kc >= GPT3B_MIN_KC[name], name
        assert -(-GPT3B_K[name] // kc) <= 8, name
        assert isinstance(step_major, bool)


@pytest.mark.parametrize("rows", [128, 256])
def test_swept_sets_are_the_fastest_shapes_of_the_committed_sweeps(rows):
    """the rule of the other sets: per projection the fastest swept shape among those with at most eight planes and a G1w tile count"""
    import json
    recs = [json.loads(l) for l in open(os.path.join(ROOT, "profiles", f"llamagen_g1_sweep_3b_{rows}rows.jsonl")) if l.strip()]
    shapes = [r for r in recs if "us" in r and "best" not in r]
    assert shapes and all(r["preset"] == "GPT-3B" and r["rows"] == rows for r in shapes)
    assert {r["proj"]: (r["N"], r["K"]) for r in shapes} == dict(qkv=(9600, 3200), o=(3200, 4096), gate_up=(17408, 3200), down=(3200, 8704), head=(16384, 3200))
    sets = dict(getattr(CLS, f"G1_CFG_LLAMAGEN_3B_{rows}ROW"), head=getattr(CLS, f"HEAD_CFG_3B_{rows}ROW"))
    for name, cfg in sets.items():
        ok = [r for r in shapes if r["proj"] == name and r["waves"] in CLS.G1_WIDE_TILES and -(-r["K"] // r["kc"]) <= 8 and r["kc"] >= GPT3B_MIN_KC[name]]
        best = min(ok, key=lambda r: r["us"])
        assert tuple(cfg) == (best["kc"], best["waves"], best["step_major"]), (name, best)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows", [128, 256])
def test_padded_batch_packing(rows, dtype):
    m = _toy(dtype)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    wo = [l.attention.wo.weight.detach().clone() for l in m.layers]
    wqkv = [l.attention.wqkv.weight.detach().clone() for l in m.layers]
    m.enable_fused(ops, gemm="sjd", max_rows=rows, pad_head_dim=True, padded_batch=True, untuned_fp16=True)
    assert m.max_rows == rows and m._fused_rows == rows and m._head_pad == 128 and m.supports_head_partials
    c = m.G1_CFG
    assert c == getattr(CLS, f"G1_CFG_LLAMAGEN_3B_{rows}ROW") and tuple(m.HEAD_CFG) == getattr(CLS, f"HEAD_CFG_3B_{rows}ROW")
    assert c is not getattr(CLS, f"G1_CFG_LLAMAGEN_3B_{rows}ROW")                   # a copy: the class's set stays what it is
    H, D = 8, 100
    for li, layer in enumerate(m.layers):
        wide = torch.zeros(H * D, H, 128, dtype=dtype)                              # wo with zero columns at each head's pad positions: K = H * 128
        wide[:, :, :D] = wo[li].view(H * D, H, D)
        assert not wide[:, :, D:].any()
        assert m._packed[li]["o"].numel() == H * D * H * 128
        assert torch.equal(m._packed[li]["o"], ops.pack_weight(wide.view(H * D, H * 128), c["o"][0], c["o"][2]))
        folded = (wqkv[li].float() * layer.attention_norm.weight.float()[None, :]).to(dtype)
        assert torch.equal(m._packed[li]["qkv"], ops.pack_weight(folded, c["qkv"][0], c["qkv"][2]))      # q|k|v at its true size: F2 pads
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_padded_batch_is_inert_elsewhere():
    a = _toy().enable_fused(ops, gemm="sjd", pad_head_dim=True)
    b = _toy().enable_fused(ops, gemm="sjd", pad_head_dim=True, padded_batch=True)              # 64 rows: the one-prompt packing, bit for bit
    assert a.G1_CFG == b.G1_CFG == CLS.G1_CFG_LLAMAGEN_3B and tuple(b.HEAD_CFG) == CLS.HEAD_CFG_3B and b.max_rows == 64
    for pa, pb in zip(a._packed, b._packed):
        assert all(torch.equal(pa[k], pb[k]) for k in pa)
    assert torch.equal(a._packed_head, b._packed_head)
    with pytest.raises(ValueError, match="head_dim 100") as e:                                    # without pad_head_dim=True: the plain refusal
        _toy().enable_fused(ops, gemm="sjd", max_rows=128, padded_batch=True)
    assert "pad_head_dim" in str(e.value)
    n = make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd", max_rows=128, pad_head_dim=True, padded_batch=True)
    assert n._head_pad is None and n.G1_CFG == CLS.G1_CFG_LLAMAGEN_128ROW and tuple(n.HEAD_CFG) == CLS.HEAD_CFG_128ROW      # head_dim 64: its own sets


def test_callers_shapes_win_and_are_checked():
    m = _toy()
    mine = dict(qkv=(400, 2, False), o=(512, 3, True), gate_up=(800, 4, False), down=(1088, 6, True))
    m.G1_CFG, m.HEAD_CFG = dict(mine), (800, 2, True)
    m.enable_fused(ops, gemm="sjd", max_rows=256, pad_head_dim=True, padded_batch=True)
    assert m.G1_CFG == mine and m.HEAD_CFG == (800, 2, True) and m.max_rows == 256
    assert m._packed[0]["o"].numel() == 800 * 8 * 128
    bad = _toy()
    bad.G1_CFG = dict(mine, o=(512, 5, True))
    with pytest.raises(ValueError, match="column tiles per workgroup.*'o'"):
        bad.enable_fused(ops, gemm="sjd", max_rows=128, pad_head_dim=True, padded_batch=True)


def test_fp16_and_max_rows_rules_hold():
    with pytest.raises(ValueError, match="fp16 windows of at most 128 rows"):
        _toy(torch.float16).enable_fused(ops, gemm="sjd", max_rows=256, pad_head_dim=True, padded_batch=True)
    m = _toy(torch.float16).enable_fused(ops, gemm="sjd", max_rows=128, pad_head_dim=True, padded_batch=True)      # 128 rows: freely
    assert m.max_rows == 128 and m.G1_CFG == CLS.G1_CFG_LLAMAGEN_3B_128ROW
    with pytest.raises(ValueError, match="max_rows is 64, 128 or 256"):
        _toy().enable_fused(ops, gemm="sjd", max_rows=96, pad_head_dim=True, padded_batch=True)
    with pytest.raises(ValueError, match="n_kv_head == n_head"):
        _toy(n_kv_head=4).enable_fused(ops, gemm="sjd", max_rows=128, pad_head_dim=True, padded_batch=True)
    r = _toy(torch.float16)
    with pytest.raises(ValueError):
        r.enable_fused(ops, gemm="sjd", max_rows=256, pad_head_dim=True, padded_batch=True)
    assert "G1_CFG" not in r.__dict__ and "HEAD_CFG" not in r.__dict__            # a refused call leaves no set behind that a later call would take for the caller's


@pytest.mark.parametrize("order", ["cache_first", "fused_first"])
def test_cache_is_128_wide_in_both_call_orders(order):
    m = _toy()
    if order == "cache_first":
        m.setup_cache(batch=8, s_max=96)
        assert m.cache.k.shape == (2, 8, 8, 96, 100)
        v0 = m.buffers_version
        m.enable_fused(ops, gemm="sjd", max_rows=128, pad_head_dim=True, padded_batch=True)
        assert m.buffers_version >= v0 + 2
    else:
        m.enable_fused(ops, gemm="sjd", max_rows=128, pad_head_dim=True, padded_batch=True)
        m.setup_cache(batch=8, s_max=96)
    assert m.cache.k.shape == (2, 8, 8, 96, 128) and m.cache.v.shape == m.cache.k.shape
    assert not m.cache.k.any() and not m.cache.v.any()
    assert m._rope_ext.shape[1:] == (50, 2)


def test_forward_window_row_limit(monkeypatch):
    m = _toy().enable_fused(ops, gemm="sjd", max_rows=256, pad_head_dim=True, padded_batch=True)
    took = []
    monkeypatch.setattr(m, "_forward_window_g1", lambda *a, **k: took.append("g1"))
    monkeypatch.setattr(m, "forward_embeds", lambda *a, **k: took.append("aten"))
    for rows in (32, 128, 256, 272):
        m.forward_window(torch.zeros(rows // 16, 16, dtype=torch.long), None, 0, None)
    assert took == ["g1", "g1", "g1", "aten"]


def test_batch_engine_refusals_name_the_arguments():
    m = _toy()
    with pytest.raises(ValueError, match=r"enable_fused\(ops, gemm='sjd', max_rows=") as e:
        SJDBatchEngine(m, 16384, "cpu", 4)                                            # not fused
    assert "padded_batch=True" in str(e.value) and "pad_head_dim=True" in str(e.value)
    m.enable_fused(ops, gemm="sjd", pad_head_dim=True)
    with pytest.raises(ValueError, match=r"max_rows=64 rows.*= 128.*max_rows=128, pad_head_dim=True, padded_batch=True"):
        SJDBatchEngine(m, 16384, "cpu", 4)                                            # packed for 64 rows, 4 x 2 x 16 = 128
    with pytest.raises(ValueError, match=r"= 256.*max_rows=256, pad_head_dim=True, padded_batch=True"):
        SJDBatchEngine(m, 16384, "cpu", 8)
    m4 = _toy().enable_fused(ops, gemm="sjd", max_rows=128, pad_head_dim=True, padded_batch=True)
    with pytest.raises(ValueError, match=r"= 160.*max_rows=256, pad_head_dim=True, padded_batch=True"):
        SJDBatchEngine(m4, 16384, "cpu", 5)
    h = _toy(torch.float16).enable_fused(ops, gemm="sjd", max_rows=128, pad_head_dim=True, padded_batch=True)
    with pytest.raises(ValueError, match=r"fp16 windows of at most 128 rows.*untuned_fp16=True, pad_head_dim=True, padded_batch=True"):
        SJDBatchEngine(h, 16384, "cpu", 5)
    n = make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd")
    with pytest.raises(ValueError, match=r"max_rows=128\)$"):                        # head_dim 64: the message it had
        SJDBatchEngine(n, 16384, "cpu", 3)


def test_example_and_bench_serve_gpt_3b_with_several_prompts():
    src = open(os.path.join(ROOT, "examples", "llamagen_c2i.py")).read()
    assert "pad_head_dim=gpt.head_dim == 100" in src and "padded_batch=rows > 64" in src
    spec = importlib.util.spec_from_file_location("llamagen_c2i_example", os.path.join(ROOT, "examples", "llamagen_c2i.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    a = ex.parse_args(["--fused", "--gpt-model", "GPT-3B", "--image-size", "384", "--class-id", "207", "1", "980", "417"])
    assert a.class_id == [207, 1, 980, 417] and a.gpt_model == "GPT-3B"
    tool = open(os.path.join(ROOT, "tools", "llamagen_bench.py")).read()
    assert "padded_batch=" in tool and "served at one prompt per forward" not in tool
    for rows in (128, 256):                                                           # the sweeps the sets were read from are in the tree
        path = os.path.join(ROOT, "profiles", f"llamagen_g1_sweep_3b_{rows}rows.jsonl")
        assert os.path.isfile(path) and os.path.getsize(path) < (1 << 20)
