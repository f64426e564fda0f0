"""CPU: LlamaGenBackbone.enable_fused(compress=True) -- the lossless 12-bit stream (ops.pack_weight_z) for the four projections and the output head:
what gets packed and counted, that it decodes back to the folded matrices bit for bit, that the default call packs what it packed before, every refusal
(which leaves the backbone as it was), and the launch-shape sets (launch_shapes.LLAMAGEN_Z_SETS) with their rule at the real widths."""
import inspect

import numpy as np
import pytest
import torch

import sjd_amd.backbones as BB
import sjd_amd.launch_shapes as LS
import sjd_amd.ops as ops
from sjd_amd.engine_batch import SJDBatchEngine
from tests.helpers import make_llamagen
from tests.test_llamagen_batch import TINY
from tests.test_llamagen_head100 import TOY100
from tests.test_pack_z import decode_z

NAMES = ("qkv", "o", "gate_up", "down")
# (heads, dim) of the LlamaGen presets; the intermediate size is 8 dim / 3 rounded up to a multiple of 256
PRESETS = {"GPT-B": (12, 768), "GPT-XL": (20, 1280), "GPT-XXL": (24, 1536), "GPT-3B": (32, 3200)}
# TINY (dim 128, intermediate 512, two layers, vocabulary 16384) on LLAMAGEN_Z_SETS[False, 64]: per unit of (chunk c, 32 columns) 1.5 bytes per weight in
# whole record pairs plus a header of 32 entries x 8 bytes.  K = 128 (q|k|v, o, gate|up, head; one chunk of 8 k-steps): (32 * 128 * 1.5 + 256) /
# (32 * 128 * 2) = 0.78125; K = 512 (down, one chunk): (32 * 512 * 1.5 + 256) / (32 * 512 * 2) = 0.7578125.  Weighted by the matrices' sizes
# (per layer 3 * 128 + 128 + 1024 rows of K = 128 and 128 rows of K = 512; the head 16384 rows of K = 128):
TINY_BYTES_RAW = 2 * (2 * ((384 + 128 + 1024) * 128 + 128 * 512) + 16384 * 128)
TINY_BYTES_PACKED = 2 * ((384 + 128 + 1024) // 32 * (32 * 128 * 3 // 2 + 256) + 128 // 32 * (32 * 512 * 3 // 2 + 256)) + 16384 // 32 * (32 * 128 * 3 // 2 + 256)
TINY_RATIO = 0.7801          # = TINY_BYTES_PACKED / TINY_BYTES_RAW = 4089856 / 5242880 = 0.78008, to four digits (no raw units in Gaussian weights)


def _model(dtype=torch.bfloat16, args=TINY, **over):
    return make_llamagen(dict(args, **over), 3, 0.25, None, dtype=dtype)


def _folded(m):
    """per layer the four matrices enable_fused packs, norm gains folded in, computed here from the parameters; then the head"""
    fold = lambda w, g: (w.float() * g.float()[None, :]).to(w.dtype)
    with torch.no_grad():
        layers = [dict(qkv=fold(b.attention.wqkv.weight, b.attention_norm.weight), o=b.attention.wo.weight.clone(),
                       gate_up=fold(torch.cat([b.feed_forward.w1.weight, b.feed_forward.w3.weight]), b.ffn_norm.weight), down=b.feed_forward.w2.weight.clone())
                  for b in m.layers]
        return layers, fold(m.output.weight, m.norm.weight)


def _stream(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def test_the_keyword_defaults_to_false():
    p = inspect.signature(BB.LlamaGenBackbone.enable_fused).parameters["compress"]
    assert p.default is False and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


@pytest.mark.parametrize("max_rows", [64, 128])
def test_compress_packs_every_matrix_and_the_head_and_decodes_bit_for_bit(max_rows):
    layers, head = _folded(_model())
    m = _model().enable_fused(ops, gemm="sjd", compress=True, max_rows=max_rows)
    cfg, head_cfg = LS.LLAMAGEN_Z_SETS[False, max_rows]
    assert m.compress is True and m.weights is None and m.max_rows == max_rows and m.G1_CFG == cfg and tuple(m.HEAD_CFG) == tuple(head_cfg)
    for d, want in zip(m._packed, layers):
        for name in NAMES:
            z, (kc, _, sm) = d[name], cfg[name]
            assert isinstance(z, ops.PackedZ) and (z.KC, z.step_major) == (kc, sm) and (z.N, z.K) == tuple(want[name].shape)
            assert np.array_equal(decode_z(z), _stream(ops.pack_weight(want[name], kc, sm)))
    zh = m._packed_head
    assert isinstance(zh, ops.PackedZ) and (zh.KC, zh.step_major) == (head_cfg[0], head_cfg[2]) and m._head_cols == zh.N == 16384
    assert np.array_equal(decode_z(zh), _stream(ops.pack_weight(head, head_cfg[0], head_cfg[2])))
    st = m.compress_stats
    assert {"compressed", "exceptions", "raw_units", "declined", "declined_reasons", "bytes_raw", "bytes_packed"} <= set(st)
    assert st["compressed"] == st["matrices"] == 4 * 2 + 1 and st["declined"] == 0 and st["declined_reasons"] == {} and st["raw_units"] == 0
    assert st["bytes_raw"] == TINY_BYTES_RAW and st["bytes_packed"] == TINY_BYTES_PACKED == m.packed_bytes()
    assert 0.74 < st["bytes_packed"] / st["bytes_raw"] < 0.80 and round(st["bytes_packed"] / st["bytes_raw"], 4) == TINY_RATIO
    assert st["exceptions"] == sum(z.n_exceptions for d in m._packed for z in d.values()) + zh.n_exceptions
    assert LS.serves_rows(m, max_rows, head=True) is None and LS.serves_rows(m, max_rows + 32, head=True) == ("max_rows", max_rows)


def test_the_default_call_packs_what_it_packed_before():
    layers, head = _folded(_model())
    for kw in (dict(), dict(compress=False)):
        m = _model().enable_fused(ops, gemm="sjd", **kw)
        cfg, head_cfg = LS.LLAMAGEN_SETS[False, 64]
        assert m.G1_CFG == cfg and "HEAD_CFG" not in m.__dict__ and tuple(m.HEAD_CFG) == tuple(head_cfg) and m.compress is False
        assert m.compress_stats == dict(matrices=8, bytes_raw=TINY_BYTES_RAW - 2 * 16384 * 128, bytes_packed=TINY_BYTES_RAW - 2 * 16384 * 128)
        for d, want in zip(m._packed, layers):
            for name in NAMES:
                assert isinstance(d[name], torch.Tensor) and torch.equal(d[name].view(torch.int16), ops.pack_weight(want[name], cfg[name][0], cfg[name][2]).view(torch.int16))
        assert isinstance(m._packed_head, torch.Tensor)
        assert torch.equal(m._packed_head.view(torch.int16), ops.pack_weight(head, head_cfg[0], head_cfg[2]).view(torch.int16))


def test_a_padded_head_dim_100_packs_its_zero_columns_as_exceptions_or_raw_units():
    """wo stored 128 wide has 28 zero columns per head: every unit of the o projection holds them, none makes the packer decline"""
    m = _model(args=TOY100).enable_fused(ops, gemm="sjd", compress=True, pad_head_dim=True, padded_batch=True, max_rows=128)
    assert m.G1_CFG == LS.LLAMAGEN_Z_SETS[True, 128][0] and m._head_pad == 128
    st = m.compress_stats
    assert st["compressed"] == st["matrices"] == 9 and st["declined"] == 0
    wo = BB.LlamaGenBackbone._pad_o_weight(m.layers[0].attention.wo.weight.detach(), 8, 100, 128)
    z = m._packed[0]["o"]
    assert isinstance(z, ops.PackedZ) and z.K == 1024 and (z.n_raw > 0 or z.n_exceptions > 0)
    assert np.array_equal(decode_z(z), _stream(ops.pack_weight(wo, z.KC, z.step_major)))


def _refused(m, match, **kw):
    """the call raises and leaves the backbone as it was (never packed: nothing assigned; packed before: the same copies)"""
    keys, before = set(m.__dict__), [p.detach().clone() for p in m.parameters()]
    packed = [dict(d) for d in getattr(m, "_packed", [])]
    with pytest.raises(ValueError, match=match):
        m.enable_fused(ops, **kw)
    assert set(m.__dict__) == keys and all(torch.equal(p, q) for p, q in zip(m.parameters(), before))
    if not packed:
        assert getattr(m, "_ops", None) is None and not hasattr(m, "_packed") and not hasattr(m, "compress") and not hasattr(m, "compress_stats")
        assert "max_rows" not in m.__dict__ and "weights" not in m.__dict__
    else:
        assert all(a[k] is b[k] for a, b in zip(packed, m._packed) for k in a)


def test_every_refusal_leaves_the_backbone_unassigned():
    _refused(_model(torch.float16), r"compress=True needs bf16 weights.*12-bit form encodes bf16", gemm="sjd", compress=True)
    for wt in ("e4m3", "mxfp4", "e4m3_as_bf16"):
        _refused(_model(), "one stream per copy", gemm="sjd", compress=True, weights=wt)
    _refused(_model(), r"at most 128 rows.*max_rows=256", gemm="sjd", compress=True, max_rows=256)
    for gemm in ("torch", "hipblaslt"):
        _refused(_model(), "gemm='sjd'", gemm=gemm, compress=True)
    # by shape: a chunk above LS.Z_MAX_KC, on a projection (whatever its K) and on the head
    for name in NAMES:
        m = _model()
        m.G1_CFG = dict(LS.LLAMAGEN_Z_SETS[False, 64][0], **{name: (4112, 2, True)})
        _refused(m, rf"at most 4096 columns.*G1_CFG\['{name}'\] = \(4112, 2, True\)", gemm="sjd", compress=True)
    m = _model()
    m.HEAD_CFG = (8192, 4, True)
    _refused(m, r"at most 4096 columns.*HEAD_CFG = \(8192, 4, True\)", gemm="sjd", compress=True)
    m = _model()
    m.G1_CFG = dict(LS.LLAMAGEN_Z_SETS[False, 128][0], o=(256, 12, False))          # twelve tiles: served up to 64 rows, not by the 65..128-row kernel
    _refused(m, r"column tiles per workgroup; offending launch shapes: \['o'\]", gemm="sjd", compress=True, max_rows=128)          # (the check every set above 64 rows meets)
    assert isinstance(m.enable_fused(ops, gemm="sjd", compress=True, max_rows=64)._packed[0]["o"], ops.PackedZ)
    # a backbone packed before keeps its copies
    m = _model().enable_fused(ops, gemm="sjd", max_rows=128)
    _refused(m, "at most 128 rows", gemm="sjd", compress=True, max_rows=256)
    _refused(m, "one stream per copy", gemm="sjd", compress=True, weights="e4m3", max_rows=128)
    assert m.compress is False and m.max_rows == 128 and isinstance(m._packed[0]["qkv"], torch.Tensor)


def _dims(preset):
    n_head, dim = PRESETS[preset]
    inter = ((int(2 * (4 * dim) / 3) + 255) // 256) * 256
    D = dim // n_head
    return dict(LS.llamagen_dims(dim, n_head, D, inter, 128 if D == 100 else None), head=(16384, dim)), D == 100


@pytest.mark.parametrize("preset", list(PRESETS))
@pytest.mark.parametrize("max_rows", [64, 128])
def test_z_sets_pass_their_rule_at_the_real_widths(preset, max_rows):
    dims, pad = _dims(preset)
    cfg, head = LS.LLAMAGEN_Z_SETS[pad, max_rows]
    assert set(cfg) == set(NAMES) and LS.z_copy_errors(cfg, dims, max_rows, head) == []
    base, base_head = LS.LLAMAGEN_SETS[pad, max_rows]
    for name in NAMES:          # the 16-bit set, every chunk capped
        assert cfg[name] == (min(base[name][0], LS.Z_MAX_KC),) + tuple(base[name][1:])
    assert tuple(head) == (min(base_head[0], LS.Z_MAX_KC),) + tuple(base_head[1:])
    assert all(kc <= LS.Z_MAX_KC for kc, _, _ in list(cfg.values()) + [head])


def test_the_sets_have_no_256_row_key_and_the_rule_names_each_failure_kind():
    assert sorted(LS.LLAMAGEN_Z_SETS) == [(False, 64), (False, 128), (True, 64), (True, 128)]
    dims = dict(qkv=(3072, 1024), o=(1024, 1024), gate_up=(5632, 1024), down=(1024, 2816), head=(16384, 1024))
    bad = dict(qkv=(4112, 4, True), o=(256, 12, False), gate_up=(264, 4, True), down=(512, 0, False))
    assert dict(LS.z_copy_errors(bad, dims, 128, (8192, 4, True))) == dict(qkv="chunk", o="tiles", gate_up="granule", down="tiles", head="chunk")
    assert dict(LS.z_copy_errors(bad, dims, 64)) == dict(qkv="chunk", gate_up="granule", down="tiles")
    assert dict(LS.z_copy_errors(dict(o=(256, 4, False)), dims, 256, (640, 4, True))) == dict(o="rows", head="rows")
    assert LS.z_copy_errors(dict(down=(4096, 8, True)), dims, 128, (4096, 16, True)) == [("head", "tiles")]


def test_batch_engine_refuses_more_rows_than_the_copy_was_packed_for():
    m = _model().enable_fused(ops, gemm="sjd", compress=True, max_rows=128)
    with pytest.raises(ValueError, match=r"at most max_rows=128 rows.*= 160"):
        SJDBatchEngine(m, 16384, "cpu", 5)
