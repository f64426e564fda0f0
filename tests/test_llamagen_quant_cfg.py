"""CPU: LlamaGenBackbone.enable_fused(weights=...) -- the quantised launch-shape sets (launch_shapes.LLAMAGEN_QUANT_SETS) and their checker, what gets
packed, what is refused and that a refusal leaves the backbone as it was."""
import pytest
import torch

import sjd_amd.backbones as BB
import sjd_amd.launch_shapes as LS
import sjd_amd.ops as ops
from sjd_amd.engine_batch import SJDBatchEngine
from tests.helpers import make_llamagen
from tests.test_llamagen_batch import TINY

# (heads, dim) of the LlamaGen presets; the intermediate size is 8 dim / 3 rounded up to a multiple of 256
PRESETS = {"GPT-B": (12, 768), "GPT-L": (16, 1024), "GPT-XL": (20, 1280), "GPT-XXL": (24, 1536), "GPT-3B": (32, 3200)}


def _dims(preset):
    n_head, dim = PRESETS[preset]
    ff = int(2 * (4 * dim) / 3)
    inter = ((ff + 255) // 256) * 256
    D = dim // n_head
    return LS.llamagen_dims(dim, n_head, D, inter, 128 if D == 100 else None), D == 100


@pytest.mark.parametrize("preset", list(PRESETS))
@pytest.mark.parametrize("max_rows", [64, 128, 256])
def test_quantised_sets_pass_the_checker_at_the_real_widths(preset, max_rows):
    dims, pad = _dims(preset)
    assert all(k % 128 == 0 for _, k in dims.values())
    cfg, head = LS.LLAMAGEN_QUANT_SETS[pad, max_rows]
    assert set(cfg) == {"qkv", "o", "gate_up", "down"} and head == LS.LLAMAGEN_SETS[pad, max_rows][1]          # the head is not quantised: its shape stays
    for gran in (128, 32):
        assert LS.llamagen_quant_errors(cfg, dims, max_rows, gran, head) == []
    for name, (kc, tiles, sm) in cfg.items():
        assert kc % 128 == 0 and kc <= LS.CHUNK_CAP_32ROW
        assert LS.chunk_for_rows(name, cfg[name], 64, dims[name][1], "mxfp4", max_rows) <= LS.CHUNK_CAP_64ROW
        assert max_rows == 64 or tiles in (3, 4, 6, 8)


def test_checker_names_each_failure_kind():
    dims = dict(qkv=(3072, 1024), o=(1024, 1024), gate_up=(5632, 1024), down=(1024, 2816), odd=(1024, 4160), big=(1024, 8192))
    bad = dict(qkv=(192, 4, True),            # chunk no multiple of 128
               o=(256, 2, True),              # two tiles above 64 rows
               gate_up=(256, 5, True),        # not a tile count at all
               down=(1408, 4, False),         # 1408 > 1280 and tile-major: no halved chunk
               odd=(1280, 4, True),           # K = 4160 = 32.5 granules
               big=(2688, 4, True))           # above what 32 rows stage
    got = dict(LS.llamagen_quant_errors(bad, dims, 256, 128, (640, 5, True)))
    assert got == dict(qkv="granule", o="tiles", gate_up="tiles", down="halved", odd="granule", big="chunk", head="tiles")
    assert dict(LS.llamagen_quant_errors(bad, dims, 64, 128, (640, 5, True))) == dict(qkv="granule", down="halved", odd="granule", big="chunk")
    # e4m3's granule is 32: 192 and 4160 are whole pairs; 1408 step-major halves to 704 = 22 x 32, but 5.5 x 128
    ok32 = dict(LS.llamagen_quant_errors(dict(bad, down=(1408, 4, True)), dims, 64, 32))
    assert ok32 == dict(big="chunk")
    assert dict(LS.llamagen_quant_errors(dict(down=(1408, 4, True)), dims, 64, 128)) == dict(down="halved")
    assert LS.llamagen_quant_errors(dict(down=(2560, 4, True)), dims, 256, 128) == []          # 2560 -> 1280: ten granules


def _model(dtype=torch.bfloat16, **over):
    return make_llamagen(dict(TINY, **over), 3, 0.25, None, dtype=dtype)


@pytest.mark.parametrize("weights,cls", [("e4m3", "PackedQ8"), ("mxfp4", "PackedQ4")])
@pytest.mark.parametrize("max_rows", [64, 256])
def test_enable_fused_packs_the_quantised_copy_and_its_twin(weights, cls, max_rows):
    m = _model().enable_fused(ops, gemm="sjd", weights=weights, max_rows=max_rows)
    t = _model().enable_fused(ops, gemm="sjd", weights=weights + "_as_bf16", max_rows=max_rows)
    assert m.G1_CFG == t.G1_CFG == LS.LLAMAGEN_QUANT_SETS[False, max_rows][0] and m.weights == weights and m.max_rows == max_rows
    for dq, dt in zip(m._packed, t._packed):
        for name in ("qkv", "o", "gate_up", "down"):
            kc, _, sm = m.G1_CFG[name]
            assert isinstance(dq[name], getattr(ops, cls)) and isinstance(dt[name], torch.Tensor)
            assert torch.equal(dt[name], ops.pack_weight(dq[name].dequant(), kc, sm))          # the twin holds the same values at 16 bits
    assert isinstance(m._packed_head, torch.Tensor) and torch.equal(m._packed_head, t._packed_head)          # lm_head is not quantised
    st, tag = m.compress_stats, "q8" if weights == "e4m3" else "q4"
    assert st["matrices"] == st[tag + "_matrices"] == 8 and 0 < st["rel_rms_error"] < (0.05 if tag == "q8" else 0.2)
    assert st["bytes_packed"] == st[tag + "_bytes_packed"] == sum(LS.packed_nbytes(w) for d in m._packed for w in d.values())
    assert st["bytes_packed"] < (0.52 if tag == "q8" else 0.27) * st["bytes_raw"] and t.compress_stats["bytes_packed"] == st["bytes_raw"]
    assert t.compress_stats["rel_rms_error"] == st["rel_rms_error"]


def test_weights_none_packs_the_same_bytes():
    for rows in (64, 128):
        a = _model().enable_fused(ops, gemm="sjd", max_rows=rows)
        b = _model().enable_fused(ops, gemm="sjd", max_rows=rows, weights=None)
        assert a.G1_CFG == b.G1_CFG == LS.LLAMAGEN_SETS[False, rows][0] and b.weights is None
        assert all(torch.equal(x[k], y[k]) for x, y in zip(a._packed, b._packed) for k in x) and torch.equal(a._packed_head, b._packed_head)


def test_refusals_leave_the_model_untouched():
    untouched = lambda m: getattr(m, "_ops", None) is None and not hasattr(m, "_packed") and "max_rows" not in m.__dict__ and "weights" not in m.__dict__
    m = _model()
    with pytest.raises(ValueError, match="'e4m3' or 'e4m3_as_bf16', 'mxfp4' or 'mxfp4_as_bf16'"):
        m.enable_fused(ops, gemm="sjd", weights="int4")
    assert untouched(m)
    h = _model(torch.float16)
    with pytest.raises(ValueError, match="needs bf16 weights"):
        h.enable_fused(ops, gemm="sjd", weights="mxfp4")
    with pytest.raises(ValueError, match="untuned_fp16"):
        m.enable_fused(ops, gemm="sjd", weights="e4m3", max_rows=256, untuned_fp16=True)
    assert untouched(h) and untouched(m)
    for bad, what in ((dict(o=(256, 2, False)), r"3, 4, 6 or 8 column tiles.*G1_CFG\['o'\]"),
                      (dict(down=(192, 4, False)), r"multiples of 128; G1_CFG\['down'\]")):
        m = _model()
        m.G1_CFG = dict(LS.LLAMAGEN_QUANT_SETS[False, 256][0], **bad)
        keep = dict(m.G1_CFG)
        with pytest.raises(ValueError, match=what):
            m.enable_fused(ops, gemm="sjd", weights="mxfp4", max_rows=256)
        assert untouched(m) and m.G1_CFG == keep and "HEAD_CFG" not in m.__dict__
    m.enable_fused(ops, gemm="sjd", weights="e4m3", max_rows=64)                  # (192 is whole e4m3 pairs, and 64 rows take any tile count)
    assert isinstance(m._packed[0]["down"], ops.PackedQ8)
    # dim 192 = 1.5 granules, heads of 64: whole e4m3 pairs, not whole MXFP4 trips
    m = _model(dim=192, n_head=3)
    with pytest.raises(ValueError, match="dim 192 .* multiples of 128"):
        m.enable_fused(ops, gemm="sjd", weights="mxfp4")
    assert untouched(m)
    # a packed backbone stays as it was
    m = _model().enable_fused(ops, gemm="sjd", max_rows=128)
    before = [{k: v.clone() for k, v in d.items()} for d in m._packed]
    m.G1_CFG = dict(LS.LLAMAGEN_SETS[False, 128][0])                               # 320-column chunks: no multiple of 128
    with pytest.raises(ValueError, match="multiples of 128"):
        m.enable_fused(ops, gemm="sjd", weights="mxfp4", max_rows=128)
    assert m.weights is None and m.max_rows == 128 and all(torch.equal(x[k], y[k]) for x, y in zip(before, m._packed) for k in x)


def test_batch_engine_accepts_a_quantised_llamagen_up_to_its_max_rows():
    m = _model().enable_fused(ops, gemm="sjd", weights="mxfp4", max_rows=128)
    assert LS.serves_rows(m, 128, head=True) is None and LS.serves_rows(m, 160, head=True) == ("max_rows", 128)
    with pytest.raises(ValueError, match=r"= 160.*max_rows=256, weights='mxfp4'"):
        SJDBatchEngine(m, 16384, "cpu", 5)
    m64 = _model().enable_fused(ops, gemm="sjd", weights="mxfp4")
    with pytest.raises(ValueError, match=r"at most max_rows=64 rows.*max_rows=128, weights='mxfp4'"):
        SJDBatchEngine(m64, 16384, "cpu", 3)
    e = _model().enable_fused(ops, gemm="sjd", weights="e4m3", max_rows=128)
    with pytest.raises(ValueError, match=r"weights='e4m3', max_rows=256"):
        SJDBatchEngine(e, 16384, "cpu", 5)


def test_quantize_mxfp4_round_trips_an_all_zero_block():
    """GPT-3B's padded wo has 28 zero columns per head: with its 100 real ones they make whole zero blocks of 32 (columns 128 h + 100 .. + 127 hold one)"""
    w = (torch.randn(32, 256, generator=torch.Generator().manual_seed(1)) * 0.05).to(torch.bfloat16)
    w[:, 96:128] = 0
    w[5] = 0
    codes, se = ops.quantize_mxfp4(w)
    assert int(se[0, 3]) == 127 and bool((se[5] == 127).all()) and not codes[:, 48:64].any() and not codes[5].any()
    deq = ops.dequantize_mxfp4(codes, se)
    assert not deq[:, 96:128].any() and not deq[5].any() and torch.equal(deq[:, 96:128].view(torch.int16), w[:, 96:128].view(torch.int16))          # +0.0, bit for bit
    pq = ops.pack_weight_q4(w, 128, True)
    assert torch.equal(pq.dequant().view(torch.int16), deq.view(torch.int16)) and pq.stats["rel_rms_error"] < 0.2
    wo = BB.LlamaGenBackbone._pad_o_weight(w[:, :200].contiguous(), 2, 100, 128)
    assert wo.shape == (32, 256) and torch.equal(ops.pack_weight_q4(wo, 128, False).dequant()[:, 100:128], torch.zeros(32, 28, dtype=torch.bfloat16))
