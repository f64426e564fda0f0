"""CPU: swin-norm (30B-class) backbones on the quantised weight streams -- the launch-shape sets, what enable_fused(swin_quant=True) accepts and
refuses, what it packs, and the predicate of the fused K = 8192 gate|up launch.

The "chunk of 1536 that is not step-major" case runs at the 30B dimensions (one layer on the meta device): at the toy's K = 512 such a chunk is
the whole K, which 33..64 rows stage as it is, so LS.q4_chunk_errors has nothing to refuse there."""
import dataclasses
import inspect

import pytest
import torch

import sjd_amd.backbones as BB
import sjd_amd.launch_shapes as LS
import sjd_amd.ops as ops
import sjd_amd.synthetic as synthetic

NAMES = ("qkv", "o", "gate_up", "down")
TOY = dict(vocab_size=1024, hidden_size=512, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4,
           max_position_embeddings=256, swin_norm=True, model_parallel_size=2)
TOY_CFG = dict(qkv=(256, 4, True), o=(128, 3, False), gate_up=(256, 8, True), down=(128, 2, False))


def _dims(a):
    H, Hkv, hid, inter = a.num_attention_heads, a.num_key_value_heads, a.hidden_size, a.intermediate_size
    D = hid // H
    return dict(qkv=((H + 2 * Hkv) * D, hid), o=(hid, H * D), gate_up=(2 * inter, hid), down=(hid, inter))


def _toy(dtype=torch.bfloat16, cfg=TOY_CFG):
    m = BB.ChameleonBackbone(BB.ChameleonArgs(qk_norm=True, **TOY)).eval()
    synthetic.fill_state_dict(m, seed=3, embed_token_scale=0.25)
    g = torch.Generator().manual_seed(1)
    for layer in m.model.layers:          # gains far from one: a folded gain would show in the packed copy
        layer.input_layernorm.weight.data = 1.0 + 0.5 * torch.randn(TOY["hidden_size"], generator=g)
        layer.post_attention_layernorm.weight.data = 1.0 + 0.5 * torch.randn(TOY["hidden_size"], generator=g)
    m = m.to(dtype)
    if cfg is not None:
        m.G1_CFG = dict(cfg)
    return m


def test_the_two_sets_pass_the_stream_rules_at_30b_dimensions():
    dims = _dims(BB.CHAMELEON_30B)
    assert dims == dict(qkv=(10240, 8192), o=(8192, 8192), gate_up=(44032, 8192), down=(8192, 22016))
    assert LS.q4_chunk_errors(LS.G1_CFG_30B_Q4, dims) == [] and LS.q4_chunk_errors(LS.G1_CFG_30B_Q8, dims) == []
    assert LS.q4_chunk_errors(LS.G1_CFG_30B, dims) == [("o", "halved"), ("down", "halved")]          # (why the uncompressed set is not the start)
    for cfg, granule in ((LS.G1_CFG_30B_Q8, 32), (LS.G1_CFG_30B_Q4, LS.Q4_GRANULE)):
        assert LS.llamagen_quant_errors(cfg, dims, 64, granule=granule) == []
        for name in NAMES:
            KC, tiles, sm = cfg[name]
            K = dims[name][1]
            assert K % granule == 0 and KC % granule == 0 and KC <= LS.CHUNK_CAP_32ROW and 1 <= tiles <= 16
            half = LS.halved_chunk(min(KC, K), K, sm)
            assert half <= LS.CHUNK_CAP_64ROW and half % granule == 0
            for T in (32, 33, 64):
                assert LS.chunk_for_rows(name, cfg[name], T, K, "mxfp4" if granule == 128 else "e4m3") == (KC if T <= 32 or KC <= LS.CHUNK_CAP_64ROW else half)
    # gate|up: the four chunks of 2048 the fused launch streams
    assert LS.G1_CFG_30B_Q4["gate_up"][0] == 2048 and dims["gate_up"][1] // 2048 == 4


def _old_default_shapes(dtype, g1_given, head_given, wide_hidden, gqa, compress, weights, max_rows, vocab_size):
    """default_shapes as it stood before the 30B quantised sets"""
    z = compress and dtype == torch.bfloat16
    head = head_given or (LS.HEAD_CFG_WIDE if vocab_size >= 131072 else None)
    if weights in LS.Q4_WEIGHTS:
        return g1_given or dict(LS.G1_CFG_EMU3_Q4 if gqa else LS.G1_CFG_Q4), head
    if weights is not None:
        wide = (LS.G1_CFG_EMU3_Q8_WIDE if gqa else LS.G1_CFG_Q8_WIDE) if (max_rows or 64) > 64 else None
        return g1_given or dict(wide or (LS.G1_CFG_EMU3_Q8 if gqa else LS.G1_CFG_Q8)), head
    g1 = g1_given or (dict(LS.G1_CFG_30B_Z if z else LS.G1_CFG_30B) if wide_hidden else dict(LS.G1_CFG_EMU3) if gqa else dict(LS.G1_CFG_Z) if z else None)
    return (dict(LS.G1_CFG_EMU3_Z) if z and g1 == LS.G1_CFG_EMU3 else g1), head


def test_default_shapes_hands_the_sets_out_for_wide_hidden_with_weights_and_nothing_else_changes():
    given = dict(qkv=(128, 2, True), o=(128, 2, True), gate_up=(128, 2, True), down=(128, 2, True))
    for dtype in (torch.bfloat16, torch.float16):
        for g1_given in (None, given):
            for wide in (False, True):
                for gqa in (False, True):
                    for compress in (False, True):
                        for weights in (None,) + LS.QUANT_WEIGHTS:
                            for max_rows in (None, 64, 128, 256):
                                for V in (65536, 184622):
                                    args = (dtype, g1_given, None, wide, gqa, compress, weights, max_rows, V)
                                    got = LS.default_shapes(*args)
                                    if wide and weights is not None:
                                        want = g1_given or (LS.G1_CFG_30B_Q4 if weights in LS.Q4_WEIGHTS else LS.G1_CFG_30B_Q8)
                                        assert got == (want, _old_default_shapes(*args)[1]), args
                                    else:
                                        assert got == _old_default_shapes(*args), args
    got, _ = LS.default_shapes(torch.bfloat16, None, None, True, True, True, "mxfp4", None, 65536)
    assert got == LS.G1_CFG_30B_Q4 and got is not LS.G1_CFG_30B_Q4          # a copy: the caller may edit it


@pytest.mark.parametrize("weights", LS.QUANT_WEIGHTS)
def test_toy_swin_backbone_refusals_leave_it_untouched(weights):
    def untouched(m, cfg):
        assert "_packed" not in m.__dict__ and "weights" not in m.__dict__ and m.__dict__.get("G1_CFG") == cfg and "max_rows" not in m.__dict__

    m = _toy()
    with pytest.raises(ValueError, match="is not served for swin-norm backbones"):
        m.enable_fused(ops, gemm="sjd", weights=weights)
    untouched(m, TOY_CFG)
    with pytest.raises(ValueError, match="is not served for swin-norm backbones"):
        m.enable_fused(ops, gemm="sjd", weights=weights, swin_quant=False)
    with pytest.raises(ValueError, match="max_rows"):
        m.enable_fused(ops, gemm="sjd", weights=weights, swin_quant=True, max_rows=128)
    untouched(m, TOY_CFG)
    with pytest.raises(ValueError, match="gemm='sjd'"):
        m.enable_fused(ops, gemm="torch", weights=weights, swin_quant=True)
    bad = dict(TOY_CFG, down=(192, 2, False))          # no multiple of the granule (32 divides it, 128 does not)
    m.G1_CFG = dict(bad)
    if weights in LS.Q4_WEIGHTS:
        with pytest.raises(ValueError, match="multiples of 128"):
            m.enable_fused(ops, gemm="sjd", weights=weights, swin_quant=True)
        untouched(m, bad)
    bad = dict(TOY_CFG, down=(144, 2, False))
    m.G1_CFG = dict(bad)
    with pytest.raises(ValueError, match="multiples of"):
        m.enable_fused(ops, gemm="sjd", weights=weights, swin_quant=True)
    untouched(m, bad)
    f16 = _toy(torch.float16)
    with pytest.raises(ValueError, match="bf16"):
        f16.enable_fused(ops, gemm="sjd", weights=weights, swin_quant=True)
    untouched(f16, TOY_CFG)


@pytest.mark.parametrize("weights", LS.QUANT_WEIGHTS)
def test_a_chunk_of_1536_that_is_not_step_major_is_refused_at_30b_dimensions(weights):
    with torch.device("meta"):
        m = BB.ChameleonBackbone(dataclasses.replace(BB.CHAMELEON_30B, num_hidden_layers=1)).to(torch.bfloat16)
    assert m.args.swin_norm and m.args.model_parallel_size == 4
    m.G1_CFG = dict(LS.G1_CFG_30B)                       # o and down: (1536, 8, False)
    with pytest.raises(ValueError, match=r"33\.\.64 rows.*G1_CFG\['o'\] = \(1536, 8, False\)"):
        m.enable_fused(ops, gemm="sjd", weights=weights, swin_quant=True)
    assert "_packed" not in m.__dict__ and "weights" not in m.__dict__ and m.__dict__["G1_CFG"] == LS.G1_CFG_30B
    with pytest.raises(ValueError, match="is not served for swin-norm backbones"):
        m.enable_fused(ops, gemm="sjd", weights=weights)


@pytest.mark.parametrize("weights", LS.QUANT_WEIGHTS)
def test_toy_swin_backbone_packs_the_checkpoints_own_matrices(weights):
    m = _toy()
    a, mlp = m.model.layers[0].self_attn, m.model.layers[0].mlp
    raw = dict(qkv=torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]).detach().clone(), o=a.o_proj.weight.detach().clone(),
               gate_up=torch.cat([mlp.gate_proj.weight, mlp.up_proj.weight]).detach().clone(), down=mlp.down_proj.weight.detach().clone())
    head = m.lm_head.weight.detach().clone()
    m.enable_fused(ops, gemm="sjd", weights=weights, swin_quant=True)
    assert m.weights == weights and m.max_rows == 64 and m.G1_CFG == TOY_CFG and not m._fold_norm and m._packed_head is None
    assert torch.equal(m.lm_head.weight, head)                                   # lm_head (and with it the prefill) keeps its 16-bit parameters
    q4 = weights in LS.Q4_WEIGHTS
    kind = torch.Tensor if weights.endswith("_as_bf16") else ops.PackedQ4 if q4 else ops.PackedQ8
    st, nbytes = m.compress_stats, 0
    for name in NAMES:
        w = raw[name]
        if q4:
            want = ops.dequantize_mxfp4(*ops.quantize_mxfp4(w))
        else:
            q, scale = ops.quantize_e4m3(w)
            want = (q.view(torch.float8_e4m3fn).float() * scale[:, None]).to(torch.bfloat16)
        pk = m._packed[0][name]
        assert isinstance(pk, kind), (name, type(pk))
        KC, _, sm = TOY_CFG[name]
        if isinstance(pk, torch.Tensor):
            assert torch.equal(pk, ops.pack_weight(want, KC, sm)), name
        else:
            assert (pk.KC, pk.step_major) == (KC, sm) and torch.equal(pk.dequant().view(torch.int16), want.view(torch.int16)), name      # no norm gain in it
            nbytes += pk.nbytes()
            assert pk.nbytes() == (w.numel() * 17 // 32 if q4 else w.numel() + 4 * w.shape[0])
    tag = "q4" if q4 else "q8"
    assert st[tag + "_matrices"] == 4 and st["matrices"] == 4 and 0.0 < st["rel_rms_error"] < (0.2 if q4 else 0.05)
    if not weights.endswith("_as_bf16"):
        assert st[tag + "_bytes_packed"] == nbytes == m.packed_bytes()
    # the row counts the copy serves
    assert LS.serves_rows(m, 64, 32) is None
    if weights != "e4m3_as_bf16":          # (that twin is 16-bit tensors: the uncompressed kernels take more rows, as on the other families)
        assert LS.serves_rows(m, 65, 32) == ("max_rows", 64)


def test_fused_gateup_predicate():
    a = BB.CHAMELEON_30B
    assert LS.gateup_silu_chunked_ok(32, a.intermediate_size, a.hidden_size, 2048) and LS.gateup_silu_chunked_ok(1, 64, 8192, 2048)
    assert ops.gateup_silu_chunked_ok is LS.gateup_silu_chunked_ok
    assert not LS.gateup_silu_chunked_ok(33, 22016, 8192, 2048)
    assert not LS.gateup_silu_chunked_ok(32, 22016, 4096, 2048)
    assert not LS.gateup_silu_chunked_ok(32, 22016, 8192, 1024) and not LS.gateup_silu_chunked_ok(32, 22016, 8192, 4096)
    assert not LS.gateup_silu_chunked_ok(32, 22016 + 32, 8192, 2048)
    assert not LS.gateup_silu_chunked_ok(32, 22016, 8192, 2048, packed_q4=False)          # the e4m3 stream has no such form
    # gateup_silu_ok is what it was: K = 8192 is not one of its shapes
    assert not LS.gateup_silu_ok(32, 22016, 8192, 4096, packed_q8=True) and LS.gateup_silu_ok(32, 11008, 4096, 2048, packed_q8=True)


def test_the_solver_passes_swin_quant_through():
    from sjd_amd.inference_solver import FlexARInferenceSolver
    p = inspect.signature(FlexARInferenceSolver.__init__).parameters
    assert p["swin_quant"].default is False and "swin_quant" in inspect.signature(BB.ChameleonBackbone.enable_fused).parameters
    assert BB.CHAMELEON_30B.swin_norm and BB.CHAMELEON_30B.model_parallel_size == 4 and BB.CHAMELEON_30B.hidden_size == 8192
