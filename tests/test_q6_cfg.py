"""CPU: what goes with ChameleonBackbone.enable_fused(weights="e2m3" / "e2m3_as_bf16") outside the kernels -- every refusal leaves the backbone as it
was, the launch shapes are the MXFP4 sets, the tuples existing tests parametrise over have not grown, compress_stats carries the q6 keys, and the names
pass through the solver and the loaders."""
import inspect
import os

import pytest
import torch

import sjd_amd._lib as L
import sjd_amd.backbones as BB
import sjd_amd.launch_shapes as LS
import sjd_amd.ops as ops
import sjd_amd.synthetic as synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = dict(vocab_size=1024, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
           max_position_embeddings=256)
TOY_CFG = dict(qkv=(128, 4, True), o=(256, 3, False), gate_up=(128, 8, True), down=(256, 4, False))


def _toy(dtype=torch.bfloat16, cfg=TOY_CFG, **kw):
    m = BB.ChameleonBackbone(BB.ChameleonArgs(qk_norm=True, **dict(TOY, **kw))).eval()
    synthetic.fill_state_dict(m, seed=3, embed_token_scale=0.25)
    m = m.to(dtype)
    m.G1_CFG = dict(cfg)
    return m


def _projections(m):
    for b in m.model.layers:
        a, mlp = b.self_attn, b.mlp
        yield from (a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, a.o_proj.weight, mlp.gate_proj.weight, mlp.up_proj.weight, mlp.down_proj.weight)


def _refused(m, match, cfg=TOY_CFG, **kw):
    before = [p.detach().clone() for p in _projections(m)]
    with pytest.raises(ValueError, match=match):
        m.enable_fused(ops, **kw)
    assert "_packed" not in m.__dict__ and "weights" not in m.__dict__ and "_ops" not in m.__dict__ and m.__dict__.get("G1_CFG") == cfg
    assert m.released_16bit is False and "compress_stats" not in m.__dict__ and "max_rows" not in m.__dict__
    assert all(torch.equal(p, q) for p, q in zip(_projections(m), before))


@pytest.mark.parametrize("weights", LS.Q6_WEIGHTS)
def test_every_refusal_leaves_the_backbone_unassigned(weights):
    _refused(_toy(torch.float16), "bf16", gemm="sjd", weights=weights)
    for gemm in ("torch", "hipblaslt"):
        _refused(_toy(), "gemm='sjd'", gemm=gemm, weights=weights)
    for rows in (32, 128, 256):
        _refused(_toy(), "max_rows is None or 64", gemm="sjd", weights=weights, max_rows=rows)
    for swin in (dict(swin_norm=True), dict(model_parallel_size=2), dict(swin_norm=True, model_parallel_size=2)):
        for sq in (False, True):
            _refused(_toy(**swin), "swin-norm", gemm="sjd", weights=weights, swin_quant=sq)
    _refused(_toy(), "release_16bit", gemm="sjd", weights=weights, release_16bit=True)
    odd = dict(TOY_CFG, down=(192, 4, False))           # a chunk that is no multiple of the granule
    _refused(_toy(cfg=odd), "multiples of 128", cfg=odd, gemm="sjd", weights=weights)
    _refused(_toy(intermediate_size=448), "multiples of 128", gemm="sjd", weights=weights)          # the down projection's K = 448
    big = dict(TOY_CFG, qkv=(2688, 4, True))
    _refused(_toy(cfg=big), "<= 2560", cfg=big, gemm="sjd", weights=weights)


def test_the_unknown_name_message_keeps_its_text_and_names_the_new_values():
    with pytest.raises(ValueError) as e:
        _toy().enable_fused(ops, gemm="sjd", weights="int6")
    assert "None, 'e4m3' or 'e4m3_as_bf16', 'mxfp4' or 'mxfp4_as_bf16'" in str(e.value) and "'e2m3' or 'e2m3_as_bf16'" in str(e.value)


def test_the_tuples_existing_tests_parametrise_over_have_not_grown():
    assert LS.Q6_WEIGHTS == ("e2m3", "e2m3_as_bf16") and LS.Q6_MAX_ROWS == 64
    assert LS.Q4_WEIGHTS == ("mxfp4", "mxfp4_as_bf16")
    assert LS.QUANT_WEIGHTS == ("e4m3", "e4m3_as_bf16", "mxfp4", "mxfp4_as_bf16")
    assert L.G1_W6_E2M3 == 0x8000 and L.G1_W6_E2M3 not in (L.G1_W8_E4M3, L.G1_W4_MXFP4) and len(L.EXPORTS) <= 45
    hdr = open(os.path.join(ROOT, "include", "sjd_hip.h")).read()
    assert "#define SJD_G1_W6_E2M3 0x8000\n" in hdr


@pytest.mark.parametrize("weights", LS.Q6_WEIGHTS)
def test_default_shapes_are_the_mxfp4_sets(weights):
    for gqa, want in ((False, LS.G1_CFG_Q4), (True, LS.G1_CFG_EMU3_Q4)):
        for rows in (None, 64):
            g1, head = LS.default_shapes(torch.bfloat16, None, None, False, gqa, True, weights, rows, 65536)
            assert g1 == want and g1 is not want and head is None
    given = dict(TOY_CFG)
    assert LS.default_shapes(torch.bfloat16, given, None, False, False, True, weights, None, 65536)[0] is given
    for name, dims in ((LS.G1_CFG_Q4, LS.chameleon_dims(4096, 32, 32, 128, 11008)), (LS.G1_CFG_EMU3_Q4, LS.chameleon_dims(4096, 32, 8, 128, 14336))):
        assert LS.quant_copy_errors(name, dims, LS.Q6_MAX_ROWS, LS.Q4_GRANULE) == []
        for proj, shape in name.items():
            for T in (32, 33, 64):
                assert LS.chunk_for_rows(proj, shape, T, dims[proj][1], weights, 64) == LS.chunk_for_rows(proj, shape, T, dims[proj][1], "mxfp4", 64)


def test_packing_stats_and_row_limits():
    m6 = _toy().enable_fused(ops, gemm="sjd", weights="e2m3")
    m16 = _toy().enable_fused(ops, gemm="sjd", weights="e2m3_as_bf16", max_rows=64)
    assert m6.weights == "e2m3" and m6.max_rows == 64 and m6.G1_CFG == TOY_CFG and m6.released_16bit is False
    assert all(isinstance(w, ops.PackedQ6) for d in m6._packed for w in d.values()) and not isinstance(m6._packed_head, ops.PackedQ6)
    assert all(isinstance(w, torch.Tensor) for d in m16._packed for w in d.values())
    n_w = 2 * (4 * 256 * 256 + 3 * 256 * 512)
    st = m6.compress_stats
    assert st["q6_matrices"] == 8 and st["q6_bytes_packed"] == m6.packed_bytes(head=False) == n_w * 3 // 4 + n_w // 32          # 6.25 bits per weight
    assert 2.0 ** -7 < st["rel_rms_error"] < 0.04 and "q4_matrices" not in st and "q8_matrices" not in st
    st16 = m16.compress_stats
    assert st16["q6_matrices"] == 8 and st16["rel_rms_error"] == st["rel_rms_error"] and "q6_bytes_packed" not in st16
    assert m16.packed_bytes(head=False) == 2 * n_w
    for li in range(2):          # the twin holds pack_weight(dequant()) on the same chunks
        for name, (kc, _, sm) in TOY_CFG.items():
            assert torch.equal(m16._packed[li][name], ops.pack_weight(m6._packed[li][name].dequant(), kc, sm))
    for m in (m6, m16):
        assert LS.serves_rows(m, 32, 16) is None and LS.serves_rows(m, 64, 32) is None
        assert LS.serves_rows(m, 65, 32) == ("max_rows", 64) == LS.serves_rows(m, 256, 32)
        assert LS.serves_rows(m, 80, 40) == ("prefill", None)
        tok = torch.zeros(8, 16, dtype=torch.long)
        with pytest.raises(ValueError, match="at most 64 rows"):          # before the first launch
            m.forward_window(tok, tok, 0, torch.zeros(8, dtype=torch.int32))


def test_llamagen_keeps_refusing_and_the_names_pass_through():
    lg = BB.LlamaGenBackbone(BB.LlamaGenArgs(dim=256, n_layer=1, n_head=4, vocab_size=64, cls_token_num=4, block_size=16)).to(torch.bfloat16)
    for weights in LS.Q6_WEIGHTS:
        with pytest.raises(ValueError, match="'mxfp4' or 'mxfp4_as_bf16'"):
            lg.enable_fused(ops, gemm="sjd", weights=weights)
    from sjd_amd.inference_solver import FlexARInferenceSolver
    import model_wrappers.model_loader as ML
    assert inspect.signature(FlexARInferenceSolver.__init__).parameters["weights"].default is None
    for fn in (ML.load_lumina_mgpt, ML.load_anole, ML.load_emu3):
        assert inspect.signature(fn).parameters["weights"].default is None
