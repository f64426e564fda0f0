"""CPU: enable_fused(..., release_16bit=True) on ChameleonBackbone -- what it accepts and refuses, what it releases, and that nothing moves without it.
(enable_fused packs on the CPU; the kernels are tests/test_gpu_prefill_quant.py's.)"""
import inspect
import os
import re

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
SWIN = dict(swin_norm=True, model_parallel_size=2)


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


def _untouched(m, before):
    assert "_packed" not in m.__dict__ and "weights" not in m.__dict__ and "_ops" not in m.__dict__ and m.__dict__.get("G1_CFG") == TOY_CFG
    assert m.released_16bit is False and "compress_stats" not in m.__dict__
    assert all(torch.equal(p, q) for p, q in zip(_projections(m), before))


@pytest.mark.parametrize("swin", [False, True])
@pytest.mark.parametrize("weights", LS.QUANT_WEIGHTS)
def test_release_is_accepted_with_each_weights_value_and_releases_the_layer_matrices(weights, swin):
    m = _toy(**(SWIN if swin else {}))
    want = sum(p.numel() * p.element_size() for p in _projections(m))
    kept = {k: v.detach().clone() for k, v in m.state_dict().items() if "_proj" not in k}
    assert want == 2 * 2 * (4 * 256 * 256 + 3 * 256 * 512)
    assert m.enable_fused(ops, gemm="sjd", weights=weights, release_16bit=True, swin_quant=swin) is m
    assert m.released_16bit is True and m.weights == weights and m.compress_stats["bytes_released"] == want
    assert all(p.numel() == 0 for p in _projections(m)) and not hasattr(m, "_fused")
    kind = torch.Tensor if weights.endswith("_as_bf16") else ops.PackedQ4 if weights in LS.Q4_WEIGHTS else ops.PackedQ8
    assert len(m._packed) == 2 and all(isinstance(w, kind) for d in m._packed for w in d.values())
    # what stays: the embedding, every norm, the QK-norm gains and lm_head
    now = dict(m.named_parameters())
    assert set(kept) <= set(now) and all(torch.equal(now[k], v) for k, v in kept.items())
    assert any("q_norm" in k for k in kept) and "lm_head.weight" in kept and "model.embed_tokens.weight" in kept
    # what a released backbone refuses, each by name
    with pytest.raises(ValueError, match="release_16bit=True"):
        m.enable_fused(ops, gemm="sjd", weights=weights, swin_quant=swin)
    with pytest.raises(ValueError, match="state_dict"):
        m.state_dict()
    m._ops = None
    tok = torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ValueError, match="un-fused forward"):
        m.forward_window(tok, tok, 0, torch.zeros(2, dtype=torch.int32))


def test_release_is_refused_before_anything_is_assigned():
    m = _toy()
    before = [p.detach().clone() for p in _projections(m)]
    with pytest.raises(ValueError, match="12-bit stream has no G1p form"):
        m.enable_fused(ops, gemm="sjd", release_16bit=True)
    _untouched(m, before)
    with pytest.raises(ValueError, match="12-bit stream has no G1p form"):
        m.enable_fused(ops, gemm="sjd", compress=True, release_16bit=True)
    _untouched(m, before)
    for gemm in ("torch", "hipblaslt"):
        with pytest.raises(ValueError, match="gemm='sjd'"):
            m.enable_fused(ops, gemm=gemm, weights="e4m3", release_16bit=True)
        _untouched(m, before)
    f16 = _toy(torch.float16)
    b16 = [p.detach().clone() for p in _projections(f16)]
    for weights in LS.QUANT_WEIGHTS:
        with pytest.raises(ValueError, match="bf16"):
            f16.enable_fused(ops, gemm="sjd", weights=weights, release_16bit=True)
        _untouched(f16, b16)
    # G1p reads whole record pairs: an e4m3 chunk of 144 packs without release_16bit and is refused with it
    odd = _toy(cfg=dict(TOY_CFG, down=(144, 4, False)))
    with pytest.raises(ValueError, match="multiples of 32"):
        odd.enable_fused(ops, gemm="sjd", weights="e4m3", release_16bit=True)
    assert "_packed" not in odd.__dict__ and all(p.numel() > 0 for p in _projections(odd))
    odd.enable_fused(ops, gemm="sjd", weights="e4m3")
    assert odd.released_16bit is False


@pytest.mark.parametrize("weights", [None, "e4m3", "mxfp4_as_bf16"])
def test_defaults_are_unchanged(weights):
    p = inspect.signature(BB.ChameleonBackbone.enable_fused).parameters
    assert p["release_16bit"].default is False and "release_16bit" not in inspect.signature(BB.LlamaGenBackbone.enable_fused).parameters
    m = _toy()
    before = [q.detach().clone() for q in _projections(m)]
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.enable_fused(ops, gemm="sjd", weights=weights)
    assert m.released_16bit is False and "bytes_released" not in m.compress_stats and len(m._fused) == 2
    assert all(torch.equal(a, b) for a, b in zip(_projections(m), before))
    after = m.state_dict()
    assert set(after) == set(sd) and all(torch.equal(after[k], sd[k]) for k in sd)
    m.enable_fused(ops, gemm="sjd", weights=weights)          # an unreleased backbone packs again, as before


def test_serves_rows_is_unchanged_for_unreleased_backbones():
    for weights, want65 in (("mxfp4", ("max_rows", 64)), ("mxfp4_as_bf16", ("max_rows", 64)), ("e4m3", ("max_rows", 64)), ("e4m3_as_bf16", None)):
        for release in (False, True):          # (the label does not move: a released backbone routes "prefill" and "max_rows" above 64 rows to G1p)
            m = _toy().enable_fused(ops, gemm="sjd", weights=weights, release_16bit=release)
            assert LS.serves_rows(m, 32, 16) is None and LS.serves_rows(m, 64, 32) is None
            assert LS.serves_rows(m, 65, 32) == want65
            assert LS.serves_rows(m, 80, 40) == ("prefill", None) and LS.serves_rows(m, 300, 150) == ("prefill", None)
    plain = _toy().enable_fused(ops, gemm="sjd")
    assert LS.serves_rows(plain, 64, 32) is None and LS.serves_rows(plain, 80, 40) == ("prefill", None)


def test_the_export_the_constant_and_the_pass_through():
    assert "sjd_prefill_gemm" in L.EXPORTS and len(L.EXPORTS) <= 45 and len(set(L.EXPORTS)) == len(L.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "sjd_hip.h")).read()
    assert re.search(r"^int sjd_prefill_gemm\(", hdr, re.M)
    src = open(os.path.join(ROOT, "accelerating-t2i-ar-with-sjd_amd", "csrc", "sjd_gemm_prefill.h")).read()
    assert int(re.search(r"constexpr int G1P_ROWS = (\d+);", src).group(1)) == LS.PREFILL_ROW_BLOCK and LS.PREFILL_ROW_BLOCK % 32 == 0
    assert list(inspect.signature(ops.prefill_gemm).parameters)[:5] == ["x", "w_packed", "N", "K", "row_scale"]
    from sjd_amd.inference_solver import FlexARInferenceSolver
    import model_wrappers.model_loader as ML
    assert inspect.signature(FlexARInferenceSolver.__init__).parameters["release_16bit"].default is False
    for fn in (ML.load_lumina_mgpt, ML.load_anole, ML.load_emu3):
        assert inspect.signature(fn).parameters["release_16bit"].default is False
