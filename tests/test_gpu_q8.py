"""GPU: the window projections streamed from 8-bit (OCP e4m3fn) weights -- kernels G1q / G1sq behind SJD_G1_W8_E4M3 (csrc/sjd_gemm_q8.h),
ops.PackedQ8, ChameleonBackbone.enable_fused(weights="e4m3").  Nothing here has a tolerance: the kernels rebuild the bf16 MFMA operand
q * scale bit for bit, so every result is compared BIT FOR BIT with the uncompressed kernels (G1 / G1s) run on PackedQ8.dequant().  All the
loss of the format is in ops.quantize_e4m3 (tests/test_q8_pack.py, CPU)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

W8 = 0x2000          # SJD_G1_W8_E4M3
UNSUPPORTED = -2


@pytest.fixture(scope="module")
def dev():
    from tests.conftest import poison_device_memory
    poison_device_memory(total_gib=1)          # the planes come from torch.empty: an unwritten element must not read as zero
    return "cuda:0"


def q8_weight(N, K, seed, dev):
    """seeded Gaussian columns whose magnitudes span 2^-20 .. 2^3 (scale exponents differ within one 32-column tile), a zero column, both
    +-448 codes, e4m3 denormals and a -0.0"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-20, 4, (N, 1), generator=g).float())
    w[1] = torch.randn(K, generator=g).clamp(-3, 3) * 0.25
    w[1, 0], w[1, 1] = 1.75, -1.75                               # 448 * 2^-8: the largest codes, both signs
    w[1, 2], w[1, 3], w[1, 9] = 3 * 2.0 ** -17, -2.0 ** -17, 7 * 2.0 ** -17       # denormal codes 3, -1, 7 at scale 2^-8
    w[2, 0] = -0.0
    w[3] = 0.0
    return w.to(torch.bfloat16).to(dev)


def check_codes(pq):
    q = pq.codes()
    mag = q & 0x7F
    assert bool((q == 0x7E).any()) and bool((q == 0xFE).any())              # +-448
    assert bool(((mag > 0) & (mag < 8)).any())                              # denormals
    assert bool((q == 0x80).any())                                          # -0.0
    assert not bool((mag == 0x7F).any())                                    # never NaN
    s = pq.scales()
    assert bool((s[3] == 1.0)) and len(set(s[:32].tolist())) > 4            # the zero column; many scales inside one tile


G1Q_CASES = [(1, 32, 16, 16, 1, False),              # one record (a half record: one k-step)
             (9, 96, 48, 32, 4, False),              # a workgroup with a missing tile; a ragged last chunk of one step
             (32, 96, 48, 16, 3, False),
             (32, 1024, 528, 128, 2, False),         # 33 steps: the last chunk is a lone half record
             (5, 512, 1024, 256, 4, True),
             (33, 256, 512, 256, 8, True), (64, 512, 1280, 1280, 8, True),      # two row tiles, at the LDS limit
             (32, 512, 2560, 2560, 8, True),         # one row tile at its limit
             (17, 64, 80, 48, 2, True), (40, 96, 176, 112, 12, False)]          # odd units: 3 + 2 steps step-major; 7 + 4 steps, 12 waves, two row tiles


@pytest.mark.parametrize("M,N,K,KC,waves,step_major", G1Q_CASES)
def test_g1q_planes_are_g1_on_the_dequantised_weight(dev, M, N, K, KC, waves, step_major):
    import sjd_amd.ops as ops
    w = q8_weight(N, K, N + K + M, dev)
    pq = ops.pack_weight_q8(w, KC, step_major)
    check_codes(pq)
    assert torch.equal(ops.quantize_e4m3(w)[0].cpu(), ops.quantize_e4m3(w.cpu())[0])          # the quantiser gives the same codes on either device
    deq = pq.dequant()
    assert torch.equal(deq.float(), pq.codes().view(torch.float8_e4m3fn).float() * pq.scales()[:, None])
    wp = ops.pack_weight(deq, KC, step_major)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16).to(dev)
    ref = ops.skinny_gemm(x, wp, N, K, KC, waves, step_major).data
    got = ops.skinny_gemm(x, pq, N, K, KC, waves, step_major).data
    torch.cuda.synchronize()
    assert got.shape == ref.shape == ((K + KC - 1) // KC, 32 * ((M + 31) // 32), N)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (got - ref).abs().max()
    assert float(ref.abs().max()) > 0
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.skinny_gemm(x, pq, N, K, KC, waves, step_major)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        cap = ops.skinny_gemm(x, pq, N, K, KC, waves, step_major).data
    cap.fill_(float("nan"))
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap.view(torch.int32), ref.view(torch.int32))


def test_g1q_column_window(dev):
    import sjd_amd.ops as ops
    M, NP, K, KC, c0, nc = 32, 512, 512, 256, 64, 352
    w = q8_weight(NP, K, 77, dev)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(dev)
    for sm in (True, False):
        pq = ops.pack_weight_q8(w, KC, sm)
        full = ops.skinny_gemm(x, pq, NP, K, KC, 8, sm).data
        ref = ops.skinny_gemm_cols(x, ops.pack_weight(pq.dequant(), KC, sm), NP, K, KC, c0, nc, 8, sm).data
        got = ops.skinny_gemm_cols(x, pq, NP, K, KC, c0, nc, 8, sm).data          # (the scales still sit at byte N_packed * K)
        torch.cuda.synchronize()
        assert got.shape == (2, 32, nc) and torch.equal(got.view(torch.int32), full[:, :, c0:c0 + nc].contiguous().view(torch.int32))
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


@pytest.mark.parametrize("step_major", [False, True])
@pytest.mark.parametrize("with_norm", [True, False])
@pytest.mark.parametrize("M,I,K", [(9, 64, 512), (32, 128, 1024), (17, 192, 2048), (32, 64, 4096)])
def test_g1sq_is_g1s_on_the_dequantised_weight(dev, M, I, K, with_norm, step_major):
    import sjd_amd.ops as ops
    w = q8_weight(2 * I, K, I + K + M, dev)
    pq = ops.pack_weight_q8(w, K // 2, step_major, gateup=True)
    check_codes(pq)
    wp = ops.pack_weight(pq.dequant(), K // 2, step_major)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M + 1)).to(torch.bfloat16).to(dev)
    assert ops.gateup_silu_ok(M, I, K, K // 2, packed_q8=True)
    rn = (ops.residual_sumsq(x.clone(), None), K, 1e-5) if with_norm else None
    ref = ops.gateup_silu(x, wp, I, K, step_major, row_norm=rn)
    got = ops.gateup_silu(x, pq, I, K, step_major, row_norm=rn)
    unfused = ops.silu_mul(ops.skinny_gemm(x, pq, 2 * I, K, K // 2, 8, step_major), rows=M, dtype=x.dtype, row_norm=rn)        # G1q + F3
    torch.cuda.synchronize()
    assert got.shape == (M, I) and got.dtype == torch.bfloat16
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (got.float() - ref.float()).abs().max()
    assert torch.equal(unfused.view(torch.int16), ref.view(torch.int16))
    assert float(ref.float().abs().max()) > 0


def test_c_boundary_refusals(dev):
    """with the bit set, what G1q / G1sq do not serve comes back as SJD_ERR_UNSUPPORTED before any launch"""
    import sjd_amd._lib as L
    lib = L.load()
    assert L.G1_W8_E4M3 == W8
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    # sjd_skinny_gemm(x, w_packed, out, M, N, K, KC, waves, step_major, dtype, stream)
    assert lib.sjd_skinny_gemm(p, p, p, 65, 32, 64, 64, 1, 0, L.DTYPE_BF16 | W8, None) == UNSUPPORTED            # more than 64 rows
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 64, 64, 1, 0, L.DTYPE_F16 | W8, None) == UNSUPPORTED             # fp16
    assert lib.sjd_skinny_gemm(p, p, p, 40, 32, 1296, 1296, 1, 0, L.DTYPE_BF16 | W8, None) == UNSUPPORTED        # 81 k-steps x two row tiles > 160 KiB
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 2576, 2576, 1, 0, L.DTYPE_BF16 | W8, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm_cols(p, p, p, 65, 32, 64, 64, 1, 0, L.DTYPE_BF16 | W8, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm_cols(p, p, p, 32, 32, 64, 64, 1, 0, L.DTYPE_F16 | W8, 64, 0, None) == UNSUPPORTED
    # sjd_gateup_silu(x, w_packed, y, M, I, K, step_major, dtype, row_norm, stream)
    assert lib.sjd_gateup_silu(p, p, p, 33, 64, 1024, 0, L.DTYPE_BF16 | W8, None, None) == UNSUPPORTED           # G1sq: 32 rows
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, 1024, 0, L.DTYPE_F16 | W8, None, None) == UNSUPPORTED
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, 768, 0, L.DTYPE_BF16 | W8, None, None) == UNSUPPORTED
    # an entry point that does not know the bit: sjd_silu_mul(gate_up, y, rows, inter, dtype, part, n_chunks, stream)
    assert lib.sjd_silu_mul(p, p, 8, 64, L.DTYPE_BF16 | W8, None, 0, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


TOY = dict(vocab_size=9216, hidden_size=512, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, max_position_embeddings=512,
           rms_norm_eps=1e-5, rope_theta=10000.0)


def _decode(dev, kv_heads, weights, g1_cfg, img_len=48, window=16, P=10, seed=5):
    """48 image tokens through SJDEngine (window 16, CFG: 32 rows per forward) on the toy backbone of tests/gpu_loop_check.py"""
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    from sjd_amd.engine import SJDEngine, SJDConfig, WindowSpec
    from sjd_amd.grammar import AnoleGrammar
    from tests.helpers import make_chameleon
    V = TOY["vocab_size"]
    model = make_chameleon(dict(TOY, num_key_value_heads=kv_heads), 29, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=dev)
    if g1_cfg is not None:
        model.G1_CFG = dict(g1_cfg)
    model.enable_fused(ops, gemm="sjd", weights=weights)
    prompt = torch.cat([synthetic.synthetic_prompt(P - 1, seed, lo=8900, hi=9200), torch.tensor([[8197]])], dim=1)
    max_len = P + img_len + 1
    model.setup_cache(batch=2, s_max=((max_len + 64 + 31) // 32) * 32)
    cfg = SJDConfig(jacobi_loop_interval_l=0, jacobi_loop_interval_r=img_len - window - 2, max_num_new_tokens=window, guidance_scale=3.0,
                    seed=seed, prefix_token_sampler_scheme="speculative_jacobi", max_length=max_len, eos_token_ids=(8196,))
    spec = WindowSpec(first_tokens=prompt.to(dev).repeat(2, 1),
                      first_positions=torch.stack([torch.arange(P), torch.tensor([1] * (P - 1) + [0])]).to(dev),
                      key_start=torch.tensor([0, P - 1], dtype=torch.int32), pos_offset=torch.tensor([0, -(P - 1)], dtype=torch.long), kv_base=0)
    eng = SJDEngine(model, V, dev, max_window=window, use_graph=True)
    seq, stats = eng.decode(prompt[0].tolist(), spec, AnoleGrammar(V, P, max_len, img_len), cfg)
    torch.cuda.synchronize()
    return model, seq[P:], list(stats.matched), eng.probs.clone()


# MHA: the architecture's own set (G1_CFG_Q8: at hidden 512 its gate|up chunk is the whole K, so G1q + F3) and one that packs gate|up in two
# K halves (G1sq); GQA: G1_CFG_EMU3_Q8
@pytest.mark.parametrize("kv_heads,g1_cfg", [(4, None), (4, dict(qkv=(256, 4, True), o=(176, 3, False), gate_up=(256, 8, True), down=(128, 2, False))),
                                              (2, None)])
def test_end_to_end_tokens_agree_with_the_bf16_twin(dev, kv_heads, g1_cfg):
    import sjd_amd.ops as ops
    m8, tok8, acc8, probs8 = _decode(dev, kv_heads, "e4m3", g1_cfg)
    m16, tok16, acc16, probs16 = _decode(dev, kv_heads, "e4m3_as_bf16", g1_cfg)
    assert len(tok8) >= 48 and tok8 == tok16
    assert acc8 == acc16 and len(acc8) > 1
    assert torch.equal(probs8.view(torch.int32), probs16.view(torch.int32)) and float(probs8.sum()) > 0
    assert all(isinstance(w, ops.PackedQ8) for d in m8._packed for w in d.values())
    assert not isinstance(m8._packed_head, ops.PackedQ8) and not any(isinstance(w, ops.PackedQ8) for d in m16._packed for w in d.values())
    if g1_cfg is None:
        assert m8.G1_CFG == (m8.G1_CFG_EMU3_Q8 if kv_heads != 4 else m8.G1_CFG_Q8) == m16.G1_CFG
    assert m8.packed_bytes(head=False) <= 0.52 * m16.packed_bytes(head=False)          # one byte per weight + 4 / K for the scales, against two
    assert m8.packed_bytes() - m8.packed_bytes(head=False) == m16.packed_bytes() - m16.packed_bytes(head=False) > 0      # the head is not quantised
    st = m8.compress_stats
    assert st["q8_matrices"] == 8 and st["q8_bytes_packed"] == m8.packed_bytes(head=False) and 0 < st["rel_rms_error"] < 2.0 ** -4
    assert m16.compress_stats["rel_rms_error"] == st["rel_rms_error"] and "q8_bytes_packed" not in m16.compress_stats


@pytest.fixture(scope="module", params=[True, False], ids=["folded", "unfolded"])
def real_size_pair(dev, request):
    """(both window forwards: the folded-norm one and _forward_window_g1)  one Lumina-sized layer (hidden 4096, 32 heads of 128; intermediate 2048) with the architecture's own G1_CFG_Q8, packed as "e4m3" and as its bf16 twin"""
    import sjd_amd.backbones as BB
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    args = BB.ChameleonArgs(vocab_size=9216, hidden_size=4096, intermediate_size=2048, num_hidden_layers=1, num_attention_heads=32,
                            num_key_value_heads=32, max_position_embeddings=512)
    out = []
    for wt in ("e4m3", "e4m3_as_bf16"):
        with torch.device(dev):
            m = BB.ChameleonBackbone(args, attn=ops.HipWindowAttention(n_split=2)).to(torch.bfloat16).eval()
        synthetic.fill_state_dict_device(m, seed=7, embed_token_scale=0.25)
        m.enable_fused(ops, gemm="sjd", weights=wt, fold_norm=request.param)
        assert m._fold_norm == request.param and m.G1_CFG == m.G1_CFG_Q8 and m.G1_CFG["gate_up"] == (2048, 8, True)
        m.setup_cache(batch=2, s_max=64)
        out.append(m)
    return out


# 32 rows: gate|up is the fused G1sq launch over its two K halves of 2048; 40 and 64 rows (a draft window of 32 with CFG, or the prefill of a
# 17..32-token prompt): G1q stages at most 1280 columns for two row tiles, so the same step-major packing is read in chunks of 1024 (+ F3)
@pytest.mark.parametrize("n", [16, 20, 32])
def test_real_size_window_of_up_to_64_rows(dev, real_size_pair, n):
    import sjd_amd.ops as ops
    m8, m16 = real_size_pair
    assert isinstance(m8._packed[0]["gate_up"], ops.PackedQ8) and m8._packed[0]["gate_up"].KC == 2048
    assert m8._q8_chunk("gate_up", 2 * n, 4096) == (2048 if n == 16 else 1024) == m16._q8_chunk("gate_up", 2 * n, 4096)
    assert m8._q8_chunk("qkv", 2 * n, 4096) == 1024 and m8._q8_chunk("down", 2 * n, 2048) == 768
    g = torch.Generator().manual_seed(n)
    tok = torch.randint(4, 8196, (2, n), generator=g).to(dev)
    pos = torch.arange(n)[None].repeat(2, 1).to(dev)
    ks = torch.zeros(2, dtype=torch.int32, device=dev)
    outs = []
    with torch.no_grad():
        for m in (m8, m16):
            outs.append(m.forward_window(tok, pos, 0, ks).float())
    torch.cuda.synchronize()
    assert outs[0].shape == (2, n, 9216) and bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_chunks_the_8bit_kernel_cannot_stage_are_refused_before_any_launch(dev):
    import sjd_amd.ops as ops
    from tests.helpers import make_chameleon
    mk = lambda: make_chameleon(dict(TOY, num_key_value_heads=4, hidden_size=4096, num_attention_heads=32, num_hidden_layers=1), 29, 0.25,
                                ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=dev)
    m = mk()
    m.G1_CFG = dict(m.G1_CFG_Q8, qkv=(4096, 8, True))
    with pytest.raises(ValueError, match="<= 2560"):
        m.enable_fused(ops, gemm="sjd", weights="e4m3")
    assert getattr(m, "weights", None) is None and getattr(m, "_ops", None) is None          # a refused call leaves the backbone as it was
    m = mk()
    m.G1_CFG = dict(m.G1_CFG_Q8, gate_up=(2048, 8, False))          # tile-major: halved chunks cannot read it
    m.enable_fused(ops, gemm="sjd", weights="e4m3")
    m.setup_cache(batch=2, s_max=64)
    z = lambda n: (torch.zeros(2, n, dtype=torch.long, device=dev), torch.zeros(2, n, dtype=torch.long, device=dev), 0, torch.zeros(2, dtype=torch.int32, device=dev))
    with torch.no_grad():
        assert m.forward_window(*z(16)).shape == (2, 16, 9216)          # 32 rows: served (G1sq)
        with pytest.raises(ValueError, match="<= 1280"):
            m.forward_window(*z(20))


def test_python_refusals(dev):
    import sjd_amd.backbones as BB
    import sjd_amd.ops as ops
    from sjd_amd.engine_batch import SJDBatchEngine
    from tests.helpers import make_chameleon
    conf = dict(TOY, num_key_value_heads=4)
    mk = lambda dtype=torch.bfloat16: make_chameleon(conf, 29, 0.25, ops.HipWindowAttention(n_split=2), dtype=dtype, device=dev)
    with pytest.raises(ValueError, match="fp16|float16"):
        mk(torch.float16).enable_fused(ops, gemm="sjd", weights="e4m3")
    with pytest.raises(ValueError, match="gemm='sjd'"):
        mk().enable_fused(ops, gemm="torch", weights="e4m3")
    with pytest.raises(ValueError, match="'e4m3'"):
        mk().enable_fused(ops, gemm="sjd", weights="int8")
    swin = BB.ChameleonBackbone(BB.ChameleonArgs(vocab_size=9216, hidden_size=512, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4,
                                                 num_key_value_heads=4, max_position_embeddings=512, swin_norm=True),
                                attn=ops.HipWindowAttention(n_split=2)).to(device=dev, dtype=torch.bfloat16)
    for wt in ("e4m3", "e4m3_as_bf16"):
        with pytest.raises(ValueError, match="swin-norm"):
            swin.enable_fused(ops, gemm="sjd", weights=wt)
    m = mk().enable_fused(ops, gemm="sjd", weights="e4m3")
    with pytest.raises(ValueError, match="one prompt per forward"):
        SJDBatchEngine(m, 9216, dev, n_prompts=2)
    m.setup_cache(batch=8, s_max=64)
    with pytest.raises(ValueError, match="at most 64 rows"):          # and the backbone itself refuses a taller window
        m.forward_window(torch.zeros(8, 16, dtype=torch.long, device=dev), torch.zeros(8, 16, dtype=torch.long, device=dev), 0,
                         torch.zeros(8, dtype=torch.int32, device=dev))
    # weights=None is what it was: the 12-bit stream by default
    d = mk().enable_fused(ops, gemm="sjd")
    assert d.weights is None and isinstance(d._packed[0]["qkv"], ops.PackedZ) and "q8_matrices" not in d.compress_stats
