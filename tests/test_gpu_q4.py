"""GPU: the window projections streamed from OCP MXFP4 weights -- kernels G1q4 / G1sq4 behind SJD_G1_W4_MXFP4 (csrc/sjd_gemm_q4.h), ops.PackedQ4,
ChameleonBackbone.enable_fused(weights="mxfp4").  Nothing here has a tolerance: the kernels rebuild the bf16 MFMA operand code * scale bit for bit,
so every result is compared BIT FOR BIT with the uncompressed kernels (G1 / G1s) run on PackedQ4.dequant().  All the loss of the format is in
ops.quantize_mxfp4 (tests/test_q4_pack.py, CPU).  G = 128 is the format's K granule."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

W4, W8 = 0x4000, 0x2000          # SJD_G1_W4_MXFP4, SJD_G1_W8_E4M3
UNSUPPORTED, BAD_ARG = -2, -1
G = 128


@pytest.fixture(scope="module")
def dev():
    from tests.conftest import poison_device_memory
    poison_device_memory(total_gib=1)          # the planes come from torch.empty: an unwritten element must not read as zero
    return "cuda:0"


def q4_weight(N, K, seed, dev):
    """seeded Gaussian blocks whose magnitudes span 2^-20 .. 2^3 block by block (the scales differ along K and within one 32-column tile), a zero
    row, a zero block and a -0.0"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.randint(-20, 4, (N, K // 32), generator=g).float()).repeat_interleave(32, dim=1)
    w = torch.randn(N, K, generator=g) * mag
    w[2, 0] = -0.0
    w[3] = 0.0
    w[4, 32:64] = 0.0
    return w.to(torch.bfloat16).to(dev)


def all_codes_weight(dev):
    """[32, 512] = one column tile, four chunks of one granule: every block of 32 holds all 16 codes twice, rotated by (column + block), so over the
    16 blocks of a column every position (k-step parity, lane half, element = byte and nibble) sees every code, -0 included.  Block exponents: chunk 0
    from the smallest allowed (-125) up, chunk 2 up to the largest (125), chunks 1 and 3 around 0 -- 32 different exponents inside the tile per block
    column.  The activation of a chunk is scaled so that its products sit near 1: nothing vanishes in, or overflows, the fp32 accumulator."""
    import sjd_amd.ops as ops
    n, k = torch.arange(32)[:, None], torch.arange(512)[None, :]
    blk = k // 32
    code = (k % 32 + n + blk) % 16
    grid = torch.tensor(ops._E2M1_VALUES)
    val = torch.where(code >= 8, -1.0, 1.0) * grid[code % 8]
    chunk = k // 128
    exp = torch.where(chunk == 0, ops.Q4_MIN_SCALE_EXP + n, torch.where(chunk == 2, ops.Q4_MAX_SCALE_EXP - 31 + n, -12 + (n + blk) % 28))
    w = torch.ldexp(val, exp.expand(32, 512)).to(torch.bfloat16)
    xs = torch.tensor([110.0, 0.0, -110.0, 0.0]).repeat_interleave(128)
    x = (torch.randn(32, 512, generator=torch.Generator().manual_seed(11)) * torch.exp2(xs)[None]).to(torch.bfloat16)
    return w.to(dev), x.to(dev)


def g1_pair(ops, x, w, KC, waves, sm):
    """(planes of G1q4 on the packed weight, planes of G1 on its dequantised twin, the PackedQ4)"""
    N, K = w.shape
    pq = ops.pack_weight_q4(w, KC, sm)
    wp = ops.pack_weight(pq.dequant(), KC, sm)
    ref = ops.skinny_gemm(x, wp, N, K, KC, waves, sm).data
    got = ops.skinny_gemm(x, pq, N, K, KC, waves, sm).data
    torch.cuda.synchronize()
    return got, ref, pq


G1Q4_CASES = [(1, 32, G, G, 1, False), (7, 32, G, G, 1, False), (32, 32, G, G, 1, True),          # one unit
              (9, 96, 2 * G, G, 4, False),                     # a workgroup with a missing tile
              (32, 96, 5 * G, 2 * G, 3, False), (17, 96, 5 * G, 2 * G, 3, True),          # two chunks and a ragged last one of one granule
              (5, 64, 3 * G, 3 * G, 2, True),                  # three half trips: the unit ends in the middle of a ring trip
              (33, 64, 1280, 1280, 8, True), (64, 64, 1280, 1280, 2, False),              # two row tiles, at the LDS limit
              (32, 64, 2560, 2560, 8, True),                   # one row tile at its limit
              (40, 416, 3 * G, 2 * G, 12, False), (32, 416, 3 * G, 2 * G, 12, True)]      # 12 waves (the 1024-thread form: ring depth 8), a missing tile


@pytest.mark.parametrize("M,N,K,KC,waves,step_major", G1Q4_CASES)
def test_g1q4_planes_are_g1_on_the_dequantised_weight(dev, M, N, K, KC, waves, step_major):
    import sjd_amd.ops as ops
    w = q4_weight(N, K, N + K + M, dev)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16).to(dev)
    got, ref, pq = g1_pair(ops, x, w, KC, waves, step_major)
    assert torch.equal(ops.quantize_mxfp4(w)[0].cpu(), ops.quantize_mxfp4(w.cpu())[0])          # the quantiser gives the same codes on either device
    assert int(pq.codes()[2, 0]) & 0xF == 8 and len(set(pq.scale_exp()[:32].flatten().tolist())) > 8
    assert got.shape == ref.shape == ((K + KC - 1) // KC, 32 * ((M + 31) // 32), N)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (got - ref).abs().max()
    assert float(ref.abs().max()) > 0


def test_g1q4_decodes_every_code_in_every_position_over_the_whole_exponent_range(dev):
    """pins the nibble / byte_sel order of v_cvt_scalef32_pk_bf16_fp4 and the e8m0 -> float scale at both ends"""
    import sjd_amd.ops as ops
    w, x = all_codes_weight(dev)
    codes, se = ops.quantize_mxfp4(w)
    assert torch.equal(ops.dequantize_mxfp4(codes, se).view(torch.int16), w.view(torch.int16))          # the weight IS on the grid: nothing is lost
    nib = torch.stack([codes & 0xF, codes >> 4], dim=2).reshape(32, 16, 32)                             # [column, block, position in the block]
    for c in range(16):
        assert bool((nib == c).any(dim=1).all()), f"code {c} misses a (column, position)"
    assert int(se.min()) == 127 + ops.Q4_MIN_SCALE_EXP == 2 and int(se.max()) == 127 + ops.Q4_MAX_SCALE_EXP == 252
    assert all(int(se[:, b].max()) - int(se[:, b].min()) >= 24 for b in range(16))                      # >= 24 binades inside the tile, in every block
    assert bool((w.view(torch.int16) == -32768).any())                                                  # -0.0
    for sm in (False, True):
        got, ref, pq = g1_pair(ops, x, w, G, 1, sm)
        assert torch.equal(pq.codes(), codes) and torch.equal(pq.scale_exp(), se)
        assert got.shape == (4, 32, 32) and torch.equal(got.view(torch.int32), ref.view(torch.int32))
        assert bool(torch.isfinite(ref).all()) and all(float(ref[c].abs().max()) > 2.0 ** -10 for c in range(4))
    # an exact product as well, independent of G1: row m of x = the unit vector e_m picks w[:, m] out of chunk 0's plane
    xe = torch.zeros(32, 512, dtype=torch.bfloat16, device=dev)
    xe[torch.arange(32), torch.arange(32)] = 1.0
    plane = ops.skinny_gemm(xe, ops.pack_weight_q4(w, G, False), 32, 512, G, 1, False).data[0]
    torch.cuda.synchronize()
    assert torch.equal(plane.t().contiguous(), w[:, :32].float())


def test_g1q4_column_window_and_graph_replay(dev):
    import sjd_amd.ops as ops
    M, NP, K, KC, c0, nc = 32, 512, 4 * G, 2 * G, 64, 352
    w = q4_weight(NP, K, 77, dev)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(dev)
    for sm in (True, False):
        pq = ops.pack_weight_q4(w, KC, sm)
        full = ops.skinny_gemm(x, pq, NP, K, KC, 8, sm).data
        ref = ops.skinny_gemm_cols(x, ops.pack_weight(pq.dequant(), KC, sm), NP, K, KC, c0, nc, 8, sm).data
        got = ops.skinny_gemm_cols(x, pq, NP, K, KC, c0, nc, 8, sm).data          # tile0 = 2 (the scales still sit behind all N_packed * K / 2 code bytes)
        torch.cuda.synchronize()
        assert got.shape == (2, 32, nc) and torch.equal(got.view(torch.int32), full[:, :, c0:c0 + nc].contiguous().view(torch.int32))
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.skinny_gemm(x, pq, NP, K, KC, 8, False)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        cap = ops.skinny_gemm(x, pq, NP, K, KC, 8, False).data
    cap.fill_(float("nan"))
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap.view(torch.int32), full.view(torch.int32))


@pytest.mark.parametrize("step_major", [False, True])
@pytest.mark.parametrize("with_norm", [True, False])
@pytest.mark.parametrize("M,I,K", [(9, 64, 512), (32, 128, 1024), (32, 64, 512), (9, 128, 1024)])
def test_g1sq4_is_g1s_on_the_dequantised_weight(dev, M, I, K, with_norm, step_major):
    import sjd_amd.ops as ops
    w = q4_weight(2 * I, K, I + K + M, dev)
    pq = ops.pack_weight_q4(w, K // 2, step_major, gateup=True)
    wp = ops.pack_weight(pq.dequant(), K // 2, step_major)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M + 1)).to(torch.bfloat16).to(dev)
    assert ops.gateup_silu_ok(M, I, K, K // 2, packed_q8=True)
    rn = (ops.residual_sumsq(x.clone(), None), K, 1e-5) if with_norm else None
    ref = ops.gateup_silu(x, wp, I, K, step_major, row_norm=rn)
    got = ops.gateup_silu(x, pq, I, K, step_major, row_norm=rn)
    unfused = ops.silu_mul(ops.skinny_gemm(x, pq, 2 * I, K, K // 2, 8, step_major), rows=M, dtype=x.dtype, row_norm=rn)        # G1q4 + F3
    torch.cuda.synchronize()
    assert got.shape == (M, I) and got.dtype == torch.bfloat16
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (got.float() - ref.float()).abs().max()
    assert torch.equal(unfused.view(torch.int16), ref.view(torch.int16))
    assert float(ref.float().abs().max()) > 0


@pytest.mark.parametrize("K", [2048, 4096])
def test_g1sq4_at_the_deep_ring_sizes(dev, K):
    """K = 2048 / 4096: the instantiations whose ring holds sixteen k-steps (the two smaller K run on a ring of eight)"""
    import sjd_amd.ops as ops
    M, I = 17, 64
    w = q4_weight(2 * I, K, K, dev)
    pq = ops.pack_weight_q4(w, K // 2, True, gateup=True)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(K)).to(torch.bfloat16).to(dev)
    ref = ops.gateup_silu(x, ops.pack_weight(pq.dequant(), K // 2, True), I, K, True)
    got = ops.gateup_silu(x, pq, I, K, True)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)) and float(ref.float().abs().max()) > 0


def test_c_boundary_refusals(dev):
    """with the bit set, what G1q4 / G1sq4 do not serve comes back as SJD_ERR_UNSUPPORTED (both weight bits: SJD_ERR_BAD_ARG) before any launch"""
    import sjd_amd._lib as L
    lib = L.load()
    assert L.G1_W4_MXFP4 == W4 == 0x4000 and L.G1_W8_E4M3 == W8
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    BF = L.DTYPE_BF16 | W4
    # sjd_skinny_gemm(x, w_packed, out, M, N, K, KC, waves, step_major, dtype, stream)
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 128, 128, 1, 0, L.DTYPE_F16 | W4, None) == UNSUPPORTED            # fp16
    assert lib.sjd_skinny_gemm(p, p, p, 65, 32, 128, 128, 1, 0, BF, None) == UNSUPPORTED                          # more than 64 rows: no wide form
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 192, 128, 1, 0, BF, None) == UNSUPPORTED                          # K no multiple of the granule
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 256, 64, 1, 0, BF, None) == UNSUPPORTED                           # KC no multiple of the granule
    assert lib.sjd_skinny_gemm(p, p, p, 40, 32, 1408, 1408, 1, 0, BF, None) == UNSUPPORTED                        # 88 k-steps x two row tiles > 160 KiB
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 2688, 2688, 1, 0, BF, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 128, 128, 1, 0, BF | W8, None) == BAD_ARG                         # both weight streams at once
    # sjd_skinny_gemm_cols(.., dtype, N_packed, tile0, stream)
    assert lib.sjd_skinny_gemm_cols(p, p, p, 65, 32, 128, 128, 1, 0, BF, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm_cols(p, p, p, 32, 32, 128, 128, 1, 0, L.DTYPE_F16 | W4, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm_cols(p, p, p, 32, 32, 192, 64, 1, 0, BF, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm_cols(p, p, p, 32, 32, 128, 128, 1, 0, BF | W8, 64, 0, None) == BAD_ARG
    # sjd_gateup_silu(x, w_packed, y, M, I, K, step_major, dtype, row_norm, stream)
    assert lib.sjd_gateup_silu(p, p, p, 33, 64, 1024, 0, BF, None, None) == UNSUPPORTED                           # G1sq4: 32 rows
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, 1024, 0, L.DTYPE_F16 | W4, None, None) == UNSUPPORTED
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, 768, 0, BF, None, None) == UNSUPPORTED
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, 1024, 0, BF | W8, None, None) == BAD_ARG
    # an entry point that does not know the bit: sjd_silu_mul(gate_up, y, rows, inter, dtype, part, n_chunks, stream)
    assert lib.sjd_silu_mul(p, p, 8, 64, BF, None, 0, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


TOY = dict(vocab_size=9216, hidden_size=512, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, max_position_embeddings=512,
           rms_norm_eps=1e-5, rope_theta=10000.0)


def _toy(dev, kv_heads, weights, g1_cfg, seed=29, **kw):
    import sjd_amd.ops as ops
    from tests.helpers import make_chameleon
    model = make_chameleon(dict(TOY, num_key_value_heads=kv_heads), seed, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=dev)
    if g1_cfg is not None:
        model.G1_CFG = dict(g1_cfg)
    return model.enable_fused(ops, gemm="sjd", weights=weights, **kw)


def _decode(dev, kv_heads, weights, g1_cfg, img_len=48, window=16, P=10, seed=5):
    """48 image tokens through SJDEngine (window 16, CFG: 32 rows per forward) on the toy backbone"""
    import sjd_amd.synthetic as synthetic
    from sjd_amd.engine import SJDEngine, SJDConfig, WindowSpec
    from sjd_amd.grammar import AnoleGrammar
    V = TOY["vocab_size"]
    model = _toy(dev, kv_heads, weights, g1_cfg)
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


# MHA: the architecture's own set (G1_CFG_Q4: at hidden 512 its gate|up chunk is the whole K, so G1q4 + F3) and one that packs gate|up in two K
# halves (G1sq4); GQA: G1_CFG_EMU3_Q4
HALVES = dict(qkv=(256, 4, True), o=(128, 3, False), gate_up=(256, 8, True), down=(128, 2, False))


@pytest.mark.parametrize("kv_heads,g1_cfg", [(4, None), (4, HALVES), (2, None)])
def test_end_to_end_tokens_agree_with_the_bf16_twin(dev, kv_heads, g1_cfg):
    import sjd_amd.ops as ops
    m4, tok4, acc4, probs4 = _decode(dev, kv_heads, "mxfp4", g1_cfg)
    m16, tok16, acc16, probs16 = _decode(dev, kv_heads, "mxfp4_as_bf16", g1_cfg)
    assert len(tok4) >= 48 and tok4 == tok16
    assert acc4 == acc16 and len(acc4) > 1
    assert torch.equal(probs4.view(torch.int32), probs16.view(torch.int32)) and float(probs4.sum()) > 0
    assert all(isinstance(w, ops.PackedQ4) for d in m4._packed for w in d.values())
    assert not isinstance(m4._packed_head, ops.PackedQ4) and not any(isinstance(w, ops.PackedQ4) for d in m16._packed for w in d.values())
    if g1_cfg is None:
        assert m4.G1_CFG == (m4.G1_CFG_EMU3_Q4 if kv_heads != 4 else m4.G1_CFG_Q4) == m16.G1_CFG
    assert m4.packed_bytes(head=False) * 32 == m16.packed_bytes(head=False) * 8.5          # 4.25 bits per weight against 16
    assert m4.packed_bytes() - m4.packed_bytes(head=False) == m16.packed_bytes() - m16.packed_bytes(head=False) > 0      # the head is not quantised
    st = m4.compress_stats
    assert st["q4_matrices"] == 8 and st["q4_bytes_packed"] == m4.packed_bytes(head=False) and 2.0 ** -6 < st["rel_rms_error"] < 0.25
    assert m16.compress_stats["rel_rms_error"] == st["rel_rms_error"] and "q4_bytes_packed" not in m16.compress_stats and "q8_matrices" not in st


def _decode_two(dev, weights, hg=3, wg=3, window=16, seed=3):
    """two Lumina-grammar images of distinct prompt lengths through SJDBatchEngine (window 16, CFG: 64 rows per forward) on the toy backbone"""
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    from sjd_amd.engine import SJDConfig, WindowSpec
    from sjd_amd.engine_batch import SJDBatchEngine
    from sjd_amd.grammar import LuminaGrammar
    V, n_prompts = TOY["vocab_size"], 2
    model = _toy(dev, 4, weights, HALVES, seed=23)
    n_img = (2 * wg + 1) * 2 * hg
    prompts, specs, lens = [], [], [9 + i for i in range(n_prompts)]
    for i, Pi in enumerate(lens):
        pr = torch.cat([synthetic.synthetic_prompt(Pi - 3, seed + 17 * i, lo=8900, hi=9200), torch.tensor([[8197, 8804 + hg, 8804 + wg]])], dim=1)
        prompts.append(pr[0].tolist())
        specs.append(WindowSpec(first_tokens=pr.to(dev).repeat(2, 1),
                                first_positions=torch.stack([torch.arange(Pi), torch.tensor([1] * (Pi - 1) + [0])]).to(dev),
                                key_start=torch.tensor([0, Pi - 1], dtype=torch.int32), pos_offset=torch.tensor([0, -(Pi - 1)], dtype=torch.long), kv_base=0))
    max_len = max(lens) + n_img + 1 + 4
    model.setup_cache(batch=2 * n_prompts, s_max=((max_len + 64 + 31) // 32) * 32)
    cfg = SJDConfig(jacobi_loop_interval_l=3, jacobi_loop_interval_r=n_img - 10, max_num_new_tokens=window, guidance_scale=3.0, seed=seed,
                    prefix_token_sampler_scheme="speculative_jacobi", max_length=1 << 20, eos_token_ids=(8196,))
    eng = SJDBatchEngine(model, V, dev, n_prompts, max_window=window, use_graph=True)
    rows, orig = [], ops.skinny_gemm

    def spy(x_, *a, **k):
        rows.append(int(x_.shape[0]))
        return orig(x_, *a, **k)
    ops.skinny_gemm = spy
    try:
        results = eng.decode_many(prompts, specs, [LuminaGrammar(2000, 10) for _ in range(n_prompts)], cfg)
    finally:
        ops.skinny_gemm = orig
    torch.cuda.synchronize()
    assert rows and max(rows) == 64, "the window forward did not run on the hand-written projections at 64 rows"
    return model, [(seq[len(p):], list(st.matched)) for (seq, st), p in zip(results, prompts)], eng.probs_all.clone()


def test_batch_engine_two_prompts_at_64_rows_agree_with_the_bf16_twin(dev):
    import sjd_amd.ops as ops
    m4, out4, probs4 = _decode_two(dev, "mxfp4")
    m16, out16, probs16 = _decode_two(dev, "mxfp4_as_bf16")
    assert isinstance(m4._packed[0]["gate_up"], ops.PackedQ4) and not isinstance(m16._packed[0]["gate_up"], ops.PackedQ4)
    for i in range(2):
        assert len(out4[i][0]) >= 42 and out4[i][0] == out16[i][0], f"prompt {i}: tokens differ"
        assert out4[i][1] == out16[i][1] and len(out4[i][1]) > 1, f"prompt {i}: acceptance counts differ"
    assert out4[0][0] != out4[1][0]
    assert torch.equal(probs4.view(torch.int32), probs16.view(torch.int32)) and float(probs4.sum()) > 0


@pytest.fixture(scope="module")
def real_size_pair(dev):
    """one Lumina-sized layer (hidden 4096, 32 heads of 128, intermediate 11008) with the architecture's own G1_CFG_Q4, packed as "mxfp4" and as its twin"""
    import sjd_amd.backbones as BB
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    args = BB.ChameleonArgs(vocab_size=9216, hidden_size=4096, intermediate_size=11008, num_hidden_layers=1, num_attention_heads=32,
                            num_key_value_heads=32, max_position_embeddings=512)
    out = []
    for wt in ("mxfp4", "mxfp4_as_bf16"):
        with torch.device(dev):
            m = BB.ChameleonBackbone(args, attn=ops.HipWindowAttention(n_split=2)).to(torch.bfloat16).eval()
        synthetic.fill_state_dict_device(m, seed=7, embed_token_scale=0.25)
        m.enable_fused(ops, gemm="sjd", weights=wt)
        assert m.G1_CFG == m.G1_CFG_Q4 and m.G1_CFG["gate_up"] == (2048, 8, True)
        m.setup_cache(batch=2, s_max=64)
        out.append(m)
    return out


# 32 rows: gate|up is the fused G1sq4 launch over its two K halves of 2048; 40 and 64 rows: G1q4 stages at most 1280 columns for two row tiles, so the
# same step-major packing is read in chunks of 1024 (+ F3); the down projection's K = 11008 = 14 chunks of 768 and a ragged one of 256
@pytest.mark.parametrize("n", [16, 20, 32])
def test_real_size_window_of_up_to_64_rows(dev, real_size_pair, n):
    import sjd_amd.ops as ops
    m4, m16 = real_size_pair
    assert isinstance(m4._packed[0]["gate_up"], ops.PackedQ4) and m4._packed[0]["gate_up"].KC == 2048
    assert m4._q8_chunk("gate_up", 2 * n, 4096) == (2048 if n == 16 else 1024) == m16._q8_chunk("gate_up", 2 * n, 4096)
    assert m4._q8_chunk("qkv", 2 * n, 4096) == 1024 and m4._q8_chunk("down", 2 * n, 11008) == 768
    g = torch.Generator().manual_seed(n)
    tok = torch.randint(4, 8196, (2, n), generator=g).to(dev)
    pos = torch.arange(n)[None].repeat(2, 1).to(dev)
    ks = torch.zeros(2, dtype=torch.int32, device=dev)
    with torch.no_grad():
        outs = [m.forward_window(tok, pos, 0, ks).float() for m in (m4, m16)]
    torch.cuda.synchronize()
    assert outs[0].shape == (2, n, 9216) and bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_python_refusals(dev):
    import sjd_amd.backbones as BB
    import sjd_amd.launch_shapes as LS
    import sjd_amd.ops as ops
    from sjd_amd.engine_batch import SJDBatchEngine
    from tests.helpers import make_chameleon
    conf = dict(TOY, num_key_value_heads=4)
    mk = lambda dtype=torch.bfloat16: make_chameleon(conf, 29, 0.25, ops.HipWindowAttention(n_split=2), dtype=dtype, device=dev)
    untouched = lambda m: getattr(m, "weights", None) is None and getattr(m, "_ops", None) is None and getattr(m, "_packed", None) is None
    for wt in ("mxfp4", "mxfp4_as_bf16"):
        for kw, match, m in ((dict(gemm="sjd"), "fp16|float16", mk(torch.float16)), (dict(gemm="torch"), "gemm='sjd'", mk()),
                             (dict(gemm="sjd", max_rows=128), "at most 64 rows", mk()), (dict(gemm="sjd", max_rows=256), "at most 64 rows", mk())):
            with pytest.raises(ValueError, match=match):
                m.enable_fused(ops, weights=wt, **kw)
            assert untouched(m)
        m = mk()
        m.G1_CFG = dict(HALVES, o=(176, 3, False))                       # no multiple of the granule
        with pytest.raises(ValueError, match="multiples of 128"):
            m.enable_fused(ops, gemm="sjd", weights=wt)
        assert untouched(m)
        m = mk()
        m.G1_CFG = dict(HALVES, qkv=(2688, 4, True))                     # above what a 32-row window stages
        with pytest.raises(ValueError, match="<= 2560"):
            m.enable_fused(ops, gemm="sjd", weights=wt)
        assert untouched(m)
        swin = BB.ChameleonBackbone(BB.ChameleonArgs(vocab_size=9216, hidden_size=512, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4,
                                                     num_key_value_heads=4, max_position_embeddings=512, swin_norm=True),
                                    attn=ops.HipWindowAttention(n_split=2)).to(device=dev, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="swin-norm"):
            swin.enable_fused(ops, gemm="sjd", weights=wt)
    with pytest.raises(ValueError, match="'mxfp4' or 'mxfp4_as_bf16'"):
        mk().enable_fused(ops, gemm="sjd", weights="int4")
    # a refused call on a backbone that IS packed leaves its packing as it was
    d = mk().enable_fused(ops, gemm="sjd")
    packed = d._packed
    with pytest.raises(ValueError, match="at most 64 rows"):
        d.enable_fused(ops, gemm="sjd", weights="mxfp4", max_rows=128)
    assert d.weights is None and d._packed is packed and isinstance(d._packed[0]["qkv"], ops.PackedZ) and "q4_matrices" not in d.compress_stats
    for wt in ("mxfp4", "mxfp4_as_bf16"):
        m = mk().enable_fused(ops, gemm="sjd", weights=wt, max_rows=64)
        assert LS.serves_rows(m, 64) is None and LS.serves_rows(m, 65) == ("max_rows", 64) == LS.serves_rows(m, 256)
        SJDBatchEngine(m, 9216, dev, n_prompts=2)                            # 64 rows: served
        with pytest.raises(ValueError, match="at most 64 window rows"):
            SJDBatchEngine(m, 9216, dev, n_prompts=3)
        m.setup_cache(batch=8, s_max=64)
        with pytest.raises(ValueError, match="at most 64 rows"):          # and the backbone itself refuses a taller window
            m.forward_window(torch.zeros(8, 16, dtype=torch.long, device=dev), torch.zeros(8, 16, dtype=torch.long, device=dev), 0,
                             torch.zeros(8, dtype=torch.int32, device=dev))
