"""GPU: the window projections streamed from 6-bit e2m3 weights -- kernels G1q6 / G1sq6 behind SJD_G1_W6_E2M3 (csrc/sjd_gemm_q6.h), ops.PackedQ6,
ChameleonBackbone.enable_fused(weights="e2m3").  Nothing here has a tolerance: the kernels rebuild the bf16 MFMA operand code * scale bit for bit (one
v_cvt_scalef32_pk32_bf16_fp6 per record and lane), so every result is compared BIT FOR BIT with the uncompressed kernels (G1 / G1s) run on
PackedQ6.dequant() -- and the one-hot probe compares with the weight itself, which pins the instruction's code order and the scale placement.  All the
loss of the format is in ops.quantize_e2m3 (tests/test_q6_pack.py, CPU).  G = 128 is the stream's K granule."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

W6, W4, W8 = 0x8000, 0x4000, 0x2000          # SJD_G1_W6_E2M3, SJD_G1_W4_MXFP4, SJD_G1_W8_E4M3
UNSUPPORTED, BAD_ARG = -2, -1
G = 128


@pytest.fixture(scope="module")
def dev():
    from tests.conftest import poison_device_memory
    poison_device_memory(total_gib=1)          # the planes come from torch.empty: an unwritten element must not read as zero
    return "cuda:0"


def block_col(K):
    k = torch.arange(K)
    return 2 * (k // 64) + (k % 16) // 8


def q6_weight(N, K, seed, dev):
    """seeded Gaussian blocks whose magnitudes span 2^-20 .. 2^3 scale block by scale block (the scales differ along K, between the lane halves and
    within one 32-column tile), a zero row, a zero record and a -0.0"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.randint(-20, 4, (N, K // 32), generator=g).float())[:, block_col(K)]
    w = torch.randn(N, K, generator=g) * mag
    w[2, 0] = -0.0
    w[3] = 0.0
    w[4, 64:128] = 0.0
    return w.to(torch.bfloat16).to(dev)


def g1_pair(ops, x, w, KC, waves, sm):
    """(planes of G1q6 on the packed weight, planes of G1 on its dequantised twin, the PackedQ6)"""
    N, K = w.shape
    pq = ops.pack_weight_q6(w, KC, sm)
    wp = ops.pack_weight(pq.dequant(), KC, sm)
    ref = ops.skinny_gemm(x, wp, N, K, KC, waves, sm).data
    got = ops.skinny_gemm(x, pq, N, K, KC, waves, sm).data
    torch.cuda.synchronize()
    return got, ref, pq


def test_one_hot_rows_read_every_code_and_scale_back_exactly(dev):
    """N = 64, K = 128: the weight is ON the grid (code * 2^exp), every block holds 32 codes of one parity -- so all 64 codes occur, each block holds a
    magnitude >= 7 that pins its scale -- and the block exponents run from the smallest to the largest the format allows.  Row m of x is the unit vector
    e_k, so the single plane IS w[:, k]: the code order inside the six dwords, the record planes and the scale byte of every (column, record, lane half)
    are what the packer says, or this fails."""
    import sjd_amd.ops as ops
    N, K = 64, 128
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    b = block_col(K)[None, :]
    e = 8 * ((k % 64) // 16) + k % 8
    code = (2 * e + n + b) % 64
    grid = torch.tensor([i * 0.125 for i in range(16)] + [2 + i * 0.25 for i in range(8)] + [4 + i * 0.5 for i in range(8)])
    val = torch.where(code >= 32, -1.0, 1.0) * grid[code % 32]
    exps = torch.tensor([ops.Q6_MIN_SCALE_EXP, -9, 0, 3, ops.Q6_MAX_SCALE_EXP])
    exp = exps[(n + b) % 5].expand(N, K)
    w = torch.ldexp(val, exp).to(torch.bfloat16).to(dev)
    pq = ops.pack_weight_q6(w, G, False)
    assert sorted(set(pq.codes().flatten().tolist())) == list(range(64))
    assert sorted(set(pq.scale_exp().flatten().tolist())) == sorted(127 + int(v) for v in exps) and len(set(pq.scale_exp()[0].tolist())) >= 3
    assert torch.equal(pq.codes().cpu(), code.to(torch.uint8)) and torch.equal(pq.scale_exp().cpu(), (exp[:, ::8][:, [0, 1, 8, 9]] + 127).to(torch.uint8))
    deq = pq.dequant()
    assert torch.equal(deq.view(torch.int16), w.view(torch.int16))                                      # the weight IS on the grid: nothing is lost
    assert bool((w.view(torch.int16) == -32768).any())                                                  # -0.0
    for sm in (False, True):
        pq = ops.pack_weight_q6(w, G, sm)
        for rep in range(4):
            x = torch.zeros(32, K, dtype=torch.bfloat16, device=dev)
            x[torch.arange(32), 32 * rep + torch.arange(32)] = 1.0
            plane = ops.skinny_gemm(x, pq, N, K, G, 2, sm).data
            torch.cuda.synchronize()
            assert plane.shape == (1, 32, N)
            assert torch.equal(plane[0].t().contiguous(), deq[:, 32 * rep:32 * rep + 32].float()), (sm, rep)


G1Q6_CASES = [(1, 32, G, G, 1, False),                        # one unit
              (32, 96, 2 * G, G, 4, False), (32, 96, 2 * G, G, 4, True),          # a workgroup with a missing tile
              (32, 96, 2 * G, G, 1, True), (32, 96, 2 * G, G, 8, False),          # one wave per workgroup; five waves without a tile
              (33, 64, 2 * G, 2 * G, 2, True),                # two row tiles
              (64, 96, 3 * G, 2 * G, 4, True),                # two chunks and a ragged last one of one granule
              (5, 64, 3 * G, 3 * G, 2, True),                 # three half trips: the unit ends in the middle of a ring trip
              (64, 64, 1280, 1280, 2, False),                 # two row tiles, at the LDS limit
              (32, 64, 2560, 2560, 8, False),                 # one row tile at its limit
              (40, 416, 3 * G, 2 * G, 12, False), (32, 416, 3 * G, 2 * G, 12, True)]      # 12 waves (the 1024-thread form: ring depth 8), a missing tile


@pytest.mark.parametrize("M,N,K,KC,waves,step_major", G1Q6_CASES)
def test_g1q6_planes_are_g1_on_the_dequantised_weight(dev, M, N, K, KC, waves, step_major):
    import sjd_amd.ops as ops
    w = q6_weight(N, K, N + K + M, dev)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16).to(dev)
    got, ref, pq = g1_pair(ops, x, w, KC, waves, step_major)
    assert torch.equal(ops.quantize_e2m3(w)[0].cpu(), ops.quantize_e2m3(w.cpu())[0])          # the quantiser gives the same codes on either device
    assert int(pq.codes()[2, 0]) == 32 and len(set(pq.scale_exp()[:32].flatten().tolist())) > 8
    assert got.shape == ref.shape == ((K + KC - 1) // KC, 32 * ((M + 31) // 32), N)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (got - ref).abs().max()
    assert float(ref.abs().max()) > 0


def test_g1q6_column_window_and_graph_replay(dev):
    import sjd_amd.ops as ops
    M, NP, K, KC, c0, nc = 32, 512, 4 * G, 2 * G, 64, 352
    w = q6_weight(NP, K, 77, dev)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(dev)
    for sm in (True, False):
        pq = ops.pack_weight_q6(w, KC, sm)
        full = ops.skinny_gemm(x, pq, NP, K, KC, 8, sm).data
        ref = ops.skinny_gemm_cols(x, ops.pack_weight(pq.dequant(), KC, sm), NP, K, KC, c0, nc, 8, sm).data
        got = ops.skinny_gemm_cols(x, pq, NP, K, KC, c0, nc, 8, sm).data          # tile0 = 2 (the scales still sit behind all N_packed * K * 3 / 4 code bytes)
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
@pytest.mark.parametrize("M,I,K", [(1, 64, 512), (32, 128, 1024), (9, 64, 4096), (17, 64, 2048)])
def test_g1sq6_is_g1q6_plus_f3(dev, M, I, K, step_major):
    import sjd_amd.ops as ops
    w = q6_weight(2 * I, K, I + K + M, dev)
    pq = ops.pack_weight_q6(w, K // 2, step_major, gateup=True)
    wp = ops.pack_weight(pq.dequant(), K // 2, step_major)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M + 1)).to(torch.bfloat16).to(dev)
    assert ops.gateup_silu_ok(M, I, K, K // 2, packed_q8=True)
    rn = (ops.residual_sumsq(x.clone(), None), K, 1e-5)
    for row_norm in (rn, None):
        ref = ops.gateup_silu(x, wp, I, K, step_major, row_norm=row_norm)
        got = ops.gateup_silu(x, pq, I, K, step_major, row_norm=row_norm)
        unfused = ops.silu_mul(ops.skinny_gemm(x, pq, 2 * I, K, K // 2, 8, step_major), rows=M, dtype=x.dtype, row_norm=row_norm)        # G1q6 + F3
        torch.cuda.synchronize()
        assert got.shape == (M, I) and got.dtype == torch.bfloat16
        assert torch.equal(got.view(torch.int16), unfused.view(torch.int16)), (got.float() - unfused.float()).abs().max()
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
        assert float(ref.float().abs().max()) > 0


def test_c_boundary_refusals(dev):
    """with the bit set, what G1q6 / G1sq6 do not serve comes back as SJD_ERR_UNSUPPORTED (two stream bits: SJD_ERR_BAD_ARG) before any launch"""
    import sjd_amd._lib as L
    lib = L.load()
    assert L.G1_W6_E2M3 == W6 and L.G1_W4_MXFP4 == W4 and L.G1_W8_E4M3 == W8
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    BF = L.DTYPE_BF16 | W6
    # sjd_skinny_gemm(x, w_packed, out, M, N, K, KC, waves, step_major, dtype, stream)
    w_, o_ = ctypes.c_void_p(buf.data_ptr() + (16 << 10)), ctypes.c_void_p(buf.data_ptr() + (32 << 10))
    assert lib.sjd_skinny_gemm(p, w_, o_, 32, 32, 128, 128, 1, 0, BF, None) == 0                                  # the bit is known: a served shape runs (zeros in, zeros out)
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 128, 128, 1, 0, L.DTYPE_F16 | W6, None) == UNSUPPORTED            # fp16
    assert lib.sjd_skinny_gemm(p, p, p, 65, 32, 128, 128, 4, 0, BF, None) == UNSUPPORTED                          # more than 64 rows: no wide form
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 192, 128, 1, 0, BF, None) == UNSUPPORTED                          # K no multiple of the granule
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 256, 64, 1, 0, BF, None) == UNSUPPORTED                           # KC no multiple of the granule
    assert lib.sjd_skinny_gemm(p, p, p, 40, 32, 1408, 1408, 1, 0, BF, None) == UNSUPPORTED                        # 88 k-steps x two row tiles > 160 KiB
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 2688, 2688, 1, 0, BF, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 128, 128, 1, 0, BF | W8, None) == BAD_ARG                         # two weight streams at once
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 128, 128, 1, 0, BF | W4, None) == BAD_ARG
    assert lib.sjd_skinny_gemm(p, p, p, 32, 32, 128, 128, 1, 0, BF | W4 | W8, None) == BAD_ARG
    # sjd_skinny_gemm_cols(.., dtype, N_packed, tile0, stream)
    assert lib.sjd_skinny_gemm_cols(p, p, p, 65, 32, 128, 128, 4, 0, BF, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm_cols(p, p, p, 32, 32, 128, 128, 1, 0, L.DTYPE_F16 | W6, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm_cols(p, p, p, 32, 32, 192, 64, 1, 0, BF, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm_cols(p, p, p, 32, 32, 128, 128, 1, 0, BF | W4, 64, 0, None) == BAD_ARG
    # sjd_gateup_silu(x, w_packed, y, M, I, K, step_major, dtype, row_norm, stream)
    assert lib.sjd_gateup_silu(p, p, p, 33, 64, 1024, 0, BF, None, None) == UNSUPPORTED                           # G1sq6: 32 rows
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, 1024, 0, L.DTYPE_F16 | W6, None, None) == UNSUPPORTED
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, 768, 0, BF, None, None) == UNSUPPORTED
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, 8192, 4 << L.G1S_CHUNKS_SHIFT, BF, None, None) == UNSUPPORTED     # no K = 8192 form
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, 1024, 0, BF | W8, None, None) == BAD_ARG
    # sjd_prefill_gemm(x, w_packed, y, M, N, K, KC, step_major, dtype, row_scale, stream): no form for this stream
    assert lib.sjd_prefill_gemm(p, p, p, 32, 32, 128, 128, 0, BF, None, None) == UNSUPPORTED
    # an entry point that does not know the bit: sjd_silu_mul(gate_up, y, rows, inter, dtype, part, n_chunks, stream)
    assert lib.sjd_silu_mul(p, p, 8, 64, BF, None, 0, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


TOY = dict(vocab_size=9216, hidden_size=512, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, max_position_embeddings=512,
           rms_norm_eps=1e-5, rope_theta=10000.0)
# packs gate|up in two K halves (G1sq6 at <= 32 rows); without it the architecture's own set (G1_CFG_Q4: at hidden 512 its gate|up chunk is the whole K,
# so G1q6 + F3) / G1_CFG_EMU3_Q4 (GQA)
HALVES = dict(qkv=(256, 4, True), o=(128, 3, False), gate_up=(256, 8, True), down=(128, 2, False))


def _toy(dev, kv_heads, weights, g1_cfg, seed=29, **kw):
    import sjd_amd.ops as ops
    from tests.helpers import make_chameleon
    model = make_chameleon(dict(TOY, num_key_value_heads=kv_heads), seed, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=dev)
    if g1_cfg is not None:
        model.G1_CFG = dict(g1_cfg)
    return model.enable_fused(ops, gemm="sjd", weights=weights, **kw)


def _decode(dev, kv_heads, weights, g1_cfg, img_len=40, window=16, P=10, seed=5):
    """40 image tokens through SJDEngine (window 16, CFG: 32 rows per forward) on the toy backbone"""
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


@pytest.mark.parametrize("kv_heads,g1_cfg", [(4, HALVES), (2, None)])
def test_end_to_end_tokens_agree_with_the_bf16_twin(dev, kv_heads, g1_cfg):
    import sjd_amd.ops as ops
    m6, tok6, acc6, probs6 = _decode(dev, kv_heads, "e2m3", g1_cfg)
    m16, tok16, acc16, probs16 = _decode(dev, kv_heads, "e2m3_as_bf16", g1_cfg)
    assert len(tok6) >= 40 and tok6 == tok16
    assert acc6 == acc16 and len(acc6) > 1
    assert torch.equal(probs6.view(torch.int32), probs16.view(torch.int32)) and float(probs6.sum()) > 0
    assert all(isinstance(w, ops.PackedQ6) for d in m6._packed for w in d.values())
    assert not isinstance(m6._packed_head, ops.PackedQ6) and not any(isinstance(w, ops.PackedQ6) for d in m16._packed for w in d.values())
    if g1_cfg is None:
        assert m6.G1_CFG == m6.G1_CFG_EMU3_Q4 == m16.G1_CFG
    assert m6.packed_bytes(head=False) * 32 == m16.packed_bytes(head=False) * 12.5          # 6.25 bits per weight against 16
    assert m6.packed_bytes() - m6.packed_bytes(head=False) == m16.packed_bytes() - m16.packed_bytes(head=False) > 0      # the head is not quantised
    st = m6.compress_stats
    assert st["q6_matrices"] == 8 and st["q6_bytes_packed"] == m6.packed_bytes(head=False) and 2.0 ** -7 < st["rel_rms_error"] < 0.04
    assert m16.compress_stats["rel_rms_error"] == st["rel_rms_error"] and "q6_bytes_packed" not in m16.compress_stats and "q4_matrices" not in st


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
    import sjd_amd.launch_shapes as LS
    import sjd_amd.ops as ops
    from sjd_amd.engine_batch import SJDBatchEngine
    m6, out6, probs6 = _decode_two(dev, "e2m3")
    m16, out16, probs16 = _decode_two(dev, "e2m3_as_bf16")
    assert isinstance(m6._packed[0]["gate_up"], ops.PackedQ6) and not isinstance(m16._packed[0]["gate_up"], ops.PackedQ6)
    for i in range(2):
        assert len(out6[i][0]) >= 42 and out6[i][0] == out16[i][0], f"prompt {i}: tokens differ"
        assert out6[i][1] == out16[i][1] and len(out6[i][1]) > 1, f"prompt {i}: acceptance counts differ"
    assert out6[0][0] != out6[1][0]
    assert torch.equal(probs6.view(torch.int32), probs16.view(torch.int32)) and float(probs6.sum()) > 0
    for m in (m6, m16):          # 3 prompts x 2 x 16 = 96 rows: refused when the engine is built, and by the backbone before its first launch
        assert LS.serves_rows(m, 64) is None and LS.serves_rows(m, 65) == ("max_rows", 64)
        with pytest.raises(ValueError, match="at most 64 window rows"):
            SJDBatchEngine(m, TOY["vocab_size"], dev, n_prompts=3)
        m.setup_cache(batch=8, s_max=64)
        with pytest.raises(ValueError, match="at most 64 rows"):
            m.forward_window(torch.zeros(8, 16, dtype=torch.long, device=dev), torch.zeros(8, 16, dtype=torch.long, device=dev), 0,
                             torch.zeros(8, dtype=torch.int32, device=dev))
