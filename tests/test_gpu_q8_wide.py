"""GPU: several prompts per forward from 8-bit (OCP e4m3fn) weights -- kernel G1wq, the 8-bit form of G1w (csrc/sjd_gemm_wide.h, template
parameter Q) behind SJD_G1_W8_E4M3 at 65..256 rows, ChameleonBackbone.enable_fused(weights="e4m3", max_rows=128 / 256) and SJDBatchEngine on
such a backbone.  Nothing here has a tolerance: the kernel rebuilds the bf16 MFMA operand q * scale bit for bit and runs G1w's MFMA sequence,
so every result is compared BIT FOR BIT with the uncompressed kernels on PackedQ8.dequant() / with the "e4m3_as_bf16" twin."""
import ctypes

import pytest
import torch

from tests.test_gpu_q8 import TOY, UNSUPPORTED, W8, check_codes, q8_weight

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from tests.conftest import poison_device_memory
    poison_device_memory(total_gib=1)          # the planes come from torch.empty: an unwritten element must not read as zero
    return "cuda:0"


G1WQ_CASES = [(65, 96, 128, 64, 3, False),              # first row past 64, one stage per chunk
              (96, 192, 352, 96, 6, True),              # two tiles per wave, six-step chunks that pad a stage, ragged last chunk
              (128, 160, 1408, 1408, 4, True),          # a workgroup with missing tiles, 88 steps
              (128, 64, 256, 128, 2, False),            # four row tiles with two tiles
              (129, 256, 512, 256, 8, True),            # XCD map (fewer than eight workgroups: its tail branch), two chunks
              (160, 288, 1024, 128, 3, False),          # eight chunks: whole rounds of eight workgroups
              (200, 128, 2048, 128, 2, True),           # sixteen chunks, whole rounds of eight
              (256, 512, 1152, 384, 8, True),           # three chunks: plain map, the register-heaviest form
              (256, 64, 64, 32, 2, False),              # chunks shorter than the weight ring
              (130, 288, 512, 128, 2, True)]            # XCD map with four chunks: two column groups per XCD and a tail of four workgroups


@pytest.mark.parametrize("M,N,K,KC,tiles,step_major", G1WQ_CASES)
def test_g1wq_planes_are_g1w_on_the_dequantised_weight(dev, M, N, K, KC, tiles, step_major):
    import sjd_amd.ops as ops
    w = q8_weight(N, K, N + K + M, dev)
    pq = ops.pack_weight_q8(w, KC, step_major)
    check_codes(pq)
    wp = ops.pack_weight(pq.dequant(), KC, step_major)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16).to(dev)
    ref = ops.skinny_gemm(x, wp, N, K, KC, tiles, step_major).data
    got = ops.skinny_gemm(x, pq, N, K, KC, tiles, step_major).data
    torch.cuda.synchronize()
    assert got.shape == ref.shape == ((K + KC - 1) // KC, 32 * ((M + 31) // 32), N)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (got - ref).abs().max()          # the whole planes, padding rows included
    assert float(ref.abs().max()) > 0
    if M % 32:
        assert float(got[:, M:].abs().max()) == 0
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.skinny_gemm(x, pq, N, K, KC, tiles, step_major)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        cap = ops.skinny_gemm(x, pq, N, K, KC, tiles, step_major).data
    cap.fill_(float("nan"))
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap.view(torch.int32), ref.view(torch.int32))


def test_g1wq_column_window(dev):
    import sjd_amd.ops as ops
    M, NP, K, KC, c0, nc = 160, 512, 512, 256, 64, 352
    w = q8_weight(NP, K, 78, dev)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).to(dev)
    for sm, tiles in ((True, 4), (False, 6)):
        pq = ops.pack_weight_q8(w, KC, sm)
        full = ops.skinny_gemm(x, pq, NP, K, KC, tiles, sm).data
        ref = ops.skinny_gemm_cols(x, ops.pack_weight(pq.dequant(), KC, sm), NP, K, KC, c0, nc, tiles, sm).data
        got = ops.skinny_gemm_cols(x, pq, NP, K, KC, c0, nc, tiles, sm).data          # (tile0 = 2; the scales still sit at byte N_packed * K)
        torch.cuda.synchronize()
        assert got.shape == (2, 160, nc) and torch.equal(got.view(torch.int32), full[:, :, c0:c0 + nc].contiguous().view(torch.int32))
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)) and float(ref.abs().max()) > 0


def test_c_boundary_refusals_above_64_rows(dev):
    """with the bit set, what G1wq does not serve comes back as SJD_ERR_UNSUPPORTED before any launch"""
    import sjd_amd._lib as L
    lib = L.load()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    bf = L.DTYPE_BF16 | W8
    # sjd_skinny_gemm(x, w_packed, out, M, N, K, KC, waves, step_major, dtype, stream)
    for waves in (1, 5, 16):
        assert lib.sjd_skinny_gemm(p, p, p, 65, 32, 64, 64, waves, 0, bf, None) == UNSUPPORTED
        assert lib.sjd_skinny_gemm_cols(p, p, p, 65, 32, 64, 64, waves, 0, bf, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm(p, p, p, 70, 64, 64, 64, 2, 0, bf, None) == UNSUPPORTED               # three row tiles x two tiles: no G1w form
    assert lib.sjd_skinny_gemm(p, p, p, 70, 64, 48, 32, 3, 0, bf, None) == UNSUPPORTED               # K = 48: a half record
    assert lib.sjd_skinny_gemm(p, p, p, 70, 64, 96, 48, 3, 0, bf, None) == UNSUPPORTED               # KC = 48
    assert lib.sjd_skinny_gemm_cols(p, p, p, 200, 32, 96, 48, 4, 1, bf, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm(p, p, p, 70, 64, 64, 64, 3, 0, L.DTYPE_F16 | W8, None) == UNSUPPORTED  # fp16
    assert lib.sjd_skinny_gemm_cols(p, p, p, 256, 32, 64, 64, 4, 0, L.DTYPE_F16 | W8, 64, 0, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


def _window(dev, B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(4, 8196, (B, n), generator=g).to(dev), torch.arange(n)[None].repeat(B, 1).to(dev), 0,
            torch.zeros(B, dtype=torch.int32, device=dev))


@pytest.fixture(scope="module", params=[4, 2], ids=["mha", "gqa"])
def toy_pair(dev, request):
    """the toy Chameleon of tests/test_gpu_q8.py packed with max_rows=256, as "e4m3" and as its bf16 twin"""
    import sjd_amd.ops as ops
    from tests.helpers import make_chameleon
    out = []
    for wt in ("e4m3", "e4m3_as_bf16"):
        m = make_chameleon(dict(TOY, num_key_value_heads=request.param), 29, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=dev)
        m.enable_fused(ops, gemm="sjd", weights=wt, max_rows=256)
        assert m.max_rows == 256 and m.G1_CFG == (m.G1_CFG_EMU3_Q8_WIDE if request.param != 4 else m.G1_CFG_Q8_WIDE)
        m.setup_cache(batch=16, s_max=64)
        out.append(m)
    return out


@pytest.mark.parametrize("B,n", [(6, 16), (8, 16), (10, 16), (16, 16), (1, 16), (3, 16)], ids=lambda v: str(v))
def test_window_logits_equal_the_twins(dev, toy_pair, B, n):
    """96, 128, 160 and 256 rows (G1wq against G1w), and 16 and 48 rows (G1q / G1sq) on the SAME packed copy"""
    import sjd_amd.ops as ops
    m8, m16 = toy_pair
    assert all(isinstance(w, ops.PackedQ8) for d in m8._packed for w in d.values())
    assert not any(isinstance(w, (ops.PackedQ8, ops.PackedZ)) for d in m16._packed for w in d.values())
    assert isinstance(m8._packed_head, torch.Tensor) and isinstance(m16._packed_head, torch.Tensor)      # max_rows=256: the head is packed uncompressed
    args = _window(dev, B, n, B)
    with torch.no_grad():
        outs = [m.forward_window(*args).float() for m in (m8, m16)]
    torch.cuda.synchronize()
    assert outs[0].shape == (B, n, 9216) and bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert m8.packed_bytes(head=False) <= 0.52 * m16.packed_bytes(head=False) and m8.compress_stats["q8_bytes_packed"] == m8.packed_bytes(head=False)


@pytest.fixture(scope="module")
def real_width_pair(dev):
    """one Lumina-7B-wide layer (hidden 4096, 32 heads of 128, intermediate 11008) on the default wide set, as "e4m3" and as its bf16 twin"""
    import sjd_amd.backbones as BB
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    args = BB.ChameleonArgs(vocab_size=9216, hidden_size=4096, intermediate_size=11008, num_hidden_layers=1, num_attention_heads=32,
                            num_key_value_heads=32, max_position_embeddings=512)
    out = []
    for wt in ("e4m3", "e4m3_as_bf16"):
        with torch.device(dev):
            m = BB.ChameleonBackbone(args, attn=ops.HipWindowAttention(n_split=2)).to(torch.bfloat16).eval()
        synthetic.fill_state_dict_device(m, seed=7, embed_token_scale=0.25)
        m.enable_fused(ops, gemm="sjd", weights=wt, max_rows=256)
        assert m.G1_CFG == m.G1_CFG_Q8_WIDE
        m.setup_cache(batch=16, s_max=64)
        out.append(m)
    return out


@pytest.mark.parametrize("B", [8, 16])
def test_real_width_window_of_128_and_256_rows(dev, real_width_pair, B):
    m8, m16 = real_width_pair
    assert m8._q8_chunk("down", 16 * B, 11008) == 1408 == m16._q8_chunk("down", 16 * B, 11008) and m8._q8_chunk("down", 64, 11008) == 704
    args = _window(dev, B, 16, 100 + B)
    with torch.no_grad():
        outs = [m.forward_window(*args).float() for m in (m8, m16)]
    torch.cuda.synchronize()
    assert outs[0].shape == (B, 16, 9216) and bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def _decode_many(dev, weights, n_prompts, hg=3, wg=3, window=16, seed=3):
    """n_prompts Lumina-grammar images of distinct prompt lengths through SJDBatchEngine (window 16, CFG) on the toy backbone"""
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    from sjd_amd.engine import SJDConfig, WindowSpec
    from sjd_amd.engine_batch import SJDBatchEngine
    from sjd_amd.grammar import LuminaGrammar
    from tests.helpers import make_chameleon
    V = TOY["vocab_size"]
    model = make_chameleon(dict(TOY, num_key_value_heads=4), 23, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=dev)
    model.enable_fused(ops, gemm="sjd", weights=weights, max_rows=128 if n_prompts * 2 * window <= 128 else 256)
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
    assert rows and max(rows) == n_prompts * 2 * window, "the window forward did not run on the hand-written projections at its full row count"
    return model, [(seq[len(p):], list(st.matched)) for (seq, st), p in zip(results, prompts)], eng.probs_all.clone()


@pytest.mark.parametrize("n_prompts", [3, 5, 8])
def test_batch_engine_tokens_agree_with_the_bf16_twin(dev, n_prompts):
    import sjd_amd.ops as ops
    m8, out8, probs8 = _decode_many(dev, "e4m3", n_prompts)
    m16, out16, probs16 = _decode_many(dev, "e4m3_as_bf16", n_prompts)
    assert isinstance(m8._packed[0]["qkv"], ops.PackedQ8) and not isinstance(m16._packed[0]["qkv"], ops.PackedQ8)
    for i in range(n_prompts):
        assert len(out8[i][0]) >= 42 and out8[i][0] == out16[i][0], f"prompt {i}: tokens differ"
        assert out8[i][1] == out16[i][1] and len(out8[i][1]) > 1, f"prompt {i}: acceptance counts differ"
    assert len({tuple(o[0]) for o in out8}) == n_prompts          # the prompts are distinct, and so are their images
    assert torch.equal(probs8.view(torch.int32), probs16.view(torch.int32)) and float(probs8.sum()) > 0


def test_python_refusals_with_max_rows(dev):
    import sjd_amd.ops as ops
    from sjd_amd.engine_batch import SJDBatchEngine
    from tests.helpers import make_chameleon
    mk = lambda: make_chameleon(dict(TOY, num_key_value_heads=4), 29, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=dev)
    untouched = lambda m: getattr(m, "weights", None) is None and getattr(m, "_ops", None) is None and "max_rows" not in m.__dict__
    m = mk()
    with pytest.raises(ValueError, match="max_rows"):
        m.enable_fused(ops, gemm="sjd", max_rows=128)                       # max_rows without weights
    with pytest.raises(ValueError, match="64, 128 or 256"):
        m.enable_fused(ops, gemm="sjd", weights="e4m3", max_rows=100)
    assert untouched(m)
    for bad, what in ((dict(m.G1_CFG_Q8_WIDE, o=(512, 5, True)), "column tiles"),                 # not a wide tile count
                      (dict(m.G1_CFG_Q8_WIDE, o=(512, 2, True)), "column tiles"),                 # no form at 65..96 rows
                      (dict(m.G1_CFG_Q8_WIDE, down=(48, 4, True)), "multiples of 32")):
        m = mk()
        m.G1_CFG = bad
        with pytest.raises(ValueError, match=what):
            m.enable_fused(ops, gemm="sjd", weights="e4m3", max_rows=256)
        assert untouched(m) and m.G1_CFG == bad
    # a chunk the 64-row kernel cannot read: tile-major, so halved chunks do not fit it (hidden 4096: the chunk is shorter than K)
    m = make_chameleon(dict(TOY, num_key_value_heads=4, hidden_size=4096, num_attention_heads=32, num_hidden_layers=1), 29, 0.25,
                       ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=dev)
    m.G1_CFG = dict(m.G1_CFG_Q8_WIDE, gate_up=(2048, 8, False))
    with pytest.raises(ValueError, match="<= 1280"):
        m.enable_fused(ops, gemm="sjd", weights="e4m3", max_rows=128)
    assert untouched(m)
    m.enable_fused(ops, gemm="sjd", weights="e4m3")          # (without max_rows it packs, as before: 32 rows are served)
    assert m.max_rows == 64
    m = mk()
    m.HEAD_CFG = (1024, 5, True)
    with pytest.raises(ValueError, match="HEAD_CFG"):
        m.enable_fused(ops, gemm="sjd", weights="e4m3", max_rows=256)
    assert untouched(m)
    m = mk().enable_fused(ops, gemm="sjd", weights="e4m3", max_rows=128)
    m.setup_cache(batch=16, s_max=64)
    with pytest.raises(ValueError, match="max_rows=128"):                   # a window taller than max_rows
        m.forward_window(*_window(dev, 10, 16, 1))
    with pytest.raises(ValueError, match=r"weights='e4m3', max_rows=256"):
        SJDBatchEngine(m, 9216, dev, n_prompts=5)
    SJDBatchEngine(m, 9216, dev, n_prompts=4)                                 # 128 rows: served
