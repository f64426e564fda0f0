"""GPU: kernel G1p (ops.prefill_gemm: the prefill projection over the packed e4m3 / MXFP4 / plain copies at any row count) and
ChameleonBackbone.enable_fused(..., release_16bit=True), which runs the prompt prefill on it and releases the 16-bit layer matrices.

A1  per-element bound against fp64: |y - y64| <= 2^-8 |y64| + (K + 2) 2^-23 S with y64 = rs sum x deq, S = rs sum |x deq| (bf16 x bf16 products are exact
    in fp32: the roundings are the fp32 accumulation over K terms, the scale multiply and ONE bf16 rounding -- derived, not measured)
A2  a quantised copy gives the bits of the plain packing of its dequantised matrix
A3  a row's output does not depend on M or on the row's position
A4  nothing is written outside y [M, N]
A5  unsupported shapes return the error code and launch nothing
A6 / A7  toy pre-norm / swin-norm backbones, stream and twin both released: bit-equal KV rows and last-row logits, the same tokens through SJDEngine
A9  what is released, and SJDBatchEngine on a released backbone
A8  one model, measured: window route and packed prefill route against an fp32 torch restatement of the folded forward over dequant()"""
import ctypes

import pytest
import torch

import sjd_amd.launch_shapes as LS

pytestmark = pytest.mark.gpu
RB = LS.PREFILL_ROW_BLOCK
MS = (1, 33, RB - 1, RB, RB + 1, 2 * RB + 7)
# (K, KC, N, gateup): one chunk; a ragged last chunk of whole MXFP4 granules; [Wg; Wu] packed in two K halves
SHAPES = [(128, 128, 32, False), (128, 128, 96, False), (384, 256, 32, False), (384, 256, 96, False), (256, 128, 64, True)]
FORMS = ("e4m3", "mxfp4", "plain")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _weight(N, K, seed, dev):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g)
    w[1] *= 2.0 ** 20          # a few columns far from the rest: the column / block scales differ
    w[N // 2] *= 2.0 ** -20
    w[N - 3, : K // 2] *= 2.0 ** 20
    return w.to(torch.bfloat16).to(dev)


def _pack(form, w, KC, sm, gateup):
    import sjd_amd.ops as ops
    if form == "plain":
        return ops.pack_weight(w, KC, sm), w
    z = (ops.pack_weight_q8 if form == "e4m3" else ops.pack_weight_q4)(w, KC, sm, gateup=gateup)
    return z, z.dequant()


def _run(x, pk, N, K, KC, sm, rs=None):
    import sjd_amd.ops as ops
    return ops.prefill_gemm(x, pk, N, K, rs, KC=KC, step_major=sm)


@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("K,KC,N,gateup", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_a1_a2_a3_bound_bit_identity_and_row_independence(dev, form, K, KC, N, gateup, sm):
    import sjd_amd.ops as ops
    w = _weight(N, K, 7 + K + N, dev)
    pk, deq = _pack(form, w, KC, sm, gateup)
    twin = ops.pack_weight(deq, KC, sm)
    g = torch.Generator().manual_seed(K + 3 * N)
    Mx = MS[-1]
    x = torch.randn(Mx, K, generator=g).to(torch.bfloat16).to(dev)
    rs_all = (0.25 + 4.0 * torch.rand(Mx, generator=g)).to(dev)
    p64 = x.double()[:, None, :] * deq.double()[None, :, :]                                       # [M, N, K]: every product, exact
    for rs in (None, rs_all):
        scale = torch.ones(Mx, dtype=torch.float64, device=dev) if rs is None else rs.double()
        y64, S = scale[:, None] * p64.sum(-1), scale[:, None] * p64.abs().sum(-1)
        bound = 2.0 ** -8 * y64.abs() + (K + 2) * 2.0 ** -23 * S
        full = _run(x, pk, N, K, KC, sm, rs)
        assert full.shape == (Mx, N) and full.dtype == torch.bfloat16
        err = (full.double() - y64).abs()
        print(f"{form} K={K} KC={KC} N={N} sm={sm} rs={rs is not None}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}")
        assert bool((err <= bound).all()), (form, K, KC, N, sm, float((err - bound).max()))       # A1
        assert torch.equal(full.view(torch.int16), _run(x, twin, N, K, KC, sm, rs).view(torch.int16))          # A2
        for M in MS[:-1]:                                                                          # A3: another M, the same rows
            part = _run(x[:M].contiguous(), pk, N, K, KC, sm, None if rs is None else rs[:M].contiguous())
            assert torch.equal(part.view(torch.int16), full[:M].view(torch.int16)), (form, M)
        r = RB + 3                                                                                 # ... and another position: row RB + 3 as row 0 of M = 1
        one = _run(x[r:r + 1].contiguous(), pk, N, K, KC, sm, None if rs is None else rs[r:r + 1].contiguous())
        assert torch.equal(one.view(torch.int16), full[r:r + 1].view(torch.int16))
    torch.cuda.synchronize()


def _lib_call(x, data, y_ptr, M, N, K, KC, sm, code, rs=None):
    import sjd_amd._lib as L
    vp = ctypes.c_void_p
    return L.load().sjd_prefill_gemm(vp(x.data_ptr()), vp(data.data_ptr()), vp(y_ptr), M, N, K, KC, int(sm), code, vp(0 if rs is None else rs.data_ptr()),
                                     vp(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("form", FORMS)
def test_a4_nothing_is_written_outside_y(dev, form, M):
    import sjd_amd._lib as L
    K, KC, N, sm = 384, 256, 96, True
    pk, _ = _pack(form, _weight(N, K, 5, dev), KC, sm, False)
    data, code = (pk, L.DTYPE_BF16) if form == "plain" else (pk.data, L.DTYPE_BF16 | (L.G1_W8_E4M3 if form == "e4m3" else L.G1_W4_MXFP4))
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16).to(dev)
    front, behind = 256, RB * N + 512
    buf = torch.full((front + M * N + behind,), 0x7a5b, dtype=torch.int16, device=dev)
    assert _lib_call(x, data, buf.data_ptr() + 2 * front, M, N, K, KC, sm, code) == 0
    torch.cuda.synchronize()
    assert bool((buf[:front] == 0x7a5b).all()) and bool((buf[front + M * N:] == 0x7a5b).all())
    want = _run(x, pk, N, K, KC, sm)
    assert torch.equal(buf[front:front + M * N].view(M, N), want.view(torch.int16))


def test_a5_unsupported_shapes_return_the_code_and_launch_nothing(dev):
    import sjd_amd._lib as L
    import sjd_amd.ops as ops
    lib = L.load()
    UNSUPPORTED, BAD_ARG = -2, -1
    assert lib.sjd_error_string(UNSUPPORTED) == b"unsupported configuration"
    BF, W8, W4 = L.DTYPE_BF16, L.DTYPE_BF16 | L.G1_W8_E4M3, L.DTYPE_BF16 | L.G1_W4_MXFP4
    buf = torch.zeros(1 << 20, dtype=torch.int16, device=dev)          # input, weight and output alike: a launch would leave something in it
    y = buf.data_ptr()
    for code, K, KC, N in ((W4, 192, 128, 32), (W4, 256, 64, 32), (W4, 256, 192, 32),           # K / KC no multiple of the MXFP4 granule
                           (W8, 144, 128, 32), (W8, 128, 48, 32), (BF, 144, 144, 32), (BF, 128, 16, 32),          # ... of 32
                           (BF, 128, 128, 48), (W8, 128, 128, 16), (W4, 128, 128, 100),         # N % 32 != 0
                           (L.DTYPE_F16, 128, 128, 32), (L.DTYPE_F16 | L.G1_W8_E4M3, 128, 128, 32), (L.DTYPE_F16 | L.G1_W4_MXFP4, 128, 128, 32),
                           (L.DTYPE_F32, 128, 128, 32)):
        assert _lib_call(buf, buf, y, 40, N, K, KC, True, code) == UNSUPPORTED, (code, K, KC, N)
    assert _lib_call(buf, buf, y, 40, 32, 128, 128, True, W8 | L.G1_W4_MXFP4) == BAD_ARG
    assert _lib_call(buf, buf, y, 0, 32, 128, 128, True, BF) == BAD_ARG and _lib_call(buf, buf, 0, 8, 32, 128, 128, True, BF) == BAD_ARG
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0
    # through ops: the library's refusal is an error, never a quiet fall-back
    x = torch.zeros(8, 144, dtype=torch.bfloat16, device=dev)
    with pytest.raises(L.SjdLibraryError, match="unsupported configuration"):
        ops.prefill_gemm(x, ops.pack_weight(torch.zeros(32, 144, dtype=torch.bfloat16, device=dev), 144), 32, 144, KC=144, step_major=False)
    with pytest.raises(L.SjdLibraryError, match="unsupported configuration"):
        ops.prefill_gemm(x.half(), ops.pack_weight(torch.zeros(32, 144, dtype=torch.float16, device=dev), 144), 32, 144, KC=144, step_major=False)


# ------------------------------------------------------------------------------------------------ toy backbones
TOY = dict(vocab_size=9216, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
           max_position_embeddings=512)
TOY_CFG = dict(qkv=(128, 4, True), o=(256, 3, False), gate_up=(128, 8, True), down=(256, 4, False))
SWIN = dict(swin_norm=True, model_parallel_size=2)


def _toy(dev, weights, swin=False, release=True, batch=2, s_max=256):
    import sjd_amd.backbones as BB
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    m = BB.ChameleonBackbone(BB.ChameleonArgs(qk_norm=True, **dict(TOY, **(SWIN if swin else {}))), attn=ops.HipWindowAttention(n_split=2)).eval()
    synthetic.fill_state_dict(m, seed=29, embed_token_scale=0.25)
    g = torch.Generator().manual_seed(1)
    for layer in m.model.layers:          # gains far from one: A8's independent reference shows a gain folded (or not) the wrong way; stream-against-twin cannot
        layer.input_layernorm.weight.data = 1.0 + 0.5 * torch.randn(TOY["hidden_size"], generator=g)
        layer.post_attention_layernorm.weight.data = 1.0 + 0.5 * torch.randn(TOY["hidden_size"], generator=g)
    m = m.to(device=dev, dtype=torch.bfloat16)
    m.G1_CFG = dict(TOY_CFG)
    m.enable_fused(ops, gemm="sjd", weights=weights, swin_quant=swin, release_16bit=release)
    m.setup_cache(batch=batch, s_max=s_max)
    return m


class _Spy:
    """the row counts ops.prefill_gemm / ops.skinny_gemm were called with"""

    def __enter__(self):
        import sjd_amd.ops as ops
        self.ops, self.saved, self.g1p, self.g1 = ops, (ops.prefill_gemm, ops.skinny_gemm), [], []

        def pg(x, *a, **k):
            self.g1p.append(int(x.shape[0]))
            return self.saved[0](x, *a, **k)

        def sg(x, *a, **k):
            self.g1.append(int(x.shape[0]))
            return self.saved[1](x, *a, **k)
        ops.prefill_gemm, ops.skinny_gemm = pg, sg
        return self

    def __exit__(self, *exc):
        self.ops.prefill_gemm, self.ops.skinny_gemm = self.saved


def _prefill(m, P, dev, seed):
    tok = torch.randint(4, 8196, (2, P), generator=torch.Generator().manual_seed(seed)).to(dev)
    pos = torch.stack([torch.arange(P), torch.tensor([1] * (P - 1) + [0])]).to(dev)
    ks = torch.tensor([0, P - 1], dtype=torch.int32, device=dev)
    with torch.no_grad():
        logits = m.forward_window(tok, pos, 0, ks)
    torch.cuda.synchronize()
    return logits.float(), m.cache.k[:, :, :, :P].clone(), m.cache.v[:, :, :, :P].clone()


def _decode(m, dev, P=40, img_len=48, window=16, seed=5):
    import sjd_amd.synthetic as synthetic
    from sjd_amd.engine import SJDEngine, SJDConfig, WindowSpec
    from sjd_amd.grammar import AnoleGrammar
    V = TOY["vocab_size"]
    prompt = torch.cat([synthetic.synthetic_prompt(P - 1, seed, lo=8900, hi=9200), torch.tensor([[8197]])], dim=1)
    max_len = P + img_len + 1
    cfg = SJDConfig(jacobi_loop_interval_l=0, jacobi_loop_interval_r=img_len - window - 2, max_num_new_tokens=window, guidance_scale=3.0,
                    seed=seed, prefix_token_sampler_scheme="speculative_jacobi", max_length=max_len, eos_token_ids=(8196,))
    spec = WindowSpec(first_tokens=prompt.to(dev).repeat(2, 1),
                      first_positions=torch.stack([torch.arange(P), torch.tensor([1] * (P - 1) + [0])]).to(dev),
                      key_start=torch.tensor([0, P - 1], dtype=torch.int32), pos_offset=torch.tensor([0, -(P - 1)], dtype=torch.long), kv_base=0)
    eng = SJDEngine(m, V, dev, max_window=window, use_graph=True)
    seq, stats = eng.decode(prompt[0].tolist(), spec, AnoleGrammar(V, P, max_len, img_len), cfg)
    torch.cuda.synchronize()
    return seq[P:], list(stats.matched)


@pytest.mark.parametrize("swin", [False, True], ids=["a6_pre_norm", "a7_swin_norm"])
@pytest.mark.parametrize("stream", ["e4m3", "mxfp4"])
def test_a6_a7_released_stream_and_twin_agree_bit_for_bit(dev, stream, swin):
    import sjd_amd.ops as ops
    mq, m16 = _toy(dev, stream, swin), _toy(dev, stream + "_as_bf16", swin)
    assert mq.released_16bit and m16.released_16bit and mq._fold_norm == (not swin)
    assert isinstance(mq._packed[1]["down"], ops.PackedQ4 if stream == "mxfp4" else ops.PackedQ8) and isinstance(m16._packed[1]["down"], torch.Tensor)
    for P in (40, 150):          # 80 rows (40 per batch row) and 300 rows: "prefill" by the window rule
        assert LS.serves_rows(mq, 2 * P, P) == ("prefill", None)
        with _Spy() as spy:
            lq, kq, vq = _prefill(mq, P, dev, seed=P)
        assert spy.g1p == [2 * P] * 8 and spy.g1 == []          # four projections x two layers on kernel G1p, nothing else
        l16, k16, v16 = _prefill(m16, P, dev, seed=P)
        assert bool(torch.isfinite(lq).all()) and float(lq.abs().max()) > 0 and float(kq.float().abs().max()) > 0
        assert torch.equal(kq.view(torch.int16), k16.view(torch.int16)) and torch.equal(vq.view(torch.int16), v16.view(torch.int16))
        assert torch.equal(lq[:, -1].view(torch.int32), l16[:, -1].view(torch.int32))
    with _Spy() as spy:
        tok_q, acc_q = _decode(mq, dev)
    assert spy.g1p and min(spy.g1p) > 64 and spy.g1 and max(spy.g1) <= 64          # the prompt on G1p, the windows on the window kernels
    tok_16, acc_16 = _decode(m16, dev)
    assert tok_q == tok_16 and acc_q == acc_16 and len(acc_q) >= 8 and len(tok_q) >= 48


def test_a6_a_65_row_input_is_served_by_a_released_mxfp4_backbone(dev):
    """65..256 rows with at most 32 per batch row: ("max_rows", 64) -- an unreleased MXFP4 backbone refuses it, a released one runs it on G1p"""
    tok = torch.randint(4, 8196, (3, 22), generator=torch.Generator().manual_seed(2)).to(dev)
    pos = torch.arange(22)[None].repeat(3, 1).to(dev)
    ks = torch.zeros(3, dtype=torch.int32, device=dev)
    plain = _toy(dev, "mxfp4", release=False, batch=3)
    assert LS.serves_rows(plain, 66, 22) == ("max_rows", 64)
    with pytest.raises(ValueError, match="at most 64 rows"), torch.no_grad():
        plain.forward_window(tok, pos, 0, ks)
    mq, m16 = _toy(dev, "mxfp4", batch=3), _toy(dev, "mxfp4_as_bf16", batch=3)
    with _Spy() as spy, torch.no_grad():
        a = mq.forward_window(tok, pos, 0, ks).float()
    assert spy.g1p == [66] * 8 and spy.g1 == []
    with torch.no_grad():
        b = m16.forward_window(tok, pos, 0, ks).float()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all()) and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_a9_release_and_the_batch_engine(dev):
    import sjd_amd.backbones as BB
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    from sjd_amd.engine import SJDConfig, WindowSpec
    from sjd_amd.engine_batch import SJDBatchEngine
    from sjd_amd.grammar import LuminaGrammar
    ref = BB.ChameleonBackbone(BB.ChameleonArgs(qk_norm=True, **TOY))
    want = sum(p.numel() * 2 for n_, p in ref.named_parameters() if "_proj" in n_)
    m = _toy(dev, "mxfp4", batch=4, s_max=192)
    projs = list(m._layer_projections())
    assert len(projs) == 14 and all(p.numel() == 0 and p.device.type == "cuda" for p in projs) and not hasattr(m, "_fused")
    assert m.released_16bit and m.compress_stats["bytes_released"] == want
    assert m.lm_head.weight.numel() > 0 and m.model.embed_tokens.weight.numel() > 0 and m.model.layers[0].self_attn.q_norm.weight.numel() > 0
    with pytest.raises(ValueError):
        m.state_dict()
    with pytest.raises(ValueError):
        m.enable_fused(ops, gemm="sjd", weights="mxfp4")
    V, n_prompts, hg, wg, window, seed = TOY["vocab_size"], 2, 3, 3, 8, 3
    n_img = (2 * wg + 1) * 2 * hg
    prompts, specs, lens = [], [], [40, 45]          # 80 / 90 rows at 40 / 45 per batch row: prefill
    for i, Pi in enumerate(lens):
        pr = torch.cat([synthetic.synthetic_prompt(Pi - 3, seed + 17 * i, lo=8900, hi=9200), torch.tensor([[8197, 8804 + hg, 8804 + wg]])], dim=1)
        prompts.append(pr[0].tolist())
        specs.append(WindowSpec(first_tokens=pr.to(dev).repeat(2, 1),
                                first_positions=torch.stack([torch.arange(Pi), torch.tensor([1] * (Pi - 1) + [0])]).to(dev),
                                key_start=torch.tensor([0, Pi - 1], dtype=torch.int32), pos_offset=torch.tensor([0, -(Pi - 1)], dtype=torch.long), kv_base=0))
    cfg = SJDConfig(jacobi_loop_interval_l=3, jacobi_loop_interval_r=n_img - 10, max_num_new_tokens=window, guidance_scale=3.0, seed=seed,
                    prefix_token_sampler_scheme="speculative_jacobi", max_length=1 << 20, eos_token_ids=(8196,))
    eng = SJDBatchEngine(m, V, dev, n_prompts, max_window=window, use_graph=True)
    with _Spy() as spy:
        results = eng.decode_many(prompts, specs, [LuminaGrammar(2000, 10) for _ in range(n_prompts)], cfg)
    torch.cuda.synchronize()
    assert spy.g1p and min(spy.g1p) > 64 and spy.g1 and max(spy.g1) <= 32
    for (seq, st), p in zip(results, prompts):
        assert list(seq[:len(p)]) == p and len(seq) > len(p) and len(st.matched) > 1


# ------------------------------------------------------------------------------------------------ A8: one model, measured
def _reference_logits(m, tok, pos):
    """fp32 torch restatement of the FOLDED pre-norm forward over the packed copies' dequant() (which hold W diag(gamma)): the projections run on the residual
    stream, rsqrt(mean h^2 + eps) scales their fp32 sums; QK-norm, rotary and causal attention as modeling_chameleon; nothing is rounded to 16 bits.
    Independent of ops.prefill_gemm, of the routing code and of every kernel.  tok, pos [B, n]; empty cache, no hidden keys -> [B, n, V] fp32"""
    a, eps = m.args, m.args.rms_norm_eps
    H, D, hid, inter = m.n_heads, m.head_dim, a.hidden_size, a.intermediate_size
    assert m.n_kv_heads == H and a.model_parallel_size == 1 and m._fold_norm
    B, n = tok.shape
    h = m.model.embed_tokens.weight.float()[tok]                                                   # [B, n, hid]
    fr = pos[:, :, None].float() * m.inv_freq.float()[None, None, :]
    emb = torch.cat([fr, fr], dim=-1)
    cos, sin = emb.cos()[:, :, None, :], emb.sin()[:, :, None, :]
    rot = lambda x: torch.cat([-x[..., D // 2:], x[..., :D // 2]], dim=-1)
    rs = lambda x: torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    causal = torch.ones(n, n, dtype=torch.bool, device=tok.device).tril()
    for li, layer in enumerate(m.model.layers):
        W = {k: v.dequant().float() for k, v in m._packed[li].items()}
        at = layer.self_attn
        q, k, v = ((h @ W["qkv"].T) * rs(h)).view(B, n, 3, H, D).unbind(2)
        ln = lambda x, nm: torch.nn.functional.layer_norm(x, (D,), None, None, 1e-5) * nm.weight.float()[0] + nm.bias.float()[0]
        q, k = ln(q, at.q_norm), ln(k, at.k_norm)
        q, k = q * cos + rot(q) * sin, k * cos + rot(k) * sin
        sc = torch.einsum("bihd,bjhd->bhij", q, k) / D ** 0.5
        p = sc.masked_fill(~causal, float("-inf")).softmax(-1)
        h = h + torch.einsum("bhij,bjhd->bihd", p, v).reshape(B, n, H * D) @ W["o"].T
        g, u = ((h @ W["gate_up"].T) * rs(h)).split(inter, dim=-1)
        h = h + (torch.nn.functional.silu(g) * u) @ W["down"].T
    return (h * rs(h) * m.model.norm.weight.float()) @ m.lm_head.weight.float().T


A8_SEEDS = (11, 12, 13, 14, 15)
# max |prefill route - reference| / max |window route - reference| over the logits, measured on one MI355X for A8_SEEDS (profiles/prefill_quant.json, "a8"):
A8_RATIOS = dict(e4m3=(1.0, 1.0, 1.0, 1.0, 1.0), mxfp4=(1.0, 1.0, 1.0, 1.0, 1.0))
# the same for the MEAN absolute error (the logits are bf16 numbers: the largest error sits on one rounding step, the mean sees every logit)
A8_RATIOS_MEAN = dict(e4m3=(0.9957, 1.0, 1.0, 1.0, 1.0), mxfp4=(1.0, 1.0029, 1.0, 1.0, 1.0))
A8_MARGIN = {k: 2.0 * max(v) for k, v in A8_RATIOS.items()}          # twice the largest ratio seen
A8_MARGIN_MEAN = {k: 2.0 * max(v) for k, v in A8_RATIOS_MEAN.items()}


def a8_errors(dev, stream, seed):
    """(max-abs logit error of the window route, of the packed prefill route called directly) against _reference_logits: 16-token prompt, CFG batch 2"""
    m = _toy(dev, stream)
    tok = torch.randint(4, 8196, (2, 16), generator=torch.Generator().manual_seed(seed)).to(dev)
    pos = torch.arange(16)[None].repeat(2, 1).to(dev)
    ks = torch.zeros(2, dtype=torch.int32, device=dev)
    assert LS.serves_rows(m, 32, 16) is None
    with torch.no_grad():
        ref = _reference_logits(m, tok, pos)
        with _Spy() as spy:
            win = m.forward_window(tok, pos, 0, ks).float()
        assert spy.g1p == [] and (spy.g1 or True)
        with _Spy() as spy:
            pre = m._forward_prefill_packed(tok, pos, 0, ks).float()
        assert spy.g1p == [32] * 8 and spy.g1 == []
    torch.cuda.synchronize()
    assert ref.shape == win.shape == pre.shape == (2, 16, TOY["vocab_size"]) and bool(torch.isfinite(ref).all())
    return dict(win=float((win - ref).abs().max()), pre=float((pre - ref).abs().max()), amax=float(ref.abs().max()),
                win_mean=float((win - ref).abs().mean()), pre_mean=float((pre - ref).abs().mean()))


@pytest.mark.parametrize("stream", ["e4m3", "mxfp4"])
def test_a8_prefill_route_and_window_route_are_one_model(dev, stream):
    """Both routes against the fp32 restatement (never against G1p).  The window route's error is the yardstick: the prefill route rounds its projections to
    bf16 before the residual adds where the window route adds fp32 planes, so it may be further off -- but only by A8_MARGIN, twice the largest
    ratio measured over the five seeds (max-abs, as planned, and mean-abs next to it).  Measured on one MI355X: every max-abs ratio 1.0000, the mean-abs
    ratios 0.9957 .. 1.0029 (A8_RATIOS / A8_RATIOS_MEAN above) -- the routes round alike: F1r too rounds a projection to bf16 before the residual add, F2 / F3
    round rs * sum once; what differs is the split-K summation order and the row scale's last bit.  A wrong row scale, a gain applied twice or a
    residual in the wrong place moves the logits by a large fraction of their range."""
    for seed in A8_SEEDS:
        e = a8_errors(dev, stream, seed)
        print(f"a8 {stream} seed {seed}: max-abs window {e['win']:.5f} prefill {e['pre']:.5f} ratio {e['pre'] / e['win']:.4f}; mean-abs window {e['win_mean']:.6f} "
              f"prefill {e['pre_mean']:.6f} ratio {e['pre_mean'] / e['win_mean']:.4f} (max |logit| {e['amax']:.2f})")
        assert 0 < e["win"] < 0.05 * e["amax"] and 0 < e["win_mean"], e          # the yardstick itself is a small fraction of the logits' range
        assert e["pre"] <= A8_MARGIN[stream] * e["win"], (stream, seed, e)
        assert e["pre_mean"] <= A8_MARGIN_MEAN[stream] * e["win_mean"], (stream, seed, e)
