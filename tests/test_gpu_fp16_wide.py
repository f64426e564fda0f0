"""fp16 draft windows of 129..256 rows on the HIP path (five to eight prompts per forward in fp16).

  1. kernel G1w's fp16 forms with five to eight row tiles, every fp32 split-K plane against an fp64 product of the same chunk;
  2. the column-window entry (the output head) in fp16 at 256 rows with tile0 > 0;
  3. F1p, F2 (table rotary: bit for bit against the ATen rotary; QK-norm form: fp64 rounding model) and F3 in fp16 at 129 and 256 rows
     from split-K planes;
  4. LlamaGen's window forward at GPT-B width, 256 rows, eight slots with their own KV lengths, against the ATen fp16 and fp32 forwards;
  5. LlamaGenSolver.generate with eight class labels on an fp16 toy model: every prompt bit for bit what the same engine gives it alone;
  6. a Chameleon-shaped fp16 backbone, three slots x window 32 x CFG = 192 rows, teacher-forced against the oracle replay of every slot.

Bounds.  (1, 2) fp16 x fp16 products are exact in fp32, so only the accumulation of a plane's n = chunk-length terms rounds:
|err| <= 2 n 2^-24 sum_k |x_k w_k| (the factor 2 covers the MFMA's internal summation order).  The bf16 G1w tests
(tests/test_gpu_glue.py) state a looser quantity for the chunk SUM (atol = rtol = 2e-3 against an fp32 matmul), not a per-plane bound, so
the per-plane bound above is the one used here.  (3) every 16-bit rounding of the kernel is one rounding of the model, evaluated in fp64
in between; a rounding that falls the other way (fp32 against fp64 in front of it) moves its value by at most one fp16 ulp
(<= 2^-10 |value|, 2^-24 for subnormals), and the bound is the sum of those over the rounding points behind an element.
(4) the rule of tests/test_gpu_llamagen_batch.py::test_real_width_forward_many_rows: hip-to-fp32 error at most 1.5 x aten16-to-fp32.
"""
import pytest
import torch

import sjd_amd._lib as L
import sjd_amd.backbones as BB
import sjd_amd.ops as ops
from tests.helpers import make_llamagen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16
ULP = 2.0 ** -10          # relative spacing of fp16
TINY = 2.0 ** -24         # its subnormal spacing


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ 1. / 2. G1w planes
_G1_REF = {}


def _g1_case(M, N, K):
    """inputs of a shape and their exact per-chunk references, computed once per (M, N, K, KC) and left alone"""
    key = (M, N, K)
    if key not in _G1_REF:
        g = torch.Generator().manual_seed(M * 7 + N + K)
        x = torch.randn(M, K, generator=g).to(F16).to(DEV)
        w = (torch.randn(N, K, generator=g) / K ** 0.5).to(F16).to(DEV)
        _G1_REF[key] = (x, w, {})
    return _G1_REF[key]


def _chunk_refs(M, N, K, KC):
    x, w, refs = _g1_case(M, N, K)
    if KC not in refs:
        xd, wd = x.double(), w.double()
        out = []
        for k0 in range(0, K, KC):
            k1 = min(K, k0 + KC)
            out.append((xd[:, k0:k1] @ wd[:, k0:k1].t(), xd[:, k0:k1].abs() @ wd[:, k0:k1].abs().t(), k1 - k0))
        refs[KC] = out
    return x, w, refs[KC]


def _check_planes(planes, refs, M, cols=slice(None)):
    worst = 0.0
    for c, (exact, mag, n) in enumerate(refs):
        err = (planes[c, :M].double() - exact[:, cols]).abs()
        bound = 2.0 * n * 2.0 ** -24 * mag[:, cols]
        worst = max(worst, float((err / bound.clamp_min(1e-30)).max()))
        assert bool((err <= bound).all()), f"plane {c}: max err / bound = {float((err / bound.clamp_min(1e-30)).max()):.3f}"
    return worst


@pytest.mark.parametrize("tiles,step_major", [(2, True), (3, False), (4, True), (6, False), (8, True), (8, False)])
@pytest.mark.parametrize("N,K", [(224, 512), (512, 528)], ids=["N7tiles-K512", "N512-K528"])
@pytest.mark.parametrize("M", [129, 160, 161, 200, 256])
def test_g1w_fp16_planes(M, N, K, tiles, step_major):
    """rows: the first row of a fifth tile, a full tile edge, one past it, a ragged middle, the limit; N = 32 x 7 leaves a workgroup of 2, 3,
    4, 6 or 8 column tiles without a full set; K = 512 / KC = 256: two whole chunks, K = 528: a ragged third one (one k-step).  The planes are
    poisoned first: every element of rows < M must be written."""
    KC = 256
    x, w, refs = _chunk_refs(M, N, K, KC)
    wp = ops.pack_weight(w, KC, step_major)
    nc = (K + KC - 1) // KC
    torch.full((2 * nc * 256 * N,), float("nan"), device=DEV)          # (freed at once: the allocator hands the block to the planes)
    part = ops.skinny_gemm(x, wp, N, K, KC, waves=tiles, step_major=step_major)
    torch.cuda.synchronize()
    assert part.n_chunks == nc and tuple(part.data.shape) == (nc, ((M + 31) // 32) * 32, N)
    assert torch.isfinite(part.data[:, :M]).all()
    worst = _check_planes(part.data, refs, M)
    print(f"g1w fp16 M={M} N={N} K={K} tiles={tiles} step_major={step_major}: max err / bound {worst:.3f}")


@pytest.mark.parametrize("tiles,step_major", [(4, True), (8, False)])
def test_g1w_fp16_column_window_256_rows(tiles, step_major):
    """the head path: columns [32 * tile0, 32 * tile0 + n_cols) of a weight packed with more columns, 256 rows of fp16"""
    M, N_packed, K, KC, col0, n_cols = 256, 512, 528, 256, 96, 224
    x, w, refs = _chunk_refs(M, N_packed, K, KC)
    wp = ops.pack_weight(w, KC, step_major)
    torch.full((2 * 3 * 256 * n_cols,), float("nan"), device=DEV)
    part = ops.skinny_gemm_cols(x, wp, N_packed, K, KC, col0, n_cols, waves=tiles, step_major=step_major)
    torch.cuda.synchronize()
    assert tuple(part.data.shape) == (3, 256, n_cols)
    worst = _check_planes(part.data, refs, M, cols=slice(col0, col0 + n_cols))
    print(f"g1w fp16 column window tiles={tiles}: max err / bound {worst:.3f}")


def test_g1_refuses_mixed_16bit_types():
    """activation and packed weight of different 16-bit types would multiply garbage: refused by the wrappers, at any row count"""
    x, w, _ = _chunk_refs(256, 224, 512, 256)
    wp = ops.pack_weight(w.to(torch.bfloat16), 256, True)
    for rows in (32, 256):
        with pytest.raises(L.SjdLibraryError, match="packed from"):
            ops.skinny_gemm(x[:rows].contiguous(), wp, 224, 512, 256, waves=4, step_major=True)
    with pytest.raises(L.SjdLibraryError, match="packed from"):
        ops.skinny_gemm_cols(x, wp, 224, 512, 256, 32, 64, waves=4, step_major=True)


# ------------------------------------------------------------------------------------------------ 3. the glue kernels from planes
def _planes(rows, ncol, n_chunks, g, scale=1.0):
    p = torch.zeros(n_chunks, ops._prows(rows), ncol, device=DEV)
    p[:, :rows] = torch.randn(n_chunks, rows, ncol, generator=g, device=DEV) * scale
    return p


def _seq_sum(planes, n):
    acc = planes[0].clone()
    for c in range(1, n):
        acc = acc + planes[c]
    return acc


def _r16(t):
    """one fp16 rounding of an fp64 value, back in fp64"""
    return t.to(F16).double()


def _ulp(t):
    return ULP * t.abs() + TINY


@pytest.mark.parametrize("rows", [129, 256])
@pytest.mark.parametrize("hidden,n_chunks", [(768, 3), (4096, 2)])
def test_f1p_fp16_many_rows(rows, hidden, n_chunks):
    """F1 from planes: h' = fp16(h + fp16(sum of planes)) bit for bit; y = fp16(w * fp16(h' * rsqrt(mean(h'^2) + eps))) -- two roundings behind
    an element (the inner one scaled by |w|)"""
    g = torch.Generator(device=DEV).manual_seed(rows + hidden)
    h = torch.randn(rows, hidden, generator=g, device=DEV).to(F16)
    planes = _planes(rows, hidden, n_chunks, g, 0.5)
    w = (1 + 0.1 * torch.randn(hidden, generator=g, device=DEV)).to(F16)
    h1 = h.clone()
    y = ops.add_rmsnorm(h1, ops.Partials(planes, n_chunks, hidden), w, 1e-5)
    torch.cuda.synchronize()
    delta = _seq_sum(planes[:, :rows], n_chunks).to(F16)
    href = (h.float() + delta.float()).to(F16)
    assert torch.equal(_bits(h1), _bits(href))
    hd = href.double()
    inner = hd * torch.rsqrt(hd.pow(2).mean(-1, keepdim=True) + 1e-5)
    model = _r16(w.double() * _r16(inner))
    bound = w.double().abs() * _ulp(inner) + _ulp(model)
    err = (y.double() - model).abs()
    print(f"f1p fp16 rows={rows} hidden={hidden}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("rows", [129, 256])
def test_f3_fp16_many_rows(rows):
    """F3 from planes: y = fp16(fp16(silu(g)) * u) with g, u = fp16(sum of planes) -- two roundings (the inner one scaled by |u|)"""
    inter, n_chunks = 1408, 3
    g = torch.Generator(device=DEV).manual_seed(rows)
    planes = _planes(rows, 2 * inter, n_chunks, g)
    y = ops.silu_mul(ops.Partials(planes, n_chunks, 2 * inter), rows=rows, dtype=F16)
    torch.cuda.synchronize()
    gu = _seq_sum(planes[:, :rows], n_chunks).to(F16).double()
    gate, up = gu[:, :inter], gu[:, inter:]
    silu = gate / (1 + torch.exp(-gate))
    model = _r16(_r16(silu) * up)
    bound = up.abs() * _ulp(silu) + _ulp(model)
    err = (y[:rows].double() - model).abs()
    assert tuple(y.shape)[-1] == inter
    print(f"f3 fp16 rows={rows}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("H", [4, 6], ids=["rows_kernel", "one_head_kernel"])
@pytest.mark.parametrize("B,n", [(3, 43), (2, 128)], ids=["129rows", "256rows"])
@pytest.mark.parametrize("D", [64, 128])
def test_f2_rope_table_fp16_many_rows_bit_exact(D, B, n, H, cls=120, grid=4, S=512, kv_len=150):
    """F2's table rotary from planes (tests/test_gpu_llamagen_batch.py::_f2_many, fp16 at 129 and 256 rows): q and the appended cache rows are
    the ATen rotary's (_apply_rope_interleaved) bit for bit, v a plain copy, every other cache row untouched"""
    rows = B * n
    g = torch.Generator(device=DEV).manual_seed(D + rows + H)
    freqs = BB._rope_2d_table(grid, D, 10000, cls).to(DEV)
    table = BB._rope_table_extended(freqs, S)
    pos = torch.stack([torch.arange(s0, s0 + n) for s0 in [120 - n // 2, 130, 120 - n // 2][:B]]).to(DEV)
    N = 3 * H * D
    part = torch.randn(3, ops._prows(rows), N, generator=g, device=DEV)
    x = ((part[0] + part[1]) + part[2])[:rows].to(F16)
    kc = torch.full((B, H, S, D), 7.0, dtype=F16, device=DEV)
    vc = torch.full((B, H, S, D), -3.0, dtype=F16, device=DEV)
    q = ops.qknorm_rope_append(ops.Partials(part, 3, N), kc, vc, None, None, None, None, None, pos.reshape(-1).contiguous(), B, n, H, H, D,
                               None, kv_len, dtype=F16, rope_table=table)
    torch.cuda.synchronize()
    fr = freqs[pos.clamp(max=freqs.shape[0] - 1)]
    xq, xk, xv = x.view(B, n, 3 * H, D).split([H, H, H], dim=2)
    rq, rk = BB._apply_rope_interleaved(xq, fr), BB._apply_rope_interleaved(xk, fr)
    assert torch.equal(_bits(q), _bits(rq))
    for b in range(B):
        assert torch.equal(_bits(kc[b, :, kv_len:kv_len + n]), _bits(rk[b].transpose(0, 1)))
        assert torch.equal(_bits(vc[b, :, kv_len:kv_len + n]), _bits(xv[b].transpose(0, 1)))
        assert bool((kc[b, :, :kv_len] == 7.0).all()) and bool((kc[b, :, kv_len + n:] == 7.0).all())
        assert bool((vc[b, :, :kv_len] == -3.0).all()) and bool((vc[b, :, kv_len + n:] == -3.0).all())
    assert not rq[0, :n // 2].any() and rq[0, n // 2:].abs().sum() > 0 and rq[1].abs().sum() > 0


@pytest.mark.parametrize("B,n", [(3, 43), (8, 32)], ids=["129rows", "256rows"])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
def test_f2_qknorm_fp16_many_rows(B, n, H, Hkv):
    """F2's QK-norm form from planes: x = fp16(sum of planes); ln = fp16(layer_norm(x)); y = fp16(fp16(ln * gain) + bias);
    out = fp16(fp16(y cos) + fp16(rotate_half(y) sin)) with cos / sin cast to fp16 -- the roundings of ChameleonLayerNorm and the rotary;
    v is a plain copy of x"""
    D, S, kv_len, rows, nc = 128, 64, 9, B * n, 3
    g = torch.Generator(device=DEV).manual_seed(rows + H)
    ncol = (H + 2 * Hkv) * D
    planes = _planes(rows, ncol, nc, g)
    gains = [(1 + 0.3 * torch.randn(1, D, generator=g, device=DEV)).to(F16) for _ in range(2)]
    biases = [(0.1 * torch.randn(1, D, generator=g, device=DEV)).to(F16) for _ in range(2)]
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, device=DEV).float() / D))
    pos = (torch.randint(0, 3000, (B, 1), generator=g, device=DEV) + torch.arange(n, device=DEV)[None]).reshape(-1).contiguous()
    kc, vc = torch.zeros(B, Hkv, S, D, dtype=F16, device=DEV), torch.zeros(B, Hkv, S, D, dtype=F16, device=DEV)
    q = ops.qknorm_rope_append(ops.Partials(planes, nc, ncol), kc, vc, gains[0], biases[0], gains[1], biases[1], inv, pos, B, n, H, Hkv, D, None,
                               kv_len, dtype=F16)
    torch.cuda.synchronize()
    x = _seq_sum(planes[:, :rows], nc).to(F16).view(B, n, H + 2 * Hkv, D)
    fr = pos.view(B, n)[:, :, None].float() * inv[None, None, :]
    emb = torch.cat((fr, fr), dim=-1)
    cos, sin = emb.cos().to(F16).double()[:, :, None, :], emb.sin().to(F16).double()[:, :, None, :]
    rot = lambda t: torch.cat((-t[..., D // 2:], t[..., :D // 2]), dim=-1)
    swap = lambda t: torch.cat((t[..., D // 2:], t[..., :D // 2]), dim=-1)          # (rotate_half without the sign: for the bounds)

    def model(xh, gain, bias):
        xd = xh.double()
        ln = (xd - xd.mean(-1, keepdim=True)) * torch.rsqrt(xd.var(-1, unbiased=False, keepdim=True) + 1e-5)
        gw, bw = gain.double(), bias.double()
        y = _r16(_r16(_r16(ln) * gw) + bw)
        e_y = gw.abs() * _ulp(ln) + _ulp(ln * gw) + _ulp(y)                    # the three roundings behind y
        a, b_ = _r16(y * cos), _r16(rot(y) * sin)
        out = _r16(a + b_)
        # cos / sin come from the kernel's own cosf / sinf: one fp16 ulp of theirs where the cast falls the other way
        bound = (cos.abs() * e_y + y.abs() * _ulp(cos) + _ulp(a)) + (sin.abs() * swap(e_y) + swap(y).abs() * _ulp(sin) + _ulp(b_)) + _ulp(out)
        return out, bound

    mq, bq = model(x[:, :, :H], gains[0], biases[0])
    mk, bk = model(x[:, :, H:H + Hkv], gains[1], biases[1])
    eq = (q.double() - mq).abs()
    ek = (kc[:, :, kv_len:kv_len + n].transpose(1, 2).double() - mk).abs()
    print(f"f2 qk-norm fp16 rows={rows} H={H}/{Hkv}: max err / bound q {float((eq / bq).max()):.3f} k {float((ek / bk).max()):.3f}")
    assert bool((eq <= bq).all()) and bool((ek <= bk).all())
    assert torch.equal(_bits(vc[:, :, kv_len:kv_len + n]), _bits(x[:, :, H + Hkv:].transpose(1, 2)))
    assert kc[:, :, :kv_len].abs().sum() == 0 and kc[:, :, kv_len + n:].abs().sum() == 0


# ------------------------------------------------------------------------------------------------ 4. real-width forward, 256 rows
def _head_logits_from_partials(ho):
    """the logits K2 derives from an ops.HeadOut (tests/test_gpu_llamagen_batch.py): planes summed in chunk order, the folded final norm as
    a row scale, the 16-bit rounding of the lm_head output"""
    p = ho.part
    acc = p.data[0].clone()
    for c in range(1, p.n_chunks):
        acc = acc + p.data[c]
    ss, hid, eps = ho.row_norm
    s = ss[0].clone()
    for i in range(1, ss.shape[0]):
        s = s + ss[i]
    r = torch.rsqrt(s / hid + eps)
    return (acc * r[:, None]).to(ho.dtype).float()


def test_real_width_forward_fp16_256_rows(monkeypatch):
    """GPT-B width (768, 12 heads of 64), three layers, fp16, packed with max_rows=256: eight slots x CFG pair x window 16, every slot at its own
    KV length.  Bound: within 1.5 x the error of the ATen fp16 forward of the same rows, both against an fp32 forward."""
    from oracle.attention_ref import OracleWindowAttention
    from sjd_amd.engine_batch import _CacheView
    import sjd_amd.synthetic as synthetic
    n_layer, n_head, dim, n_slots = 3, 12, 768, 8
    a = BB.LlamaGenArgs(dim=dim, n_layer=n_layer, n_head=n_head, vocab_size=16384, block_size=256, model_type="c2i", cls_token_num=1, num_classes=1000)
    with torch.device(DEV):
        h16 = BB.LlamaGenBackbone(a, attn=ops.HipWindowAttention()).to(F16).eval()
    synthetic.fill_state_dict_device(h16, seed=5, embed_token_scale=0.5)
    sd = h16.state_dict()
    with torch.device(DEV):
        a16 = BB.LlamaGenBackbone(a, attn=ops.HipWindowAttention()).to(F16).eval()
        f32 = BB.LlamaGenBackbone(a, attn=OracleWindowAttention(torch.float32)).eval()
    a16.load_state_dict(sd)
    f32.load_state_dict({k: v.float() for k, v in sd.items()})
    h16.enable_fused(ops, gemm="sjd", max_rows=256, untuned_fp16=True)
    assert h16.G1_CFG == BB.LlamaGenBackbone.G1_CFG_LLAMAGEN_256ROW and tuple(h16.HEAD_CFG) == BB.LlamaGenBackbone.HEAD_CFG_256ROW
    W, nb = 16, 2
    B, S = n_slots * nb, 288
    KV = [200, 30, 177, 121, 52, 236, 148, 64]
    g = torch.Generator(device=DEV).manual_seed(11)
    cls = torch.randint(0, 1000, (B,), generator=g, device=DEV)
    ks = torch.zeros(B, dtype=torch.int32, device=DEV)
    ctx = torch.randint(0, 16384, (B, max(KV) - 1), generator=g, device=DEV)
    for m in (h16, a16, f32):
        m.setup_cache(batch=B, s_max=S)
        emb = torch.cat([m.embed_condition(cls), m.tok_embeddings(ctx)], dim=1)
        if hasattr(m.attn, "params"):
            m.attn.params = None
        with torch.no_grad():
            for b0 in range(0, B, 2):
                full = m.cache
                m.cache = _CacheView(full, b0, b0 + 2)
                m.forward_embeds(emb[b0:b0 + 2], torch.arange(max(KV), device=DEV)[None].repeat(2, 1), 0, ks[b0:b0 + 2])
                m.cache = full
    toks = torch.randint(0, 16384, (B, W), generator=g, device=DEV)
    kv_rows = torch.tensor(KV, device=DEV).repeat_interleave(nb)
    pos = kv_rows[:, None] + torch.arange(W, device=DEV)[None]
    params = ops.BlobArray(L.IterParams, n_slots, torch.device(DEV))
    for j, kv in enumerate(KV):
        v = params.blobs[j].view
        v.n_rows, v.kv_len, v.batch_rows = W, kv, nb
    params.upload()
    seen = []
    real = ops.skinny_gemm
    monkeypatch.setattr(ops, "skinny_gemm", lambda x, *a_, **k_: (seen.append(int(x.shape[0])), real(x, *a_, **k_))[1])
    with torch.no_grad():
        h16.attn.params = params
        ho = h16.forward_window(toks, pos, -1, ks, head_partials=True)
        h16.attn.params = None
        assert isinstance(ho, ops.HeadOut) and ho.col0 == 0 and ho.urow_off == W and ho.dtype == F16
        assert len(seen) == 4 * n_layer and set(seen) == {B * W}, "the projections ran at the full row count"
        hip = _head_logits_from_partials(ho)[:B * W].view(B, W, -1)
        aten = torch.empty(B, W, 16384, device=DEV)
        ref = torch.empty(B, W, 16384, device=DEV)
        for m, out in ((a16, aten), (f32, ref)):
            for b0 in range(0, B, 2):
                full = m.cache
                m.cache = _CacheView(full, b0, b0 + 2)
                out[b0:b0 + 2] = m.forward_window(toks[b0:b0 + 2], pos[b0:b0 + 2], KV[b0 // 2], ks[b0:b0 + 2])
                m.cache = full
    assert torch.isfinite(hip).all()
    for s in range(n_slots):                                   # per slot
        rows = slice(s * nb, (s + 1) * nb)
        e_hip, e_aten = (hip[rows] - ref[rows]).abs(), (aten[rows] - ref[rows]).abs()
        rec = dict(slot=s, kv=KV[s], hip_max=float(e_hip.max()), aten_max=float(e_aten.max()), hip_mean=float(e_hip.mean()),
                   aten_mean=float(e_aten.mean()))
        print("llamagen fp16 GPT-B width forward, 256 rows:", rec)
        assert e_hip.max() <= 1.5 * e_aten.max() + 1e-3 and e_hip.mean() <= 1.5 * e_aten.mean() + 1e-4, rec


# ------------------------------------------------------------------------------------------------ 5. the solver, eight labels
TOY_C2I = dict(dim=128, n_layer=2, n_head=2, vocab_size=16384, block_size=256, cls_token_num=1, model_type="c2i", num_classes=1000)
LABELS = (207, 1, 980, 417, 88, 555, 23, 761)
NEW = 64


def _solver_model(seed=7):
    from llamagen.llamagen_solver import renew_llamagen
    from scheduler.jacobi_iteration_lumina_mgpt import renew_sampler
    model = make_llamagen(TOY_C2I, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=F16, device=DEV)
    model.enable_fused(ops, gemm="sjd", max_rows=256, untuned_fp16=True)
    jac = dict(jacobi_loop_interval_l=1, jacobi_loop_interval_r=NEW - 16 - 2, max_num_new_tokens=16, guidance_scale=4.0, seed=seed,
               multi_token_init_scheme='random', do_cfg=True, image_top_k=1000, text_top_k=10, prefix_token_sampler_scheme='speculative_jacobi')
    model.__class__ = renew_llamagen(model.__class__)
    model._init_new_params(**jac)
    model.__class__ = renew_sampler(model.__class__)
    model._init_new_params(**jac)
    model.sjd_use_graph = True
    return model


def test_solver_generates_eight_fp16_prompts_per_forward(monkeypatch):
    """eight class labels share every window forward (256 rows of fp16); each prompt's tokens are bit for bit those it gets when the prompts
    decode one slot at a time (per-slot independence)"""
    from llamagen.llamagen_solver import LlamaGenSolver
    from sjd_amd.engine_batch import SJDBatchEngine
    model = _solver_model()
    solver = LlamaGenSolver(model=model, image_top_k=1000, image_top_p=1.0)
    assert solver.slots_for(len(LABELS), 2) == 8
    rows = []
    real = ops.skinny_gemm
    monkeypatch.setattr(ops, "skinny_gemm", lambda x, *a_, **k_: (rows.append(int(x.shape[0])), real(x, *a_, **k_))[1])
    kw = dict(cfg_scale=4.0, temperature=1.0, top_k=1000, top_p=1.0, sample_logits=True)
    toks = solver.generate(torch.tensor(LABELS, device=DEV), NEW, None, **kw)
    assert tuple(toks.shape) == (8, NEW) and toks.dtype == torch.long and int(toks.min()) >= 0 and int(toks.max()) < 16384
    assert max(rows) == 256, "the window forward ran on G1 at 256 rows"
    assert all(isinstance(e, SJDBatchEngine) and e.P == 8 and e.head_partials for e in model._sjd_engines.values())
    # one slot at a time: the same backbone, packing and engine class with ONE slot (continuous batching over the eight prompts, each with the
    # seed it had in the batch) -- 32-row launches of the same chunking
    del rows[:]
    alone = LlamaGenSolver(model=model, image_top_k=1000, image_top_p=1.0, prompts_per_forward=1).generate(torch.tensor(LABELS, device=DEV), NEW, None, **kw)
    assert max(rows) == 32 and any(isinstance(e, SJDBatchEngine) and e.P == 1 for e in model._sjd_engines.values())
    for j in range(8):
        assert torch.equal(toks[j], alone[j]), f"prompt {j}: its tokens depend on its neighbours"


# ------------------------------------------------------------------------------------------------ 6. Chameleon-shaped, 192 rows
def test_chameleon_fp16_three_slots_window_32():
    """three slots x window 32 x CFG = 192 rows of fp16 through SJDBatchEngine (QK-norm backbone at toy width, uncompressed packing on G1w):
    every slot takes exactly the decisions of its own oracle replay"""
    from tests.gpu_loop_check import teacher_forced_batch_check
    rs = teacher_forced_batch_check(n_prompts=3, window=32, P=(12, 9, 14), dtype=F16)
    assert len(rs) == 3 and all(r["last"] == 8196 and r["tokens"] == 73 for r in rs)
