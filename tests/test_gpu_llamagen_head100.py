"""LlamaGen GPT-3B's head_dim 100 on the HIP path: heads stored 128 wide with zero pad columns.

  * F2's padded-head form (SJD_F2_HEAD_PAD128) bit for bit against the ATen rotary and a plain copy for v, over buffers pre-filled with 0xFF:
    the pad columns of every written row are zero, everything else keeps its 0xFF bytes;
  * K1 with the logical head dim (SJD_K1_HEAD_DIM_100) through every form the dispatcher picks, inside the rounding bound of
    tests/blob_array_cases.py::attention_fp64 at D = 100 and OUTSIDE it against the same reference scaled by 1/sqrt(128);
  * the refusals of both bits; the prefill through HipWindowAttention.__call__; the fused window forward at GPT-3B's width in the envelope of the
    ATen 16-bit forward; teacher-forced loops and LlamaGenSolver.generate on a head_dim-100 toy.

The toy is dim 800 / 8 heads, the smallest head_dim-100 model kernel G1 packs (see tests/test_llamagen_head100.py).
"""
import ctypes

import pytest
import torch

import sjd_amd._lib as L
import sjd_amd.backbones as BB
import sjd_amd.ops as ops
from oracle import sjd_oracle as O
from oracle.attention_ref import OracleWindowAttention
from tests.blob_array_cases import attention_fp64
from tests.gpu_loop_check import _Recorder, _loop_cfg, _replay
from tests.helpers import llamagen_prefill_sample, make_llamagen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOY = dict(dim=800, n_layer=2, n_head=8, vocab_size=16384, block_size=256, cls_token_num=1, model_type="c2i", num_classes=1000)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ F2
STARTS = [100, 130, 125, 0, 118, 133, 7, 119]          # first position of a batch row: condition rows (< 120), image rows, across the table's end (136 rows)


def _f2_case(dtype, src, H, B, n, blobs=None, S=200, kv_len=150, cls=120, grid=4):
    D, DS = 100, 128
    g = torch.Generator(device=DEV).manual_seed(B * n + H + (src == "planes"))
    freqs = BB._rope_2d_table(grid, D, 10000, cls).to(DEV)                 # [136, 50, 2], the first 120 rows zero
    table = BB._rope_table_extended(freqs, S)
    assert table.shape == (S, 50, 2)
    pos = torch.stack([torch.arange(STARTS[b % len(STARTS)], STARTS[b % len(STARTS)] + n) for b in range(B)]).to(DEV)
    N, T = 3 * H * D, B * n
    if src == "dense":
        x = torch.randn(T, N, generator=g, device=DEV).to(dtype)
        qkv, part, nc = x, None, 0
    else:
        part = torch.randn(3, ((T + 31) // 32) * 32, N, generator=g, device=DEV)
        x = ((part[0] + part[1]) + part[2])[:T].to(dtype)                   # F2 sums the planes in chunk order, then rounds once
        qkv, nc = None, 3
    ff = lambda *shape: torch.full(shape, -1, dtype=torch.int16, device=DEV).view(dtype)       # 0xFF bytes
    q, kc, vc = ff(B, n, H, DS), ff(B, H, S, DS), ff(B, H, S, DS)
    params = None
    if blobs is not None:                                                   # one blob per batch row, each with its own kv_len
        params = ops.BlobArray(L.IterParams, B, torch.device(DEV))
        for b, kv in enumerate(blobs):
            v = params.blobs[b].view
            v.n_rows, v.kv_len, v.batch_rows = n, kv, 1
            params.blobs[b].upload()
    rc = L.load().sjd_qknorm_rope_append_ex(_p(qkv), _p(q), _p(kc), _p(vc), None, None, None, None, _p(table), _p(pos.reshape(-1).contiguous()), B, n, H, H,
                                           D, S, ops._dtype_code(dtype) | L.F2_ROPE_TABLE | L.F2_HEAD_PAD128, 0, 1.0, 1.0, None,
                                           params.blobs[0].ptr if params is not None else None, kv_len if params is None else 0, _p(part), nc, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    fr = freqs[pos.clamp(max=freqs.shape[0] - 1)]
    xq, xk, xv = x.view(B, n, 3 * H, D).split([H, H, H], dim=2)
    rq, rk = BB._apply_rope_interleaved(xq, fr), BB._apply_rope_interleaved(xk, fr)
    assert torch.equal(_bits(q[..., :D]), _bits(rq))
    assert not _bits(q[..., D:]).any()                                       # pad columns exactly zero (not -0)
    kvs = blobs if blobs is not None else [kv_len] * B
    for b in range(B):
        r0 = kvs[b]
        assert torch.equal(_bits(kc[b, :, r0:r0 + n, :D]), _bits(rk[b].transpose(0, 1)))
        assert torch.equal(_bits(vc[b, :, r0:r0 + n, :D]), _bits(xv[b].transpose(0, 1)))
        assert not _bits(kc[b, :, r0:r0 + n, D:]).any() and not _bits(vc[b, :, r0:r0 + n, D:]).any()
        for c in (kc, vc):                                                   # unwritten cache rows keep their 0xFF bytes
            assert (_bits(c[b, :, :r0]) == -1).all() and (_bits(c[b, :, r0 + n:]) == -1).all()
    assert not rq[0].any() and rq[1].abs().sum() > 0                        # (batch row 0 really is condition rows, row 1 is not)
    if src == "planes" and blobs is None:                                   # the Python wrapper: same q bits, 128 wide
        kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
        q2 = ops.qknorm_rope_append(ops.Partials(part, 3, N), kc2, vc2, None, None, None, None, None, pos.reshape(-1).contiguous(), B, n, H, H, D, None,
                                    kv_len, dtype=dtype, rope_table=table, head_pad=128)
        torch.cuda.synchronize()
        assert q2.shape == (B, n, H, DS) and torch.equal(_bits(q2), _bits(q))


@pytest.mark.parametrize("src", ["dense", "planes"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_f2_head_pad_bit_exact(dtype, src):
    _f2_case(dtype, src, H=3, B=2, n=16)                                     # (an odd head count: nothing may assume groups of four heads)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("H,B", [(3, 6), (4, 6), (4, 16)], ids=["96rows_3heads_one_head_kernel", "96rows_4heads", "256rows_4heads"])
def test_f2_head_pad_many_rows(H, B, dtype):
    _f2_case(dtype, "planes", H=H, B=B, n=16)                                # four heads per wave where H % 4 == 0, the one-head kernel otherwise


@pytest.mark.parametrize("H,B", [(3, 2), (4, 6)], ids=["32rows", "96rows"])
def test_f2_head_pad_batch_rows_blobs(H, B):
    _f2_case(torch.bfloat16, "planes", H=H, B=B, n=16, blobs=[150, 171, 3, 96, 40, 133][:B])


def test_f2_head_pad_refusals():
    lib = L.load()
    H, B, n, S = 2, 1, 4, 64
    qkv = torch.zeros(B * n, 3 * H * 128, dtype=torch.bfloat16, device=DEV)
    q = torch.empty(B, n, H, 128, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(B, H, S, 128, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    tab = torch.zeros(S, 64, 2, device=DEV)
    pos = torch.arange(n, device=DEV)

    def call(dt, D_):
        return lib.sjd_qknorm_rope_append_ex(_p(qkv), _p(q), _p(kc), _p(vc), None, None, None, None, _p(tab), _p(pos), B, n, H, H, D_, S, dt, 0, 1.0, 1.0,
                                             None, None, 0, None, 0, _stream())
    assert call(L.DTYPE_BF16 | L.F2_ROPE_TABLE | L.F2_HEAD_PAD128, 100) == 0
    torch.cuda.synchronize()
    assert call(L.DTYPE_BF16 | L.F2_HEAD_PAD128, 100) == -2                    # the bit without SJD_F2_ROPE_TABLE
    for D_ in (64, 96, 128):
        assert call(L.DTYPE_BF16 | L.F2_ROPE_TABLE | L.F2_HEAD_PAD128, D_) == -2      # ... with D != 100
    assert call(L.DTYPE_BF16 | L.F2_ROPE_TABLE, 100) == -2                     # D = 100 without the bit: as before
    assert call(L.DTYPE_BF16, 100) == -2
    assert lib.sjd_qknorm_rope_append_fp8(_p(qkv), _p(q), _p(kc), _p(vc), None, None, None, None, _p(tab), _p(pos), B, n, H, H, 100, S,
                                          L.DTYPE_BF16 | L.F2_ROPE_TABLE | L.F2_HEAD_PAD128, 1.0, 1.0, None, 0, None, 0, _stream()) == -2


# ------------------------------------------------------------------------------------------------ K1
class _Cache:
    def __init__(self, k, v):
        self.k, self.v, self.s_max = k, v, k.shape[3]


K1_FORMS = {"colsplit": (16, 4, "colsplit"), "direct": (16, 1, "keysplit"), "combine": (16, 4, "keysplit"), "window32": (32, 4, "keysplit"),
            "window64_ring": (64, 2, "keysplit")}
_K1_REF = {}


def _k1_inputs(dtype, n, kv_len):
    """random q / k / v at D = 100 (the window's rows already in the caches), their zero-padded twins, the fp64 references at both scales"""
    key = (dtype, n, kv_len)
    if key not in _K1_REF:
        B, H, S, D = 2, 2, 768, 100
        ks = [0, 11]
        g = torch.Generator().manual_seed(n * 1000 + kv_len)
        kc = torch.randn(B, H, S, D, generator=g).to(dtype)
        vc = torch.randn(B, H, S, D, generator=g).to(dtype)
        q = (torch.randn(B, n, H, D, generator=g) * 1.5).to(dtype)
        zp = lambda t: torch.nn.functional.pad(t, (0, 28))
        exact, bound, vis = attention_fp64(q, kc, vc, kv_len, n, ks, dtype)                   # scale 1/sqrt(100)
        wrong, wbound, _ = attention_fp64(zp(q), zp(kc), zp(vc), kv_len, n, ks, dtype)        # the same operands at scale 1/sqrt(128)
        wrong, wbound = wrong[..., :D], wbound[..., :D]
        # the inputs must tell the two scales apart: somewhere the references differ by more than both rounding bounds together
        sep = ((exact - wrong).abs() > bound + wbound)
        sep[~vis] = False
        assert sep.any(), "the chosen inputs do not separate 1/sqrt(100) from 1/sqrt(128)"
        # the loose reference: OracleWindowAttention in fp64 at D = 100 (it appends the window's own rows again: same values)
        k_new, v_new = kc[:, :, kv_len:kv_len + n].transpose(1, 2).contiguous(), vc[:, :, kv_len:kv_len + n].transpose(1, 2).contiguous()
        ref = OracleWindowAttention()(0, q, k_new, v_new, _Cache(kc[None].clone(), vc[None].clone()), kv_len, ks).float()
        _K1_REF[key] = (zp(q), zp(kc), zp(vc), ks, exact, bound, vis, wrong, wbound, ref)
    return _K1_REF[key]


@pytest.mark.parametrize("kv_len", [37, 150, 700])
@pytest.mark.parametrize("form", list(K1_FORMS))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_k1_head_dim_100(dtype, form, kv_len):
    n, n_split, regime = K1_FORMS[form]
    qp, kcp, vcp, ks, exact, bound, vis, wrong, wbound, ref = _k1_inputs(dtype, n, kv_len)
    cache = _Cache(kcp[None].to(DEV), vcp[None].to(DEV))
    attn = ops.HipWindowAttention(n_split=n_split)
    attn.regime = regime
    if regime == "colsplit":
        assert ops.colsplit_ok(2, n, 2, 2, 128, dtype)
    out = attn.attend(0, qp.to(DEV), cache, kv_len, torch.tensor(ks, dtype=torch.int32, device=DEV), head_dim=100)
    torch.cuda.synchronize()
    got = out.cpu()
    assert got.shape == (2, n, 2, 128) and torch.isfinite(got.float()).all()
    assert not _bits(got[..., 100:]).any()                                    # pad output columns exactly zero
    got = got[..., :100].double()
    assert (got[~vis] == 0).all()
    e = (got - exact).abs()
    print(f"k1 head_dim 100 {form} kv {kv_len}: max err {float(e[vis].max()):.3e}, max err / bound {float((e / bound)[vis].max()):.3f}, "
          f"against 1/sqrt(128): max err / bound {float(((got - wrong).abs() / wbound)[vis].max()):.1f}")
    err = (got.float() - ref).abs()
    assert err[vis].max() < 3e-2 and err[vis].mean() < 3e-3
    over = e > bound
    over[~vis] = False
    assert not over.any(), f"{form}: err {float(e[over].max()):.3e} over the rounding bound at {over.nonzero()[0].tolist()} (batch row, row, head, column)"
    wover = (got - wrong).abs() > wbound                                     # ... and NOT what a launch with 1/sqrt(128) computes
    wover[~vis] = False
    assert wover.any(), f"{form}: the output is inside the rounding bound of the 1/sqrt(128) reference"


def test_k1_head_dim_100_refusals():
    lib = L.load()
    B, n, S = 1, 16, 128
    st, ksp = _stream(), torch.zeros(B, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.float32, device=DEV)

    def bufs(H, Hkv, D, dt=torch.bfloat16):
        return (torch.zeros(B, n, H, D, dtype=dt, device=DEV), torch.zeros(B, Hkv, S, D, dtype=dt, device=DEV),
                torch.zeros(B, Hkv, S, D, dtype=dt, device=DEV), torch.zeros(B, n, H, D, dtype=dt, device=DEV))

    def ex(H, Hkv, D, code, dt=torch.bfloat16):
        q, kc, vc, out = bufs(H, Hkv, D, dt)
        rc = lib.sjd_draft_window_attention_ex(_p(q), _p(kc), _p(vc), _p(out), B, n, H, Hkv, D, S, code, _p(ksp), None, 8, 1, _p(ws), st, None, None)
        torch.cuda.synchronize()
        return rc

    def colsplit(H, Hkv, D, code):
        q, kc, vc, out = bufs(H, Hkv, D)
        rc = lib.sjd_draft_window_attention_colsplit(_p(q), _p(kc), _p(vc), _p(out), B, n, H, Hkv, D, S, code, _p(ksp), None, 8, st)
        torch.cuda.synchronize()
        return rc
    bit = L.K1_HEAD_DIM_100
    assert ex(2, 2, 128, L.DTYPE_BF16 | bit) == 0 and ex(2, 2, 128, L.DTYPE_F16 | bit, torch.float16) == 0 and colsplit(2, 2, 128, L.DTYPE_BF16 | bit) == 0
    assert ex(2, 2, 64, L.DTYPE_BF16 | bit) == -2 and colsplit(2, 2, 64, L.DTYPE_BF16 | bit) == -2          # D != 128
    assert ex(4, 2, 128, L.DTYPE_BF16 | bit) == -2 and ex(8, 2, 128, L.DTYPE_F16 | bit, torch.float16) == -2   # grouped-query attention
    assert ex(2, 2, 128, L.DTYPE_F32 | bit, torch.float32) == -2                                               # the fp32 variant
    assert ex(2, 2, 100, L.DTYPE_BF16) == -2 and ex(2, 2, 100, L.DTYPE_BF16 | bit) == -2                       # D = 100 itself: as before
    q, kc, vc, out = bufs(2, 2, 128)
    kc8, vc8 = kc.view(torch.uint8)[..., :128].contiguous(), vc.view(torch.uint8)[..., :128].contiguous()
    assert lib.sjd_draft_window_attention_fp8(_p(q), _p(kc8), _p(vc8), _p(out), B, n, 2, 2, 128, S, L.DTYPE_BF16 | bit, 1.0, 1.0, _p(ksp), None, 8, 1,
                                              _p(ws), st) == -2
    assert lib.sjd_draft_window_attention_fp8_colsplit(_p(q), _p(kc8), _p(vc8), _p(out), B, n, 2, 2, 128, S, L.DTYPE_BF16 | bit, 1.0, 1.0, _p(ksp), None,
                                                       8, st) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ prefill
class _RecordingAttention:
    """HipWindowAttention behind a recorder of the k / v the ATen rotary hands to the attention backend"""

    def __init__(self):
        self.inner, self.seen, self.params = ops.HipWindowAttention(n_split=2), {}, None

    def __call__(self, layer, q, k, v, cache, kv_len, key_start):
        self.seen[layer] = (k.clone(), v.clone())
        return self.inner(layer, q, k, v, cache, kv_len, key_start)


def test_prefill_writes_padded_cache_rows():
    rec = _RecordingAttention()
    model = make_llamagen(TOY, 17, 0.25, rec, dtype=torch.bfloat16, device=DEV)
    model.setup_cache(batch=2, s_max=96)
    model.enable_fused(ops, gemm="sjd", pad_head_dim=True)                     # (this order: the 100-wide cache is replaced)
    assert model.cache.k.shape[-1] == 128
    model.cache.k.view(torch.int16).fill_(-1)
    model.cache.v.view(torch.int16).fill_(-1)
    g = torch.Generator(device=DEV).manual_seed(5)
    n, kv = 40, 0                                                             # more rows than a fused window: forward_embeds (from row 0: nothing reads the 0xFF rows)
    toks = torch.randint(0, 16384, (2, n), generator=g, device=DEV)
    pos = (kv + torch.arange(n, device=DEV))[None].repeat(2, 1)
    ks = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    logits = model.forward_window(toks, pos, kv, ks)
    torch.cuda.synchronize()
    assert logits.shape == (2, n, 16384) and torch.isfinite(logits).all()
    for li in range(model.n_layers):
        k, v = rec.seen[li]
        assert k.shape == (2, n, 8, 100)
        for c, x in ((model.cache.k[li], k), (model.cache.v[li], v)):
            assert torch.equal(_bits(c[:, :, kv:kv + n, :100]), _bits(x.transpose(1, 2)))
            assert not _bits(c[:, :, kv:kv + n, 100:]).any()
            assert (_bits(c[:, :, :kv]) == -1).all() and (_bits(c[:, :, kv + n:]) == -1).all()
    # the same prefill on an un-padded twin with the fp32 oracle backend: the padded K1 computes head_dim-100 attention
    ref = make_llamagen(TOY, 17, 0.25, OracleWindowAttention(torch.float32), dtype=torch.float32, device=DEV)
    ref.setup_cache(batch=2, s_max=96)
    with torch.no_grad():
        want = ref.forward_window(toks, pos, kv, ks)
    assert (logits.float() - want).abs().max() < 0.15 * want.abs().max()


# ------------------------------------------------------------------------------------------------ GPT-3B's width
def _head_logits_from_partials(ho):
    """the logits K2 derives from an ops.HeadOut: planes summed in chunk order, the folded final norm as a row scale, the 16-bit rounding"""
    p = ho.part
    acc = p.data[0].clone()
    for c in range(1, p.n_chunks):
        acc = acc + p.data[c]
    ss, hid, eps = ho.row_norm
    s = ss[0].clone()
    for i in range(1, ss.shape[0]):
        s = s + ss[i]
    return (acc * torch.rsqrt(s / hid + eps)[:, None]).to(ho.dtype).float()


def test_real_width_window_forward_gpt_3b():
    """measured on one MI355X: see profiles/llamagen_3b_forward.json"""
    import sjd_amd.synthetic as synthetic
    a = BB.LlamaGenArgs(dim=3200, n_layer=3, n_head=32, vocab_size=16384, block_size=576, model_type="c2i", cls_token_num=1, num_classes=1000)
    with torch.device(DEV):
        h16 = BB.LlamaGenBackbone(a, attn=ops.HipWindowAttention()).to(torch.bfloat16).eval()
    synthetic.fill_state_dict_device(h16, seed=5, embed_token_scale=0.5)
    sd = h16.state_dict()
    with torch.device(DEV):
        a16 = BB.LlamaGenBackbone(a, attn=OracleWindowAttention(torch.bfloat16)).to(torch.bfloat16).eval()
        f32 = BB.LlamaGenBackbone(a, attn=OracleWindowAttention(torch.float32)).eval()
    a16.load_state_dict(sd)
    f32.load_state_dict({k: v.float() for k, v in sd.items()})
    h16.enable_fused(ops, gemm="sjd", pad_head_dim=True)
    S, KV = 608, (500, 100)
    g = torch.Generator(device=DEV).manual_seed(11)
    cond = torch.tensor([207, 1000], device=DEV)                              # the class and the unconditional row
    ks = torch.zeros(2, dtype=torch.int32, device=DEV)
    ctx = torch.randint(0, 16384, (1, max(KV) - 1), generator=g, device=DEV).repeat(2, 1)
    for m in (h16, a16, f32):
        m.setup_cache(batch=2, s_max=S)
        emb = torch.cat([m.embed_condition(cond), m.tok_embeddings(ctx)], dim=1)
        if hasattr(m.attn, "params"):
            m.attn.params = None
        with torch.no_grad():
            m.forward_embeds(emb, torch.arange(max(KV), device=DEV)[None].repeat(2, 1), 0, ks)
    assert h16.cache.k.shape[-1] == 128 and a16.cache.k.shape[-1] == 100
    for kv in KV:           # (500 first: the window at 100 overwrites cache rows the longer one would read)
        toks = torch.randint(0, 16384, (1, 16), generator=g, device=DEV).repeat(2, 1)
        pos = (kv + torch.arange(16, device=DEV))[None].repeat(2, 1)
        with torch.no_grad():
            ho = h16.forward_window(toks, pos, kv, ks, head_partials=True)
            assert isinstance(ho, ops.HeadOut) and ho.col0 == 0 and ho.urow_off == 16
            hip = _head_logits_from_partials(ho)[:32].view(2, 16, -1)
            aten = a16.forward_window(toks, pos, kv, ks)
            ref = f32.forward_window(toks, pos, kv, ks)
        e_hip, e_aten = (hip - ref).abs(), (aten.float() - ref).abs()
        rec = dict(kv=kv, hip_max=float(e_hip.max()), aten_max=float(e_aten.max()), hip_mean=float(e_hip.mean()), aten_mean=float(e_aten.mean()),
                   max_ratio=float(e_hip.max() / e_aten.max()), mean_ratio=float(e_hip.mean() / e_aten.mean()),
                   argmax_agree=float((hip.argmax(-1) == aten.argmax(-1)).float().mean()))
        print("llamagen GPT-3B-width forward:", rec)
        assert torch.isfinite(hip).all()
        assert e_hip.max() <= 1.5 * e_aten.max() + 1e-3 and e_hip.mean() <= 1.5 * e_aten.mean() + 1e-4, rec


# ------------------------------------------------------------------------------------------------ loops
def _tf_loop(scheme, use_graph, window=16, seed=7, top_k=1000, cfg_scale=4.0):
    from sjd_amd.engine import SJDConfig, SJDEngine, WindowSpec
    from sjd_amd.grammar import TopKTopPGrammar
    model = make_llamagen(TOY, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
    model.enable_fused(ops, gemm="sjd", pad_head_dim=True)
    T, N = model.cls_token_num, TOY["block_size"]
    model.setup_cache(batch=2, s_max=((T + N + 64 + 31) // 32) * 32)
    assert model.cache.k.shape[-1] == 128
    ks = torch.zeros(2, dtype=torch.int32, device=DEV)
    cond = torch.tensor([207, model.num_classes], device=DEV)
    model.attn.params = None
    logits = model.forward_embeds(model.embed_condition(cond), torch.arange(T, device=DEV)[None].repeat(2, 1), 0, ks)
    torch.manual_seed(seed)
    first = int(llamagen_prefill_sample(logits.float().cpu(), cfg_scale, 1.0, top_k, 1.0)[0, 0])
    cfg = SJDConfig(jacobi_loop_interval_l=1, jacobi_loop_interval_r=N - window - 2, max_num_new_tokens=window, guidance_scale=cfg_scale,
                    seed=seed, prefix_token_sampler_scheme=scheme, max_length=N)
    spec = WindowSpec(first_tokens=torch.tensor([[first], [first]], device=DEV), first_positions=torch.full((2, 1), T, dtype=torch.long, device=DEV),
                      key_start=ks, pos_offset=torch.zeros(2, dtype=torch.long), kv_base=T)
    eng = SJDEngine(model, 16384, DEV, max_window=window, use_graph=use_graph)
    assert eng.head_partials
    rec = _Recorder()
    eng.hook = rec
    seq, stats = eng.decode([first], spec, TopKTopPGrammar(top_k, 1.0), cfg)
    seq_ref, tr, _ = _replay(rec, [first], lambda c, n: O.llamagen_rules(c, n, top_k, 1.0), _loop_cfg(cfg), 16384, device=DEV)
    assert seq == seq_ref, "token sequences differ"
    assert stats.matched == tr.matched and stats.nfe == len(tr.matched)
    assert not _bits(model.cache.k[..., 100:]).any() and not _bits(model.cache.v[..., 100:]).any()      # the pad columns stayed zero
    return seq


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("scheme", ["speculative_jacobi", "jacobi"])
def test_teacher_forced_toy_head_dim_100(scheme, use_graph):
    _tf_loop(scheme, use_graph)


def _solver_tokens(use_graph, seed=7):
    from llamagen.llamagen_solver import LlamaGenSolver, renew_llamagen
    from scheduler.jacobi_iteration_lumina_mgpt import renew_sampler
    model = make_llamagen(TOY, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
    model.enable_fused(ops, gemm="sjd", pad_head_dim=True)
    jac = dict(jacobi_loop_interval_l=1, jacobi_loop_interval_r=256 - 16 - 2, max_num_new_tokens=16, guidance_scale=4.0, seed=seed,
               multi_token_init_scheme='random', do_cfg=True, image_top_k=1000, text_top_k=10, prefix_token_sampler_scheme='speculative_jacobi')
    model.__class__ = renew_llamagen(model.__class__)
    model._init_new_params(**jac)
    model.__class__ = renew_sampler(model.__class__)
    model._init_new_params(**jac)
    model.sjd_use_graph = use_graph
    solver = LlamaGenSolver(model=model, image_top_k=1000, image_top_p=1.0)
    torch.manual_seed(seed)
    toks = solver.generate(torch.tensor([207], device=DEV), 256, None, cfg_scale=4.0, temperature=1.0, top_k=1000, top_p=1.0, sample_logits=True)
    assert toks.shape == (1, 256) and int(toks.min()) >= 0 and int(toks.max()) < 16384
    assert model.last_sjd_stats.nfe < 256 and model.cache.k.shape[-1] == 128
    assert all(e.head_partials for e in model._sjd_engines.values())
    return toks.cpu()


def test_solver_generate_head_dim_100_repeats_and_graph_equals_eager():
    a = _solver_tokens(True)
    b = _solver_tokens(True)
    c = _solver_tokens(False)
    assert torch.equal(a, b)
    assert torch.equal(a, c)
