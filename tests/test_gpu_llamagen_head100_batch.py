"""Several prompts per forward at head_dim 100 (LlamaGen GPT-3B stored 128 wide): the kernels in the combinations the wider windows bring together.

  a. kernel G1w's split-K planes at GPT-3B-like shapes, bit for bit against the 32-row kernel run row block by row block at the same chunking:
     a column-tile count that is no multiple of the tiles per workgroup (300 tiles by 8, 75 tiles by 2 / 4 / 6: the last workgroup is partial),
     K / KC = 3200 / 640, 4096 / 512, 8704 / 1088 and every launch shape the sets G1_CFG_LLAMAGEN_3B_128ROW / _256ROW name at GPT-3B's true size;
  b. F2's rows kernel in its padded form (SJD_F2_HEAD_PAD128) under an array of sjd_iter_params, two and eight slots, every slot its own kv_len
     and positions, 96 / 130 / 256 rows (130 = 2 slots x 5 batch rows x 13: eight slots do not divide it), against the one-head padded kernel
     and the ATen rotary, over caches pre-filled with 0xFF bytes;
  c. K1 with the logical head dim (SJD_K1_HEAD_DIM_100) for 4 and 16 batch rows whose kv_len come from the blob array, both regimes;
  d. the fused window forward at GPT-3B's width (two layers) with 128 and 256 rows, per prompt within 1.5 x the error of the bf16 ATen (SDPA)
     forward, both against fp32;
  e. teacher-forced several-prompt loops on the head_dim-100 toy against the CPU oracle (captions of distinct lengths, a refill, a guidance
     scale per prompt) and LlamaGenSolver.generate with several class ids.
"""
import pytest
import torch
import torch.nn.functional as F

import sjd_amd._lib as L
import sjd_amd.backbones as BB
import sjd_amd.ops as ops
from oracle import sjd_oracle as O
from oracle.attention_ref import OracleWindowAttention
from tests.blob_array_cases import attention_fp64
from tests.gpu_loop_check import _Recorder, _loop_cfg, _replay
from tests.helpers import make_llamagen
from tests.test_gpu_llamagen_head100 import TOY, _bits, _head_logits_from_partials

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLS = BB.LlamaGenBackbone
PAD = dict(pad_head_dim=True, padded_batch=True)


# ------------------------------------------------------------------------------------------------ a. G1w planes
GPT3B_SHAPES = dict(qkv=(9600, 3200), o=(3200, 4096), gate_up=(17408, 3200), down=(3200, 8704), head=(16384, 3200))       # (N, K), heads stored 128 wide


def _g1_cases():
    cases = [(9600, 3200, 640, 8, True), (2400, 3200, 640, 6, False), (2400, 4096, 512, 2, False), (2400, 4096, 512, 4, True),
             (2400, 8704, 1088, 4, False), (2400, 8704, 1088, 2, True)]
    for rows in (128, 256):                                            # ... and what the new sets actually launch
        sets = dict(getattr(CLS, f"G1_CFG_LLAMAGEN_3B_{rows}ROW"), head=getattr(CLS, f"HEAD_CFG_3B_{rows}ROW"))
        for name, (kc, tiles, sm) in sets.items():
            case = GPT3B_SHAPES[name] + (kc, tiles, bool(sm))
            if case not in cases:
                cases.append(case)
    return cases


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,K,KC,tiles,sm", _g1_cases(), ids=lambda v: str(int(v)))
def test_g1w_planes_equal_the_32_row_kernel_row_block_by_row_block(N, K, KC, tiles, sm, dtype):
    g = torch.Generator(device=DEV).manual_seed(N + K + KC + tiles)
    w = (torch.randn(N, K, generator=g, device=DEV) / K ** 0.5).to(dtype)
    x = torch.randn(256, K, generator=g, device=DEV).to(dtype)
    packed = ops.pack_weight(w, KC, sm)
    nc = -(-K // KC)
    ref = torch.empty(nc, 256, N, device=DEV)
    for r0 in range(0, 256, 32):                                       # g1_skinny_gemm: one row tile, the whole chunk staged in LDS
        ref[:, r0:r0 + 32] = ops.skinny_gemm(x[r0:r0 + 32].contiguous(), packed, N, K, KC, tiles, sm).data
    want = x[:8].float() @ w[:96].float().t()                          # (the reference itself computes the projection)
    assert (ref[:, :8, :96].sum(0) - want).abs().max() < 2e-2 * max(1.0, float(want.abs().max()))
    # bf16: 65 / 128 rows (three / four row tiles) and 129 / 160 / 256 (five and eight: kernel G1w proper); fp16 runs on G1w from 129 rows on
    for M in ((65, 128, 129, 160, 256) if dtype == torch.bfloat16 else (256,)):
        got = ops.skinny_gemm(x[:M].contiguous(), packed, N, K, KC, tiles, sm)
        torch.cuda.synchronize()
        assert got.n_chunks == nc and got.data.shape == (nc, ops._prows(M), N)
        same = torch.equal(got.data[:, :M].view(torch.int32), ref[:, :M].view(torch.int32))
        if not same:
            bad = (got.data[:, :M] != ref[:, :M]).nonzero()
            raise AssertionError(f"M {M}: {bad.shape[0]} plane elements differ, first at (chunk, row, column) {bad[0].tolist()}")


# ------------------------------------------------------------------------------------------------ b. F2, padded rows kernel, blob array
F2_SLOT_KV = [150, 171, 3, 96, 40, 133, 0, 88]
F2_SLOT_POS = [100, 130, 125, 0, 118, 133, 7, 119]                      # first position of a slot: condition rows (< 120), image rows, across the table's end


def _f2_padded_slots(dtype, slots, batch_rows, n, H, one_head, S=256, cls=120, grid=4):
    D, DS = 100, 128
    B = slots * batch_rows
    rows = B * n
    g = torch.Generator(device=DEV).manual_seed(rows + slots + H)
    freqs = BB._rope_2d_table(grid, D, 10000, cls).to(DEV)               # [136, 50, 2]
    table = BB._rope_table_extended(freqs, S)
    pos = torch.stack([torch.arange(F2_SLOT_POS[b // batch_rows], F2_SLOT_POS[b // batch_rows] + n) for b in range(B)]).to(DEV)
    N = 3 * H * D
    part = torch.randn(3, ops._prows(rows), N, generator=g, device=DEV)
    x = ((part[0] + part[1]) + part[2])[:rows].to(dtype)                  # F2 sums the planes in chunk order, then rounds once
    ff = lambda *shape: torch.full(shape, -1, dtype=torch.int16, device=DEV).view(dtype)        # 0xFF bytes
    kc, vc = ff(B, H, S, DS), ff(B, H, S, DS)
    params = ops.BlobArray(L.IterParams, slots, torch.device(DEV))
    for j in range(slots):
        v = params.blobs[j].view
        v.n_rows, v.kv_len, v.batch_rows = n, F2_SLOT_KV[j], batch_rows
    params.upload()
    q = ops.qknorm_rope_append(ops.Partials(part, 3, N), kc, vc, None, None, None, None, None, pos.reshape(-1).contiguous(), B, n, H, H, D,
                               params.blobs[0], 0, dtype=dtype, rope_table=table, head_pad=128, one_head=one_head)
    torch.cuda.synchronize()
    assert q.shape == (B, n, H, DS)
    fr = freqs[pos.clamp(max=freqs.shape[0] - 1)]
    xq, xk, xv = x.view(B, n, 3 * H, D).split([H, H, H], dim=2)
    rq, rk = BB._apply_rope_interleaved(xq, fr), BB._apply_rope_interleaved(xk, fr)
    assert torch.equal(_bits(q[..., :D]), _bits(rq))
    assert not _bits(q[..., D:]).any()                                    # pad columns 100..127: zero bits
    for b in range(B):
        r0 = F2_SLOT_KV[b // batch_rows]
        assert torch.equal(_bits(kc[b, :, r0:r0 + n, :D]), _bits(rk[b].transpose(0, 1)))
        assert torch.equal(_bits(vc[b, :, r0:r0 + n, :D]), _bits(xv[b].transpose(0, 1)))
        assert not _bits(kc[b, :, r0:r0 + n, D:]).any() and not _bits(vc[b, :, r0:r0 + n, D:]).any()
        for c in (kc, vc):                                                # every other cache row keeps its 0xFF bytes
            assert (_bits(c[b, :, :r0]) == -1).all() and (_bits(c[b, :, r0 + n:]) == -1).all()
    return q, kc, vc


# slots, batch rows per slot, window rows: 96 / 130 / 256 rows in all
F2_GEOMETRY = {"2slots_96rows": (2, 2, 24), "8slots_96rows": (8, 2, 6), "2slots_130rows": (2, 5, 13), "2slots_256rows": (2, 8, 16), "8slots_256rows": (8, 2, 16)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("geo", list(F2_GEOMETRY))
def test_f2_padded_rows_kernel_under_a_blob_array(geo, dtype):
    slots, br, n = F2_GEOMETRY[geo]
    a = _f2_padded_slots(dtype, slots, br, n, 8, one_head=False)           # four heads per wave (H % 4 == 0, more than 64 rows)
    b = _f2_padded_slots(dtype, slots, br, n, 8, one_head=True)            # the one-head padded kernel: the same bits everywhere
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v))


# ------------------------------------------------------------------------------------------------ c. K1, logical head dim, blob array
class _Cache:
    def __init__(self, k, v):
        self.k, self.v, self.s_max = k, v, k.shape[3]


K1_SLOT_KV = [40, 700, 1300, 736, 737, 5, 1000, 77]                       # both sides of the regime switch (736 keys)
_K1 = {}


def _k1_reference(dtype, B):
    """q / k / v at D = 100, two batch rows per slot, every slot its own kv_len; the fp64 references slot by slot"""
    if (dtype, B) not in _K1:
        H, S, D, n = 2, 1344, 100, 16
        g = torch.Generator().manual_seed(B)
        kc = torch.randn(B, H, S, D, generator=g).to(dtype)
        vc = torch.randn(B, H, S, D, generator=g).to(dtype)
        q = (torch.randn(B, n, H, D, generator=g) * 1.5).to(dtype)
        ks = [(5 * b) % 23 if b % 2 else 0 for b in range(B)]
        exact, bound, vis, loose = [], [], [], []
        for s in range(B // 2):
            lo, hi, kv = 2 * s, 2 * s + 2, K1_SLOT_KV[s]
            e, bd, vs = attention_fp64(q[lo:hi], kc[lo:hi], vc[lo:hi], kv, n, ks[lo:hi], dtype)
            k_new, v_new = kc[lo:hi, :, kv:kv + n].transpose(1, 2).contiguous(), vc[lo:hi, :, kv:kv + n].transpose(1, 2).contiguous()
            ref = OracleWindowAttention()(0, q[lo:hi], k_new, v_new, _Cache(kc[None, lo:hi].clone(), vc[None, lo:hi].clone()), kv, ks[lo:hi])
            exact.append(e), bound.append(bd), vis.append(vs), loose.append(ref.float())
        _K1[dtype, B] = (q, kc, vc, ks, torch.cat(exact), torch.cat(bound), torch.cat(vis), torch.cat(loose))
    return _K1[dtype, B]


@pytest.mark.parametrize("regime", ["keysplit", "colsplit"])
@pytest.mark.parametrize("B", [4, 16])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_k1_head_dim_100_batch_rows_from_a_blob_array(dtype, B, regime):
    q, kc, vc, ks, exact, bound, vis, loose = _k1_reference(dtype, B)
    zp = lambda t: F.pad(t, (0, 28)).to(DEV)
    cache = _Cache(zp(kc)[None], zp(vc)[None])
    params = ops.BlobArray(L.IterParams, B // 2, torch.device(DEV))
    for s in range(B // 2):
        v = params.blobs[s].view
        v.n_rows, v.kv_len, v.batch_rows = 16, K1_SLOT_KV[s], 2
    params.upload()
    attn = ops.HipWindowAttention(n_split=4)
    attn.regime, attn.params = regime, params
    if regime == "colsplit":
        assert ops.colsplit_ok(B, 16, 2, 2, 128, dtype)                    # (two heads: 16 batch rows still fit the column split)
    out = attn.attend(0, zp(q), cache, -1, torch.tensor(ks, dtype=torch.int32, device=DEV), head_dim=100)
    torch.cuda.synchronize()
    got = out.cpu()
    assert got.shape == (B, 16, 2, 128) and torch.isfinite(got.float()).all()
    assert not _bits(got[..., 100:]).any()
    got = got[..., :100]
    assert (got[~vis] == 0).all()
    err = (got.float() - loose).abs()                                     # the tolerance of test_k1_k3_attention for 16-bit caches
    print(f"k1 head_dim 100, {B} batch rows, {regime}: max err {float(err[vis].max()):.3e}, mean {float(err[vis].mean()):.3e}")
    assert err[vis].max() < 3e-2 and err[vis].mean() < 3e-3
    e = (got.double() - exact).abs()                                      # ... and its element-wise rounding bound
    over = e > bound
    over[~vis] = False
    assert not over.any(), f"err {float(e[over].max()):.3e} over the rounding bound at {over.nonzero()[0].tolist()} (batch row, row, head, column)"


# ------------------------------------------------------------------------------------------------ d. GPT-3B's width, 128 / 256 rows
class _SdpaAttention:
    """the plain ATen attention of the 16-bit leg: K / V appended to the cache, scaled_dot_product_attention over the visible keys"""
    params = None

    def __call__(self, layer, q, k, v, cache, kv_len, key_start):
        kv_len, (B, n, H, D) = int(kv_len), q.shape
        kc, vc = cache.k[layer], cache.v[layer]
        kc[:, :, kv_len:kv_len + n] = k.transpose(1, 2)
        vc[:, :, kv_len:kv_len + n] = v.transpose(1, 2)
        total = kv_len + n
        j = torch.arange(total, device=q.device)[None, None, None, :]
        i = torch.arange(n, device=q.device)[None, None, :, None]
        vis = (j >= torch.as_tensor(key_start, device=q.device).view(B, 1, 1, 1)) & (j <= kv_len + i)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), kc[:, :, :total], vc[:, :, :total], attn_mask=vis)
        return o.transpose(1, 2)


REAL_KV = [500, 100, 333, 60, 256, 468, 124, 320]
_REAL = {}


def _real_width_references():
    """the two-layer GPT-3B-width model in bf16 (ATen, SDPA) and fp32: eight prompts (CFG pairs), every one at its own KV length; their window
    logits, computed once"""
    if not _REAL:
        import sjd_amd.synthetic as synthetic
        a = BB.LlamaGenArgs(dim=3200, n_layer=2, n_head=32, vocab_size=16384, block_size=576, model_type="c2i", cls_token_num=1, num_classes=1000)
        with torch.device(DEV):
            a16 = BB.LlamaGenBackbone(a, attn=_SdpaAttention()).to(torch.bfloat16).eval()
        synthetic.fill_state_dict_device(a16, seed=5, embed_token_scale=0.5)
        sd = a16.state_dict()
        with torch.device(DEV):
            f32 = BB.LlamaGenBackbone(a, attn=OracleWindowAttention(torch.float32)).eval()
        f32.load_state_dict({k: v.float() for k, v in sd.items()})
        assert a16.layers[0].feed_forward.w1.weight.shape[0] == 8704
        g = torch.Generator(device=DEV).manual_seed(11)
        S, W = 608, 16
        ks = torch.zeros(2, dtype=torch.int32, device=DEV)
        conds = [torch.tensor([(207 + 101 * j) % 1000, 1000], device=DEV) for j in range(8)]
        ctx = [torch.randint(0, 16384, (1, REAL_KV[j] - 1), generator=g, device=DEV).repeat(2, 1) for j in range(8)]
        toks = torch.randint(0, 16384, (8, 1, W), generator=g, device=DEV).repeat(1, 2, 1)
        out = {}
        for name, m in (("aten", a16), ("ref", f32)):
            m.setup_cache(batch=2, s_max=S)
            lg = []
            with torch.no_grad():
                for j in range(8):
                    kv = REAL_KV[j]
                    emb = torch.cat([m.embed_condition(conds[j]), m.tok_embeddings(ctx[j])], dim=1)
                    m.forward_embeds(emb, torch.arange(kv, device=DEV)[None].repeat(2, 1), 0, ks)
                    lg.append(m.forward_window(toks[j], (kv + torch.arange(W, device=DEV))[None].repeat(2, 1), kv, ks).float())
            out[name] = torch.stack(lg)                                    # [8, 2, W, V]
            m.cache = None
        del f32
        torch.cuda.empty_cache()
        _REAL.update(args=a, sd=sd, conds=conds, ctx=ctx, toks=toks, S=S, W=W, **out)
    return _REAL


@pytest.mark.parametrize("n_slots", [4, 8], ids=["128rows", "256rows"])
def test_real_width_window_forward_gpt_3b_many_rows(n_slots, monkeypatch):
    """measured on one MI355X: profiles/llamagen_3b_forward.json (several_prompts)"""
    from sjd_amd.engine_batch import _CacheView
    R = _real_width_references()
    S, W, nb = R["S"], R["W"], 2
    with torch.device(DEV):
        h16 = BB.LlamaGenBackbone(R["args"], attn=ops.HipWindowAttention()).to(torch.bfloat16).eval()
    h16.load_state_dict(R["sd"])
    h16.enable_fused(ops, gemm="sjd", max_rows=n_slots * nb * W, **PAD)
    assert h16.G1_CFG == getattr(CLS, f"G1_CFG_LLAMAGEN_3B_{n_slots * nb * W}ROW")
    h16.setup_cache(batch=n_slots * nb, s_max=S)
    assert h16.cache.k.shape[-1] == 128
    h16.cache.k.view(torch.int16).fill_(-1)                               # (0xFF bytes: a row nobody wrote would show)
    h16.cache.v.view(torch.int16).fill_(-1)
    ks = torch.zeros(n_slots * nb, dtype=torch.int32, device=DEV)
    full = h16.cache
    with torch.no_grad():
        for j in range(n_slots):                                           # every prompt's context through the prefill over ITS batch rows, as the engine does
            kv = REAL_KV[j]
            emb = torch.cat([h16.embed_condition(R["conds"][j]), h16.tok_embeddings(R["ctx"][j])], dim=1)
            h16.cache = _CacheView(full, nb * j, nb * j + nb)
            h16.attn.params = None
            h16.forward_embeds(emb, torch.arange(kv, device=DEV)[None].repeat(2, 1), 0, ks[:2])
            h16.cache = full
            assert not _bits(full.k[:, nb * j:nb * j + nb, :, :kv, 100:]).any() and not _bits(full.v[:, nb * j:nb * j + nb, :, :kv, 100:]).any()
    params = ops.BlobArray(L.IterParams, n_slots, torch.device(DEV))
    for j in range(n_slots):
        v = params.blobs[j].view
        v.n_rows, v.kv_len, v.batch_rows = W, REAL_KV[j], nb
    params.upload()
    toks = R["toks"][:n_slots].reshape(n_slots * nb, W)
    pos = torch.tensor(REAL_KV[:n_slots], device=DEV).repeat_interleave(nb)[:, None] + torch.arange(W, device=DEV)[None]
    seen, real = [], ops.skinny_gemm
    monkeypatch.setattr(ops, "skinny_gemm", lambda x, *a_, **k_: (seen.append(int(x.shape[0])), real(x, *a_, **k_))[1])
    with torch.no_grad():
        h16.attn.params = params
        ho = h16.forward_window(toks, pos, -1, ks, head_partials=True)
        h16.attn.params = None
    torch.cuda.synchronize()
    assert isinstance(ho, ops.HeadOut) and ho.col0 == 0 and ho.urow_off == W
    assert len(seen) == 4 * 2 and set(seen) == {n_slots * nb * W}, "the projections ran on G1 at the full row count"
    hip = _head_logits_from_partials(ho)[:n_slots * nb * W].view(n_slots, nb, W, -1)
    assert torch.isfinite(hip).all()
    for j in range(n_slots):
        e_hip, e_aten = (hip[j] - R["ref"][j]).abs(), (R["aten"][j] - R["ref"][j]).abs()
        rec = dict(rows=n_slots * nb * W, prompt=j, kv=REAL_KV[j], hip_max=float(e_hip.max()), aten_max=float(e_aten.max()), hip_mean=float(e_hip.mean()),
                   aten_mean=float(e_aten.mean()), max_ratio=float(e_hip.max() / e_aten.max()), mean_ratio=float(e_hip.mean() / e_aten.mean()),
                   argmax_agree=float((hip[j].argmax(-1) == R["aten"][j].argmax(-1)).float().mean()))
        print("llamagen GPT-3B-width forward, several prompts:", rec)
        assert e_hip.max() <= 1.5 * e_aten.max() and e_hip.mean() <= 1.5 * e_aten.mean(), rec


# ------------------------------------------------------------------------------------------------ e. loops on the head_dim-100 toy
TOY_T2I = dict(TOY, block_size=64, cls_token_num=12, model_type="t2i", caption_dim=64)       # captions of 12 rows, left-padded: every prompt its own length
WINDOW = 16
_toy = {}


def _toy_model(rows):
    """the toy packed for `rows` rows (its own swept set), shared by the loop tests of that row count"""
    if rows not in _toy:
        m = make_llamagen(TOY_T2I, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
        m.enable_fused(ops, gemm="sjd", max_rows=rows, **PAD)
        _toy[rows] = m
    return _toy[rows]


def _rows_for(n_slots):
    rows = n_slots * 2 * WINDOW
    return 64 if rows <= 64 else (128 if rows <= 128 else 256)


def _spec(model, j, cfg_scale=4.0, top_k=1000):
    from sjd_amd.engine import WindowSpec
    T = model.cls_token_num
    cap = (torch.randn(1, T, TOY_T2I["caption_dim"], generator=torch.Generator().manual_seed(3 + j)) * 0.5).to(DEV, torch.bfloat16)
    cond = torch.cat([cap, torch.zeros_like(cap) + model.cls_embedding.uncond_embedding])
    ks = torch.full((2,), (3 * j + 1) % 11, dtype=torch.int32)             # 12 - key_start caption rows: a length per prompt
    return WindowSpec(first_tokens=None, first_positions=None, key_start=ks, pos_offset=torch.zeros(2, dtype=torch.long), kv_base=T,
                      cond_embeds=model.embed_condition(cond), cond_sampling=dict(cfg_scale=cfg_scale, temperature=1.0, top_k=top_k, top_p=1.0, sample_logits=True))


def _config(seed=7, cfg_scale=4.0, scheme="speculative_jacobi"):
    from sjd_amd.engine import SJDConfig
    N = TOY_T2I["block_size"]
    return SJDConfig(jacobi_loop_interval_l=1, jacobi_loop_interval_r=N - WINDOW - 2, max_num_new_tokens=WINDOW, guidance_scale=cfg_scale, seed=seed,
                     prefix_token_sampler_scheme=scheme, max_length=N)


def _tf_batch(n_prompts, n_slots, use_graph=True, top_k=1000):
    """every prompt's recorded logits, replayed into the CPU oracle with the prompt's own seed from its first image token on, must give that
    prompt's token sequence and accept lengths (tests/test_gpu_llamagen_batch.py::_tf_batch at head_dim 100)"""
    from sjd_amd.engine_batch import SJDBatchEngine
    from sjd_amd.grammar import TopKTopPGrammar
    rows = n_slots * 2 * WINDOW
    model = _toy_model(_rows_for(n_slots))
    T, N = model.cls_token_num, TOY_T2I["block_size"]
    model.setup_cache(batch=2 * n_slots, s_max=((T + N + 64 + 31) // 32) * 32)
    assert model.cache.k.shape[-1] == 128
    model.cache.k.view(torch.int16).fill_(-1)                             # 0xFF bytes: a pad column somebody forgot to write would show below
    model.cache.v.view(torch.int16).fill_(-1)
    cfg = _config()
    eng = SJDBatchEngine(model, 16384, DEV, n_slots, max_window=WINDOW, use_graph=use_graph)
    assert eng.head_partials
    calls, real = [], ops.skinny_gemm
    ops.skinny_gemm = lambda x, *a, **k: (calls.append(int(x.shape[0])), real(x, *a, **k))[1]
    recs = [_Recorder() for _ in range(n_prompts)]
    eng.hook = lambda i, d: recs[i](d)
    try:
        results = eng.decode_many([[] for _ in range(n_prompts)], [_spec(model, j) for j in range(n_prompts)],
                                  [TopKTopPGrammar(top_k, 1.0) for _ in range(n_prompts)], cfg)
    finally:
        ops.skinny_gemm = real
    assert max(calls) == rows, "the window forward did not run on G1 at its full row count"
    firsts = []
    for j, (seq, stats) in enumerate(results):
        c = _loop_cfg(cfg)
        c.seed = cfg.seed + j
        assert len(seq) == N and 0 <= min(seq) and max(seq) < 16384
        seq_ref, tr, _ = _replay(recs[j], seq[:1], lambda cx, n: O.llamagen_rules(cx, n, top_k, 1.0), c, 16384, device=DEV)
        assert seq == seq_ref, f"prompt {j}: token sequences differ"
        assert stats.matched == tr.matched and stats.nfe == len(tr.matched), f"prompt {j}: accept lengths differ"
        assert stats.nfe < N
        firsts.append(seq[0])
    # every cache row a prompt wrote (its caption, its image tokens) has zero pad columns -- the rows of a refilled slot included
    for b in range(2 * n_slots):
        assert not _bits(model.cache.k[:, b, :, :T + N - 1, 100:]).any() and not _bits(model.cache.v[:, b, :, :T + N - 1, 100:]).any()
    return firsts


@pytest.mark.parametrize("n_prompts", [2, 5, 8])
def test_teacher_forced_batch_head_dim_100(n_prompts):
    _tf_batch(n_prompts, n_prompts)                                       # 64, 160 and 256 rows


def test_teacher_forced_batch_head_dim_100_eager_four_prompts():
    _tf_batch(4, 4, use_graph=False)                                      # 128 rows: the 128-row set


def test_teacher_forced_batch_head_dim_100_refill():
    """seven prompts on four slots: a finished slot prefills the next caption over its own (used) cache rows; the first tokens are those of
    the seven-slot run (a prompt's first draw depends on its own seed only)"""
    a = _tf_batch(7, 4)
    b = _tf_batch(7, 7)
    assert a == b


def test_decode_many_one_guidance_scale_per_prompt_head_dim_100():
    """four prompts, four scales, 128 rows: every prompt decodes what it decodes with its own single config at the same number of slots (the
    reference of tests/test_gpu_batch_per_prompt.py)"""
    from sjd_amd.engine_batch import SJDBatchEngine
    from sjd_amd.grammar import TopKTopPGrammar
    scales, seeds, n = [1.5, 3.0, 4.0, 7.5], [7, 1234, 99, 5], 4
    model = _toy_model(128)
    model.setup_cache(batch=2 * n, s_max=((12 + 64 + 64 + 31) // 32) * 32)
    eng = SJDBatchEngine(model, 16384, DEV, n, max_window=WINDOW, use_graph=True)
    gram = lambda: TopKTopPGrammar(1000, 1.0)
    solo = []
    for j in range(n):
        res = eng.decode_many([[] for _ in range(n)], [_spec(model, j, scales[j]) for _ in range(n)], [gram() for _ in range(n)],
                              _config(seeds[j], scales[j]), seeds=[seeds[j]] * n)
        assert all(r[0] == res[0][0] for r in res), "the slots of one solo run agree"
        solo.append((list(res[0][0]), list(res[0][1].matched)))
    assert len({tuple(s) for s, _ in solo}) == n
    res = eng.decode_many([[] for _ in range(n)], [_spec(model, j, scales[j]) for j in range(n)], [gram() for _ in range(n)],
                          [_config(seeds[j], scales[j]) for j in range(n)])
    for j, (seq, stats) in enumerate(res):
        assert seq == solo[j][0], f"prompt {j} (guidance {scales[j]}): token sequences differ"
        assert stats.matched == solo[j][1], f"prompt {j}: accept lengths differ"


# ------------------------------------------------------------------------------------------------ LlamaGenSolver.generate
def _solver(max_rows, padded_batch, seed=7):
    from llamagen.llamagen_solver import LlamaGenSolver, renew_llamagen
    from scheduler.jacobi_iteration_lumina_mgpt import renew_sampler
    N = 64
    model = make_llamagen(dict(TOY, block_size=N), 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
    model.enable_fused(ops, gemm="sjd", max_rows=max_rows, pad_head_dim=True, padded_batch=padded_batch)
    jac = dict(jacobi_loop_interval_l=1, jacobi_loop_interval_r=N - 16 - 2, max_num_new_tokens=16, guidance_scale=4.0, seed=seed,
               multi_token_init_scheme='random', do_cfg=True, image_top_k=1000, text_top_k=10, prefix_token_sampler_scheme='speculative_jacobi')
    model.__class__ = renew_llamagen(model.__class__)
    model._init_new_params(**jac)
    model.__class__ = renew_sampler(model.__class__)
    model._init_new_params(**jac)
    return model, LlamaGenSolver(model=model, image_top_k=1000, image_top_p=1.0)


def test_solver_generate_several_class_ids_head_dim_100():
    kw = dict(temperature=1.0, top_k=1000, top_p=1.0, sample_logits=True)
    model, solver = _solver(128, True)
    labels = torch.tensor([207, 1, 980], device=DEV)
    a = solver.generate(labels, 64, None, cfg_scale=4.0, **kw).cpu()
    assert a.shape == (3, 64) and a.dtype == torch.long and int(a.min()) >= 0 and int(a.max()) < 16384
    assert isinstance(model.last_sjd_stats, list) and len(model.last_sjd_stats) == 3 and all(st.nfe < 64 for st in model.last_sjd_stats)
    assert all(e.head_partials for e in model._sjd_engines.values()) and model.cache.k.shape[-1] == 128
    assert torch.equal(a, solver.generate(labels, 64, None, cfg_scale=4.0, **kw).cpu()), "a second identical call returns identical tokens"
    assert len({tuple(r.tolist()) for r in a}) == 3
    b = solver.generate(labels, 64, None, cfg_scale=[1.5, 4.0, 7.5], temperature=[1.0, 0.8, 1.25], top_k=1000, top_p=1.0, sample_logits=True).cpu()
    assert b.shape == (3, 64) and int(b.min()) >= 0 and int(b.max()) < 16384 and not torch.equal(a, b)     # per-prompt lists: K2a in front of each slot's K2
    # one class id: the one-prompt path on the 64-row packing, which padded_batch leaves alone (tests/test_llamagen_head100_batch.py compares the
    # packed weights bit for bit) -- the same tokens with and without the argument
    one = []
    for flag in (False, True):
        m1, s1 = _solver(64, flag)
        torch.manual_seed(7)
        one.append(s1.generate(labels[:1], 64, None, cfg_scale=4.0, **kw).cpu())
        assert one[-1].shape == (1, 64) and not isinstance(m1.last_sjd_stats, list)
    assert torch.equal(one[0], one[1])
