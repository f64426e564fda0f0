"""Several LlamaGen images per forward on the hand-written HIP path.

  * F2's table rotary (SJD_F2_ROPE_TABLE) for 65..256 rows read from split-K planes, bit for bit against the ATen rotary
    (_apply_rope_interleaved) and a plain copy of v: the four-heads-per-wave kernel, the one-head kernel, SJD_F2_ONE_HEAD, one blob and an
    array of blobs with batch_rows = 2; the refusals that stay;
  * the fused window forward at GPT-XL width with 128 and 256 rows (eight slots, every slot its own KV length) against an fp32 forward, in
    the envelope of the ATen bf16 forward;
  * teacher-forced loops through SJDBatchEngine (conditioning prefilled per slot, continuous batching), every prompt replayed into the CPU
    oracle; LlamaGenSolver.generate with several class labels end to end.
"""
import ctypes

import pytest
import torch

import sjd_amd._lib as L
import sjd_amd.backbones as BB
import sjd_amd.ops as ops
from oracle import sjd_oracle as O
from tests.gpu_loop_check import _Recorder, _loop_cfg, _replay
from tests.helpers import make_llamagen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ a. F2, table mode, many rows
def _f2_many(D, dtype, rows, H, slots=None, cls=120, grid=4, S=512, kv_len=150, one_head=False):
    """B batch rows x n window rows = `rows`, three planes of ceil32(rows) rows.  slots None: two batch rows, one kv_len by value.
    slots = [kv, kv']: two slots of two batch rows each (batch_rows = 2), every slot its own kv_len from its blob."""
    B = 2 if slots is None else 2 * len(slots)
    n = rows // B
    assert B * n == rows
    g = torch.Generator(device=DEV).manual_seed(D + rows + H)
    freqs = BB._rope_2d_table(grid, D, 10000, cls).to(DEV)                 # cls + grid^2 = 136 rows, the first 120 zero
    table = BB._rope_table_extended(freqs, S)
    # even batch rows: from inside the condition rows (zero rotary) on; odd batch rows: across the end of the table (clamped rows)
    pos = torch.stack([torch.arange(s0, s0 + n) for s0 in ([120 - n // 2, 130] * (B // 2))]).to(DEV)
    N = 3 * H * D
    prows = ((rows + 31) // 32) * 32
    part = torch.randn(3, prows, N, generator=g, device=DEV)
    x = ((part[0] + part[1]) + part[2])[:rows].to(dtype)                   # F2 sums the planes in chunk order, then rounds once
    kc = torch.full((B, H, S, D), 7.0, dtype=dtype, device=DEV)
    vc = torch.full((B, H, S, D), -3.0, dtype=dtype, device=DEV)
    params = None
    if slots is not None:
        params = ops.BlobArray(L.IterParams, len(slots), torch.device(DEV))
        for j, kv in enumerate(slots):
            v = params.blobs[j].view
            v.n_rows, v.kv_len, v.batch_rows = n, kv, 2
            params.blobs[j].upload()
    q = ops.qknorm_rope_append(ops.Partials(part, 3, N), kc, vc, None, None, None, None, None, pos.reshape(-1).contiguous(), B, n, H, H, D,
                               params.blobs[0] if params is not None else None, kv_len if params is None else 0, dtype=dtype, rope_table=table,
                               one_head=one_head)
    torch.cuda.synchronize()
    fr = freqs[pos.clamp(max=freqs.shape[0] - 1)]
    xq, xk, xv = x.view(B, n, 3 * H, D).split([H, H, H], dim=2)
    rq, rk = BB._apply_rope_interleaved(xq, fr), BB._apply_rope_interleaved(xk, fr)
    assert torch.equal(_bits(q), _bits(rq))
    for b in range(B):
        r0 = kv_len if slots is None else slots[b // 2]
        assert torch.equal(_bits(kc[b, :, r0:r0 + n]), _bits(rk[b].transpose(0, 1)))
        assert torch.equal(_bits(vc[b, :, r0:r0 + n]), _bits(xv[b].transpose(0, 1)))
        assert bool((kc[b, :, :r0] == 7.0).all()) and bool((kc[b, :, r0 + n:] == 7.0).all())          # rows outside the appended ones
        assert bool((vc[b, :, :r0] == -3.0).all()) and bool((vc[b, :, r0 + n:] == -3.0).all())
    assert not rq[0, :n // 2].any() and rq[0, n // 2:].abs().sum() > 0 and rq[1].abs().sum() > 0          # condition rows really are zero
    return q, kc, vc


F2_SHAPES = [(torch.bfloat16, 96), (torch.bfloat16, 256), (torch.float16, 96)]


@pytest.mark.parametrize("H", [4, 6], ids=["rows_kernel", "one_head_kernel"])
@pytest.mark.parametrize("dtype,rows", F2_SHAPES, ids=["bf16-96", "bf16-256", "fp16-96"])
@pytest.mark.parametrize("D", [64, 128])
def test_f2_rope_table_many_rows_bit_exact(D, dtype, rows, H):
    _f2_many(D, dtype, rows, H)


@pytest.mark.parametrize("H", [4, 6], ids=["rows_kernel", "one_head_kernel"])
@pytest.mark.parametrize("dtype,rows", F2_SHAPES, ids=["bf16-96", "bf16-256", "fp16-96"])
@pytest.mark.parametrize("D", [64, 128])
def test_f2_rope_table_many_rows_slot_blobs(D, dtype, rows, H):
    _f2_many(D, dtype, rows, H, slots=[150, 171])


@pytest.mark.parametrize("D", [64, 128])
def test_f2_rope_table_many_rows_forms_agree(D):
    """the four-heads-per-wave kernel and the one-head kernel (one_head=True: SJD_F2_ONE_HEAD) write the same bits"""
    a = _f2_many(D, torch.bfloat16, 256, 4, slots=[150, 171])
    b = _f2_many(D, torch.bfloat16, 256, 4, slots=[150, 171], one_head=True)
    c = _f2_many(D, torch.float16, 96, 4, one_head=True)
    d = _f2_many(D, torch.float16, 96, 4)
    for u, v in zip(a + c, b + d):
        assert torch.equal(_bits(u), _bits(v))


# ------------------------------------------------------------------------------------------------ b. refusals that stay
def test_f2_rope_table_many_rows_refusals():
    lib = L.load()
    assert lib.sjd_version() >= 103
    H, D, B, n, S = 4, 64, 1, 4, 128
    qkv = torch.zeros(B * n, 3 * H * D, dtype=torch.bfloat16, device=DEV)
    part = torch.zeros(2, 96, 3 * H * 128, device=DEV)                        # planes for up to 96 rows at either head_dim
    q = torch.empty(96, H, 128, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(B, H, S, 128, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    tab = torch.zeros(S, 64, 2, device=DEV)
    pos = torch.arange(96, device=DEV)
    w = torch.ones(128, dtype=torch.bfloat16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    T = L.DTYPE_BF16 | L.F2_ROPE_TABLE

    def call(dt=T, norm=None, fp8=0, D_=D, n_=n, planes=False):
        return lib.sjd_qknorm_rope_append_ex(None if planes else p(qkv), p(q), p(kc), p(vc), p(norm), p(norm), p(norm), p(norm), p(tab), p(pos), B,
                                             n_, H, H, D_, S, dt, fp8, 1.0, 1.0, None, None, 0, p(part) if planes else None, 2 if planes else 0, st)
    assert call(n_=65) == -2                                   # SJD_ERR_UNSUPPORTED: a dense source above 64 rows (returns before any launch)
    assert call(n_=256) == -2
    assert call(n_=96, planes=True, fp8=1) == -2               # ... an fp8 cache
    assert call(n_=96, planes=True, D_=96) == -2               # ... head_dim 96
    assert call(n_=96, planes=True, norm=w) == -1              # SJD_ERR_BAD_ARG: LlamaGen has no QK-norm
    assert call(n_=257, planes=True) == -1                     # ... more rows than the planes of G1 hold
    assert call(n_=96, planes=True) == 0                       # (and the widened mode itself is served: 96 rows into rows [0, 96) of the cache)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ c. real-width forward, 128 / 256 rows
def _head_logits_from_partials(ho):
    """the logits K2 derives from an ops.HeadOut: planes summed in chunk order, the folded final norm as a row scale, the 16-bit rounding
    of the lm_head output"""
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


@pytest.mark.parametrize("n_slots", [4, 8], ids=["128rows", "256rows"])
def test_real_width_forward_many_rows(n_slots, monkeypatch):
    """GPT-XL width, all layers, packed with max_rows=256: n_slots slots x CFG pair x window 16, every slot at its own KV length (its blob of
    the sjd_iter_params array).  Bound: within 1.5 x the error of the ATen bf16 forward of the same rows, both against an fp32 forward."""
    from oracle.attention_ref import OracleWindowAttention
    from sjd_amd.engine_batch import _CacheView
    import sjd_amd.synthetic as synthetic
    n_layer, n_head, dim = 36, 20, 1280
    a = BB.LlamaGenArgs(dim=dim, n_layer=n_layer, n_head=n_head, vocab_size=16384, block_size=1024, model_type="t2i", cls_token_num=120)
    with torch.device(DEV):
        h16 = BB.LlamaGenBackbone(a, attn=ops.HipWindowAttention()).to(torch.bfloat16).eval()
    synthetic.fill_state_dict_device(h16, seed=5, embed_token_scale=0.5)
    sd = h16.state_dict()
    with torch.device(DEV):
        a16 = BB.LlamaGenBackbone(a, attn=ops.HipWindowAttention()).to(torch.bfloat16).eval()
        f32 = BB.LlamaGenBackbone(a, attn=OracleWindowAttention(torch.float32)).eval()
    a16.load_state_dict(sd)
    f32.load_state_dict({k: v.float() for k, v in sd.items()})
    h16.enable_fused(ops, gemm="sjd", max_rows=256)
    assert h16.G1_CFG == BB.LlamaGenBackbone.G1_CFG_LLAMAGEN_256ROW
    W, nb = 16, 2
    B, S = n_slots * nb, 1216
    KV = [1000, 300, 777, 121, 512, 936, 248, 640][:n_slots]
    g = torch.Generator(device=DEV).manual_seed(11)
    cap = torch.randn(B, 120, a.caption_dim, generator=g, device=DEV) * 0.5
    ks = torch.tensor([5, 5, 0, 0, 17, 17, 9, 9, 1, 1, 30, 30, 3, 3, 12, 12][:B], dtype=torch.int32, device=DEV)     # left-padded captions
    ctx = torch.randint(0, 16384, (B, max(KV) - 120), generator=g, device=DEV)
    for m in (h16, a16, f32):
        m.setup_cache(batch=B, s_max=S)
        dt = m.output.weight.dtype
        emb = torch.cat([m.embed_condition(cap.to(dt)), m.tok_embeddings(ctx)], dim=1)
        if hasattr(m.attn, "params"):
            m.attn.params = None
        with torch.no_grad():
            for b0 in range(0, B, 2):           # the context of every slot through the ATen prefill (two batch rows at a time: fp32 memory)
                full = m.cache
                m.cache = _CacheView(full, b0, b0 + 2)
                m.forward_embeds(emb[b0:b0 + 2], torch.arange(max(KV), device=DEV)[None].repeat(2, 1), 0, ks[b0:b0 + 2])
                m.cache = full
    toks = torch.randint(0, 16384, (B, W), generator=g, device=DEV)
    kv_rows = torch.tensor(KV, device=DEV).repeat_interleave(nb)
    pos = kv_rows[:, None] + torch.arange(W, device=DEV)[None]
    # the HIP forward: every slot's kv_len / n_rows from its blob
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
        assert isinstance(ho, ops.HeadOut) and ho.col0 == 0 and ho.urow_off == W
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
    e_hip, e_aten = (hip - ref).abs(), (aten - ref).abs()
    rec = dict(rows=B * W, hip_max=float(e_hip.max()), aten_max=float(e_aten.max()), hip_mean=float(e_hip.mean()), aten_mean=float(e_aten.mean()),
               argmax_agree=float((hip.argmax(-1) == aten.argmax(-1)).float().mean()))
    print("llamagen real-width forward, many rows:", rec)
    assert torch.isfinite(hip).all()
    assert e_hip.max() <= 1.5 * e_aten.max() + 1e-3 and e_hip.mean() <= 1.5 * e_aten.mean() + 1e-4, rec


# ------------------------------------------------------------------------------------------------ d. teacher-forced loops, SJDBatchEngine
TOY_C2I = dict(dim=128, n_layer=2, n_head=2, vocab_size=16384, block_size=256, cls_token_num=1, model_type="c2i", num_classes=1000)
XL_T2I = dict(dim=1280, n_layer=2, n_head=20, vocab_size=16384, block_size=1024, cls_token_num=120, model_type="t2i", caption_dim=2048)


def _tf_batch(args, n_prompts, n_slots, scheme="speculative_jacobi", use_graph=True, window=16, seed=7, top_k=1000, cfg_scale=4.0):
    """every prompt's recorded logits, replayed into the CPU oracle with the prompt's own seed (seed + j) from its first image token on,
    must give that prompt's token sequence and accept lengths"""
    from sjd_amd.engine import SJDConfig, WindowSpec
    from sjd_amd.engine_batch import SJDBatchEngine
    from sjd_amd.grammar import TopKTopPGrammar
    model = make_llamagen(args, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
    rows = n_slots * 2 * window
    model.enable_fused(ops, gemm="sjd", max_rows=64 if rows <= 64 else (128 if rows <= 128 else 256))
    T, N = model.cls_token_num, args["block_size"]
    model.setup_cache(batch=2 * n_slots, s_max=((T + N + 64 + 31) // 32) * 32)
    specs = []
    for j in range(n_prompts):
        if args["model_type"] == "c2i":
            cond = torch.tensor([(207 + 101 * j) % 1000, model.num_classes], device=DEV)
            ks = torch.zeros(2, dtype=torch.int32)
        else:
            cap = (torch.randn(1, T, args["caption_dim"], generator=torch.Generator().manual_seed(3 + j)) * 0.5).to(DEV, torch.bfloat16)
            cond = torch.cat([cap, torch.zeros_like(cap) + model.cls_embedding.uncond_embedding])
            ks = torch.full((2,), 4 * j + 1, dtype=torch.int32)                       # every caption its own left-padding
        specs.append(WindowSpec(first_tokens=None, first_positions=None, key_start=ks, pos_offset=torch.zeros(2, dtype=torch.long), kv_base=T,
                                cond_embeds=model.embed_condition(cond),
                                cond_sampling=dict(cfg_scale=cfg_scale, temperature=1.0, top_k=top_k, top_p=1.0, sample_logits=True)))
    cfg = SJDConfig(jacobi_loop_interval_l=1, jacobi_loop_interval_r=N - window - 2, max_num_new_tokens=window, guidance_scale=cfg_scale,
                    seed=seed, prefix_token_sampler_scheme=scheme, max_length=N)
    eng = SJDBatchEngine(model, 16384, DEV, n_slots, max_window=window, use_graph=use_graph)
    assert eng.head_partials
    calls, real = [], ops.skinny_gemm
    ops.skinny_gemm = lambda x, *a, **k: (calls.append(int(x.shape[0])), real(x, *a, **k))[1]
    recs = [_Recorder() for _ in range(n_prompts)]
    eng.hook = lambda i, d: recs[i](d)
    try:
        results = eng.decode_many([[] for _ in range(n_prompts)], specs, [TopKTopPGrammar(top_k, 1.0) for _ in range(n_prompts)], cfg)
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
    return firsts


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("scheme", ["speculative_jacobi", "jacobi"])
def test_teacher_forced_batch_toy_c2i_3_prompts(scheme, use_graph):
    _tf_batch(TOY_C2I, 3, 3, scheme=scheme, use_graph=use_graph)                     # 96 rows


def test_teacher_forced_batch_toy_c2i_8_prompts():
    _tf_batch(TOY_C2I, 8, 8)                                                         # 256 rows


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_teacher_forced_batch_toy_c2i_continuous(use_graph):
    """five prompts on two slots: a finished slot prefills the next prompt's conditioning over its own rows; the first tokens are those of
    the five-slot run (a prompt's first draw depends on its own seed only)"""
    a = _tf_batch(TOY_C2I, 5, 2, use_graph=use_graph)
    b = _tf_batch(TOY_C2I, 5, 5, use_graph=use_graph)
    assert a == b


def test_teacher_forced_batch_gpt_xl_width_t2i_8_captions():
    _tf_batch(XL_T2I, 8, 8)


# ------------------------------------------------------------------------------------------------ e. LlamaGenSolver end to end
def _solver_many(use_graph, slots, seed=7, labels=(207, 1, 980, 417, 88)):
    from llamagen.llamagen_solver import LlamaGenSolver, renew_llamagen
    from scheduler.jacobi_iteration_lumina_mgpt import renew_sampler
    model = make_llamagen(TOY_C2I, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
    model.enable_fused(ops, gemm="sjd", max_rows=256)
    jac = dict(jacobi_loop_interval_l=1, jacobi_loop_interval_r=256 - 16 - 2, max_num_new_tokens=16, guidance_scale=4.0, seed=seed,
               multi_token_init_scheme='random', do_cfg=True, image_top_k=1000, text_top_k=10, prefix_token_sampler_scheme='speculative_jacobi')
    model.__class__ = renew_llamagen(model.__class__)
    model._init_new_params(**jac)
    model.__class__ = renew_sampler(model.__class__)
    model._init_new_params(**jac)
    model.sjd_use_graph = use_graph
    solver = LlamaGenSolver(model=model, image_top_k=1000, image_top_p=1.0, prompts_per_forward=slots)
    toks = solver.generate(torch.tensor(labels, device=DEV), 256, None, cfg_scale=4.0, temperature=1.0, top_k=1000, top_p=1.0, sample_logits=True)
    assert toks.shape == (len(labels), 256) and toks.dtype == torch.long and int(toks.min()) >= 0 and int(toks.max()) < 16384
    assert isinstance(model.last_sjd_stats, list) and len(model.last_sjd_stats) == len(labels)
    assert all(st.nfe < 256 for st in model.last_sjd_stats)
    assert all(e.head_partials for e in model._sjd_engines.values())
    return toks.cpu()


def test_solver_generate_many_labels():
    a = _solver_many(True, None)                 # five slots (min(N, 256 // 32))
    b = _solver_many(True, None)
    c = _solver_many(False, None)
    assert torch.equal(a, b), "a second identical call returns identical tokens"
    assert torch.equal(a, c), "graph equals eager"
    d = _solver_many(True, 2)                    # two slots, continuous batching: the same five first tokens
    assert torch.equal(a[:, 0], d[:, 0])
