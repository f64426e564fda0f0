"""LlamaGen's draft-window forward on the hand-written HIP path (LlamaGenBackbone.enable_fused).

  * F2 in its table-rotary mode (SJD_F2_ROPE_TABLE) bit for bit against the ATen rotary (_apply_rope_interleaved) and a plain copy for v;
  * the fused window forward at the GPT-B / XL / XXL shapes against an fp32 forward, in the envelope of the ATen 16-bit forward;
  * teacher-forced loops (the CPU oracle replays the engine's logits) and LlamaGenSolver.generate end to end on a fused model.
"""
import ctypes

import pytest
import torch

import sjd_amd._lib as L
import sjd_amd.backbones as BB
import sjd_amd.ops as ops
from oracle import sjd_oracle as O
from tests.gpu_loop_check import _Recorder, _loop_cfg, _replay
from tests.helpers import llamagen_prefill_sample, make_llamagen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _f2_case(D, dtype, src, H=4, B=2, n=16, cls=120, grid=4, S=200, kv_len=150, blobs=None):
    g = torch.Generator(device=DEV).manual_seed(D + (src == "planes"))
    freqs = BB._rope_2d_table(grid, D, 10000, cls).to(DEV)                 # cls + grid^2 = 136 rows, the first 120 zero
    table = BB._rope_table_extended(freqs, S)
    # batch row 0: condition positions (zero rotary); batch row 1: across the end of the table (clamped rows)
    pos = torch.stack([torch.arange(100, 100 + n), torch.arange(130, 130 + n)]).to(DEV)
    N = 3 * H * D
    if src == "dense":
        qkv = torch.randn(B * n, N, generator=g, device=DEV).to(dtype)
        x, arg = qkv, qkv
    else:
        part = torch.randn(3, 32, N, generator=g, device=DEV)
        x = ((part[0] + part[1]) + part[2])[:B * n].to(dtype)               # F2 sums the planes in chunk order, then rounds once
        arg = ops.Partials(part, 3, N)
    kc = torch.zeros(B, H, S, D, dtype=dtype, device=DEV)
    vc = torch.zeros_like(kc)
    params = None
    if blobs is not None:                                                   # one blob per batch row, each with its own kv_len
        params = ops.BlobArray(L.IterParams, B, torch.device(DEV))
        for b, kv in enumerate(blobs):
            v = params.blobs[b].view
            v.n_rows, v.kv_len, v.batch_rows = n, kv, 1
            params.blobs[b].upload()
    q = ops.qknorm_rope_append(arg, kc, vc, None, None, None, None, None, pos.reshape(-1).contiguous(), B, n, H, H, D,
                               params.blobs[0] if params is not None else None, kv_len if params is None else 0, dtype=dtype, rope_table=table)
    torch.cuda.synchronize()
    fr = freqs[pos.clamp(max=freqs.shape[0] - 1)]
    xq, xk, xv = x.view(B, n, 3 * H, D).split([H, H, H], dim=2)
    rq, rk = BB._apply_rope_interleaved(xq, fr), BB._apply_rope_interleaved(xk, fr)
    assert torch.equal(_bits(q), _bits(rq))
    kvs = blobs if blobs is not None else [kv_len] * B
    for b in range(B):
        r0 = kvs[b]
        assert torch.equal(_bits(kc[b, :, r0:r0 + n]), _bits(rk[b].transpose(0, 1)))
        assert torch.equal(_bits(vc[b, :, r0:r0 + n]), _bits(xv[b].transpose(0, 1)))
        assert not kc[b, :, :r0].any() and not kc[b, :, r0 + n:].any()
    assert not rq[0, :, :, :].any() and rq[1].abs().sum() > 0           # (the condition rows really are zero, the image rows are not)


@pytest.mark.parametrize("src", ["dense", "planes"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_f2_rope_table_bit_exact(D, dtype, src):
    _f2_case(D, dtype, src)


@pytest.mark.parametrize("D", [64, 128])
def test_f2_rope_table_batch_rows_blobs(D):
    _f2_case(D, torch.bfloat16, "planes", blobs=[150, 171])


def test_f2_rope_table_refusals():
    lib = L.load()
    H, D, B, n, S = 2, 64, 1, 4, 64
    qkv = torch.zeros(B * n, 3 * H * D, dtype=torch.bfloat16, device=DEV)
    q = torch.empty(B, n, H, D, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(B, H, S, D, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    tab = torch.zeros(S, D // 2, 2, device=DEV)
    pos = torch.arange(n, device=DEV)
    w = torch.ones(D, dtype=torch.bfloat16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(dt, norm=None, fp8=0, D_=D, n_=n):
        return lib.sjd_qknorm_rope_append_ex(p(qkv), p(q), p(kc), p(vc), p(norm), p(norm), p(norm), p(norm), p(tab), p(pos), B, n_, H, H, D_, S,
                                             dt, fp8, 1.0, 1.0, None, None, 0, None, 0, st)
    assert call(L.DTYPE_BF16 | L.F2_ROPE_TABLE) == 0
    torch.cuda.synchronize()
    assert call(L.DTYPE_BF16 | L.F2_ROPE_TABLE, norm=w) == -1                 # SJD_ERR_BAD_ARG: LlamaGen has no QK-norm
    assert call(L.DTYPE_BF16 | L.F2_ROPE_TABLE, fp8=1) == -2                  # SJD_ERR_UNSUPPORTED: fp8 cache
    assert call(L.DTYPE_BF16 | L.F2_ROPE_TABLE, D_=96) == -2                  # ... head_dim 96
    assert call(L.DTYPE_BF16 | L.F2_ROPE_TABLE, n_=65) == -2                  # ... more than 64 rows
    assert lib.sjd_qknorm_rope_append_fp8(p(qkv), p(q), p(kc), p(vc), None, None, None, None, p(tab), p(pos), B, n, H, H, D, S,
                                          L.DTYPE_BF16 | L.F2_ROPE_TABLE, 1.0, 1.0, None, 0, None, 0, st) == -2


# ------------------------------------------------------------------------------------------------ real-width window forward
PRESETS = {"GPT-B": (12, 12, 768), "GPT-XL": (36, 20, 1280), "GPT-XXL": (48, 24, 1536)}


def _head_logits_from_partials(ho, model):
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


@pytest.mark.parametrize("preset", list(PRESETS))
def test_real_width_window_forward(preset):
    from oracle.attention_ref import OracleWindowAttention
    import sjd_amd.synthetic as synthetic
    n_layer, n_head, dim = PRESETS[preset]
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
    h16.enable_fused(ops, gemm="sjd")
    S, KV = 1216, (1000, 300)
    g = torch.Generator(device=DEV).manual_seed(11)
    cap = torch.randn(2, 120, a.caption_dim, generator=g, device=DEV) * 0.5
    ks = torch.tensor([5, 5], dtype=torch.int32, device=DEV)                 # left-padded caption
    ctx = torch.randint(0, 16384, (1, max(KV) - 120), generator=g, device=DEV).repeat(2, 1)
    for m in (h16, a16, f32):
        m.setup_cache(batch=2, s_max=S)
        dt = m.output.weight.dtype
        emb = torch.cat([m.embed_condition(cap.to(dt)), m.tok_embeddings(ctx)], dim=1)
        if hasattr(m.attn, "params"):
            m.attn.params = None
        m.forward_embeds(emb, torch.arange(max(KV), device=DEV)[None].repeat(2, 1), 0, ks)
    report = []
    for kv in KV:           # (1000 first: the window at 300 overwrites cache rows the longer one would read)
        toks = torch.randint(0, 16384, (1, 16), generator=g, device=DEV).repeat(2, 1)
        pos = (kv + torch.arange(16, device=DEV))[None].repeat(2, 1)
        with torch.no_grad():
            ho = h16.forward_window(toks, pos, kv, ks, head_partials=True)
            assert isinstance(ho, ops.HeadOut) and ho.col0 == 0 and ho.urow_off == 16
            hip = _head_logits_from_partials(ho, h16)[:32].view(2, 16, -1)
            aten = a16.forward_window(toks, pos, kv, ks)
            ref = f32.forward_window(toks, pos, kv, ks)
        e_hip, e_aten = (hip - ref).abs(), (aten - ref).abs()
        agree = float((hip.argmax(-1) == aten.argmax(-1)).float().mean())
        rec = dict(preset=preset, kv=kv, hip_max=float(e_hip.max()), aten_max=float(e_aten.max()), hip_mean=float(e_hip.mean()),
                   aten_mean=float(e_aten.mean()), argmax_agree=agree)
        print("llamagen real-width forward:", rec)
        report.append(rec)
        assert torch.isfinite(hip).all()
        assert e_hip.max() <= 1.5 * e_aten.max() + 1e-3 and e_hip.mean() <= 1.5 * e_aten.mean() + 1e-4, rec


# ------------------------------------------------------------------------------------------------ teacher-forced loops
def _tf_loop(args, scheme, use_graph, pad=0, window=16, seed=7, top_k=1000, cfg_scale=4.0):
    from sjd_amd.engine import SJDConfig, SJDEngine, WindowSpec
    from sjd_amd.grammar import TopKTopPGrammar
    model = make_llamagen(args, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
    model.enable_fused(ops, gemm="sjd")
    T, N = model.cls_token_num, args["block_size"]
    model.setup_cache(batch=2, s_max=((T + N + 64 + 31) // 32) * 32)
    ks = torch.full((2,), pad, dtype=torch.int32, device=DEV)
    if args["model_type"] == "c2i":
        cond = torch.tensor([207, model.num_classes], device=DEV)
    else:
        cap = (torch.randn(1, T, args["caption_dim"], generator=torch.Generator().manual_seed(3)) * 0.5).to(DEV, torch.bfloat16)
        cond = torch.cat([cap, torch.zeros_like(cap) + model.cls_embedding.uncond_embedding])
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
    return stats


def test_teacher_forced_gpt_xl_width_t2i_graph():
    args = dict(dim=1280, n_layer=2, n_head=20, vocab_size=16384, block_size=1024, cls_token_num=120, model_type="t2i", caption_dim=2048)
    _tf_loop(args, "speculative_jacobi", True, pad=9)


@pytest.mark.parametrize("scheme", ["speculative_jacobi", "jacobi"])
def test_teacher_forced_toy_c2i(scheme):
    args = dict(dim=128, n_layer=2, n_head=2, vocab_size=16384, block_size=256, cls_token_num=1, model_type="c2i", num_classes=1000)
    _tf_loop(args, scheme, True)


# ------------------------------------------------------------------------------------------------ LlamaGenSolver end to end
def _solver_tokens(use_graph, seed=7):
    from llamagen.llamagen_solver import LlamaGenSolver, renew_llamagen
    from scheduler.jacobi_iteration_lumina_mgpt import renew_sampler
    args = dict(dim=128, n_layer=2, n_head=2, vocab_size=16384, block_size=256, cls_token_num=1, model_type="c2i", num_classes=1000)
    model = make_llamagen(args, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
    model.enable_fused(ops, gemm="sjd")
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
    assert model.last_sjd_stats.nfe < 256
    assert all(e.head_partials for e in model._sjd_engines.values())
    return toks.cpu()


def test_solver_generate_fused_repeats_and_graph_equals_eager():
    a = _solver_tokens(True)
    b = _solver_tokens(True)
    c = _solver_tokens(False)
    assert torch.equal(a, b)
    assert torch.equal(a, c)
