"""GPU: LlamaGen on the lossless 12-bit weight stream (LlamaGenBackbone.enable_fused(compress=True), kernels G1z and their raw-unit fix-up).
Nothing here has a tolerance: the 12-bit kernels rebuild the MFMA operands of the uncompressed packing bit for bit, so split-K planes, logits, cache
rows, tokens, accept counts and probabilities are compared bit for bit against the same call on ops.pack_weight / compress=False.

  * kernel level: ops.skinny_gemm over pack_weight_z against pack_weight at the conditions LlamaGen's widths bring -- a ragged last chunk (K no multiple
    of the chunk), a second row tile, 64-row windows on two and on four column tiles (kernel G1w's 12-bit form), 65 and 128 rows on the sub-tiled
    kernel with a ragged chunk, K = 3200 -- tile-major and step-major, on Gaussian weights, heavy-tailed weights with raw units, and zero column
    blocks as GPT-3B's padded o projection has; the output head's column window at V = 16384;
  * model level: forward_window of a compress=True backbone against compress=False on the same launch shapes at 16 / 32 / 64 / 128 rows, head_dim 64
    and head_dim 100 stored 128 wide; LlamaGenSolver.generate with 1 and 4 prompts; a captured graph; the batch engine's row limit."""
import pytest
import torch

import sjd_amd.launch_shapes as LS
import sjd_amd.ops as ops
from tests.helpers import make_llamagen
from tests.test_gpu_llamagen_head100 import TOY as TOY100
from tests.test_gpu_llamagen_quant import _same_head, _window

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------------ a. kernel level
def _weight(kind, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    if kind == "heavy":
        # Student-t with two degrees of freedom (tens of out-of-window weights per unit: wide headers), and the first column tile log-normal over
        # ~6 binades of standard deviation: far more than 127 weights of a unit outside any sixteen-binade window -- raw units
        w = w / torch.sqrt(-torch.log(torch.rand(N, K, generator=g).clamp_min(1e-6)))
        w[:32] = w[:32] * torch.exp(4.0 * torch.randn(32, K, generator=g))
    if kind == "zero_block":          # columns 100..127 of every 128: the pad positions of heads of 100 stored 128 wide
        w.view(N, K // 128, 128)[:, :, 100:] = 0
    return w.to(torch.bfloat16).to(DEV)


# M, N, K, KC, column tiles per workgroup
SHAPES = [(32, 96, 1280, 896, 2),          # ragged last chunk: 896 + 384
          (33, 96, 1280, 896, 2),          # second row tile
          (64, 64, 768, 384, 2),           # 64-row window, whole chunks staged in LDS
          (64, 64, 768, 384, 4),           # ... on four column tiles: kernel G1w's 12-bit form + the fix-up launch
          (65, 64, 1280, 896, 2),          # sub-tiled kernel, ragged chunk, three row tiles
          (128, 64, 1280, 896, 4),         # ... four row tiles
          (16, 32, 3200, 1664, 1)]         # GPT-3B width: 1664 + 1536


@pytest.mark.parametrize("kind", ["gaussian", "heavy", "zero_block"])
@pytest.mark.parametrize("step_major", [False, True], ids=["tile_major", "step_major"])
@pytest.mark.parametrize("M,N,K,KC,waves", SHAPES, ids=[f"M{s[0]}-N{s[1]}-K{s[2]}-KC{s[3]}-w{s[4]}" for s in SHAPES])
def test_g1z_planes_equal_g1_at_llamagen_shapes(M, N, K, KC, waves, step_major, kind):
    w = _weight(kind, N, K, M + N + K)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(K + M)).to(torch.bfloat16).to(DEV)
    wp, wz = ops.pack_weight(w, KC, step_major), ops.pack_weight_z(w, KC, step_major)
    assert isinstance(wz, ops.PackedZ) and (wz.KC, wz.step_major) == (KC, step_major)
    if kind == "gaussian":
        assert wz.n_raw == 0 and wz.stats["raw_units"] == 0 and wz.nbytes() < 0.80 * wp.numel() * 2
    else:          # (the verbatim units: multiplied in the kernel up to 64 rows on two tiles, by the fix-up launch behind the other kernels)
        assert wz.n_raw > 0 and wz.stats["raw_units"] == wz.n_raw
    if kind == "heavy" and N > 32:          # (more than one column tile: the others carry exceptions in their headers)
        assert wz.n_exceptions > 0 and wz.n_raw < wz.stats["units"]
    ref = ops.skinny_gemm(x, wp, N, K, KC, waves, step_major)
    got = ops.skinny_gemm(x, wz, N, K, KC, waves, step_major)
    torch.cuda.synchronize()
    assert got.n_chunks == ref.n_chunks == -(-K // KC) and got.data.shape == ref.data.shape == (ref.n_chunks, 32 * -(-M // 32), N)
    assert torch.equal(_bits(got.data), _bits(ref.data))
    assert bool(torch.isfinite(ref.data).all()) and all(float(ref.data[c, :M].abs().max()) > 0 for c in range(ref.n_chunks))


@pytest.mark.parametrize("M,waves", [(32, 4), (64, 4), (64, 8), (128, 4)], ids=["32rows", "64rows-g1w", "64rows", "128rows"])
def test_g1z_head_column_window_at_v_16384(M, waves):
    """the output head's launch: V = 16384, K = 768 in chunks of 640 (ragged: 640 + 128), step-major; a column window that starts and ends inside the matrix,
    with one raw tile inside it and one outside"""
    V, K, KC, c0, nc = 16384, 768, 640, 5024, 4096
    g = torch.Generator().manual_seed(M)
    w = torch.randn(V, K, generator=g) / K ** 0.5
    for t in (3, 200):          # tiles 3 (outside the window) and 200 (columns 6400..6431, inside): raw
        w[32 * t:32 * t + 32] *= torch.exp(4.0 * torch.randn(32, K, generator=g))
    w = w.to(torch.bfloat16).to(DEV)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    wp, wz = ops.pack_weight(w, KC, True), ops.pack_weight_z(w, KC, True)
    assert wz.n_raw == 4 and sorted(set(wz.raw_index[:, 1].tolist())) == [3, 200]
    ref = ops.skinny_gemm_cols(x, wp, V, K, KC, c0, nc, waves, True).data
    got = ops.skinny_gemm_cols(x, wz, V, K, KC, c0, nc, waves, True).data
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (2, 32 * -(-M // 32), nc) and torch.equal(_bits(got), _bits(ref))
    assert float(ref[:, :M].abs().max()) > 0 and float(ref[1, :M, 6400 - c0:6432 - c0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ b. model level
TOY64 = dict(dim=256, n_layer=2, n_head=4, vocab_size=16384, block_size=256, cls_token_num=1, model_type="c2i", num_classes=1000)
MODELS = {"head_dim_64": (TOY64, {}), "head_dim_100": (TOY100, dict(pad_head_dim=True, padded_batch=True))}


def _backbone(args, compress, **kw):
    m = make_llamagen(args, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
    pad = bool(kw.get("pad_head_dim"))
    cfg, head = LS.LLAMAGEN_Z_SETS[pad, 128]
    if not compress:          # the same launch shapes, spelled out (today the 12-bit sets ARE the 16-bit ones)
        m.G1_CFG, m.HEAD_CFG = dict(cfg), tuple(head)
    m.enable_fused(ops, gemm="sjd", max_rows=128, compress=compress, **kw)
    assert m.G1_CFG == cfg and tuple(m.HEAD_CFG) == tuple(head) and m.compress is compress
    return m


@pytest.fixture(scope="module", params=list(MODELS))
def pair(request):
    args, kw = MODELS[request.param]
    out = [_backbone(args, c, **kw) for c in (True, False)]
    for m in out:
        m.setup_cache(batch=8, s_max=64)
    mz, mp = out
    assert all(isinstance(z, ops.PackedZ) for d in mz._packed for z in d.values()) and isinstance(mz._packed_head, ops.PackedZ)
    assert all(isinstance(t, torch.Tensor) for d in mp._packed for t in d.values()) and isinstance(mp._packed_head, torch.Tensor)
    st = mz.compress_stats
    assert st["compressed"] == st["matrices"] == 9 and st["declined"] == 0
    if kw:          # the padded wo: zero pad columns in every unit, and still packed
        assert mz._head_pad == 128 and mz._packed[0]["o"].K == 1024 and st["raw_units"] > 0
    else:
        assert 0.74 < st["bytes_packed"] / st["bytes_raw"] < 0.80
    return out


@pytest.mark.parametrize("rows", [16, 32, 64, 128])
def test_window_logits_equal_the_uncompressed_backbone(pair, rows, monkeypatch):
    seen, real = [], ops.skinny_gemm
    monkeypatch.setattr(ops, "skinny_gemm", lambda x, w, *a, **k: (seen.append((int(x.shape[0]), type(w).__name__)), real(x, w, *a, **k))[1])
    args = _window(rows // 16, 16, rows)
    for m in pair:
        m.cache.k.fill_(7.0)
        m.cache.v.fill_(7.0)
    with torch.no_grad():
        hz, hp = [m.forward_window(*args, head_partials=True) for m in pair]
        lz, lp = [m.forward_window(*args) for m in pair]
    torch.cuda.synchronize()
    _same_head(hz, hp, rows)
    assert lz.shape == (rows // 16, 16, 16384) and torch.equal(_bits(lz), _bits(lp)) and bool(torch.isfinite(lz).all())
    assert len(seen) == 2 * 2 * 4 * 2 and {k for r, k in seen if r == rows} == {"PackedZ", "Tensor"} and {r for r, _ in seen} == {rows}
    for a, b in ((pair[0].cache.k, pair[1].cache.k), (pair[0].cache.v, pair[1].cache.v)):
        assert torch.equal(_bits(a), _bits(b)) and float(a[:, :rows // 16, :, :16].float().abs().max()) > 0


def test_captured_graph_replays_the_first_run(pair):
    mz = pair[0]
    args = _window(2, 16, 5)
    with torch.no_grad():
        first = mz.forward_window(*args, head_partials=True)
        torch.cuda.synchronize()
        ref, ref_ss = first.part.data.clone(), first.row_norm[0].clone()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            mz.forward_window(*args, head_partials=True)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            cap = mz.forward_window(*args, head_partials=True)
    cap.part.data.fill_(float("nan"))
    for _ in range(2):
        gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(cap.part.data), _bits(ref)) and torch.equal(_bits(cap.row_norm[0][:, :32]), _bits(ref_ss[:, :32]))


def _generate(compress, labels, seed=7):
    """LlamaGenSolver.generate on the toy: ids, per-prompt accept counts, the engines' probability buffers as the last iteration left them"""
    from llamagen.llamagen_solver import LlamaGenSolver, renew_llamagen
    from scheduler.jacobi_iteration_lumina_mgpt import renew_sampler
    model = _backbone(TOY64, compress)
    jac = dict(jacobi_loop_interval_l=1, jacobi_loop_interval_r=256 - 16 - 2, max_num_new_tokens=16, guidance_scale=4.0, seed=seed,
               multi_token_init_scheme='random', do_cfg=True, image_top_k=1000, text_top_k=10, prefix_token_sampler_scheme='speculative_jacobi')
    model.__class__ = renew_llamagen(model.__class__)
    model._init_new_params(**jac)
    model.__class__ = renew_sampler(model.__class__)
    model._init_new_params(**jac)
    model.sjd_use_graph = True
    solver = LlamaGenSolver(model=model, image_top_k=1000, image_top_p=1.0)
    torch.manual_seed(seed)
    toks = solver.generate(torch.tensor(labels, device=DEV), 256, None, cfg_scale=4.0, temperature=1.0, top_k=1000, top_p=1.0, sample_logits=True)
    torch.cuda.synchronize()
    assert toks.shape == (len(labels), 256) and int(toks.min()) >= 0 and int(toks.max()) < 16384
    stats = model.last_sjd_stats if isinstance(model.last_sjd_stats, list) else [model.last_sjd_stats]
    assert len(stats) == len(labels) and all(st.nfe < 256 for st in stats) and all(e.head_partials for e in model._sjd_engines.values())
    probs = [(e.probs_all if hasattr(e, "probs_all") else e.probs).clone() for e in model._sjd_engines.values()]
    return toks.cpu(), [list(st.matched) for st in stats], probs


@pytest.mark.parametrize("labels", [(207,), (207, 1, 980, 417)], ids=["1-prompt", "4-prompts-128-rows"])
def test_solver_generate_equals_the_uncompressed_backbone(labels):
    (tz, az, pz), (tp, ap, pp) = _generate(True, labels), _generate(False, labels)
    assert torch.equal(tz, tp), "the 12-bit backbone accepted different tokens"
    assert az == ap and len(pz) == len(pp) >= 1
    assert all(a.shape == b.shape and torch.equal(_bits(a), _bits(b)) and float(a.max()) > 0 for a, b in zip(pz, pp))
    assert len({tuple(r.tolist()) for r in tz}) == len(labels)


def test_an_engine_that_asks_for_160_rows_is_refused_before_any_launch(monkeypatch):
    from sjd_amd.engine_batch import SJDBatchEngine
    m = _backbone(TOY64, True)
    m.setup_cache(batch=10, s_max=64)
    monkeypatch.setattr(ops, "skinny_gemm", lambda *a, **k: pytest.fail("a projection was launched"))
    monkeypatch.setattr(ops, "skinny_gemm_cols", lambda *a, **k: pytest.fail("the head was launched"))
    with pytest.raises(ValueError, match=r"at most max_rows=128 rows.*= 160"):
        SJDBatchEngine(m, 16384, DEV, 5)
    assert isinstance(SJDBatchEngine(m, 16384, DEV, 4), SJDBatchEngine)
