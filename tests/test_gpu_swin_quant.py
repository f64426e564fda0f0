"""GPU: swin-norm (30B-class) backbones decoded from e4m3 / MXFP4 weights (enable_fused(weights=..., swin_quant=True)).

  * the K = 8192 form of G1sq4 (sjd_gateup_silu with SJD_G1S_CHUNKS(4)): bit for bit G1q4(KC = 2048) + F3 on the same PackedQ4, and on
    pack_weight(dequant); nothing outside y [M, I] is written; what it does not serve is refused before any launch;
  * a toy swin-norm model: every stream and its "_as_bf16" twin write the same window logits at 2, 32 and 64 rows; the prefill is not quantised;
  * two layers at the full 30B width through SJDEngine (hipGraph): "mxfp4" and its twin decode the same tokens, the fused launch is on the route,
    and the window logits sit inside the project's envelope around an fp32 forward of the dequantised weights.
"""
import ctypes
import dataclasses
import json

import pytest
import torch

from tests.test_gpu_q4 import q4_weight
from tests.test_gpu_swin_norm import _IndependentSwinForward, _allowed_columns

pytestmark = pytest.mark.gpu

W4, W8 = 0x4000, 0x2000          # SJD_G1_W4_MXFP4, SJD_G1_W8_E4M3
UNSUPPORTED, BAD_ARG = -2, -1
CH4 = 4 << 8                     # SJD_G1S_CHUNKS(4)
K30 = 8192
POISON = 0x7fc1                  # a bf16 NaN no kernel writes


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return "cuda:0"


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.fixture(scope="module")
def kernel_refs(dev):
    """per (I, step_major): the weight, its PackedQ4 in four chunks of 2048 and the 16-bit packing of its dequantised values -- made once, never written"""
    import sjd_amd.ops as ops
    out = {}
    for I in (64, 192):
        w = q4_weight(2 * I, K30, I + K30, dev)
        for sm in (False, True):
            pq = ops.pack_weight_q4(w, 2048, sm)
            out[I, sm] = (pq, ops.pack_weight(pq.dequant(), 2048, sm))
    return out


@pytest.mark.parametrize("step_major", [False, True])
@pytest.mark.parametrize("with_norm", [False, True])
@pytest.mark.parametrize("I", [64, 192])                 # 192: three workgroups, the last one's tiles are the odd pair 4, 5
@pytest.mark.parametrize("M", [1, 9, 32])
def test_fused_gateup_at_k8192_is_g1q4_then_f3(dev, kernel_refs, M, I, with_norm, step_major):
    import sjd_amd._lib as L
    import sjd_amd.ops as ops
    pq, wp = kernel_refs[I, step_major]
    assert pq.KC == 2048 and pq.nbytes() == 2 * I * K30 * 17 // 32 and ops.gateup_silu_chunked_ok(M, I, K30, pq.KC)
    g = torch.Generator().manual_seed(100 * M + I)
    x = torch.randn(M, K30, generator=g).to(torch.bfloat16).to(dev)
    # the row scale of a folded norm: sums of squares in four slices of 32 rows (any positive numbers do: both routes read the same ones)
    rn = ((torch.rand(4, 32, generator=g) * 3000 + 50).to(dev), K30, 1e-5) if with_norm else None
    unfused = ops.silu_mul(ops.skinny_gemm(x, pq, 2 * I, K30, 2048, 8, step_major), rows=M, dtype=x.dtype, row_norm=rn)          # G1q4 + F3, four planes
    ref16 = ops.silu_mul(ops.skinny_gemm(x, wp, 2 * I, K30, 2048, 8, step_major), rows=M, dtype=x.dtype, row_norm=rn)           # G1 + F3 on the dequantised weight
    # the fused launch writes into the middle of a poisoned buffer
    buf = torch.full(((M + 2) * I,), POISON, dtype=torch.int16, device=dev)
    y = buf[I:I + M * I]
    rc = L.load().sjd_gateup_silu(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(pq.data.data_ptr()), ctypes.c_void_p(y.data_ptr()), M, I, K30,
                                  int(step_major) | CH4, L.DTYPE_BF16 | W4, ops._row_norm(rn), ops._stream())
    assert rc == 0, rc          # (the parent commit: SJD_ERR_UNSUPPORTED)
    got = ops.gateup_silu(x, pq, I, K30, step_major, row_norm=rn)                # the same launch through ops
    torch.cuda.synchronize()
    assert got.shape == (M, I) and got.dtype == torch.bfloat16
    assert torch.equal(unfused.view(torch.int16), ref16.view(torch.int16))
    assert torch.equal(y.view(M, I), unfused.view(torch.int16)), (y.view(M, I).view(torch.bfloat16).float() - unfused.float()).abs().max()
    assert torch.equal(got.view(torch.int16), unfused.view(torch.int16))
    assert bool((buf[:I] == POISON).all()) and bool((buf[I + M * I:] == POISON).all())
    assert float(unfused.float().abs().max()) > 0 and bool(torch.isfinite(unfused.float()).all())


def test_fused_gateup_refusals_before_any_launch(dev):
    import sjd_amd._lib as L
    import sjd_amd.ops as ops
    lib = L.load()
    assert L.G1S_CHUNKS_SHIFT == 8
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    BF = L.DTYPE_BF16 | W4
    # sjd_gateup_silu(x, w_packed, y, M, I, K, step_major | SJD_G1S_CHUNKS(n), dtype, row_norm, stream)
    assert lib.sjd_gateup_silu(p, p, p, 33, 64, K30, CH4, BF, None, None) == UNSUPPORTED                          # 33 rows
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, K30, CH4, L.DTYPE_F16 | W4, None, None) == UNSUPPORTED            # fp16
    assert lib.sjd_gateup_silu(p, p, p, 32, 96, K30, CH4, BF, None, None) == UNSUPPORTED                          # I % 64
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, K30, 0, BF, None, None) == UNSUPPORTED                            # a weight packed with KC = 4096: two chunks
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, K30, 1 | (2 << 8), BF, None, None) == UNSUPPORTED
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, K30, 8 << 8, BF, None, None) == UNSUPPORTED                       # ... with KC = 1024
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, 4096, CH4, BF, None, None) == UNSUPPORTED                         # four chunks at another K
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, K30, CH4, L.DTYPE_BF16 | W8, None, None) == UNSUPPORTED           # the e4m3 stream has no such form
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, K30, CH4, L.DTYPE_BF16, None, None) == UNSUPPORTED                # nor has the 16-bit one
    assert lib.sjd_gateup_silu(p, p, p, 32, 64, K30, CH4, BF | W8, None, None) == BAD_ARG                         # both weight bits
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0
    # through ops: a PackedQ4 in two chunks of 4096 is refused by the library
    w = q4_weight(128, K30, 5, dev)
    x = torch.zeros(32, K30, dtype=torch.bfloat16, device=dev)
    with pytest.raises(L.SjdLibraryError):
        ops.gateup_silu(x, ops.pack_weight_q4(w, 4096, True, gateup=True), 64, K30, True)
    with pytest.raises(L.SjdLibraryError):
        ops.gateup_silu(torch.zeros(33, K30, dtype=torch.bfloat16, device=dev), ops.pack_weight_q4(w, 2048, True), 64, K30, True)


# ------------------------------------------------------------------------------------------------ a toy swin-norm model
TOY = dict(vocab_size=9216, hidden_size=512, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
           max_position_embeddings=512, swin_norm=True, model_parallel_size=2)
TOY_CFG = dict(qkv=(256, 4, True), o=(128, 3, False), gate_up=(256, 8, True), down=(128, 2, False))


def _toy(dev, weights):
    import sjd_amd.backbones as BB
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    m = BB.ChameleonBackbone(BB.ChameleonArgs(qk_norm=True, **TOY), attn=ops.HipWindowAttention(n_split=2)).eval()
    synthetic.fill_state_dict(m, seed=29, embed_token_scale=0.25)
    m = m.to(device=dev, dtype=torch.bfloat16)
    m.G1_CFG = dict(TOY_CFG)
    if weights is None:
        m.enable_fused(ops, gemm="sjd")
    else:
        m.enable_fused(ops, gemm="sjd", weights=weights, swin_quant=True)
    m.setup_cache(batch=2, s_max=128)
    return m


@pytest.fixture(scope="module")
def toy_models(dev):
    return {wt: _toy(dev, wt) for wt in (None, "mxfp4", "mxfp4_as_bf16", "e4m3", "e4m3_as_bf16")}


@pytest.mark.parametrize("n", [1, 16, 32])          # 2, 32 and 64 rows
@pytest.mark.parametrize("stream", ["mxfp4", "e4m3"])
def test_toy_swin_window_logits_equal_the_twins(dev, toy_models, stream, n):
    import sjd_amd.ops as ops
    mq, m16 = toy_models[stream], toy_models[stream + "_as_bf16"]
    assert isinstance(mq._packed[1]["down"], ops.PackedQ4 if stream == "mxfp4" else ops.PackedQ8) and isinstance(m16._packed[1]["down"], torch.Tensor)
    assert mq.args.swin_norm and mq.args.model_parallel_size == 2 and not mq._fold_norm
    g = torch.Generator().manual_seed(n)
    tok = torch.randint(4, 8196, (2, n), generator=g).to(dev)
    pos = torch.arange(n)[None].repeat(2, 1).to(dev)
    ks = torch.zeros(2, dtype=torch.int32, device=dev)
    with torch.no_grad():
        outs = [m.forward_window(tok, pos, 0, ks).float() for m in (mq, m16, toy_models[None])]
    torch.cuda.synchronize()
    assert outs[0].shape == (2, n, 9216) and bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert not torch.equal(outs[0], outs[2])                                      # the quantised model is another model
    assert mq.gateup_route[2 * n] == "g1+f3" == m16.gateup_route[2 * n]           # hidden 512: no fused form


@pytest.mark.parametrize("weights", ["mxfp4", "e4m3"])
def test_toy_swin_prefill_is_not_quantised(dev, toy_models, weights):
    n = 40                                                                        # more than 32 rows per batch row: the prefill path
    tok = torch.randint(4, 8196, (2, n), generator=torch.Generator().manual_seed(3)).to(dev)
    pos = torch.arange(n)[None].repeat(2, 1).to(dev)
    ks = torch.zeros(2, dtype=torch.int32, device=dev)
    with torch.no_grad():
        a = toy_models[weights].forward_window(tok, pos, 0, ks).float()
        b = toy_models[None].forward_window(tok, pos, 0, ks).float()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and float(a.abs().max()) > 0


def test_toy_swin_refusals_on_the_device(dev):
    import sjd_amd.backbones as BB
    import sjd_amd.ops as ops
    from sjd_amd.engine_batch import SJDBatchEngine
    m = _toy(dev, "mxfp4")
    with pytest.raises(ValueError):
        SJDBatchEngine(m, 9216, dev, n_prompts=2)                                 # the batch engine keeps refusing swin-norm backbones
    with pytest.raises(ValueError, match="fp8 KV cache"):
        m.setup_cache(batch=2, s_max=128, dtype=torch.float8_e4m3fn)
    assert BB.CHAMELEON_30B.swin_norm and ops is not None


# ------------------------------------------------------------------------------------------------ the full 30B-class width
def _model_30b(dev, weights):
    import sjd_amd.backbones as BB
    import sjd_amd.launch_shapes as LS
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    margs = dataclasses.replace(BB.CHAMELEON_30B, num_hidden_layers=2)
    with torch.device(dev):
        model = BB.ChameleonBackbone(margs, attn=ops.HipWindowAttention()).to(torch.bfloat16).eval()
    synthetic.fill_state_dict_device(model, seed=0, embed_token_scale=0.7)
    model.enable_fused(ops, gemm="sjd", weights=weights, swin_quant=True)
    assert not model._fold_norm and model.G1_CFG == LS.G1_CFG_30B_Q4 and model._packed[0]["gate_up"].numel() == 44032 * 8192
    model.gateup_fused = True          # the K = 8192 launch (off by default: profiles/swin30b_quant.json); the twin has no 4-bit copy for it to take
    model.setup_cache(batch=2, s_max=256)
    return model


@torch.no_grad()
def test_decode_at_30b_width_from_mxfp4_weights(dev):
    """two swin-norm layers at the full 30B-class width on "mxfp4" and on its twin: SJDEngine (hipGraph, window 16 with CFG = 32 rows) decodes the same
    tokens with the same accept lengths; the fused gate|up launch was on the route of the one and not of the other; the bytes are 4.25 bits per
    weight; and the window logits keep the envelope of tests/test_gpu_swin_norm.py -- |hip16 - fp32| <= 1.5 x |aten16 - fp32| in max and mean, plus its
    argmax rule -- around independent forwards of the model the route computes: the prompt through the 16-bit parameters (the prefill is not
    quantised), the windows through the packed copies' dequant()."""
    import sjd_amd.ops as ops
    from sjd_amd.engine import SJDEngine, SJDConfig
    from sjd_amd.frontends import lumina_window_spec, lumina_prompt
    from sjd_amd.grammar import LuminaGrammar
    V, window, P, seed = 65536, 16, 100, 17
    prompt = lumina_prompt(P, 48, 48, seed=seed)
    spec = lumina_window_spec(prompt, dev)
    cfg = SJDConfig(jacobi_loop_interval_l=0, jacobi_loop_interval_r=48 * 48 + 48 - 13, max_num_new_tokens=window, guidance_scale=3.0,
                    seed=seed, max_length=P + 120, eos_token_ids=(8196,))
    runs = {}
    for wt in ("mxfp4", "mxfp4_as_bf16"):
        model = _model_30b(dev, wt)
        eng = SJDEngine(model, V, dev, max_window=window, use_graph=True)
        recs = []

        def hook(d):
            n = d["n_rows"]
            lo, hi = _allowed_columns(d["rules"], V)
            live = [i for i, r in enumerate(d["rules"][:n]) if r.forced < 0]
            recs.append(dict(first=d["first"], n=n, kv_len=int(eng.params.view.kv_len), cols=(lo, hi), live=live,
                             graph=(not d["first"]) and eng.logit_columns(d["rules"]) in eng.captured_column_windows(),
                             ids=None if d["first"] else eng.input_ids[:, :n].clone(),
                             hip=torch.stack([d["logits_c"][:, lo:hi], d["logits_u"][:, lo:hi]]).clone()))

        eng.hook = hook
        seq, stats = eng.decode(prompt, spec, LuminaGrammar(2000, 10), cfg, warmup_iters=0, timed_iters=8)
        eng.hook = None
        torch.cuda.synchronize()
        runs[wt] = dict(model=model, seq=list(seq), matched=list(stats.matched), recs=recs)
        del eng
    a, b = runs["mxfp4"], runs["mxfp4_as_bf16"]
    m4, m16 = a["model"], b["model"]
    assert a["seq"] == b["seq"] and len(a["seq"]) > len(prompt) and a["matched"] == b["matched"] and len(a["matched"]) >= 8
    assert all(torch.equal(ra["hip"].view(torch.int32), rb["hip"].view(torch.int32)) for ra, rb in zip(a["recs"], b["recs"]))
    # the route: 32 rows on the fused launch for the 4-bit copy, G1 + F3 for the twin
    assert isinstance(m4._packed[0]["gate_up"], ops.PackedQ4) and m4._packed[0]["gate_up"].KC == 2048
    assert m4.gateup_route.get(2 * window) == "fused" and m16.gateup_route.get(2 * window) == "g1+f3", (m4.gateup_route, m16.gateup_route)
    dims = [(10240, 8192), (8192, 8192), (44032, 8192), (8192, 22016)]
    assert m4.compress_stats["q4_bytes_packed"] == 2 * sum(N * K * 17 // 32 for N, K in dims) == m4.packed_bytes()
    assert m4.compress_stats["q4_matrices"] == 8 and 0 < m4.compress_stats["rel_rms_error"] < 0.2
    # the twin's parameters become the packed copies' dequant(): the model the window forwards compute
    for l4, l16 in zip(m4._packed, m16.model.layers):
        at, mlp = l16.self_attn, l16.mlp
        qkv, gu = l4["qkv"].dequant(), l4["gate_up"].dequant()
        nq, nk, ni = at.q_proj.weight.shape[0], at.k_proj.weight.shape[0], mlp.gate_proj.weight.shape[0]
        at.q_proj.weight.data, at.k_proj.weight.data, at.v_proj.weight.data = qkv[:nq], qkv[nq:nq + nk], qkv[nq + nk:]
        mlp.gate_proj.weight.data, mlp.up_proj.weight.data = gu[:ni], gu[ni:]
        at.o_proj.weight.data, mlp.down_proj.weight.data = l4["o"].dequant(), l4["down"].dequant()
    m16._packed = None
    torch.cuda.empty_cache()
    recs = a["recs"]
    wins = [r for r in recs if not r["first"] and r["n"] > 1]
    assert recs[0]["first"] and len(wins) >= 3 and any(r["graph"] for r in wins)
    ks, po = spec.key_start.to(dev), spec.pos_offset.to(dev)
    outs = {}
    for tag, fdt in (("aten16", torch.bfloat16), ("fp32", torch.float32)):
        pre, win = _IndependentSwinForward(m4, fdt), _IndependentSwinForward(m16, fdt)
        win.k, win.v = pre.k, pre.v                                                # one KV cache: the prompt's rows come from the 16-bit parameters
        res = []
        for r in recs:
            if r["first"]:
                res.append(pre.forward(spec.first_tokens.to(dev), 0, ks, po, r["cols"])[:, -1:])
            else:
                win.rollback(r["kv_len"])
                res.append(win.forward(r["ids"], r["kv_len"], ks, po, r["cols"]))
        outs[tag] = res
        del pre, win
        torch.cuda.empty_cache()
    rep = dict(family="chameleon30b_2layers_mxfp4", iterations=[])
    for i, r in enumerate(recs):
        rows = [0] if r["first"] else r["live"]
        if not rows:
            continue
        hip, a16, f32 = r["hip"][:, rows], outs["aten16"][i][:, rows], outs["fp32"][i][:, rows]
        assert torch.isfinite(hip).all() and hip.shape == a16.shape == f32.shape
        e_hip, e_aten = (hip - f32).abs(), (a16 - f32).abs()
        ia, ib = hip.argmax(-1), a16.argmax(-1)
        gap = (f32.gather(-1, ib[..., None]) - f32.gather(-1, ia[..., None])).abs()[..., 0]
        ok = (ia == ib) | (gap <= 2.0 * e_aten.max())
        it = dict(first=r["first"], graph=bool(r["graph"]), rows=len(rows), kv_len=r["kv_len"], hip16_max=round(float(e_hip.max()), 5),
                  hip16_mean=round(float(e_hip.mean()), 6), aten16_max=round(float(e_aten.max()), 5), aten16_mean=round(float(e_aten.mean()), 6),
                  argmax_agree=round(float((ia == ib).float().mean()), 4))
        rep["iterations"].append(it)
        print("30b-width mxfp4 forward:", json.dumps(it))
        assert ok.all(), it
        assert e_hip.max() <= 1.5 * e_aten.max() + 1e-3 and e_hip.mean() <= 1.5 * e_aten.mean() + 1e-4, it
