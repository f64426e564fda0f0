"""CPU: the fp64 glue models (tests/glue_models.py) themselves.  The GPU tests of tests/test_gpu_glue_bounds.py rest on them, so here
  * each model agrees with the project's own unfused 16-bit sequence (_CRMSNorm, _HeadLayerNorm, _rotate_half + the cos / sin cast, F.silu(g) * u,
    LlamaGen's table rotary) within its class B bound -- h, V and the pad columns bit for bit;
  * an fp32 emulation of every kernel (the same formula with fp32 intermediates) stays inside the bound and under the 1 % cap on every input set the
    GPU tests use -- a correct kernel can pass;
  * every planted defect (truncation, eps x 10, the last plane dropped, a neighbour row's sumsq, cos / sin left unrounded, the gain in front of the inner
    rounding, gate and up swapped, an FMA in the table rotary) is REJECTED on those inputs -- a subtly wrong kernel cannot."""
import pytest
import torch
import torch.nn.functional as F

from tests import glue_models as M

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
F32 = torch.float32


def _bits(t):
    return t.contiguous().view(torch.int16)


def test_ulp():
    for dt, mant, emin, emax in ((torch.bfloat16, 7, -126, 127), (torch.float16, 10, -14, 15)):
        fi = torch.finfo(dt)
        v = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 0.0, fi.tiny, fi.tiny / 4, fi.max, float("inf")], dtype=torch.float64)
        want = torch.tensor([2.0 ** (e - mant) for e in (0, 0, 1, -1, 1, emin, emin, emin, emax, emax)], dtype=torch.float64)
        assert torch.equal(M.ulp(dt, v), want), dt
        one = torch.tensor([1.0, 2.0, 0.0], dtype=dt)          # the spacing is what separates a value from its upper neighbour
        up = (one.view(torch.int16) + 1).view(dt)
        assert torch.equal((up.double() - one.double()), M.ulp(dt, one.double()))
    assert torch.equal(M.ulp_e4m3(torch.tensor([0.0, 2.0 ** -9, 1.0, 300.0, 448.0, 1e4])), torch.tensor([2.0 ** -9, 2.0 ** -9, 0.125, 32.0, 32.0, 32.0], dtype=torch.float64))


def test_planes_sum_is_sequential_fp32():
    p = torch.tensor([1.0, 2.0 ** -24, 2.0 ** -24, -1.0], dtype=F32).view(4, 1, 1)
    assert M.planes_sum(p).item() == 0.0                                  # ((1 + 2^-24) + 2^-24) - 1 in fp32: both small terms are lost
    assert M.planes_sum(p.flip(0)).item() == 2.0 ** -23                    # ((-1 + 2^-24) + 2^-24) + 1: the other order keeps them
    assert M.planes_sum(torch.tensor([-0.0], dtype=F32).view(1, 1, 1)).signbit().item() is False          # the sum starts from +0.0f


def test_trunc_plant_rounds_toward_zero():
    for dt in DTYPES:
        x = torch.tensor([1.0 + 2.0 ** -6 * 0.9, -(1.0 + 2.0 ** -6 * 0.9), 1.0, 3e-3, -0.0], dtype=torch.float64) * (2.0 ** -3 if dt == torch.float16 else 1)
        t = M._trunc(x, dt).double()
        assert (t.abs() <= x.abs()).all() and ((x.abs() - t.abs()) < M.ulp(dt, x)).all()


# ------------------------------------------------------------------------------------------------ the cases, evaluated by the model in some precision
def _count(plain, shape):
    return plain[:, None].expand(shape)


def _f1_runs(dtype, post, **kw):
    """-> [(case id, [(name, value, tol | None, count)])] over every F1 / F1p input set of the GPU file"""
    runs = []
    dense = [(r, hd, "dense") for r, hd in M.F1_POST_DENSE_CASES] if post else M.F1_DENSE_CASES
    for rows, hidden, src in dense:
        inp = M.f1_inputs(dtype, rows, hidden, dense=src == "dense")
        runs.append(((rows, hidden, src), inp, M.f1_model(inp["h"], inp["w"], 1e-5, dtype, delta=inp["delta"], post=post, **kw)))
    for rows, hidden, nc in (M.F1P_POST_CASES if post else M.F1P_CASES):
        inp = M.f1_inputs(dtype, rows, hidden, n_chunks=nc)
        runs.append(((rows, hidden, nc), inp, M.f1_model(inp["h"], inp["w"], 1e-5, dtype, planes=inp["planes"], post=post, **kw)))
    return runs


def _f1_verdict(ref, got, post, inp):
    """class B check of one F1 run against the fp64 model's run -> (ok, share, worst)"""
    key = "h" if post else "y"
    share, worst = M.class_b(got[key], ref[key], ref[key + "_tol"], _count(inp["plain"], ref[key].shape))
    ok = share <= M.SHARE_CAP and worst <= 1.0 and (post or torch.equal(got["h"].to(torch.float64), ref["h"]))
    return ok, share, worst


def _f3_runs(dtype, **kw):
    runs = []
    for rows, inter in M.F3_DENSE_CASES:
        inp = M.f3_inputs(dtype, rows, inter)
        runs.append(((rows, inter), inp, M.f3_model(dtype, gu=inp["gu"], **kw)))
    for rows, inter, nc, sl in M.F3_PLANE_CASES:
        inp = M.f3_inputs(dtype, rows, inter, nc, sl)
        runs.append(((rows, inter, nc, sl), inp, M.f3_model(dtype, planes=inp["planes"], rows=rows, row_norm=inp["row_norm"], **kw)))
    return runs


def _f3_verdict(ref, got):
    share, worst = M.class_b(got["y"], ref["y"], ref["y_tol"], ref["g"].abs() <= 8)
    return share <= M.SHARE_CAP and worst <= 1.0, share, worst


def _f2_runs(dtype, D, **kw):
    runs = []
    for H, Hkv, nc, sl, norm, shards, blobs, fp8 in M.F2_CASES:
        inp = M.f2_inputs(dtype, D, H, Hkv, M.F2_B * M.F2_N, nc, sl, norm, shards, M.F2_POS)
        runs.append(((H, Hkv, nc, sl, norm, shards, fp8), inp,
                     M.f2_model(dtype, inp["positions"], inp["inv_freq"], H, Hkv, D, qkv=inp["qkv"], planes=inp["planes"], row_norm=inp["row_norm"],
                                qn=inp["qn"], kn=inp["kn"], qk_shards=shards, kv_scale=M.F2_KV_SCALE if fp8 else None, **kw)))
    if D == 128 and dtype == torch.bfloat16:
        for nc, sl, norm, shards, fp8 in M.F2_ROWS_CASES:
            inp = M.f2_inputs(dtype, D, 4, 4, M.F2_ROWS_B * M.F2_ROWS_N, nc, sl, norm, shards, M.f2_rows_positions())
            runs.append((("rows", nc, sl, norm, shards, fp8), inp,
                         M.f2_model(dtype, inp["positions"], inp["inv_freq"], 4, 4, D, planes=inp["planes"], row_norm=inp["row_norm"], qn=inp["qn"],
                                    kn=inp["kn"], qk_shards=shards, kv_scale=M.F2_KV_SCALE if fp8 else None, **kw)))
    return runs


def _f2_verdict(ref, got):
    ok, share, worst = True, 0.0, 0.0
    for key in ("q", "k", "v") + (("k8", "v8") if "k8" in ref else ()):
        s, w = M.class_b(got[key], ref[key], ref[key + "_tol"])
        ok, share, worst = ok and s <= M.SHARE_CAP and w <= 1.0, max(share, s), max(worst, w)
    return ok, share, worst


# ------------------------------------------------------------------------------------------------ models against the project's 16-bit sequences
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f1_model_against_crmsnorm(dtype):
    from sjd_amd.backbones import _CRMSNorm
    for rows, hidden in ((7, 2056), (33, 512), (1, 8)):
        inp = M.f1_inputs(dtype, rows, hidden, n_chunks=3, dense=True)
        norm = _CRMSNorm(hidden, 1e-5).to(dtype)
        norm.weight.data = inp["w"]
        cnt = _count(inp["plain"], (rows, hidden))
        with torch.no_grad():
            for delta in (None, inp["delta"], M.planes_sum(inp["planes"])[:rows].to(dtype)):
                m = M.f1_model(inp["h"], inp["w"], 1e-5, dtype, delta=delta)
                href = inp["h"] if delta is None else inp["h"] + delta
                assert torch.equal(_bits(m["h"].to(dtype)), _bits(href))
                assert M.class_b_ok(norm(href), m["y"], m["y_tol"], cnt), M.class_b(norm(href), m["y"], m["y_tol"], cnt)
            m = M.f1_model(inp["h"], inp["w"], 1e-5, dtype, planes=inp["planes"])                      # the plane form = dense on dtype(plane sum)
            assert torch.equal(m["h"], M.f1_model(inp["h"], inp["w"], 1e-5, dtype, delta=delta)["h"])
            m = M.f1_model(inp["h"], inp["w"], 1e-5, dtype, delta=inp["delta"], post=True)           # swin order: h + norm(sublayer output)
            ref = inp["h"] + norm(inp["delta"])
            assert M.class_b_ok(ref, m["h"], m["h_tol"], cnt), M.class_b(ref, m["h"], m["h_tol"], cnt)
        assert torch.equal(m["h"][2], inp["h"][2].double()) if rows >= 4 else True                    # the all-zero sublayer row leaves h alone


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f1r_model(dtype):
    inp = M.f1_inputs(dtype, 33, 516, n_chunks=9)
    m = M.f1r_model(inp["h"], dtype, planes=inp["planes"])
    href = inp["h"] + M.planes_sum(inp["planes"])[:33].to(dtype)
    assert torch.equal(_bits(m["h"].to(dtype)), _bits(href))
    assert m["sumsq"].shape == (2, 33) and torch.allclose(m["sumsq"].sum(0), href.double().pow(2).sum(-1), rtol=1e-12)
    assert torch.equal(m["sumsq"][1], href[:, 512:].double().pow(2).sum(-1))
    assert torch.equal(M.f1r_model(inp["h"], dtype)["h"], inp["h"].double())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f3_model_against_silu_mul(dtype):
    for rows, inter in ((5, 1376), (1, 8)):
        inp = M.f3_inputs(dtype, rows, inter)
        m = M.f3_model(dtype, gu=inp["gu"])
        ref = F.silu(inp["gu"][:, :inter]) * inp["gu"][:, inter:]
        ok = M.class_b_ok(ref, m["y"], m["y_tol"], m["g"].abs() <= 8)
        assert ok, M.class_b(ref, m["y"], m["y_tol"], m["g"].abs() <= 8)
    inp = M.f3_inputs(dtype, 33, 136, 5, 0)                                 # planes without a row scale = dense on dtype(plane sum)
    a = M.f3_model(dtype, planes=inp["planes"], rows=33)
    b = M.f3_model(dtype, gu=M.planes_sum(inp["planes"])[:33].to(dtype))
    assert torch.equal(a["y"], b["y"]) and torch.equal(a["y_tol"], b["y_tol"])


@pytest.mark.parametrize("qk_norm,shards,H,Hkv", [(False, 1, 3, 1), (True, 1, 3, 1), (True, 2, 4, 2)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f2_model_against_unfused_sequence(dtype, D, qk_norm, shards, H, Hkv):
    from sjd_amd.backbones import _HeadLayerNorm, _rotate_half
    T = M.F2_B * M.F2_N
    inp = M.f2_inputs(dtype, D, H, Hkv, T, qk_norm=qk_norm, qk_shards=shards, positions=M.F2_POS)
    m = M.f2_model(dtype, inp["positions"], inp["inv_freq"], H, Hkv, D, qkv=inp["qkv"], qn=inp["qn"], kn=inp["kn"], qk_shards=shards)
    x = inp["qkv"].view(T, H + 2 * Hkv, D)
    qr, kr, vr = x[:, :H], x[:, H:H + Hkv], x[:, H + Hkv:]
    with torch.no_grad():
        if qk_norm:
            qn, kn = _HeadLayerNorm(D, H, shards).to(dtype), _HeadLayerNorm(D, Hkv, shards).to(dtype)
            qn.weight.data, qn.bias.data, kn.weight.data, kn.bias.data = inp["qn"][0], inp["qn"][1], inp["kn"][0], inp["kn"][1]
            qr, kr = qn(qr), kn(kr)
        freqs = inp["positions"].reshape(-1)[:, None].float() * inp["inv_freq"][None, :]          # the cos / sin cast of backbones.py
        emb = torch.cat((freqs, freqs), dim=-1)
        cos, sin = emb.cos().to(dtype)[:, None, :], emb.sin().to(dtype)[:, None, :]
        qr = qr * cos + _rotate_half(qr) * sin
        kr = kr * cos + _rotate_half(kr) * sin
    assert torch.equal(_bits(m["v"].to(dtype)), _bits(vr)) and not m["v_tol"].any()
    for got, key in ((qr, "q"), (kr, "k")):
        assert M.class_b_ok(got, m[key], m[key + "_tol"]), (key, M.class_b(got, m[key], m[key + "_tol"]))


@pytest.mark.parametrize("D,pad", [(64, None), (128, None), (100, 128)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f2_table_model_against_llamagen_rotary(dtype, D, pad):
    from sjd_amd.backbones import _apply_rope_interleaved
    B, n, H, S = 1, 5, 2, 8
    for src in ("dense", 3):
        inp = M.f2_table_inputs(dtype, D, H, H, B, n, src, S)
        m = M.f2_table_model(dtype, inp["positions"], inp["table"], S, H, H, D, qkv=inp["qkv"], planes=inp["planes"], head_pad=pad)
        x = (inp["qkv"] if src == "dense" else M.planes_sum(inp["planes"])[:B * n].to(dtype)).view(B, n, 3 * H, D)
        fr = inp["table"][inp["positions"].clamp(0, S - 1)].view(B, n, D // 2, 2)
        for key, sl in (("q", slice(0, H)), ("k", slice(H, 2 * H))):
            ref = _apply_rope_interleaved(x[:, :, sl], fr).view(B * n, H, D)
            assert torch.equal(_bits(m[key][..., :D]), _bits(ref))
        assert torch.equal(_bits(m["v"][..., :D]), _bits(x[:, :, 2 * H:].reshape(B * n, H, D)))
        if pad:
            assert all(m[k].shape[-1] == 128 and not _bits(m[k][..., D:]).any() for k in "qkv")
        assert not m["q"][2].any() and m["q"][0].any()                       # the condition row of the table gives zeros
        for fma in (1, 2):                                                   # either product contracted into the sum must show in q
            f = M.f2_table_model(dtype, inp["positions"], inp["table"], S, H, H, D, qkv=inp["qkv"], planes=inp["planes"], head_pad=pad, fma=fma)
            assert not torch.equal(_bits(f["q"][3:5, 0]), _bits(m["q"][3:5, 0])), f"contraction {fma} does not show"


# ------------------------------------------------------------------------------------------------ fp32 emulation passes, planted defects fail
def _judge(ref_runs, got_runs, verdict):
    out = []
    for (cid, inp, ref), (_, _, got) in zip(ref_runs, got_runs):
        out.append((cid,) + tuple(verdict(ref, got, inp)))
    return out


def _f1v(post):
    return lambda ref, got, inp: _f1_verdict(ref, got, post, inp)


_F3V = lambda ref, got, inp: _f3_verdict(ref, got)
_F2V = lambda ref, got, inp: _f2_verdict(ref, got)


@pytest.fixture(scope="module")
def model_runs():
    """the fp64 model over every input set of the GPU file, evaluated once per (kernel, dtype)"""
    cache = {}

    def get(kind, dtype, D=None):
        key = (kind, dtype, D)
        if key not in cache:
            cache[key] = {"f1": lambda: _f1_runs(dtype, False), "f1post": lambda: _f1_runs(dtype, True), "f3": lambda: _f3_runs(dtype),
                          "f2": lambda: _f2_runs(dtype, D)}[kind]()
        return cache[key]
    return get


KINDS = {"f1": (lambda dt, D, **kw: _f1_runs(dt, False, **kw), _f1v(False), ("trunc", "eps10", "drop_plane", "gain_first")),
         "f1post": (lambda dt, D, **kw: _f1_runs(dt, True, **kw), _f1v(True), ("trunc", "eps10", "drop_plane", "gain_first")),
         "f3": (lambda dt, D, **kw: _f3_runs(dt, **kw), _F3V, ("trunc", "eps10", "drop_plane", "neighbour_sumsq", "swap_gate_up")),
         "f2": (lambda dt, D, **kw: _f2_runs(dt, D, **kw), _F2V, ("trunc", "eps10", "drop_plane", "neighbour_sumsq", "cs_unrounded", "gain_first"))}
KIND_PARAMS = [("f1", None), ("f1post", None), ("f3", None), ("f2", 64), ("f2", 128)]


@pytest.mark.parametrize("kind,D", KIND_PARAMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fp32_emulation_passes_and_plants_fail(model_runs, dtype, kind, D):
    runs, verdict, plants = KINDS[kind]
    ref = model_runs(kind, dtype, D)
    res = _judge(ref, runs(dtype, D, f=F32), verdict)
    print(f"\n{kind} {dtype} D={D}: fp32 emulation, worst share {max(r[2] for r in res):.5f}, worst error/bound {max(r[3] for r in res):.3f}")
    assert all(r[1] for r in res), [r for r in res if not r[1]]
    for plant in plants:
        res = _judge(ref, runs(dtype, D, f=F32, plant=plant), verdict)
        caught = [r[0] for r in res if not r[1]]
        print(f"  plant {plant}: rejected on {len(caught)} of {len(res)} input sets")
        assert caught, f"{plant} passes the class B check on every {kind} input set"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f1r_emulation_and_plants(dtype):
    for rows, hidden, nc in M.F1R_CASES:
        inp = M.f1_inputs(dtype, rows, hidden, n_chunks=nc)
        ref = M.f1r_model(inp["h"], dtype, planes=inp["planes"])
        emu = M.f1r_model(inp["h"], dtype, planes=inp["planes"], f=F32)
        ss32 = torch.stack([(emu["h"][:, s * 512:(s + 1) * 512] ** 2).sum(-1) for s in range(ref["sumsq"].shape[0])])        # an fp32 sum in some order
        assert torch.equal(emu["h"].double(), ref["h"]) and ((ss32.double() - ref["sumsq"]).abs() <= ref["sumsq_tol"]).all()
        if nc and rows > 1:
            for plant in ("drop_plane", "trunc"):
                bad = M.f1r_model(inp["h"], dtype, planes=inp["planes"], f=F32, plant=plant)
                assert not torch.equal(bad["h"].double(), ref["h"])
            bad = M.f1r_model(inp["h"], dtype, planes=inp["planes"], plant="drop_plane")
            assert not ((bad["sumsq"] - ref["sumsq"]).abs() <= ref["sumsq_tol"]).all() or nc == 0
