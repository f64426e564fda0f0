"""GPU: the fused glue kernels F1 / F1p / F1r / F2 / F3 (csrc/sjd_glue.hip) held per element to the fp64 models of tests/glue_models.py, at the
shapes where the kernels branch (load schedules by plane count, stripes, slices of row_sumsq, the grid-stride pass, one head or four per wave).

  class A  torch.equal on the raw bits: everything that is only IEEE add, multiply or rounding -- h after the pre-norm forms, V rows, the table
           rotary, pad columns, and every cache row the launch must leave alone (all buffers hold a sentinel before the launch);
  class B  |kernel - model| <= the model's derived per-element tolerance (glue_models: one dtype ulp per documented rounding point, propagated), and
           at most 1 % of a tensor's elements may differ from the model at all -- the condition a wrong rounding mode fails.
Every case prints the share of differing elements and the worst error / bound.  tests/test_glue_models.py shows on the CPU that an fp32 emulation
passes these checks on the same inputs and that each planted defect fails them."""
import ctypes

import pytest
import torch

from tests import glue_models as M
from tests.fp8_model import e4m3_value

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
EPS = 1e-5
F32_SENTINEL = 12345.5
BYTE_SENTINEL = 0x5B


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    import sjd_amd._lib as L
    return L, L.load()


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(dtype):
    return 0 if dtype == torch.bfloat16 else 1


def _sentinel(shape, dtype, dev):
    return torch.full(shape, M.SENTINEL_BITS, dtype=torch.int16, device=dev).view(dtype)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _is_sentinel(t):
    return bool((_bits(t) == M.SENTINEL_BITS).all())


def _class_a(got, model, dtype, what):
    assert torch.equal(_bits(got.cpu()), _bits(model.to(dtype))), f"{what}: not the model's bits"


def _class_b(got, model, tol, what, count=None):
    share, worst = M.class_b(got.cpu(), model, tol, count)
    print(f"\n  {what}: {100 * share:.4f} % of the elements differ, worst error / bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: an element is {worst:.3f} x its derived bound away from the model"
    assert share <= M.SHARE_CAP, f"{what}: {100 * share:.3f} % of the elements differ from the model"


def _row_norm(L, rn, dev):
    """(sumsq, hidden, eps) on the CPU -> (ctypes pointer, the device tensor it points at)"""
    if rn is None:
        return None, None
    ss = rn[0].to(dev)
    s = L.RowNorm()
    s.sumsq, s.slices, s.hidden, s.eps = ss.data_ptr(), ss.shape[0], int(rn[1]), float(rn[2])
    return ctypes.pointer(s), ss


# ------------------------------------------------------------------------------------------------ F1 / F1p
def _f1_launch(dev, dtype, inp, post, y=True):
    L, lib = _lib()
    rows, hidden = inp["h"].shape
    h, w = inp["h"].to(dev), inp["w"].to(dev)
    d = inp["delta"].to(dev) if inp["delta"] is not None else None
    pl = inp["planes"].to(dev) if inp["planes"] is not None else None
    yb = _sentinel((rows, hidden), dtype, dev) if y else None
    rc = lib.sjd_add_rmsnorm(_p(h), _p(d), _p(w), _p(yb), rows, hidden, EPS, _code(dtype) | (L.F1_POST_NORM if post else 0), _p(pl),
                             0 if pl is None else pl.shape[0], _st())
    torch.cuda.synchronize()
    return rc, h, yb


def _f1_check(dev, dtype, inp, post, what):
    rc, h, y = _f1_launch(dev, dtype, inp, post)
    assert rc == 0
    m = M.f1_model(inp["h"], inp["w"], EPS, dtype, delta=inp["delta"], planes=inp["planes"], post=post)
    count = inp["plain"][:, None].expand(inp["h"].shape)
    if post:
        _class_b(h, m["h"], m["h_tol"], what + " h", count)
        assert _is_sentinel(y), "the POST form does not write y"
    else:
        _class_a(h, m["h"], dtype, what + " h")
        _class_b(y, m["y"], m["y_tol"], what + " y", count)


@pytest.mark.parametrize("rows,hidden,src", M.F1_DENSE_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f1_dense(dev, dtype, rows, hidden, src):
    """F1 on a dense delta and without one: one vector per thread, the second stripe's first vector (2056), the 8192 cap"""
    _f1_check(dev, dtype, M.f1_inputs(dtype, rows, hidden, dense=src == "dense"), False, f"F1 {rows}x{hidden} {src}")


@pytest.mark.parametrize("rows,hidden", M.F1_POST_DENSE_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f1_post_dense(dev, dtype, rows, hidden):
    _f1_check(dev, dtype, M.f1_inputs(dtype, rows, hidden, dense=True), True, f"F1 POST {rows}x{hidden}")


@pytest.mark.parametrize("rows,hidden,n_chunks", M.F1P_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f1p_planes(dev, dtype, rows, hidden, n_chunks):
    """F1p: planes in batches of sixteen (16 | 17), stripes of 4096 columns (4096 | 4104), 33 rows in planes padded to 64 whose pad rows hold a sentinel"""
    _f1_check(dev, dtype, M.f1_inputs(dtype, rows, hidden, n_chunks=n_chunks), False, f"F1p {rows}x{hidden} {n_chunks} planes")


@pytest.mark.parametrize("rows,hidden,n_chunks", M.F1P_POST_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f1p_post_planes(dev, dtype, rows, hidden, n_chunks):
    _f1_check(dev, dtype, M.f1_inputs(dtype, rows, hidden, n_chunks=n_chunks), True, f"F1p POST {rows}x{hidden} {n_chunks} planes")


# ------------------------------------------------------------------------------------------------ F1r
def _f1r_launch(dev, dtype, h, planes, rows, hidden):
    _, lib = _lib()
    slices = (hidden + 511) // 512
    out = torch.full((slices, M.prows(rows)), F32_SENTINEL, dtype=torch.float32, device=dev)
    rc = lib.sjd_residual_sumsq(_p(h), _p(planes), 0 if planes is None else planes.shape[0], rows, hidden, _code(dtype), _p(out), _st())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("rows,hidden,n_chunks", M.F1R_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f1r(dev, dtype, rows, hidden, n_chunks):
    """F1r: the three load schedules (<= 8, 9..16, > 16 planes), a last slice of four columns (516), part = None (n_chunks 0)"""
    inp = M.f1_inputs(dtype, rows, hidden, n_chunks=n_chunks)
    h = inp["h"].to(dev)
    rc, out = _f1r_launch(dev, dtype, h, inp["planes"].to(dev) if n_chunks else None, rows, hidden)
    assert rc == 0
    m = M.f1r_model(inp["h"], dtype, planes=inp["planes"])
    _class_a(h, m["h"], dtype, "F1r h")
    out = out.cpu()
    err = (out[:, :rows].double() - m["sumsq"]).abs()
    worst = float((err / m["sumsq_tol"].clamp(min=1e-300)).max())
    print(f"\n  F1r {rows}x{hidden} {n_chunks} planes: worst sumsq error / (hidden 2^-24 bound) {worst:.4f}")
    assert (err <= m["sumsq_tol"]).all()
    assert (out[:, rows:] == F32_SENTINEL).all(), "a pad row of sumsq was written"


# ------------------------------------------------------------------------------------------------ F3
def _f3_launch(dev, dtype, inp, rows, inter):
    L, lib = _lib()
    gu = inp["gu"].to(dev) if inp["gu"] is not None else None
    pl = inp["planes"].to(dev) if inp["planes"] is not None else None
    rn, keep = _row_norm(L, inp["row_norm"], dev)
    y = _sentinel((rows, inter), dtype, dev)
    rc = lib.sjd_silu_mul_ex(_p(gu), _p(y), rows, inter, _code(dtype), _p(pl), 0 if pl is None else pl.shape[0], rn, _st())
    torch.cuda.synchronize()
    return rc, y


@pytest.mark.parametrize("rows,inter", M.F3_DENSE_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f3_dense(dev, dtype, rows, inter):
    """F3 on a dense gate|up: one vector, a ragged row, and the first shape whose vectors exceed one grid pass (256 x 16392); gate extremes in row 0"""
    inp = M.f3_inputs(dtype, rows, inter)
    rc, y = _f3_launch(dev, dtype, inp, rows, inter)
    assert rc == 0
    m = M.f3_model(dtype, gu=inp["gu"])
    _class_b(y, m["y"], m["y_tol"], f"F3 {rows}x{inter}", m["g"].abs() <= 8)


@pytest.mark.parametrize("rows,inter,n_chunks,slices", M.F3_PLANE_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f3_planes(dev, dtype, rows, inter, n_chunks, slices):
    """F3 on split-K planes (batches of four: 1 | 4 | 5), with and without the folded row norm (slices in batches of eight: 1 | 8 | 9)"""
    inp = M.f3_inputs(dtype, rows, inter, n_chunks, slices)
    rc, y = _f3_launch(dev, dtype, inp, rows, inter)
    assert rc == 0
    m = M.f3_model(dtype, planes=inp["planes"], rows=rows, row_norm=inp["row_norm"])
    _class_b(y, m["y"], m["y_tol"], f"F3 {rows}x{inter} {n_chunks} planes {slices} slices", m["g"].abs() <= 8)


# ------------------------------------------------------------------------------------------------ F2
def _f2_launch(dev, dtype, inp, B, n, H, Hkv, D, S, kv_lens, blobs, fp8=False, shards=1, table=None, head_pad=None):
    """-> (rc, q, k_cache, v_cache) on the CPU; every output holds its sentinel before the launch.  kv_lens: one per batch row; blobs: through an
    array of parameter blobs (one per batch row) in place of the host argument (which then needs one value for all rows)."""
    import sjd_amd.ops as ops
    L, lib = _lib()
    DS = head_pad or D
    T = B * n
    qkv = inp["qkv"].to(dev) if inp["qkv"] is not None else None
    pl = inp["planes"].to(dev) if inp["planes"] is not None else None
    rn, keep = _row_norm(L, inp.get("row_norm"), dev)
    norms = [t.to(dev).contiguous() for pair in (inp.get("qn"), inp.get("kn")) if pair is not None for t in pair] or [None] * 4
    q = _sentinel((B, n, H, DS), dtype, dev)
    if fp8:
        kc, vc = (torch.full((B, Hkv, S, DS), BYTE_SENTINEL, dtype=torch.uint8, device=dev) for _ in range(2))
    else:
        kc, vc = _sentinel((B, Hkv, S, DS), dtype, dev), _sentinel((B, Hkv, S, DS), dtype, dev)
    mode = _code(dtype) | (shards << L.QKN_SHARDS_SHIFT if shards > 1 else 0)
    freq = inp["inv_freq"].to(dev) if table is None else table.to(dev)
    if table is not None:
        mode |= L.F2_ROPE_TABLE | (L.F2_HEAD_PAD128 if head_pad else 0)
    params = None
    if blobs:
        params = ops.BlobArray(L.IterParams, B, dev)
        for b in range(B):
            v = params.blobs[b].view
            v.n_rows, v.kv_len, v.batch_rows = n, kv_lens[b], 1
        params.upload()
    else:
        assert len(set(kv_lens)) == 1
    pos = inp["positions"].reshape(-1).contiguous().to(dev)
    rc = lib.sjd_qknorm_rope_append_ex(_p(qkv), _p(q), _p(kc), _p(vc), *[_p(t) for t in norms], _p(freq), _p(pos), B, n, H, Hkv, D, S, mode, int(fp8),
                                       M.F2_KV_SCALE[0], M.F2_KV_SCALE[1], rn, params.blobs[0].ptr if params is not None else None,
                                       0 if blobs else kv_lens[0], _p(pl), 0 if pl is None else pl.shape[0], _st())
    torch.cuda.synchronize()
    return rc, q.cpu(), kc.cpu(), vc.cpu()


def _cache_split(cache, B, n, kv_lens, S):
    """cache [B, Hkv, S, D] -> (the written rows [T', Hkv, D], their token indices, the rows the launch must leave alone [., Hkv, D])"""
    rows = M.cache_rows(B, n, kv_lens, S)
    bi, ri = torch.tensor([r[0] for r in rows]), torch.tensor([r[2] for r in rows])
    tok = torch.tensor([r[0] * n + r[1] for r in rows])
    by_row = cache.permute(0, 2, 1, 3)                          # [B, S, Hkv, D]
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[bi, ri] = True
    return by_row[bi, ri], tok, by_row[~mask]


def _f2_check(dev, dtype, D, H, Hkv, B, n, S, kv_lens, blobs, inp, fp8, shards, what):
    rc, q, kc, vc = _f2_launch(dev, dtype, inp, B, n, H, Hkv, D, S, kv_lens, blobs, fp8, shards)
    assert rc == 0
    m = M.f2_model(dtype, inp["positions"], inp["inv_freq"], H, Hkv, D, qkv=inp["qkv"], planes=inp["planes"], row_norm=inp["row_norm"], qn=inp["qn"],
                   kn=inp["kn"], qk_shards=shards, kv_scale=M.F2_KV_SCALE if fp8 else None)
    _class_b(q.view(B * n, H, D), m["q"], m["q_tol"], what + " q")
    for name, cache in (("k", kc), ("v", vc)):
        got, tok, rest = _cache_split(cache, B, n, kv_lens, S)
        if fp8:
            assert (rest == BYTE_SENTINEL).all(), f"{what}: a {name} cache row outside the window was written"
            _class_b(e4m3_value(got.contiguous()), m[name + "8"][tok], m[name + "8_tol"][tok], f"{what} {name} (e4m3, decoded)")
            continue
        assert _is_sentinel(rest), f"{what}: a {name} cache row outside the window was written"
        if name == "v" and inp["row_norm"] is None:
            _class_a(got, m["v"][tok], dtype, what + " v")
        else:
            _class_b(got, m[name][tok], m[name + "_tol"][tok], f"{what} {name}")


@pytest.mark.parametrize("H,Hkv,n_chunks,slices,qk_norm,shards,blobs,fp8", M.F2_CASES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f2_one_head(dev, dtype, D, H, Hkv, n_chunks, slices, qk_norm, shards, blobs, fp8):
    """the one-head kernel: its three plane schedules (<= 2, <= 4, batches of eight), row_sumsq in batches of eight, QK-norm (sharded too), positions 0
    and >= 8192, a kv_len per batch row from parameter blobs with the last window rows of one batch row beyond S_max, an fp8 cache at scales 0.037 / 0.051"""
    inp = M.f2_inputs(dtype, D, H, Hkv, M.F2_B * M.F2_N, n_chunks, slices, qk_norm, shards, M.F2_POS)
    kv_lens = list(M.F2_KV_BLOBS) if blobs else [M.F2_KV_HOST] * M.F2_B
    _f2_check(dev, dtype, D, H, Hkv, M.F2_B, M.F2_N, M.F2_S, kv_lens, blobs, inp, fp8, shards,
              f"F2 D={D} heads=({H},{Hkv}) {n_chunks} planes {slices} slices norm={qk_norm}/{shards}")


@pytest.mark.parametrize("n_chunks,slices,qk_norm,shards,fp8", M.F2_ROWS_CASES)
def test_f2_many_rows(dev, n_chunks, slices, qk_norm, shards, fp8):
    """the many-row kernel (65 rows of planes, four heads per wave, bf16 D = 128) against the same model as the one-head kernel"""
    dtype, D, H = torch.bfloat16, 128, 4
    B, n, S = M.F2_ROWS_B, M.F2_ROWS_N, M.F2_ROWS_S
    inp = M.f2_inputs(dtype, D, H, H, B * n, n_chunks, slices, qk_norm, shards, M.f2_rows_positions())
    _f2_check(dev, dtype, D, H, H, B, n, S, [M.F2_ROWS_KV] * B, False, inp, fp8, shards, f"F2 rows {n_chunks} planes {slices} slices norm={qk_norm}/{shards}")


@pytest.mark.parametrize("D,pad,B,n,H,Hkv,src,S,kv", M.F2_TABLE_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_f2_table(dev, dtype, D, pad, B, n, H, Hkv, src, S, kv):
    """the table rotary is four fp32 operations and one rounding: q, k, v, the pad columns and the untouched cache rows bit for bit (a product
    contracted into an FMA shows on tokens 3 and 4, see glue_models.f2_table_inputs); positions clamp at both ends, a zero table row"""
    inp = M.f2_table_inputs(dtype, D, H, Hkv, B, n, src, S)
    rc, q, kc, vc = _f2_launch(dev, dtype, inp, B, n, H, Hkv, D, S, [kv] * B, False, table=inp["table"], head_pad=pad)
    assert rc == 0
    m = M.f2_table_model(dtype, inp["positions"], inp["table"], S, H, Hkv, D, qkv=inp["qkv"], planes=inp["planes"], head_pad=pad)
    _class_a(q.view(B * n, H, -1), m["q"], dtype, "table q")
    for name, cache in (("k", kc), ("v", vc)):
        got, tok, rest = _cache_split(cache, B, n, [kv] * B, S)
        assert _is_sentinel(rest), f"a {name} cache row outside the window was written"
        _class_a(got, m[name][tok], dtype, "table " + name)
    if pad:
        assert not _bits(q[..., D:]).any(), "pad columns of q"


# ------------------------------------------------------------------------------------------------ launcher refusals
def test_refusals_leave_the_outputs_alone(dev):
    """SJD_ERR_BAD_ARG (-1) before any launch, and the outputs keep their sentinel"""
    L, lib = _lib()
    dt = torch.bfloat16
    for hidden in (8200, 12):                                               # beyond the 256-thread kernel's 8192 columns; not whole 8-element vectors
        inp = M.f1_inputs(dt, 2, hidden, dense=True)
        rc, h, y = _f1_launch(dev, dt, inp, False)
        assert rc == -1 and _is_sentinel(y) and torch.equal(_bits(h.cpu()), _bits(inp["h"]))
    inp = M.f1_inputs(dt, 2, 64)                                            # the POST form normalises a sublayer output: there must be one
    rc, h, y = _f1_launch(dev, dt, inp, True, y=False)
    assert rc == -1 and torch.equal(_bits(h.cpu()), _bits(inp["h"]))
    for rows, hidden in ((2, 6), (257, 8)):                                 # F1r: whole 4-element vectors, at most 256 rows
        h = _sentinel((rows, hidden), dt, dev)
        rc, out = _f1r_launch(dev, dt, h, None, rows, hidden)
        assert rc == -1 and _is_sentinel(h) and (out == F32_SENTINEL).all()
    gu = torch.zeros(2, 24, dtype=dt)                                       # F3: inter = 12 is not whole 8-element vectors
    rc, y = _f3_launch(dev, dt, dict(gu=gu, planes=None, row_norm=None), 2, 12)
    assert rc == -1 and _is_sentinel(y)
    inp = M.f2_inputs(dt, 64, 3, 1, M.F2_B * M.F2_N, 0, 0, False, 1, M.F2_POS)      # F2: a row norm needs the planes it scales
    inp["row_norm"] = (torch.ones(1, 32), 512, EPS)
    rc, q, kc, vc = _f2_launch(dev, dt, inp, M.F2_B, M.F2_N, 3, 1, 64, M.F2_S, [M.F2_KV_HOST] * M.F2_B, False)
    assert rc == -1 and _is_sentinel(q) and _is_sentinel(kc) and _is_sentinel(vc)
