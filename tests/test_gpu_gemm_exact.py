"""GPU: the window GEMMs held, split-K plane by split-K plane, to EXACT fp64 sums (tests/gemm_exact_cases.py: operands on which fp32 addition is
exact and associative, so every correct kernel writes the bits of the fp64 sum of its own chunk -- zero tolerance, in rows and columns 2^-40 of
their neighbours as much as in the largest).  The quantised streams meet x @ w.T of the ORIGINAL weight (it packs without loss), never G1 and
never dequant().  Every launch writes into a buffer with guard zones through the C entry points and is run twice into differently poisoned
buffers.  Only test_wide_range_bound is not exact: Gaussian operands against the accumulation term of bound A1 (tests/test_gpu_prefill_quant.py).

Which kernel a (stream, rows, column tiles, chunk) reaches is restated in _routes() from csrc/sjd_gemm.hip's dispatch and launch_shapes' limits."""
import ctypes

import pytest
import torch

import sjd_amd.launch_shapes as LS
from tests import gemm_exact_cases as C
from tests import glue_models as GM

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
UNSUPPORTED = -2
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _stream_ptr():
    return vp(torch.cuda.current_stream().cuda_stream)


def _pack(stream, w, KC, sm, gateup=False):
    import sjd_amd.ops as ops
    if stream in ("bf16", "fp16"):
        return ops.pack_weight(w, KC, sm)
    if stream.startswith("z_"):
        pz = ops.pack_weight_z(w, KC, sm, gateup=gateup)
        assert pz is not None
        return pz
    return dict(q8=ops.pack_weight_q8, q4=ops.pack_weight_q4, q6=ops.pack_weight_q6)[stream](w, KC, sm, gateup=gateup)


def _flag(wp):
    import sjd_amd._lib as L
    import sjd_amd.ops as ops
    return L.G1_W8_E4M3 if isinstance(wp, ops.PackedQ8) else L.G1_W4_MXFP4 if isinstance(wp, ops.PackedQ4) else L.G1_W6_E2M3 if isinstance(wp, ops.PackedQ6) else 0


def _g1_call(x, wp, out_ptr, M, n_cols, K, KC, waves, sm, N_packed, col0=0):
    """the C entry point behind ops.skinny_gemm / skinny_gemm_cols for this packing, writing its planes at out_ptr -> the return code"""
    import sjd_amd._lib as L
    import sjd_amd.ops as ops
    lib = L.load()
    if isinstance(wp, ops.PackedZ):
        return lib.sjd_skinny_gemm_z(vp(x.data_ptr()), vp(wp.data.data_ptr()), vp(wp.exc.data_ptr()), wp.cap, vp(out_ptr), M, n_cols, K, KC, waves, int(sm),
                                     L.DTYPE_BF16, N_packed, col0 // 32, ops._raw_units(wp), _stream_ptr())
    data = wp if isinstance(wp, torch.Tensor) else wp.data
    code = (L.DTYPE_F16 if x.dtype == torch.float16 else L.DTYPE_BF16) | _flag(wp)
    if col0 == 0 and n_cols == N_packed:
        return lib.sjd_skinny_gemm(vp(x.data_ptr()), vp(data.data_ptr()), vp(out_ptr), M, n_cols, K, KC, waves, int(sm), code, _stream_ptr())
    return lib.sjd_skinny_gemm_cols(vp(x.data_ptr()), vp(data.data_ptr()), vp(out_ptr), M, n_cols, K, KC, waves, int(sm), code, N_packed, col0 // 32, _stream_ptr())


def _guarded_g1(dev, x, wp, n_cols, K, KC, waves, sm, N_packed, col0=0, poison=GM.PLANE_SENTINEL, what=""):
    """one launch into a guarded buffer: assertion (b) -- guards untouched, pad rows zero, every element of rows < M written, all finite -> the planes"""
    M = x.shape[0]
    g = C.guarded_planes((K + KC - 1) // KC, GM.prows(M), n_cols, dev, poison)
    rc = _g1_call(x, wp, g.ptr(), M, n_cols, K, KC, waves, sm, N_packed, col0)
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: the library returned {rc}"
    bad = g.problems(M)
    assert not bad, f"{what}: " + "; ".join(bad)
    return g.planes


def _routes(stream, M, K, KC):
    """[(column tiles per workgroup, kernel)] worth running at M rows: every branch csrc/sjd_gemm.hip takes for this stream at this row band and chunk, with
    tile counts that leave waves without a column tile at N = 64 / 96 (two / three tiles).  () where the stream has no kernel for the shape."""
    MT, kc = (M + 31) // 32, min(KC, K)
    whole = kc <= (LS.CHUNK_CAP_32ROW if MT == 1 else LS.CHUNK_CAP_64ROW)          # the activation chunk is staged whole in LDS
    if stream in ("bf16", "fp16"):
        if MT == 1:
            return [(2, "G1<1 row tile>"), (5, "G1<1 row tile>"), (11, "G1<1 row tile, 1024 threads>")]
        if MT == 2:
            r = [(t, "G1w<2 row tiles>") for t in LS.WIDE_TILES] + [(5, "G1<2 row tiles>" if whole else "G1 sub-tiled<2>")]
            return r + ([(11, "G1<2 row tiles, 1024 threads>")] if whole else [])
        if MT <= 4:
            if stream == "bf16":
                return [(t, f"G1w<{MT} row tiles>") for t in LS.WIDE_TILES if (MT, t) != (3, 2)] + [(5, f"G1 sub-tiled<{MT}>")] + ([(2, "G1 sub-tiled<3>")] if MT == 3 else [])
            return [(t, f"G1 sub-tiled8<{MT}>" if t in (4, 8) else f"G1 sub-tiled<{MT}>") for t in (2, 3, 4, 5, 6, 8)]
        return [(t, f"G1w<{MT} row tiles>") for t in LS.WIDE_TILES]
    if stream.startswith("z_"):
        if M > LS.Z_MAX_ROWS:
            return []
        if MT == 1:
            return [(2, "G1z<1>"), (5, "G1z<1>"), (11, "G1z<1, 1024 threads>")]
        if MT == 2:
            return [(4, "G1w 12-bit<2 row tiles>"), (5, "G1z<2>" if whole else "G1z sub-tiled<2>")] + ([(11, "G1z<2, 1024 threads>")] if whole else [])
        return [(3, f"G1z sub-tiled<{MT}>"), (8, f"G1z sub-tiled<{MT}>")]
    name = dict(q8="G1q", q4="G1q4", q6="G1q6")[stream]
    if MT <= 2:
        return [(2, f"{name}<{MT}>"), (5, f"{name}<{MT}>"), (11, f"{name}<{MT}, 1024 threads>")] if whole else []
    if stream == "q6" or M > LS.WINDOW_MAX_ROWS:
        return []
    wide = dict(q8="G1wq", q4="G1wq4")[stream]
    return [(t, f"{wide}<{MT} row tiles>") for t in LS.WIDE_TILES if (MT, t) != (3, 2)]


def _rows_of(stream):
    limit = LS.Z_MAX_ROWS if stream.startswith("z_") else LS.Q6_MAX_ROWS if stream == "q6" else LS.WINDOW_MAX_ROWS
    return [M for M in C.ROWS if M <= limit]


REACHED = {}


def _note(stream, M, kernel):
    band = "<= 32" if M <= 32 else "33..64" if M <= 64 else "65..128" if M <= 128 else "129..256"
    REACHED.setdefault((stream, band), set()).add(kernel)


# ------------------------------------------------------------------------------------------------ the planes, exact
@pytest.mark.parametrize("stream,N,K,KC", [(s, *shape) for s in C.STREAMS for shape in C.stream_shapes(s)])
def test_planes_are_the_exact_chunk_sums(dev, stream, N, K, KC):
    """(a) every plane holds the bits of the fp64 sum of its own chunk; (b) guards, pad rows, nothing unwritten, nothing non-finite; (c) a second launch
    into a buffer poisoned with NaN in place of the sentinel gives the same bits.  Both packings, every row band, every dispatch branch of the band.
    The 12-bit stream: z_clean has no exceptions, z_outliers has them in its headers, z_raw consists of raw units (tests/test_gemm_exact_cases.py
    asserts all three on the CPU), so the exact weight does produce each of the stream's paths."""
    x_all, w, exact = C.g1_case(stream, N, K, KC)
    x_all, w, exact = x_all.to(dev), w.to(dev), exact.to(dev)
    launches = 0
    for sm in (False, True):
        wp = _pack(stream, w, KC, sm)
        for M in _rows_of(stream):
            x = x_all[:M].contiguous()
            for tiles, kernel in _routes(stream, M, K, KC):
                what = f"{stream} M={M} N={N} K={K} KC={KC} tiles={tiles} step_major={sm} [{kernel}]"
                p1 = _guarded_g1(dev, x, wp, N, K, KC, tiles, sm, N, what=what)
                msg = C.first_mismatch(p1, exact[:, :M], what)
                assert msg is None, msg
                p2 = _guarded_g1(dev, x, wp, N, K, KC, tiles, sm, N, poison=NAN, what=what + " (NaN-poisoned)")
                assert torch.equal(p1.view(torch.int32), p2.view(torch.int32)), f"{what}: the result depends on what the buffer held"
                _note(stream, M, kernel)
                launches += 1
    assert launches > 0
    print(f"\n  {stream} N={N} K={K} KC={KC}: {launches} routes x 2 launches exact; kernels per row band so far:")
    for (s, band), ks in sorted(REACHED.items()):
        if s == stream:
            print(f"    {band:>9} rows: {', '.join(sorted(ks))}")


@pytest.mark.parametrize("stream", ["q8", "q4", "q6"])
def test_packing_on_the_gpu_gives_the_bytes_of_packing_on_the_cpu(dev, stream):
    """the exact tests pack on the GPU, as the backbones do; tests/test_gemm_exact_cases.py proves the CPU packing lossless.  The two must be the same
    bytes, scales included: the e4m3 packer used to take its column scales from torch.ldexp, which on the GPU is one ulp below 2^e at e = 16..20, 22, ...
    -- the kernels read the scale's exponent field and multiplied those columns by half their scale (found by test_planes_are_the_exact_chunk_sums)."""
    for N, K, KC in C.QUANT_SHAPES:
        _, w, _ = C.g1_case(stream, N, K, KC)
        assert torch.equal(_pack(stream, w.to(dev), KC, True).data.cpu(), _pack(stream, w, KC, True).data), (stream, N, K, KC)


@pytest.mark.parametrize("stream", ["q8", "q4"])
def test_two_column_tiles_are_refused_at_65_to_96_rows(dev, stream):
    """kernels G1wq / G1wq4 have no form of three row tiles x two column tiles: the library says so before any launch, and writes nothing"""
    N, K, KC = C.QUANT_SHAPES[0]
    x_all, w, _ = C.g1_case(stream, N, K, KC)
    wp = _pack(stream, w.to(dev), KC, True)
    for M in (65, 96):
        g = C.guarded_planes(K // KC, GM.prows(M), N, dev)
        assert _g1_call(x_all[:M].contiguous().to(dev), wp, g.ptr(), M, N, K, KC, 2, True, N) == UNSUPPORTED
        torch.cuda.synchronize()
        assert g.untouched()


@pytest.mark.parametrize("stream", ["bf16", "q4"])
def test_column_window_is_the_exact_window(dev, stream):
    """skinny_gemm_cols over columns 32..63 of N = 96: columns 32..63 of the exact planes, through the same guarded buffer"""
    N, K, KC = C.COLS_SHAPE
    col0, n_cols = C.COLS_WINDOW
    x_all, w, exact = C.g1_case(stream, N, K, KC)
    x_all, w, exact = x_all.to(dev), w.to(dev), exact[:, :, col0:col0 + n_cols].contiguous().to(dev)
    for sm in (False, True):
        wp = _pack(stream, w, KC, sm)
        for M in (7, 64, 129):
            x = x_all[:M].contiguous()
            for tiles, kernel in _routes(stream, M, K, KC):
                what = f"{stream} columns {col0}..{col0 + n_cols - 1} M={M} tiles={tiles} step_major={sm} [{kernel}]"
                p1 = _guarded_g1(dev, x, wp, n_cols, K, KC, tiles, sm, N, col0, what=what)
                msg = C.first_mismatch(p1, exact[:, :M], what, col0)
                assert msg is None, msg
                p2 = _guarded_g1(dev, x, wp, n_cols, K, KC, tiles, sm, N, col0, poison=NAN, what=what)
                assert torch.equal(p1.view(torch.int32), p2.view(torch.int32)), what


# ------------------------------------------------------------------------------------------------ fused gate|up
GATEUP_CASES = ([(s, "small", M) for s in C.STREAMS for M in (1, 32)] + [(s, "tall64", 64) for s in ("bf16", "fp16", "z_clean", "z_outliers", "z_raw")]
                + [(s, "tall128", 128) for s in ("bf16", "fp16")] + [("q4", "k4", M) for M in (1, 32)])


def _gateup_call(x, wp, y_ptr, T, inter, hidden, sm, rn_ptr):
    """the C entry point behind ops.gateup_silu for this packing -> the return code"""
    import sjd_amd._lib as L
    import sjd_amd.ops as ops
    lib = L.load()
    if isinstance(wp, ops.PackedZ):
        return lib.sjd_gateup_silu_z(vp(x.data_ptr()), vp(wp.data.data_ptr()), vp(wp.exc.data_ptr()), wp.cap, vp(y_ptr), T, inter, hidden, int(sm), L.DTYPE_BF16,
                                     rn_ptr, ops._raw_units(wp, gateup=True), _stream_ptr())
    data = wp if isinstance(wp, torch.Tensor) else wp.data
    code = (L.DTYPE_F16 if x.dtype == torch.float16 else L.DTYPE_BF16) | _flag(wp)
    chunks = hidden // wp.KC if isinstance(wp, ops.PackedQ4) else 2
    arg = int(sm) | (0 if chunks == 2 else chunks << L.G1S_CHUNKS_SHIFT)
    return lib.sjd_gateup_silu(vp(x.data_ptr()), vp(data.data_ptr()), vp(y_ptr), T, inter, hidden, arg, code, rn_ptr, _stream_ptr())


def _sumsq(M, hidden, seed):
    """F1r's per-slice sums [slices <= 8, prows] for row scales r between 1/2 and 2 from row to row; pad rows hold the plane sentinel"""
    g = torch.Generator().manual_seed(seed)
    slices = min(8, hidden // 512)
    ss = torch.full((slices, GM.prows(M)), GM.PLANE_SENTINEL, dtype=torch.float32)
    ss[:, :M] = (torch.rand(slices, M, generator=g) + 0.5) * (hidden / slices) * torch.ldexp(torch.ones(M), torch.randint(-2, 3, (M,), generator=g))[None, :]
    return ss


@pytest.mark.parametrize("with_norm", [False, True])
@pytest.mark.parametrize("stream,name,M", GATEUP_CASES)
def test_gateup_silu_is_f3_on_the_exact_sums(dev, stream, name, M, with_norm):
    """the gate and up sums of the fused launch are exact, so its output is glue_models.f3_model fed with the exact planes, held to that model's own
    class B tolerance and SHARE_CAP (nothing new is tuned); 1 and 32 rows, the tall forms (64 rows at hidden 1024; 128 rows at hidden 4096, 16-bit
    only) and the four-chunk MXFP4 route at hidden 8192 (LS.gateup_silu_chunked_ok: kernel g1q4_gateup_silu_k4)."""
    import sjd_amd.ops as ops
    inter, hidden, chunks, _, _ = C.GATEUP_SHAPES[name]
    KC = hidden // chunks
    assert LS.gateup_silu_chunked_ok(M, inter, hidden, KC) if name == "k4" else LS.gateup_silu_ok(M, inter, hidden, KC, stream.startswith("z_"), stream in ("q8", "q4", "q6"))
    x, w, exact = C.gateup_case(stream, name, M)
    dtype = C.stream_dtype(stream)
    ss = _sumsq(M, hidden, 3 * M + hidden) if with_norm else None
    m = GM.f3_model(dtype, planes=exact.float(), rows=M, row_norm=(ss, hidden, 1e-5) if with_norm else None)
    xd, wd = x.to(dev), w.to(dev)
    ss_dev = ss.to(dev) if with_norm else None
    for sm in (False, True):
        wp = _pack(stream, wd, KC, sm, gateup=chunks == 2)
        front = 1024
        outs = []
        for poison in (GM.SENTINEL_BITS, 0x7FFF):          # a finite odd pattern, then NaN (both 16-bit types)
            buf = torch.full((2 * front + M * inter,), poison, dtype=torch.int16, device=dev)
            rc = _gateup_call(xd, wp, buf.data_ptr() + 2 * front, M, inter, hidden, sm, ops._row_norm((ss_dev, hidden, 1e-5)) if with_norm else None)
            torch.cuda.synchronize()
            what = f"gate|up {stream} {name} M={M} step_major={sm} norm={with_norm}"
            assert rc == 0, f"{what}: the library returned {rc}"
            assert bool((buf[:front] == poison).all()) and bool((buf[front + M * inter:] == poison).all()), f"{what}: written outside y"
            y = buf[front:front + M * inter].view(M, inter)
            assert not bool((y == poison).any()), f"{what}: an element of y was never written"
            outs.append(y.cpu())
        assert torch.equal(outs[0], outs[1]), f"{what}: the result depends on what the buffer held"
        share, worst = GM.class_b(outs[0].view(dtype), m["y"], m["y_tol"], m["g"].abs() <= 8)
        print(f"\n  {what}: {100 * share:.4f} % of the elements differ from the model, worst error / bound {worst:.3f}")
        assert worst <= 1.0 and share <= GM.SHARE_CAP, (what, share, worst)


# ------------------------------------------------------------------------------------------------ the reduce epilogue
@pytest.mark.parametrize("M", [5, 32])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_reduce_epilogue_is_f1r_on_the_exact_sums(dev, dtype, M):
    """G1 with F1r as its tail: h afterwards is glue_models.f1r_model's (class A: bit for bit) fed with the exact planes, the row sums of squares
    within that model's tolerance"""
    import sjd_amd.ops as ops
    N, K, KC, waves, sm = C.REDUCE_SHAPE
    assert ops.skinny_gemm_reduce_ok(M, N, K, KC, waves, dev)
    stream = "fp16" if dtype == torch.float16 else "bf16"
    x, w = C.operands(stream, M, N, K, KC, 41 + M, C.GATEUP_ROW_RNG, C.GATEUP_COL_RNG)
    h0 = torch.randn(M, N, generator=torch.Generator().manual_seed(M)).to(dtype)
    m = GM.f1r_model(h0, dtype, planes=C.exact_planes(x, w, KC).float())
    h = h0.clone().to(dev)
    ss = ops.skinny_gemm_reduce(x.to(dev), ops.pack_weight(w.to(dev), KC, sm), N, K, KC, h, waves=waves, step_major=sm)
    torch.cuda.synchronize()
    assert ops.reduce_timeouts() == 0
    assert torch.equal(h.cpu().view(torch.int16), m["h"].to(dtype).view(torch.int16)), "h is not dtype(h + dtype(exact sum))"
    err = (ss.cpu()[:, :M].double() - m["sumsq"]).abs()
    print(f"\n  reduce epilogue {stream} M={M}: worst sumsq error / bound {float((err / m['sumsq_tol'].clamp(min=1e-300)).max()):.4f}")
    assert bool((err <= m["sumsq_tol"]).all())


# ------------------------------------------------------------------------------------------------ G1p
@pytest.mark.parametrize("M", [1, LS.PREFILL_ROW_BLOCK + 1])
@pytest.mark.parametrize("N,K,KC", C.QUANT_SHAPES)
@pytest.mark.parametrize("form", ["bf16", "q8", "q4"], ids=["plain", "e4m3", "mxfp4"])
def test_prefill_gemm_is_the_exact_sum_rounded_once(dev, form, N, K, KC, M):
    """G1p: the fp32 sum over the whole of K is exact and ONE rounding follows, so y is the bf16 rounding of the exact sum, bit for bit -- also under
    a power-of-two row_scale, which multiplies the finished sum exactly"""
    import sjd_amd.ops as ops
    x_all, w, exact = C.g1_case(form, N, K, KC)
    x = x_all[:M].contiguous().to(dev)
    total = exact[:, :M].sum(0)
    rs = torch.ldexp(torch.ones(M), torch.randint(-6, 7, (M,), generator=torch.Generator().manual_seed(M)))
    for sm in (False, True):
        wp = _pack(form, w.to(dev), KC, sm)
        for scale in (None, rs):
            y = ops.prefill_gemm(x, wp, N, K, None if scale is None else scale.to(dev), KC=KC, step_major=sm)
            want = (total if scale is None else total * scale.double()[:, None]).to(torch.bfloat16)
            bad = (y.cpu().view(torch.int16) != want.view(torch.int16)).nonzero()
            assert bad.numel() == 0, f"G1p {form} M={M} N={N} K={K} KC={KC} step_major={sm} row_scale={scale is not None}: row {int(bad[0, 0])} column {int(bad[0, 1])}"


# ------------------------------------------------------------------------------------------------ the wide-range bound
BOUND_ROUTES = {          # stream -> [(rows, column tiles)]: one launch per kernel route at BOUND_SHAPE
    "bf16": [(7, 5), (64, 5), (64, 4), (100, 5), (100, 4), (256, 8)], "fp16": [(7, 5), (64, 5), (64, 4), (100, 5), (100, 4), (256, 8)],
    "z_outliers": [(7, 5), (64, 5), (64, 4), (100, 8)], "q8": [(7, 5), (64, 5), (100, 4), (256, 8)], "q4": [(7, 5), (64, 5), (100, 4), (256, 8)], "q6": [(7, 5), (64, 5)]}


@pytest.mark.parametrize("stream", list(BOUND_ROUTES))
def test_wide_range_bound(dev, stream):
    """the ONE check that is not exact, and the only one on weights off the grid (a quantised stream: dequant() of a Gaussian weight, as the other
    tests of those streams do): Gaussian operands with rows and columns scaled by powers of two; every element of every plane within
    (KC_c + 2) 2^-23 S_c, the accumulation term of bound A1.  Prints the worst error / bound per kernel route: a record, not a threshold."""
    N, K, KC = C.BOUND_SHAPE
    dtype = C.stream_dtype(stream)
    rr, cr = C.WIDE_EXP_RANGE[dtype]
    x_all, w = C.wide_range_operands(dtype, 256, N, K, 17, C.spread_exps(256, *rr, 18), C.spread_exps(N, *cr, 19))
    wp = _pack(stream, w.to(dev), KC, True)
    if stream in ("q8", "q4", "q6"):
        w = wp.dequant().cpu()
    for M, tiles in BOUND_ROUTES[stream]:
        kernel = dict(_routes(stream, M, K, KC))[tiles]
        exact, bound = C.plane_bounds(x_all[:M], w, KC)
        what = f"{stream} M={M} tiles={tiles} [{kernel}]"
        p = _guarded_g1(dev, x_all[:M].contiguous().to(dev), wp, N, K, KC, tiles, True, N, what=what)
        err = (p[:, :M].double().cpu() - exact).abs()
        ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        print(f"\n  wide-range bound {what}: worst error / bound = {float(ratio.max()):.4f}")
        assert bool((err <= bound).all()), (what, float(ratio.max()))


# ------------------------------------------------------------------------------------------------ NaN / Inf confinement
CONFINE = [("bf16", 7, 5, 176, 80), ("bf16", 100, 5, 176, 80), ("fp16", 100, 4, 176, 80), ("z_outliers", 7, 5, 176, 80), ("q8", 7, 5, 176, 80), ("q4", 7, 5, 384, 256)]


@pytest.mark.parametrize("stream,M,tiles,K,KC", CONFINE)
def test_poison_behind_a_chunk_end_stays_in_its_own_plane(dev, stream, M, tiles, K, KC):
    """test_g1_wide_chunk_neighbours_do_not_leak's pattern for the 32-row G1, the sub-tiled kernels (bf16 with five column tiles, fp16 with four),
    G1z, G1q and G1q4: NaN / Inf in the first k-step behind a ragged chunk end, and in the head of every row (what lies behind the LAST chunk's
    end), may change the poisoned chunk's plane only.  NaN is data here; the poison goes into x (quantised weights cannot hold one)."""
    N = 96
    g = torch.Generator().manual_seed(K + M)
    dtype = C.stream_dtype(stream)
    x = torch.randn(M, K, generator=g).to(dtype).to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).to(dev)
    kernel = dict(_routes(stream, M, K, KC))[tiles]
    wp = _pack(stream, w, KC, True)
    nc = (K + KC - 1) // KC

    def run(xx, what):          # (a poisoned run is expected to hold NaN: no guarded finiteness check, the buffer is still guarded)
        gp = C.guarded_planes(nc, GM.prows(M), N, dev)
        assert _g1_call(xx, wp, gp.ptr(), M, N, K, KC, tiles, True, N) == 0
        torch.cuda.synchronize()
        assert [b for b in gp.problems(M) if "non-finite" not in b] == [], what
        return gp.planes
    clean = run(x, "clean").clone()
    assert bool(torch.isfinite(clean).all())
    for value in (NAN, float("inf")):
        xa = x.clone()
        xa[:, KC:KC + 16] = value              # the first k-step of chunk 1: right behind chunk 0's end
        got = run(xa, f"{kernel} poison behind chunk 0")
        for c in range(nc):
            if c != 1:
                assert torch.equal(got[c], clean[c]), f"{kernel}: {value} behind chunk 0's end reached plane {c}"
        assert not bool(torch.isfinite(got[1][:M]).any()), f"{kernel}: the poisoned chunk's own plane is finite"
        xb = x.clone()
        xb[:, :48] = value                     # the head of every row: behind the last chunk's end lies the next row's first columns
        got = run(xb, f"{kernel} poison in the row heads")
        for c in range(1, nc):
            assert torch.equal(got[c], clean[c]), f"{kernel}: {value} in the row heads reached plane {c}"
