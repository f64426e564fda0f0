"""Operands, references and case tables that hold the window GEMMs (kernels G1, sub-tiled G1, G1w, G1z, G1q, G1wq, G1q4, G1wq4, G1q6, the fused
gate|up forms, G1p) to EXACT fp64 sums, split-K plane by split-K plane.

The construction: x holds small integers times a power of two per row, w holds e2m1 grid values {0, .5, 1, 1.5, 2, 3, 4, 6} times a power of two per
(column, 64-k record) and per column.  Every product x[m, k] w[n, k] is then a whole number of units u[m, n] = 2^-1 2^row_exp[m] 2^col_exp[n], and
so is every partial sum over any subset of k in any order; with K max|x| max|w| < 2^24 units none of them needs more than fp32's 24 significand
bits.  fp32 addition is therefore EXACT and associative on these operands: a correct kernel, whatever its MFMA shape, k order or split, writes the
bits of the fp64 sum of its own chunk -- zero tolerance, and a row or column that is 2^-40 of its neighbour is held as tightly as the largest.
The same w sits on the e2m1 grid under a power-of-two scale per 64-k record, so it packs WITHOUT LOSS into the e4m3, MXFP4, e2m3 and 12-bit
streams: each quantised kernel meets x @ w.T in fp64 directly, not another kernel and not dequant().

tests/test_gemm_exact_cases.py checks on the CPU that the operands hold these conditions (lossless packing, exactness in three accumulation
orders) and that the exact check rejects the planted defects below; tests/test_gpu_gemm_exact.py runs the kernels.  Nothing here touches the GPU
or libsjd_hip.so.
"""
import functools

import torch

from tests.glue_models import PLANE_SENTINEL, prows

F64 = torch.float64
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
X_MAX = 8                  # |x| <= 8 2^row_exp: integers
BE_MAX = 6                 # the record exponent `be` of w lies in 0..6: |w| <= 6 * 2^6 * 2^col_exp
K_MAX = 2730               # K * 8 * (6 * 2^6 / 0.5) < 2^24  <=>  K <= 2730 at the defaults
# (row exponents, column exponents) a dtype's own range holds.  fp16: 1 * 2^r >= 2^-14 (normal) and 8 * 2^r <= 65504 give r in [-14, 12]; 0.5 * 2^c >= 2^-14
# and 6 * 2^6 * 2^c <= 65504 give c in [-13, 7]; the ranges below lie inside.  bf16 has fp32's exponent range: [-20, 20] is the issue's choice.
EXP_RANGE = {torch.bfloat16: ((-20, 20), (-20, 20)), torch.float16: ((-12, 10), (-12, 6))}
# the same for wide_range_operands, whose Gaussian values are of order 1 (x) and K^-1/2 (w) and have tails on both sides: fp16 keeps [-8, 8] for rows and
# [-6, 6] for columns, where all but a few per cent of the values are normal fp16 numbers (the rest are set to zero) and six sigma stays finite
WIDE_EXP_RANGE = {torch.bfloat16: EXP_RANGE[torch.bfloat16], torch.float16: ((-8, 8), (-6, 6))}

# ------------------------------------------------------------------------------------------------ the case tables of the GPU file
# (N, K, KC): four even chunks; a ragged last chunk of one 128-granule with N no multiple of 64; a last chunk of three k-steps (16-bit and 12-bit
# streams only: K is no multiple of 32 / 128); one chunk above CHUNK_CAP_64ROW, which at 64 rows runs on the sub-tiled kernel
SHAPES = ((64, 512, 128), (96, 384, 256), (96, 176, 64), (64, 1408, 1408))
QUANT_SHAPES = tuple(s for s in SHAPES if s[1] % 128 == 0 and s[2] % 128 == 0)
ROWS = (1, 7, 32, 33, 64, 65, 128, 129, 256)
BOUND_SHAPE = (96, 384, 256)
COLS_SHAPE, COLS_WINDOW = (96, 384, 256), (32, 32)          # skinny_gemm_cols: col0, n_cols
# fused gate|up: (inter, hidden, chunks, x_max, be_max).  hidden 4096 / 8192 exceed K_MAX at the defaults, so the record exponent is narrowed until
# the precondition holds again (exact_operands asserts it): 4096 * 8 * 12 * 2^5 and 8192 * 8 * 12 * 2^4 are 3 * 2^22 < 2^24.
GATEUP_SHAPES = dict(small=(64, 512, 2, X_MAX, BE_MAX), tall64=(64, 1024, 2, X_MAX, BE_MAX), tall128=(64, 4096, 2, X_MAX, 5), k4=(64, 8192, 4, X_MAX, 4))
REDUCE_SHAPE = (512, 1024, 256, 4, True)                    # N, K, KC, waves, step_major: the smallest shape ops.skinny_gemm_reduce_ok takes
Z_KINDS = ("clean", "outliers", "raw")


def spread_exps(n, lo, hi, seed):
    """n integer exponents in [lo, hi]: the two extremes side by side in front, the rest uniform"""
    e = torch.randint(lo, hi + 1, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    if n >= 2:
        e[0], e[1] = lo, hi
    return e


def tile_exps(N, lo, hi, seed):
    """one exponent per 32-column tile: the 12-bit stream's exception window (sixteen binades per (chunk, tile) unit) holds such a weight whole"""
    return spread_exps((N + 31) // 32, lo, hi, seed).repeat_interleave(32)[:N]


# ------------------------------------------------------------------------------------------------ the operands
# the four (32-k block of the MXFP4 stream) x (lane half h of the e2m3 stream) cells of a 64-k record: k = 16 u + 8 h + j, block = k // 32
_CELLS = {(b, h): torch.tensor([32 * b + 16 * u + 8 * h + j for u in (0, 1) for j in range(8)]) for b in (0, 1) for h in (0, 1)}


def exact_operands(dtype, M, N, K, seed, row_exp, col_exp, *, x_max=X_MAX, be_max=BE_MAX, zero_share=0.125):
    """-> (x [M, K], w [N, K]) in `dtype` on the CPU.  x = integers in [-x_max, x_max] * 2^row_exp[m]; w = sign * E2M1 * 2^be * 2^col_exp[n] with be in
    0..be_max drawn once per (column, 64-k record).  Every record holds a 6 and a 0.5 in each of its MXFP4 blocks AND each of its e2m3 blocks (lane
    halves), so every stored block scale is forced to 2^(be + col_exp).  zero_share: how often w is 0 (the 12-bit stream stores a zero as an
    exception).  row_exp / col_exp: an int or one per row / column.  Asserts the precondition of exactness, that the cast to `dtype` changes nothing
    and that no value or product is subnormal."""
    g = torch.Generator().manual_seed(seed)
    re = torch.as_tensor(row_exp, dtype=torch.int32).reshape(-1).expand(M) if torch.as_tensor(row_exp).numel() == 1 else torch.as_tensor(row_exp, dtype=torch.int32)
    ce = torch.as_tensor(col_exp, dtype=torch.int32).reshape(-1).expand(N) if torch.as_tensor(col_exp).numel() == 1 else torch.as_tensor(col_exp, dtype=torch.int32)
    assert re.shape == (M,) and ce.shape == (N,)
    (rlo, rhi), (clo, chi) = EXP_RANGE[dtype]
    assert rlo <= int(re.min()) and int(re.max()) <= rhi and clo <= int(ce.min()) and int(ce.max()) <= chi, "exponents outside what the dtype holds"
    # THE PRECONDITION: in units of the smallest product (1 * 0.5) every partial sum stays below 2^24
    units = K * x_max * int(E2M1[-1] * 2 ** be_max / E2M1[1])
    assert units < 2 ** 24, f"K = {K}: a sum can reach {units} units of the smallest product, fp32 holds 2^24"
    xi = torch.randint(-x_max, x_max + 1, (M, K), generator=g)
    x = torch.ldexp(xi.to(F64), re[:, None])
    R = (K + 63) // 64
    idx = torch.randint(1, 8, (N, K), generator=g)
    idx[torch.rand(N, K, generator=g) < zero_share] = 0
    n_i, r_i = torch.meshgrid(torch.arange(N), torch.arange(R), indexing="ij")
    for (b, h), cell in _CELLS.items():          # a 6 where block and lane half agree, a 0.5 where they differ: every block of either kind holds both
        pick = torch.randint(0, 16, (N, R), generator=g)
        k = 64 * r_i + cell[pick]
        k = torch.where(k < K, k, 64 * r_i + cell[pick % 8])          # a partial last record: the cell's first eight positions
        ok = k < K
        idx[n_i[ok], k[ok]] = 7 if b == h else 1
    be = torch.randint(0, be_max + 1, (N, R), generator=g, dtype=torch.int32).repeat_interleave(64, dim=1)[:, :K]
    sign = torch.where(idx == 0, 1, torch.randint(0, 2, (N, K), generator=g) * 2 - 1)          # (no negative zeros: the comparisons below are on bits)
    w = torch.ldexp(sign.to(F64) * torch.tensor(E2M1, dtype=F64)[idx], be + ce[:, None])
    xt, wt = x.to(dtype), w.to(dtype)
    assert torch.equal(xt.to(F64), x) and torch.equal(wt.to(F64), w), "an operand does not survive the cast"
    tiny, tiny32 = float(torch.finfo(dtype).tiny), float(torch.finfo(torch.float32).tiny)
    ax, aw = x.abs(), w.abs()
    assert float(ax[ax > 0].min()) >= tiny and float(aw[aw > 0].min()) >= tiny, "a subnormal operand"
    assert float(ax[ax > 0].min()) * float(aw[aw > 0].min()) >= tiny32, "a subnormal product"
    assert units * 2.0 ** (int(re.max()) + int(ce.max()) - 1) < float(torch.finfo(torch.float32).max), "a sum can overflow fp32"
    return xt, wt


def chunks_of(K, KC):
    return [(k0, min(k0 + KC, K)) for k0 in range(0, K, KC)]


def exact_planes(x, w, KC):
    """fp64 [n_chunks, M, N]: plane c = the sum over k0 <= k < min(k0 + KC, K) only"""
    xd, wd = x.to(F64), w.to(F64)
    return torch.stack([xd[:, k0:k1] @ wd[:, k0:k1].t() for k0, k1 in chunks_of(x.shape[1], KC)])


def wide_range_operands(dtype, M, N, K, seed, row_exp, col_exp):
    """Gaussian x and w / sqrt(K) with rows and columns scaled by powers of two over WIDE_EXP_RANGE (bf16: exact_operands' range); values the dtype
    would hold as subnormals are zero (the reference is taken from the cast operands, so nothing is assumed about how a kernel treats them)"""
    g = torch.Generator().manual_seed(seed)
    re, ce = torch.as_tensor(row_exp, dtype=torch.int32), torch.as_tensor(col_exp, dtype=torch.int32)
    (rlo, rhi), (clo, chi) = WIDE_EXP_RANGE[dtype]
    assert rlo <= int(re.min()) and int(re.max()) <= rhi and clo <= int(ce.min()) and int(ce.max()) <= chi
    x = torch.ldexp(torch.randn(M, K, generator=g), re[:, None]).to(dtype)
    w = torch.ldexp(torch.randn(N, K, generator=g) / K ** 0.5, ce[:, None]).to(dtype)
    tiny = float(torch.finfo(dtype).tiny)
    x[x.abs() < tiny] = 0
    w[w.abs() < tiny] = 0
    return x, w


def plane_bounds(x, w, KC):
    """-> (fp64 planes, fp64 bounds), both [n_chunks, M, N]: bound = (KC_c + 2) 2^-23 S_c with S_c the chunk's sum of |x_k w_k| -- the accumulation
    term of bound A1 in tests/test_gpu_prefill_quant.py (products of two 16-bit values are exact in fp32; what is left is the fp32 accumulation
    over KC_c terms).  Derived there, not measured; not to be tuned."""
    xd, wd = x.to(F64), w.to(F64)
    ch = chunks_of(x.shape[1], KC)
    S = torch.stack([xd[:, k0:k1].abs() @ wd[:, k0:k1].abs().t() for k0, k1 in ch])
    kc = torch.tensor([k1 - k0 for k0, k1 in ch], dtype=F64)[:, None, None]
    return exact_planes(x, w, KC), (kc + 2) * 2.0 ** -23 * S


# ------------------------------------------------------------------------------------------------ fp32 emulations (the CPU test's subject)
ORDERS = ("forward", "reversed", "pairwise16")


def emulate_planes(x, w, KC, order="forward", acc=torch.float32):
    """[n_chunks, M, N] in `acc`: the chunk sums accumulated in `acc` arithmetic one product at a time (forward / reversed k order), or in 16-wide
    k-steps whose sixteen fp32 products are summed pairwise before they join the accumulator.  Products are formed in fp32 (exact for 16-bit operands)."""
    xf, wf = x.float(), w.float()
    out = []
    for k0, k1 in chunks_of(x.shape[1], KC):
        a = torch.zeros(x.shape[0], w.shape[0], dtype=acc)
        if order == "pairwise16":
            for s0 in range(k0, k1, 16):
                p = xf[:, None, s0:s0 + 16] * wf[None, :, s0:s0 + 16]
                while p.shape[-1] > 1:
                    p = p[..., 0::2] + p[..., 1::2]
                a = (a.float() + p[..., 0]).to(acc)
        else:
            for k in (range(k0, k1) if order == "forward" else range(k1 - 1, k0 - 1, -1)):
                a = (a.float() + xf[:, k, None] * wf[None, :, k]).to(acc)
        out.append(a)
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------ planted defects
# Each: (x, w, KC) -> fp32 planes [n_chunks, M, N] of an emulation that is wrong in ONE way a kernel of this family can be wrong.  All need >= 2 chunks,
# >= 2 k-steps in chunk 0 and N >= 64.
def _step(x, w, k0):
    return emulate_planes(x[:, k0:k0 + 16], w[:, k0:k0 + 16], 16)[0]


def _next_plane(x, w, KC):          # the last k-step of chunk 0 credited to plane 1: invisible in sum(0)
    p = emulate_planes(x, w, KC)
    s = _step(x, w, KC - 16)
    p[0], p[1] = p[0] - s, p[1] + s
    return p


def _drop_step(x, w, KC):           # k-step 1 of chunk 0 never multiplied
    p = emulate_planes(x, w, KC)
    p[0] = p[0] - _step(x, w, 16)
    return p


def _swap_planes(x, w, KC):
    p = emulate_planes(x, w, KC)
    return torch.cat([p[1:2], p[0:1], p[2:]])


def _swap_halves(x, w, KC):         # the lane halves h of record 0 (k = 16 s + 8 h + j) of column tile 0 trade places
    w2 = w.clone()
    w2[:32, 0:8], w2[:32, 8:16] = w[:32, 8:16], w[:32, 0:8]
    return emulate_planes(x, w2, KC)


def _scale_x2(x, w, KC):            # the scale of (column 5, 32-k block 1) read as twice what it is
    w2 = w.clone()
    w2[5, 32:64] = w2[5, 32:64] * 2
    return emulate_planes(x, w2, KC)


def _unwritten_plane(x, w, KC):     # the last plane keeps what the buffer held
    p = emulate_planes(x, w, KC)
    p[-1] = PLANE_SENTINEL
    return p


def _column_shift(x, w, KC):        # column 3 lands one tile to the right (column 3 itself still holds a stale right answer)
    p = emulate_planes(x, w, KC)
    p[:, :, 35] = p[:, :, 3]
    return p


DEFECTS = dict(next_plane=_next_plane, drop_step=_drop_step, swap_planes=_swap_planes, swap_halves=_swap_halves, scale_x2=_scale_x2,
               unwritten_plane=_unwritten_plane, column_shift=_column_shift)


def planted(name, x, w, KC, rows=None):
    """the defect `name` confined to `rows` (default: every row); the other rows are the correct emulation's"""
    bad = DEFECTS[name](x, w, KC)
    if rows is None:
        return bad
    out = emulate_planes(x, w, KC)
    out[:, rows] = bad[:, rows]
    return out


# ------------------------------------------------------------------------------------------------ the checks
def first_mismatch(got, exact, what, col0=0):
    """None when got[:, :M] (fp32 planes, pad rows allowed behind M) holds the bits of `exact` (fp64 [n_chunks, M, N]), else a sentence naming the
    first element that does not: chunk, row, column (col0: where a column window starts) and stream."""
    M = exact.shape[1]
    assert got.dtype == torch.float32 and got.shape[0] == exact.shape[0] and got.shape[2] == exact.shape[2] and got.shape[1] >= M
    g = got[:, :M].to(F64)
    bad = ~(g == exact.to(g.device))          # (NaN is a mismatch)
    if not bool(bad.any()):
        return None
    c, m, n = (int(v) for v in bad.nonzero()[0])
    return (f"{what}: chunk {c} row {m} column {col0 + n}: got {float(g[c, m, n])!r}, the exact sum is {float(exact[c, m, n])!r} "
            f"({int(bad.sum())} of {bad.numel()} elements differ; per chunk {[int(v) for v in bad.sum((1, 2))]})")


class GuardedPlanes:
    """an fp32 buffer [guard | n_chunks x prows x N planes | guard], all of it `poison` before the launch; a guard is one plane and 1024 words long, so a
    plane written one slot early or late lands in it"""

    def __init__(self, n_chunks, rows, N, dev, poison=PLANE_SENTINEL):
        assert rows % 32 == 0
        self.guard, self.numel = rows * N + 1024, n_chunks * rows * N
        self.buf = torch.full((2 * self.guard + self.numel,), poison, dtype=torch.float32, device=dev)
        self.bits = int(torch.tensor(poison, dtype=torch.float32).view(torch.int32))
        self.front, self.behind = self.buf[:self.guard], self.buf[self.guard + self.numel:]
        self.planes = self.buf[self.guard:self.guard + self.numel].view(n_chunks, rows, N)

    def ptr(self):
        return self.planes.data_ptr()

    def _is_poison(self, t):
        return t.view(torch.int32) == self.bits

    def untouched(self):
        return bool(self._is_poison(self.buf).all())

    def problems(self, M):
        """what is wrong with the buffer after a launch of M rows ([] when nothing is): the guards untouched, rows M.. of every plane exactly zero
        (today's contract), no poison left inside rows < M, nothing non-finite"""
        bad = []
        for name, g in (("in front of", self.front), ("behind", self.behind)):
            hit = ~self._is_poison(g)
            if bool(hit.any()):
                bad.append(f"{int(hit.sum())} words {name} the planes were written (first at offset {int(hit.nonzero()[0])} of that guard)")
        pad = self.planes[:, M:]
        if pad.numel() and not bool((pad.view(torch.int32) == 0).all()):
            bad.append(f"pad rows {M}.. are not zero ({int((pad.view(torch.int32) != 0).sum())} words)")
        left = self._is_poison(self.planes[:, :M])
        if bool(left.any()):
            c, m, n = (int(v) for v in left.nonzero()[0])
            bad.append(f"{int(left.sum())} elements of rows < {M} were never written (first: chunk {c} row {m} column {n})")
        if not bool(torch.isfinite(self.planes).all()):
            bad.append("a plane holds a non-finite value")
        return bad


def guarded_planes(n_chunks, rows, N, dev, poison=PLANE_SENTINEL):
    assert rows == prows(rows)
    return GuardedPlanes(n_chunks, rows, N, dev, poison)


# ------------------------------------------------------------------------------------------------ the weights of the 12-bit stream's three kinds
def z_operands(kind, M, N, K, KC, seed, row_rng=(-20, 20), col_rng=(-20, 20), x_max=X_MAX, be_max=BE_MAX):
    """bf16 exact operands for the 12-bit stream.  The stream stores, per (chunk, 32-column tile) unit, a window of sixteen binades; a weight outside
    it -- a zero among them -- is an exception, and a unit with more than 127 exceptions travels raw.  The exact weight spans ten binades per column
    (0.5 .. 6 * 2^6), so:
      clean     one column exponent per tile, no zeros: no exceptions at all
      outliers  the same with about twenty zeros per unit: exception headers
      raw       one exponent per COLUMN and every eighth weight zero: every unit is raw"""
    rows = spread_exps(M, *row_rng, seed + 1)
    if kind == "raw":
        return exact_operands(torch.bfloat16, M, N, K, seed, rows, spread_exps(N, *col_rng, seed + 2), x_max=x_max, be_max=be_max)
    share = 0.0 if kind == "clean" else 20.0 / (32 * min(K, KC))
    return exact_operands(torch.bfloat16, M, N, K, seed, rows, tile_exps(N, *col_rng, seed + 2), x_max=x_max, be_max=be_max, zero_share=share)


# ------------------------------------------------------------------------------------------------ the cases both test files share (computed once; read-only)
STREAMS = ("bf16", "fp16", "z_clean", "z_outliers", "z_raw", "q8", "q4", "q6")


def stream_dtype(stream):
    return torch.float16 if stream == "fp16" else torch.bfloat16


def stream_shapes(stream):
    return QUANT_SHAPES if stream in ("q8", "q4", "q6") else SHAPES


def operands(stream, M, N, K, KC, seed, row_rng=None, col_rng=None, **kw):
    if stream.startswith("z_"):
        return z_operands(stream[2:], M, N, K, KC, seed, row_rng or (-20, 20), col_rng or (-20, 20), **kw)
    dtype = stream_dtype(stream)
    rr, cr = EXP_RANGE[dtype]
    return exact_operands(dtype, M, N, K, seed, spread_exps(M, *(row_rng or rr), seed + 1), spread_exps(N, *(col_rng or cr), seed + 2), **kw)


@functools.lru_cache(maxsize=None)
def g1_case(stream, N, K, KC, M=ROWS[-1]):
    """(x [M, K], w [N, K], exact fp64 planes [n_chunks, M, N]) of a stream at one of SHAPES; a test takes the first rows of x"""
    x, w = operands(stream, M, N, K, KC, N + K + KC)
    return x, w, exact_planes(x, w, KC)


# gate|up: exponents that put the gates between 1e-3 and a few tens, where SiLU bends and saturates, and keep silu(g) * u inside fp16's range.
# GATE_MAX: glue_models.f3_model evaluates exp(-g) in fp64, the kernels in fp32, where it overflows below g = -88.7 (SiLU is then -0 in place of a
# bf16 subnormal); the model is the kernels' arithmetic for |g r| < 87 only, so the cases keep |g| below 40 and the row scale r below 2.
GATEUP_ROW_RNG, GATEUP_COL_RNG, GATE_MAX = (-12, -8), (-10, -4), 40.0


@functools.lru_cache(maxsize=None)
def gateup_case(stream, name, M):
    """(x [M, hidden], w = [Wg; Wu] [2 inter, hidden], exact fp64 planes [chunks, M, 2 inter]) of GATEUP_SHAPES[name]"""
    inter, hidden, chunks, x_max, be_max = GATEUP_SHAPES[name]
    x, w = operands(stream, M, 2 * inter, hidden, hidden // chunks, 7 * hidden + M, GATEUP_ROW_RNG, GATEUP_COL_RNG, x_max=x_max, be_max=be_max)
    exact = exact_planes(x, w, hidden // chunks)
    assert float(exact.sum(0).abs().max()) < GATE_MAX
    return x, w, exact
