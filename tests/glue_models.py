"""fp64 models of the fused glue kernels F1 / F1p / F1r / F2 / F3 (csrc/sjd_glue.hip), evaluated as the kernels' comments state their arithmetic:
intermediates in fp64, the value rounded to the activation dtype exactly at the documented points.  Pure torch on the CPU; nothing here imports
the package or touches a GPU.  tests/test_glue_models.py guards these models, tests/test_gpu_glue_bounds.py holds the kernels to them.

Two classes of output:
  A  only IEEE adds, multiplies and roundings in a fixed order (plane sums, residual updates, V copies, the table rotary): compared bit for bit.
  B  passes through rsqrtf / __expf / sincosf or a wave reduction: the fp32 intermediate may sit on a rounding boundary of the activation dtype,
     so a documented rounding point may land on the neighbouring dtype value.  Each model returns, beside the value, a per-element TOLERANCE that
     propagates one such flip per rounding point to the output.

How the tolerance is tracked (the rules behind every `*_tol` below; a pair (v, d) is a model value and a bound on |kernel - model|):
  round   (v, d) -> (dtype(v), d + ulp(dtype, |dtype(v)| + d)): what came in, plus one spacing of the dtype at the (perturbed) value.  ulp() is
          monotone in |v|, so the spacing at |v| + d bounds the spacing at any value the kernel can hold there.  A rounding whose operand is bit-exact
          in the kernel (a plane sum, a 16-bit input) adds nothing.
  scale   by an exact factor c: (c v, |c| d)
  product (a, da) (b, db) -> (a b, |a| db + |b| da + da db)
  sum     (a + b, da + db)
Every `f=` / `plant=` argument exists for tests/test_glue_models.py: f=torch.float32 turns a model into an fp32 emulation of the kernel, `plant`
names ONE deliberate defect (PLANTS) that the class B check must reject.
"""
import math

import torch

from tests.fp8_model import e4m3_value, sat_e4m3_bytes

F64 = torch.float64
_MANT = {torch.bfloat16: 7, torch.float16: 10}
_EMIN = {torch.bfloat16: -126, torch.float16: -14}
SHARE_CAP = 0.01                     # the share of elements of a class B tensor that may differ from the model at all
SILU_LIPSCHITZ = 1.1                 # sup |silu'(x)| = 1.0998 (at x = 2.3994): a perturbation of the gate grows by at most this factor
PLANTS = ("trunc", "eps10", "drop_plane", "neighbour_sumsq", "cs_unrounded", "gain_first", "swap_gate_up")


def ulp(dtype, v):
    """spacing of `dtype` at |v| (fp64 tensor), floored at the smallest subnormal"""
    v = torch.as_tensor(v, dtype=F64).abs().clamp(max=float(torch.finfo(dtype).max))
    _, e = torch.frexp(v)                                       # |v| = m 2^e, m in [0.5, 1): floor(log2 |v|) = e - 1
    e = torch.where(v > 0, e - 1, torch.full_like(e, _EMIN[dtype])).clamp(min=_EMIN[dtype])
    return torch.ldexp(torch.ones_like(v), e - _MANT[dtype])


def ulp_e4m3(v):
    """spacing of OCP e4m3 at |v|: three mantissa bits, 2^-9 below 2^-6, the top binade [256, 448]"""
    v = torch.as_tensor(v, dtype=F64).abs().clamp(max=448.0)
    _, e = torch.frexp(v)
    e = torch.where(v > 0, e - 1, torch.full_like(e, -6)).clamp(min=-6)
    return torch.ldexp(torch.ones_like(v), e - 3)


def _trunc(x, dtype):
    """round toward zero (the planted defect): the nearest-even result, stepped one code toward zero where it overshot"""
    r = x.to(dtype)
    over = (r.to(F64).abs() > x.to(F64).abs()) & torch.isfinite(r)
    bits = r.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(dtype)        # sign-magnitude codes: code - 1 is one step toward zero


class _Num:
    def __init__(self, dtype, f=F64, plant=None):
        assert plant is None or plant in PLANTS
        self.dtype, self.f, self.plant = dtype, f, plant

    def q(self, x):
        """x -> dtype (round to nearest even) -> back to the working precision"""
        return (_trunc(x, self.dtype) if self.plant == "trunc" else x.to(self.dtype)).to(self.f)

    def rnd(self, v, d=0.0, exact=False):
        r = self.q(v)
        d = torch.as_tensor(d, dtype=F64)
        return r, (d if exact else d + ulp(self.dtype, r.to(F64).abs() + d))


def _mul(a, da, b, db):
    a64, b64 = a.to(F64).abs(), b.to(F64).abs()
    return a * b, a64 * db + b64 * da + da * db


def planes_sum(planes):
    """fp32 split-K planes [n_chunks, R, N] -> their fp32 sum in chunk order from 0.0f (IEEE adds in a fixed order: bit-reproducible)"""
    assert planes.dtype == torch.float32
    s = torch.zeros(planes.shape[1:], dtype=torch.float32)
    for c in range(planes.shape[0]):
        s = s + planes[c]
    return s


def _planes(planes, plant):
    return planes[:-1] if plant == "drop_plane" else planes


def residual(h, d, num):
    """dtype(h + dtype(d)): h in the activation dtype, d the projection output (fp32 plane sum, or a 16-bit tensor)"""
    return num.q(h.to(num.f) + num.q(d.to(num.f)))


def row_scale(sumsq, hidden, eps, rows, num):
    """r = 1 / sqrt(sumsq_total / hidden + eps) per row from F1r's per-slice sums [slices, R] -> [rows, 1]"""
    tot = sumsq.to(num.f).sum(0)
    if num.plant == "neighbour_sumsq":
        tot = torch.roll(tot[:rows], -1, 0) if rows > 1 else tot * 2
    e = eps * 10 if num.plant == "eps10" else eps
    return (1.0 / torch.sqrt(tot[:rows] / hidden + e))[:, None]


# ------------------------------------------------------------------------------------------------ F1 / F1p
def f1_model(h, w, eps, dtype, delta=None, planes=None, post=False, f=F64, plant=None):
    """F1 / F1p.  h [rows, hidden], w [hidden], delta [rows, hidden] in `dtype`; planes fp32 [n_chunks, prows, hidden].
    pre-norm:  h' = dtype(h + dtype(d)) (class A);  y = dtype(w * p1), p1 = dtype(h' * inv), inv = 1 / sqrt(mean(h'^2) + eps)
        y_tol = |w| ulp(p1) + ulp(|y| + |w| ulp(p1)): p1 is the one rounding point upstream of y (h' is bit-exact, inv is not a dtype value), the
        gain is an exact factor, and the final store adds its own ulp.
    POST:      delta = dtype(d) (bit-exact), p2 = dtype(delta * inv(delta)), p3 = dtype(w * p2), h' = dtype(h + p3)
        h_tol = d3 + ulp(|h'| + d3), d3 = |w| ulp(p2) + ulp(|p3| + |w| ulp(p2)): p2's flip scaled by the gain, p3's own, the store's own.
    -> dict(h, y, y_tol) / dict(h, h_tol); values in `f`, tolerances fp64."""
    num = _Num(dtype, f, plant)
    rows = h.shape[0]
    hf, wf = h.to(f), w.to(f)
    d = None
    if planes is not None:
        d = num.q(planes_sum(_planes(planes, plant))[:rows].to(f))
    elif delta is not None:
        d = delta.to(f)
    e = eps * 10 if plant == "eps10" else eps
    if not post:
        x = hf if d is None else num.q(hf + d)
        inv = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + e)
        if plant == "gain_first":
            y, y_tol = num.rnd(wf * (x * inv))
        else:
            p1, d1 = num.rnd(x * inv)
            y, y_tol = num.rnd(*_mul(wf, 0.0, p1, d1))
        return dict(h=x, y=y, y_tol=y_tol)
    assert d is not None
    inv = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + e)
    if plant == "gain_first":
        p3, d3 = num.rnd(wf * (d * inv))
    else:
        p2, d2 = num.rnd(d * inv)
        p3, d3 = num.rnd(*_mul(wf, 0.0, p2, d2))
    hn, h_tol = num.rnd(hf + p3, d3)
    return dict(h=hn, h_tol=h_tol)


# ------------------------------------------------------------------------------------------------ F1r
def f1r_model(h, dtype, planes=None, f=F64, plant=None):
    """F1r: h' = dtype(h + dtype(plane sum)) (class A; planes None: h' = h) and the sums of h'^2 per 512-column slice, in fp64.
    -> dict(h, sumsq [slices, rows], sumsq_tol): the kernel sums hidden fp32 products in fp32, so a slice may differ from fp64 by
    hidden 2^-24 relative; the absolute floor is that factor times the largest h'^2 of the row (a slice of zeros beside one large element)."""
    num = _Num(dtype, f, plant)
    rows, hidden = h.shape
    x = h.to(f)
    if planes is not None:
        x = residual(h, planes_sum(_planes(planes, plant))[:rows], num)
    x2 = x.to(F64) ** 2
    slices = (hidden + 511) // 512
    ss = torch.stack([x2[:, s * 512:(s + 1) * 512].sum(-1) for s in range(slices)])
    tol = hidden * 2.0 ** -24 * torch.maximum(ss, x2.max(-1).values[None])
    return dict(h=x, sumsq=ss, sumsq_tol=tol)


# ------------------------------------------------------------------------------------------------ F3
def f3_model(dtype, gu=None, planes=None, rows=None, row_norm=None, f=F64, plant=None):
    """F3: y = dtype(s * u), s = dtype(silu(g)).  gu [rows, 2I] in `dtype` (gate | up), or planes fp32 [n_chunks, prows, 2I] with an optional
    row_norm = (sumsq [slices, R] fp32, hidden, eps): g, u = dtype(sum * r).
    dense / planes without r: g and u are bit-exact, s is the one rounding point upstream:  y_tol = |u| ulp(s) + ulp(|y| + |u| ulp(s))
    planes with r: dg = ulp(g), du = ulp(u) (the products with r are fp32 intermediates); silu is 1.1-Lipschitz, so ds = 1.1 dg + ulp(|s| + 1.1 dg);
        y_tol = dy + ulp(|y| + dy), dy = |s| du + |u| ds + ds du
    -> dict(y, y_tol, g): g the gate as the kernel's SiLU sees it (the share of differing elements is counted over |g| <= 8)."""
    num = _Num(dtype, f, plant)
    if planes is not None:
        s = planes_sum(_planes(planes, plant))[:rows].to(f)
        if row_norm is not None:
            s = s * row_scale(*row_norm, rows, num)
        x, dx = num.rnd(s, exact=row_norm is None)
    else:
        x, dx = gu.to(f), torch.zeros((), dtype=F64)
    inter = x.shape[1] // 2
    g, u = x[:, :inter], x[:, inter:]
    dg, du = (dx[:, :inter], dx[:, inter:]) if dx.dim() else (dx, dx)
    if plant == "swap_gate_up":
        g, u, dg, du = u, g, du, dg
    sl, ds = num.rnd(g / (1.0 + torch.exp(-g)), SILU_LIPSCHITZ * dg)
    y, y_tol = num.rnd(*_mul(sl, ds, u, du))
    return dict(y=y, y_tol=y_tol, g=g)


# ------------------------------------------------------------------------------------------------ F2, rotate-half path
def f2_source(dtype, qkv=None, planes=None, rows=None, row_norm=None, f=F64, plant=None):
    """the [rows, ncol] values F2 starts from and their tolerance: a 16-bit tensor as it is, or dtype(plane sum [* r])"""
    num = _Num(dtype, f, plant)
    if planes is None:
        return qkv.to(f), torch.zeros(qkv.shape, dtype=F64)
    s = planes_sum(_planes(planes, plant))[:rows].to(f)
    if row_norm is not None:
        s = s * row_scale(*row_norm, rows, num)
    x, dx = num.rnd(s, exact=row_norm is None)
    return x, dx + torch.zeros(x.shape, dtype=F64)


def _head_layernorm(x, dx, gain, bias, num):
    """per-head LayerNorm (eps 1e-5) over the last dim; gain / bias [heads, D] (already expanded from their shards).
    n = dtype((x - mean) inv), g = dtype(n gain), y = dtype(g + bias).  A flip of x_j moves the statistics of the whole head; to first order
    dn_i/dx_j = inv (delta_ij - 1/D - n_i n_j / D), so  dn <= inv (dx_i + mean_j dx_j + |n_i| mean_j |n_j| dx_j)  (zero when x is bit-exact)."""
    D = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    inv = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    nx = xc * inv
    n64, i64 = nx.to(F64).abs(), inv.to(F64)
    dn = i64 * (dx + dx.mean(-1, keepdim=True) + n64 * (n64 * dx).mean(-1, keepdim=True))
    assert D == gain.shape[-1]
    if num.plant == "gain_first":
        g, dg = num.rnd(nx * gain.to(num.f), dn * gain.to(F64).abs())
    else:
        n, dn = num.rnd(nx, dn)
        g, dg = num.rnd(*_mul(n, dn, gain.to(num.f), 0.0))
    return num.rnd(g + bias.to(num.f), dg)


def f2_model(dtype, positions, inv_freq, H, Hkv, D, qkv=None, planes=None, row_norm=None, qn=None, kn=None, qk_shards=1, kv_scale=None,
             f=F64, plant=None):
    """F2, rotate-half path, for T = len(positions) tokens.  qn / kn = (gain, bias) [qk_shards, D] or None.
    x = the source (f2_source); q / k heads: optional LayerNorm (_head_layernorm); RoPE with ang = fp32(pos) * inv_freq IN FP32, c = dtype(cos ang),
    s = dtype(sin ang) taken in fp64 of that fp32 angle;  out[:half] = dtype(dtype(x0 c) + dtype(-x1 s)), out[half:] = dtype(dtype(x1 c) + dtype(x0 s)).
        with (x, dx), (c, ulp c), (s, ulp s): each product a = dtype(x c): da = |x| ulp(c) + |c| dx + dx ulp(c), plus its own ulp; the sum adds
        both and the store's ulp -- the `round` / `product` / `sum` rules of the module docstring, applied in the order of the formula.
    V is the rounded copy of x (bit-exact unless r is applied).
    kv_scale = (k, v): the cache holds sat_e4m3(dtype_value * fp32(1 / scale)); k8 / v8 are the DECODED bytes (the e4m3 value, unscaled) and their
        tolerance d * inv_scale + ulp_e4m3(|value| + d * inv_scale): the 16-bit value's tolerance scaled, plus one e4m3 spacing.
    -> dict(q [T,H,D], q_tol, k [T,Hkv,D], k_tol, v, v_tol [, k8, k8_tol, v8, v8_tol])"""
    num = _Num(dtype, f, plant)
    T = positions.numel()
    x, dx = f2_source(dtype, qkv, planes, T, row_norm, f, plant)
    x, dx = x.view(T, H + 2 * Hkv, D), dx.view(T, H + 2 * Hkv, D)
    ang = positions.reshape(-1).to(torch.float32)[:, None] * inv_freq.to(torch.float32)[None, :]          # fp32 product, as the kernel and the reference
    cosv, sinv = torch.cos(ang.to(f)), torch.sin(ang.to(f))
    if plant == "cs_unrounded":
        (c, dc), (s, ds) = (cosv, torch.zeros((), dtype=F64)), (sinv, torch.zeros((), dtype=F64))
    else:
        (c, dc), (s, ds) = num.rnd(cosv), num.rnd(sinv)
    c, s = c[:, None, :], s[:, None, :]
    dc, ds = (dc[:, None, :], ds[:, None, :]) if dc.dim() else (dc, ds)
    out = {}
    for name, h0, nh, norm in (("q", 0, H, qn), ("k", H, Hkv, kn)):
        y, dy = x[:, h0:h0 + nh], dx[:, h0:h0 + nh]
        if norm is not None:
            per = nh // qk_shards
            gain, bias = (t.repeat_interleave(per, dim=0) for t in norm)
            y, dy = _head_layernorm(y, dy, gain, bias, num)
        half = D // 2
        y0, y1, d0, d1 = y[..., :half], y[..., half:], dy[..., :half], dy[..., half:]
        a0, b0 = num.rnd(*_mul(y0, d0, c, dc)), num.rnd(*_mul(-y1, d1, s, ds))
        a1, b1 = num.rnd(*_mul(y1, d1, c, dc)), num.rnd(*_mul(y0, d0, s, ds))
        o0, o1 = num.rnd(a0[0] + b0[0], a0[1] + b0[1]), num.rnd(a1[0] + b1[0], a1[1] + b1[1])
        out[name], out[name + "_tol"] = torch.cat((o0[0], o1[0]), -1), torch.cat((o0[1], o1[1]), -1)
    out["v"], out["v_tol"] = x[:, H + Hkv:], dx[:, H + Hkv:]
    if kv_scale is not None:
        for name, sc in (("k", kv_scale[0]), ("v", kv_scale[1])):
            inv32 = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(sc, dtype=torch.float32)
            val = e4m3_value(sat_e4m3_bytes((out[name].to(torch.float32) * inv32).contiguous())).to(F64)
            d = out[name + "_tol"] * float(inv32)
            out[name + "8"], out[name + "8_tol"] = val, d + ulp_e4m3(val.abs() + d)
    return out


# ------------------------------------------------------------------------------------------------ F2, table path (LlamaGen)
def f2_table_model(dtype, positions, table, S_max, H, Hkv, D, qkv=None, planes=None, head_pad=None, fma=0):
    """F2 with SJD_F2_ROPE_TABLE: class A throughout.  x = the 16-bit source (dense, or dtype(plane sum)); row p = clamp(position, 0, S_max - 1) of
    the fp32 (cos, sin) table [S_rows, D/2, 2]; the interleaved pair (2i, 2i + 1):  out0 = x0 c - x1 s, out1 = x1 c + x0 s, every product and sum
    rounded to fp32 separately, then ONE rounding to dtype.  head_pad = 128 (D = 100): columns 100..127 of q, k and v are zeros.
    fma = 1 / 2 is the planted contraction (the first / second product fused into the sum) that the bit-for-bit comparison must reject.
    -> dict(q [T,H,DS], k [T,Hkv,DS], v [T,Hkv,DS]) in `dtype`"""
    T = positions.numel()
    x = (qkv if planes is None else planes_sum(planes)[:T].to(dtype)).view(T, H + 2 * Hkv, D)
    cs = table[positions.reshape(-1).clamp(0, S_max - 1)]                # [T, D/2, 2]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    xf = x.to(torch.float32)
    x0, x1 = xf[..., 0::2], xf[..., 1::2]
    if fma == 1:                       # the first product fused into the sum (exact in fp64: 11 x 24 bits), the second rounded to fp32
        o0 = (x0.double() * c.double() - (x1 * s).double()).to(torch.float32)
        o1 = (x1.double() * c.double() + (x0 * s).double()).to(torch.float32)
    elif fma == 2:                     # ... or the second
        o0 = ((x0 * c).double() - x1.double() * s.double()).to(torch.float32)
        o1 = ((x1 * c).double() + x0.double() * s.double()).to(torch.float32)
    else:
        o0, o1 = x0 * c - x1 * s, x1 * c + x0 * s
    rot = torch.stack((o0, o1), -1).flatten(-2).to(dtype)
    q, k, v = rot[:, :H], rot[:, H:H + Hkv], x[:, H + Hkv:]
    if head_pad is not None and head_pad != D:
        q, k, v = (torch.cat((t, torch.zeros(*t.shape[:-1], head_pad - D, dtype=dtype)), -1) for t in (q, k, v))
    return dict(q=q, k=k, v=v)


def cache_rows(B, n, kv_lens, S_max):
    """where the window's rows go: -> list of (b, i, cache row) for every row that fits; rows with kv_len + i >= S_max are dropped"""
    return [(b, i, kv_lens[b] + i) for b in range(B) for i in range(n) if kv_lens[b] + i < S_max]


# ------------------------------------------------------------------------------------------------ the class B check
def class_b(got, model, tol, count=None):
    """got / model / tol: tensors of one shape (any float dtype; compared in fp64).  -> (share of the counted elements that differ at all, worst
    error / bound over ALL elements).  Equal values (inf == inf, NaN where the model has NaN) are no difference; count: mask of the elements the
    share is taken over (default: all)."""
    g, m, t = got.to(F64), model.to(F64), tol.to(F64)
    same = (g == m) | (torch.isnan(g) & torch.isnan(m))
    err = torch.where(same, torch.zeros_like(g), (g - m).abs())
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    ratio = torch.where(same, torch.zeros_like(g), err / t)
    cnt = ~same if count is None else (~same & count)
    total = same.numel() if count is None else int(count.sum())
    return float(cnt.sum()) / max(total, 1), float(ratio.max()) if ratio.numel() else 0.0


def class_b_ok(got, model, tol, count=None):
    share, worst = class_b(got, model, tol, count)
    return share <= SHARE_CAP and worst <= 1.0


# ------------------------------------------------------------------------------------------------ the inputs the GPU tests use
SENTINEL_BITS = 0x4B4D               # a finite odd 16-bit pattern: bf16 1.3e7, fp16 14.6
PLANE_SENTINEL = 7.7e7               # pad rows of fp32 planes: a kernel that reads one is far off


def prows(rows):
    return (rows + 31) // 32 * 32


def edge_rows(x):
    """rows 1..3 of a Gaussian [rows, hidden] block become the rows where kernels go wrong without a random input noticing: one scaled to 3e-3
    (mean(x^2) near eps), one of zeros, one with magnitudes of a few hundred (squares overflow fp16, not fp32).  -> mask of the rows left Gaussian"""
    rows = x.shape[0]
    plain = torch.ones(rows, dtype=torch.bool)
    if rows >= 4:
        x[1] *= 3e-3
        x[2] = 0.0
        x[3] *= 300.0
        plain[1:4] = False
    return plain


def make_planes(gen, n_chunks, rows, ncol, scale=None):
    """fp32 planes [n_chunks, prows, ncol] whose sum has unit variance; pad rows hold PLANE_SENTINEL.  scale [rows]: per-row factor"""
    p = torch.full((n_chunks, prows(rows), ncol), PLANE_SENTINEL, dtype=torch.float32)
    body = torch.randn(n_chunks, rows, ncol, generator=gen) / n_chunks ** 0.5
    if scale is not None:
        body = body * scale[None, :, None]
    p[:, :rows] = body
    return p


def make_sumsq(gen, slices, rows, spread):
    """F1r's per-slice sums [slices, prows] for hidden = 512 * slices: mean squares spread over 10^+-spread from row to row (a neighbour's value is
    far off), row 1 at mean(h^2) = eps = 1e-5 (r = 224: the one place eps matters; its planes are scaled to 3e-3), pad rows PLANE_SENTINEL"""
    ss = torch.full((slices, prows(rows)), PLANE_SENTINEL, dtype=torch.float32)
    ss[:, :rows] = (torch.rand(slices, rows, generator=gen) + 0.5) * 512 * torch.logspace(-spread, spread, rows)[None, :]
    if rows > 1:
        ss[:, 1] = 1e-5 * 512
    return ss


def _eps_row_scale(rows, slices, base=1.0):
    scale = torch.full((rows,), base)
    if slices and rows > 1:
        scale[1] = 3e-3 * base
    return scale


def f1_inputs(dtype, rows, hidden, n_chunks=0, dense=False, seed=0):
    """-> dict(h, w, delta | None, planes | None, plain): rows 1..3 are the edge rows when there are at least four"""
    gen = torch.Generator().manual_seed(1000 * hidden + 10 * rows + n_chunks + seed)
    h = torch.randn(rows, hidden, generator=gen)
    scale = torch.ones(rows)
    plain = edge_rows(h)
    if rows >= 4:
        scale[1], scale[2], scale[3] = 3e-3, 0.0, 300.0
    w = (1 + 0.1 * torch.randn(hidden, generator=gen)).to(dtype)
    delta = (torch.randn(rows, hidden, generator=gen) * scale[:, None]).to(dtype) if dense else None
    planes = make_planes(gen, n_chunks, rows, hidden, scale) if n_chunks else None
    return dict(h=h.to(dtype), w=w, delta=delta, planes=planes, plain=plain)


F1_DENSE_CASES = [(r, hd, src) for hd in (8, 2048, 2056, 8192) for r in (1, 7) for src in ("dense", "none")]
F1_POST_DENSE_CASES = [(1, 8), (7, 2048), (7, 2056), (1, 8192)]
# (rows, hidden, n_chunks): every hidden, every chunk count, both row counts; 33 rows with the 17 planes of two batches of sixteen and the odd stripe
F1P_CASES = [(1, 8, 1), (33, 8, 17), (1, 4096, 4), (33, 4096, 5), (33, 4104, 16), (1, 4104, 17), (33, 8192, 1), (1, 8192, 16), (33, 8192, 17),
             (1, 4104, 5), (33, 4096, 16), (33, 4104, 4)]
F1P_POST_CASES = F1P_CASES + [(1, 16384, 5), (33, 16384, 17)]
# (rows, hidden, n_chunks): the three load schedules (<= 8, 9..16, > 16) at every hidden; 0 = part None
F1R_CASES = [(1, 4, 1), (33, 4, 9), (1, 512, 8), (33, 512, 17), (33, 516, 15), (1, 516, 16), (33, 768, 9), (1, 768, 17), (33, 3200, 8),
             (1, 3200, 15), (33, 3200, 16), (33, 516, 1), (33, 768, 0), (1, 3200, 0)]


def f3_extremes(dtype):
    return torch.tensor([0.0, -0.0, 30.0, -30.0, 100.0, -100.0, float(torch.finfo(dtype).max)], dtype=torch.float32)


def f3_inputs(dtype, rows, inter, n_chunks=0, slices=0, seed=0):
    """-> dict(gu | None, planes | None, row_norm | None, hidden).  The first gate columns of row 0 hold the extremes when I >= 8 (7 values);
    with planes they sit in plane 0 over zeros in the others, and row 0's sumsq keeps r below 1."""
    gen = torch.Generator().manual_seed(77 * inter + 5 * rows + 11 * n_chunks + slices + seed)
    ext = f3_extremes(dtype)
    if not n_chunks:
        gu = torch.randn(rows, 2 * inter, generator=gen) * 2
        gu[0, :ext.numel()] = ext
        return dict(gu=gu.to(dtype), planes=None, row_norm=None)
    planes = make_planes(gen, n_chunks, rows, 2 * inter, _eps_row_scale(rows, slices, 2.0))
    planes[:, 0, :ext.numel()] = 0.0
    planes[0, 0, :ext.numel()] = ext
    row_norm = None
    if slices:
        ss = make_sumsq(gen, slices, rows, 1.0)
        ss[:, 0] = 4 * 512.0                                    # r = 0.5 on the row of the extremes
        row_norm = (ss, 512 * slices, 1e-5)
    return dict(gu=None, planes=planes, row_norm=row_norm)


F3_DENSE_CASES = [(1, 8), (5, 1376), (256, 16392)]
# (rows, inter, n_chunks, slices)
F3_PLANE_CASES = [(33, 8, 1, 0), (33, 136, 4, 0), (33, 136, 5, 0), (33, 8, 4, 1), (33, 136, 1, 8), (33, 136, 5, 9), (33, 8, 5, 8), (33, 136, 4, 9)]


def f2_inputs(dtype, D, H, Hkv, T, n_chunks=0, slices=0, qk_norm=False, qk_shards=1, positions=None, seed=0):
    gen = torch.Generator().manual_seed(13 * D + 7 * n_chunks + 3 * slices + H + 100 * T + seed)
    ncol = (H + 2 * Hkv) * D
    out = dict(qkv=None, planes=None, row_norm=None, qn=None, kn=None)
    if n_chunks:
        out["planes"] = make_planes(gen, n_chunks, T, ncol, _eps_row_scale(T, slices))
        if slices:
            out["row_norm"] = (make_sumsq(gen, slices, T, 0.5), 512 * slices, 1e-5)
    else:
        out["qkv"] = torch.randn(T, ncol, generator=gen).to(dtype)
    if qk_norm:
        mk = lambda: ((1 + 0.2 * torch.randn(qk_shards, D, generator=gen)).to(dtype), (0.1 * torch.randn(qk_shards, D, generator=gen)).to(dtype))
        out["qn"], out["kn"] = mk(), mk()
    out["inv_freq"] = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    out["positions"] = positions
    return out


F2_B, F2_N, F2_S = 2, 5, 24
F2_POS = torch.tensor([[0, 1, 2, 3, 4], [8190, 8191, 8192, 8193, 8194]])
F2_KV_HOST, F2_KV_BLOBS = 3, (3, 21)          # blobs: batch row 1 writes rows 21..23, its last two window rows fall beyond S_max = 24
# (H, Hkv, n_chunks, slices, qk_norm, qk_shards, blobs, fp8): every plane count (<= 2, <= 4, > 4, > 8), every slice count, norm on and off
F2_CASES = [(3, 1, 0, 0, False, 1, False, False), (3, 1, 0, 0, True, 1, True, False), (3, 1, 1, 0, False, 1, True, False),
            (3, 1, 2, 1, True, 1, False, False), (3, 1, 3, 8, False, 1, True, False), (3, 1, 4, 9, True, 1, False, False),
            (3, 1, 5, 17, True, 1, True, False), (3, 1, 8, 0, True, 1, False, False), (3, 1, 9, 8, False, 1, False, False),
            (3, 1, 17, 9, True, 1, True, False), (4, 2, 3, 9, True, 2, True, False), (4, 2, 0, 0, True, 2, False, False),
            (3, 1, 0, 0, False, 1, True, True), (3, 1, 5, 9, True, 1, True, True), (3, 1, 9, 0, False, 1, False, True)]
F2_KV_SCALE = (0.037, 0.051)
# many-row kernel: 65 rows of planes, (H, Hkv) = (4, 4), D = 128, bf16: (n_chunks, slices, qk_norm, qk_shards, fp8)
F2_ROWS_B, F2_ROWS_N, F2_ROWS_S, F2_ROWS_KV = 5, 13, 16, 5          # rows 5..17: the last two of every batch row fall beyond S_max = 16
F2_ROWS_CASES = [(5, 9, True, 1, False), (4, 0, False, 1, False), (9, 17, True, 2, False), (3, 8, True, 1, True)]


def f2_rows_positions():
    return (torch.tensor([0, 100, 8185, 3000, 70000])[:, None] + torch.arange(F2_ROWS_N)[None]).contiguous()


def f2_table_inputs(dtype, D, H, Hkv, B, n, src, S_max, seed=0):
    """LlamaGen's table mode: a (cos, sin) table of S_max + 3 rows, row 2 zeros (a condition row); positions with one negative, one >= S_max and
    one on the zero row.  src: 'dense' or a plane count.
    After ONE rounding to 16 bits a contracted product shows in about one element of 2^13, so two tokens are built to show it: token 3 reads table
    row 1 with s = 1/2 and c = fp32((x1 / 2) / x0) of its first q head, token 4 row 3 with c = 1/2 and s = fp32((x0 / 2) / x1).  There x0 c - x1 s
    cancels: with both products rounded to fp32 the difference is 0 (or one fp32 step), with either product fused into the subtraction it is the
    product's rounding error -- a nonzero 16-bit value (the head is scaled by 1024 so that fp16 holds it)."""
    gen = torch.Generator().manual_seed(17 * D + 5 * B * n + (0 if src == "dense" else src) + seed)
    T, ncol = B * n, (H + 2 * Hkv) * D
    ang = torch.rand(S_max + 3, D // 2, generator=gen) * 6.283
    table = torch.stack((torch.cos(ang), torch.sin(ang)), -1).contiguous()
    table[2] = 0.0
    pos = torch.randint(4, S_max, (T,), generator=gen)
    pos[:5] = torch.tensor([-3, S_max + 1, 2, 1, 3])
    out = dict(table=table, positions=pos, qkv=None, planes=None)
    if src == "dense":
        q = torch.randn(T, ncol, generator=gen)
        q[3:5, :D] *= 1024.0
        x = out["qkv"] = q.to(dtype)
    else:
        out["planes"] = make_planes(gen, src, T, ncol)
        out["planes"][:, 3:5, :D] *= 1024.0
        x = planes_sum(out["planes"])[:T].to(dtype)
    x0, x1 = x[3:5, :D:2].double(), x[3:5, 1:D:2].double()
    table[1, :, 0], table[1, :, 1] = ((x1[0] / 2) / x0[0]).to(torch.float32), 0.5
    table[3, :, 0], table[3, :, 1] = 0.5, ((x0[1] / 2) / x1[1]).to(torch.float32)
    assert torch.isfinite(table).all()
    return out


# (D, head_pad, B, n, H, Hkv, src, S_max, kv_len): 5 rows dense, 5 rows of planes, 65 rows of planes (heads in fours: the many-row kernel)
F2_TABLE_CASES = [(D, pad, B, n, H, H, src, S, kv) for D, pad in ((64, None), (128, None), (100, 128))
                  for B, n, H, src, S, kv in ((1, 5, 2, "dense", 8, 4), (1, 5, 2, 3, 8, 4), (5, 13, 4, 5, 16, 5))]
