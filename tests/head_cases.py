"""Inputs, the fp64 model and the branch predicates that hold K2's output-head front end -- k2_logits_to_probs_sample<PART>, k2_row_scale(s), k2_round16
and k2a_head_combine in csrc/sjd_sampling.hip -- to an independent statement at every (chunks, slices) pair the product runs and at the edges of
every branch in between.

What the front end does per row: sum the lm_head's fp32 split-K planes in chunk order, multiply by the folded final-RMSNorm row scale
rsqrtf(sum of slices / hidden + eps), round to the activation dtype, the same for the uncond row `urow_off` rows further, and hand the pair to the
CFG combine.  THE MODEL is glue_models.f2_source -- the fp64 statement of dtype(plane sum [* r]) with its per-element tolerance; nothing is restated
here.  Without a fold (or with round_dtype fp32, the form K2 takes behind K2a) the output is class A: compared bit for bit.  With a fold it is
class B: f2_source's tolerance and glue_models.SHARE_CAP.  No bound of this module is new.

Pure torch / numpy on the CPU; nothing here imports the package or touches a GPU.  tests/test_head_cases.py guards the inputs (each reaches the branch
it is named for, the fp32 emulation passes, every wrong model is rejected), tests/test_gpu_head_exact.py runs the kernels.
"""
import functools
import math
import zlib

import torch

from tests import glue_models as M
from tests import sampling_edge_cases as SE

F64 = torch.float64
GUIDANCE, EPS = 3.0, 1e-5
N_ROWS, LMAX = 4, 8                  # live rows of a launch / rows of probs_out, the observers and the token buffer
HEAD_COMBINE_MIN_COLS = 16384        # ops._HEAD_COMBINE_MIN_COLS's default: K2a serves heads at least this wide

# ------------------------------------------------------------------------------------------------ the shape table
# name -> (chunks, slices, hidden).  chunks = ceil(hidden / HEAD_CFG[0]), slices = ceil(hidden / 512) (sjd_residual_sumsq).  The product triples, restated
# from launch_shapes (HEAD_CFG 1024, HEAD_CFG_WIDE 2048, LLAMAGEN_SETS' head chunks 640 / 1088 / 1600) and the backbones' hidden sizes;
# tests/test_head_cases.py recomputes them from launch_shapes itself.
PRODUCT = dict(lumina7b=(4, 8, 4096), emu3=(2, 8, 4096), swin30b=(8, 16, 8192), llamagen_xl=(2, 3, 1280), llamagen_3b=(3, 7, 3200),
               llamagen_3b_wide=(2, 7, 3200))
PRODUCT_SOURCE = dict(lumina7b=("HEAD_CFG", 4096), emu3=("HEAD_CFG_WIDE", 4096), swin30b=("HEAD_CFG", 8192), llamagen_xl=((False, 64), 1280),
                      llamagen_3b=((True, 64), 3200), llamagen_3b_wide=((True, 128), 3200))
# the branch edges, as pairs: chunks {1, 2, 4, 8, 9, 16} (8: the brim of "all planes in flight", 9: the first count of the loop), slices
# {1, 3, 7, 8, 9, 16} (8: the brim of the register-preloaded statistics, where min(q, slices - 1) is never clamped; 9, 16: k2_row_scales' second batch)
EDGES = {f"c{c}s{s}": (c, s, 512 * s) for c, s in ((1, 1), (4, 7), (8, 8), (9, 9), (16, 16), (1, 16), (16, 1), (9, 8), (8, 9), (2, 3))}
SHAPES = {**PRODUCT, **EDGES}
CHUNK_AXIS, SLICE_AXIS = (1, 2, 4, 8, 9, 16), (1, 3, 7, 8, 9, 16)

# ------------------------------------------------------------------------------------------------ the windows
# V, the head's vocabulary columns [cols), the hull [wlo, whi) of the image rows' rule (None: text rows over all of V), the gap of the two-range rule of
# row 1, top_k, and the form the row's scores are staged in (csrc/sjd_sampling.hip:294, 381).  The smallest sizes that still reach each form:
#   image0 / image992  an 8192-column window inside V = 9216, the head starting at column 0 / at a non-zero multiple of 32 (odd hull bounds): registers
#   emu3               the 32768 visual columns of Emu3's V = 184622 (V % 4 = 2: every column of K2's own pass takes the scalar branch): LDS, K2a by default
#   text               text rows over all of V = 9216.  9216 columns are three groups of 4 * SJD_TPB: this window is staged in REGISTERS, like the image rows
#   text_wide          text rows over all of V = 38432, the smallest multiple of 32 above the 38400 floats of sjd_stage_lds_floats' cap: the global form
WINDOWS = dict(
    image0=dict(V=9216, cols=(0, 8224), hull=(4, 8196), gap=(4000, 4100), top_k=2000, form="registers"),
    image992=dict(V=9216, cols=(992, 9216), hull=(1001, 9193), gap=(5000, 5101), top_k=2000, form="registers"),
    emu3=dict(V=184622, cols=(151840, 184640), hull=(151854, 184622), gap=(160000, 160100), top_k=2048, form="lds"),
    text=dict(V=9216, cols=(0, 9216), hull=None, gap=None, top_k=10, form="registers"),
    text_wide=dict(V=38432, cols=(0, 38432), hull=None, gap=None, top_k=10, form="global"),
)
# (shape, window): pairs, not a product -- every shape on the cheap window, the product triples on the windows their backbones use, the edges of both
# axes on every other window
CASES = tuple((s, "image0") for s in SHAPES) + (
    ("lumina7b", "image992"), ("swin30b", "image992"), ("c9s9", "image992"), ("c1s1", "image992"),
    ("emu3", "emu3"), ("c8s8", "emu3"), ("c9s9", "emu3"), ("c4s7", "emu3"), ("swin30b", "emu3"),
    ("lumina7b", "text"), ("swin30b", "text"), ("c16s1", "text"),
    ("lumina7b", "text_wide"), ("c9s9", "text_wide"))
# (rounding dtype, fold): class B with a fold, class A without; fp32 = no rounding (the head K2 reads behind K2a), without a fold only
FORMS = ((torch.bfloat16, True), (torch.float16, True), (torch.bfloat16, False), (torch.float16, False), (torch.float32, False))
FORM_IDS = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


def rules_of(window, n_rows=N_ROWS, two_range_rows=(1,), forced=None):
    """rule dicts (oracle.sjd_oracle.rule's arguments) of the rows: the hull as one range; on `two_range_rows` two ranges with the gap between them;
    forced: {row: token}"""
    w = WINDOWS[window]
    out = []
    for i in range(n_rows):
        if forced and i in forced:
            out.append(dict(ranges=(), forced=forced[i], top_k=0))
        elif w["hull"] is None:
            out.append(dict(ranges=(), forced=-1, top_k=w["top_k"]))
        elif i in two_range_rows:
            out.append(dict(ranges=((w["hull"][0], w["gap"][0]), (w["gap"][1], w["hull"][1])), forced=-1, top_k=w["top_k"]))
        else:
            out.append(dict(ranges=(w["hull"],), forced=-1, top_k=w["top_k"]))
    return out


def hull_of(rule, V):
    return SE.rule_window(rule["ranges"], V)


# ------------------------------------------------------------------------------------------------ the branches, each from the source line it mirrors
def branches(chunks, slices, fold, window, rule, prows=32, min_cols=HEAD_COMBINE_MIN_COLS):
    """which way a row of this launch goes (csrc/sjd_sampling.hip unless noted)"""
    w = WINDOWS[window]
    V, (col0, col1) = w["V"], w["cols"]
    n_cols = col1 - col0
    row_stride, chunk_stride = n_cols, prows * n_cols                                # ops._head_partials
    wlo, whi = hull_of(rule, V)
    width = whi - (wlo & ~3)
    lds = SE.stage_lds_floats(n_cols + 8 + 2 * SE.SJD_DRAW_LIST)                     # :985  sjd_logits_to_probs_sample_part
    vec = V % 4 == 0 and row_stride % 4 == 0 and col0 % 4 == 0                       # :275
    groups = range(wlo & ~3, whi, 4)
    in4 = [vec and c0 >= col0 and c0 + 3 < col0 + n_cols and c0 + 3 < V for c0 in groups]      # :315
    fits = (width + 4 * SE.SJD_TPB - 1) // (4 * SE.SJD_TPB) <= SE.K2_NI              # :381
    in_lds = width <= lds                                                            # :294
    return dict(
        stats8=bool(fold) and slices <= 8,                                           # :202  the register-preloaded statistics; else k2_row_scales
        clamped=bool(fold) and slices < 8,                                           # :207  min(q, slices - 1) repeats the last slice
        second_batch=bool(fold) and slices > 8,                                      # :87   k2_row_scales' loop runs more than once
        planes_in_flight=chunks <= 8,                                                # :122 (K2a), :318 (K2); else the chunk loop
        vec=vec, in4_all=all(in4), in4_none=not any(in4),
        fits=fits, in_lds=in_lds, form="registers" if fits else "lds" if in_lds else "global",
        head_combine_ok=n_cols >= min_cols and n_cols % 4 == 0 and row_stride % 4 == 0 and chunk_stride % 4 == 0,       # ops.py head_combine_ok
        inside=col0 <= wlo and whi <= min(col1, V))                                  # the hull lies inside the head's columns


# ------------------------------------------------------------------------------------------------ builders
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ordered_rows(gen, chunks, n, ncol):
    """[chunks, n, ncol] fp32 whose sum depends on the ORDER of the chunks.  Odd columns: Gaussians whose chunk magnitudes run from 2^2 down to 2^-22
    (the plain case: the first chunk carries the value).  Even columns, from two chunks on, telescope: chunk 0 = A_0, chunk c = fp32(A_c - A_{c-1}) with
    |A_c| falling from 2^12 to 2^-1.  In chunk order every add cancels the previous level exactly and the sum keeps the fine bits of the last, small
    terms; in any order that meets the large chunks late those bits are lost against 2^12 (spacing 2^-11): another order gives other fp32 bits in most
    elements, and other 16-bit values after the rounding in a good share of them."""
    e = torch.linspace(12, -12, chunks) if chunks > 1 else torch.zeros(1)
    body = torch.randn(chunks, n, ncol, generator=gen) * torch.exp2(e - 10)[:, None, None]
    if chunks >= 2:
        half = body[:, :, 0::2].shape[-1]
        A = torch.randn(chunks, n, half, generator=gen) * torch.exp2(torch.linspace(12, -1, chunks))[:, None, None]
        body[0, :, 0::2] = A[0]
        body[1:, :, 0::2] = A[1:] - A[:-1]
    return body


# log2 of the mean square of the k-th live cond / uncond row (None: total ~ 0, eps decides the scale).  Spread over 2^+-2 from row to row; a cond row and
# its uncond row differ by 2^2 at least, so do neighbours, and so do the rows i of the two prompts of a shared head.
_G_COND = (-2.0, 0.0, None, 2.0, 0.0, 2.0, 0.0, -2.0)
_G_UNCOND = (0.0, 2.0, 1.0, -0.5, 2.0, 0.0, -2.0, 0.0)
EPS_ROW, EPS_ROW_PLANE_SCALE = 2, 3e-3          # cond row 2: r = eps^-1/2 = 316; its planes are scaled so that the logits stay O(1)


def stats_rows(gen, slices, hidden, g_list):
    """[slices, len(g_list)] fp32 per-slice sums of h^2: mean square 2^g per row, the later slices up to three times as heavy as the first (dropping
    slices 8.. is visible), a factor 0.75 .. 1.25 of noise per entry"""
    w = 1.0 + 2.0 * torch.arange(slices) / slices
    w = w / w.mean()
    out = torch.empty(slices, len(g_list))
    for k, g in enumerate(g_list):
        noise = 0.75 + 0.5 * torch.rand(slices, generator=gen)
        out[:, k] = noise * w * (hidden / slices) * (2.0 ** g if g is not None else 1e-12)
    return out


@functools.lru_cache(maxsize=2)
def inputs(shape, window, prompts=1, prows=32, urow_off=LMAX, n_rows=N_ROWS):
    """-> dict(planes [chunks, prows, n_cols] fp32, sumsq [slices, prows] fp32, hidden, chunks, slices, live: [(cond row, uncond row)] per prompt row).
    Prompt p's cond rows start at partial row p * LMAX, its uncond rows urow_off further.  Every other row of the planes and the statistics holds
    glue_models.PLANE_SENTINEL (finite: the clean run; the confinement test puts NaN and Inf there).  Treat as read-only (cached)."""
    chunks, slices, hidden = SHAPES[shape]
    w = WINDOWS[window]
    n_cols = w["cols"][1] - w["cols"][0]
    gen = _gen("head", shape, window, prompts, prows, urow_off, n_rows)
    cond = [p * LMAX + i for p in range(prompts) for i in range(n_rows)]
    unc = [r + urow_off for r in cond]
    assert max(unc) < prows and not set(cond) & set(unc)
    planes = torch.full((chunks, prows, n_cols), M.PLANE_SENTINEL, dtype=torch.float32)
    body = ordered_rows(gen, chunks, 2 * len(cond), n_cols)
    body[:, EPS_ROW] *= EPS_ROW_PLANE_SCALE
    planes[:, cond + unc] = body
    sumsq = torch.full((slices, prows), M.PLANE_SENTINEL, dtype=torch.float32)
    sumsq[:, cond] = stats_rows(gen, slices, hidden, [_G_COND[k % 8] for k in range(len(cond))])
    sumsq[:, unc] = stats_rows(gen, slices, hidden, [_G_UNCOND[k % 8] for k in range(len(cond))])
    return dict(planes=planes, sumsq=sumsq, hidden=hidden, chunks=chunks, slices=slices, n_cols=n_cols, col0=w["cols"][0], V=w["V"], cond=cond, unc=unc,
                urow_off=urow_off, prows=prows, n_rows=n_rows)


# ------------------------------------------------------------------------------------------------ the model
WRONG = ("reversed", "drop_first", "slices8", "ru_is_rc", "round_first")       # beside glue_models' plants "drop_plane", "neighbour_sumsq", "trunc", "eps10"


def model(inp, dtype, fold, row0=0, urow_off=None, n_rows=None, f=F64, plant=None, wrong=None):
    """the logits of the launch's rows as the front end must derive them -> dict(c, c_tol[, u, u_tol]), each [n_rows, n_cols] (values in `f`, tolerances
    fp64): glue_models.f2_source on partial rows row0 + i with those rows' statistics, and on rows row0 + urow_off + i for the uncond half.
    plant: one of glue_models.PLANTS; wrong: one of WRONG -- the chunk order reversed, chunk 0 never added, the statistics' slices 8.. dropped, the
    uncond row scaled by the cond row's statistics, the rounding applied before the scale (and again behind it)."""
    planes, ss = inp["planes"], inp["sumsq"]
    n = inp["n_rows"] if n_rows is None else n_rows
    uo = inp["urow_off"] if urow_off is None else urow_off
    if wrong == "reversed":
        planes = planes.flip(0)
    elif wrong == "drop_first":
        planes = planes[1:]
    elif wrong == "slices8":
        ss = ss[:8]
    out = {}
    for key, r0 in (("c", row0),) + ((("u", row0 + uo),) if uo > 0 else ()):
        s0 = row0 if wrong == "ru_is_rc" else r0
        rn = (ss[:, s0:s0 + n], inp["hidden"], EPS) if fold else None
        if wrong == "round_first" and fold:
            num = M._Num(dtype, f)
            x, tol = num.rnd(num.q(M.planes_sum(planes[:, r0:r0 + n])[:n].to(f)) * M.row_scale(*rn, n, num))
        else:
            x, tol = M.f2_source(dtype, planes=planes[:, r0:r0 + n], rows=n, row_norm=rn, f=f, plant=plant)
        out[key], out[key + "_tol"] = x, tol + torch.zeros(x.shape, dtype=F64)
    return out


def judge(got, ref, fold, dtype, cols=None):
    """the comparison of the GPU test, on dicts of [n_rows, n_cols] tensors (`cols`: per row the (lo, hi) column slice that is compared, relative to the
    tensors' column 0) -> (ok, share, worst).  Class A (no fold, or fp32): every bit -- share is the share of differing elements and must be 0.
    Class B: glue_models.class_b over everything compared: worst <= 1 and share <= SHARE_CAP."""
    g, m, t = [], [], []
    for key in ("c", "u"):
        if key not in ref:
            continue
        for i in range(ref[key].shape[0]):
            lo, hi = cols[i] if cols is not None else (0, ref[key].shape[1])
            g.append(got[key][i, lo:hi].to(F64))
            m.append(ref[key][i, lo:hi].to(F64))
            t.append(ref[key + "_tol"][i, lo:hi])
    g, m, t = torch.cat(g), torch.cat(m), torch.cat(t)
    if not fold or dtype == torch.float32:
        same = (g == m) & (g.signbit() == m.signbit()) | (torch.isnan(g) & torch.isnan(m))
        share = 1.0 - float(same.double().mean())
        return share == 0.0, share, 0.0 if share == 0.0 else float("inf")
    share, worst = M.class_b(g, m, t)
    return share <= M.SHARE_CAP and worst <= 1.0, share, worst


# ------------------------------------------------------------------------------------------------ ties: sums on a half-way point of the 16-bit grid
TIE_WINDOW = "image0"


def _half_away(x, dtype):
    """round to nearest, ties AWAY from zero (a wrong rounding the tie inputs must tell from nearest-even)"""
    lo = M._trunc(x, dtype)
    up = (lo.view(torch.int16) + 1).view(dtype)                   # sign-magnitude codes: one step away from zero (max + 1 = inf)
    a, l, u = x.to(F64).abs(), lo.to(F64).abs(), up.to(F64).abs()
    mx = float(torch.finfo(dtype).max)
    u = torch.where(torch.isinf(u), torch.full_like(u, mx + float(M.ulp(dtype, mx))), u)          # (the step behind max, as if the grid went on)
    return torch.where((a - l) >= (u - a), up, lo)


ROUNDINGS = dict(rne=lambda x, dt: x.to(dt), trunc=M._trunc, half_away=_half_away)


def tie_values(dtype):
    """-> (moderate [n, 2], extreme [m, 2]) fp32 pairs (hi, lo) whose fp32 sum is EXACT and sits on, one fp32 step above or one below a half-way point
    of `dtype`.  moderate: binades 2^-3 .. 2^5, the neighbours k, k + 1 of both parities at both ends of the binade (the last one rounds up into the
    next binade), both signs; and half-way points between fp16 SUBNORMALS (k 2^-24 + 2^-25: normal fp32 numbers).  extreme: the largest finite value
    itself, the tie below it, the last value that still rounds to it and the first that rounds to infinity (max + half a spacing), both signs."""
    m = M._MANT[dtype]
    rows = []
    for E in range(-3, 6):
        u, d = 2.0 ** (E - m), 2.0 ** (E - 23)
        for k in (2 ** m, 2 ** m + 1, 2 ** m + 2, 2 ** m + 3, 2 ** (m + 1) - 2, 2 ** (m + 1) - 1):
            for lo in (u / 2, u / 2 + d, u / 2 - d):
                rows += [(k * u, lo), (-k * u, -lo)]
    for k in (1, 2, 3, 1022, 1023):
        for lo in (2.0 ** -25, 2.0 ** -25 + 2.0 ** -38, 2.0 ** -25 - 2.0 ** -38):
            rows += [(k * 2.0 ** -24, lo), (-k * 2.0 ** -24, -lo)]
    mx = float(torch.finfo(dtype).max)
    u = float(M.ulp(dtype, mx))
    top = 2.0 ** (math.frexp(mx)[1] - 1)                          # the power of two of max's binade
    d = top * 2.0 ** -23
    ext = []
    for hi, lo in ((top, mx - top), (mx - u, u / 2), (mx, u / 2 - d), (mx, u / 2)):
        ext += [(hi, lo), (-hi, -lo)]
    mod, ext = torch.tensor(rows, dtype=F64), torch.tensor(ext, dtype=F64)
    for t in (mod, ext):
        assert torch.equal(t.to(torch.float32).to(F64), t) and torch.equal((t[:, 0].float() + t[:, 1].float()).to(F64), t.sum(1)), "a tie sum is not exact in fp32"
    return mod.float(), ext.float()


@functools.lru_cache(maxsize=2)
def tie_inputs(dtype, prows=32):
    """two chunks hi + lo over TIE_WINDOW: the moderate ties tile every column, rolled by another amount per row (cond and uncond rows differ); the
    extremes -- the largest finite value, the first that rounds to infinity -- go ONLY into the gap of the rows' two-range rule, inside the hull (the
    observers record them) but masked by the grammar (no infinite score reaches selection).  No fold."""
    w = WINDOWS[TIE_WINDOW]
    n_cols, col0 = w["cols"][1] - w["cols"][0], w["cols"][0]
    mod, ext = tie_values(dtype)
    cond, unc = list(range(N_ROWS)), [LMAX + i for i in range(N_ROWS)]
    planes = torch.full((2, prows, n_cols), M.PLANE_SENTINEL, dtype=torch.float32)
    g0, g1 = w["gap"][0] - col0, w["gap"][1] - col0
    for k, r in enumerate(cond + unc):
        idx = (torch.arange(n_cols) + 37 * k) % mod.shape[0]
        planes[:, r] = mod[idx].t()
        gi = (torch.arange(g1 - g0) + 3 * k) % ext.shape[0]
        planes[:, r, g0:g1] = ext[gi].t()
    sumsq = torch.full((1, prows), M.PLANE_SENTINEL, dtype=torch.float32)
    return dict(planes=planes, sumsq=sumsq, hidden=512, chunks=2, slices=1, n_cols=n_cols, col0=col0, V=w["V"], cond=cond, unc=unc, urow_off=LMAX,
                prows=prows, n_rows=N_ROWS, gap=(g0, g1))


# ------------------------------------------------------------------------------------------------ the real producer (G1 + F1r -> K2), on the exact grid
PRODUCER = dict(hidden=1024, KC=512, V=2080, chunks=2, slices=2, row_rng=(-4, 4), col_rng=(-12, -8))


@functools.lru_cache(maxsize=2)
def producer_inputs(dtype):
    """x [2 LMAX, hidden] and a head weight w [V, hidden] on gemm_exact_cases' exact grid: every split-K plane of x @ w.T and every per-slice sum of x^2 is
    exact in fp32, so the planes and statistics a correct G1 / F1r hands to K2 are known to the bit -> dict(x, w, planes fp32 [chunks, 2 LMAX, V] (exact),
    sumsq fp32 [slices, 2 LMAX] (exact))"""
    from tests import gemm_exact_cases as G
    P = PRODUCER
    rows = 2 * LMAX
    x, w = G.exact_operands(dtype, rows, P["V"], P["hidden"], 4242, G.spread_exps(rows, *P["row_rng"], 1), G.spread_exps(P["V"], *P["col_rng"], 2))
    planes64 = G.exact_planes(x, w, P["KC"])
    x2 = x.to(F64) ** 2
    ss64 = torch.stack([x2[:, s * 512:(s + 1) * 512].sum(-1) for s in range(P["slices"])])
    planes, sumsq = planes64.float(), ss64.float()
    assert torch.equal(planes.to(F64), planes64) and torch.equal(sumsq.to(F64), ss64) and torch.equal(M.planes_sum(planes).to(F64), planes64.sum(0))
    return dict(x=x, w=w, planes=planes, sumsq=sumsq, hidden=P["hidden"], chunks=P["chunks"], slices=P["slices"], n_cols=P["V"], col0=0, V=P["V"],
                cond=list(range(N_ROWS)), unc=[LMAX + i for i in range(N_ROWS)], urow_off=LMAX, prows=rows, n_rows=N_ROWS)
