"""Case tables, branch predicates and the definitional reference of the K2 / K4 selection-edge tests.

The sampling kernels (csrc/sjd_sampling.hip, csrc/sjd_device.h) branch on the DATA: how many scores share the value bin of the k-th largest,
whether that bin is the pooled bin 0, whether the k-th largest is tied, how many entries carry mass against the room of the in-kernel draw list.
Dense Gaussian fp32 logits reach none of these branches.  This module builds scores that do -- on power-of-two grids, so that ties survive the
CFG combine g * (c - u) + u exactly -- names the branch every row is built for, and restates in ONE place the kernel constants the predicates
need.  tests/test_sampling_edge_cases.py checks on the CPU that every row reaches its branch and that the oracle equals the definitional
reference below; tests/test_gpu_sampling_edges.py holds the kernels to the oracle on the same rows.  Nothing here touches the GPU or
libsjd_hip.so, and the oracle is only ever handed in by the caller.
"""
import zlib

import numpy as np

# ------------------------------------------------------------------------------------------------ the kernel's constants, restated once
SJD_TPB = 1024                          # csrc/sjd_device.h:13       threads per row; a column group is 4 * SJD_TPB columns
VALUE_BINS = 2048                       # csrc/sjd_device.h:15       SJD_RADIX_BINS: bins of block_kth_largest_spread's value histogram
BIN_SPAN = 32.0                         # csrc/sjd_device.h:440      the bins cover [zmax - 32, zmax]; everything below shares bin 0
RANK_CAP = 256                          # csrc/sjd_device.h:452      survivors the rank loop takes; more: the three radix passes
K2_NI = 3                               # csrc/sjd_sampling.hip:163  column groups K2 keeps in registers
SJD_DRAW_LIST = 2304                    # csrc/sjd_sampling.hip:922  draw-list entries the launchers ask LDS room for
STAGE_CAP_FLOATS = 150 * 1024 // 4      # csrc/sjd_sampling.hip:925  sjd_stage_lds_floats: 150 KiB of dynamic LDS at the most
EXP_CUT = -87.0                         # csrc/sjd_device.h:19       sjd_expf is 0 below -87


def stage_lds_floats(cols):
    """sjd_stage_lds_floats (csrc/sjd_sampling.hip:923-927)"""
    return (cols + 3) & ~3 if cols < STAGE_CAP_FLOATS else STAGE_CAP_FLOATS


def lds_floats(V):
    """what sjd_logits_to_probs_sample_ex / sjd_verify_accept_ex launch with (csrc/sjd_sampling.hip:963, 1016)"""
    return stage_lds_floats(V + 2 * SJD_DRAW_LIST)


def rule_window(ranges, V):
    """rule_window (csrc/sjd_sampling.hip:27-36): the hull of the allowed ranges"""
    if not ranges:
        return 0, V
    lo, hi = max(min(r[0] for r in ranges), 0), min(max(r[1] for r in ranges), V)
    return lo, max(hi, lo)


def staging(V, ranges, kernel="k2"):
    """where the row is staged and how many entries its draw list holds (K2: csrc/sjd_sampling.hip:286, 373, 479-482; K4: :707, 786-789)"""
    wlo, whi = rule_window(ranges, V)
    width = whi - (wlo & ~3)
    lds = lds_floats(V)
    in_lds = width <= lds
    fits = kernel == "k2" and (width + 4 * SJD_TPB - 1) // (4 * SJD_TPB) <= K2_NI
    assert in_lds or not fits
    list_base = ((width + 3) & ~3) if in_lds else 0
    list_cap = (lds - list_base) // 2
    return dict(wlo=wlo, whi=whi, form="registers" if fits else "lds" if in_lds else "global", list_cap=list_cap, compact=list_cap >= 64)


def bin_of(z, zmax):
    """bin_of in block_kth_largest_spread (csrc/sjd_device.h:440-441): min(max((z - (zmax - 32)) * (2047 / 32), 0), 2047), truncated, in fp32"""
    z = np.asarray(z, np.float32)
    lo = np.float32(zmax) - np.float32(BIN_SPAN)
    inv = np.float32(VALUE_BINS - 1) / np.float32(BIN_SPAN)
    x = (z - lo).astype(np.float32) * inv
    return np.minimum(np.maximum(x.astype(np.float32), np.float32(0)), np.float32(VALUE_BINS - 1)).astype(np.int64)


def allowed_mask(ranges, V):
    if not ranges:
        return np.ones(V, bool)
    m = np.zeros(V, bool)
    for lo, hi in ranges:
        m[max(lo, 0):min(hi, V)] = True
    return m


def combine(c, u, g):
    """the CFG combine as K2 and the oracle round it: three fp32 operations"""
    c, u = np.asarray(c, np.float32), np.asarray(u, np.float32)
    t = (c - u).astype(np.float32)
    t = (np.float32(g) * t).astype(np.float32)
    return (t + u).astype(np.float32)


def select_stats(z, rule, V):
    """Which branch of K2's top-k a row of combined scores reaches.  z: fp32 [V]; rule: dict(ranges, top_k, ...)."""
    zz = np.where(allowed_mask(rule.get("ranges", ()), V), np.asarray(z, np.float32), np.float32(-np.inf)).astype(np.float32)
    fin = zz > -np.inf
    n_finite, k = int(fin.sum()), int(rule.get("top_k", 0) or 0)
    st = dict(n_finite=n_finite, top_k=k, zmax=float(zz.max()), select=0 < k < V and k < n_finite, bsel=None, survivors=0, tie=0,
              kth=-np.inf, kept=n_finite, scores=zz)
    if st["select"]:
        b = bin_of(zz[fin], st["zmax"])
        hist = np.bincount(b, minlength=VALUE_BINS)
        above = np.cumsum(hist[::-1])[::-1]                   # scores in bins >= b
        bsel = int(np.flatnonzero(above >= k).max())            # (radix_pick: descending bins until k scores are covered)
        kth = np.sort(zz)[::-1][k - 1]
        assert bin_of(kth, st["zmax"]) == bsel
        st.update(bsel=bsel, survivors=int(hist[bsel]), kth=float(kth), tie=int((zz == kth).sum()), kept=int((zz >= kth).sum()))
    elif 0 < k < V:
        st["kth"] = -np.inf                                     # top_k >= n_finite: the kernel leaves kth at -inf, nothing is removed
    return st


# ------------------------------------------------------------------------------------------------ the definitional reference (fp64)
def _tie_cut(scores, weights, top_p):
    """the top-p rule under ties (csrc/sjd_device.h, block_top_p_cut_key): whole groups of equal score are removed in ascending order while
    the removed mass stays <= float32(1 - top_p).  -> (removed bool, dict of the figures the tests assert on)"""
    thr = float(np.float32(1.0 - float(top_p)))
    live = weights > 0
    p = weights / weights.sum()
    vals, inv = np.unique(scores[live], return_inverse=True)
    mass = np.bincount(inv, weights=p[live], minlength=len(vals))
    size = np.bincount(inv, minlength=len(vals))
    cum = np.cumsum(mass)
    n_rm = int((cum <= thr).sum())
    assert n_rm < len(vals), "the group of the maximum is never removed (thr < 1)"
    removed = np.zeros(scores.shape, bool)
    removed[np.flatnonzero(live)[inv < n_rm]] = True
    rm_mass = float(cum[n_rm - 1]) if n_rm else 0.0
    info = dict(thr=thr, removed_mass=rm_mass, next_mass=float(mass[n_rm]), margin_removed=thr - rm_mass,
                margin_next=rm_mass + float(mass[n_rm]) - thr, cut_group_sizes=(int(size[n_rm - 1]) if n_rm else 0, int(size[n_rm])),
                n_groups=len(vals))
    return removed, info


def reference_k2_row(z, rule, V):
    """HF semantics on one row of combined scores, in fp64: grammar mask, top-k keeps scores >= the k-th largest (ties kept), temperature,
    top-p by the tie rule, softmax.  -> dict(support, probs, kth, top_p info or None)"""
    zz = np.where(allowed_mask(rule.get("ranges", ()), V), np.asarray(z, np.float32), np.float32(-np.inf)).astype(np.float64)
    k = int(rule.get("top_k", 0) or 0)
    kth = -np.inf
    if 0 < k < V:
        kth = np.sort(zz)[::-1][k - 1]
        zz = np.where(zz < kth, -np.inf, zz)
    T = float(rule.get("temperature", 1.0) or 1.0)
    zt = zz / T if T != 1.0 else zz
    zmax = zt.max()
    # (the canonical exponential is exactly 0 below -87: part of the specification the oracle and the kernel share)
    w = np.where(zt - zmax >= EXP_CUT, np.exp(zt - zmax), 0.0)
    info = None
    if rule.get("top_p") is not None and rule["top_p"] < 1.0:
        removed, info = _tie_cut(zt, w, rule["top_p"])
        imax = int(np.argmax(w))                                # lowest index among the maxima: always kept
        removed[imax] = False
        w = np.where(removed, 0.0, w)
    return dict(support=w > 0, probs=w / w.sum(), kth=float(kth), top_p=info)


# ------------------------------------------------------------------------------------------------ score builders: fp32 [W] over the rule's window
def bf16_round(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def qgauss(sigma, step):
    """Gaussian scores rounded to multiples of `step`: runs of equal values everywhere"""
    def f(rng, W, ctx):
        return (np.round(rng.standard_normal(W) * (sigma / step)) * step + 0.0).astype(np.float32)       # (+ 0.0: no -0.0 from rounding)
    return f


def levels(step, per_level):
    """W // per_level equally likely score levels `step` apart: every run of equal scores is about per_level long, the top one included"""
    def f(rng, W, ctx):
        return (step * rng.integers(0, max(W // per_level, 8), W)).astype(np.float32)
    return f


def gauss(sigma):
    def f(rng, W, ctx):
        return (rng.standard_normal(W) * sigma).astype(np.float32)
    return f


def plateau(kept_of):
    """top_k - 100 scores above, then a run of equal scores that holds the k-th largest and brings the kept count to kept_of(ctx), the rest below"""
    def f(rng, W, ctx):
        k, kept = ctx["top_k"], int(kept_of(ctx))
        above = k - 100
        assert above > 0 and k < kept <= W
        z = np.empty(W, np.float32)
        perm = rng.permutation(W)
        z[perm[:above]] = 2.0 + 0.125 * rng.integers(1, 48, above)
        z[perm[above:kept]] = 2.0
        z[perm[kept:]] = 2.0 - 0.125 * rng.integers(1, 64, W - kept)
        return z
    return f


def signed_zero(rng, W, ctx):
    """a fine-grid row shifted so that its k-th largest is 0; the zeros alternate between +0.0 and -0.0 (equal floats, different radix keys)"""
    z = qgauss(3.0, 0.125)(rng, W, ctx)
    z = (z - np.sort(z)[::-1][ctx["top_k"] - 1]).astype(np.float32)
    zeros = np.flatnonzero(z == 0)
    z[zeros[1::2]] = np.float32(-0.0)
    return z


def bf16_with_minus_inf(n_finite_of):
    """bf16-rounded Gaussian logits of which only n_finite_of(ctx, W) are finite: -inf inside the allowed window"""
    def f(rng, W, ctx):
        z = bf16_round(rng.standard_normal(W).astype(np.float32) * np.float32(3.0))
        z[rng.permutation(W)[int(n_finite_of(ctx, W)):]] = -np.inf
        return z
    return f


# ------------------------------------------------------------------------------------------------ branch predicates over select_stats (+ oracle mass)
# n_mass = entries with probability > 0 = what K2 appends to its draw list (sh.misc[1]); list_cap from staging()
PREDICATES = {
    "select_runs": lambda s: s["select"],
    "rank_overflow": lambda s: s["select"] and s["survivors"] > RANK_CAP,                     # the radix fallback behind the rank loop
    "rank_loop_tie": lambda s: s["select"] and s["survivors"] <= RANK_CAP and s["tie"] > 1,    # "equal keys all write the same word"
    "radix_tie": lambda s: s["select"] and s["survivors"] > RANK_CAP and s["tie"] > 1,         # radix_pick with krem inside a run of equal keys
    "bin0": lambda s: s["select"] and s["bsel"] == 0,                                         # the k-th largest lies in the pooled bin
    "kept_gt_topk": lambda s: s["kept"] > s["top_k"] > 0,
    "list_full": lambda s: s["top_k"] < s["n_mass"] <= s["list_cap"],
    "list_brim": lambda s: s["n_mass"] == s["list_cap"],
    "list_overflow": lambda s: s["n_mass"] > s["list_cap"],
    "topk_eq_finite": lambda s: s["top_k"] == s["n_finite"] and not s["select"],
    "topk_gt_finite": lambda s: s["top_k"] > s["n_finite"] and not s["select"],
    "minus_inf_inside": lambda s: s["n_finite"] < s["window"],
    "signed_zero": lambda s: s["select"] and s["kth"] == 0.0 and len({bool(np.signbit(v)) for v in s["scores"][s["scores"] == 0]}) == 2,
    "top_p_tie": lambda s: s["top_p"] is not None and max(s["top_p"]["cut_group_sizes"]) > 1,
    "top_p_margin": lambda s: s["top_p"] is not None and min(s["top_p"]["margin_removed"], s["top_p"]["margin_next"]) >= 1e-4,
}

TOP_K = 2000
GUIDANCE = 3.0


def _row(build, expect, step=None, **rule):
    rule.setdefault("top_k", TOP_K)
    return dict(build=build, expect=tuple(expect), step=step, rule=rule)


def _case(name, cfg, rows):
    """cfg: "grid" -- the scores lie on the rows' power-of-two grid and are split into (c, u) with g * (c - u) + u exact in fp32;
    "raw" -- c and u are drawn independently by the row's builder and combined with the three roundings; "off" -- no CFG, c is the score"""
    assert cfg in ("grid", "raw", "off") and 4 <= len(rows) <= 8
    return dict(name=name, cfg=cfg, rows=rows)


_TOP_P_ROWS = [
    _row(levels(0.25, 341), ("top_p_tie", "top_p_margin"), 0.25, top_k=0, top_p=0.9),
    _row(levels(0.25, 341), ("top_p_tie", "top_p_margin"), 0.25, top_k=0, top_p=0.5),
    _row(levels(0.25, 341), ("top_p_tie", "top_p_margin", "kept_gt_topk"), 0.25, top_p=0.9),
    _row(levels(0.25, 341), ("top_p_tie", "top_p_margin", "kept_gt_topk"), 0.25, top_p=0.5),
    _row(levels(0.25, 341), ("top_p_tie", "top_p_margin", "kept_gt_topk"), 0.25, top_p=0.9, temperature=0.7),
]

# every selection case runs at the three staging forms of SELECTION_FORMS
K2_SELECTION_CASES = [
    _case("rank_overflow", "grid", [_row(qgauss(3.0, 1.0), ("rank_overflow", "radix_tie", "kept_gt_topk"), 1.0)] * 4),
    _case("bin0_gauss40", "raw", [_row(gauss(40.0), ("bin0", "rank_overflow"))] * 4),
    _case("bin0_grid", "grid", [_row(qgauss(20.0, 4.0), ("bin0", "rank_overflow", "radix_tie", "kept_gt_topk"), 4.0)] * 4),
    _case("ties_at_kth", "grid", [_row(qgauss(3.0, 0.125), ("rank_loop_tie", "kept_gt_topk", "list_full"), 0.125)] * 4),
    _case("signed_zero", "off", [_row(signed_zero, ("signed_zero", "rank_loop_tie", "kept_gt_topk"))] * 4),
    _case("topk_eq_finite", "off", [_row(bf16_with_minus_inf(lambda c, W: c["top_k"]), ("topk_eq_finite", "minus_inf_inside"))] * 4),
    _case("topk_gt_finite", "off", [_row(bf16_with_minus_inf(lambda c, W, j=j: c["top_k"] - 1 - 499 * j), ("topk_gt_finite", "minus_inf_inside"))
                                    for j in range(4)]),
    _case("minus_inf_inside", "off", [_row(bf16_with_minus_inf(lambda c, W: W // 2), ("select_runs", "minus_inf_inside")),
                                      _row(bf16_with_minus_inf(lambda c, W: c["top_k"] + 1), ("select_runs", "minus_inf_inside")),
                                      _row(bf16_with_minus_inf(lambda c, W: W - 1), ("select_runs", "minus_inf_inside")),
                                      _row(bf16_with_minus_inf(lambda c, W: W // 3), ("select_runs", "minus_inf_inside"))]),
    _case("top_p_ties", "grid", _TOP_P_ROWS),
]

# the draw list: kept counts on both sides of the list's capacity and AT it, reached through a tie at the k-th largest; run with both noise sources
K2_LIST_CASES = [
    _case("list_full", "grid", [_row(plateau(lambda c: c["list_cap"]), ("list_full", "list_brim", "radix_tie"), 0.125),
                                _row(plateau(lambda c: c["list_cap"] - 1), ("list_full", "radix_tie"), 0.125),
                                _row(plateau(lambda c: c["top_k"] + 7), ("list_full", "rank_loop_tie"), 0.125),
                                _row(plateau(lambda c: (c["top_k"] + c["list_cap"]) // 2), ("list_full", "kept_gt_topk"), 0.125)]),
    _case("list_overflow", "grid", [_row(plateau(lambda c: c["list_cap"] + 1), ("list_overflow", "radix_tie"), 0.125),
                                    _row(plateau(lambda c: c["list_cap"] + 64), ("list_overflow", "radix_tie"), 0.125),
                                    _row(plateau(lambda c: 2 * c["list_cap"]), ("list_overflow", "radix_tie"), 0.125),
                                    _row(plateau(lambda c: min(3 * c["list_cap"], c["window"] - 64)), ("list_overflow", "radix_tie"), 0.125),
                                    _row(plateau(lambda c: min(4 * c["list_cap"], c["window"] - 32)), ("list_overflow", "radix_tie"), 0.125),
                                    _row(plateau(lambda c: c["list_cap"]), ("list_brim",), 0.125)]),
]

# one row of each kind over Emu3's odd vocabulary: V % 4 == 2 (no 16-byte loads), the window starts and ends off a multiple of 4
K2_ODD_CASE = _case("odd_vocab_mixed", "grid", [
    _row(qgauss(3.0, 1.0), ("rank_overflow", "radix_tie"), 1.0),
    _row(qgauss(3.0, 0.125), ("rank_loop_tie", "kept_gt_topk"), 0.125),
    _row(qgauss(20.0, 4.0), ("bin0", "radix_tie"), 4.0),
    _row(plateau(lambda c: c["list_cap"]), ("list_brim",), 0.125),
    _row(plateau(lambda c: c["list_cap"] + 1), ("list_overflow",), 0.125),
    _TOP_P_ROWS[0], _TOP_P_ROWS[3], _TOP_P_ROWS[4]])

FORMS = {
    # name: (V, allowed ranges, the staging form K2 takes there)
    "registers": (9216, ((5, 8197),), "registers"),                 # 8192 columns, three column groups; wlo off a multiple of 4
    "lds": (36864, ((1026, 33794),), "lds"),                        # 32768 columns: too wide for registers, staged in the workgroup's LDS
    "lds_llamagen": (16384, (), "lds"),                             # LlamaGen's unruled row: the list holds exactly SJD_DRAW_LIST entries
    "global": (65536, (), "global"),                                # a whole text vocabulary: staged in probs_out
    "odd": (184622, ((151855, 184621),), "lds"),
}
SELECTION_FORMS = ("registers", "lds", "global")
LIST_FORMS = ("registers", "lds", "lds_llamagen", "global")


def build_k2(case, form):
    """-> dict(c, u [n, V] fp32, use_cfg, rules [n dicts], V, staging, z [n, V] the combined scores)"""
    V, ranges, want_form = FORMS[form]
    stg = staging(V, ranges)
    assert stg["form"] == want_form and stg["compact"], (form, stg)
    wlo, whi = stg["wlo"], stg["whi"]
    W, n = whi - wlo, len(case["rows"])
    c, u = np.empty((n, V), np.float32), np.empty((n, V), np.float32)
    rules = []
    for j, row in enumerate(case["rows"]):
        rng = np.random.default_rng(zlib.crc32(f"{case['name']}/{form}/{j}".encode()))
        rule = dict(row["rule"], ranges=ranges)
        ctx = dict(top_k=rule["top_k"], list_cap=stg["list_cap"], window=W)
        # outside the window: finite grid values ABOVE everything inside -- a kernel that read them would keep them
        if case["cfg"] == "raw":
            c[j], u[j] = gauss(40.0)(rng, V, ctx), gauss(40.0)(rng, V, ctx)
        else:
            z = np.full(V, 512.0, np.float32)
            z[wlo:whi] = row["build"](rng, W, ctx)
            if case["cfg"] == "off":
                c[j], u[j] = z, rng.standard_normal(V).astype(np.float32)          # (use_cfg = 0: never read)
            else:
                s = row["step"]
                t = rng.integers(-32, 33, V).astype(np.float64) * s               # c - u
                uu = z.astype(np.float64) - GUIDANCE * t
                c[j], u[j] = (uu + t).astype(np.float32), uu.astype(np.float32)
                assert np.abs(c[j]).max() < 1024 and np.abs(u[j]).max() < 1024
                assert np.array_equal(combine(c[j], u[j], GUIDANCE).view(np.uint32), z.view(np.uint32)), "the grid keeps the combine exact"
        rules.append(rule)
    use_cfg = case["cfg"] != "off"
    z = combine(c, u, GUIDANCE) if use_cfg else c.copy()
    return dict(c=c, u=u, use_cfg=use_cfg, rules=rules, V=V, staging=stg, z=z, name=f"{case['name']}@{form}")


def row_stats(built, j, probs_row=None):
    """select_stats of row j + what the predicates need beside it (n_mass from the oracle's probabilities, when given)"""
    rule, V, stg = built["rules"][j], built["V"], built["staging"]
    st = select_stats(built["z"][j], rule, V)
    ref = reference_k2_row(built["z"][j], rule, V)
    st.update(window=stg["whi"] - stg["wlo"], list_cap=stg["list_cap"], top_p=ref["top_p"], ref=ref,
              n_mass=int((probs_row > 0).sum()) if probs_row is not None else int(ref["support"].sum()))
    return st


def describe(st):
    """the record of what ran: one line per row"""
    return (f"n_finite {st['n_finite']} top_k {st['top_k']} select {int(st['select'])} bin {st['bsel']} survivors {st['survivors']} "
            f"tie {st['tie']} kept {st['kept']} n_mass {st['n_mass']} list_cap {st['list_cap']}"
            + (f" top_p removed {st['top_p']['removed_mass']:.6f} thr {st['top_p']['thr']:.6f} next {st['top_p']['next_mass']:.6f} "
               f"groups {st['top_p']['cut_group_sizes']}" if st["top_p"] else ""))


def k2_params():
    out = [(c, f) for c in K2_SELECTION_CASES for f in SELECTION_FORMS]
    out += [(c, f) for c in K2_LIST_CASES for f in LIST_FORMS]
    return out + [(K2_ODD_CASE, "odd")]


# ------------------------------------------------------------------------------------------------ K4: target / draft rows with runs of equal values
K4_N = 6                 # window rows
K4_REJECT = 3            # the first rejected draft: the residual resample runs on row K4_REJECT - 1
K4_SHAPES = {
    # V: (ranges of the target rows' K2 rule -- a hole no target row has mass in --, the hole, residual staging)
    9216: (((5, 4000), (4100, 8195)), (4000, 4100), "lds"),
    65536: (((0, 30000), (30100, 65536)), (30000, 30100), "global"),
}


def k4_scores(V):
    """score rows of the target (zp) and the draft (zq) distributions: coarse grids, the draft a perturbed copy of the previous target row"""
    rng = np.random.default_rng(4000 + V)
    zp = (np.round(rng.standard_normal((K4_N, V)) * 6.0) * 0.5).astype(np.float32)
    zq = (np.roll(zp, 1, 0) + np.round(rng.standard_normal((K4_N, V)) * 2.0) * 0.5).astype(np.float32)
    return zp, zq


def k4_rules(V):
    ranges, hole, _ = K4_SHAPES[V]
    return dict(ranges=ranges, top_k=TOP_K), dict(ranges=((ranges[0][0], ranges[-1][1]),), top_k=TOP_K)


_K4_PQ = {}


def k4_pq(V, O):
    """target rows p and draft rows q [K4_N, V]: the oracle's (O = oracle.sjd_oracle) K2 probabilities of the tied-score rows above -- genuine
    normalised rows with runs of equal values and exact zeros.  Computed once per V, never written."""
    if V not in _K4_PQ:
        zp, zq = k4_scores(V)
        rp, rq = k4_rules(V)
        ones = np.ones_like(zp)
        _, p = O.logits_to_probs_sample(zp, None, 1.0, [O.rule(**rp)] * K4_N, ones)
        _, q = O.logits_to_probs_sample(zq, None, 1.0, [O.rule(**rq)] * K4_N, ones)
        _K4_PQ[V] = (p, q)
    return _K4_PQ[V]


def residual(p_row, q_row, ranges, V):
    """d = max(p - q, 0) in fp32 under the rule's ranges"""
    d = np.maximum((np.asarray(p_row, np.float32) - np.asarray(q_row, np.float32)).astype(np.float32), np.float32(0))
    return np.where(allowed_mask(ranges, V), d, np.float32(0)).astype(np.float32)


def _tied_rank(d):
    """a top_k whose k-th largest of d is tied: the most frequent positive value with at least ten values above it"""
    vals, counts = np.unique(d[d > 0], return_counts=True)
    above = len(d[d > 0]) - np.cumsum(counts)                    # values strictly above vals[i]
    ok = np.flatnonzero((counts > 1) & (above >= 10))
    i = ok[np.argmax(counts[ok])]
    return int(above[i]) + 1 + int(counts[i]) // 2               # inside the run


# name -> (rule kwargs as a function of (d, n_pos), tags).  The rules' ranges are () (added by k4_residual_rule: the V-wide window)
K4_RESIDUAL_RULES = {
    "topk_tie": (lambda d, n_pos: dict(top_k=_tied_rank(d)), ("k4_topk_tie",)),
    "topk_eq_npos": (lambda d, n_pos: dict(top_k=n_pos), ("k4_topk_eq_npos",)),
    "topk_gt_npos": (lambda d, n_pos: dict(top_k=n_pos + 7), ("k4_topk_gt_npos",)),
    "top_p_tied": (lambda d, n_pos: dict(top_p=0.9), ("k4_top_p_tie",)),
    "topk_top_p": (lambda d, n_pos: dict(top_k=_tied_rank(d), top_p=0.9), ("k4_topk_tie", "k4_top_p_tie")),
    "T0.7": (lambda d, n_pos: dict(top_k=_tied_rank(d), temperature=0.7), ("k4_topk_tie",)),
}


def residual_stats(d, rule, V):
    """which branch of K4's residual resample the weights d reach under `rule`"""
    n_pos, k = int((d > 0).sum()), int(rule.get("top_k", 0) or 0)
    st = dict(n_pos=n_pos, top_k=k, select=0 < k < V and k < n_pos, tie=0, kept=n_pos, top_p=None)
    w = d.astype(np.float64)
    if st["select"]:
        kth = np.sort(d)[::-1][k - 1]
        st.update(kth=float(kth), tie=int((d == kth).sum()), kept=int((d >= kth).sum()))
        w = np.where(d < kth, 0.0, w)
    if rule.get("top_p") is not None and w.sum() > 0:
        _, st["top_p"] = _tie_cut(w, w, rule["top_p"])
    return st


K4_PREDICATES = {
    "k4_topk_tie": lambda s: s["select"] and s["tie"] > 1 and s["kept"] > s["top_k"],
    "k4_topk_eq_npos": lambda s: s["top_k"] == s["n_pos"] and not s["select"],
    "k4_topk_gt_npos": lambda s: s["top_k"] > s["n_pos"] > 0 and not s["select"],
    "k4_top_p_tie": lambda s: s["top_p"] is not None and max(s["top_p"]["cut_group_sizes"]) > 1
    and min(s["top_p"]["margin_removed"], s["top_p"]["margin_next"]) >= 1e-4,
}
