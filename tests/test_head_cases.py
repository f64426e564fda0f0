"""CPU: the inputs and the model of tests/head_cases.py.  tests/test_gpu_head_exact.py rests on them, so here
  * the shape table is what launch_shapes and the backbones' hidden sizes give, and both axes hold every branch edge;
  * every input reaches the branch it is named for -- the predicates restate stats8, n_chunks <= 8, vec, in4, fits, in_lds and head_combine_ok, each
    from the source line it mirrors;
  * the ordered planes give other bits in another chunk order, the statistics separate a row from its neighbour, its uncond row and its clamped self;
  * the tie inputs round differently under nearest-even, truncation and round-half-away;
  * the fp32 emulation of the model stays inside its own tolerance and under the 1 % cap on every folded case -- the cap is met by the reference alone;
  * every wrong model (the last plane dropped, chunk 0 dropped, the chunk order reversed, the slices clamped at eight, the uncond row scaled by the cond
    row's statistics, a neighbour's statistics, the rounding in front of the scale, truncation, eps x 10) is REJECTED by the comparison the GPU test uses."""
import pytest
import torch

from tests import glue_models as M
from tests import head_cases as H

F32 = torch.float32
DT16 = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


def _cols(inp, rules):
    """per row the hull of its rule, as a column slice of the head's window"""
    return [tuple(c - inp["col0"] for c in H.hull_of(r, inp["V"])) for r in rules]


def test_shape_table_restates_the_product():
    import sjd_amd.launch_shapes as LS
    for name, (src, hidden) in H.PRODUCT_SOURCE.items():
        kc = getattr(LS, src)[0] if isinstance(src, str) else LS.LLAMAGEN_SETS[src][1][0]
        assert H.PRODUCT[name] == (-(-hidden // kc), -(-hidden // 512), hidden), (name, kc)
    assert {c for c, _, _ in H.SHAPES.values()} >= set(H.CHUNK_AXIS) and {s for _, s, _ in H.SHAPES.values()} >= set(H.SLICE_AXIS)
    used = {s for s, _ in H.CASES}
    assert used == set(H.SHAPES), "a shape of the table is never run"
    assert {w for _, w in H.CASES} == set(H.WINDOWS)
    by_window = {w: {H.SHAPES[s][:2] for s, ww in H.CASES if ww == w} for w in H.WINDOWS}
    assert (2, 8) in by_window["emu3"] and (4, 8) in by_window["image0"] and (8, 16) in by_window["image0"] and (4, 8) in by_window["text"]
    # the Emu3 vocabulary's scalar branch at more than one chunk count, on both sides of the chunk loop's threshold
    assert {c for c, _ in by_window["emu3"]} >= {2, 4, 8, 9}


def test_every_case_reaches_its_branches():
    seen = dict(stats8=set(), clamped=set(), second_batch=set(), planes_in_flight=set())
    for shape, window in H.CASES:
        chunks, slices, _ = H.SHAPES[shape]
        w = H.WINDOWS[window]
        for i, rule in enumerate(H.rules_of(window)):
            b = H.branches(chunks, slices, True, window, rule)
            assert b["inside"], (shape, window, i)
            assert b["form"] == w["form"], (shape, window, i, b)
            if window == "emu3":            # V % 4 = 2: no float4 anywhere in K2's own pass; the head is wide enough for K2a by default
                assert not b["vec"] and b["in4_none"] and b["head_combine_ok"]
            else:
                assert b["vec"] and b["in4_all"]
                assert b["head_combine_ok"] == (window == "text_wide")
            assert H.branches(chunks, slices, True, window, rule, min_cols=4)["head_combine_ok"], "the K2a route can be forced"
            assert not H.branches(chunks, slices, True, window, rule, min_cols=1 << 30)["head_combine_ok"]
            assert b["stats8"] == (slices <= 8) and b["second_batch"] == (slices > 8) and b["planes_in_flight"] == (chunks <= 8)
            assert not H.branches(chunks, slices, False, window, rule)["stats8"]
        print(f"{shape:>16} on {window:<9}: chunks {chunks:2d} ({'in flight' if b['planes_in_flight'] else 'loop'}), slices {slices:2d} "
              f"({'stats8' + (', clamped' if b['clamped'] else '') if b['stats8'] else 'k2_row_scales, two batches'}), "
              f"{'float4' if b['in4_all'] else 'scalar'} loads, staged in {b['form']}, K2a by default: {b['head_combine_ok']}")
        for k in seen:
            seen[k].add((window, b[k]))
    for window in ("image0", "emu3"):        # both sides of every threshold on the register form and on the scalar / LDS form
        for k in ("stats8", "clamped", "planes_in_flight"):
            assert {(window, True), (window, False)} <= seen[k], (window, k)
    assert {w for w, v in seen["second_batch"] if v} >= {"image0", "image992", "emu3", "text"}
    assert ("text_wide", False) in seen["planes_in_flight"] and ("text_wide", True) in seen["planes_in_flight"]


def test_ordered_planes_give_other_bits_in_another_order():
    for shape in H.SHAPES:
        inp = H.inputs(shape, "image0")
        live = inp["cond"] + inp["unc"]
        fwd, rev = M.planes_sum(inp["planes"][:, live]), M.planes_sum(inp["planes"][:, live].flip(0))
        share = float((fwd != rev).double().mean())
        print(f"{shape}: {inp['chunks']} chunks, reversed order changes {share:.3f} of the fp32 sums")
        if inp["chunks"] >= 3:              # (a + b = b + a: one or two chunks have no order)
            assert share >= 0.25, shape
        else:
            assert share == 0.0
        mag = inp["planes"][:, live][:, :, 1::2].abs().amax((1, 2))          # the plain columns: per chunk
        if inp["chunks"] > 1:
            assert float(mag.max() / mag.min()) > 2.0 ** 20
        assert torch.isfinite(fwd).all() and float(fwd.abs().max()) < 64.0          # logits of sane size: r <= 2 keeps them inside fp16


def test_statistics_separate_the_rows():
    for shape in H.SHAPES:
        for prompts, prows, uo in ((1, 32, H.LMAX), (2, 64, 32)):
            inp = H.inputs(shape, "image0", prompts, prows, uo)
            tot = inp["sumsq"].double().sum(0) / inp["hidden"]
            c, u = tot[inp["cond"]], tot[inp["unc"]]
            ratio = torch.maximum(c / u, u / c)
            assert float(ratio.min()) >= 2.0, (shape, ratio)
            assert float(c[H.EPS_ROW]) < H.EPS * 1e-3                                 # eps decides this row's scale
            other = torch.cat((c[:H.EPS_ROW], c[H.EPS_ROW + 1:]))
            assert 2.0 ** -2.5 < float(other.min()) and float(other.max()) < 2.0 ** 2.5
            nb = torch.maximum(c[1:] / c[:-1], c[:-1] / c[1:])
            assert float(nb.min()) >= 2.0                                           # a neighbour's statistics are far off
            if prompts == 2:                                                        # ... and so are those of the same row of the other prompt
                a, b = c[:H.N_ROWS], c[H.N_ROWS:]
                assert float(torch.maximum(a / b, b / a).min()) >= 1.9
            if inp["slices"] > 8:
                live = inp["cond"] + inp["unc"]
                late = inp["sumsq"][8:, live].double().sum(0) / inp["sumsq"][:, live].double().sum(0)
                # (nine slices: the one late slice is a seventh of the total, r moves by 7 %, dozens of 16-bit spacings)
                assert float(late.min()) > (0.4 if inp["slices"] == 16 else 0.1), "slices 8.. carry too little to be missed"


@pytest.mark.parametrize("dtype", DT16, ids=IDS)
def test_tie_inputs_tell_the_roundings_apart(dtype):
    mod, ext = H.tie_values(dtype)
    both = torch.cat((mod, ext))
    s = both[:, 0] + both[:, 1]                                                     # exact (tie_values asserts it)
    r = {k: f(s, dtype) for k, f in H.ROUNDINGS.items()}
    for a, b in (("rne", "trunc"), ("rne", "half_away"), ("trunc", "half_away")):
        n = int((r[a].view(torch.int16) != r[b].view(torch.int16)).sum())
        print(f"{dtype}: {a} and {b} differ on {n} of {s.numel()} tie sums")
        assert n >= 20
    lo, up = M._trunc(s, dtype).double(), H._half_away(s, dtype).double()
    fin = torch.isfinite(up)
    on_tie = fin & ((s.double() - lo).abs() == (up - s.double()).abs()) & (lo != up)
    even = (r["rne"].view(torch.int16) & 1) == 0
    assert int(on_tie.sum()) >= 100 and bool(even[on_tie].all()), "nearest-even lands on an even code on every tie"
    assert bool((on_tie & (r["rne"].double() == lo)).any()) and bool((on_tie & (r["rne"].double() == up)).any()), "ties of both parities"
    tiny = float(torch.finfo(torch.float16).tiny)
    assert bool(((s.abs() < tiny) & (s != 0)).any()), "a half-way point between fp16 subnormals"
    mx = float(torch.finfo(dtype).max)
    e = ext[:, 0] + ext[:, 1]
    re = e.to(dtype).double()
    assert bool((re == mx).any()) and bool((re == -mx).any()) and bool(torch.isinf(re).any()) and bool(torch.isfinite(e).all())
    assert float(e[torch.isinf(re)].abs().min()) == mx + float(M.ulp(dtype, mx)) / 2, "the FIRST value that rounds to infinity"
    # the planes: infinities only in the gap of the two-range rule, which every row has; what the grammar lets through combines to finite scores
    inp = H.tie_inputs(dtype)
    rules = H.rules_of(H.TIE_WINDOW, two_range_rows=range(H.N_ROWS))
    m = H.model(inp, dtype, False)
    g0, g1 = inp["gap"]
    for i, rule in enumerate(rules):
        lo_c, hi_c = _cols(inp, [rule])[0]
        allowed = torch.zeros(inp["n_cols"], dtype=torch.bool)
        for a, b in rule["ranges"]:
            allowed[a - inp["col0"]:b - inp["col0"]] = True
        assert not allowed[g0:g1].any() and lo_c <= g0 and g1 <= hi_c
        c, u = m["c"][i].float(), m["u"][i].float()
        assert bool(torch.isinf(c[g0:g1]).any()) and bool(torch.isfinite(c[allowed]).all()) and bool(torch.isfinite(u[allowed]).all())
        z = H.GUIDANCE * (c - u) + u
        assert bool(torch.isfinite(z[allowed]).all()) and float(z[allowed].abs().max()) < 1e3
        assert not torch.equal(c, u)
    assert torch.equal(m["c"].to(dtype).view(torch.int16), M.planes_sum(inp["planes"])[:H.N_ROWS].to(dtype).view(torch.int16))
    for name in ("trunc", "half_away"):          # either wrong rounding shows in the observers' comparison
        bad = {k: H.ROUNDINGS[name](M.planes_sum(inp["planes"])[r0:r0 + H.N_ROWS], dtype).double() for k, r0 in (("c", 0), ("u", H.LMAX))}
        assert not H.judge(bad, m, False, dtype, _cols(inp, rules))[0], name


def test_class_a_comparison_is_on_bits():
    ref = dict(c=torch.tensor([[0.0, 1.0, float("inf")]], dtype=torch.float64), c_tol=torch.zeros(1, 3, dtype=torch.float64))
    assert H.judge(dict(c=ref["c"].clone()), ref, False, torch.bfloat16)[0]
    assert not H.judge(dict(c=torch.tensor([[-0.0, 1.0, float("inf")]], dtype=torch.float64)), ref, False, torch.bfloat16)[0]
    assert not H.judge(dict(c=torch.tensor([[0.0, 1.0, float("nan")]], dtype=torch.float64)), ref, False, torch.bfloat16)[0]
    assert not H.judge(dict(c=torch.tensor([[0.0, 1.0, 3e38]], dtype=torch.float64)), ref, True, torch.float32)[0]


@pytest.mark.parametrize("dtype", DT16, ids=IDS)
def test_fp32_emulation_stays_inside_the_model(dtype):
    """the cap and the bound are met by the reference alone: a kernel that computes the same formula in fp32 passes on EVERY case"""
    worst_share = worst_ratio = 0.0
    for shape, window in H.CASES:
        inp = H.inputs(shape, window)
        cols = _cols(inp, H.rules_of(window))
        ref, emu = H.model(inp, dtype, True), H.model(inp, dtype, True, f=F32)
        ok, share, worst = H.judge(emu, ref, True, dtype, cols)
        assert ok, (shape, window, share, worst)
        worst_share, worst_ratio = max(worst_share, share), max(worst_ratio, worst)
        for dt, fold in ((dtype, False), (F32, False)):                 # class A: the same bits in either precision
            assert H.judge(H.model(inp, dt, fold, f=F32), H.model(inp, dt, fold), fold, dt, cols)[0], (shape, window, dt)
    print(f"\n{dtype}: fp32 emulation over {len(H.CASES)} cases: largest share {worst_share:.5f}, largest error / bound {worst_ratio:.3f}")
    inp = H.inputs("lumina7b", "image0", 2, 64, 32)                         # the shared head of two prompts
    assert H.judge(H.model(inp, dtype, True, row0=H.LMAX, f=F32), H.model(inp, dtype, True, row0=H.LMAX), True, dtype)[0]


# wrong model -> (keyword of head_cases.model, the forms it can show in: True = needs the fold, None = any, the chunk counts it needs)
_WRONG = dict(drop_plane=("plant", None, 2), drop_first=("wrong", None, 2), reversed=("wrong", None, 3), slices8=("wrong", True, 1),
              ru_is_rc=("wrong", True, 1), neighbour_sumsq=("plant", True, 1), round_first=("wrong", True, 1), trunc=("plant", None, 1),
              eps10=("plant", True, 1))


@pytest.mark.parametrize("dtype", DT16, ids=IDS)
def test_every_wrong_model_is_rejected(dtype):
    """each of the wrong models -- an fp32 emulation with ONE defect -- fails the GPU test's comparison, with a fold (class B) and, where the defect does
    not live in the fold, without one (class A).  Printed: on how many of the shapes of the first window."""
    shapes = [s for s, w in H.CASES if w == "image0"]
    for name, (kw, needs_fold, min_chunks) in _WRONG.items():
        for fold in ((True,) if needs_fold else (True, False)):
            caught, could = [], []
            for shape in shapes:
                inp = H.inputs(shape, "image0")
                if inp["chunks"] < min_chunks or (name == "slices8" and inp["slices"] <= 8):
                    continue
                cols = _cols(inp, H.rules_of("image0"))
                ref = H.model(inp, dtype, fold)
                bad = H.model(inp, dtype, fold, f=F32, **{kw: name})
                could.append(shape)
                if not H.judge(bad, ref, fold, dtype, cols)[0]:
                    caught.append(shape)
            print(f"{dtype} fold {fold}: wrong model {name}: rejected on {len(caught)} of {len(could)} shapes")
            assert could and caught == could, (name, fold, sorted(set(could) - set(caught)))
    # row0: the rows of the OTHER prompt of a shared head (planes and statistics of row i instead of row row0 + i) are rejected as well
    inp = H.inputs("lumina7b", "image0", 2, 64, 32)
    ref = H.model(inp, dtype, True, row0=H.LMAX)
    assert not H.judge(H.model(inp, dtype, True, row0=0, f=F32), ref, True, dtype)[0]
    mixed = H.model(inp, dtype, True, row0=H.LMAX, f=F32)                  # ... and so are the right planes under the other prompt's statistics
    r_oth = M.row_scale(inp["sumsq"][:, :H.N_ROWS], inp["hidden"], H.EPS, H.N_ROWS, M._Num(dtype, F32))
    mixed["c"] = (M.planes_sum(inp["planes"][:, H.LMAX:H.LMAX + H.N_ROWS]) * r_oth).to(dtype).float()
    assert not H.judge(mixed, ref, True, dtype)[0]


def test_producer_inputs_are_exact():
    for dtype in DT16:
        p = H.producer_inputs(dtype)
        assert p["planes"].shape == (2, 2 * H.LMAX, 2080) and p["sumsq"].shape == (2, 2 * H.LMAX)
        m = H.model(p, dtype, True)
        r = 1.0 / torch.sqrt(p["sumsq"].double().sum(0) / p["hidden"] + H.EPS)
        want = (r[:H.N_ROWS, None] * (p["x"].double() @ p["w"].double().t())[:H.N_ROWS]).to(dtype)       # dtype(r * exact x @ w.T)
        assert torch.equal(m["c"].to(dtype).view(torch.int16), want.view(torch.int16))
        assert 0.05 < float(m["c"].abs().mean()) < 64 and torch.isfinite(m["c"]).all()
        ok, share, worst = H.judge(H.model(p, dtype, True, f=F32), m, True, dtype)
        assert ok, (share, worst)
