"""GPU: K2's output-head front end -- k2_logits_to_probs_sample<PART>, k2_row_scale(s), k2_round16, k2a_head_combine (csrc/sjd_sampling.hip) -- against
the fp64 model of tests/head_cases.py (glue_models.f2_source) at every (chunks, slices) pair the product runs and at the edges of every branch.

Every launch goes through ops.logits_to_probs_sample_part with the `dbg` observers, a float guidance of 3.0 and tensor noise, once with K2 reading the
planes itself and once through K2a (ops._HEAD_COMBINE_MIN_COLS forced either way).
  (a) the observed logits over the hull of every row against the model: bit for bit without a fold and with fp32 "rounding" (class A), inside
      f2_source's tolerance with at most glue_models.SHARE_CAP of the elements off the model with a fold (class B); the two routes identical in
      observers, probabilities and tokens
  (b) the dense K2, fed with the observed logits, gives the same probabilities and tokens: the rest of K2 is untouched by the front end
  (c) sums on half-way points of the 16-bit grids, the largest finite value and the first that rounds to infinity, bit for bit
  (d) use_cfg = 0 beside an uncond row, urow_off = 0, row0 = 8 on a head two prompts share
  (e) NaN / Inf in everything the launch must not use; rows >= n_rows and the guard zones keep their poison
  (f) the real producer: G1 planes and F1r statistics of operands on the exact grid -> dtype(r * exact x @ w.T)
tests/test_head_cases.py shows on the CPU that every input reaches its branch and that the comparisons reject each wrong front end.
Every test prints its figures: the log is the record."""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sjd_oracle as O
from tests import glue_models as M
from tests import head_cases as H
from tests.test_gpu_kernels import _ops, to_dev_rule

SENT = M.PLANE_SENTINEL                 # what the observers and the pad rows hold before a launch
TOK_POISON, PROBS_FILL = -5, -7.0
ROUTES = ("k2", "k2a")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@contextlib.contextmanager
def _route(ops, route):
    """K2 reading the planes itself, or K2a then K2 over one plane: ops.head_combine_ok decides by this width"""
    was = ops._HEAD_COMBINE_MIN_COLS
    ops._HEAD_COMBINE_MIN_COLS = 4 if route == "k2a" else 1 << 30
    try:
        yield
    finally:
        ops._HEAD_COMBINE_MIN_COLS = was


def _params(dev, rules, n_rows, use_cfg):
    ops, L = _ops()
    params = ops.DeviceBlob(L.IterParams, dev)
    params.view.n_rows, params.view.use_cfg = n_rows, int(use_cfg)
    for j, r in enumerate(rules):
        params.view.rules[j] = to_dev_rule(L, ops, O.rule(**r))
    params.upload()
    return params


def _noise(dev, V, seed):
    return torch.empty(H.LMAX, V).exponential_(generator=torch.Generator().manual_seed(seed)).clamp_(min=1e-30).to(dev)


class _Out:
    """probs_out [LMAX, V] and the token buffer [LMAX] between guard zones, the observers [2, LMAX, V]; everything poisoned before the launch"""

    def __init__(self, dev, V, probs_fill=PROBS_FILL):
        self.g = V
        self.pbuf = torch.full((2 * self.g + H.LMAX * V,), probs_fill, dtype=torch.float32, device=dev)
        self.tbuf = torch.full((3 * H.LMAX,), TOK_POISON, dtype=torch.int64, device=dev)
        self.probs = self.pbuf[self.g:self.g + H.LMAX * V].view(H.LMAX, V)
        self.toks = self.tbuf[H.LMAX:2 * H.LMAX]
        self.dbg = torch.full((2, H.LMAX, V), SENT, dtype=torch.float32, device=dev)
        self.fill = torch.tensor(probs_fill, dtype=torch.float32).view(torch.int32).item()

    def kept(self, t):
        return bool((t.contiguous().view(torch.int32) == self.fill).all())

    def problems(self, n):
        """[] when the launch wrote nothing but rows < n: guard zones, rows >= n of the probabilities, the tokens and the observers"""
        bad = []
        if not (self.kept(self.pbuf[:self.g]) and self.kept(self.pbuf[self.g + self.probs.numel():])):
            bad.append("a guard zone of probs_out was written")
        if not self.kept(self.probs[n:]):
            bad.append(f"rows >= {n} of probs_out were written")
        if not (bool((self.tbuf[:H.LMAX] == TOK_POISON).all()) and bool((self.tbuf[2 * H.LMAX:] == TOK_POISON).all())):
            bad.append("a guard zone of the token buffer was written")
        if not bool((self.toks[n:] == TOK_POISON).all()):
            bad.append(f"tokens of rows >= {n} were written")
        if not bool((self.dbg[:, n:] == SENT).all()):
            bad.append(f"observers of rows >= {n} were written")
        return bad


def _launch(dev, inp, planes, sumsq, dtype, fold, params, noise, route, *, urow_off=None, row0=0, probs_fill=PROBS_FILL):
    ops, L = _ops()
    part = ops.Partials(planes, inp["chunks"], inp["n_cols"])
    head = ops.HeadOut(part, inp["col0"], inp["urow_off"] if urow_off is None else urow_off, dtype,
                       row_norm=(sumsq, inp["hidden"], H.EPS) if fold else None)
    out = _Out(dev, inp["V"], probs_fill)
    with _route(ops, route):
        took_k2a = ops.head_combine_ok(ops._head_partials(head, H.LMAX, inp["V"], dev, None, row0, None))
        ops.logits_to_probs_sample_part(head, H.GUIDANCE, params, noise, out.probs, ctypes.c_void_p(out.toks.data_ptr()), dbg=out.dbg, row0=row0)
    torch.cuda.synchronize()
    assert took_k2a == (route == "k2a"), "the route could not be forced"
    return out


def _observed(out, inp, n, both=True):
    """the observers' columns of the head's window (as far as V reaches), rows < n, on the CPU"""
    c0, c1 = inp["col0"], min(inp["col0"] + inp["n_cols"], inp["V"])
    got = dict(c=out.dbg[0, :n, c0:c1].cpu())
    if both:
        got["u"] = out.dbg[1, :n, c0:c1].cpu()
    return got


def _cols(inp, rules):
    return [tuple(c - inp["col0"] for c in H.hull_of(r, inp["V"])) if r["forced"] < 0 else (0, 0) for r in rules]


def _same(a, b, inp, rules, n, both=True, observers=True):
    """observers over every hull, probabilities and tokens of rows < n of two launches: the same bits -> list of what differs"""
    bad = []
    for i, (lo, hi) in enumerate(_cols(inp, rules) if observers else ()):
        lo, hi = lo + inp["col0"], hi + inp["col0"]
        for k in range(2 if both else 1):
            if not torch.equal(a.dbg[k, i, lo:hi].view(torch.int32), b.dbg[k, i, lo:hi].view(torch.int32)):
                bad.append(f"observer {k} of row {i}")
    if not torch.equal(a.probs[:n].view(torch.int32), b.probs[:n].view(torch.int32)):
        bad.append(f"probabilities ({int((a.probs[:n].view(torch.int32) != b.probs[:n].view(torch.int32)).sum())} elements)")
    if not torch.equal(a.toks[:n], b.toks[:n]):
        bad.append("tokens")
    return bad


def _dense(dev, a, params, noise, V, both=True):
    """the dense-logits K2 on what the front end derived"""
    ops, _ = _ops()
    out = _Out(dev, V)
    ops.logits_to_probs_sample(a.dbg[0], a.dbg[1] if both else None, H.GUIDANCE, params, noise, out.probs, ctypes.c_void_p(out.toks.data_ptr()))
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ (a), (b): one set of launches per case, shared
_RUNS = {}


def _run_case(dev, shape, window):
    if (shape, window) in _RUNS:
        return _RUNS[shape, window]
    inp = H.inputs(shape, window)
    n, V = inp["n_rows"], inp["V"]
    rules = H.rules_of(window)
    cols = _cols(inp, rules)
    planes, sumsq = inp["planes"].to(dev), inp["sumsq"].to(dev)
    params, noise = _params(dev, rules, n, 1), _noise(dev, V, len(_RUNS))
    rec = []
    for dtype, fold in H.FORMS:
        ref = H.model(inp, dtype, fold)
        a, b = (_launch(dev, inp, planes, sumsq, dtype, fold, params, noise, r) for r in ROUTES)
        ok, share, worst = H.judge(_observed(a, inp, n), ref, fold, dtype, cols)
        d = _dense(dev, a, params, noise, V)
        mass = a.probs[:n].sum(-1)
        rec.append(dict(form=f"{H.FORM_IDS[dtype]}{'+fold' if fold else ''}", dtype=dtype, fold=fold, ok=ok, share=share, worst=worst,
                        routes=_same(a, b, inp, rules, n), dense=_same(a, d, inp, rules, n, observers=False),
                        problems=a.problems(n) + b.problems(n) + d.problems(n), mass=(float(mass.min()), float(mass.max()))))
    _RUNS[shape, window] = rec
    return rec


_IDS = [f"{s}-{w}" for s, w in H.CASES]


@pytest.mark.parametrize("shape,window", H.CASES, ids=_IDS)
def test_derived_logits_equal_the_model_on_both_routes(dev, shape, window):
    chunks, slices, _ = H.SHAPES[shape]
    b = H.branches(chunks, slices, True, window, H.rules_of(window)[0])
    print(f"\n{shape} on {window}: {chunks} chunks ({'in flight' if b['planes_in_flight'] else 'loop'}), {slices} slices "
          f"({'preloaded' if b['stats8'] else 'k2_row_scales'}), {'float4' if b['in4_all'] else 'scalar'} loads, staged in {b['form']}")
    for r in _run_case(dev, shape, window):
        print(f"  {r['form']:>9}: share {r['share']:.5f} worst error / bound {r['worst']:.3f}  class {'B' if r['fold'] else 'A'}  mass {r['mass']}")
    for r in _run_case(dev, shape, window):
        assert r["ok"], (r["form"], r["share"], r["worst"])
        assert not r["routes"], (r["form"], "K2 and K2a + K2 differ in", r["routes"])
        assert not r["problems"], (r["form"], r["problems"])
        assert 0.999 < r["mass"][0] and r["mass"][1] < 1.001, (r["form"], r["mass"])


@pytest.mark.parametrize("shape,window", H.CASES, ids=_IDS)
def test_the_rest_of_k2_is_untouched_by_the_front_end(dev, shape, window):
    for r in _run_case(dev, shape, window):
        assert not r["dense"], (r["form"], "the dense K2 on the observed logits differs in", r["dense"])


# ------------------------------------------------------------------------------------------------ (c) ties
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_ties_round_to_nearest_even(dev, dtype):
    inp = H.tie_inputs(dtype)
    n, V = inp["n_rows"], inp["V"]
    rules = H.rules_of(H.TIE_WINDOW, two_range_rows=range(n))
    cols = _cols(inp, rules)
    ref = H.model(inp, dtype, False)
    planes, sumsq = inp["planes"].to(dev), inp["sumsq"].to(dev)
    params, noise = _params(dev, rules, n, 1), _noise(dev, V, 99)
    outs = [_launch(dev, inp, planes, sumsq, dtype, False, params, noise, r) for r in ROUTES]
    for route, o in zip(ROUTES, outs):
        got = _observed(o, inp, n)
        ok, share, _ = H.judge(got, ref, False, dtype, cols)
        g0, g1 = inp["gap"]
        n_inf = int(torch.isinf(got["c"][:, g0:g1]).sum())
        print(f"{dtype} {route}: share of observed logits off nearest-even {share:.5f}; {n_inf} infinities observed in the gap")
        assert ok, (route, share)
        assert n_inf > 0 and not o.problems(n)
        assert bool(torch.isfinite(o.probs[:n]).all()) and float((o.probs[:n].sum(-1) - 1).abs().max()) < 1e-3
    assert not _same(outs[0], outs[1], inp, rules, n)


# ------------------------------------------------------------------------------------------------ (d) CFG switches
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_cfg_switches(dev, dtype):
    shape, window = "lumina7b", "image0"
    inp = H.inputs(shape, window)
    n, V = inp["n_rows"], inp["V"]
    rules = H.rules_of(window)
    cols = _cols(inp, rules)
    noise = _noise(dev, V, 7)
    planes, sumsq = inp["planes"].to(dev), inp["sumsq"].to(dev)
    planes_nan, sumsq_nan = planes.clone(), sumsq.clone()
    planes_nan[:, H.LMAX:] = float("nan")                                  # the uncond half of the head and its statistics
    sumsq_nan[:, H.LMAX:] = float("nan")
    ref = H.model(inp, dtype, True, urow_off=0)                            # the cond rows alone
    for what, use_cfg, uo in (("use_cfg = 0 beside an uncond row", 0, H.LMAX), ("urow_off = 0", 1, 0)):
        params = _params(dev, rules, n, use_cfg)
        runs = []
        for route in ROUTES:
            clean = _launch(dev, inp, planes, sumsq, dtype, True, params, noise, route, urow_off=uo)
            dirty = _launch(dev, inp, planes_nan, sumsq_nan, dtype, True, params, noise, route, urow_off=uo)
            ok, share, worst = H.judge(_observed(clean, inp, n, both=False), ref, True, dtype, cols)
            print(f"{dtype} {what}, {route}: share {share:.5f} worst error / bound {worst:.3f}")
            assert ok, (what, route, share, worst)
            assert bool((clean.dbg[1] == SENT).all()) and bool((dirty.dbg[1] == SENT).all()), "the uncond observer was written"
            assert not _same(clean, dirty, inp, rules, n, both=False), (what, route, "NaN in the uncond half shows")
            assert not clean.problems(n) and not dirty.problems(n)
            dense = _dense(dev, clean, params, noise, V, both=False)
            assert not _same(clean, dense, inp, rules, n, observers=False), (what, route)
            runs.append(clean)
        assert not _same(runs[0], runs[1], inp, rules, n, both=False), what
    # row0: two prompts share one head of 64 partial rows; prompt p's cond rows start at row p * LMAX, its uncond rows 32 further
    inp2 = H.inputs(shape, window, 2, 64, 32)
    planes2, sumsq2 = inp2["planes"].to(dev), inp2["sumsq"].to(dev)
    params = _params(dev, rules, n, 1)
    for row0 in (H.LMAX, 0):
        ref2 = H.model(inp2, dtype, True, row0=row0)
        runs = [_launch(dev, inp2, planes2, sumsq2, dtype, True, params, noise, route, row0=row0) for route in ROUTES]
        for route, o in zip(ROUTES, runs):
            ok, share, worst = H.judge(_observed(o, inp2, n), ref2, True, dtype, cols)
            print(f"{dtype} row0 = {row0}, {route}: share {share:.5f} worst error / bound {worst:.3f}")
            assert ok, (row0, route, share, worst)
            assert not o.problems(n)
        assert not _same(runs[0], runs[1], inp2, rules, n), row0


# ------------------------------------------------------------------------------------------------ (e) confinement
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("shape", ["lumina7b", "swin30b"])
def test_nothing_outside_the_live_rows_and_hulls_is_used(dev, shape, poison):
    window, dtype = "image0", torch.bfloat16
    inp = H.inputs(shape, window)
    n, V = inp["n_rows"], inp["V"]
    rules = H.rules_of(window)
    noise, params = _noise(dev, V, 11), _params(dev, rules, n, 1)
    planes, sumsq = inp["planes"].to(dev), inp["sumsq"].to(dev)
    live = inp["cond"] + inp["unc"]
    dead = [r for r in range(inp["prows"]) if r not in live]                # partial rows >= n_rows of either half, and the pad rows up to prows
    lo = min(c[0] for c in _cols(inp, rules))
    hi = max(c[1] for c in _cols(inp, rules))
    assert lo > 0 and hi < inp["n_cols"], "the head has columns outside every hull"
    planes_p, sumsq_p = planes.clone(), sumsq.clone()
    planes_p[:, dead] = poison
    sumsq_p[:, dead] = poison
    planes_p[:, :, :lo] = poison                                            # head columns outside every row's hull
    planes_p[:, :, hi:] = poison
    for route in ROUTES:
        clean = _launch(dev, inp, planes, sumsq, dtype, True, params, noise, route)
        dirty = _launch(dev, inp, planes_p, sumsq_p, dtype, True, params, noise, route, probs_fill=poison)
        assert not _same(clean, dirty, inp, rules, n), (route, "poison outside the live rows and hulls shows")
        assert not clean.problems(n), (route, clean.problems(n))
        assert not dirty.problems(n), (route, dirty.problems(n))
        assert bool(torch.isfinite(dirty.probs[:n]).all())


# ------------------------------------------------------------------------------------------------ (f) the real producer
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_g1_planes_and_f1r_statistics_into_k2(dev, dtype):
    """the planes of ops.skinny_gemm_cols and the statistics of ops.residual_sumsq over operands on the exact grid: both are known to the bit, and the
    logits K2 derives from them are dtype(r * exact x @ w.T) within f2_source's tolerance -- the linear layer the kernel replaces"""
    ops, L = _ops()
    p = H.producer_inputs(dtype)
    P = H.PRODUCER
    n, V = p["n_rows"], p["V"]
    x, w = p["x"].to(dev), p["w"].to(dev)
    part = ops.skinny_gemm_cols(x, ops.pack_weight(w, P["KC"], True), V, P["hidden"], P["KC"], 0, V, waves=4, step_major=True)
    h = x.clone()
    ss = ops.residual_sumsq(h)
    torch.cuda.synchronize()
    rows = x.shape[0]
    assert part.n_chunks == P["chunks"] and torch.equal(part.data[:, :rows].cpu().view(torch.int32), p["planes"].view(torch.int32)), "G1's planes are not the exact sums"
    assert torch.equal(h, x) and torch.equal(ss[:, :rows].cpu().view(torch.int32), p["sumsq"].view(torch.int32)), "F1r's statistics are not the exact sums"
    rules = [dict(ranges=(), forced=-1, top_k=10)] * n
    params, noise = _params(dev, rules, n, 1), _noise(dev, V, 5)
    ref = H.model(p, dtype, True)
    inp = dict(p, prows=part.data.shape[1])
    outs = [_launch(dev, inp, part.data, ss, dtype, True, params, noise, route) for route in ROUTES]
    for route, o in zip(ROUTES, outs):
        ok, share, worst = H.judge(_observed(o, inp, n), ref, True, dtype, _cols(inp, rules))
        print(f"{dtype} {route}: G1 + F1r -> K2: share {share:.5f} worst error / bound {worst:.3f}")
        assert ok, (route, share, worst)
        assert not o.problems(n)
    assert not _same(outs[0], outs[1], inp, rules, n)
