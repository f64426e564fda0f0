"""GPU: K2 (k2_logits_to_probs_sample) and K4 (k4_verify_accept) against the CPU oracle on tied, wide-range and masked scores.

The rows come from tests/sampling_edge_cases.py; tests/test_sampling_edge_cases.py shows on the CPU that each of them reaches the data-dependent
branch it is named for -- more than RANK_CAP survivors in the selected value bin (the radix passes), the pooled bin 0, a tie at the k-th largest
(in the rank loop and inside radix_pick), +0.0 / -0.0 at the k-th position, top_k equal to / above the finite count, -inf inside the window, a
tie at the top-p cut, the draw list filled to its last entry and overflowing (both noise sources), and in K4 a tied k-th largest of the residual,
top_k == n_pos, top_k > n_pos, a tied top-p cut and the degenerate residual -- and that the oracle equals the definitional fp64 reference there.
Here the kernels must equal the oracle: tokens, and the bit patterns of the whole probability row, written into a -7.0-poisoned buffer.
Every test prints the branch predicates of its rows: the log is the record of what ran.

Not covered: +inf, NaN or all-masked rows (the reference and the oracle produce NaN probabilities there and nothing defines the token), hence
K2's path for zmax == +inf (block_kth_largest_bisect called from K2) stays untested.  The partial-sum head forms and K2a are tied bit for bit
to the dense K2 elsewhere (tests/test_gpu_kernels.py).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sjd_oracle as O
from tests import sampling_edge_cases as SE
from tests.test_gpu_kernels import _ops, run_k2, run_k4, to_dev_rule

SEED = 20250307
K2_OFFSET = 4 * 977                    # Philox offset of K2's draw; K4: rs at K4_OFFSETS[1], the residual draw at K4_OFFSETS[2]
K4_OFFSETS = (0, 4096, 1 << 20)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _philox_fill(dev, numel, offset, kind):
    """the tensor K2 / K4 would generate in place for (SEED, offset) over `numel` elements (kind 0: uniform, 1: Exp(1)), as tests/test_gpu_philox.py"""
    ops, L = _ops()
    out = torch.empty(numel, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.load().sjd_philox_fill(out.data_ptr(), numel, SEED, offset, ops.philox_max_blocks(dev), kind, stream), "sjd_philox_fill")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _run_k2_philox(dev, logits, use_cfg, guidance, rules):
    """run_k2 with the noise generated in the kernel (params->philox_blocks > 0, no noise tensor)"""
    ops, L = _ops()
    _, n, V = logits.shape
    params = ops.DeviceBlob(L.IterParams, dev)
    pv = params.view
    pv.n_rows, pv.use_cfg = n, int(use_cfg)
    pv.philox_blocks, pv.philox_seed = ops.philox_max_blocks(dev), SEED
    pv.philox_offset[0] = K2_OFFSET
    for j, r in enumerate(rules):
        pv.rules[j] = to_dev_rule(L, ops, r)
    params.upload()
    lg = torch.from_numpy(logits).to(dev)
    probs = torch.full((n, V), -7.0, device=dev)
    toks = torch.full((n,), -5, dtype=torch.int64, device=dev)
    ops.logits_to_probs_sample(lg[0], lg[1], guidance, params, None, probs, ctypes.c_void_p(toks.data_ptr()))
    torch.cuda.synchronize()
    return toks.cpu().numpy(), probs.cpu().numpy()


_K2 = SE.k2_params()
_LIST_NAMES = {c["name"] for c in SE.K2_LIST_CASES} | {SE.K2_ODD_CASE["name"]}
_K2_PARAMS = [(i, "tensor") for i in range(len(_K2))] + [(i, "philox") for i, (c, f) in enumerate(_K2) if c["name"] in _LIST_NAMES]


@pytest.mark.parametrize("i,noise", _K2_PARAMS, ids=[f"{_K2[i][0]['name']}@{_K2[i][1]}-{nz}" for i, nz in _K2_PARAMS])
def test_k2_equals_the_oracle(dev, i, noise):
    case, form = _K2[i]
    b = SE.build_k2(case, form)
    n, V = b["c"].shape
    rules = [O.rule(**r) for r in b["rules"]]
    logits = np.stack([b["c"], b["u"]])
    if noise == "philox":       # the oracle reads what sjd_philox_fill writes for the same seed, offset, n_rows * V and block count
        e = _philox_fill(dev, n * V, K2_OFFSET, 1).reshape(n, V)
    else:
        e = np.maximum(np.random.default_rng(1000 + i).standard_exponential((n, V)).astype(np.float32), np.float32(1e-30))
    toks_ref, probs_ref = O.logits_to_probs_sample(b["c"], b["u"] if b["use_cfg"] else None, SE.GUIDANCE, rules, e)
    for j, row in enumerate(case["rows"]):
        st = SE.row_stats(b, j, probs_ref[j])
        print(f"{b['name']} [{noise}, {b['staging']['form']}] row {j}: {SE.describe(st)}  [{', '.join(row['expect'])}]")
        for tag in row["expect"]:
            assert SE.PREDICATES[tag](st), (tag, SE.describe(st))
    if noise == "philox":
        toks, probs = _run_k2_philox(dev, logits, b["use_cfg"], SE.GUIDANCE, rules)
    else:
        toks, probs = run_k2(dev, logits, b["use_cfg"], SE.GUIDANCE, rules, e)
    bad = probs.view(np.uint32) != probs_ref.view(np.uint32)
    assert not bad.any(), (f"{b['name']}: {int(bad.sum())} probabilities differ, rows {sorted(set(np.nonzero(bad)[0].tolist()))}, "
                           f"support {(probs > 0).sum(-1).tolist()} vs {(probs_ref > 0).sum(-1).tolist()}, max |dp| {np.abs(probs - probs_ref).max()}")
    assert toks.tolist() == toks_ref.tolist()


# ------------------------------------------------------------------------------------------------ K4
def _k4_launch(dev, win, Y, p, q_rows, resid, rs, e2, philox, max_rows=16):
    """one launch of the one-slot K4 -> (m, tokens, state.rejected as the kernel wrote it: 0 / 1 / 2).  philox: rs and e2 are None and the
    kernel generates both (the lenience tests show the blob's fields)"""
    ops, L = _ops()
    n, V = p.shape
    params, state = ops.DeviceBlob(L.IterParams, dev), ops.DeviceBlob(L.State, dev)
    pv, sv = params.view, state.view
    pv.n_rows, pv.scheme, pv.iter_seq = n, 0, 555
    for j, r in enumerate(resid):
        pv.resid_rules[j] = to_dev_rule(L, ops, r)
    if philox:
        pv.philox_blocks, pv.philox_seed = ops.philox_max_blocks(dev), SEED
        for a in range(3):
            pv.philox_offset[a] = K4_OFFSETS[a]
    prev = torch.zeros(max_rows, V, device=dev)
    for i in range(n):
        sv.win_tok[i], sv.tokens[i] = int(win[i]), int(Y[i])
        sv.q_src[i] = -1 if q_rows[i] is None else i
        if q_rows[i] is not None:
            prev[i] = torch.from_numpy(np.asarray(q_rows[i])).to(dev)
    params.upload()
    state.dev.copy_(state.host)
    probs = torch.zeros(max_rows, V, device=dev)
    probs[:n] = torch.from_numpy(np.asarray(p)).to(dev)
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ops.verify_accept(params, state, probs, prev, to(rs), to(e2), torch.empty(V, device=dev))
    torch.cuda.synchronize()
    st = state.download()
    return int(st.m), [int(st.tokens[i]) for i in range(n)], int(st.rejected)


def _k4_inputs(dev, V, noise):
    """window ids, uniforms and the residual draw's noise such that drafts 1 .. K4_REJECT - 1 are accepted and draft K4_REJECT is the first
    rejection; every draft has p(x) > 0.  tensor: rs is 0 in front of the rejection and 1.0 at rs[K4_REJECT, x].  philox: rs / noise2 are the
    tensors the kernel generates (sjd_philox_fill: n * V uniforms at offset 1, V exponentials at offset 2) and the drafts are chosen among the
    columns with p(x) > 0 by what those uniforms decide."""
    p, q = SE.k4_pq(V, O)
    n, R = SE.K4_N, SE.K4_REJECT
    if noise == "philox":
        rs = _philox_fill(dev, n * V, K4_OFFSETS[1], 0).reshape(n, V)
        e2 = _philox_fill(dev, V, K4_OFFSETS[2], 1)
    else:
        rs = np.zeros((n, V), np.float32)
        e2 = np.maximum(np.random.default_rng(77 + V).standard_exponential(V).astype(np.float32), np.float32(1e-30))
    win = [7]
    for i in range(1, n):
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.minimum(p[i - 1] / q[i], np.float32(1.0))
        cand = np.flatnonzero(p[i - 1] > 0)
        if noise == "philox" and i < R:
            cand = cand[rs[i, cand] < ratio[cand]]
        elif noise == "philox" and i == R:
            cand = cand[(q[i, cand] > 0) & ~(rs[i, cand] < ratio[cand])]
        x = int(cand[(7 * i) % len(cand)])
        if noise == "tensor" and i == R:
            rs[i, x] = 1.0
        win.append(x)
    Y = [int(t) for t in np.random.default_rng(5).integers(0, V, n)]
    return p, q, win, Y, rs, e2


_K4_PARAMS = [(V, name, noise) for V in SE.K4_SHAPES for name in list(SE.K4_RESIDUAL_RULES) + ["degenerate"] for noise in ("tensor", "philox")]


@pytest.mark.parametrize("V,name,noise", _K4_PARAMS, ids=[f"V{V}-{name}-{nz}" for V, name, nz in _K4_PARAMS])
def test_k4_residual_equals_the_oracle(dev, V, name, noise):
    p, q, win, Y, rs, e2 = _k4_inputs(dev, V, noise)
    n, R = SE.K4_N, SE.K4_REJECT
    _, hole, form = SE.K4_SHAPES[V]
    d = SE.residual(p[R - 1], q[R], (), V)
    if name == "degenerate":                 # the rule allows only columns where no target row has mass: max(p - q, 0) is 0 on all of them
        rule = dict(ranges=(hole,))
        assert not (SE.residual(p[R - 1], q[R], rule["ranges"], V) > 0).any()
    else:
        mk, tags = SE.K4_RESIDUAL_RULES[name]
        rule = mk(d, int((d > 0).sum()))
        st = SE.residual_stats(d, rule, V)
        stg = SE.staging(V, (), kernel="k4")
        assert stg["form"] == form
        print(f"K4 V {V} [{noise}, {form}] {name}: rule {rule} n_pos {st['n_pos']} tie {st['tie']} kept {st['kept']} list_cap {stg['list_cap']} "
              f"top_p {st['top_p']}")
        for t in tags:
            assert SE.K4_PREDICATES[t](st), (t, st)
    resid = [O.rule(**rule)] * (n - 1)
    q_rows = [None] + [q[i] for i in range(1, n)]
    m_ref, tok_ref, rej_ref = O.verify_accept(win, Y, p, q_rows, rs, resid, e2)
    assert (m_ref, rej_ref) == (R, True), "the inputs force the first rejection at the chosen row"
    if name != "degenerate" and noise == "tensor":
        m, tok, rej = run_k4(dev, win, Y, p, q_rows, rs, resid, e2)
        rej = int(rej)
    else:
        m, tok, rej = _k4_launch(dev, win, Y, p, q_rows, resid, None if noise == "philox" else rs, None if noise == "philox" else e2,
                                 noise == "philox")
    assert m == m_ref
    if name == "degenerate":                 # the reference's multinomial raises here: the kernel flags it, the token is not defined
        assert rej == 2
        assert tok[:m - 1] == tok_ref[:m - 1].tolist() == win[1:m]
    else:
        assert rej == 1
        assert tok[:m] == tok_ref[:m].tolist()
        assert tok[m - 1] >= 0 and d[tok[m - 1]] > 0, "the resampled id has residual mass"
    assert tok[m:] == Y[m:]                  # the unverified tail is carried unchanged
