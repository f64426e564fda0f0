"""CPU guard of the K2 / K4 selection-edge tests: every row of tests/sampling_edge_cases.py reaches the branch it is named for, the dense
Gaussian inputs of the older K2 tests reach none of them, and the oracle (what the kernels are held to on the GPU) equals the definitional
fp64 reference on every row before any kernel is involved."""
import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import sjd_oracle as O
from tests import sampling_edge_cases as SE

_K2 = SE.k2_params()
_IDS = [f"{c['name']}@{f}" for c, f in _K2]


@functools.lru_cache(maxsize=None)
def _oracle_k2(i):
    case, form = _K2[i]
    b = SE.build_k2(case, form)
    rules = [O.rule(**r) for r in b["rules"]]
    toks, probs = O.logits_to_probs_sample(b["c"], b["u"] if b["use_cfg"] else None, SE.GUIDANCE, rules, np.ones_like(b["c"]))
    return b, probs


@pytest.mark.parametrize("i", range(len(_K2)), ids=_IDS)
def test_every_row_reaches_the_branch_it_is_named_for(i):
    b, probs = _oracle_k2(i)
    case, form = _K2[i]
    assert np.all(np.isfinite(b["z"]) | (b["z"] == -np.inf)), "scores are finite or -inf"
    for j, row in enumerate(case["rows"]):
        st = SE.row_stats(b, j, probs[j])
        print(f"{b['name']} row {j}: {SE.describe(st)}  [{', '.join(row['expect'])}]")
        assert st["n_finite"] >= 1
        assert row["expect"], "a row without a named branch checks nothing new"
        for tag in row["expect"]:
            assert SE.PREDICATES[tag](st), f"{b['name']} row {j}: {tag} does not hold: {SE.describe(st)}"


def test_the_tables_cover_every_named_branch_at_every_staging_form():
    for form in SE.SELECTION_FORMS:
        tags = {t for c, f in _K2 if f == form for r in c["rows"] for t in r["expect"]}
        assert tags >= set(SE.PREDICATES) - {"list_brim", "list_overflow"}, (form, set(SE.PREDICATES) - tags)
    for form in SE.LIST_FORMS:
        tags = {t for c, f in _K2 if f == form for r in c["rows"] for t in r["expect"]}
        assert {"list_full", "list_brim", "list_overflow"} <= tags
    assert [SE.staging(*SE.FORMS[f][:2])["form"] for f in SE.SELECTION_FORMS] == ["registers", "lds", "global"]
    assert SE.staging(*SE.FORMS["lds_llamagen"][:2])["list_cap"] == SE.SJD_DRAW_LIST
    V, ranges, _ = SE.FORMS["odd"]
    assert V % 4 and ranges[0][0] % 4 and ranges[0][1] % 4


@pytest.mark.parametrize("use_cfg", [False, True])
def test_the_dense_gaussian_inputs_of_test_k2_bit_exact_reach_no_tie_list_or_count_branch(use_cfg):
    """documents the gap: the first case of K2_CASES (Lumina image rows, top-k 2000 of 8192 columns in V = 65536), drawn as test_k2_bit_exact
    draws it, never has a tie at the k-th largest, never keeps more than top_k entries, never fills the draw list and has no -inf inside the
    window.  Without CFG the selected bin holds a dozen or two scores and is never bin 0; with CFG at guidance 3 the scores spread to about
    3 * sqrt(13) per unit of logit scale, the k-th largest falls just below zmax - 32 in most rows, and those rows DO take bin 0 and the radix
    passes -- over distinct keys only, which is all of the named branches the older inputs reach (measured here, printed per row)."""
    from tests.test_gpu_kernels import K2_CASES
    name, V, n, builder = K2_CASES[0]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 10000)
    logits = (torch.randn(2, n, V, generator=g) * 3.0).numpy()
    z = SE.combine(logits[0], logits[1], 3.0) if use_cfg else logits[0]
    seen = 0
    for j, r in enumerate(builder(n)):
        if r.forced >= 0:
            continue
        rule = dict(ranges=tuple((r.lo[a], r.hi[a]) for a in range(r.n_ranges)), top_k=r.top_k)
        stg = SE.staging(V, rule["ranges"])
        st = SE.select_stats(z[j], rule, V)
        st.update(window=stg["whi"] - stg["wlo"], list_cap=stg["list_cap"], n_mass=st["kept"], top_p=None)
        print(f"{name} use_cfg {use_cfg} row {j}: {SE.describe(st)}")
        reached = {t for t, pred in SE.PREDICATES.items() if t != "select_runs" and pred(st)}
        assert st["select"] and st["kept"] == st["top_k"] and st["tie"] == 1
        if use_cfg:
            assert reached <= {"bin0", "rank_overflow"}, reached
        else:
            assert reached == set() and st["bsel"] > 0 and st["survivors"] <= SE.RANK_CAP // 4, reached
        seen += 1
    assert seen >= 8


@pytest.mark.parametrize("i", range(len(_K2)), ids=_IDS)
def test_oracle_equals_the_definitional_reference(i):
    b, probs = _oracle_k2(i)
    case, form = _K2[i]
    for j, row in enumerate(case["rows"]):
        rule = b["rules"][j]
        ref = SE.reference_k2_row(b["z"][j], rule, b["V"])
        assert np.isfinite(probs[j]).all() and abs(float(probs[j].astype(np.float64).sum()) - 1.0) < 1e-5
        # the support is EXACTLY {z >= k-th largest} inside the rule (less what the canonical exponential flushes: z - zmax < -87, which only
        # the scale-40 Gaussian rows have), after the tie rule of top-p where the row has one: a set equality
        assert np.array_equal(probs[j] > 0, ref["support"]), f"{b['name']} row {j}: {int(((probs[j] > 0) != ref['support']).sum())} columns differ"
        if case["name"] != "bin0_gauss40":
            st = SE.select_stats(b["z"][j], rule, b["V"])
            if rule.get("top_p") is None:
                assert int(ref["support"].sum()) == st["kept"], "nothing underflows: the support is the whole kept set"
        if rule.get("top_p") is None and rule.get("temperature", 1.0) == 1.0:
            np.testing.assert_allclose(probs[j], ref["probs"], atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("i", [i for i, (c, f) in enumerate(_K2) if any(r["rule"].get("top_p") for r in c["rows"])],
                         ids=lambda i: _IDS[i])
def test_top_p_rows_follow_the_tie_rule(i):
    b, probs = _oracle_k2(i)
    case, form = _K2[i]
    for j, row in enumerate(case["rows"]):
        rule = b["rules"][j]
        if rule.get("top_p") is None:
            continue
        ref = SE.reference_k2_row(b["z"][j], dict(rule, top_p=None), b["V"])         # before the cut: the fp64 probabilities the cut works on
        info = SE.reference_k2_row(b["z"][j], rule, b["V"])["top_p"]
        z, p64 = b["z"][j], ref["probs"]
        kept, before = probs[j] > 0, ref["support"]
        imax = int(np.argmax(np.where(before, z, -np.inf)))                           # lowest index among the maxima
        assert kept[imax]
        # columns with equal scores share their fate (but the lowest-index maximum, which always survives)
        for v in np.unique(z[before]):
            grp = np.flatnonzero(before & (z == v))
            fate = {bool(kept[c]) for c in grp if c != imax}
            assert len(fate) <= 1, f"{b['name']} row {j}: the run of score {v} is split"
        removed_mass = float(p64[before & ~kept].sum())
        thr = float(np.float32(1.0 - rule["top_p"]))
        assert removed_mass <= thr
        smallest_kept = np.min(z[kept])
        also = removed_mass + float(p64[before & kept & (z == smallest_kept)].sum())
        assert also > thr, "removing the smallest kept run as well would exceed 1 - top_p"
        # both sums are at least 1e-4 away from the threshold: the fp32 canonical sums cannot flip either comparison
        assert thr - removed_mass >= 1e-4 and also - thr >= 1e-4, (removed_mass, also, thr)
        assert abs(info["removed_mass"] - removed_mass) < 1e-9 and max(info["cut_group_sizes"]) > 1


# ------------------------------------------------------------------------------------------------ K4
@pytest.mark.parametrize("V", list(SE.K4_SHAPES))
def test_k4_residual_rules_reach_their_branches(V):
    p, q = SE.k4_pq(V, O)
    ranges, hole, form = SE.K4_SHAPES[V]
    assert SE.staging(V, (), kernel="k4")["form"] == form
    for rows in (p, q):                       # genuine normalised rows with runs of equal values and exact zeros
        assert np.allclose(rows.astype(np.float64).sum(-1), 1.0, atol=1e-5) and (rows == 0).any(-1).all()
        assert all(len(np.unique(r[r > 0])) < 0.1 * int((r > 0).sum()) for r in rows)
    assert (p[:, hole[0]:hole[1]] == 0).all(), "no target row has mass in the hole"
    d = SE.residual(p[SE.K4_REJECT - 1], q[SE.K4_REJECT], (), V)
    n_pos = int((d > 0).sum())
    assert n_pos > 100 and len(np.unique(d[d > 0])) < n_pos, "tied residual weights"
    for name, (mk, tags) in SE.K4_RESIDUAL_RULES.items():
        rule = mk(d, n_pos)
        st = SE.residual_stats(d, rule, V)
        print(f"V {V} {name}: rule {rule} n_pos {st['n_pos']} tie {st['tie']} kept {st['kept']} top_p {st['top_p']}")
        for t in tags:
            assert SE.K4_PREDICATES[t](st), (name, t, st)
    # the degenerate residual: the rule allows only the hole, where p = 0 <= q
    assert not (SE.residual(p[SE.K4_REJECT - 1], q[SE.K4_REJECT], (hole,), V) > 0).any()
    assert (q[SE.K4_REJECT, hole[0]:hole[1]] > 0).any()
