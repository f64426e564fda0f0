"""CPU guard of tests/attention_probe_cases.py (no GPU, no libsjd_hip.so): before a probe runs on a kernel, the tile / split model shows that
every case reaches the branch it is named for, fp64 attention gives the closed-form answers, the float32 model of the kernels' order of
operations produces exactly the asserted integers and bits, and the comparators catch deliberately wrong models.

The float32 model runs every probe of every (form, key range) at every key-split count, except that over the two long contexts (39 / 33
tiles) the dominant layouts run at the largest split count only (the census runs at all of them): the model is a Python loop over tiles.
"""
import math

import numpy as np
import pytest
import torch

from tests import attention_probe_cases as P
from tests import blob_array_cases as BA


def _probes():
    return [("census", None)] + [("dominant", lay) for lay in P.LAYOUTS]


def _check(form, geo, inp, n_split, mutant=None):
    out = P.kernel_model(form, geo, inp, n_split, mutant)
    if inp["probe"] == "census":
        return P.census_failures(form, geo, inp["expect"], out)
    return P.dominant_failures(form, geo, inp["expect"], torch.from_numpy(out).to(P.TORCH_DTYPE[form["dtype"]]))


# ------------------------------------------------------------------------------------------------ the cases reach what they are named for
RANGE_BRANCH = {          # range -> what some (batch row, chunk) of it must show at the largest split count of a key-split form
    "kv0": {"hidden_rows"}, "tiles4_edge0": {"tiles4", "eff1"}, "tiles5": {"tiles5", "eff2", "short_last_split", "key_start_mid_tile"},
    "tiles8": {"tiles8", "eff2"}, "edge1": {"partial_last_tile", "key_start_mid_tile"}, "middle_row": {"hidden_rows"}, "all_hidden": {"no_tile"},
    "last_split_short": {"eff8", "short_last_split"}, "last_split_empty": {"dropped_split"}, "device_blob": {"padding_rows"}}


@pytest.mark.parametrize("form", P.FORMS, ids=[f["name"] for f in P.FORMS])
def test_cases_reach_their_branches(form):
    one_chunk = form["n"] <= P.ROWS
    for rng in P.ranges_of(form):
        geo = P.geometry(form, rng)
        assert geo["S"] % P.KT == 0 and geo["S"] <= 1312 and max(geo["kv"]) + geo["n"] <= geo["S"]
        got = P.branches(form, geo, 8)
        want = set(RANGE_BRANCH[rng["name"]])
        if not one_chunk:          # (several chunks: the tile counts named are those of a 16-row window; the other branches hold for some chunk)
            want -= {"tiles4", "tiles5", "tiles8", "eff1", "eff2", "eff8", "short_last_split", "dropped_split"}
        if form["n"] == 1 or (rng["name"] == "kv0" and form["n"] < 2):
            want -= {"hidden_rows"}
        assert want <= got, (form["name"], rng["name"], sorted(want - got), sorted(got))
    # ranges are congruent as named
    for rng in P.ranges_of(form):
        n = form["n"]
        if rng["name"] == "tiles4_edge0":
            assert (rng["kv"] + n) % 32 == 0 and rng["ks"][1] % 32 == 0
        if rng["name"] == "edge1":
            assert (rng["kv"] + n) % 32 == 1 and all(k % 32 == 31 for k in rng["ks"])
        if rng["name"] == "middle_row":
            assert rng["ks"][0] == rng["kv"] + n // 2
        if rng["name"] == "all_hidden":
            assert rng["ks"][0] > rng["kv"] + n - 1


def test_tile_range_edges():
    """k1_tile_range restated: the K1_MIN_TILES_PER_SPLIT edges, a short and a dropped last split, the 130-tile case of the ring kernel"""
    assert P.tile_range(0, 128, 8)[2:] == (1, 4) and P.tile_range(0, 160, 8)[2:] == (2, 3) and P.tile_range(0, 256, 8)[2:] == (2, 4)
    assert P.tile_range(0, 1233, 8) == (0, 39, 8, 5) and P.tile_range(0, 1056, 8) == (0, 33, 7, 5)
    assert P.tile_range(0, 4101 + 16, 16) == (0, 129, 15, 9) and P.tile_range(0, 4101 + 32, 16) == (0, 130, 15, 9)
    assert P.tile_range(100, 64, 8) == (3, 2, 1, 0)
    for f in P.FORMS:
        for s in P.splits_of(f):
            P.route(f, s)
    reached = {d for f in P.FORMS for s in P.splits_of(f) for d in [P.route(f, s)["detail"]] + (["k1_combine"] if P.route(f, s)["combine"] else [])}
    assert set(P.REQUIRED_DETAILS) <= reached, sorted(set(P.REQUIRED_DETAILS) - reached)
    assert P.route(P.FORM["prefill60"], 4)["detail"] == "k1_partial_ring<4 pairs>"      # four chunks of one head share their tiles: the ring kernel


def test_census_integer_decode_and_rounding_bound():
    """round(round16(fl32(c fl32(1 / N))) N) == c for every N the cases use, both 16-bit types, with room for another fp32 ulp; the error is
    within half a 16-bit ulp + 2^-22 relative -- and NOT within (2^-9 + 2^-22) c / N (bf16), which a correctly rounded result already
    exceeds: half an ulp is up to 2^-8 of the value (8 significant bits), 2^-11 in fp16"""
    Ns = set()
    for form in P.FORMS:
        for rng in P.ranges_of(form) + [P.BLOB_ARRAY_RANGE]:
            geo = P.geometry(form, rng)
            Ns |= set(np.unique(P.census_answer(form, geo)["N"]).tolist())
    Ns |= set(range(4090, 4140))
    Ns.discard(0)
    beyond_literal = 0
    for dtype in ("bf16", "fp16"):
        for N in sorted(Ns):
            c = np.arange(0, min(N, math.ceil(N / 64) + 2) + 1, dtype=np.float32)
            inv = np.float32(1.0) / np.float32(N)
            for bump in (0, 1, -1):                              # another fp32 ulp either way
                x = (c * inv).astype(np.float32)
                x = np.nextafter(x, np.float32(np.inf if bump > 0 else -np.inf)) if bump else x
                x = np.where(c == 0, np.float32(0), x)
                got = P._round16(x, dtype).astype(np.float64)
                assert (np.rint(got * N) == c).all(), (dtype, N)
                if bump == 0:
                    exact = c.astype(np.float64) / N
                    tol = P.HALF_ULP_REL[dtype] * 2.0 ** np.floor(np.log2(np.where(exact > 0, exact, 1.0))) * (exact > 0) + 2.0 ** -22 * exact
                    assert (np.abs(got - exact) <= tol).all(), (dtype, N)
                    beyond_literal += int((np.abs(got - exact) > (P.HALF_ULP_REL[dtype] / 2 + 2.0 ** -22) * exact).sum())
    assert beyond_literal > 0


# ------------------------------------------------------------------------------------------------ closed forms, margins, the float32 model
@pytest.mark.parametrize("form", P.FORMS, ids=[f["name"] for f in P.FORMS])
def test_closed_forms_margins_and_float32_model(form):
    extra = {"partial8_bf16": [P.BLOB_ARRAY_RANGE], "dsplit_bf16": [P.BLOB_ARRAY_RANGE], "fp8_mha": [P.BLOB_ARRAY_RANGE]}.get(form["name"], [])
    applied = 0
    for rng in P.ranges_of(form) + extra:
        geo = P.geometry(form, rng)
        long_ctx = geo["S"] > 1000
        splits = P.splits_of(form)
        ring = P.route(form, 4)["kernel"] == "k1_partial_ring"      # (its tie layouts run at every split count: the one-split walk is the longest)
        for probe, layout in _probes():
            seen_reason = None
            for n_split in splits:
                if probe == "dominant" and long_ctx and n_split != splits[-1] and not (ring and layout.startswith("ties")):
                    continue
                inp = P.build(form, geo, probe, layout, n_split)
                if isinstance(inp, str):
                    seen_reason = inp
                    continue
                applied += 1
                what = (form["name"], rng["name"], n_split, layout or "census")
                if probe == "dominant":
                    # one level is >= 40 nats and the winner is a level above everything else the row sees
                    assert P.nats_per_level(form) >= P.MARGIN_NATS and inp["expect"]["margin"] >= 1.0, what
                    vv = np.abs(inp["vval"].numpy())
                    live = vv[np.isfinite(vv) & (vv > 0)]
                    assert live.min() >= 2.0 ** -4 and live.max() <= 4.0, what
                    others = geo["S"] * math.exp(-P.nats_per_level(form)) * 4.0
                    assert others < 2.0 ** -30 * live.min(), what
                    assert P.ring_exponent_ok(form, inp, n_split), what
                if n_split == splits[-1] and not geo["nb"]:
                    _fp64_equals_closed_form(form, geo, inp, what)
                fails = _check(form, geo, inp, n_split)
                assert not fails, (what, fails[:3])
            del seen_reason
    assert applied


def _fp64_equals_closed_form(form, geo, inp, what):
    """blob_array_cases.attention_fp64 on the probe's own operands (the dequantised cache for fp8) is the closed-form answer"""
    kv, nv = geo["kv"][0], geo["nv"][0]
    G = form["H"] // form["Hkv"]
    q = inp["q"].double()
    if form["DL"] != form["D"]:                      # (attention_fp64 scales by 1 / sqrt(D): the probes' margins hold for either scale)
        pass
    exact, _, vis = BA.attention_fp64(q, inp["kval"], inp["vval"], kv, nv, geo["ks"], torch.bfloat16)
    exact = exact.numpy()
    if inp["probe"] == "census":
        c, N = inp["expect"]["counts"][:, :nv, None, :], inp["expect"]["N"][:, :nv, None, None]
        sv = form["scales"][1] if form["cache"] == "fp8" else 1.0
        want = np.where(N > 0, c / np.maximum(N, 1), 0.0) * sv
        assert np.abs(exact - want).max() <= 1e-12, what
    else:
        want = np.repeat(inp["expect"]["value"][:, :nv], G, axis=2)
        assert np.abs(exact - want).max() <= 2.0 ** -30, what
    hidden = np.array([[len(w) == 0 for w in rows[:nv]] for rows in inp["expect"]["winners"]]) if inp["probe"] != "census" else inp["expect"]["N"][:, :nv] == 0
    assert (vis.numpy() == ~hidden).all(), what


def test_ring_tie_drift_is_modelled(monkeypatch):
    """the float32 model keeps k1_partial_ring's exp2(fma(s, c1, -fl(m c1))): with the tie level at 120 (m c1 inexact) two winners 37 tiles
    apart on one split miss the mean -- what the kernel did on the GPU -- and ring_exponent_ok() says so beforehand; at level 64 both hold"""
    form = P.FORM["ring8_n32"]
    rng = next(r for r in P.ranges_of(form) if r["name"] == "last_split_short")
    geo = P.geometry(form, rng)
    inp = P.build(form, geo, "dominant", "ties2", 1)
    assert P.ring_exponent_ok(form, inp, 1) and not _check(form, geo, inp, 1)
    monkeypatch.setattr(P, "TIE_LEVEL_16BIT", 120)
    inp = P.build(form, geo, "dominant", "ties2", 1)
    assert not P.ring_exponent_ok(form, inp, 1) and _check(form, geo, inp, 1)


# ------------------------------------------------------------------------------------------------ the comparators catch wrong kernels
CATCH = [      # (form, range, n_split): small cases, chosen so that every mutant changes something
    ("partial8_bf16", "tiles8", 8), ("partial8_bf16", "edge1", 4), ("partial4", "tiles5", 8), ("ring8_n20", "tiles8", 8),
    ("fp8_mha", "tiles8", 4), ("partial1_two_chunks", "tiles8", 8)]
CENSUS_BLIND = {"old_max_in_rescale", "unshifted_split_max"}      # every maximum of a census is 0 and every weight exp(0): by construction


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_comparators_catch_a_wrong_model(mutant):
    caught = {"census": [], "dominant": []}
    for name, rname, n_split in CATCH:
        form = P.FORM[name]
        rng = next(r for r in P.ranges_of(form) if r["name"] == rname)
        geo = P.geometry(form, rng)
        for probe, layout in _probes():
            inp = P.build(form, geo, probe, layout, n_split)
            if isinstance(inp, str):
                continue
            assert not _check(form, geo, inp, n_split)
            if _check(form, geo, inp, n_split, mutant):
                caught[probe].append((name, rname, layout))
    assert caught["dominant"], mutant
    if mutant in CENSUS_BLIND:
        assert not caught["census"], (mutant, caught["census"])
    else:
        assert caught["census"], mutant
    print(f"\n  {mutant}: census cases {len(caught['census'])}, dominant layouts {sorted({c[2] for c in caught['dominant']})}")


# ------------------------------------------------------------------------------------------------ how sharp is the Gaussian tests' bound?
SENSITIVITY_CASES = [("mha_d128_mid", 2, 4, 4, 128, 1280, 1216, 16, [0, 59], torch.bfloat16),
                     ("gqa4_d128", 2, 8, 2, 128, 4224, 4100, 16, [3, 0], torch.float16)]      # rows of test_gpu_kernels.ATTN_CASES


def sensitivity(case):
    """-> share of output elements (visible rows) beyond attention_fp64's bound when the fp64 reference loses (a) each row's key at the causal
    edge, (b) the 32-key tile in the middle of the context, (c) the last full tile in front of the window"""
    name, B, H, Hkv, D, S_max, kv_len, n, key_start, dtype = case
    g = torch.Generator().manual_seed(len(name))
    kc = torch.randn(1, B, Hkv, S_max, D, generator=g).to(dtype)
    vc = torch.randn(1, B, Hkv, S_max, D, generator=g).to(dtype)
    q = (torch.randn(B, n, H, D, generator=g) * 1.5).to(dtype)
    k = torch.randn(B, n, Hkv, D, generator=g).to(dtype)
    v = torch.randn(B, n, Hkv, D, generator=g).to(dtype)
    kc[0, :, :, kv_len:kv_len + n] = k.transpose(1, 2)
    vc[0, :, :, kv_len:kv_len + n] = v.transpose(1, 2)
    exact, bound, vis = BA.attention_fp64(q, kc[0], vc[0], kv_len, n, key_start, dtype)
    assert torch.equal(P.attention_fp64_masked(q, kc[0], vc[0], kv_len, n, key_start), exact)
    total = kv_len + n
    shares = []
    t_mid, t_last = (kv_len // P.KT) // 2, kv_len // P.KT - 1
    for kind in ("edge", t_mid, t_last):
        drop = torch.zeros(B, n, total, dtype=torch.bool)
        if kind == "edge":
            drop[:, torch.arange(n), kv_len + torch.arange(n)] = True
        else:
            drop[:, :, kind * P.KT:(kind + 1) * P.KT] = True
        pert = P.attention_fp64_masked(q, kc[0], vc[0], kv_len, n, key_start, drop)
        over = ((pert - exact).abs() > bound)[vis]
        shares.append(float(over.double().mean()))
    return shares


def test_bound_sensitivity_of_the_gaussian_tests():
    """the measurement of the module docstring of attention_probe_cases.py: a record; asserted only in that neither perturbation is beyond the
    bound everywhere (which is what "orders of magnitude above it" would have meant)"""
    for case in SENSITIVITY_CASES:
        edge, mid, last = sensitivity(case)
        print(f"\n  {case[0]}: beyond the bound -- causal-edge key dropped {edge:.4f}, mid tile dropped {mid:.4f}, last full tile dropped {last:.4f}")
        assert 0.0 <= edge < 1.0 and 0.0 <= mid < 1.0 and 0.0 <= last < 1.0
