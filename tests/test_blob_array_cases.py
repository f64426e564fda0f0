"""CPU guard of the several-prompt ("blob array") kernel tests: the case tables of tests/blob_array_cases.py hold the conditions that
make the GPU tests bite, and the fp64 reference and the rounding bound are consistent with the oracle before any kernel is involved."""
import pytest
import torch

from oracle.attention_ref import OracleWindowAttention
from tests import blob_array_cases as BA


def _all_cases():
    out = []
    for c in BA.BLOB_CASES:
        out.append(c)
        if c["reverse"]:
            out.append(BA.ordered(c, True))
    return out


@pytest.mark.parametrize("case", _all_cases(), ids=lambda c: c["name"])
def test_case_holds_the_conditions_that_make_it_bite(case):
    kv, rows, nb, W = case["kv"], case["rows"], case["nb"], case["window"]
    assert len(kv) >= 2 and kv[0] != kv[-1], "blob 0 and the last blob must differ, or a lookup that always takes blob 0 passes"
    assert len(set(kv)) == len(kv), "every slot its own kv_len"
    assert all(1 <= r <= W for r in rows) and max(rows) == W
    S = BA.s_max_of(case)
    assert S % 32 == 0 and all(k + W <= S for k in kv), "kv_j + window <= S_max for every slot"
    hidden, pad = BA.hidden_rows(case), BA.padding_rows(case)
    assert (hidden & ~pad).any(), "at least one valid row with no visible key"
    if nb == 2:
        ks = case["key_start"]
        assert all(ks[2 * j] == 0 and ks[2 * j + 1] > 0 for j in range(len(kv))), "non-zero key_start on the uncond row of each CFG pair"
    excluded = (hidden | pad).float().mean()
    assert excluded < 0.5, f"{float(excluded):.2f} of the (batch row, window row) entries are hidden or padding: the case compares too little"
    for form in case["forms"] + case["fp8_forms"]:
        assert form == "colsplit" or isinstance(form, int) or (form[0] == "merged" and form[1] > 1)


def test_tables_cover_the_edges():
    kvs = [k for c in BA.BLOB_CASES for k in c["kv"]]
    assert any(min(k % 32, 32 - k % 32) <= 1 for k in kvs if k > 0), "a kv_len within one of a key-tile edge"
    assert any(1 in c["rows"] for c in BA.BLOB_CASES), "a finished slot's one-row dummy window"
    assert sum(1 in c["rows"] and c["window"] in c["rows"] for c in BA.BLOB_CASES) >= 3, "n_rows differs per blob inside one launch"
    assert 0 in kvs
    # the reversed order puts the distinctive slots on both code paths of the lookup (blob 0 / blob > 0)
    for c in BA.BLOB_CASES[:2]:
        r = BA.ordered(c, True)
        assert c["reverse"] and r["kv"] == c["kv"][::-1] and r["rows"] == c["rows"][::-1]
        assert r["key_start"][:c["nb"]] == c["key_start"][-c["nb"]:]
    assert all(k + 16 <= 1152 for k in BA.F2_SLOT_KV) and len(set(BA.F2_SLOT_KV)) == len(BA.F2_SLOT_KV)


class _Cache:
    def __init__(self, k, v):
        self.k, self.v = k, v


@pytest.mark.parametrize("case", BA.BLOB_CASES, ids=lambda c: c["name"])
def test_oracle_agrees_with_the_fp64_reference_within_the_bound(case):
    """OracleWindowAttention per slot (what test_k1_k3_attention compares K1 with) against the vectorised fp64 reference, inside the
    rounding bound: the oracle's one output rounding is half an ulp, the bound about two"""
    nb, W = case["nb"], case["window"]
    for dtype in case["dtypes"]:
        q, k, v, kc, vc = BA.make_inputs(case, dtype)
        compared = 0
        for j, (kv, n) in enumerate(zip(case["kv"], case["rows"])):
            lo, hi = j * nb, (j + 1) * nb
            ks = case["key_start"][lo:hi]
            cache = _Cache(kc[:, lo:hi].clone(), vc[:, lo:hi].clone())
            ref = OracleWindowAttention()(0, q[lo:hi, :n], k[lo:hi, :n], v[lo:hi, :n], cache, kv, ks)
            assert torch.isfinite(ref.float()).all()
            exact, bound, vis = BA.attention_fp64(q[lo:hi], cache.k[0], cache.v[0], kv, n, ks, dtype)
            assert exact.shape == ref.shape and torch.isfinite(exact).all() and (bound > 0).all()
            assert torch.equal(vis, ~BA.hidden_rows(case)[lo:hi, :n])
            e = (ref.double() - exact).abs()
            assert (e[vis] <= bound[vis]).all(), f"{case['name']} slot {j}: oracle {float((e / bound)[vis].max()):.3f} x the bound"
            assert (exact[~vis] == 0).all() and (ref[~vis] == 0).all()
            # the bound is tight enough to see one key too many or too few: a neighbour's kv_len is far outside it
            if kv > 0 and vis.any():
                other, _, _ = BA.attention_fp64(q[lo:hi], cache.k[0], cache.v[0], kv - 1, n, ks, dtype)
                both = vis & (torch.tensor(kv - 1) + torch.arange(n)[None] >= torch.tensor(ks)[:, None])
                assert ((other - exact).abs()[both] > bound[both]).any()
            compared += int(vis.sum())
        assert compared * 2 > nb * len(case["kv"]) * W


def test_fp8_references_agree_with_each_other():
    """the two fp8 references (kernel arithmetic restated / exact attention over the dequantised cache) differ by far less than the
    tolerance between kernel and exact: what is asserted on the GPU is about the kernel, not about the references"""
    case = BA.BLOB_CASES[0]
    nb = case["nb"]
    q, k, v, kc, vc = BA.make_inputs(case, torch.bfloat16)
    kd, vd = (kc.float() * 1.2).to(BA.FP8).float(), (vc.float() * 1.2).to(BA.FP8).float()
    for j, (kv, n) in enumerate(zip(case["kv"], case["rows"])):
        if kv == 0:
            continue
        lo, hi = j * nb, (j + 1) * nb
        emu, want, conc, vis = BA.attention_fp8_refs(q[lo:hi], kd[0, lo:hi], vd[0, lo:hi], kv, n, case["key_start"][lo:hi])
        assert torch.isfinite(emu).all() and torch.isfinite(want).all() and (conc[vis] > 0).all() and (conc <= 1.0 + 1e-9).all()
        err = (emu - want).abs()
        assert (err.amax(-1) < 0.2 * conc + 1e-2)[vis].all()
