"""CPU: the exact-operand construction of tests/gemm_exact_cases.py holds what tests/test_gpu_gemm_exact.py relies on, before any kernel is involved --
the weights pack without loss into every compressed stream at every shape the GPU file uses, fp32 accumulation is exact on the operands in three
different orders (which proves the precondition, not a kernel), the exact check rejects every planted defect even in a row 2^-20 of the rest (where
the old 2e-3 anchor is blind), and the wide-range bound separates fp32 accumulation from bf16 accumulation."""
import numpy as np
import pytest
import torch

import sjd_amd.ops as ops
from tests import gemm_exact_cases as C
from tests.glue_models import PLANE_SENTINEL
from tests.test_pack_z import decode_z, raw_stream

PACKERS = dict(q8=ops.pack_weight_q8, q4=ops.pack_weight_q4, q6=ops.pack_weight_q6)


def _bits(t):
    return t.view(torch.int16)


def _assert_lossless(stream, w, KC, sm, gateup=False):
    pk = PACKERS[stream](w, KC, sm, gateup=gateup)
    assert torch.equal(_bits(pk.dequant()), _bits(w)), f"{stream}: dequant() is not the weight"
    assert pk.stats["rel_rms_error"] == 0


# ------------------------------------------------------------------------------------------------ lossless packing
@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("N,K,KC", C.QUANT_SHAPES)
@pytest.mark.parametrize("stream", ["q8", "q4", "q6"])
def test_quantised_streams_hold_the_exact_weight_without_loss(stream, N, K, KC, sm):
    _, w, _ = C.g1_case(stream, N, K, KC)
    _assert_lossless(stream, w, KC, sm)


@pytest.mark.parametrize("stream,name", [("q8", "small"), ("q4", "small"), ("q6", "small"), ("q4", "k4")])
def test_quantised_gateup_weights_pack_without_loss(stream, name):
    inter, hidden, chunks, _, _ = C.GATEUP_SHAPES[name]
    _, w, _ = C.gateup_case(stream, name, 32)
    for sm in (False, True):
        _assert_lossless(stream, w, hidden // chunks, sm, gateup=chunks == 2)


def test_one_exponent_per_32_consecutive_k_is_what_e2m3_cannot_hold():
    """why `be` is drawn per 64-k record: the e2m3 stream's scale blocks interleave across a record (k = 64 R + 16 u + 8 h + j), so a weight whose
    exponent changes every 32 consecutive k puts two exponents into one block -- nine binades apart here, more than the format's grid spans"""
    w = torch.ones(32, 128)
    w[:, 32:64] = 2.0 ** 9
    w[:, 0] = 0.5
    w = w.to(torch.bfloat16)
    assert torch.equal(ops.pack_weight_q4(w, 128).dequant(), w)
    assert not torch.equal(ops.pack_weight_q6(w, 128).dequant(), w)


@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("N,K,KC", C.SHAPES)
@pytest.mark.parametrize("kind", C.Z_KINDS)
def test_12bit_stream_reads_back_the_exact_weight(kind, N, K, KC, sm):
    """PackedZ has no read-back of its own: tests/test_pack_z.py's restatement of the kernel's decoder is the CPU read-back.  Also: each kind is what
    its name says (no exceptions / exceptions in headers / raw units), so the GPU file reaches those three paths."""
    _, w, _ = C.g1_case("z_" + kind, N, K, KC)
    pz = ops.pack_weight_z(w, KC, sm)
    assert pz is not None and np.array_equal(decode_z(pz), raw_stream(w, KC, sm))
    if kind == "clean":
        assert pz.n_exceptions == 0 and pz.n_raw == 0
    elif kind == "outliers":
        assert pz.n_exceptions > 0 and pz.n_raw == 0
    else:
        assert pz.n_raw == pz.stats["units"]


@pytest.mark.parametrize("kind,name", [(k, n) for k in C.Z_KINDS for n in ("small", "tall64")])
def test_12bit_gateup_weights_read_back(kind, name):
    inter, hidden, chunks, _, _ = C.GATEUP_SHAPES[name]
    _, w, _ = C.gateup_case("z_" + kind, name, 32)
    pz = ops.pack_weight_z(w, hidden // 2, True, gateup=True)
    assert np.array_equal(decode_z(pz), raw_stream(w, hidden // 2, True))
    assert (pz.n_raw > 0) == (kind == "raw") and (pz.n_exceptions > 0 or kind != "outliers")


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("order", C.ORDERS)
@pytest.mark.parametrize("N,K,KC", C.SHAPES)
@pytest.mark.parametrize("stream", ["bf16", "fp16", "z_raw"])
def test_fp32_accumulation_is_exact_in_any_order(stream, N, K, KC, order):
    """forward, reversed and 16-wide k-steps summed pairwise: the same bits as the fp64 sum.  Rows 0 and 1 are the exponent range's two ends."""
    x, w, exact = C.g1_case(stream, N, K, KC)
    got = C.emulate_planes(x[:6], w, KC, order)
    assert C.first_mismatch(got, exact[:, :6], f"{stream} {order}") is None


@pytest.mark.parametrize("name", list(C.GATEUP_SHAPES))
def test_gateup_operands_are_exact_too(name):
    """hidden 4096 / 8192 meet the precondition with a narrower record exponent; reversed order at K = 8192 is the longest sum any case forms"""
    x, w, exact = C.gateup_case("q4" if name == "k4" else "bf16", name, 32)
    inter, hidden, chunks, _, _ = C.GATEUP_SHAPES[name]
    for order in ("reversed", "pairwise16"):
        assert C.first_mismatch(C.emulate_planes(x[:2], w, hidden // chunks, order), exact[:, :2], f"{name} {order}") is None


def test_the_precondition_is_asserted():
    C.exact_operands(torch.bfloat16, 2, 32, C.K_MAX - C.K_MAX % 2, 0, 0, 0)
    with pytest.raises(AssertionError, match="units of the smallest product"):
        C.exact_operands(torch.bfloat16, 2, 32, C.K_MAX + 6, 0, 0, 0)
    with pytest.raises(AssertionError, match="exponents outside"):
        C.exact_operands(torch.float16, 2, 32, 64, 0, -15, 0)
    with pytest.raises(AssertionError, match="exponents outside"):
        C.exact_operands(torch.float16, 2, 32, 64, 0, 0, 8)


def test_every_block_scale_is_forced():
    """each MXFP4 block and each e2m3 block (lane half of a record) holds a 6 and a 0.5 times the record's power of two"""
    _, w, _ = C.g1_case("q4", 96, 384, 256)
    a = w.double().abs()
    q4 = a.reshape(96, -1, 32)
    q6 = ops._q6_block_view(a, 384)
    for blk in (q4, q6):
        amax = blk.amax(-1)
        amin = torch.where(blk > 0, blk, torch.full_like(blk, float("inf"))).amin(-1)
        assert torch.equal(amax, 12 * amin)


# ------------------------------------------------------------------------------------------------ planted defects
N_, K_, KC_ = 96, 176, 64          # chunks of 4, 4 and 3 k-steps
SMALL_ROW = 3


def _defect_operands(small):
    rows = torch.zeros(8, dtype=torch.int32)
    if small:
        rows[SMALL_ROW] = -20
    return C.exact_operands(torch.bfloat16, 8, N_, K_, 11, rows, -8)          # (columns at 2^-8: plane sums of order one, as in the old anchor's operands)


@pytest.mark.parametrize("name", list(C.DEFECTS))
def test_every_planted_defect_fails_the_exact_check(name):
    x, w = _defect_operands(False)
    exact = C.exact_planes(x, w, KC_)
    assert C.first_mismatch(C.emulate_planes(x, w, KC_), exact, "correct") is None
    msg = C.first_mismatch(C.planted(name, x, w, KC_), exact, name)
    assert msg is not None and "chunk" in msg and "row" in msg and "column" in msg and name in msg


@pytest.mark.parametrize("name", list(C.DEFECTS))
def test_a_defect_in_a_row_2_to_the_minus_20_of_the_rest_still_fails(name):
    x, w = _defect_operands(True)
    exact = C.exact_planes(x, w, KC_)
    msg = C.first_mismatch(C.planted(name, x, w, KC_, rows=[SMALL_ROW]), exact, name)
    assert msg is not None and f"row {SMALL_ROW}" in msg


def test_the_old_anchor_is_blind_in_a_small_row_and_to_a_moved_k_step():
    """test_g1_skinny_gemm's check -- sum(0) against an fp32 matmul at atol = rtol = 2e-3 -- passes a k-step dropped in the small row, and passes a
    k-step credited to the neighbouring plane in EVERY row (it cancels in the sum)"""
    x, w = _defect_operands(True)
    ref = x.float() @ w.float().t()
    assert float(ref.abs().max()) > 1          # the other rows are of the old operands' order
    for name, rows in (("drop_step", [SMALL_ROW]), ("next_plane", None), ("swap_planes", None)):
        torch.testing.assert_close(C.planted(name, x, w, KC_, rows=rows).sum(0), ref, atol=2e-3, rtol=2e-3)
    with pytest.raises(AssertionError):          # ... while the same drop in every row is what it does see
        torch.testing.assert_close(C.planted("drop_step", x, w, KC_).sum(0), ref, atol=2e-3, rtol=2e-3)


# ------------------------------------------------------------------------------------------------ the wide-range bound
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_wide_range_bound_holds_for_fp32_and_fails_for_bf16_accumulation(dtype):
    N, K, KC = C.BOUND_SHAPE
    rr, cr = C.WIDE_EXP_RANGE[dtype]
    x, w = C.wide_range_operands(dtype, 8, N, K, 5, C.spread_exps(8, *rr, 6), C.spread_exps(N, *cr, 7))
    exact, bound = C.plane_bounds(x, w, KC)
    assert float((bound > 0).double().mean()) > 0.99
    bound = bound.clamp_min(1e-300)          # (an all-zero column: error and bound are both zero)
    for order in C.ORDERS:
        ratio = ((C.emulate_planes(x, w, KC, order).double() - exact).abs() / bound).max()
        assert float(ratio) < 0.25, (order, float(ratio))          # a margin of four: sequential fp32 sums use a fraction of the worst case
    ratio = ((C.emulate_planes(x, w, KC, "forward", acc=torch.bfloat16).double() - exact).abs() / bound).max()
    assert float(ratio) > 1, float(ratio)


# ------------------------------------------------------------------------------------------------ the guarded buffer
def test_guarded_planes_report_what_a_launch_did_wrong():
    dev, M = torch.device("cpu"), 5

    def filled(poison=PLANE_SENTINEL):
        g = C.guarded_planes(2, 32, 64, dev, poison)
        assert g.untouched() and g.ptr() == g.buf.data_ptr() + 4 * g.guard
        g.planes[:, :M] = 1.0
        g.planes[:, M:] = 0.0
        return g
    assert filled().problems(M) == [] and filled(float("nan")).problems(M) == []
    g = filled()
    g.front[-1] = 0.0
    assert "in front of" in g.problems(M)[0]
    g = filled()
    g.behind[0] = 0.0
    assert "behind" in g.problems(M)[0]
    g = filled()
    g.planes[1, M + 1, 3] = 1e-30
    assert "pad rows" in g.problems(M)[0]
    g = filled()
    g.planes[1, 2, 7] = PLANE_SENTINEL
    assert "chunk 1 row 2 column 7" in g.problems(M)[0]
    g = filled(float("nan"))
    g.planes[0, 0, 0] = float("inf")
    assert "non-finite" in g.problems(M)[0]
