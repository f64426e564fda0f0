"""CPU: tests/fp8_model.py, the saturating e4m3 model the GPU fp8 tests compare against, checked on its own -- against torch's cast where that
cast is right (|x| <= 464), against the stated contract beyond it, and the reason the cache writers are held to x * fl32(1 / scale)."""
import numpy as np
import torch

from tests.fp8_model import e4m3_value, hilo, sat_e4m3_bytes


def _all_16bit_as_f32():
    u = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    bf16 = (u.astype(np.uint32) << 16).view(np.float32)
    with np.errstate(invalid="ignore"):
        fp16 = u.view(np.float16).astype(np.float32)
    return {"bf16": bf16, "fp16": fp16}


def test_model_equals_torch_cast_in_range_and_saturates_beyond():
    for name, x in _all_16bit_as_f32().items():
        got = sat_e4m3_bytes(x)
        assert got.dtype == np.uint8 and got.shape == x.shape
        with np.errstate(invalid="ignore"):
            inr = np.abs(x) <= 464.0                                   # (false for NaN)
        want = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        assert inr.sum() > 30000 and np.array_equal(got[inr], want[inr]), name
        nan = np.isnan(x)
        above = ~inr & ~nan                                             # finite above 464, and +-inf
        assert np.isinf(x[above]).sum() == 2 and above.sum() > 1000
        assert np.array_equal(got[above], np.where(x[above] > 0, 0x7E, 0xFE).astype(np.uint8)), name
        assert nan.sum() > 0 and ((got[nan] & 0x7F) == 0x7F).all(), name
        assert not ((got[~nan] & 0x7F) == 0x7F).any(), name             # nothing but NaN gives the NaN code


def test_model_edges():
    f = lambda *v: sat_e4m3_bytes(np.array(v, dtype=np.float32)).tolist()
    assert f(0.0, -0.0) == [0x00, 0x80]
    assert f(2.0 ** -10, 1.5 * 2.0 ** -10, 2.0 ** -9, 3 * 2.0 ** -10) == [0, 1, 1, 2]      # ties to even at the bottom of the subnormals
    assert f(2.0 ** -6, -(2.0 ** -6), 7.5 * 2.0 ** -9) == [0x08, 0x88, 0x08]                   # minimum normal; the tie below it rounds up into it
    assert f(1.0, 447.0, 448.0, 456.0, 464.0, 472.0, 480.0, 1e4, 3.0e38) == [0x38, 0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0x7E]
    assert f(432.0, 424.0) == [0x7E, 0x7D]                                                    # 432 is the tie between 416 and 448: to the even mantissa
    assert f(-464.0, float("-inf"), float("inf"), -1e30) == [0xFE, 0xFE, 0x7E, 0xFE]
    assert f(1e-30, -1e-30, 1e-45) == [0x00, 0x80, 0x00]
    assert [b & 0x7F for b in f(float("nan"), -float("nan"))] == [0x7F, 0x7F]
    t = sat_e4m3_bytes(torch.tensor([1.0, -2.0, 1000.0]))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.tolist() == [0x38, 0xC0, 0x7E]


def test_value_round_trips_every_code():
    codes = np.arange(256, dtype=np.uint8)
    vals = e4m3_value(codes)
    keep = (codes & 0x7F) != 0x7F
    assert keep.sum() == 254 and np.isnan(vals[~keep]).all() and np.isfinite(vals[keep]).all()
    assert np.array_equal(sat_e4m3_bytes(vals[keep]), codes[keep])
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy()
    assert np.array_equal(vals[keep], want[keep])
    assert vals[0x7E] == 448.0 and vals[0xFE] == -448.0 and vals[0x01] == 2.0 ** -9 and vals[0x08] == 2.0 ** -6


def test_hilo_is_exact_to_2_pow_minus_8_in_range_and_finite_beyond():
    x = _all_16bit_as_f32()["bf16"]
    x = x[np.isfinite(x)]
    v = hilo(x)
    assert v.dtype == np.float64 and np.isfinite(v).all()
    inr = (np.abs(x) <= 448.0) & (np.abs(x) >= 2.0 ** -6)
    assert (np.abs(v[inr] - x[inr]) <= np.abs(x[inr]) * 2.0 ** -8).all()
    big = np.abs(x) >= 476.0                                           # hi = 448 and lo = 448: the largest operand value, 448 + 448 / 16
    assert np.array_equal(v[big], np.sign(x[big]) * 476.0)
    assert hilo(torch.tensor([448.0, 449.0, 464.0, 2000.0, -60000.0, 1e30])).tolist() == [448.0, 449.0, 464.0, 476.0, -476.0, 476.0]


def test_multiply_by_reciprocal_is_not_the_division():
    """The cache writers compute x * fl32(1 / scale) (one fp32 multiply by a reciprocal formed on the host), not x / scale: at a calibrated
    scale (never a power of two) the two differ in the last fp32 bit often enough to land on different sides of an e4m3 rounding boundary, so a
    byte-exact reference has to use the multiply."""
    x = _all_16bit_as_f32()["bf16"]
    x = x[np.isfinite(x)]
    s = np.float32(1.7)
    inv = np.float32(1.0) / s
    with np.errstate(over="ignore"):
        mul, div = (x * inv).astype(np.float32), (x / s).astype(np.float32)
    n = int((sat_e4m3_bytes(mul) != sat_e4m3_bytes(div)).sum())
    assert n >= 1
    # ... and never at a power of two, which is why the suite could not see it before
    for p2 in (0.25, 0.5, 2.0):
        s = np.float32(p2)
        with np.errstate(over="ignore"):
            assert np.array_equal(sat_e4m3_bytes((x * (np.float32(1.0) / s)).astype(np.float32)), sat_e4m3_bytes((x / s).astype(np.float32)))
