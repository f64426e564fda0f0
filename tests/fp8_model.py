"""An independent model of the saturating OCP e4m3 conversion the fp8 KV-cache path is held to, in fp64 / integer
arithmetic -- no call to torch's cast, which does not saturate (464 -> 0x7e, 480 -> 0x7f) and so cannot serve beyond the range.

e4m3 (OCP "fn"): 1 sign, 4 exponent (bias 7), 3 mantissa bits; minimum normal 2^-6, subnormal step 2^-9, largest finite value 448 (0x7e);
exponent 15 with mantissa 7 is the only NaN (0x7f / 0xff), there is no infinity.

  sat_e4m3_bytes(x)   fp32 -> byte: round to nearest, ties to even; every finite value that would round above 448, and +-inf, gives +-448;
                      NaN gives the NaN code with the input's sign; -0 gives 0x80
  e4m3_value(b)       byte -> fp32 value (NaN for the two NaN codes)
  hilo(x)             the value hi + lo / 16 of K1's two on-chip e4m3 operands: hi = sat_e4m3(x), lo = sat_e4m3(16 (x - hi)), the residual and its
                      scaling evaluated in fp32 as the kernel does
"""
import numpy as np
import torch

E4M3_MAX = 448.0
NAN_CODE = 0x7F


def _as_f32(x):
    if isinstance(x, torch.Tensor):
        assert x.dtype == torch.float32 and not x.is_cuda, "fp32 CPU tensor"
        return x.detach().contiguous().numpy(), True
    x = np.asarray(x)
    assert x.dtype == np.float32, "fp32 array"
    return np.ascontiguousarray(x), False


def _sat_bytes(x):
    sign = ((x.view(np.uint32) >> 31) << 7).astype(np.uint8)
    nan = np.isnan(x)
    with np.errstate(invalid="ignore"):                          # (signalling NaN patterns)
        a = np.abs(x).astype(np.float64)
    a = np.where(np.isfinite(a), a, 1e9)                        # inf saturates like any value above the range (NaN: overwritten below)
    _, e = np.frexp(a)                                           # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    e = np.maximum(e - 1, -6)                                    # below 2^-6 the subnormals keep the step of the lowest binade
    step = np.ldexp(1.0, e - 3)                                  # three mantissa bits: 8 steps per binade, 2^-9 at the bottom
    v = np.minimum(np.rint(a / step) * step, E4M3_MAX)           # a / step is exact (a power of two); rint: ties to even = even mantissa
    _, ev = np.frexp(v)
    ev = ev - 1
    normal = v >= 2.0 ** -6
    mant_n = (v / np.ldexp(1.0, np.where(normal, ev, 0) - 3)).astype(np.int64) - 8
    code_n = ((np.where(normal, ev, 0) + 7) << 3) | np.where(normal, mant_n, 0)
    code_s = (v * 2.0 ** 9).astype(np.int64)                     # subnormals (and zero): mantissa = v / 2^-9, exponent field 0
    code = np.where(normal, code_n, code_s).astype(np.uint8)
    code = np.where(nan, np.uint8(NAN_CODE), code)
    return (code | sign).astype(np.uint8)


def sat_e4m3_bytes(x):
    """fp32 numpy array or CPU tensor -> uint8 of the same kind and shape"""
    a, is_t = _as_f32(x)
    out = _sat_bytes(a)
    return torch.from_numpy(out) if is_t else out


def _value(b):
    b = b.astype(np.int64)
    s = np.where(b & 0x80, -1.0, 1.0)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * np.ldexp(1.0, e - 10))
    v = np.where((e == 15) & (m == 7), np.nan, v)
    return (s * v).astype(np.float32)


def e4m3_value(b):
    """uint8 numpy array or CPU tensor -> the fp32 values of the e4m3 bytes"""
    if isinstance(b, torch.Tensor):
        assert b.dtype == torch.uint8 and not b.is_cuda
        return torch.from_numpy(_value(b.contiguous().numpy()))
    b = np.asarray(b)
    assert b.dtype == np.uint8
    return _value(b)


def hilo(x):
    """fp32 -> fp64 value of the saturating hi / lo operand pair (kernel K1's q and P operands over an fp8 cache)"""
    a, is_t = _as_f32(x)
    hi = _value(_sat_bytes(a))
    with np.errstate(over="ignore", invalid="ignore"):
        res = ((a - hi).astype(np.float32) * np.float32(16.0)).astype(np.float32)      # two fp32 operations, as in the kernel
    lo = _value(_sat_bytes(res))
    out = hi.astype(np.float64) + lo.astype(np.float64) / 16.0
    return torch.from_numpy(out) if is_t else out
