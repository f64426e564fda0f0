// sjd_fp8.h -- the saturating fp32 -> OCP e4m3 conversion of the fp8 KV-cache path (F2 into an fp8 cache, K3, K1's q operand).
//
// gfx950's v_cvt_pk_fp8_f32 rounds to nearest even and does NOT saturate: every finite input that rounds above 448, and +-inf, comes out as the
// NaN code 0x7f / 0xff (measured: tests/test_gpu_fp8_range.py on the kernels before this header existed -- 0 of the out-of-range inputs saturated,
// all became the NaN code, and one such byte in a K row makes every query that sees the row NaN).  The contract of the cache writers and of the
// q operand is sat_e4m3: values beyond +-448, +-inf included, give +-448 (0x7e / 0xfe); NaN stays NaN.  In-range bytes are
// those of the bare instruction: (448, 464] rounds to 448 either way, and nothing at or below 448 is touched.
// P (K1's probabilities times 256) is at most 256 by construction and keeps the bare conversion.
#pragma once

__device__ __forceinline__ float sjd_e4m3_clamp(float x)
{
    const float c = __builtin_amdgcn_fmed3f(x, 448.0f, -448.0f);      // (v_med3_f32 returns one of the bounds for a NaN input)
    return x != x ? x : c;
}

// the four values as e4m3 bytes of one dword, a in the low byte
template <bool SAT>
__device__ __forceinline__ unsigned sjd_pack4_e4m3(float a, float b, float c, float d)
{
    if constexpr (SAT) { a = sjd_e4m3_clamp(a); b = sjd_e4m3_clamp(b); c = sjd_e4m3_clamp(c); d = sjd_e4m3_clamp(d); }
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
    return (unsigned)v;
}
