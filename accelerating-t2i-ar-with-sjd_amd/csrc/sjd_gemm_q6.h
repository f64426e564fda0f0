// sjd_gemm_q6.h -- G1q6 / G1sq6: the window projections streamed from 6-bit weights (OCP e2m3 codes, one e8m0 scale per 32 weights): 6.25 bits per
// weight.  Included by sjd_gemm.hip behind sjd_gemm_qblock.h: the kernels are its templates over G1Q6Stream (below), the ones the MXFP4 stream
// (sjd_gemm_q4.h) instantiates too; the format, its decode and the launchers are here.
//
// The format (sjd_amd.ops.pack_weight_q6): ONE buffer = the code records (N_packed * K * 3 / 4 bytes), then the scale bytes (N_packed * K / 32) behind
// them.  Weight w[n][k] is stored as code q (sign, 2 exponent bits, 3 mantissa bits: 0 .. 7.5) times the scale 2^(byte - 127) of its BLOCK, so q * scale
// is exactly a bf16 value: the kernels rebuild the bf16 MFMA operand bit for bit and run the MFMA sequence of G1 / G1s, so the planes / the 16-bit
// output are those of sjd_skinny_gemm / sjd_gateup_silu on pack_weight(q * scale), bit for bit.  All the loss is in the host-side quantiser.
//   THE BLOCK is what ONE v_cvt_scalef32_pk32_bf16_fp6 decodes: 32 codes in six VGPRs times one scale per lane -> 32 bf16 in sixteen VGPRs.  Lane
//       l = 32 h + r of k-step s holds q[32 t + r][k0 + 16 s + 8 h + j], j = 0..7, so the conversion fills a lane's B operands of FOUR k-steps:
//       block (column, record R of 64 k, lane half h) = the weights at k = 64 R + 16 u + 8 h + j, u = 0..3 -- NOT 32 consecutive k: a private stream
//       format, not an interchange format.  Element e = 8 u + j of the conversion is code bits [6 e, 6 e + 6) of the 192, little-endian; VGPR quad
//       4 u .. 4 u + 3 of its result is the B operand of k-step 4 R + u.
//   K GRANULE 128 (as the MXFP4 stream's): K and every chunk are multiples of 128 columns = two records = one scale dword per column.  No tail path.
//   RECORD R (1536 B) = k-steps 4R .. 4R + 3: 64 lanes x 16 B {the lane's code dwords 0..3}, then 64 lanes x 8 B {dwords 4, 5} -- one aligned
//       16-byte and one aligned 8-byte load per lane (the shape of the 12-bit stream's record pair); a chunk starts at byte k0 * N_packed * 3 / 4;
//   tile-major: a unit is S * 384 contiguous bytes; step-major: the chunk holds record 0 of every tile, record 1 of every tile, ...
//   scales, at byte N_packed * K * 3 / 4: per unit and TRIP q (two records) 128 bytes = 32 columns x 4 bytes, byte 2 i + h of column r = the e8m0
//       scale of block (r, record 2 q + i, half h) -- a lane takes a trip's scales with one aligned dword load and shifts its half's bytes down;
//       the trips of a unit are laid out like MXFP4's (a chunk starts at scale byte k0 * N_packed / 32).
// bf16; M <= 64 (G1q6) / M <= 32, K in {512, 1024, 2048, 4096} (G1sq6): see the launchers.  No wide (65..256-row), K = 8192 or prefill form.
#pragma once

typedef __attribute__((ext_vector_type(6))) int g1q6_i32x6;
typedef __attribute__((ext_vector_type(32))) __bf16 g1q6_bf16x32;
struct g1q6_rec { u32x4 lo; u32x2 hi; };          // a lane's six code dwords of one record
struct g1q6_ops { u32x4 b[4]; };                  // ... decoded: the B operands of its four k-steps

// the record's 32 weights of this lane as bf16: one conversion
__device__ __forceinline__ g1q6_ops g1q6_operands(const g1q6_rec &c, float sc)
{
    const g1q6_i32x6 v = {(int)c.lo.x, (int)c.lo.y, (int)c.lo.z, (int)c.lo.w, (int)c.hi.x, (int)c.hi.y};
    return __builtin_bit_cast(g1q6_ops, (g1q6_bf16x32)__builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(v, sc));
}

// one HALF TRIP: the eight k-steps of two ring records against the scale dword `sd`, already shifted down by 8 h (bytes 0 and 2: the lane half's
// scales of the two records; the e8m0 byte IS the float's exponent field); a_read(a, u) fetches the A fragments of the trip's k-step u (the next one
// is read ahead of the current MFMA); the caller refills the two records and the dword behind it
template <int MT, typename AR>
__device__ __forceinline__ void g1q6_half_trip(f32x16 (&acc)[MT], const g1q6_rec &rec0, const g1q6_rec &rec1, unsigned sd, AR a_read)
{
    constexpr int DT = SJD_DTYPE_BF16;
    u32x4 a[2][MT];
    a_read(a[0], 0);
    const g1q6_ops b0 = g1q6_operands(rec0, __builtin_bit_cast(float, (sd << 23) & 0x7f800000u));
    const g1q6_ops b1 = g1q6_operands(rec1, __builtin_bit_cast(float, (sd << 7) & 0x7f800000u));
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (u + 1 < 8) a_read(a[(u + 1) & 1], u + 1);
        const u32x4 b = u < 4 ? b0.b[u & 3] : b1.b[u & 3];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a[u & 1][mt], b, acc[mt]);
    }
}

// the stream as the kernels of sjd_gemm_qblock.h take it
struct G1Q6Stream {
    using rec = g1q6_rec;
    static constexpr int REC_BYTES = 1536, TILE_K_BYTES = 24;
    static constexpr int DEPTH = 16;                  // a ring of four records (6 KiB per wave)
    static __device__ __forceinline__ rec load(__amdgpu_buffer_rsrc_t wr, int lane, unsigned byte_off)
    {
        rec v;
        v.lo = __builtin_amdgcn_raw_buffer_load_b128(wr, (unsigned)lane * 16u + byte_off, 0u, G1Z_AUX);
        v.hi = __builtin_amdgcn_raw_buffer_load_b64(wr, 1024u + (unsigned)lane * 8u + byte_off, 0u, G1Z_AUX);
        return v;
    }
    static __device__ __forceinline__ unsigned lane_scales(unsigned sd, unsigned hsh) { return sd >> hsh; }      // (the lane half's bytes down to 0 and 2)
    template <int MT, typename AR>
    static __device__ __forceinline__ void half_trip(f32x16 (&acc)[MT], const rec &rec0, const rec &rec1, unsigned sd, AR a_read) { g1q6_half_trip<MT>(acc, rec0, rec1, sd, a_read); }
};

// SJD_G1_W6_E2M3 on sjd_skinny_gemm / sjd_skinny_gemm_cols: g1qb_launch's shapes (M <= 64), K and KC multiples of 128.  No form for more rows.
static int g1q6_launch(const void *x, const void *wq, float *out, int M, int N, int K, int KC, int waves, int step_major, int n_tiles, int tile0,
                       hipStream_t s)
{
    return g1qb_launch<G1Q6Stream>(x, wq, out, M, N, K, KC, waves, step_major, n_tiles, tile0, s,
        [&] { return ((K % 128) != 0 || (KC % 128) != 0 || M > 64) ? (int)SJD_ERR_UNSUPPORTED : G1_STREAM_GO; });
}

// SJD_G1_W6_E2M3 on sjd_gateup_silu: g1sqb_launch's shapes (M <= 32, K in {512, 1024, 2048, 4096})
static int g1sq6_launch(const void *x, const void *wq, void *y, int M, int I, int K, int step_major, const sjd_row_norm *rn, hipStream_t s)
{
    return g1sqb_launch<G1Q6Stream>(x, wq, y, M, I, K, step_major, rn, s);
}
