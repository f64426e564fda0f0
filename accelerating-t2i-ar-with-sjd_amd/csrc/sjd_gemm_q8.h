// sjd_gemm_q8.h -- G1q / G1sq: the window projections streamed from 8-bit (OCP e4m3fn) weights, one byte per weight.  Included by
// sjd_gemm.hip behind the declarations it shares with G1 / G1z (g1_slot, G1Mfma, g1z_unit_rsrc, the ring depth and cache policy).
//
// The format (sjd_amd.ops.pack_weight_q8): ONE buffer = the records, then the fp32 column scales [N_packed] at byte offset N_packed * K.
// Column n of the weight is stored as q[n][k] = e4m3(w[n][k] / scale[n]) with scale[n] a power of two, so q * scale is exactly a bf16 value:
// the kernels rebuild the bf16 MFMA operand bit for bit (v_cvt_scalef32_pk_bf16_fp8, the scale in the conversion: four conversions per eight
// weights against twelve VALU of the 12-bit decode) and run the MFMA sequence of G1 / G1s, so the planes / the 16-bit output are those of
// sjd_skinny_gemm / sjd_gateup_silu on pack_weight(q * scale), bit for bit.  All the loss is in the host-side quantiser.
//   unit (k-chunk c, 32-column tile t), S = its k-steps: record s, lane l, byte j = q[32 t + (l & 31)][k0 + 16 s + 8 (l >> 5) + j] (pack_weight's
//       element order at one byte each; a chunk starts at byte k0 * N_packed);
//   record PAIR p (1024 B) = k-steps 2p and 2p + 1: 64 lanes x 16 B {bytes 0..7 of k-step 2p, bytes 0..7 of k-step 2p + 1} -- one aligned
//       16-byte load per lane;
//   an odd last k-step (S odd: a ragged last chunk) is a HALF record of 512 B = 64 lanes x 8 B behind the unit's pairs -- no padding, the
//       buffer holds exactly N * K weight bytes;
//   tile-major: a unit is S * 512 contiguous bytes (pairs, then the half record); step-major: the chunk holds pair 0 of every tile, pair 1
//       of every tile, ..., then the half record of every tile.
// No headers, no exceptions, no raw units, no fix-up launch.  bf16; M <= 64 (G1q) / M <= 32 (G1sq): see the launchers.  65..256 rows: kernel G1wq, the
// 8-bit form of G1w (csrc/sjd_gemm_wide.h, template parameter Q), for K and KC multiples of 32 (whole pairs, no half records).
#pragma once

typedef __attribute__((ext_vector_type(2))) __bf16 g1q_bf16x2;

// the MFMA B operand (eight bf16) of one k-step from its eight e4m3 bytes and the column's scale
__device__ __forceinline__ u32x4 g1q_operand(unsigned b0, unsigned b1, float sc)
{
    u32x4 d;
    d.x = __builtin_bit_cast(unsigned, (g1q_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b0, sc, false));
    d.y = __builtin_bit_cast(unsigned, (g1q_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b0, sc, true));
    d.z = __builtin_bit_cast(unsigned, (g1q_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b1, sc, false));
    d.w = __builtin_bit_cast(unsigned, (g1q_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b1, sc, true));
    return d;
}

// G1q: g1z_skinny_gemm's structure (whole activation chunk in LDS, one buffer descriptor per unit, a ring of G1Z_DEPTH k-steps refilled
// unconditionally behind its consumer, non-temporal loads) over the 8-bit stream.  The ring carries the unit's WHOLE pairs; the half record
// of an odd unit is one 8-byte load through a descriptor of its own (empty when the unit has none) and its MFMA comes last, in k order.
template <int MT, int MAXT>
__global__ __launch_bounds__(MAXT) void g1q_skinny_gemm(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wq,
                                                        const float *__restrict__ scales, float *__restrict__ out, int M, int N, int K, int KC,
                                                        int n_tiles, int rec_stride, int tile0, int n_waves)
{
    constexpr int DT = SJD_DTYPE_BF16;
    constexpr int D = MAXT <= 512 ? G1Z_DEPTH : (G1Z_DEPTH < 8 ? G1Z_DEPTH : 8);
    constexpr int DP = D / 2;
    constexpr int TL = D < 8 ? 8 : D;
    static_assert(D % 2 == 0 && TL % 8 == 0 && TL % D == 0, "g1_slot(.., s) depends on s & 7: a trip starts at a multiple of eight");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);
    const int chunk = blockIdx.y;
    const int k0 = chunk * KC;
    const int steps = min(KC, K - k0) / 16;
    const int npf = steps >> 1;                                   // whole record pairs of this unit
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int t_out = blockIdx.x * n_waves + w;
    const bool has_tile = t_out < N / 32;
    const int t = has_tile ? tile0 + t_out : 0;
    const unsigned char *cb = wq + (size_t)k0 * ((size_t)n_tiles * 32);
    const unsigned rsb = (unsigned)rec_stride * 1024u;           // bytes from a pair of the unit to the next
    const unsigned char *first = cb + (rec_stride == 1 ? (size_t)t * steps * 512 : (size_t)t * 1024);
    const unsigned char *half = cb + (rec_stride == 1 ? (size_t)t * steps * 512 + (size_t)npf * 1024 : (size_t)npf * n_tiles * 1024 + (size_t)t * 512);
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(first, (has_tile && npf > 0) ? (unsigned)(npf - 1) * rsb + 1024u : 0u);
    const __amdgpu_buffer_rsrc_t wh = g1z_unit_rsrc(half, (has_tile && (steps & 1)) ? 512u : 0u);
    auto w_load = [&](int p) -> u32x4 { return __builtin_amdgcn_raw_buffer_load_b128(wr, (unsigned)lane * 16u, (unsigned)p * rsb, G1Z_AUX); };
    u32x4 ring[DP];
    const int ppr = 2 * steps;
    const int nth = n_waves * 64;
    constexpr int STAGE = MAXT <= 512 ? 2 * G1_STAGE : G1_STAGE;
    const int dm = nth / ppr, dj = nth - dm * ppr;
    int pm = threadIdx.x / ppr, pj = threadIdx.x - pm * ppr;
    auto advance = [&](int &m, int &j) { m += dm; j += dj; if (j >= ppr) { j -= ppr; ++m; } };
    auto x_load = [&](int m, int j) -> u32x4 {
        return (m < M) ? *reinterpret_cast<const u32x4 *>(x + (size_t)m * K + k0 + 8 * j) : u32x4{0u, 0u, 0u, 0u};
    };
    auto x_store = [&](int m, int j, u32x4 val) {
        const int s = j >> 1;
        if (m < 32 * MT) xl[((m >> 5) * steps + s) * 64 + g1_slot(j & 1, m & 31, s)] = val;
    };
    float sc;
    u32x2 hrec;
    {   // first activation batch, the column's scale, the first D k-steps and the half record right behind it (all unconditional)
        u32x4 val[STAGE];
        int m = pm, j = pj;
#pragma unroll
        for (int i = 0; i < STAGE; ++i) { val[i] = x_load(m, j); advance(m, j); }
        sc = scales[32 * t + (lane & 31)];
#pragma unroll
        for (int u = 0; u < DP; ++u) ring[u] = w_load(u);
        hrec = __builtin_amdgcn_raw_buffer_load_b64(wh, (unsigned)lane * 8u, 0u, G1Z_AUX);
        m = pm; j = pj;
#pragma unroll
        for (int i = 0; i < STAGE; ++i) { x_store(m, j, val[i]); advance(m, j); }
        pm = m; pj = j;
    }
    while (pm < 32 * MT) {
        u32x4 val[G1_STAGE];
        int m = pm, j = pj;
#pragma unroll
        for (int i = 0; i < G1_STAGE; ++i) { val[i] = x_load(m, j); advance(m, j); }
        m = pm; j = pj;
#pragma unroll
        for (int i = 0; i < G1_STAGE; ++i) { x_store(m, j, val[i]); advance(m, j); }
        pm = m; pj = j;
    }
    __syncthreads();
    if (!has_tile) return;
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;
    const int xs = steps * 64;
    auto a_read = [&](u32x4 (&a)[MT], int s, int u) {          // (the address stays inside the staged chunk)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = xl[mt * xs + min(s, steps - 1) * 64 + g1_slot(lane >> 5, lane & 31, u)];
    };
    // ring trips of D k-steps: a consumed pair is refilled with the one D k-steps further on, after it was consumed and unconditionally (a
    // pair past the unit's end costs an instruction, no traffic); the pairs of the last trip that lie past the unit are skipped by uniform branches
    const int sw = 2 * npf;
    for (int s0 = 0; s0 < sw; s0 += TL) {
        u32x4 a0[MT], a1[MT];
        a_read(a0, s0, 0);
#pragma unroll
        for (int u = 0; u < TL / 2; ++u) {
            const int sa = s0 + 2 * u, sb = sa + 1;
            u32x4 &slot = ring[u % DP];
            u32x4 b1 = {0u, 0u, 0u, 0u};
            if (sa < sw) {
                a_read(a1, sb, 2 * u + 1);
                const u32x4 b0 = g1q_operand(slot.x, slot.y, sc);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a0[mt], b0, acc[mt]);
                if (u + 1 < TL / 2) a_read(a0, sb + 1, 2 * u + 2);
                b1 = g1q_operand(slot.z, slot.w, sc);
            }
            slot = w_load(s0 / 2 + u + DP);
            if (sa < sw) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a1[mt], b1, acc[mt]);
            }
        }
    }
    if (steps & 1) {                                              // the half record: the unit's last k-step
        u32x4 a0[MT];
        a_read(a0, steps - 1, (steps - 1) & 7);
        const u32x4 b0 = g1q_operand(hrec.x, hrec.y, sc);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a0[mt], b0, acc[mt]);
    }
    float *o = out + ((size_t)chunk * (32 * MT)) * N + (size_t)t_out * 32 + (lane & 31);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            o[(size_t)m * N] = acc[mt][r];
        }
}

// G1sq: g1z_gateup_silu over the 8-bit stream -- eight waves = two K halves x {gate, up} x two column tiles, two activation phases per K
// half, the epilogue of sjd_mlp_epilogue.h on the planes in LDS.  A K half has 2 SP k-steps (K / 32: always even -- no half records).
template <int SP>
__global__ __launch_bounds__(512) void g1q_gateup_silu(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wq,
                                                       const float *__restrict__ scales, unsigned short *__restrict__ y, int M, int I, int K,
                                                       int rec_stride, const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden,
                                                       float rs_eps)
{
    constexpr int DT = SJD_DTYPE_BF16;
    constexpr int D = SP >= G1Z_DEPTH ? G1Z_DEPTH : 8;
    constexpr int DP = D / 2;
    constexpr int TL = D < 8 ? 8 : D;
    static_assert(SP % TL == 0 && TL % 8 == 0 && TL % D == 0 && D % 2 == 0, "a phase is whole trips; g1_slot(.., s) depends on s & 7");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);
    __shared__ float rsc[32];
    constexpr int PPS = 2 * SP;
    constexpr int NPT = (32 * 2 * PPS) / 512;
    static_assert(NPT >= 1, "at least one piece per thread");
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int kh = w >> 2, q = w & 3;
    const int n_gate = I / 32, n_tiles = 2 * n_gate;
    const int t_act = 2 * blockIdx.x + (q & 1);
    const int t = (q < 2 ? 0 : n_gate) + t_act;
    constexpr int pairs = SP;                                     // record pairs of a K half (2 SP k-steps)
    const unsigned char *cb = wq + (size_t)kh * (K / 2) * ((size_t)n_tiles * 32);
    const unsigned rsb = (unsigned)rec_stride * 1024u;
    const unsigned char *first = cb + (rec_stride == 1 ? (size_t)t * pairs * 1024 : (size_t)t * 1024);
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(first, (unsigned)(pairs - 1) * rsb + 1024u);
    auto w_load = [&](int p) -> u32x4 { return __builtin_amdgcn_raw_buffer_load_b128(wr, (unsigned)lane * 16u, (unsigned)p * rsb, G1Z_AUX); };
    auto x_load = [&](int ph, int i) -> u32x4 {
        const int v = i * 512 + threadIdx.x;
        const int m = v / (2 * PPS), hh = (v / PPS) & 1, j = v % PPS;
        return (m < M) ? *reinterpret_cast<const u32x4 *>(x + (size_t)m * K + hh * (K / 2) + ph * (K / 4) + 8 * j) : u32x4{0u, 0u, 0u, 0u};
    };
    auto x_store = [&](int i, u32x4 val) {
        const int v = i * 512 + threadIdx.x;
        const int m = v / (2 * PPS), hh = (v / PPS) & 1, j = v % PPS;
        xl[(hh * SP + (j >> 1)) * 64 + g1_slot(j & 1, m, j >> 1)] = val;
    };
    u32x4 ring[DP];
    u32x4 val[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(0, i);
    float ssv[8];
    g1s_row_sumsq_load<32>(ssv, x, row_sumsq, rs_slices, 32);
    const float sc = scales[32 * t + (lane & 31)];
#pragma unroll
    for (int u = 0; u < DP; ++u) ring[u] = w_load(u);
#pragma unroll
    for (int i = 0; i < NPT; ++i) x_store(i, val[i]);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(1, i);
    g1s_row_scale<32>(rsc, ssv, row_sumsq, rs_slices, rs_inv_hidden, rs_eps);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const u32x4 *xa = xl + (size_t)kh * SP * 64;
    // one ring trip: k-steps s0 .. s0 + TL - 1 of the K half, staged as LDS records l0 .. of the current phase; every consumed pair is
    // refilled with the one D k-steps further on (unconditional; past the unit's end: no traffic)
    auto trip = [&](int l0, int s0) {
        u32x4 a[2];
        a[0] = xa[l0 * 64 + g1_slot(lane >> 5, lane & 31, 0)];
#pragma unroll
        for (int u = 0; u < TL / 2; ++u) {
            u32x4 &slot = ring[u % DP];
            a[1] = xa[(l0 + 2 * u + 1) * 64 + g1_slot(lane >> 5, lane & 31, 2 * u + 1)];
            const u32x4 b0 = g1q_operand(slot.x, slot.y, sc);
            acc = G1Mfma<DT>::mma(a[0], b0, acc);
            if (u + 1 < TL / 2) a[0] = xa[(l0 + 2 * u + 2) * 64 + g1_slot(lane >> 5, lane & 31, 2 * u + 2)];
            const u32x4 b1 = g1q_operand(slot.z, slot.w, sc);
            slot = w_load(s0 / 2 + u + DP);
            acc = G1Mfma<DT>::mma(a[1], b1, acc);
        }
    };
    for (int g = 0; g < SP / TL; ++g) trip(g * TL, g * TL);                   // ---- phase 0
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPT; ++i) x_store(i, val[i]);
    __syncthreads();
    for (int g = 0; g < SP / TL; ++g) trip(g * TL, SP + g * TL);              // ---- phase 1
    __syncthreads();
    float *red = reinterpret_cast<float *>(smem);
    g1s_plane_store<1>(red, kh * 4 + q, &acc);
    __syncthreads();
    g1s_finish<DT, 1, 2>(red, rsc, y, M, I);
}

// SJD_G1_W8_E4M3 on sjd_skinny_gemm / sjd_skinny_gemm_cols (which have checked the common arguments): M <= 64 with the whole activation chunk in
// LDS -- min(KC, K) <= 2560 up to 32 rows, <= 1280 at 33..64; 65..256 rows go to g1wq_launch.  The scales sit behind the N_packed * K record bytes.
static int g1q_launch(const void *x, const void *wq, float *out, int M, int N, int K, int KC, int waves, int step_major, int n_tiles, int tile0,
                      hipStream_t s)
{
    return g1_stream_launch(wq, M, N, K, KC, waves, step_major, n_tiles, tile0, 32,
        [&] { return M > 64 ? g1wq_launch(x, wq, out, M, N, K, KC, waves, step_major, n_tiles, tile0, s) : G1_STREAM_GO; },      // (G1wq, csrc/sjd_gemm_wide.h, or unsupported)
        [&](auto mt, auto maxt, dim3 grid, dim3 block, size_t lds, const unsigned char *scales, int rs) {
            return g1_launch_kernel(g1q_skinny_gemm<decltype(mt)::value, decltype(maxt)::value>, grid, block, lds, s, x, wq,
                                    reinterpret_cast<const float *>(scales), out, M, N, K, KC, n_tiles, rs, tile0, waves); });
}

// SJD_G1_W8_E4M3 on sjd_gateup_silu (which has checked the common arguments): M <= 32; the scales sit behind the 2 I * K record bytes.
static int g1sq_launch(const void *x, const void *wq, void *y, int M, int I, int K, int step_major, const sjd_row_norm *rn, hipStream_t s)
{
    return g1s_stream_launch(wq, M, I, K, step_major, 32, rn,
        [&](auto sp, dim3 grid, dim3 block, size_t lds, const unsigned char *scales, int rec_stride, const g1s_norm_args &n) {
            return g1_launch_kernel(g1q_gateup_silu<decltype(sp)::value>, grid, block, lds, s, x, wq, reinterpret_cast<const float *>(scales), y, M, I, K,
                                    rec_stride, n.ss, n.sl, n.ih, n.eps); });
}
