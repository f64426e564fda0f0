// sjd_gemm_q6.h -- G1q6 / G1sq6: the window projections streamed from 6-bit weights (OCP e2m3 codes, one e8m0 scale per 32 weights): 6.25 bits per
// weight.  Included by sjd_gemm.hip behind sjd_gemm_q4.h, whose structure (G1q4 / G1sq4) these kernels keep.
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

#define G1Q6_DEPTH 16          // k-steps a wave keeps in flight: a ring of four records (6 KiB per wave)

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

// G1q6: g1q4_skinny_gemm's structure (whole activation chunk in LDS, one buffer descriptor per unit -- loads past its end move nothing --, a register
// ring refilled unconditionally behind its consumer, non-temporal loads) over the 6-bit stream.  The record's byte offset rides in the per-lane
// offset of the loads, the part of the address the descriptor's range check covers.  A unit is whole records and whole scale dwords
// (steps % 8 == 0): the half trips past a unit's end are skipped by uniform branches, there is nothing else at the end of a unit.
template <int MT, int MAXT>
__global__ __launch_bounds__(MAXT) void g1q6_skinny_gemm(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wq,
                                                         const unsigned char *__restrict__ scales, float *__restrict__ out, int M, int N, int K, int KC,
                                                         int n_tiles, int rec_stride, int tile0, int n_waves)
{
    constexpr int D = MAXT <= 512 ? G1Q6_DEPTH : 8;
    constexpr int DR = D / 4;                                     // ring records
    constexpr int HT = D / 8;                                     // half trips per ring trip
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);
    const int chunk = blockIdx.y;
    const int k0 = chunk * KC;
    const int steps = min(KC, K - k0) / 16;                       // a multiple of eight (the launcher has checked K and KC)
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int t_out = blockIdx.x * n_waves + w;
    const bool has_tile = t_out < N / 32;
    const int t = has_tile ? tile0 + t_out : 0;
    const unsigned char *cb = wq + (size_t)k0 * ((size_t)n_tiles * 24);
    const unsigned char *sb = scales + (size_t)k0 * (size_t)n_tiles;
    const unsigned rsb = (unsigned)rec_stride * 1536u, ssb = (unsigned)rec_stride * 128u;      // bytes from a record / a trip's scales to the next
    const unsigned char *first = cb + (rec_stride == 1 ? (size_t)t * steps * 384 : (size_t)t * 1536);
    const unsigned char *sfirst = sb + (rec_stride == 1 ? (size_t)t * steps * 16 : (size_t)t * 128);
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(first, has_tile ? (unsigned)(steps / 4 - 1) * rsb + 1536u : 0u);
    const __amdgpu_buffer_rsrc_t sr = g1z_unit_rsrc(sfirst, has_tile ? (unsigned)(steps / 8 - 1) * ssb + 128u : 0u);
    auto w_load = [&](int r) -> g1q6_rec {
        g1q6_rec v;
        v.lo = __builtin_amdgcn_raw_buffer_load_b128(wr, (unsigned)lane * 16u + (unsigned)r * rsb, 0u, G1Z_AUX);
        v.hi = __builtin_amdgcn_raw_buffer_load_b64(wr, 1024u + (unsigned)lane * 8u + (unsigned)r * rsb, 0u, G1Z_AUX);
        return v;
    };
    const unsigned hsh = (unsigned)(lane >> 5) * 8u;              // the lane half's byte of a record's scale pair
    auto s_load = [&](int q) -> unsigned { return __builtin_amdgcn_raw_buffer_load_b32(sr, (unsigned)(lane & 31) * 4u + (unsigned)q * ssb, 0u, G1Z_AUX); };
    g1q6_rec ring[DR];
    unsigned scr[HT];
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
    {   // first activation batch, the first D k-steps and their scales right behind it (all unconditional)
        u32x4 val[STAGE];
        int m = pm, j = pj;
#pragma unroll
        for (int i = 0; i < STAGE; ++i) { val[i] = x_load(m, j); advance(m, j); }
#pragma unroll
        for (int h = 0; h < HT; ++h) {          // (the order the loop refills them in)
            ring[2 * h] = w_load(2 * h);
            ring[2 * h + 1] = w_load(2 * h + 1);
            scr[h] = s_load(h);
        }
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
    // ring trips of D k-steps: a consumed record is refilled with the one D k-steps further on, the scale dword of a half trip with the one D k-steps
    // further on, both unconditionally (past the unit's end: an instruction, no traffic)
    for (int s0 = 0; s0 < steps; s0 += D) {
#pragma unroll
        for (int h = 0; h < HT; ++h) {
            const int sh = s0 + 8 * h;
            if (sh < steps)          // (uniform: the last trip of a unit of an odd number of half trips)
                g1q6_half_trip<MT>(acc, ring[2 * h], ring[2 * h + 1], scr[h] >> hsh, [&](u32x4 (&a)[MT], int u) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) a[mt] = xl[mt * xs + (sh + u) * 64 + g1_slot(lane >> 5, lane & 31, u)];
                });
            ring[2 * h] = w_load(sh / 4 + DR);          // (outside the branch: every path through the loop issues the same loads, so its waits count exactly)
            ring[2 * h + 1] = w_load(sh / 4 + 1 + DR);
            scr[h] = s_load(sh / 8 + HT);
        }
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

// G1sq6: g1q4_gateup_silu over the 6-bit stream -- eight waves = two K halves x {gate, up} x two column tiles, two activation phases per K half,
// the tail of sjd_gemm_parts.h on the planes in LDS.  A K half has 2 SP k-steps (K / 32: a multiple of eight for every K served).
template <int SP>
__global__ __launch_bounds__(512) void g1q6_gateup_silu(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wq,
                                                        const unsigned char *__restrict__ scales, unsigned short *__restrict__ y, int M, int I, int K,
                                                        int rec_stride, const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden,
                                                        float rs_eps)
{
    constexpr int DT = SJD_DTYPE_BF16;
    constexpr int D = SP >= G1Q6_DEPTH ? G1Q6_DEPTH : 8;
    constexpr int DR = D / 4, HT = D / 8;
    static_assert(SP % D == 0 && D % 8 == 0, "a phase is whole trips; g1_slot(.., s) depends on s & 7");
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
    constexpr int recs = SP / 2, trips = SP / 4;                 // records / scale dwords of a K half (2 SP k-steps)
    const unsigned char *cb = wq + (size_t)kh * (K / 2) * ((size_t)n_tiles * 24);
    const unsigned char *sb = scales + (size_t)kh * (K / 2) * (size_t)n_tiles;
    const unsigned rsb = (unsigned)rec_stride * 1536u, ssb = (unsigned)rec_stride * 128u;
    const unsigned char *first = cb + (rec_stride == 1 ? (size_t)t * recs * 1536 : (size_t)t * 1536);
    const unsigned char *sfirst = sb + (rec_stride == 1 ? (size_t)t * trips * 128 : (size_t)t * 128);
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(first, (unsigned)(recs - 1) * rsb + 1536u);
    const __amdgpu_buffer_rsrc_t sr = g1z_unit_rsrc(sfirst, (unsigned)(trips - 1) * ssb + 128u);
    auto w_load = [&](int r) -> g1q6_rec {
        g1q6_rec v;
        v.lo = __builtin_amdgcn_raw_buffer_load_b128(wr, (unsigned)lane * 16u + (unsigned)r * rsb, 0u, G1Z_AUX);
        v.hi = __builtin_amdgcn_raw_buffer_load_b64(wr, 1024u + (unsigned)lane * 8u + (unsigned)r * rsb, 0u, G1Z_AUX);
        return v;
    };
    const unsigned hsh = (unsigned)(lane >> 5) * 8u;
    auto s_load = [&](int qq) -> unsigned { return __builtin_amdgcn_raw_buffer_load_b32(sr, (unsigned)(lane & 31) * 4u + (unsigned)qq * ssb, 0u, G1Z_AUX); };
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
    g1q6_rec ring[DR];
    unsigned scr[HT];
    u32x4 val[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(0, i);
    float ssv[8];
    g1s_row_sumsq_load<32>(ssv, x, row_sumsq, rs_slices, 32);
#pragma unroll
    for (int h = 0; h < HT; ++h) {
        ring[2 * h] = w_load(2 * h);
        ring[2 * h + 1] = w_load(2 * h + 1);
        scr[h] = s_load(h);
    }
#pragma unroll
    for (int i = 0; i < NPT; ++i) x_store(i, val[i]);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(1, i);
    g1s_row_scale<32>(rsc, ssv, row_sumsq, rs_slices, rs_inv_hidden, rs_eps);
    f32x16 acc[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = 0.0f;
    const u32x4 *xa = xl + (size_t)kh * SP * 64;
    // one ring trip: k-steps s0 .. s0 + D - 1 of the K half, staged as LDS records l0 .. of the current phase; every consumed record and scale
    // dword is refilled with the one D k-steps further on (unconditional; past the unit's end: no traffic)
    auto trip = [&](int l0, int s0) {
#pragma unroll
        for (int h = 0; h < HT; ++h) {
            const int sh = s0 + 8 * h, lh = l0 + 8 * h;
            g1q6_half_trip<1>(acc, ring[2 * h], ring[2 * h + 1], scr[h] >> hsh,
                [&](u32x4 (&a)[1], int u) { a[0] = xa[(lh + u) * 64 + g1_slot(lane >> 5, lane & 31, u)]; });
            ring[2 * h] = w_load(sh / 4 + DR);
            ring[2 * h + 1] = w_load(sh / 4 + 1 + DR);
            scr[h] = s_load(sh / 8 + HT);
        }
    };
    for (int g = 0; g < SP / D; ++g) trip(g * D, g * D);                      // ---- phase 0
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPT; ++i) x_store(i, val[i]);
    __syncthreads();
    for (int g = 0; g < SP / D; ++g) trip(g * D, SP + g * D);                 // ---- phase 1
    __syncthreads();
    float *red = reinterpret_cast<float *>(smem);
    g1s_plane_store<1>(red, kh * 4 + q, acc);
    __syncthreads();
    g1s_finish<DT, 1, 2>(red, rsc, y, M, I);
}

// SJD_G1_W6_E2M3 on sjd_skinny_gemm / sjd_skinny_gemm_cols (which have checked the common arguments): K and KC multiples of 128; M <= 64 with the whole
// activation chunk in LDS -- min(KC, K) <= 2560 up to 32 rows, <= 1280 at 33..64.  No form for more rows.  The scales sit behind the
// N_packed * K * 3 / 4 code bytes.
static int g1q6_launch(const void *x, const void *wq, float *out, int M, int N, int K, int KC, int waves, int step_major, int n_tiles, int tile0,
                       hipStream_t s)
{
    return g1_stream_launch(wq, M, N, K, KC, waves, step_major, n_tiles, tile0, 24,
        [&] { return ((K % 128) != 0 || (KC % 128) != 0 || M > 64) ? (int)SJD_ERR_UNSUPPORTED : G1_STREAM_GO; },
        [&](auto mt, auto maxt, dim3 grid, dim3 block, size_t lds, const unsigned char *scales, int rs) {
            return g1_launch_kernel(g1q6_skinny_gemm<decltype(mt)::value, decltype(maxt)::value>, grid, block, lds, s, x, wq, scales, out, M, N, K, KC,
                                    n_tiles, rs, tile0, waves); });
}

// SJD_G1_W6_E2M3 on sjd_gateup_silu (which has checked the common arguments: K in {512, 1024, 2048, 4096}, so a K half is a multiple of 128): M <= 32;
// the scales sit behind the 2 I * K * 3 / 4 code bytes.
static int g1sq6_launch(const void *x, const void *wq, void *y, int M, int I, int K, int step_major, const sjd_row_norm *rn, hipStream_t s)
{
    return g1s_stream_launch(wq, M, I, K, step_major, 24, rn,
        [&](auto sp, dim3 grid, dim3 block, size_t lds, const unsigned char *scales, int rec_stride, const g1s_norm_args &n) {
            return g1_launch_kernel(g1q6_gateup_silu<decltype(sp)::value>, grid, block, lds, s, x, wq, scales, y, M, I, K, rec_stride, n.ss, n.sl, n.ih,
                                    n.eps); });
}
