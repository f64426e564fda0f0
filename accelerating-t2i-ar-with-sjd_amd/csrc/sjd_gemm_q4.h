// sjd_gemm_q4.h -- G1q4 / G1sq4: the window projections streamed from OCP MXFP4 weights (e2m1 codes, one e8m0 scale per 32 weights along K):
// 4.25 bits per weight.  Included by sjd_gemm.hip behind sjd_gemm_q8.h, whose structure (G1q / G1sq) these kernels keep.
//
// The format (sjd_amd.ops.pack_weight_q4): ONE buffer = the code records (N_packed * K / 2 bytes), then the scale bytes (N_packed * K / 32) behind them.
// Weight w[n][k] is stored as code q (sign, 2 exponent bits, 1 mantissa bit: 0, 0.5, 1, 1.5, 2, 3, 4, 6) times scale[n][k / 32] = 2^(byte - 127),
// so q * scale is exactly a bf16 value: the kernels rebuild the bf16 MFMA operand bit for bit (v_cvt_scalef32_pk_bf16_fp4, the scale in the
// conversion: four conversions per eight weights, as many as the e4m3 decode, from half the bytes) and run the MFMA sequence of G1 / G1s, so the
// planes / the 16-bit output are those of sjd_skinny_gemm / sjd_gateup_silu on pack_weight(q * scale), bit for bit.  All the loss is in the
// host-side quantiser.
//   K GRANULE g = 128: K and every chunk are multiples of 128 columns = eight k-steps = two records = four scale blocks.  A unit is then whole
//       records AND whole scale dwords: the kernels have no tail path (no half record, no odd pair) -- the packer and the launchers refuse the rest.
//   unit (k-chunk c, 32-column tile t), S = its k-steps: k-step s, lane l = 32 h + r, element j = q[32 t + r][k0 + 16 s + 8 h + j] (pack_weight's
//       element order); the eight codes of (s, l) are FOUR bytes, byte i = code 2i in the low nibble, code 2i + 1 in the high nibble;
//   RECORD R (1024 B) = k-steps 4R .. 4R + 3: 64 lanes x 16 B {the lane's four bytes of k-step 4R, of 4R + 1, of 4R + 2, of 4R + 3} -- one aligned
//       16-byte load per lane; a chunk starts at byte k0 * N_packed / 2;
//   tile-major: a unit is S * 256 contiguous bytes; step-major: the chunk holds record 0 of every tile, record 1 of every tile, ...
//   scales, at byte N_packed * K / 2: per unit and TRIP q (eight k-steps) 128 bytes = 32 columns x 4 bytes, byte b of column r = the e8m0 scale of
//       the column's block 4q + b of the chunk (k-steps 8q + 2b and 8q + 2b + 1, both lane halves) -- a lane takes a trip's scales with one aligned
//       dword load; the trips of a unit are laid out like its records (a chunk starts at scale byte k0 * N_packed / 32; tile-major: S / 8
//       consecutive 128-byte groups per unit; step-major: trip 0 of every tile, trip 1 of every tile, ...).
// bf16; M <= 64 (G1q4) / M <= 32 (G1sq4): see the launchers.  65..256 rows: kernel G1wq4, the Q && WIDE form of g1_wide (csrc/sjd_gemm_wide.h), which
// streams the same buffer -- g1q4_launch sends those row counts there.
// K = 8192 (30B-class hidden): g1q4_gateup_silu_k4, the form of G1sq4 over the copy G1q4 streams in FOUR chunks of 2048 (sjd_gateup_silu with
// SJD_G1S_CHUNKS(4)): bit for bit G1q4(KC = 2048) + F3 on the same buffer.  The e4m3 stream has no such form (G1q + F3 there).
#pragma once

#define G1Q4_DEPTH 16          // k-steps a wave keeps in flight: a ring of four records, the 4 KiB per wave that G1q's ring of eight k-steps holds

// the MFMA B operand (eight bf16) of one k-step from its four code bytes and the block's scale
__device__ __forceinline__ u32x4 g1q4_operand(unsigned c, float sc)
{
    u32x4 d;
    d.x = __builtin_bit_cast(unsigned, (g1q_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 0));
    d.y = __builtin_bit_cast(unsigned, (g1q_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 1));
    d.z = __builtin_bit_cast(unsigned, (g1q_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 2));
    d.w = __builtin_bit_cast(unsigned, (g1q_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, sc, 3));
    return d;
}

// the float 2^(byte - 127) of scale byte B (0..3) of a trip's dword: the e8m0 byte IS the float's exponent field
template <int B>
__device__ __forceinline__ float g1q4_scale(unsigned sd)
{
    return __builtin_bit_cast(float, (B == 0 ? sd << 23 : B == 1 ? sd << 15 : B == 2 ? sd << 7 : sd >> 1) & 0x7f800000u);
}

// one HALF TRIP: the eight k-steps of two ring records against the scale dword `sd`; a_read(a, u) fetches the A fragments of the trip's k-step u
// (the next one is read ahead of the current MFMA); the caller refills the two records and the dword behind it
template <int MT, typename AR>
__device__ __forceinline__ void g1q4_half_trip(f32x16 (&acc)[MT], const u32x4 &rec0, const u32x4 &rec1, unsigned sd, AR a_read)
{
    constexpr int DT = SJD_DTYPE_BF16;
    u32x4 a[2][MT];
    a_read(a[0], 0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (u + 1 < 8) a_read(a[(u + 1) & 1], u + 1);
        const u32x4 &rec = u < 4 ? rec0 : rec1;
        const unsigned c = (u & 3) == 0 ? rec.x : (u & 3) == 1 ? rec.y : (u & 3) == 2 ? rec.z : rec.w;
        const float sc = (u >> 1) == 0 ? g1q4_scale<0>(sd) : (u >> 1) == 1 ? g1q4_scale<1>(sd) : (u >> 1) == 2 ? g1q4_scale<2>(sd) : g1q4_scale<3>(sd);
        const u32x4 b = g1q4_operand(c, sc);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a[u & 1][mt], b, acc[mt]);
    }
}

// G1q4: g1q_skinny_gemm's structure (whole activation chunk in LDS, one buffer descriptor per unit -- loads past its end move nothing --, a register
// ring refilled unconditionally behind its consumer, non-temporal loads) over the 4-bit stream.  The record's byte offset rides in the per-lane
// offset of the load, the part of the address the descriptor's range check covers.  A unit is whole records and whole scale dwords
// (steps % 8 == 0): the half trips past a unit's end are skipped by uniform branches, there is nothing else at the end of a unit.
template <int MT, int MAXT>
__global__ __launch_bounds__(MAXT) void g1q4_skinny_gemm(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wq,
                                                         const unsigned char *__restrict__ scales, float *__restrict__ out, int M, int N, int K, int KC,
                                                         int n_tiles, int rec_stride, int tile0, int n_waves)
{
    constexpr int D = MAXT <= 512 ? G1Q4_DEPTH : 8;
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
    const unsigned char *cb = wq + (size_t)k0 * ((size_t)n_tiles * 16);
    const unsigned char *sb = scales + (size_t)k0 * (size_t)n_tiles;
    const unsigned rsb = (unsigned)rec_stride * 1024u, ssb = (unsigned)rec_stride * 128u;      // bytes from a record / a trip's scales to the next
    const unsigned char *first = cb + (rec_stride == 1 ? (size_t)t * steps * 256 : (size_t)t * 1024);
    const unsigned char *sfirst = sb + (rec_stride == 1 ? (size_t)t * steps * 16 : (size_t)t * 128);
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(first, has_tile ? (unsigned)(steps / 4 - 1) * rsb + 1024u : 0u);
    const __amdgpu_buffer_rsrc_t sr = g1z_unit_rsrc(sfirst, has_tile ? (unsigned)(steps / 8 - 1) * ssb + 128u : 0u);
    auto w_load = [&](int r) -> u32x4 { return __builtin_amdgcn_raw_buffer_load_b128(wr, (unsigned)lane * 16u + (unsigned)r * rsb, 0u, G1Z_AUX); };
    auto s_load = [&](int q) -> unsigned { return __builtin_amdgcn_raw_buffer_load_b32(sr, (unsigned)(lane & 31) * 4u + (unsigned)q * ssb, 0u, G1Z_AUX); };
    u32x4 ring[DR];
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
                g1q4_half_trip<MT>(acc, ring[2 * h], ring[2 * h + 1], scr[h], [&](u32x4 (&a)[MT], int u) {
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

// G1sq4: g1q_gateup_silu over the 4-bit stream -- eight waves = two K halves x {gate, up} x two column tiles, two activation phases per K half,
// the epilogue of sjd_mlp_epilogue.h on the planes in LDS.  A K half has 2 SP k-steps (K / 32: a multiple of eight for every K served).
template <int SP>
__global__ __launch_bounds__(512) void g1q4_gateup_silu(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wq,
                                                        const unsigned char *__restrict__ scales, unsigned short *__restrict__ y, int M, int I, int K,
                                                        int rec_stride, const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden,
                                                        float rs_eps)
{
    constexpr int DT = SJD_DTYPE_BF16;
    constexpr int D = SP >= G1Q4_DEPTH ? G1Q4_DEPTH : 8;
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
    const unsigned char *cb = wq + (size_t)kh * (K / 2) * ((size_t)n_tiles * 16);
    const unsigned char *sb = scales + (size_t)kh * (K / 2) * (size_t)n_tiles;
    const unsigned rsb = (unsigned)rec_stride * 1024u, ssb = (unsigned)rec_stride * 128u;
    const unsigned char *first = cb + (rec_stride == 1 ? (size_t)t * recs * 1024 : (size_t)t * 1024);
    const unsigned char *sfirst = sb + (rec_stride == 1 ? (size_t)t * trips * 128 : (size_t)t * 128);
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(first, (unsigned)(recs - 1) * rsb + 1024u);
    const __amdgpu_buffer_rsrc_t sr = g1z_unit_rsrc(sfirst, (unsigned)(trips - 1) * ssb + 128u);
    auto w_load = [&](int r) -> u32x4 { return __builtin_amdgcn_raw_buffer_load_b128(wr, (unsigned)lane * 16u + (unsigned)r * rsb, 0u, G1Z_AUX); };
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
    u32x4 ring[DR];
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
            g1q4_half_trip<1>(acc, ring[2 * h], ring[2 * h + 1], scr[h],
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

// G1sq4 at K = 8192 (30B-class hidden): the gate|up weight is the copy G1q4 streams in FOUR chunks of 2048, so F3 would sum four planes and a wave keeps one
// fp32 accumulator per K quarter.  Eight waves as above (two K halves x {gate, up} x two column tiles); a K half is two chunks = two units per wave, each
// under its own pair of descriptors, and four activation phases of SP = 64 k-steps (2 x 64 KiB of LDS per phase).  The wave switches accumulator and unit
// after two phases; the ring is never drained in between: the last trip of the first unit refills from the head of the second (still unconditional
// loads, one per consumed record / scale dword), the last trip of the second refills past its end (no traffic).
__global__ __launch_bounds__(512) void g1q4_gateup_silu_k4(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wq,
                                                           const unsigned char *__restrict__ scales, unsigned short *__restrict__ y, int M, int I,
                                                           int rec_stride, const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden,
                                                           float rs_eps)
{
    constexpr int DT = SJD_DTYPE_BF16;
    constexpr int K = 8192, KC = 2048, SP = 64;
    constexpr int D = G1Q4_DEPTH, DR = D / 4, HT = D / 8;
    constexpr int NPH = K / 2 / (16 * SP);                       // phases per K half: four, two per chunk
    static_assert(SP % D == 0 && D % 8 == 0 && NPH == 4 && KC == 2 * 16 * SP, "a phase is whole trips; a chunk is two phases");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);
    __shared__ float rsc[32];
    constexpr int PPS = 2 * SP;
    constexpr int NPT = (32 * 2 * PPS) / 512;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int kh = w >> 2, q = w & 3;
    const int n_gate = I / 32, n_tiles = 2 * n_gate;
    const int t_act = 2 * blockIdx.x + (q & 1);
    const int t = (q < 2 ? 0 : n_gate) + t_act;
    constexpr int recs = KC / 64, trips = KC / 128;              // records / scale dwords of a unit
    const unsigned rsb = (unsigned)rec_stride * 1024u, ssb = (unsigned)rec_stride * 128u;
    const size_t uoff = rec_stride == 1 ? (size_t)t * recs * 1024 : (size_t)t * 1024;
    const size_t soff = rec_stride == 1 ? (size_t)t * trips * 128 : (size_t)t * 128;
    const size_t cbytes = (size_t)KC * ((size_t)n_tiles * 16), sbytes = (size_t)KC * (size_t)n_tiles;      // a chunk's records / scales
    const unsigned ubytes = (unsigned)(recs - 1) * rsb + 1024u, usbytes = (unsigned)(trips - 1) * ssb + 128u;      // a unit's extent under its descriptor
    const unsigned char *cb = wq + (size_t)(2 * kh) * cbytes + uoff;                           // the wave's unit of chunk 2 kh; that of chunk 2 kh + 1 is cbytes on
    const unsigned char *sb = scales + (size_t)(2 * kh) * sbytes + soff;
    auto w_load = [&](const __amdgpu_buffer_rsrc_t &wr, int r) -> u32x4 {
        return __builtin_amdgcn_raw_buffer_load_b128(wr, (unsigned)lane * 16u + (unsigned)r * rsb, 0u, G1Z_AUX); };
    auto s_load = [&](const __amdgpu_buffer_rsrc_t &sr, int qq) -> unsigned {
        return __builtin_amdgcn_raw_buffer_load_b32(sr, (unsigned)(lane & 31) * 4u + (unsigned)qq * ssb, 0u, G1Z_AUX); };
    // piece v = 512 i + thread of a phase: row m = v / (2 PPS) = 2 i + m0, K half hh, 16-byte piece j of the half's SP k-steps; xp = x + the phase's
    // first column (uniform), so a piece is one 32-bit offset from a scalar base
    const int m0 = threadIdx.x / (2 * PPS), hh0 = (threadIdx.x / PPS) & 1, j0 = threadIdx.x % PPS;
    static_assert(512 == 2 * (2 * PPS) && NPT == 16, "two rows per batch of 512 pieces");
    const unsigned xo = (unsigned)(m0 * K + hh0 * (K / 2) + 8 * j0);
    auto x_load = [&](const unsigned short *xp, int i) -> u32x4 {
        return (2 * i + m0 < M) ? *reinterpret_cast<const u32x4 *>(xp + (xo + (unsigned)(2 * i * K))) : u32x4{0u, 0u, 0u, 0u};
    };
    auto x_store = [&](int i, u32x4 val) {
        xl[(hh0 * SP + (j0 >> 1)) * 64 + g1_slot(j0 & 1, 2 * i + m0, j0 >> 1)] = val;
    };
    u32x4 ring[DR];
    unsigned scr[HT];
    u32x4 val[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(x, i);
    float ssv[8];
    g1s_row_sumsq_load<32>(ssv, x, row_sumsq, rs_slices, 32);
    {
        const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(cb, ubytes), sr = g1z_unit_rsrc(sb, usbytes);
#pragma unroll
        for (int h = 0; h < HT; ++h) {
            ring[2 * h] = w_load(wr, 2 * h);
            ring[2 * h + 1] = w_load(wr, 2 * h + 1);
            scr[h] = s_load(sr, h);
        }
    }
#pragma unroll
    for (int i = 0; i < NPT; ++i) x_store(i, val[i]);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(x + 16 * SP, i);
    g1s_row_scale<32>(rsc, ssv, row_sumsq, rs_slices, rs_inv_hidden, rs_eps);
    f32x16 acc[1], first[1];                                      // the chunk in flight; chunk 2 kh once it is done
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.0f; first[0][r] = 0.0f; }
    const u32x4 *xa = xl + (size_t)kh * SP * 64;
    // one ring trip: D k-steps staged as LDS records l0 .. of the current phase; every consumed record and scale dword is refilled from record r0 .. /
    // dword q0 .. of (wr, sr) -- D k-steps further on in the same unit, or the head of the next one
    auto trip = [&](int l0, const __amdgpu_buffer_rsrc_t &wr, const __amdgpu_buffer_rsrc_t &sr, int r0, int q0) {
#pragma unroll
        for (int h = 0; h < HT; ++h) {
            const int lh = l0 + 8 * h;
            g1q4_half_trip<1>(acc, ring[2 * h], ring[2 * h + 1], scr[h],
                [&](u32x4 (&af)[1], int u) { af[0] = xa[(lh + u) * 64 + g1_slot(lane >> 5, lane & 31, u)]; });
            ring[2 * h] = w_load(wr, r0 + 2 * h);
            ring[2 * h + 1] = w_load(wr, r0 + 2 * h + 1);
            scr[h] = s_load(sr, q0 + h);
        }
    };
    auto restage = [&]() {          // the phase just read gives way to the one held in `val`
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NPT; ++i) x_store(i, val[i]);
        __syncthreads();
    };
    // the wave's two units, one pass each: LDS holds phase 2 u and `val` phase 2 u + 1 on entry.  The pass is a loop, not unrolled, so that the two
    // units share their code and nothing of one is kept in registers across the other.
#pragma nounroll
    for (int u = 0; u < 2; ++u) {
        const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(cb + (size_t)u * cbytes, ubytes), sr = g1z_unit_rsrc(sb + (size_t)u * sbytes, usbytes);
        // what the unit's last trip refills from: the head of the next unit; behind the last one a descriptor of no bytes (an instruction, no traffic)
        const __amdgpu_buffer_rsrc_t nwr = g1z_unit_rsrc(cb + (size_t)(u + 1) * cbytes, u == 0 ? ubytes : 0u);
        const __amdgpu_buffer_rsrc_t nsr = g1z_unit_rsrc(sb + (size_t)(u + 1) * sbytes, u == 0 ? usbytes : 0u);
        const unsigned short *xp = x + (size_t)u * (2 * 16 * SP);
        for (int g = 0; g < SP / D; ++g) trip(g * D, wr, sr, g * D / 4 + DR, g * D / 8 + HT);                          // ---- the unit's k-steps 0 .. SP - 1
        restage();
        if (u == 0) {
#pragma unroll
            for (int i = 0; i < NPT; ++i) val[i] = x_load(xp + 2 * 16 * SP, i);
        }
        for (int g = 0; g < SP / D - 1; ++g) trip(g * D, wr, sr, (SP + g * D) / 4 + DR, (SP + g * D) / 8 + HT);        // ---- SP .. 2 SP - 1
        trip(SP - D, nwr, nsr, 0, 0);
        if (u == 0) {
            restage();
#pragma unroll
            for (int i = 0; i < NPT; ++i) val[i] = x_load(xp + 3 * 16 * SP, i);
#pragma unroll
            for (int r = 0; r < 16; ++r) { first[0][r] = acc[0][r]; acc[0][r] = 0.0f; }
        }
    }
    __syncthreads();
    float *red = reinterpret_cast<float *>(smem);                // sixteen planes: (chunk, q), 32 rows of G1S_RP floats each
    g1s_plane_store<1>(red, (2 * kh) * 4 + q, first);
    g1s_plane_store<1>(red, (2 * kh + 1) * 4 + q, acc);
    __syncthreads();
    g1s_finish<DT, 1, 4>(red, rsc, y, M, I);
}

// SJD_G1_W4_MXFP4 on sjd_skinny_gemm / sjd_skinny_gemm_cols (which have checked the common arguments): K and KC multiples of 128; M <= 64 with the whole
// activation chunk in LDS -- min(KC, K) <= 2560 up to 32 rows, <= 1280 at 33..64; 65..256 rows go to g1wq4_launch.  The scales sit behind the
// N_packed * K / 2 code bytes.
static int g1q4_launch(const void *x, const void *wq, float *out, int M, int N, int K, int KC, int waves, int step_major, int n_tiles, int tile0,
                       hipStream_t s)
{
    return g1_stream_launch(wq, M, N, K, KC, waves, step_major, n_tiles, tile0, 16,
        [&] {          // (whole records and scale dwords only; 65..256 rows: G1wq4, csrc/sjd_gemm_wide.h, or unsupported)
            if ((K % 128) != 0 || (KC % 128) != 0) return (int)SJD_ERR_UNSUPPORTED;
            return M > 64 ? g1wq4_launch(x, wq, out, M, N, K, KC, waves, step_major, n_tiles, tile0, s) : G1_STREAM_GO; },
        [&](auto mt, auto maxt, dim3 grid, dim3 block, size_t lds, const unsigned char *scales, int rs) {
            return g1_launch_kernel(g1q4_skinny_gemm<decltype(mt)::value, decltype(maxt)::value>, grid, block, lds, s, x, wq, scales, out, M, N, K, KC,
                                    n_tiles, rs, tile0, waves); });
}

// SJD_G1_W4_MXFP4 on sjd_gateup_silu (which has checked the common arguments: K in {512, 1024, 2048, 4096}, so a K half is a multiple of 128): M <= 32;
// the scales sit behind the I * K code bytes.
static int g1sq4_launch(const void *x, const void *wq, void *y, int M, int I, int K, int step_major, const sjd_row_norm *rn, hipStream_t s)
{
    return g1s_stream_launch(wq, M, I, K, step_major, 16, rn,
        [&](auto sp, dim3 grid, dim3 block, size_t lds, const unsigned char *scales, int rec_stride, const g1s_norm_args &n) {
            return g1_launch_kernel(g1q4_gateup_silu<decltype(sp)::value>, grid, block, lds, s, x, wq, scales, y, M, I, K, rec_stride, n.ss, n.sl, n.ih,
                                    n.eps); });
}

// SJD_G1_W4_MXFP4 | SJD_G1S_CHUNKS(4) on sjd_gateup_silu (which has checked the arguments): M <= 32, K = 8192 in four chunks of 2048, the scales behind the I * K code bytes.  The
// activation arena is one phase of two K halves x 64 k-steps = 128 KiB; the epilogue's sixteen planes (72 KiB) reuse it.
static int g1sq4k4_launch(const void *x, const void *wq, void *y, int M, int I, int step_major, const sjd_row_norm *rn, hipStream_t s)
{
    constexpr int K = 8192;
    const dim3 grid(I / 64), block(512);
    const size_t lds_x = (size_t)2 * 64 * 1024, lds_red = 2 * g1s_epilogue_lds(1);
    const size_t lds = lds_x > lds_red ? lds_x : lds_red;
    static_assert((size_t)2 * 64 * 1024 <= 160 * 1024 && 2 * g1s_epilogue_lds(1) <= 160 * 1024, "the arena the launchers allow");
    const int rec_stride = step_major ? 2 * (I / 32) : 1;
    const unsigned char *scales = static_cast<const unsigned char *>(wq) + (size_t)(2 * (I / 32)) * 16 * K;
    const g1s_norm_args n(rn);
    return g1_launch_kernel(g1q4_gateup_silu_k4, grid, block, lds, s, x, wq, scales, y, M, I, rec_stride, n.ss, n.sl, n.ih, n.eps);
}
