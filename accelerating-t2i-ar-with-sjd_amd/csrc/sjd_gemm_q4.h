// sjd_gemm_q4.h -- G1q4 / G1sq4: the window projections streamed from OCP MXFP4 weights (e2m1 codes, one e8m0 scale per 32 weights along K):
// 4.25 bits per weight.  Included by sjd_gemm.hip behind sjd_gemm_qblock.h: the kernels are its templates over G1Q4Stream (below), which the
// launchers here name; the format, its decode and the K = 8192 gate|up kernel are here.
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

// the stream as the kernels of sjd_gemm_qblock.h take it
struct G1Q4Stream {
    using rec = u32x4;                                // a lane's four code dwords of one record
    static constexpr int REC_BYTES = 1024, TILE_K_BYTES = 16;
    static constexpr int DEPTH = 16;                  // a ring of four records, the 4 KiB per wave that G1q's ring of eight k-steps holds
    static __device__ __forceinline__ rec load(__amdgpu_buffer_rsrc_t wr, int lane, unsigned byte_off)
    {
        return __builtin_amdgcn_raw_buffer_load_b128(wr, (unsigned)lane * 16u + byte_off, 0u, G1Z_AUX);
    }
    static __device__ __forceinline__ unsigned lane_scales(unsigned sd, unsigned) { return sd; }      // (both lane halves: the same four blocks)
    template <int MT, typename AR>
    static __device__ __forceinline__ void half_trip(f32x16 (&acc)[MT], const rec &rec0, const rec &rec1, unsigned sd, AR a_read) { g1q4_half_trip<MT>(acc, rec0, rec1, sd, a_read); }
};

// G1sq4 at K = 8192 (30B-class hidden): the gate|up weight is the copy G1q4 streams in FOUR chunks of 2048, so F3 would sum four planes and a wave keeps one
// fp32 accumulator per K quarter.  Eight waves as g1qb_gateup_silu's (two K halves x {gate, up} x two column tiles); a K half is two chunks = two units per wave, each
// under its own pair of descriptors, and four activation phases of SP = 64 k-steps (2 x 64 KiB of LDS per phase).  The wave switches accumulator and unit
// after two phases; the ring is never drained in between: the last trip of the first unit refills from the head of the second (still unconditional
// loads, one per consumed record / scale dword), the last trip of the second refills past its end (no traffic).
__global__ __launch_bounds__(512) void g1q4_gateup_silu_k4(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wq,
                                                           const unsigned char *__restrict__ scales, unsigned short *__restrict__ y, int M, int I,
                                                           int rec_stride, const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden,
                                                           float rs_eps)
{
    using S = G1Q4Stream;
    constexpr int DT = SJD_DTYPE_BF16;
    constexpr int K = 8192, KC = 2048, SP = 64;
    constexpr int D = S::DEPTH, DR = D / 4, HT = D / 8;
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
    const unsigned rsb = (unsigned)rec_stride * (unsigned)S::REC_BYTES, ssb = (unsigned)rec_stride * 128u;
    const size_t uoff = rec_stride == 1 ? (size_t)t * recs * S::REC_BYTES : (size_t)t * S::REC_BYTES;
    const size_t soff = rec_stride == 1 ? (size_t)t * trips * 128 : (size_t)t * 128;
    const size_t cbytes = (size_t)KC * ((size_t)n_tiles * S::TILE_K_BYTES), sbytes = (size_t)KC * (size_t)n_tiles;      // a chunk's records / scales
    const unsigned ubytes = (unsigned)(recs - 1) * rsb + (unsigned)S::REC_BYTES, usbytes = (unsigned)(trips - 1) * ssb + 128u;      // a unit's extent under its descriptor
    const unsigned char *cb = wq + (size_t)(2 * kh) * cbytes + uoff;                           // the wave's unit of chunk 2 kh; that of chunk 2 kh + 1 is cbytes on
    const unsigned char *sb = scales + (size_t)(2 * kh) * sbytes + soff;
    auto w_load = [&](const __amdgpu_buffer_rsrc_t &wr, int r) -> u32x4 { return S::load(wr, lane, (unsigned)r * rsb); };
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
            S::half_trip<1>(acc, ring[2 * h], ring[2 * h + 1], scr[h],
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

// SJD_G1_W4_MXFP4 on sjd_skinny_gemm / sjd_skinny_gemm_cols: g1qb_launch's shapes (M <= 64), K and KC multiples of 128; 65..256 rows go to g1wq4_launch.
static int g1q4_launch(const void *x, const void *wq, float *out, int M, int N, int K, int KC, int waves, int step_major, int n_tiles, int tile0,
                       hipStream_t s)
{
    return g1qb_launch<G1Q4Stream>(x, wq, out, M, N, K, KC, waves, step_major, n_tiles, tile0, s,
        [&] {          // (whole records and scale dwords only; 65..256 rows: G1wq4, csrc/sjd_gemm_wide.h, or unsupported)
            if ((K % 128) != 0 || (KC % 128) != 0) return (int)SJD_ERR_UNSUPPORTED;
            return M > 64 ? g1wq4_launch(x, wq, out, M, N, K, KC, waves, step_major, n_tiles, tile0, s) : G1_STREAM_GO; });
}

// SJD_G1_W4_MXFP4 on sjd_gateup_silu: g1sqb_launch's shapes (M <= 32, K in {512, 1024, 2048, 4096})
static int g1sq4_launch(const void *x, const void *wq, void *y, int M, int I, int K, int step_major, const sjd_row_norm *rn, hipStream_t s)
{
    return g1sqb_launch<G1Q4Stream>(x, wq, y, M, I, K, step_major, rn, s);
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
    const unsigned char *scales = static_cast<const unsigned char *>(wq) + (size_t)(2 * (I / 32)) * G1Q4Stream::TILE_K_BYTES * K;
    const g1s_norm_args n(rn);
    return g1_launch_kernel(g1q4_gateup_silu_k4, grid, block, lds, s, x, wq, scales, y, M, I, rec_stride, n.ss, n.sl, n.ih, n.eps);
}
