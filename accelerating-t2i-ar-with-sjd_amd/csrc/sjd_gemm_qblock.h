// sjd_gemm_qblock.h -- the kernels of the block-scaled streams, once: the whole-chunk kernel (G1q4, G1q6) and the 32-row gate|up kernel (G1sq4,
// G1sq6) as templates over a STREAM, with their launchers.  Included by sjd_gemm.hip behind sjd_gemm_q8.h, whose structure (G1q / G1sq) these
// kernels keep, and in front of the streams' own headers (sjd_gemm_q4.h: G1Q4Stream, sjd_gemm_q6.h: G1Q6Stream), which describe their formats,
// decode them and name these templates in their launchers.
// Common to the streams: 64-k RECORDS (k-steps 4R .. 4R + 3 of a 32-column tile), one e8m0 scale per 32 weights, 128 bytes of scales per unit and
// TRIP (two records: one dword per column), the K granule 128 (a unit is whole records and whole scale dwords: no tail path) and both layouts
// (tile-major: a unit's records contiguous; step-major: record 0 of every tile, record 1 of every tile, ...; a trip's scales like the records).
// What a stream S supplies, and all that differs between the instantiations:
//   S::rec, S::DEPTH                          a lane's code dwords of one record, and the k-steps a wave keeps in flight: a ring of DEPTH / 4 rec
//   S::REC_BYTES, S::TILE_K_BYTES             a record's bytes (64 lanes), and the record bytes per 32-column tile and column of K (REC_BYTES / 64)
//   S::load(rsrc, lane, byte_off)             the lane's part of the record at byte_off of the unit's descriptor (non-temporal buffer loads)
//   S::lane_scales(sd, hsh)                   a trip's scale dword as the half trip wants it (hsh = 8 * the lane's half)
//   S::half_trip<MT>(acc, rec0, rec1, sd, a_read)   the eight k-steps of two ring records: decode and MFMA
// The bodies are written in place, once; only types and constants come from S, so an instantiation is the kernel its stream's header used to spell
// out (tools/kernel_diff.py against those copies: DESIGN.md 4.2h).  Staging, ring fill and plane store are NOT functions: see sjd_gemm_parts.h.
#pragma once

// G1q4 / G1q6: g1q_skinny_gemm's structure (whole activation chunk in LDS, one buffer descriptor per unit -- loads past its end move nothing --, a
// register ring refilled unconditionally behind its consumer, non-temporal loads) over a block-scaled stream.  The record's byte offset rides in
// the per-lane offset of the loads, the part of the address the descriptor's range check covers.  A unit is whole records and whole scale dwords
// (steps % 8 == 0): the half trips past a unit's end are skipped by uniform branches, there is nothing else at the end of a unit.
template <typename S, int MT, int MAXT>
__global__ __launch_bounds__(MAXT) void g1qb_skinny_gemm(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wq,
                                                         const unsigned char *__restrict__ scales, float *__restrict__ out, int M, int N, int K, int KC,
                                                         int n_tiles, int rec_stride, int tile0, int n_waves)
{
    using rec_t = typename S::rec;
    constexpr int D = MAXT <= 512 ? S::DEPTH : 8;
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
    const unsigned char *cb = wq + (size_t)k0 * ((size_t)n_tiles * S::TILE_K_BYTES);
    const unsigned char *sb = scales + (size_t)k0 * (size_t)n_tiles;
    const unsigned rsb = (unsigned)rec_stride * (unsigned)S::REC_BYTES, ssb = (unsigned)rec_stride * 128u;      // bytes from a record / a trip's scales to the next
    const unsigned char *first = cb + (rec_stride == 1 ? (size_t)t * steps * (S::REC_BYTES / 4) : (size_t)t * S::REC_BYTES);
    const unsigned char *sfirst = sb + (rec_stride == 1 ? (size_t)t * steps * 16 : (size_t)t * 128);
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(first, has_tile ? (unsigned)(steps / 4 - 1) * rsb + (unsigned)S::REC_BYTES : 0u);
    const __amdgpu_buffer_rsrc_t sr = g1z_unit_rsrc(sfirst, has_tile ? (unsigned)(steps / 8 - 1) * ssb + 128u : 0u);
    auto w_load = [&](int r) -> rec_t { return S::load(wr, lane, (unsigned)r * rsb); };
    const unsigned hsh = (unsigned)(lane >> 5) * 8u;              // the lane half's byte of a record's scale pair
    auto s_load = [&](int q) -> unsigned { return __builtin_amdgcn_raw_buffer_load_b32(sr, (unsigned)(lane & 31) * 4u + (unsigned)q * ssb, 0u, G1Z_AUX); };
    rec_t ring[DR];
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
                S::template half_trip<MT>(acc, ring[2 * h], ring[2 * h + 1], S::lane_scales(scr[h], hsh), [&](u32x4 (&a)[MT], int u) {
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

// G1sq4 / G1sq6: g1q_gateup_silu over a block-scaled stream -- eight waves = two K halves x {gate, up} x two column tiles, two activation phases
// per K half, the tail of sjd_gemm_parts.h on the planes in LDS.  A K half has 2 SP k-steps (K / 32: a multiple of eight for every K served).
template <typename S, int SP>
__global__ __launch_bounds__(512) void g1qb_gateup_silu(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wq,
                                                        const unsigned char *__restrict__ scales, unsigned short *__restrict__ y, int M, int I, int K,
                                                        int rec_stride, const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden,
                                                        float rs_eps)
{
    using rec_t = typename S::rec;
    constexpr int DT = SJD_DTYPE_BF16;
    constexpr int D = SP >= S::DEPTH ? S::DEPTH : 8;
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
    const unsigned char *cb = wq + (size_t)kh * (K / 2) * ((size_t)n_tiles * S::TILE_K_BYTES);
    const unsigned char *sb = scales + (size_t)kh * (K / 2) * (size_t)n_tiles;
    const unsigned rsb = (unsigned)rec_stride * (unsigned)S::REC_BYTES, ssb = (unsigned)rec_stride * 128u;
    const unsigned char *first = cb + (rec_stride == 1 ? (size_t)t * recs * S::REC_BYTES : (size_t)t * S::REC_BYTES);
    const unsigned char *sfirst = sb + (rec_stride == 1 ? (size_t)t * trips * 128 : (size_t)t * 128);
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(first, (unsigned)(recs - 1) * rsb + (unsigned)S::REC_BYTES);
    const __amdgpu_buffer_rsrc_t sr = g1z_unit_rsrc(sfirst, (unsigned)(trips - 1) * ssb + 128u);
    auto w_load = [&](int r) -> rec_t { return S::load(wr, lane, (unsigned)r * rsb); };
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
    rec_t ring[DR];
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
            S::template half_trip<1>(acc, ring[2 * h], ring[2 * h + 1], S::lane_scales(scr[h], hsh),
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

// The launcher of stream S's whole-chunk kernel on sjd_skinny_gemm / sjd_skinny_gemm_cols (which have checked the common arguments): M <= 64 with
// the whole activation chunk in LDS -- min(KC, K) <= 2560 up to 32 rows, <= 1280 at 33..64.  The scales sit behind the N_packed * K / 32 *
// S::TILE_K_BYTES code bytes.  other_form(): the stream's own refusals and its forms for more rows (g1_stream_launch, sjd_gemm_parts.h).
template <typename S, typename Other>
static int g1qb_launch(const void *x, const void *wq, float *out, int M, int N, int K, int KC, int waves, int step_major, int n_tiles, int tile0,
                       hipStream_t s, Other other_form)
{
    return g1_stream_launch(wq, M, N, K, KC, waves, step_major, n_tiles, tile0, S::TILE_K_BYTES, other_form,
        [&](auto mt, auto maxt, dim3 grid, dim3 block, size_t lds, const unsigned char *scales, int rs) {
            return g1_launch_kernel(g1qb_skinny_gemm<S, decltype(mt)::value, decltype(maxt)::value>, grid, block, lds, s, x, wq, scales, out, M, N, K, KC,
                                    n_tiles, rs, tile0, waves); });
}

// ... and of its gate|up kernel on sjd_gateup_silu (which has checked the common arguments: K in {512, 1024, 2048, 4096}, so a K half is a multiple
// of 128): M <= 32; the scales sit behind the 2 I * K / 32 * S::TILE_K_BYTES code bytes.
template <typename S>
static int g1sqb_launch(const void *x, const void *wq, void *y, int M, int I, int K, int step_major, const sjd_row_norm *rn, hipStream_t s)
{
    return g1s_stream_launch(wq, M, I, K, step_major, S::TILE_K_BYTES, rn,
        [&](auto sp, dim3 grid, dim3 block, size_t lds, const unsigned char *scales, int rec_stride, const g1s_norm_args &n) {
            return g1_launch_kernel(g1qb_gateup_silu<S, decltype(sp)::value>, grid, block, lds, s, x, wq, scales, y, M, I, K, rec_stride, n.ss, n.sl, n.ih,
                                    n.eps); });
}
