// sjd_gemm.hip -- G1: weight-streaming projection for the draft window (M <= 32 rows) on gfx950.
//
// One SJD iteration multiplies a [B_cfg*L = 32, K] activation by every weight matrix of the transformer: 13.5 GB of bf16
// weights streamed for 432 GFLOP -- intensity 32 flop/B, an order of magnitude under the ridge, so the op is a pure HBM
// stream and a 32-row problem is exactly ONE v_mfma_f32_32x32x16 tile tall.  rocprofv3 (profiles/r1b_*) shows the library
// GEMMs at 2.8-4.3 TB/s for these shapes; this kernel is written for the stream instead:
//
//   * weights are PRE-PACKED once (host, at load time) into MFMA-fragment-major order: unit (k-chunk c, 32-column tile t)
//     is `steps` consecutive 1-KiB records, record s = the B operand of k-step s, lane l holding
//     W[32t + (l&31)][k0 + 16s + 8(l>>5) .. +7].  A wave therefore reads ONE contiguous run of 16..64 KiB with
//     1-KiB-per-instruction 16-byte loads straight into MFMA operand registers -- no LDS, no transposes, no address math;
//   * the activation chunk x[:, k0:k0+KC] is staged once per workgroup in LDS in the same fragment-major order (A operand;
//     coalesced global reads, a per-record slot permutation keeps both the ds_write_b128 and the ds_read_b128 side free of
//     bank conflicts), shared by the 8 waves (8 column tiles) of the workgroup;
//   * split-K over grid.y gives every CU several waves; the fp32 partials [n_chunks, 32, N] are summed by the CONSUMER
//     kernel (F1 / F2 / F3 take n_chunks), so no reduction pass and no atomics;
//   * loads are issued 8 k-steps ahead of their MFMA (register double buffer) and marked non-temporal (read once).
#include <hip/hip_runtime.h>
#include <type_traits>

#include "../../include/sjd_hip.h"
#include "sjd_mlp_epilogue.h"
#include "sjd_coherent.h"
#ifdef SJD_EXPERIMENTAL
#include "sjd_l2_prefetch.h"
#endif

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// The launch sequence of every projection kernel in this file, sjd_gemm_wide.h and sjd_gemm_q8.h: raise the kernel's dynamic-LDS limit where the launch
// needs more than the 64 KiB a kernel gets unasked, launch, and map hipGetLastError() to SJD_OK / SJD_ERR_LAUNCH.  One argument per kernel parameter
// (a pointer to a kernel carries no default arguments).
template <typename... P, typename... A>
static int g1_launch_kernel(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args)
{
    static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, s, static_cast<P>(args)...);
    return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
}

// phase timestamps of g1_skinny_gemm (tools/phase_trace.py, -DSJD_TRACE; compiled out otherwise), see sjd_attention.hip
#ifdef SJD_TRACE
__device__ unsigned long long g_g1_trace[4096][8];
#define SJD_TR(i) do { if (threadIdx.x == 0) g_g1_trace[(blockIdx.y * gridDim.x + blockIdx.x) & 4095][i] = wall_clock64(); } while (0)
// slot 7: where the workgroup ran -- XCC_ID (hwreg 20) in the high word, HW_ID (hwreg 4: wave / SIMD / CU / SH / SE) in the low word
#define SJD_TR_HW() do { if (threadIdx.x == 0) g_g1_trace[(blockIdx.y * gridDim.x + blockIdx.x) & 4095][7] = \
    ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4); } while (0)
#define SJD_TR_CLK(i) do { if (threadIdx.x == 0) g_g1_trace[(blockIdx.y * gridDim.x + blockIdx.x) & 4095][i] = __builtin_readcyclecounter(); } while (0)
#else
#define SJD_TR(i) do { } while (0)
#define SJD_TR_HW() do { } while (0)
#define SJD_TR_CLK(i) do { } while (0)
#endif
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

#ifndef G1_UNROLL
#define G1_UNROLL 8
#endif
#define G1_STAGE 8          // activation pieces (16 B) a thread keeps in flight while staging

// Slot of an A-fragment piece inside its 1-KiB record (lane l = 32 half + mm of the MFMA operand).  The 64 pieces are permuted
// so that BOTH sides are bank-conflict free: the MFMA side reads a record with lanes = consecutive mm (fixed s), the staging
// side writes with lanes = consecutive (s, half) of ONE row (fixed mm).
__device__ __forceinline__ int g1_slot(int half, int mm, int s)
{
    return (half << 5) | (mm & 16) | ((mm & 15) ^ (((s & 7) << 1) | half));
}

template <int DT> struct G1Mfma;
template <> struct G1Mfma<SJD_DTYPE_BF16> {
    static __device__ __forceinline__ f32x16 mma(u32x4 a, u32x4 b, f32x16 c)
    { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0); }
};
template <> struct G1Mfma<SJD_DTYPE_F16> {
    static __device__ __forceinline__ f32x16 mma(u32x4 a, u32x4 b, f32x16 c)
    { return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0); }
};

#include "sjd_gemm_parts.h"         // (the constants and launcher bodies the G1 family shares)

#ifdef SJD_EXPERIMENTAL        // round-3 option (G1 with F1r as its tail)
// ---- F1r inside the producer (round 3; VERDICT r2 "next #3", the experiment DESIGN.md 4.6 item 6 stopped short of).
// Every workgroup of an o / down launch has written its fp32 partial tile with device-coherent stores.  The workgroups that share a
// 512-column SLICE of the output (16 / waves column groups x n_chunks K chunks: 16 for o, 26 for down) then meet at a ticket in device
// memory and each reduces a few ROWS of the slice: the chunk planes are read back with device-coherent 16-byte loads (all of them in
// flight at once), summed in chunk order, rounded, added to the residual stream h and squared -- F1r's arithmetic element by element
// (sjd_mlp_epilogue.h), one wave per (row, 256-column half) exactly as F1r's two waves, so h AND the per-slice sums of squares are
// bit-identical to G1 followed by F1r.  No L2 write-back / invalidate anywhere (that costs 14 us): coherence is per access.
// tools/last_arriver_probe.hip measured the scheme against the two graph nodes before it was built: o 19.3 -> 11.1 us, down 25.1 -> 20.4 us
// per pair (a last-arriver-does-all variant without the wait: 14.2 / 23.8), profiles/r3_last_arriver_probe.jsonl.
// The wait is bounded: all workgroups of a launch (<= 208) are resident at once on the 256 CUs, so the count completes within the
// launch; if it ever does not (a partitioned or shared GPU), the workgroup goes on after ~2^21 polls and raises g1_red_timeouts, which
// the host reads (sjd_reduce_timeouts) -- an error, not a hang.  The ticket resets itself: the launch is replayable from a hipGraph.
__device__ unsigned g1_red_timeouts;

template <int DT>
__device__ __forceinline__ void g1_reduce_tail(const float *__restrict__ part, unsigned short *__restrict__ h, float *__restrict__ sumsq,
                                               unsigned *__restrict__ ticket, int M, int N, int C, int chunk, int group, int n_waves)
{
    __shared__ float red[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int gps = 16 / n_waves;                       // column groups per 512-column slice (n_waves in {1, 2, 4, 8, 16})
    const int slice = group / gps;
    const unsigned total = (unsigned)(gps * C);
    unsigned *tk = ticket + 32 * slice;                 // [0]: arrivals, [16]: departures (another 64-byte line)
    __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0): this thread's plane stores are acknowledged (gfx9 counts stores there)
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned a = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
        int spins = 0;
        while (a < total && spins < (1 << 21)) { a = __hip_atomic_load(tk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); ++spins; }
        if (a < total) atomicAdd(&g1_red_timeouts, 1u);
    }
    __syncthreads();
    const int idx = (group % gps) * C + chunk;          // this workgroup among the slice's `total`
    const int per = (32 + (int)total - 1) / (int)total; // rows per workgroup
    const int row = idx * per + (w >> 1), half = w & 1;
    const bool work = (w < 2 * per) && (idx * per + (w >> 1) < 32) && row < M && (w >> 1) < per;
    float ss = 0.f;
    if (work) {
        const int col = slice * 512 + half * 256 + 4 * lane;
        const float *p0 = part + (size_t)row * N + col;
        const size_t cstride = (size_t)32 * N;
        sjd_f4 v[16];
#pragma unroll
        for (int ch = 0; ch < 16; ++ch)                                // all chunk planes of this thread's four columns in flight at once:
            v[ch] = sjd_ld_coherent_f4(p0 + (size_t)min(ch, C - 1) * cstride);      // UNCONDITIONAL (clamped) loads, or the compiler serialises them
        unsigned short *hp = h + (size_t)row * N + col;
        const uint2 hv = *reinterpret_cast<const uint2 *>(hp);
        float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll
        for (int ch = 0; ch < 16; ++ch) {
            const bool on = ch < C;
            d0 += on ? v[ch].x : 0.f; d1 += on ? v[ch].y : 0.f; d2 += on ? v[ch].z : 0.f; d3 += on ? v[ch].w : 0.f;
        }
        const float hx[4] = {SjdAct<DT>::to_f((unsigned short)(hv.x & 0xffffu)), SjdAct<DT>::to_f((unsigned short)(hv.x >> 16)),
                             SjdAct<DT>::to_f((unsigned short)(hv.y & 0xffffu)), SjdAct<DT>::to_f((unsigned short)(hv.y >> 16))};
        const float dd[4] = {d0, d1, d2, d3};
        unsigned short ob[4];
        float hn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { ob[j] = sjd_residual_elem<DT>(hx[j], dd[j]); hn[j] = SjdAct<DT>::to_f(ob[j]); }
        uint2 ho;
        ho.x = (unsigned)ob[0] | ((unsigned)ob[1] << 16);
        ho.y = (unsigned)ob[2] | ((unsigned)ob[3] << 16);
        *reinterpret_cast<uint2 *>(hp) = ho;
        ss = sjd_sumsq4(0.f, hn[0], hn[1], hn[2], hn[3]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);       // wave_sum of sjd_glue.hip
    if (lane == 0 && w < 16) red[w] = ss;
    __syncthreads();
    if ((int)threadIdx.x < per) {
        const int r = idx * per + (int)threadIdx.x;
        if (r < 32 && r < M) sumsq[(size_t)slice * 32 + r] = red[2 * threadIdx.x] + red[2 * threadIdx.x + 1];     // F1r: red[0] + red[1]
    }
    if (threadIdx.x == 0) {      // departures: the last one out re-arms the ticket for the next launch (everybody has passed the wait by then)
        const unsigned dp = __hip_atomic_fetch_add(tk + 16, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
        if (dp == total) {
            __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(tk + 16, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

#endif  // SJD_EXPERIMENTAL
// x: [M, K] row-major (M <= 32*MT; missing rows read as zero).  wp: packed weights.  out: fp32 [n_chunks, 32*MT, N].
// MT = 2 serves a 64-row window (B_cfg * L with a draft window of 32): every weight record feeds two MFMAs.
// Column window: the launch covers tiles [tile0, tile0 + N/32) of a weight packed with `n_tiles` tiles (N = columns of THIS launch's
// output): the output head is evaluated only for the vocabulary columns the grammar allows out of one packed copy.
// MAXT: 512 (<= 8 waves: 256 VGPRs, sixteen activation pieces per thread in flight -> a 2048-column chunk is staged in ONE round trip)
// or 1024 (9..16 waves, eight pieces).
// red_h != nullptr (round 3, MT = 1, <= 8 waves): the split-K reduction, the residual add and the row statistics -- stage F1r, until
// now a graph node of its own behind every o / down projection -- run in the TAIL of this kernel (g1_reduce_tail).  A RUN-TIME switch of
// the one kernel, not a second instantiation: the q|k|v, o and down launches of a layer then execute the same 12 KB of code.  The hot
// kernels of a layer (G1, G1s, K1, F2) add up to about the 64 KB instruction cache two CUs share; with a separate reducing instantiation
// next to the plain one the working set no longer fitted and EVERY configuration of the library lost 2-3 us per layer, whichever
// kernels it ran (bisected on one box by swapping single translation units, profiles/r3_code_layout_bisect.txt).
template <int DT, int MT, int MAXT>
__global__ __launch_bounds__(MAXT) void g1_skinny_gemm(const unsigned short *__restrict__ x, const u32x4 *__restrict__ wp,
                                                                float *__restrict__ out, int M, int N, int K, int KC, int n_tiles,
                                                                int rec_stride, int tile0, int n_waves,
                                                                unsigned short *__restrict__ red_h = nullptr, float *__restrict__ red_sumsq = nullptr,
                                                                unsigned *__restrict__ red_ticket = nullptr)
{
    // n_waves = blockDim.x / 64 as an ARGUMENT: blockDim lives in the implicit kernel arguments, which are not preloaded into SGPRs -- the
    // kernel opened with an s_load round trip for it in front of every address it computes (ISA, late round 2)
    SJD_TR(0);                    // entry
    SJD_TR_HW();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);
    const int chunk = blockIdx.y;
    const int k0 = chunk * KC;
    const int steps = min(KC, K - k0) / 16;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int waves = n_waves;
    const int t_out = blockIdx.x * waves + w;          // tile of this launch's output
    const int t = tile0 + t_out;                       // tile of the packed weight
    const bool has_tile = t_out < N / 32;
    // record (chunk, s, t) in 1-KiB units: all earlier chunks are full (KC/16 steps each).
    //   rec_stride == 1      : tile-major   -- a wave streams one contiguous run of `steps` KiB
    //   rec_stride == n_tiles: step-major   -- at every k-step the whole grid row reads n_tiles contiguous KiB, i.e. the
    //                                           chip sweeps the weight matrix like a linear copy (DRAM row locality)
    const size_t chunk_base = (size_t)chunk * n_tiles * (KC / 16);
    const size_t tile_off = (rec_stride == 1) ? (size_t)(has_tile ? t : 0) * steps : (size_t)(has_tile ? t : 0);
    const u32x4 *wu = wp + (chunk_base + tile_off) * 64 + lane;
    const size_t rs = (size_t)rec_stride * 64;
    u32x4 cur[G1_UNROLL], nxt[G1_UNROLL];
    const int full = steps / G1_UNROLL;
    // stage the activation chunk in A-fragment order: the piece of (row m, k-step s, half) = x[m][k0 + 16s + 8 half .. +7] goes
    // to record (mt, s), slot g1_slot(half, m % 32, s).  Pieces are walked in ROW order (coalesced 16-byte reads along k), eight
    // round trips in flight per thread.  The first weight group is requested right BEHIND the first batch of x loads: vector loads
    // retire in order, so the (cached) activation is not held up by the HBM round trip of the weights, and the weight loads
    // travel while the activation is written to LDS.
    const int ppr = 2 * steps;                                    // pieces per row of the chunk
    const int nth = n_waves * 64;
    constexpr int STAGE = MAXT <= 512 ? 2 * G1_STAGE : G1_STAGE;
    // piece v = (row m, 16-byte piece j of the row); a thread's pieces are nth apart: (m, j) advance without a division per piece
    const int dm = nth / ppr, dj = nth - dm * ppr;
    int pm = threadIdx.x / ppr, pj = threadIdx.x - pm * ppr;
    auto advance = [&](int &m, int &j) { m += dm; j += dj; if (j >= ppr) { j -= ppr; ++m; } };
    auto x_load = [&](int m, int j) -> u32x4 {
        return (m < M) ? *reinterpret_cast<const u32x4 *>(x + (size_t)m * K + k0 + 8 * j) : u32x4{0u, 0u, 0u, 0u};      // (M <= 32 MT)
    };
    auto x_store = [&](int m, int j, u32x4 val) {
        const int s = j >> 1;
        if (m < 32 * MT) xl[((m >> 5) * steps + s) * 64 + g1_slot(j & 1, m & 31, s)] = val;
    };
    {   // first batch, then the first weight group right behind it.  The weight loads are UNCONDITIONAL (a wave without a tile reads
        // tile 0, a chunk shorter than a group re-reads its last record): the compiler can then count them and wait for the activation
        // with vmcnt(8) -- with a conditional block it waits with vmcnt(0), i.e. the LDS writes and the barrier below sat behind the
        // whole HBM round trip of the weights (in-kernel timestamps, round 2: 1.7 us).
        u32x4 val[STAGE];
        int m = pm, j = pj;
#pragma unroll
        for (int i = 0; i < STAGE; ++i) { val[i] = x_load(m, j); advance(m, j); }
#pragma unroll
        for (int u = 0; u < G1_UNROLL; ++u) cur[u] = __builtin_nontemporal_load(wu + (size_t)min(u, steps - 1) * rs);
        m = pm; j = pj;
#pragma unroll
        for (int i = 0; i < STAGE; ++i) { x_store(m, j, val[i]); advance(m, j); }
        pm = m; pj = j;
    }
    while (pm < 32 * MT) {                                         // what is left of a tall / long chunk
        u32x4 val[G1_STAGE];
        int m = pm, j = pj;
#pragma unroll
        for (int i = 0; i < G1_STAGE; ++i) { val[i] = x_load(m, j); advance(m, j); }
        m = pm; j = pj;
#pragma unroll
        for (int i = 0; i < G1_STAGE; ++i) { x_store(m, j, val[i]); advance(m, j); }
        pm = m; pj = j;
    }
    SJD_TR(1);                    // this wave's share of the activation chunk is in LDS
    __syncthreads();
    SJD_TR(2);                    // all of it is
    if (!has_tile) return;
    // Nothing may be pending on the vector-memory counter when the main loop is entered: the compiler places ONE s_waitcnt per MFMA
    // for every path into the loop, and with the prologue's weight loads possibly outstanding it would wait for the group just
    // issued (vmcnt(7)..vmcnt(0)) instead of letting the MFMAs of this group run under the loads of the next one.
    __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0)
    SJD_TR(3);                    // first weight group arrived
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;
    const int xs = steps * 64;           // records per m-tile in LDS
    for (int g = 0; g < full; ++g) {
        const bool more = g + 1 < full;
        if (more) {
#pragma unroll
            for (int u = 0; u < G1_UNROLL; ++u) nxt[u] = __builtin_nontemporal_load(wu + (size_t)((g + 1) * G1_UNROLL + u) * rs);
        }
#pragma unroll
        for (int u = 0; u < G1_UNROLL; ++u)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                acc[mt] = G1Mfma<DT>::mma(xl[mt * xs + (g * G1_UNROLL + u) * 64 + g1_slot(lane >> 5, lane & 31, u)], cur[u], acc[mt]);
        if (more) {
#pragma unroll
            for (int u = 0; u < G1_UNROLL; ++u) cur[u] = nxt[u];
        }
    }
    {   // ragged tail (K chunk not a multiple of 128): its up to seven records in ONE round trip (they used to be seven)
        const int s0 = full * G1_UNROLL, rem = steps - s0;
        u32x4 tl[G1_UNROLL - 1];
#pragma unroll
        for (int u = 0; u < G1_UNROLL - 1; ++u)
            if (u < rem) tl[u] = __builtin_nontemporal_load(wu + (size_t)(s0 + u) * rs);
#pragma unroll
        for (int u = 0; u < G1_UNROLL - 1; ++u)
            if (u < rem) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    acc[mt] = G1Mfma<DT>::mma(xl[mt * xs + (s0 + u) * 64 + g1_slot(lane >> 5, lane & 31, s0 + u)], tl[u], acc[mt]);
            }
    }

    SJD_TR(4);                    // main loop done
    // D[m][n]: reg r of lane l -> row m = (r&3) + 8*(r>>2) + 4*(l>>5), column n = 32t + (l&31): 128-B coalesced rows
    float *o = out + ((size_t)chunk * (32 * MT)) * N + (size_t)t_out * 32 + (lane & 31);
#ifdef SJD_EXPERIMENTAL        // (the reducing tail: libsjd_hip_exp.so only -- the product kernel is compiled without it)
    if constexpr (MT == 1 && MAXT == 512) if (red_h) {
#pragma unroll
        for (int r = 0; r < 16; ++r)          // the plane goes out DEVICE-COHERENT (sc1: written through this XCD's L2)
            __hip_atomic_store(o + (size_t)((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * N, acc[0][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        g1_reduce_tail<DT>(out, red_h, red_sumsq, red_ticket, M, N, (int)gridDim.y, chunk, (int)blockIdx.x, n_waves);
        return;
    }
#endif
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            o[(size_t)m * N] = acc[mt][r];        // (non-temporal stores measured slower end to end: 3.55 / 3.57 against 3.52 ms/step)
        }
#ifdef SJD_TRACE
    SJD_TR(5);                    // partial stores issued
    __builtin_amdgcn_s_waitcnt(0x0F70);
    SJD_TR(6);                    // acknowledged
#endif
}


// ---- windows of 65..128 rows (three / four prompts per forward): MT = 3, 4.
// The whole activation chunk no longer fits in LDS (128 rows x 896 columns = 224 KiB), so it is staged in SUB-TILES of G1_SUB = 16 k-steps
// (256 columns: MT x 16 KiB), double-buffered: the global loads of sub-tile i+1 are issued before the MFMAs of sub-tile i and written to
// the other LDS buffer behind them.  KC -- and with it the number of fp32 partial planes the consumer sums -- stays what it is for 32 rows.
// With four MFMAs per weight record the wave is no longer idle between memory round trips, so the loop is written for the scheduler:
//   * a sub-tile is exactly two weight groups held in two register sets A and B that alternate WITHOUT copies; the group after next is
//     requested before the MFMAs of the current one, so 8 KiB per wave stay in flight through the MFMAs AND through the barrier;
//   * every load is unconditional (row / column / group indices are clamped, invalid pieces are zeroed after the load, a wave without a
//     column tile multiplies tile 0 and skips the store): straight-line code, for which the compiler's s_waitcnt counts are exact
//     (vmcnt(N) leaves the younger loads in flight; a conditional load forces vmcnt(0));
//   * the A operands of k-step u+1 are read from LDS while the MFMAs of k-step u issue.
// <= 8 waves (up to 256 VGPRs).
#define G1_SUB 16
template <int DT, int MT>
__device__ __forceinline__ void g1_group(const u32x4 *__restrict__ xb, int sl0, const u32x4 (&W)[G1_UNROLL], f32x16 (&acc)[MT], int lane)
{
    u32x4 a[2][MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) a[0][mt] = xb[(mt * G1_SUB + sl0) * 64 + g1_slot(lane >> 5, lane & 31, 0)];
#pragma unroll
    for (int u = 0; u < G1_UNROLL; ++u) {
        if (u + 1 < G1_UNROLL) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[(u + 1) & 1][mt] = xb[(mt * G1_SUB + sl0 + u + 1) * 64 + g1_slot(lane >> 5, lane & 31, u + 1)];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a[u & 1][mt], W[u], acc[mt]);
    }
}

template <int DT, int MT>
__global__ __launch_bounds__(512) void g1_skinny_gemm_tiled(const unsigned short *__restrict__ x, const u32x4 *__restrict__ wp,
                                                                     float *__restrict__ out, int M, int N, int K, int KC, int n_tiles,
                                                                     int rec_stride, int tile0, int n_waves)
{
    SJD_TR(0);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);                 // two buffers of MT * G1_SUB records
    const int chunk = blockIdx.y;
    const int k0 = chunk * KC;
    const int steps = min(KC, K - k0) / 16;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int waves = n_waves;
    const int t_out = blockIdx.x * waves + w;
    const bool has_tile = t_out < N / 32;                        // a wave without a tile multiplies tile 0 and stores nothing
    const int t = tile0 + (has_tile ? t_out : 0);
    const size_t chunk_base = (size_t)chunk * n_tiles * (KC / 16);
    const size_t tile_off = (rec_stride == 1) ? (size_t)t * steps : (size_t)t;
    const u32x4 *wu = wp + (chunk_base + tile_off) * 64 + lane;
    const size_t rs = (size_t)rec_stride * 64;
    const int nth = n_waves * 64;
    constexpr int BUF = MT * G1_SUB * 64;                         // u32x4 per LDS buffer
    constexpr int PPR = 2 * G1_SUB;                               // 16-byte pieces per row of a sub-tile
    constexpr int NP = MT * 32 * PPR;                             // pieces per sub-tile
    constexpr int NV = NP / 512;                                  // pieces per thread at 512 threads (2 MT)
    const int full = steps / G1_UNROLL;                           // whole weight groups of the chunk
    const int n_sub_full = steps / G1_SUB, rem = steps - n_sub_full * G1_SUB;
    const int k_end = k0 + steps * 16;
    u32x4 A[G1_UNROLL], B[G1_UNROLL];
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;
    // piece v of sub-tile st: row m = v / PPR, 8 columns from k0 + 256 st + 8 (v % PPR); always a legal address, zero if outside the chunk
    auto x_load = [&](int st, int v) -> u32x4 {
        const int m = v / PPR, j = v - m * PPR, col = k0 + st * (16 * G1_SUB) + 8 * j;
        const u32x4 val = *reinterpret_cast<const u32x4 *>(x + (size_t)min(m, M - 1) * K + min(col, K - 8));
        return (m < M && col < k_end) ? val : u32x4{0u, 0u, 0u, 0u};
    };
    auto x_store = [&](int buf, int v, u32x4 val) {
        const int m = v / PPR, j = v - m * PPR, sl = j >> 1;
        xl[buf * BUF + ((m >> 5) * G1_SUB + sl) * 64 + g1_slot(j & 1, m & 31, sl)] = val;
    };
    auto w_load = [&](u32x4 (&W)[G1_UNROLL], int g) {
        const int gc = max(0, min(g, full - 1));                  // clamped: a group past the end re-reads the last one and is not used
#pragma unroll
        for (int u = 0; u < G1_UNROLL; ++u) W[u] = __builtin_nontemporal_load(wu + (size_t)(gc * G1_UNROLL + u) * rs);
    };
    auto stage = [&](int st_next, int buf, u32x4 (&val)[NV], bool load) {      // (load / store halves of staging sub-tile st_next)
        if (load) {
#pragma unroll
            for (int i = 0; i < NV; ++i) val[i] = x_load(st_next, min(threadIdx.x + i * nth, NP - 1));
        } else {
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (threadIdx.x + i * nth < NP) x_store(buf, threadIdx.x + i * nth, val[i]);
            for (int v = threadIdx.x + NV * nth; v < NP; v += nth) x_store(buf, v, x_load(st_next, v));      // fewer than 8 waves
        }
    };
    {
        u32x4 val[NV];
        stage(0, 0, val, true);
        if (steps >= G1_UNROLL) w_load(A, 0);
        stage(0, 0, val, false);
    }
    __syncthreads();
    SJD_TR(1);                    // first sub-tile staged
    // all full sub-tiles but the last: the next sub-tile and the group after next always exist -> unconditional, straight-line
    for (int st = 0; st + 1 < n_sub_full; ++st) {
        const u32x4 *xb = xl + (st & 1) * BUF;
        u32x4 val[NV];
        // (sched_barrier: the machine scheduler otherwise sinks the loads into the MFMA sequence to save registers, i.e. issues them late)
        stage(st + 1, (st + 1) & 1, val, true);
        w_load(B, 2 * st + 1);
        __builtin_amdgcn_sched_barrier(0);
        g1_group<DT, MT>(xb, 0, A, acc, lane);
        __builtin_amdgcn_sched_barrier(0);
        if (st == 1) SJD_TR(5);       // (second sub-tile: group A multiplied)
        w_load(A, 2 * st + 2);
        __builtin_amdgcn_sched_barrier(0);
        g1_group<DT, MT>(xb, G1_UNROLL, B, acc, lane);
        __builtin_amdgcn_sched_barrier(0);
        if (st == 1) SJD_TR(6);       // (group B multiplied)
        stage(st + 1, (st + 1) & 1, val, false);
        if (st == 1) SJD_TR(7);       // (next sub-tile written to LDS)
        __syncthreads();
        if (st == 0) SJD_TR(4);       // (first sub-tile done, barrier passed)
    }
    SJD_TR(2);                    // all but the last full sub-tile done
    if (n_sub_full > 0) {                                           // last full sub-tile: what follows it may not exist (uniform branches)
        const int st = n_sub_full - 1;
        const u32x4 *xb = xl + (st & 1) * BUF;
        u32x4 val[NV];
        if (rem > 0) stage(st + 1, (st + 1) & 1, val, true);
        w_load(B, 2 * st + 1);
        g1_group<DT, MT>(xb, 0, A, acc, lane);
        if (rem >= G1_UNROLL) w_load(A, 2 * st + 2);
        g1_group<DT, MT>(xb, G1_UNROLL, B, acc, lane);
        if (rem > 0) stage(st + 1, (st + 1) & 1, val, false);
        __syncthreads();
    }
    if (rem > 0) {                                                  // last, partial sub-tile: one whole group (in A) and / or single k-steps
        const u32x4 *xb = xl + (n_sub_full & 1) * BUF;
        int sl = 0;
        if (rem >= G1_UNROLL) { g1_group<DT, MT>(xb, 0, A, acc, lane); sl = G1_UNROLL; }
        for (; sl < rem; ++sl) {
            const u32x4 wv = __builtin_nontemporal_load(wu + (size_t)(n_sub_full * G1_SUB + sl) * rs);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(xb[(mt * G1_SUB + sl) * 64 + g1_slot(lane >> 5, lane & 31, sl)], wv, acc[mt]);
        }
    }
    SJD_TR(3);                    // main loop done
    if (!has_tile) return;
    float *o = out + ((size_t)chunk * (32 * MT)) * N + (size_t)t_out * 32 + (lane & 31);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            o[(size_t)m * N] = acc[mt][r];
        }
}

// ---- 65..128-row windows, second form (round 3): TWO workgroups per CU.
// The kernel above owns a CU alone (2 x MT x 16 KiB of LDS, 8 waves x ~250 VGPRs), and its 8 waves meet at a barrier every 16 k-steps with
// one weight group per wave in flight: the phase stamps put 0.45 us of LDS writes + ~0.7 us of barrier on top of every 3.2-4 us sub-tile.
// Here a sub-tile is 8 k-steps = ONE weight group, a workgroup is 4 waves and 2 x MT x 8 KiB of LDS (64 KiB at four row tiles), so two
// workgroups share a CU (2 waves per SIMD, <= 256 VGPRs each as before): while one stages and waits at its barrier the other streams and
// multiplies.  The weight sets A / B are a ring of 16 k-steps refilled in place; the activation pieces of the NEXT sub-tile are requested
// before the MFMAs of the current one; every load is unconditional (a record past the chunk reads as zero through the wave's buffer
// descriptor, an activation piece past it is zeroed on its way into LDS) and the loop has no branch but its back edge.  Same MFMA
// sequence per (tile, chunk, row tile) as g1_skinny_gemm: bit-identical planes.
// NW = 8 (late round 3): the same loop with eight waves -- one workgroup per CU again, but its staged sub-tile feeds eight column tiles
// (half the activation re-reads per weight byte); every 8-wave launch of a 65..128-row window runs here instead of the 16-step kernel
// (gate|up 49.4 -> 43.3 us, q|k|v 29.4 -> 26.7, down 29.3 -> 25.2).
// Probe builds (-DT8_NOSTORE / -DT8_NOX / -DT8_NOMFMA, profiles/r3_g1_tiled8.txt): the partial planes cost 3-6 us of a 25-49 us launch, the
// activation staging 6-7 us.  Two things measured against the planes and NOT kept: the tiles written through LDS as 16-byte row pieces
// (16 stores per wave instead of 64: no gain -- it is not the address pipe) and non-temporal plane stores (q|k|v 28.7 -> 25.3 us, down
// 25.0 -> 22.5 alone, but 5.098 -> 5.091 ms per step with four prompts: the consumer kernel pays for them).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t g1z_unit_rsrc(const unsigned char *first_record, unsigned bytes);
template <int DT, int MT, int NW>           // NW = 4: two workgroups per CU; NW = 8 (late round 3): one, its staged sub-tile shared by eight column tiles
__global__ __launch_bounds__(64 * NW, (NW == 4 && MT <= 4) ? 2 : 1) void g1_skinny_gemm_tiled8(const unsigned short *__restrict__ x, const u32x4 *__restrict__ wp,
                                                                float *__restrict__ out, int M, int N, int K, int KC, int n_tiles,
                                                                int rec_stride, int tile0)
{
    SJD_TR(0);
    constexpr int SUB = 8;
    static_assert(G1_UNROLL == SUB, "a sub-tile is one weight group");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);                 // two buffers of MT * SUB records
    const int chunk = blockIdx.y;
    const int k0 = chunk * KC;
    const int steps = min(KC, K - k0) / 16;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int t_out = blockIdx.x * NW + w;                        // exactly NW waves (the launcher sends other wave counts to the 16-step kernel)
    const bool has_tile = t_out < N / 32;                        // a wave without a tile multiplies tile 0 and stores nothing
    const int t = tile0 + (has_tile ? t_out : 0);
    const size_t chunk_base = (size_t)chunk * n_tiles * (KC / 16);
    const size_t tile_off = (rec_stride == 1) ? (size_t)t * steps : (size_t)t;
    // one buffer descriptor per wave over its unit: records past the unit's end read as zero WITHOUT touching memory, the record offset is a
    // scalar and the lane offset the only address register (the eight 64-bit addresses of a group spilled at four row tiles)
    const unsigned rsb = (unsigned)rec_stride * 1024u;
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(reinterpret_cast<const unsigned char *>(wp + (chunk_base + tile_off) * 64),
                                                    (unsigned)(steps - 1) * rsb + 1024u);
    constexpr int BUF = MT * SUB * 64;                            // u32x4 per LDS buffer
    constexpr int PPR = 2 * SUB;                                  // 16-byte pieces per row of a sub-tile
    constexpr int NP = MT * 32 * PPR;                             // pieces per sub-tile
    constexpr int NV = NP / (64 * NW);                            // pieces per thread (2 MT at four waves, MT at eight)
    const int n_sub = (steps + SUB - 1) / SUB;
    const int k_end = k0 + steps * 16;
    u32x4 A[SUB], B[SUB];
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;
    // activation pieces through a buffer descriptor over x [M, K] as well: a row >= M (its product rows must be zero) or a piece past the
    // matrix reads as zero; the pieces past the chunk's last k-step are zeroed on their way into LDS.  One 32-bit offset per thread.
    const __amdgpu_buffer_rsrc_t xr = g1z_unit_rsrc(reinterpret_cast<const unsigned char *>(x), (unsigned)M * (unsigned)K * 2u);
    // thread tid stages pieces tid + 256 i: row m0 + 16 i (m0 = tid / 16 < 16), the SAME 8 columns j0 = tid % 16 of the sub-tile for every
    // i -- so the global offset of piece i is ONE per-lane offset + the scalar (16 i) rows, its LDS slot ONE per-lane slot + a constant
    // (row tile i / 2, bit 4 of the row = i & 1), and the column test below is one compare per sub-tile (16 address / predicate registers less).
    const int m0 = threadIdx.x >> 4, j0 = threadIdx.x & 15;      // (eight waves: pieces tid + 512 i = row m0 + 32 i, m0 < 32 -- row tile i)
    const unsigned x_off0 = ((unsigned)m0 * (unsigned)K + (unsigned)(k0 + 8 * j0)) * 2u;
    const int x_slot0 = (j0 >> 1) * 64 + g1_slot(j0 & 1, m0, j0 >> 1);      // (includes bit 4 of m0 at eight waves)
    auto x_load = [&](int st, int i) -> u32x4 {                   // (a row >= M lies past the descriptor's end: zero)
        const unsigned so = (unsigned)__builtin_amdgcn_readfirstlane(st) * (32u * SUB) + (unsigned)(8 * NW * i) * (unsigned)K;      // (4 NW rows on)
        return __builtin_amdgcn_raw_buffer_load_b128(xr, x_off0, so, 0);
    };
    auto x_store = [&](int st, int buf, int i, u32x4 val) {       // (the zeroing sits on the store side: the loads stay in flight through the MFMAs)
        xl[buf * BUF + (NW == 4 ? (i >> 1) * (SUB * 64) + ((i & 1) << 4) : i * (SUB * 64)) + x_slot0] =
            (k0 + st * (16 * SUB) + 8 * j0 < k_end) ? val : u32x4{0u, 0u, 0u, 0u};          // (a column past the chunk is the next chunk's or the next row's)
    };
    auto w_rec = [&](int g, int u) -> u32x4 {                     // k-step 8 g + u of the chunk
        return __builtin_amdgcn_raw_buffer_load_b128(wr, (unsigned)lane * 16u, (unsigned)(__builtin_amdgcn_readfirstlane(g) * SUB + u) * rsb, 2 /* nt */);
    };
    auto stage = [&](int st_next, int buf, u32x4 (&val)[NV], bool load) {
#ifdef T8_NOX             // (probe: only the first sub-tile is staged; every sub-tile multiplies it)
        if (st_next > 0) return;
#endif
        if (load) {
#pragma unroll
            for (int i = 0; i < NV; ++i) val[i] = x_load(st_next, i);
        } else {
#pragma unroll
            for (int i = 0; i < NV; ++i) x_store(st_next, buf, i, val[i]);
        }
    };
    // one sub-tile: no branches.  The A operands of k-step u + 1 are read from LDS before the MFMAs of k-step u issue; a weight record is
    // REFILLED IN PLACE right after its MFMAs with the record two sub-tiles on (the sets A / B are a ring of 16 k-steps: 8-16 KiB per wave
    // in flight through the MFMAs and the barrier, no second copy of a set).  The k-steps past a ragged chunk's end multiply zero records
    // by zeroed activation pieces: +0 added to an accumulator that is never -0 (it starts at +0) leaves every bit as it is.
    auto sub_tile = [&](const u32x4 *xb, u32x4 (&W)[SUB], int g_refill) {
        u32x4 a[2][MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[0][mt] = xb[(mt * SUB) * 64 + g1_slot(lane >> 5, lane & 31, 0)];
#pragma unroll
        for (int u = 0; u < SUB; ++u) {
            if (u + 1 < SUB) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) a[(u + 1) & 1][mt] = xb[(mt * SUB + u + 1) * 64 + g1_slot(lane >> 5, lane & 31, u + 1)];
            }
            __builtin_amdgcn_sched_barrier(0);                    // (the scheduler otherwise sinks each LDS read to its MFMA and the refills to the end)
#ifdef T8_NOMFMA      // (probe: the stream and the staging without the matrix cores)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt][u] += __builtin_bit_cast(float, a[u & 1][mt].x ^ W[u].x);
#else
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a[u & 1][mt], W[u], acc[mt]);
#endif
            W[u] = w_rec(g_refill, u);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    {
        u32x4 val[NV];
        stage(0, 0, val, true);
#pragma unroll
        for (int u = 0; u < SUB; ++u) A[u] = w_rec(0, u);
#pragma unroll
        for (int u = 0; u < SUB; ++u) B[u] = w_rec(1, u);
        stage(0, 0, val, false);
    }
    __syncthreads();
    SJD_TR(1);                    // first sub-tile staged
    int st = 0;
    for (; st + 1 < n_sub; st += 2) {                             // pairs of sub-tiles: set A on LDS buffer 0, set B on buffer 1
        {
            u32x4 val[NV];
            stage(st + 1, 1, val, true);
            __builtin_amdgcn_sched_barrier(0);
            sub_tile(xl, A, st + 2);
            __builtin_amdgcn_sched_barrier(0);
            stage(st + 1, 1, val, false);
            __syncthreads();
        }
        {
            u32x4 val[NV];
            stage(st + 2, 0, val, true);                          // (past the last sub-tile: zeros nobody reads)
            __builtin_amdgcn_sched_barrier(0);
            sub_tile(xl + BUF, B, st + 3);
            __builtin_amdgcn_sched_barrier(0);
            stage(st + 2, 0, val, false);
            __syncthreads();
        }
    }
    if (st < n_sub) sub_tile(xl, A, st + 2);                      // an odd number of sub-tiles: the last one (its refills read as zero)
    SJD_TR(3);                    // main loop done
#ifdef T8_NOSTORE         // (probe: no partial planes)
    if (acc[0][0] != 12345.0f) return;
#endif
    if (!has_tile) return;
    float *o = out + ((size_t)chunk * (32 * MT)) * N + (size_t)t_out * 32 + (lane & 31);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            o[(size_t)m * N] = acc[mt][r];
        }
}


#ifdef SJD_EXPERIMENTAL        // weight prefetch / L2 head pulls (rounds 2 and 5, measured no-go) and the XCC map probe
// ------------------------------------------------------------------------------------------------ weight prefetch
// While the latency-bound kernels of a layer run (F1r / F2 / K1 / combine / F3: ~1.15 ms of a 3.9 ms step, rocprofv3 round 1) HBM is
// idle although the step as a whole is bound by the 13 GB weight stream.  This kernel, launched on a SIDE stream (a parallel branch of
// the forward hipGraph), reads the packed weights of the NEXT projection with plain (temporal) 16-byte loads and throws them away:
// the lines land in the 256 MiB memory-side Infinity Cache, so the G1 launch that follows streams from there instead of from HBM.
// It owns few resources on purpose (small grid, ~16 VGPRs, no LDS) so that it co-resides with whatever the main branch is running.
__global__ __launch_bounds__(256) void g1_prefetch(const u32x4 *__restrict__ p, size_t n_vec, unsigned *__restrict__ sink)
{
    const size_t nthreads = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    u32x4 acc = {0u, 0u, 0u, 0u};
    for (; i + 3 * nthreads < n_vec; i += 4 * nthreads) {          // grid-stride, four 16-B loads in flight per lane
        const u32x4 a = p[i], b = p[i + nthreads], c = p[i + 2 * nthreads], d = p[i + 3 * nthreads];
        acc ^= a ^ b ^ c ^ d;
    }
    for (; i < n_vec; i += nthreads) acc ^= p[i];
    // never true for real data in practice, but the compiler cannot prove it: keeps the loads alive without a store
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x9e3779b9u && acc.x == 0x7f4a7c15u) sink[0] = acc.x;
}

extern "C" int sjd_weight_prefetch(const void *w, int64_t nbytes, int blocks, void *sink, void *stream)
{
    if (!w || !sink || nbytes < 16 || blocks < 1 || blocks > 4096) return SJD_ERR_BAD_ARG;
    return g1_launch_kernel(g1_prefetch, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, (size_t)(nbytes / 16), sink);
}

// ------------------------------------------------------------------------------------------------ L2 head pull (round 5, sjd_l2_prefetch.h)
__global__ __launch_bounds__(256) void g1_l2_head_pull(const sjd_l2_head d) { sjd_l2_head_pull(d, (int)blockIdx.x, (int)gridDim.x); }

__global__ void g1_xcc_map(int *out)
{
    if (threadIdx.x == 0) {
        unsigned v;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
        out[blockIdx.y * gridDim.x + blockIdx.x] = (int)(v & 0xfu);
    }
}

extern "C" int sjd_debug_xcc_map(int32_t *out, int gx, int gy, void *stream)
{
    if (!out || gx < 1 || gy < 1) return SJD_ERR_BAD_ARG;
    return g1_launch_kernel(g1_xcc_map, dim3(gx, gy), dim3(64), 0, (hipStream_t)stream, out);
}

// the grid sjd_skinny_gemm_z launches for these arguments (kept next to it: see SJD_G1Z_LAUNCH / SJD_G1ZT below)
extern "C" int sjd_l2_head_gemm_z(sjd_l2_head *out, const void *wz, int M, int N, int K, int KC, int waves, int step_major, int N_packed, int tile0, int head_pairs)
{
    if (!out || !wz || M < 1 || N < 32 || (N % 32) || (N_packed % 32) || (K % 16) || KC < 16 || (KC % 16) || waves < 1 || waves > 16 || head_pairs < 1)
        return SJD_ERR_BAD_ARG;
    const int n_out = N / 32, n_tiles = N_packed / 32, n_chunks = (K + KC - 1) / KC;
    if (tile0 < 0 || tile0 + n_out > n_tiles) return SJD_ERR_BAD_ARG;
    const int steps_last = (K - (n_chunks - 1) * KC) / 16;
    out->wz = wz;
    out->kind = 0;
    out->gx = (n_out + waves - 1) / waves;
    out->gy = n_chunks;
    out->waves = waves;
    out->n_tiles = n_tiles;
    out->tile0 = tile0;
    out->n_out = n_out;
    out->pairs_full = (KC / 16 + 1) / 2;
    out->pairs_last = (steps_last + 1) / 2;
    out->step_major = step_major ? 1 : 0;
    out->head_pairs = head_pairs < out->pairs_full ? head_pairs : out->pairs_full;
    return SJD_OK;
}

extern "C" int sjd_l2_head_gateup_z(sjd_l2_head *out, const void *wz, int M, int I, int K, int step_major, int head_pairs)
{
    if (!out || !wz || M < 1 || M > 64 || I < 64 || (I % 64) || K < 512 || (K % 64) || head_pairs < 1) return SJD_ERR_BAD_ARG;
    out->wz = wz;
    out->kind = 1;
    out->gx = I / 64;
    out->gy = 1;
    out->waves = 8;
    out->n_tiles = 2 * (I / 32);
    out->tile0 = 0;
    out->n_out = out->n_tiles;
    out->pairs_full = out->pairs_last = K / 64;
    out->step_major = step_major ? 1 : 0;
    out->head_pairs = head_pairs < out->pairs_full ? head_pairs : out->pairs_full;
    return SJD_OK;
}

extern "C" int64_t sjd_l2_head_bytes(const sjd_l2_head *d)
{
    if (!d) return 0;
    int64_t pairs = 0;
    if (d->kind == 0) {
        for (int by = 0; by < d->gy; ++by) {
            const int pu = by == d->gy - 1 ? d->pairs_last : d->pairs_full;
            pairs += (int64_t)d->n_out * (pu < d->head_pairs ? pu : d->head_pairs);
        }
    } else pairs = (int64_t)d->gx * 8 * d->head_pairs;
    return pairs * 1536;
}

extern "C" int sjd_weight_prefetch_head(const sjd_l2_head *head, int blocks, void *stream)
{
    if (!head || !head->wz || blocks < 8 || (blocks % 8) || blocks > 4096) return SJD_ERR_BAD_ARG;
    return g1_launch_kernel(g1_l2_head_pull, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *head);
}

// ------------------------------------------------------------------------------------------------ G1s (gate|up + SiLU * up in one launch)
// Per layer the MLP was gate|up G1 (split-K over two workgroup rows) -> F3 (sums the two fp32 partial planes, row scale, SiLU, product) ->
// down G1.  F3 is a dependent stage at its latency floor (4.8 us in situ: a graph-node boundary plus one cold round trip for 5.6 MB of
// partials another XCD has just written) and the per-workgroup timestamps of this round show the projections themselves streaming at
// 6.7 TB/s between their first load and their last: what is left to take out of a layer is STAGES, not bytes per second.
// Here the K split moves INSIDE the workgroup: 8 waves = 4 column tiles (gate tiles 2j, 2j+1 and the up tiles of the same columns) x the
// two K halves, i.e. every wave still streams exactly the run of records it streamed before (one tile, one half of K, same order, same
// accumulator), from the SAME packed weight (pack_weight(W, K/2)), and the grid is still I/64 = 172 workgroups.  The activation no longer
// fits in LDS at once (32 x 4096 bf16 = 256 KiB): it is staged in two PHASES of 2 x (K/4) columns -- the first quarter of each K half,
// then the second -- with one restaging between them whose global loads are issued a whole weight group ahead of the barrier.
// Epilogue: the plane of K half 1 and the up planes go through LDS (reusing the activation arena) to the two gate waves of K half 0, which
// apply F3's arithmetic -- (0 + p0 + p1), row scale, rounding to the activation dtype where nn.Linear / SiLU would round -- and write
// the 16-bit activation of the down projection.  Same operations in the same order as G1 + F3: the result is BIT-IDENTICAL
// (tests/test_gpu_glue.py::test_g1_gateup_silu_matches_g1_then_f3), so nothing downstream changes.
// replaces, like G1 + F3: gate_proj / up_proj / act_fn / the product of ChameleonMLP.forward (reference modeling_chameleon.py:193-195).
// SP = k-steps per phase per K half = K / 64 (K = 4096: 64).
#endif  // SJD_EXPERIMENTAL
template <int DT, int SP>
__global__ __launch_bounds__(512) void g1_gateup_silu(const unsigned short *__restrict__ x, const u32x4 *__restrict__ wp,
                                                      unsigned short *__restrict__ y, int M, int I, int K, int rec_stride,
                                                      const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden, float rs_eps)
{
    SJD_TR(0);
    SJD_TR_HW();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);                  // [2 K halves][SP records][64 slots] of 16 B
    __shared__ float rsc[32];
    constexpr int GP = SP / 8;                                    // weight groups per phase
    constexpr int PPS = 2 * SP;                                   // 16-byte pieces per (row, K half) of a phase
    constexpr int NPT = (32 * 2 * PPS) / 512;                     // pieces per thread and phase (K = 4096: 16)
    static_assert(SP % 8 == 0 && NPT >= 1, "phase = whole weight groups, at least one piece per thread");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int kh = w >> 2, q = w & 3;                             // K half; 0, 1 = gate tiles, 2, 3 = the up tiles of the same columns
    const int n_gate = I / 32, n_tiles = 2 * n_gate;
    const int t_act = 2 * blockIdx.x + (q & 1);                   // 32-column tile of the activation
    const int t = (q < 2 ? 0 : n_gate) + t_act;                   // tile of the packed gate|up weight
    const int steps = 2 * SP;                                     // k-steps of a K half (= of a chunk of the packed weight)
    const size_t chunk_base = (size_t)kh * n_tiles * steps;
    const size_t tile_off = (rec_stride == 1) ? (size_t)t * steps : (size_t)t;
    const u32x4 *wu = wp + (chunk_base + tile_off) * 64 + lane;
    const size_t rs = (size_t)rec_stride * 64;
    // piece v of a phase: row m = v / (2 PPS), K half hh = (v / PPS) & 1, piece j of that (row, half): 8 columns from
    // hh * K/2 + ph * K/4 + 8 j -> record hh * SP + j / 2, slot g1_slot(j & 1, m, j / 2)
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
    u32x4 cur[G1_UNROLL], nxt[G1_UNROLL], val[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(0, i);
    // the per-slice sums of h^2 behind the row scale r = rsqrt(mean(h^2) + eps) of the folded RMSNorm (F1r wrote them; K <= 4096: at most
    // eight slices).  Every thread issues the eight loads -- unconditional, so the waits around them stay exact -- BEHIND the activation
    // and ahead of the weights: they are cache hits and cost the staging nothing (first version: threads 0..31 did this first, +0.7 us).
    float ssv[8];
    g1s_row_sumsq_load<32>(ssv, x, row_sumsq, rs_slices, 32);
#pragma unroll
    for (int u = 0; u < G1_UNROLL; ++u) cur[u] = __builtin_nontemporal_load(wu + (size_t)u * rs);      // first weight group right behind
#pragma unroll
    for (int i = 0; i < NPT; ++i) x_store(i, val[i]);
    SJD_TR(1);
    __syncthreads();
    SJD_TR(2);
    // the activation of phase 1 is requested NOW and travels under the whole of phase 0 (first version: requested one weight group ahead
    // of the restaging barrier, which then took ~4 us with one weight group per wave in flight)
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(1, i);
    g1s_row_scale<32>(rsc, ssv, row_sumsq, rs_slices, rs_inv_hidden, rs_eps);
    __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): nothing pending when the loop is entered (see g1_skinny_gemm)
    SJD_TR(3);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const u32x4 *xa = xl + (size_t)kh * SP * 64;
    auto mfma_group = [&](int g) {
#pragma unroll
        for (int u = 0; u < G1_UNROLL; ++u)
            acc = G1Mfma<DT>::mma(xa[(g * G1_UNROLL + u) * 64 + g1_slot(lane >> 5, lane & 31, u)], cur[u], acc);
    };
    auto load_group = [&](int gi) {               // group gi of the K half (0 .. 2 GP - 1)
#pragma unroll
        for (int u = 0; u < G1_UNROLL; ++u) nxt[u] = __builtin_nontemporal_load(wu + (size_t)(gi * G1_UNROLL + u) * rs);
    };
    auto adopt = [&]() {
#pragma unroll
        for (int u = 0; u < G1_UNROLL; ++u) cur[u] = nxt[u];
    };
    // ---- phase 0, all but its last group
    for (int g = 0; g + 1 < GP; ++g) {
        load_group(g + 1);
        mfma_group(g);
        adopt();
    }
    // ---- last group of phase 0: the first weight group of phase 1 is requested before its MFMAs and stays in flight through the
    // restaging; then every wave is done with the staged columns and they are replaced (the new ones have been in registers for long)
    load_group(GP);
    mfma_group(GP - 1);
    adopt();
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPT; ++i) x_store(i, val[i]);
    __syncthreads();
    SJD_TR(4);                    // (trace: restaged)
    // ---- phase 1
    for (int g = 0; g < GP; ++g) {
        const bool more = g + 1 < GP;
        if (more) load_group(GP + g + 1);
        mfma_group(g);
        if (more) adopt();
    }
    SJD_TR(5);                    // main loop done
    // ---- epilogue: the eight planes (tile q x K half) go through LDS (row-major, rows padded to 36 floats: conflict-free both ways), then
    // every thread finishes FOUR outputs: one (activation tile, row, four columns) each -- first version: the two gate waves of K half 0 did
    // all sixteen IEEE divisions per lane and 2-byte stores, 3.6 us.
    __syncthreads();                                              // the activation arena is free
    float *red = reinterpret_cast<float *>(smem);                 // [8 planes][32 rows][G1S_RP]
    g1s_plane_store<1>(red, kh * 4 + q, &acc);
    __syncthreads();
    g1s_finish<DT, 1, 2>(red, rsc, y, M, I);
    SJD_TR(6);
}

// ---- G1s for a 64-row window (round 3): MT = 2 row tiles per weight record, staging phases and (optionally) a double-buffered arena.  The
// 32-row kernel above is left exactly as it was (the generalised form costs it 1.5 us per launch: clamped unconditional loads, one more
// barrier shape); same arithmetic in the same order: bit-identical to G1 + F3 like the 32-row kernel.
template <int DT, int SP, int MT, bool DB>
__global__ __launch_bounds__(512) void g1_gateup_silu_tall(const unsigned short *__restrict__ x, const u32x4 *__restrict__ wp,
                                                      unsigned short *__restrict__ y, int M, int I, int K, int rec_stride,
                                                      const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden, float rs_eps)
{
    // SP = k-steps of a staging phase per K half; (K / 32) / SP phases.  MT = 2 (round 3): a 64-row window (draft window 32 with CFG -- Emu3 --
    // or two prompts per forward); every weight record feeds two MFMAs.
    // DB = false: ONE arena of 2 MT phases (K = 4096: 128 KB), restaged between phases behind a stop-the-world barrier pair (the next
    //   phase's columns have been in registers since the previous barrier).
    // DB = true: the arena is two buffers of half-length phases; phase p + 1 is written into the other buffer while phase p is multiplied
    //   and ONE barrier per phase publishes it.  Measured per shape (profiles/r3_g1s_64rows.txt): the extra barriers cost a 32-row window
    //   more than the restaging stall (gate|up 33.3 -> 34.9 us, 12-bit stream 26.8 -> 28.2) and the 12-bit 64-row kernel too (two prompts
    //   3.66 -> 3.76 ms per step), but Emu3's fp16 64-row gate|up gains 6 us per layer (4.83 -> 4.63 ms per step): the launcher picks.
    SJD_TR(0);
    SJD_TR_HW();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);                  // [2 buffers][MT row tiles][2 K halves][SP records][64 slots] of 16 B
    constexpr int R = 32 * MT;
    __shared__ float rsc[R];
    constexpr int GP = SP / 8;                                    // weight groups per phase
    constexpr int PPS = 2 * SP;                                   // 16-byte pieces per (row, K half) of a phase
    constexpr int NPT = (R * 2 * PPS) / 512;                      // pieces per thread and phase
    constexpr int BUF = MT * 2 * SP * 64;                         // u32x4 per buffer
    static_assert(SP % 8 == 0 && NPT >= 1, "phase = whole weight groups, at least one piece per thread");
    auto bufof = [](int ph) { return DB ? (ph & 1) : 0; };
    const int nph = (K / 32) / SP;                                // phases
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int kh = w >> 2, q = w & 3;                             // K half; 0, 1 = gate tiles, 2, 3 = the up tiles of the same columns
    const int n_gate = I / 32, n_tiles = 2 * n_gate;
    const int t_act = 2 * blockIdx.x + (q & 1);                   // 32-column tile of the activation
    const int t = (q < 2 ? 0 : n_gate) + t_act;                   // tile of the packed gate|up weight
    const int steps = K / 32;                                     // k-steps of a K half (= of a chunk of the packed weight)
    const size_t chunk_base = (size_t)kh * n_tiles * steps;
    const size_t tile_off = (rec_stride == 1) ? (size_t)t * steps : (size_t)t;
    const u32x4 *wu = wp + (chunk_base + tile_off) * 64 + lane;
    const size_t rs = (size_t)rec_stride * 64;
    // piece v of a phase: row m = v / (2 PPS), K half hh = (v / PPS) & 1, piece j of that (row, half): 8 columns from
    // hh * K/2 + ph * 16 SP + 8 j -> record ((m / 32) * 2 + hh) * SP + j / 2, slot g1_slot(j & 1, m % 32, j / 2)
    auto x_load = [&](int ph, int i) -> u32x4 {
        const int v = i * 512 + threadIdx.x;
        const int m = v / (2 * PPS), hh = (v / PPS) & 1, j = v % PPS;
        // (unconditional: a phase past the last one re-reads the last, a row past M reads row M - 1 -- zeroed / unused)
        const u32x4 val = *reinterpret_cast<const u32x4 *>(x + (size_t)min(m, M - 1) * K + hh * (K / 2) + min(ph, nph - 1) * (16 * SP) + 8 * j);
        return (m < M) ? val : u32x4{0u, 0u, 0u, 0u};
    };
    auto x_store = [&](int buf, int i, u32x4 val) {
        const int v = i * 512 + threadIdx.x;
        const int m = v / (2 * PPS), hh = (v / PPS) & 1, j = v % PPS;
        xl[buf * BUF + (((m >> 5) * 2 + hh) * SP + (j >> 1)) * 64 + g1_slot(j & 1, m & 31, j >> 1)] = val;
    };
    u32x4 cur[G1_UNROLL], nxt[G1_UNROLL], val[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(0, i);
    // the per-slice sums of h^2 behind the row scale r = rsqrt(mean(h^2) + eps) of the folded RMSNorm (F1r wrote them; K <= 4096: at most
    // eight slices).  Every thread issues the eight loads -- unconditional, so the waits around them stay exact -- BEHIND the activation
    // and ahead of the weights: they are cache hits and cost the staging nothing (first version: threads 0..31 did this first, +0.7 us).
    float ssv[8];
    g1s_row_sumsq_load<R>(ssv, x, row_sumsq, rs_slices, ((M + 31) / 32) * 32);      // F1r's slices are [rows padded to 32]: 96 for a 65..96-row window on the four-tile kernel
#pragma unroll
    for (int u = 0; u < G1_UNROLL; ++u) cur[u] = __builtin_nontemporal_load(wu + (size_t)u * rs);      // first weight group right behind
#pragma unroll
    for (int i = 0; i < NPT; ++i) x_store(0, i, val[i]);
    SJD_TR(1);
    __syncthreads();
    SJD_TR(2);
    // the activation of the next phase is requested NOW and travels under the whole of this one
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(1, i);
    g1s_row_scale<R>(rsc, ssv, row_sumsq, rs_slices, rs_inv_hidden, rs_eps);
    SJD_TR(3);
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;
    auto mfma_group = [&](const u32x4 *xb, int g) {
#pragma unroll
        for (int u = 0; u < G1_UNROLL; ++u)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                acc[mt] = G1Mfma<DT>::mma(xb[((mt * 2 + kh) * SP + g * G1_UNROLL + u) * 64 + g1_slot(lane >> 5, lane & 31, u)], cur[u], acc[mt]);
    };
    const int last_group = nph * GP - 1;
    for (int ph = 0; ph < nph; ++ph) {
        const u32x4 *xb = xl + bufof(ph) * BUF;
        for (int g = 0; g < GP; ++g) {
            const int gi = ph * GP + g;                            // group of the K half; the next one is requested before this one's MFMAs
#pragma unroll
            for (int u = 0; u < G1_UNROLL; ++u) nxt[u] = __builtin_nontemporal_load(wu + (size_t)(min(gi + 1, last_group) * G1_UNROLL + u) * rs);
            __builtin_amdgcn_sched_barrier(0);           // (the machine scheduler otherwise sinks the loads behind the MFMAs: requested a group late)
            mfma_group(xb, g);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < G1_UNROLL; ++u) cur[u] = nxt[u];
        }
        // phase ph + 1 (in registers since the previous barrier) goes into the other buffer -- nobody reads that one any more: the barrier that
        // published THIS phase came after everybody's last read of it -- and phase ph + 2 is requested
        if (ph + 1 < nph) {
            if (!DB) __syncthreads();      // (one arena: every wave is done with the staged columns before they are replaced)
#pragma unroll
            for (int i = 0; i < NPT; ++i) x_store(bufof(ph + 1), i, val[i]);
#pragma unroll
            for (int i = 0; i < NPT; ++i) val[i] = x_load(ph + 2, i);
        }
        __syncthreads();
        if (ph == 0) SJD_TR(4);           // (trace: first phase done, second published)
    }
    SJD_TR(5);                    // main loop done
    // ---- epilogue: the eight planes (tile q x K half) go through LDS (row-major, rows padded to 36 floats: conflict-free both ways), then
    // every thread finishes FOUR outputs per row tile: one (activation tile, row, four columns) each -- first version: the two gate waves
    // of K half 0 did all sixteen IEEE divisions per lane and 2-byte stores, 3.6 us.  (the last barrier of the loop freed the arena)
    float *red = reinterpret_cast<float *>(smem);                 // [8 planes][R rows][G1S_RP]
    g1s_plane_store<MT>(red, kh * 4 + q, acc);
    __syncthreads();
    g1s_finish<DT, MT, 2>(red, rsc, y, M, I);
    SJD_TR(6);
}

// G1s over the 12-bit weight stream (see G1z below): the same kernel, every record decoded (and its unit's exceptions patched in) in
// front of its MFMA, the records travelling through a RING of G1Z_DEPTH registers sets that is refilled as it is consumed.
// Bit-identical to g1_gateup_silu on the uncompressed packing of the same weight.  bf16.
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
#ifndef G1Z_DEPTH
#define G1Z_DEPTH 8           // k-steps a wave keeps in flight (a ring of G1Z_DEPTH / 2 record pairs); 4 / 8 / 16 / 32 measured: 8 (profiles/r3_g1z_microbench.txt)
#endif
// Experiment (off): a barrier between a workgroup's activation loads and its first weight loads, so that no activation request queues
// behind another wave's HBM round trips in the CU's in-order vector memory pipe.  Measured equal or slightly slower at ring depth 8 and 16
// (profiles/r3_g1z_microbench.txt): the 1.8 us until the activation is staged is the cold round trip itself.
#ifndef G1Z_XFIRST
#define G1Z_XFIRST 0
#endif
#if G1Z_XFIRST
#define G1Z_XFIRST_BARRIER() __builtin_amdgcn_s_barrier()
#else
#define G1Z_XFIRST_BARRIER() do { } while (0)
#endif
#ifndef G1Z_AUX
#define G1Z_AUX 2             // cache policy of the weight loads: nt (streamed once)
#endif
struct g1z_hdr { unsigned base4, v_step, v_pos, v_val, v_step2, v_pos2, v_val2; bool wide; };    // (second entry per lane: headers of 128)
struct g1z_hraw { u32x2 a, b; };
struct g1z_pair { u32x4 lo; u32x2 c; };          // two k-steps: {low bytes 0..3, 4..7} x 2, {codes} x 2
template <bool WIDE> __device__ __forceinline__ u32x4 g1z_operand(unsigned lo0, unsigned lo1, unsigned c, unsigned s, const g1z_hdr &hd, int lane);
template <bool WIDE> __device__ __forceinline__ g1z_hdr g1z_header(g1z_hraw e, int lane, int cap);
// the header of unit `unit`: cap = 32 / 64 / 128 entries of 8 bytes; lane l takes entry min(l, cap - 1) and, in a header of 128, entry 64 + l
// (WIDE = a header of 128: a template parameter -- the second register set and its compare per k-step cost the common case 0.4 us per launch
// when they were a run-time switch)
template <bool WIDE>
__device__ __forceinline__ g1z_hraw g1z_header_load(const u32x2 *__restrict__ exc, size_t unit, int lane, int cap)
{
    g1z_hraw h;
    const u32x2 *e = exc + unit * (size_t)cap;
    h.a = e[min(lane, cap - 1)];
    if constexpr (WIDE) h.b = e[64 + lane]; else h.b = h.a;
    return h;
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t g1z_unit_rsrc(const unsigned char *first_record, unsigned bytes);
// ---- RAW units (round 6): a unit whose weights do not fit the format (more than 127 outside any sixteen-binade window: zero rows, pruned blocks)
// is zero-filled in the stream; its header says {base 0, count -1}, entry 1 holds the byte offset -- from `exc` -- of its weights as plain 1-KiB
// records (sjd_skinny_gemm's order), which sjd_amd.ops.pack_weight_z appends to the header array.  The wave that owns such a unit runs the
// PLAIN loop over those records (eight in flight, no decode) instead of the 12-bit one: one wave-uniform branch per kernel, the same MFMA
// sequence, and a matrix without raw units never leaves the old path.  (A fix-up launch behind the kernel was built first, csrc/sjd_gemm_raw.h:
// +5-7 us per projection with 1 % raw units -- a unit's MFMA chain is serial -- it now serves only the kernels without this path: the
// dispatchers sjd_skinny_gemm_z and g1sz_launch launch it behind them.)
__device__ __forceinline__ bool g1z_unit_is_raw(const g1z_hraw &h) { return __builtin_amdgcn_readfirstlane((int)h.a.y) < 0; }
__device__ __forceinline__ const u32x4 *g1z_raw_records(const u32x2 *__restrict__ exc, const g1z_hraw &h, int lane)
{
    const unsigned off = (unsigned)__builtin_amdgcn_readlane((int)h.a.x, 1);
    return reinterpret_cast<const u32x4 *>(reinterpret_cast<const unsigned char *>(exc) + off) + lane;
}
__device__ __forceinline__ g1z_pair g1z_load(__amdgpu_buffer_rsrc_t wr, unsigned lane, unsigned soff)
{
    g1z_pair v;          // (a pair past the unit's end reads as zero without touching memory; nt: streamed once)
    v.lo = __builtin_amdgcn_raw_buffer_load_b128(wr, lane * 16u, soff, G1Z_AUX);
    v.c = __builtin_amdgcn_raw_buffer_load_b64(wr, 1024u + lane * 8u, soff, G1Z_AUX);
    return v;
}

#include "sjd_gemm_wide.h"          // (kernel G1w: behind the declarations of the 12-bit decode it shares with G1z)
#include "sjd_gemm_q8.h"            // (kernels G1q / G1sq: the 8-bit e4m3 stream, SJD_G1_W8_E4M3)
#include "sjd_gemm_qblock.h"        // (the kernel templates of the two block-scaled streams below)
#include "sjd_gemm_q4.h"            // (kernels G1q4 / G1sq4: the MXFP4 stream, SJD_G1_W4_MXFP4)
#include "sjd_gemm_q6.h"            // (kernels G1q6 / G1sq6: the 6-bit e2m3 stream, SJD_G1_W6_E2M3)

// more than one weight-stream bit in a call's dtype
static inline bool g1_two_streams(int dtype)
{
    const int b = dtype & (SJD_G1_W8_E4M3 | SJD_G1_W4_MXFP4 | SJD_G1_W6_E2M3);
    return (b & (b - 1)) != 0;
}
#include "sjd_gemm_prefill.h"       // (kernel G1p: the prefill projection over the same packed copies, any row count)

// (keeps its own copy of the gate|up tail: with the helpers of sjd_gemm_parts.h the headline decode, whose MLP runs this kernel, missed its timing rule -- DESIGN.md 4.2f)
template <int SP, bool WIDE>
__global__ __launch_bounds__(512) void g1z_gateup_silu(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wz,
                                                       const u32x2 *__restrict__ exc, unsigned short *__restrict__ y, int M, int I, int K,
                                                       int stride_cap, const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden,
                                                       float rs_eps)
{
    const int rec_stride = stride_cap & 0xffff, exc_cap = stride_cap >> 16;      // (one dword: see g1z_skinny_gemm)
    constexpr int DT = SJD_DTYPE_BF16;
    constexpr int D = SP >= G1Z_DEPTH ? G1Z_DEPTH : 8;           // k-steps in flight per wave, as a ring of D / 2 record pairs
    constexpr int DP = D / 2;
    constexpr int TL = D < 8 ? 8 : D;                             // k-steps of a loop trip (unrolled; the ring goes round TL / D times)
    static_assert(SP % TL == 0 && TL % 8 == 0 && TL % D == 0 && D % 2 == 0, "a phase is whole trips; g1_slot(.., s) depends on s & 7");
    SJD_TR(0);
    SJD_TR_HW();
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
    const size_t chunk_base = (size_t)kh * n_tiles * pairs;
    const size_t tile_off = (rec_stride == 1) ? (size_t)t * pairs : (size_t)t;
    const unsigned rsb = (unsigned)rec_stride * 1536u;           // bytes from a pair of the unit to the next
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(wz + (chunk_base + tile_off) * 1536, (unsigned)(pairs - 1) * rsb + 1536u);
    auto w_load = [&](int p) -> g1z_pair { return g1z_load(wr, (unsigned)lane, (unsigned)p * rsb); };
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
    g1z_pair ring[DP];
    u32x4 val[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(0, i);
    float ssv[8];
    {
        const float *ssp = row_sumsq ? row_sumsq : reinterpret_cast<const float *>(x);
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) ssv[qq] = ssp[(size_t)(row_sumsq ? min(qq, rs_slices - 1) : 0) * 32 + (threadIdx.x & 31)];
    }
    G1Z_XFIRST_BARRIER();
    const g1z_hraw hraw = g1z_header_load<WIDE>(exc, (size_t)kh * n_tiles + t, lane, exc_cap);
#pragma unroll
    for (int u = 0; u < DP; ++u) ring[u] = w_load(u);
#pragma unroll
    for (int i = 0; i < NPT; ++i) x_store(i, val[i]);
    SJD_TR(1);
    __syncthreads();
    SJD_TR(2);
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(1, i);
    if (threadIdx.x < 32) {
        float tsum = 0.f;
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) tsum += (qq < rs_slices) ? ssv[qq] : 0.f;
        rsc[threadIdx.x] = row_sumsq ? rsqrtf(__builtin_fmaf(tsum, rs_inv_hidden, rs_eps)) : 1.0f;
    }
    SJD_TR(3);
    const g1z_hdr hd = g1z_header<WIDE>(hraw, lane, exc_cap);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const u32x4 *xa = xl + (size_t)kh * SP * 64;
    // one ring trip: k-steps s0 .. s0 + D - 1 of the K half, staged as LDS records l0 .. of the current phase; every consumed pair is
    // refilled with the one D k-steps further on (unconditional: exact s_waitcnt counts, D k-steps in flight through MFMAs and barriers alike)
    auto trip = [&](int l0, int s0) {
        u32x4 a[2];
        a[0] = xa[l0 * 64 + g1_slot(lane >> 5, lane & 31, 0)];
#pragma unroll
        for (int u = 0; u < TL / 2; ++u) {
            g1z_pair &slot = ring[u % DP];
            a[1] = xa[(l0 + 2 * u + 1) * 64 + g1_slot(lane >> 5, lane & 31, 2 * u + 1)];
            const u32x4 b0 = g1z_operand<WIDE>(slot.lo.x, slot.lo.y, slot.c.x, (unsigned)(s0 + 2 * u), hd, lane);
            acc = G1Mfma<DT>::mma(a[0], b0, acc);
            if (u + 1 < TL / 2) a[0] = xa[(l0 + 2 * u + 2) * 64 + g1_slot(lane >> 5, lane & 31, 2 * u + 2)];
            const u32x4 b1 = g1z_operand<WIDE>(slot.lo.z, slot.lo.w, slot.c.y, (unsigned)(s0 + 2 * u + 1), hd, lane);
            slot = w_load(s0 / 2 + u + DP);
            acc = G1Mfma<DT>::mma(a[1], b1, acc);
        }
    };
    // a unit that travels verbatim (see g1z_raw_records): the plain trip over its 1-KiB records, eight in flight
    const bool z_raw = g1z_unit_is_raw(hraw);
    const u32x4 *rr = z_raw ? g1z_raw_records(exc, hraw, lane) : reinterpret_cast<const u32x4 *>(x);
    u32x4 rc[8];
    if (z_raw) {
#pragma unroll
        for (int u = 0; u < 8; ++u) rc[u] = __builtin_nontemporal_load(rr + (size_t)u * 64);
    }
    auto trip_raw = [&](int l0, int s0) {
#pragma unroll
        for (int u = 0; u < TL; ++u) {
            const u32x4 ar = xa[(l0 + u) * 64 + g1_slot(lane >> 5, lane & 31, u)];
            acc = G1Mfma<DT>::mma(ar, rc[u & 7], acc);
            rc[u & 7] = __builtin_nontemporal_load(rr + (size_t)min(s0 + u + 8, 2 * SP - 1) * 64);
        }
    };
    // (ONE branch around both phases, not one per trip: the 12-bit ring and the raw ring are then never live together)
    if (z_raw) {
        for (int g = 0; g < SP / TL; ++g) trip_raw(g * TL, g * TL);               // ---- phase 0
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NPT; ++i) x_store(i, val[i]);
        __syncthreads();
        for (int g = 0; g < SP / TL; ++g) trip_raw(g * TL, SP + g * TL);          // ---- phase 1
    } else {
        for (int g = 0; g < SP / TL; ++g) trip(g * TL, g * TL);                   // ---- phase 0
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NPT; ++i) x_store(i, val[i]);
        __syncthreads();
        SJD_TR(4);
        for (int g = 0; g < SP / TL; ++g) trip(g * TL, SP + g * TL);              // ---- phase 1
    }
    SJD_TR(5);
    __syncthreads();
    constexpr int RP = G1S_RP;
    float *red = reinterpret_cast<float *>(smem);
    {
        float *mine = red + (size_t)(kh * 4 + q) * 32 * RP + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) mine[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * RP] = acc[r];
    }
    __syncthreads();
    {
        const int a = threadIdx.x >> 8, m = (threadIdx.x >> 3) & 31, c4 = (threadIdx.x & 7) * 4;
        auto plane = [&](int kh_, int q_) { return *reinterpret_cast<const float4 *>(red + ((size_t)(kh_ * 4 + q_) * 32 + m) * RP + c4); };
        const float4 g0 = plane(0, a), g1 = plane(1, a), u0 = plane(0, 2 + a), u1 = plane(1, 2 + a);
        const float gs[4] = {g0.x, g0.y, g0.z, g0.w}, gt[4] = {g1.x, g1.y, g1.z, g1.w};
        const float us_[4] = {u0.x, u0.y, u0.z, u0.w}, ut[4] = {u1.x, u1.y, u1.z, u1.w};
        const float rr = rsc[m];
        unsigned short o16[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gsum = 0.f, usum = 0.f;
            gsum += gs[j]; gsum += gt[j];
            usum += us_[j]; usum += ut[j];
            o16[j] = sjd_silu_mul_elem<DT>(gsum, usum, rr);
        }
        if (m < M) {
            uint2 pk{(unsigned)o16[0] | ((unsigned)o16[1] << 16), (unsigned)o16[2] | ((unsigned)o16[3] << 16)};
            *reinterpret_cast<uint2 *>(y + (size_t)m * I + 32 * (2 * blockIdx.x + a) + c4) = pk;
        }
    }
    SJD_TR(6);
}

// Does the G1sz instantiation (SP k-steps per phase, MT row tiles) multiply raw units in the kernel?  SP = 32 with two row tiles -- hidden 4096 at
// 64 rows -- sits at its 256 registers: there g1sz_launch runs the fix-up launch behind the kernel (csrc/sjd_gemm_raw.h).  The kernel body and the
// launcher both read this.
constexpr bool g1sz_raw_inline(int SP, int MT) { return !(SP == 32 && MT == 2); }

// ---- G1sz for a 64-row window (see g1_gateup_silu_tall)
template <int SP, int MT, bool DB, bool WIDE>
__global__ __launch_bounds__(512) void g1z_gateup_silu_tall(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wz,
                                                       const u32x2 *__restrict__ exc, unsigned short *__restrict__ y, int M, int I, int K,
                                                       int stride_cap, const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden,
                                                       float rs_eps)
{
    const int rec_stride = stride_cap & 0xffff, exc_cap = stride_cap >> 16;      // (one dword: see g1z_skinny_gemm)
    constexpr int DT = SJD_DTYPE_BF16;
    constexpr int D = SP >= G1Z_DEPTH ? G1Z_DEPTH : 8;           // k-steps in flight per wave, as a ring of D / 2 record pairs
    constexpr int DP = D / 2;
    constexpr int TL = D < 8 ? 8 : D;                             // k-steps of a loop trip (unrolled; the ring goes round TL / D times)
    static_assert(SP % TL == 0 && TL % 8 == 0 && TL % D == 0 && D % 2 == 0, "a phase is whole trips; g1_slot(.., s) depends on s & 7");
    SJD_TR(0);
    SJD_TR_HW();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);                  // two buffers of [MT][2 K halves][SP records][64 slots] (see g1_gateup_silu)
    constexpr int R = 32 * MT;
    __shared__ float rsc[R];
    constexpr int PPS = 2 * SP;
    constexpr int NPT = (R * 2 * PPS) / 512;
    constexpr int BUF = MT * 2 * SP * 64;
    static_assert(NPT >= 1, "at least one piece per thread");
    auto bufof = [](int ph) { return DB ? (ph & 1) : 0; };
    const int nph = (K / 32) / SP;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int kh = w >> 2, q = w & 3;
    const int n_gate = I / 32, n_tiles = 2 * n_gate;
    const int t_act = 2 * blockIdx.x + (q & 1);
    const int t = (q < 2 ? 0 : n_gate) + t_act;
    const int pairs = K / 64;                                     // record pairs of a K half (K / 32 k-steps)
    const size_t chunk_base = (size_t)kh * n_tiles * pairs;
    const size_t tile_off = (rec_stride == 1) ? (size_t)t * pairs : (size_t)t;
    const unsigned rsb = (unsigned)rec_stride * 1536u;           // bytes from a pair of the unit to the next
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(wz + (chunk_base + tile_off) * 1536, (unsigned)(pairs - 1) * rsb + 1536u);
    auto w_load = [&](int p) -> g1z_pair { return g1z_load(wr, (unsigned)lane, (unsigned)p * rsb); };
    auto x_load = [&](int ph, int i) -> u32x4 {
        const int v = i * 512 + threadIdx.x;
        const int m = v / (2 * PPS), hh = (v / PPS) & 1, j = v % PPS;
        const u32x4 val = *reinterpret_cast<const u32x4 *>(x + (size_t)min(m, M - 1) * K + hh * (K / 2) + min(ph, nph - 1) * (16 * SP) + 8 * j);
        return (m < M) ? val : u32x4{0u, 0u, 0u, 0u};
    };
    auto x_store = [&](int buf, int i, u32x4 val) {
        const int v = i * 512 + threadIdx.x;
        const int m = v / (2 * PPS), hh = (v / PPS) & 1, j = v % PPS;
        xl[buf * BUF + (((m >> 5) * 2 + hh) * SP + (j >> 1)) * 64 + g1_slot(j & 1, m & 31, j >> 1)] = val;
    };
    g1z_pair ring[DP];
    u32x4 val[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(0, i);
    float ssv[8];
    g1s_row_sumsq_load<R>(ssv, x, row_sumsq, rs_slices, R);
    G1Z_XFIRST_BARRIER();
    const g1z_hraw hraw = g1z_header_load<WIDE>(exc, (size_t)kh * n_tiles + t, lane, exc_cap);
#pragma unroll
    for (int u = 0; u < DP; ++u) ring[u] = w_load(u);
#pragma unroll
    for (int i = 0; i < NPT; ++i) x_store(0, i, val[i]);
    SJD_TR(1);
    __syncthreads();
    SJD_TR(2);
#pragma unroll
    for (int i = 0; i < NPT; ++i) val[i] = x_load(1, i);
    g1s_row_scale<R>(rsc, ssv, row_sumsq, rs_slices, rs_inv_hidden, rs_eps);
    SJD_TR(3);
    const g1z_hdr hd = g1z_header<WIDE>(hraw, lane, exc_cap);
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;
    // one ring trip: k-steps s0 .. s0 + TL - 1 of the K half, staged as LDS records l0 .. of the current phase's buffer; every consumed pair is
    // refilled with the one D k-steps further on (unconditional: exact s_waitcnt counts, D k-steps in flight through MFMAs and barriers alike)
    auto trip = [&](const u32x4 *xb, int l0, int s0) {
        auto a_read = [&](u32x4 (&a)[MT], int l, int u) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[mt] = xb[((mt * 2 + kh) * SP + l) * 64 + g1_slot(lane >> 5, lane & 31, u)];
        };
        u32x4 a0[MT], a1[MT];
        a_read(a0, l0, 0);
#pragma unroll
        for (int u = 0; u < TL / 2; ++u) {
            g1z_pair &slot = ring[u % DP];
            a_read(a1, l0 + 2 * u + 1, 2 * u + 1);
            const u32x4 b0 = g1z_operand<WIDE>(slot.lo.x, slot.lo.y, slot.c.x, (unsigned)(s0 + 2 * u), hd, lane);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a0[mt], b0, acc[mt]);
            if (u + 1 < TL / 2) a_read(a0, l0 + 2 * u + 2, 2 * u + 2);
            const u32x4 b1 = g1z_operand<WIDE>(slot.lo.z, slot.lo.w, slot.c.y, (unsigned)(s0 + 2 * u + 1), hd, lane);
            slot = w_load(s0 / 2 + u + DP);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a1[mt], b1, acc[mt]);
        }
    };
    // a unit that travels verbatim (see g1z_raw_records): the plain trip over its 1-KiB records, eight in flight
    constexpr bool RAW_HERE = g1sz_raw_inline(SP, MT);
    const bool z_raw = RAW_HERE && g1z_unit_is_raw(hraw);
    const u32x4 *rr = z_raw ? g1z_raw_records(exc, hraw, lane) : reinterpret_cast<const u32x4 *>(x);
    constexpr int RD = 4;                     // records in flight
    u32x4 rc[RD];
    if (z_raw) {
#pragma unroll
        for (int u = 0; u < RD; ++u) rc[u] = __builtin_nontemporal_load(rr + (size_t)u * 64);
    }
    auto trip_raw = [&](const u32x4 *xb, int l0, int s0) {
#pragma unroll
        for (int u = 0; u < TL; ++u) {
            u32x4 ar[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) ar[mt] = xb[((mt * 2 + kh) * SP + l0 + u) * 64 + g1_slot(lane >> 5, lane & 31, u)];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(ar[mt], rc[u % RD], acc[mt]);
            rc[u % RD] = __builtin_nontemporal_load(rr + (size_t)min(s0 + u + RD, K / 32 - 1) * 64);
        }
    };
    // (ONE branch around the phase loop, not one per trip: the 12-bit ring and the raw ring are then never live together)
#define SJD_G1SZ_PHASES(TRIP_)                                                                                                              \
    for (int ph = 0; ph < nph; ++ph) {                                                                                                      \
        const u32x4 *xb = xl + bufof(ph) * BUF;                                                                                             \
        for (int g = 0; g < SP / TL; ++g) TRIP_(xb, g * TL, ph * SP + g * TL);                                                              \
        if (ph + 1 < nph) {    /* the next phase replaces this one (DB: the other buffer), the one after it is requested (g1_gateup_silu) */ \
            if (!DB) __syncthreads();                                                                                                       \
            _Pragma("unroll") for (int i = 0; i < NPT; ++i) x_store(bufof(ph + 1), i, val[i]);                                               \
            _Pragma("unroll") for (int i = 0; i < NPT; ++i) val[i] = x_load(ph + 2, i);                                                      \
        }                                                                                                                                   \
        __syncthreads();                                                                                                                    \
        if (ph == 0) SJD_TR(4);                                                                                                             \
    }
    if constexpr (RAW_HERE) { if (z_raw) { SJD_G1SZ_PHASES(trip_raw) } else { SJD_G1SZ_PHASES(trip) } } else { SJD_G1SZ_PHASES(trip) }
#undef SJD_G1SZ_PHASES
    SJD_TR(5);
    float *red = reinterpret_cast<float *>(smem);
    g1s_plane_store<MT>(red, kh * 4 + q, acc);
    __syncthreads();
    g1s_finish<DT, MT, 2>(red, rsc, y, M, I);
    SJD_TR(6);
}

#include "sjd_gemm_raw.h"          // (the fix-up launch for raw units behind the stream kernels that have no in-kernel path for them)

static int g1sz_launch(const void *x, const void *wz, const void *exc, int exc_cap, void *y, int M, int I, int K, int step_major, const sjd_row_norm *rn,
                       const sjd_raw_units *raw, hipStream_t s)
{
    const int MT = M <= 32 ? 1 : 2;
    const int SP = K / (64 * MT);                                  // one arena, 2 MT phases (double-buffered half phases measured slower: g1_gateup_silu)
    const dim3 grid(I / 64), block(512);
    const size_t lds_x = (size_t)MT * 2 * SP * 1024, lds_red = g1s_epilogue_lds(MT);
    const size_t lds = lds_x > lds_red ? lds_x : lds_red;
    const int rec_stride = step_major ? 2 * (I / 32) : 1;
    const g1s_norm_args n(rn);
#define SJD_G1SZ_CASE(SP_, MT_) SJD_G1SZ_CASE_W(SP_, MT_, false) SJD_G1SZ_CASE_W(SP_, MT_, true)
#define SJD_G1SZ_CASE_W(SP_, MT_, W_) \
    if (SP == SP_ && MT == MT_ && (exc_cap > 64) == W_) { \
        const int rc = g1_launch_kernel(g1z_gateup_silu_tall<SP_, MT_, false, W_>, grid, block, lds, s, x, wz, exc, y, M, I, K, rec_stride | (exc_cap << 16), n.ss, n.sl, n.ih, n.eps); \
        return rc != SJD_OK || g1sz_raw_inline(SP_, MT_) ? rc : g1_raw_gateup_launch(x, raw, y, M, I, K, rn, s); \
    }
#define SJD_G1SZ_CASE32(SP_) SJD_G1SZ_CASE32_W(SP_, false) SJD_G1SZ_CASE32_W(SP_, true)
#define SJD_G1SZ_CASE32_W(SP_, W_) \
    if (SP == SP_ && MT == 1 && (exc_cap > 64) == W_) \
        return g1_launch_kernel(g1z_gateup_silu<SP_, W_>, grid, block, lds, s, x, wz, exc, y, M, I, K, rec_stride | (exc_cap << 16), n.ss, n.sl, n.ih, n.eps);
    SJD_G1SZ_CASE32(8) SJD_G1SZ_CASE32(16) SJD_G1SZ_CASE32(32) SJD_G1SZ_CASE32(64)
#undef SJD_G1SZ_CASE32
#undef SJD_G1SZ_CASE32_W
    SJD_G1SZ_CASE(8, 2) SJD_G1SZ_CASE(16, 2) SJD_G1SZ_CASE(32, 2)
#undef SJD_G1SZ_CASE
#undef SJD_G1SZ_CASE_W
    return SJD_ERR_UNSUPPORTED;
}

// sjd_gateup_silu over ops.pack_weight_z([Wg; Wu], K / 2, step_major): same result, bit for bit; bf16 only.
extern "C" int sjd_gateup_silu_z(const void *x, const void *wz, const void *exc, int exc_cap, void *y, int M, int I, int K, int step_major, int dtype,
                                 const sjd_row_norm *row_norm, const sjd_raw_units *raw, void *stream)
{
    if (!x || !wz || !exc || !y || M < 1 || I < 64 || K < 512 || !(exc_cap == 32 || exc_cap == 64 || exc_cap == 128)) return SJD_ERR_BAD_ARG;
    if (!g1_raw_desc_ok(raw)) return SJD_ERR_BAD_ARG;
    if (row_norm && (!row_norm->sumsq || row_norm->slices < 1 || row_norm->hidden < 1)) return SJD_ERR_BAD_ARG;
    if (row_norm && row_norm->slices > 8) return SJD_ERR_UNSUPPORTED;
    if (M > 64 || (I % 64) != 0 || !(K == 512 || K == 1024 || K == 2048 || K == 4096) || (M > 32 && K == 512) || dtype != SJD_DTYPE_BF16)
        return SJD_ERR_UNSUPPORTED;
    return g1sz_launch(x, wz, exc, exc_cap, y, M, I, K, step_major, row_norm, raw, (hipStream_t)stream);
}

template <int DT>
static int g1s_launch(const void *x, const void *w_packed, void *y, int M, int I, int K, int step_major, const sjd_row_norm *rn, hipStream_t s)
{
    const int MT = M <= 32 ? 1 : M <= 64 ? 2 : 4;                  // (65..128 rows -- three / four prompts per forward -- run as four row tiles, K = 4096)
    const bool db = MT >= 2 && K >= 2048;                          // double-buffered half-length phases: the fp16 / bf16 64-row kernel (see the kernel)
    const int SP = K / ((db ? 128 : 64) * MT);
    const dim3 grid(I / 64), block(512);
    const size_t lds_x = (size_t)(db ? 2 : 1) * MT * 2 * SP * 1024, lds_red = g1s_epilogue_lds(MT);
    const size_t lds = lds_x > lds_red ? lds_x : lds_red;        // the epilogue's planes reuse the activation arena
    const int rec_stride = step_major ? 2 * (I / 32) : 1;
    const g1s_norm_args n(rn);
#define SJD_G1S_CASE(SP_, MT_, DB_) \
    if (SP == SP_ && MT == MT_ && db == DB_) \
        return g1_launch_kernel(g1_gateup_silu_tall<DT, SP_, MT_, DB_>, grid, block, lds, s, x, w_packed, y, M, I, K, rec_stride, n.ss, n.sl, n.ih, n.eps);
#define SJD_G1S_CASE32(SP_) \
    if (SP == SP_ && MT == 1) return g1_launch_kernel(g1_gateup_silu<DT, SP_>, grid, block, lds, s, x, w_packed, y, M, I, K, rec_stride, n.ss, n.sl, n.ih, n.eps);
    SJD_G1S_CASE32(8) SJD_G1S_CASE32(16) SJD_G1S_CASE32(32) SJD_G1S_CASE32(64)
#undef SJD_G1S_CASE32
    SJD_G1S_CASE(8, 2, false) SJD_G1S_CASE(8, 2, true) SJD_G1S_CASE(16, 2, true) SJD_G1S_CASE(8, 4, true)
#undef SJD_G1S_CASE
    return SJD_ERR_UNSUPPORTED;
}

// y [M, I] = silu(r * (x Wg^T)) * (r * (x Wu^T)) with F3's rounding points; w_packed = pack_weight([Wg; Wu] ([2 I, K]), KC = K / 2, step_major).
// M <= 32 rows and K in {512, 1024, 2048, 4096}, or M <= 64 rows (the sums of squares then come with 64 rows per slice) and K in {1024, 2048, 4096};
// I % 64 == 0.  SJD_ERR_UNSUPPORTED otherwise: the caller keeps G1 + F3.
extern "C" int sjd_gateup_silu(const void *x, const void *w_packed, void *y, int M, int I, int K, int step_major, int dtype,
                               const sjd_row_norm *row_norm, void *stream)
{
    if (!x || !w_packed || !y || M < 1 || I < 64 || K < 512) return SJD_ERR_BAD_ARG;
    if (row_norm && (!row_norm->sumsq || row_norm->slices < 1 || row_norm->hidden < 1)) return SJD_ERR_BAD_ARG;
    if (row_norm && row_norm->slices > 8) return SJD_ERR_UNSUPPORTED;      // the kernel sums one batch of eight 512-column slices
    if (const int n_chunks = step_major >> SJD_G1S_CHUNKS_SHIFT; n_chunks != 0) {      // the copy sjd_skinny_gemm streams in more than two chunks: one form
        if (g1_two_streams(dtype)) return SJD_ERR_BAD_ARG;
        if (dtype != (SJD_DTYPE_BF16 | SJD_G1_W4_MXFP4) || n_chunks != 4 || K != 8192 || M > 32 || (I % 64) != 0) return SJD_ERR_UNSUPPORTED;
        return g1sq4k4_launch(x, w_packed, y, M, I, step_major & 1, row_norm, (hipStream_t)stream);      // w_packed = ops.pack_weight_q4([Wg; Wu], 2048, step_major)
    }
    if (M > 128 || (I % 64) != 0 || !(K == 512 || K == 1024 || K == 2048 || K == 4096) || (M > 32 && K == 512) || (M > 64 && K != 4096)) return SJD_ERR_UNSUPPORTED;
    if (g1_two_streams(dtype)) return SJD_ERR_BAD_ARG;          // one weight stream per call
    if (dtype & SJD_G1_W6_E2M3)                                            // w_packed = ops.pack_weight_q6([Wg; Wu], K / 2, step_major, gateup=True): G1sq6
        return dtype == (SJD_DTYPE_BF16 | SJD_G1_W6_E2M3) ? g1sq6_launch(x, w_packed, y, M, I, K, step_major, row_norm, (hipStream_t)stream) : SJD_ERR_UNSUPPORTED;
    if (dtype & SJD_G1_W4_MXFP4)                                           // w_packed = ops.pack_weight_q4([Wg; Wu], K / 2, step_major, gateup=True): G1sq4
        return dtype == (SJD_DTYPE_BF16 | SJD_G1_W4_MXFP4) ? g1sq4_launch(x, w_packed, y, M, I, K, step_major, row_norm, (hipStream_t)stream) : SJD_ERR_UNSUPPORTED;
    if (dtype & SJD_G1_W8_E4M3)                                            // w_packed = ops.pack_weight_q8([Wg; Wu], K / 2, step_major, gateup=True): G1sq
        return dtype == (SJD_DTYPE_BF16 | SJD_G1_W8_E4M3) ? g1sq_launch(x, w_packed, y, M, I, K, step_major, row_norm, (hipStream_t)stream) : SJD_ERR_UNSUPPORTED;
    if (dtype == SJD_DTYPE_BF16) return g1s_launch<SJD_DTYPE_BF16>(x, w_packed, y, M, I, K, step_major, row_norm, (hipStream_t)stream);
    if (dtype == SJD_DTYPE_F16) return g1s_launch<SJD_DTYPE_F16>(x, w_packed, y, M, I, K, step_major, row_norm, (hipStream_t)stream);
    return SJD_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------ G1z (12-bit lossless weight stream)
// The window forward is a stream of the layer weights (12.96 GB per SJD iteration at Lumina-7B) through a fabric that sustains ~6.7 TB/s
// whatever the launch shape: what is left is to stream FEWER BYTES.  The high byte of a bf16 weight (sign + the seven
// high exponent bits) takes very few values inside one (k-chunk, 32-column tile) unit: a trained or Gaussian-initialised matrix puts all
// but ~1e-4 of a unit's weights into 16 consecutive binades.  G1z streams every weight as its LOW BYTE (exponent lsb + mantissa, verbatim)
// plus a 4-BIT CODE of the high byte -- (sign, offset 0..7 from a per-unit base) -- i.e. 12 bits per weight, 768-byte records instead of
// 1-KiB ones; the few weights outside the unit's window ("exceptions") travel verbatim in a header per unit (256 bytes = 31 exceptions, or 512 /
// 1024 bytes = 63 / 127 where a matrix needs them: heavy-tailed weights, folded norm gains) and are patched into the operand registers
// before the MFMA.  The B operand a wave feeds its MFMA is BIT-IDENTICAL to the uncompressed kernel's, so are the
// accumulation order and the result (tests/test_gpu_glue.py::test_g1z_*): this is a lossless re-encoding of the weight stream, not a
// change of precision.  A matrix some unit of which has more than 127 exceptions is simply left uncompressed by the packer
// (ops.pack_weight_z returns None).  bf16 only: fp16's high byte (sign, 5 exponent bits, 2 mantissa bits) does not concentrate.
//   record PAIR (1536 B, k-steps 2p and 2p + 1 of a unit; an odd last k-step is padded with zeros) =
//       64 lanes x 16 B {low bytes of weights 0..3, 4..7 of k-step 2p; the same of k-step 2p + 1}, then
//       64 lanes x  8 B {codes of k-step 2p, of k-step 2p + 1: byte i = code(w_i) | code(w_{i+4}) << 4}
//     -- both parts naturally aligned 16- / 8-byte loads (12-byte lane records as ONE dwordx3 load measured slower: a lane's bytes
//     straddle cache lines, profiles/r3_g1z_microbench.txt)
//   header (cap x 8 B, cap = 32 / 64 / 128 per matrix) = {pos, val}: entry 0 = {base, count}; entry i >= 1 = {k-step << 9 | lane << 3 | element,
//       the weight's 16 bits}; unused entries 0xffffffff.  A lane keeps entry `lane` (and entry 64 + lane of a 128-entry header) in registers.
// Decoding is 12 VALU instructions per record and wave (the kernel is at ~6 % MFMA-busy, the VALU idle); exceptions cost a wave-uniform
// compare per k-step and two selects on the ~10 % of k-steps that have one.  A wave keeps a ring of G1Z_DEPTH k-steps (record pairs) in
// flight through ONE buffer descriptor over its unit and refills a slot right after consuming it (first version, two register groups of
// eight like G1: the decode sat on the critical path between two round trips -- o slower than G1).
// high bytes of a record's eight weights from its code word: hA = weights 0..3, hB = weights 4..7 (byte i = sign << 7 | base + offset)
__device__ __forceinline__ void g1z_high(unsigned c, unsigned base4, unsigned &hA, unsigned &hB)
{
    hA = (((c & 0x08080808u) << 4) | (c & 0x07070707u)) + base4;
    const unsigned c2 = c >> 4;
    hB = (((c2 & 0x08080808u) << 4) | (c2 & 0x07070707u)) + base4;
}

// The MFMA B operand of k-step s from its 12 bytes {low bytes 0..3, low bytes 4..7, codes}: decode the high bytes, patch the
// unit's exceptions of this k-step into them (an exception differs from its coded form only in the HIGH byte -- the low byte travels
// verbatim; wave-uniform control flow, two selects per exception), interleave.  v_step = pos >> 9 of this lane's entry.
template <bool WIDE>
__device__ __forceinline__ u32x4 g1z_operand(unsigned lo0, unsigned lo1, unsigned c, unsigned s, const g1z_hdr &hd, int lane)
{
    unsigned hA, hB;
    g1z_high(c, hd.base4, hA, hB);
    auto patch = [&](unsigned long long mk, unsigned v_pos, unsigned v_val) {
        while (mk) {
            const int i = __builtin_ctzll(mk);
            mk &= mk - 1;
            const unsigned pos = __builtin_amdgcn_readlane(v_pos, i), hi = (__builtin_amdgcn_readlane(v_val, i) >> 8) & 0xffu;
            const int tl = (int)((pos >> 3) & 63u);
            const unsigned sh = (pos & 3u) * 8u, keep = ~(0xffu << sh), put = hi << sh;
            const bool me = lane == tl, upper = (pos & 4u) != 0u;
            hA = (me && !upper) ? ((hA & keep) | put) : hA;
            hB = (me && upper) ? ((hB & keep) | put) : hB;
        }
    };
#ifndef G1Z_NO_PATCH          // (G1Z_NO_PATCH: timing experiments only -- the results are wrong wherever a unit has an exception)
    patch(__ballot(hd.v_step == s), hd.v_pos, hd.v_val);
    if constexpr (WIDE) patch(__ballot(hd.v_step2 == s), hd.v_pos2, hd.v_val2);
#endif
    u32x4 d;
    d.x = __builtin_amdgcn_perm(hA, lo0, 0x05010400u);       // {lo.b0, hA.b0, lo.b1, hA.b1}
    d.y = __builtin_amdgcn_perm(hA, lo0, 0x07030602u);
    d.z = __builtin_amdgcn_perm(hB, lo1, 0x05010400u);
    d.w = __builtin_amdgcn_perm(hB, lo1, 0x07030602u);
    return d;
}

// the header of unit (chunk, tile): every lane gets entry (lane & 31); returns base * 0x01010101 and leaves this lane's exception in
// (v_step, v_pos, v_val) -- lanes 0 (base / count) and 32..63 (duplicates) hold none
template <bool WIDE>
__device__ __forceinline__ g1z_hdr g1z_header(g1z_hraw e, int lane, int cap)
{
    g1z_hdr h;
    h.base4 = (unsigned)__builtin_amdgcn_readfirstlane((int)e.a.x) * 0x01010101u;
    const bool live = lane >= 1 && lane < min(cap, 64);          // (lane 0: base / count; lanes past a short header: duplicates)
    h.v_pos = e.a.x;
    h.v_val = e.a.y;
    h.v_step = live ? (e.a.x >> 9) : 0xffffffffu;
    h.wide = WIDE;
    h.v_pos2 = e.b.x;
    h.v_val2 = e.b.y;
    h.v_step2 = WIDE ? (e.b.x >> 9) : 0xffffffffu;                // (unused entries hold 0xffffffff: their k-step never matches)
    return h;
}

// buffer descriptor over the records of ONE unit (wave-uniform by construction: the pointer goes through readfirstlane so that the
// compiler can see it -- guide T20); loads past `bytes` return zero and move nothing
__device__ __forceinline__ __amdgpu_buffer_rsrc_t g1z_unit_rsrc(const unsigned char *first_record, unsigned bytes)
{
    const unsigned long long a = (unsigned long long)first_record;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), 0, (int)__builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
}

template <int MT, int MAXT, bool WIDE>
__global__ __launch_bounds__(MAXT) void g1z_skinny_gemm(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wz,
                                                        const u32x2 *__restrict__ exc, float *__restrict__ out, int M, int N, int K, int KC,
                                                        int n_tiles, int rec_stride, int tile0, int waves_cap)
{
    // (the header capacity rides in the high half of the wave count: a 17th argument dword would not be preloaded into SGPRs and the kernel
    // would open with a scalar load round trip for it -- +0.04 ms per step when it was an argument of its own)
    const int n_waves = waves_cap & 0xffff, exc_cap = waves_cap >> 16;
    constexpr int DT = SJD_DTYPE_BF16;
    constexpr int D = MAXT <= 512 ? G1Z_DEPTH : (G1Z_DEPTH < 8 ? G1Z_DEPTH : 8);      // k-steps in flight per wave, as a ring of D / 2 record pairs (128 VGPRs at 9..16 waves)
    constexpr int DP = D / 2;
    constexpr int TL = D < 8 ? 8 : D;                             // k-steps of a loop trip (unrolled; the ring goes round TL / D times)
    static_assert(D % 2 == 0 && TL % 8 == 0 && TL % D == 0, "g1_slot(.., s) depends on s & 7: a trip starts at a multiple of eight");
    SJD_TR(0);
    SJD_TR_HW();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);
    const int chunk = blockIdx.y;
    const int k0 = chunk * KC;
    const int steps = min(KC, K - k0) / 16;
    const int pairs = (steps + 1) / 2, pairs_full = (KC / 16 + 1) / 2;          // record pairs of this unit / of a full chunk's unit
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int t_out = blockIdx.x * n_waves + w;
    const int t = tile0 + t_out;
    const bool has_tile = t_out < N / 32;
    const size_t chunk_base = (size_t)chunk * n_tiles * pairs_full;
    const size_t tile_off = (rec_stride == 1) ? (size_t)(has_tile ? t : 0) * pairs : (size_t)(has_tile ? t : 0);
    const unsigned rsb = (unsigned)rec_stride * 1536u;
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(wz + (chunk_base + tile_off) * 1536, has_tile ? (unsigned)(pairs - 1) * rsb + 1536u : 0u);
    auto w_load = [&](int p) -> g1z_pair { return g1z_load(wr, (unsigned)lane, (unsigned)p * rsb); };
    g1z_pair ring[DP];
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
    g1z_hraw hraw;
    {   // first activation batch, the unit's header and the first D records right behind it (all unconditional, see g1_skinny_gemm)
        u32x4 val[STAGE];
        int m = pm, j = pj;
#pragma unroll
        for (int i = 0; i < STAGE; ++i) { val[i] = x_load(m, j); advance(m, j); }
        G1Z_XFIRST_BARRIER();
        hraw = g1z_header_load<WIDE>(exc, (size_t)chunk * n_tiles + (has_tile ? t : 0), lane, exc_cap);
#pragma unroll
        for (int u = 0; u < DP; ++u) ring[u] = w_load(u);
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
    SJD_TR(1);
    __syncthreads();
    SJD_TR(2);
    if (!has_tile) return;
    const g1z_hdr hd = g1z_header<WIDE>(hraw, lane, exc_cap);
    SJD_TR(3);
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;
    const int xs = steps * 64;
    // ring trips of D k-steps: every consumed pair is refilled with the one D k-steps further on, AFTER it was consumed (the refill lands in
    // the registers it frees: no copies at the back edge) and unconditionally (exact s_waitcnt counts; a pair past the unit's end costs an
    // instruction, no traffic), so D k-steps stay in flight per wave through the MFMAs.  The k-steps of the last trip that lie past the
    // chunk are skipped by uniform branches.
    auto a_read = [&](u32x4 (&a)[MT], int s, int u) {      // (read ahead of the patch branch; the address stays inside the staged chunk)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = xl[mt * xs + min(s, steps - 1) * 64 + g1_slot(lane >> 5, lane & 31, u)];
    };
    if (g1z_unit_is_raw(hraw)) {          // this wave's unit travels verbatim: the plain loop (see g1z_raw_records)
        const u32x4 *rr = g1z_raw_records(exc, hraw, lane);
        constexpr int RD = (MT == 2 && MAXT == 1024) ? 2 : 8;      // records in flight (the 128-register budget of 16-wave workgroups with two row tiles: 2)
        u32x4 rc[RD];
#pragma unroll
        for (int u = 0; u < RD; ++u) rc[u] = __builtin_nontemporal_load(rr + (size_t)min(u, steps - 1) * 64);
        for (int s0 = 0; s0 < steps; s0 += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int sr = s0 + u;
                if (sr < steps) {
                    u32x4 ar[MT];
                    a_read(ar, sr, u);
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(ar[mt], rc[u % RD], acc[mt]);
                }
                rc[u % RD] = __builtin_nontemporal_load(rr + (size_t)min(sr + RD, steps - 1) * 64);
            }
        }
    } else
    for (int s0 = 0; s0 < steps; s0 += TL) {
        u32x4 a0[MT], a1[MT];
        a_read(a0, s0, 0);
#pragma unroll
        for (int u = 0; u < TL / 2; ++u) {
            const int sa = s0 + 2 * u, sb = sa + 1;
            g1z_pair &slot = ring[u % DP];
            if (sa < steps) {
                a_read(a1, sb, 2 * u + 1);
                const u32x4 b0 = g1z_operand<WIDE>(slot.lo.x, slot.lo.y, slot.c.x, (unsigned)sa, hd, lane);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a0[mt], b0, acc[mt]);
            }
            u32x4 b1 = {0u, 0u, 0u, 0u};
            if (sb < steps) {
                if (u + 1 < TL / 2) a_read(a0, sb + 1, 2 * u + 2);
                b1 = g1z_operand<WIDE>(slot.lo.z, slot.lo.w, slot.c.y, (unsigned)sb, hd, lane);
            }
            slot = w_load(s0 / 2 + u + DP);
            if (sb < steps) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a1[mt], b1, acc[mt]);
            }
        }
    }
    SJD_TR(4);
    float *o = out + ((size_t)chunk * (32 * MT)) * N + (size_t)t_out * 32 + (lane & 31);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            o[(size_t)m * N] = acc[mt][r];
        }
#ifdef SJD_TRACE
    SJD_TR(5);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    SJD_TR(6);
#endif
}

// ---- G1z for windows of 65..128 rows (three / four prompts per forward) and for 64-row windows whose K chunk does not fit in LDS: the
// sub-tiled kernel (see g1_skinny_gemm_tiled) over the 12-bit stream.  A sub-tile is 16 k-steps = two groups of four record pairs held in
// two register sets A and B that alternate without copies; the group after next is requested before the MFMAs of the current one; every
// load is unconditional (pairs past the unit's end read as zero through the buffer descriptor, activation pieces are clamped and zeroed),
// the k-steps past a ragged chunk's end are skipped by uniform branches -- ONE loop body for full, last and partial sub-tiles.  With MT
// MFMAs per record the decode (12 VALU) runs under them.  Same MFMA sequence per (tile, chunk) as G1: bit-identical planes.
template <int MT, bool WIDE>
__global__ __launch_bounds__(512) void g1z_skinny_gemm_tiled(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wz,
                                                             const u32x2 *__restrict__ exc, float *__restrict__ out, int M, int N, int K, int KC,
                                                             int n_tiles, int rec_stride, int tile0, int waves_cap)
{
    constexpr int DT = SJD_DTYPE_BF16;
    const int n_waves = waves_cap & 0xffff, exc_cap = waves_cap >> 16;
    SJD_TR(0);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);                 // two buffers of MT * G1_SUB records
    const int chunk = blockIdx.y;
    const int k0 = chunk * KC;
    const int steps = min(KC, K - k0) / 16;
    const int pairs = (steps + 1) / 2, pairs_full = (KC / 16 + 1) / 2;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int t_out = blockIdx.x * n_waves + w;
    const bool has_tile = t_out < N / 32;                        // a wave without a tile streams nothing (its descriptor is empty) and stores nothing
    const int t = tile0 + (has_tile ? t_out : 0);
    const size_t chunk_base = (size_t)chunk * n_tiles * pairs_full;
    const size_t tile_off = (rec_stride == 1) ? (size_t)t * pairs : (size_t)t;
    const unsigned rsb = (unsigned)rec_stride * 1536u;
    const __amdgpu_buffer_rsrc_t wr = g1z_unit_rsrc(wz + (chunk_base + tile_off) * 1536, has_tile ? (unsigned)(pairs - 1) * rsb + 1536u : 0u);
    const int nth = n_waves * 64;
    constexpr int BUF = MT * G1_SUB * 64;                         // u32x4 per LDS buffer
    constexpr int PPR = 2 * G1_SUB;                               // 16-byte pieces per row of a sub-tile
    constexpr int NP = MT * 32 * PPR;                             // pieces per sub-tile
    constexpr int NV = NP / 512;                                  // pieces per thread at 512 threads (2 MT)
    const int n_sub = (steps + G1_SUB - 1) / G1_SUB;
    const int k_end = k0 + steps * 16;
    g1z_pair A[4], B[4];
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;
    auto x_load = [&](int st, int v) -> u32x4 {
        const int m = v / PPR, j = v - m * PPR, col = k0 + st * (16 * G1_SUB) + 8 * j;
        const u32x4 val = *reinterpret_cast<const u32x4 *>(x + (size_t)min(m, M - 1) * K + min(col, K - 8));
        return (m < M && col < k_end) ? val : u32x4{0u, 0u, 0u, 0u};
    };
    auto x_store = [&](int buf, int v, u32x4 val) {
        const int m = v / PPR, j = v - m * PPR, sl = j >> 1;
        xl[buf * BUF + ((m >> 5) * G1_SUB + sl) * 64 + g1_slot(j & 1, m & 31, sl)] = val;
    };
    auto w_load = [&](g1z_pair (&W)[4], int g) {                  // group g of the chunk = pairs 4 g .. 4 g + 3
#pragma unroll
        for (int u = 0; u < 4; ++u) W[u] = g1z_load(wr, (unsigned)lane, (unsigned)(4 * g + u) * rsb);
    };
    auto stage = [&](int st_next, int buf, u32x4 (&val)[NV], bool load) {
        if (load) {
#pragma unroll
            for (int i = 0; i < NV; ++i) val[i] = x_load(st_next, min(threadIdx.x + i * nth, NP - 1));
        } else {
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (threadIdx.x + i * nth < NP) x_store(buf, threadIdx.x + i * nth, val[i]);
            for (int v = threadIdx.x + NV * nth; v < NP; v += nth) x_store(buf, v, x_load(st_next, v));      // fewer than 8 waves
        }
    };
    g1z_hraw hraw;
    {
        u32x4 val[NV];
        stage(0, 0, val, true);
        hraw = g1z_header_load<WIDE>(exc, (size_t)chunk * n_tiles + t, lane, exc_cap);
        w_load(A, 0);
        stage(0, 0, val, false);
    }
    __syncthreads();
    SJD_TR(1);
    const g1z_hdr hd = g1z_header<WIDE>(hraw, lane, exc_cap);
    // eight k-steps from LDS records sl0 .. of the current buffer against the four pairs of W; s0 = the group's first k-step in the chunk
    auto group = [&](const u32x4 *xb, int sl0, const g1z_pair (&W)[4], int s0) {
        u32x4 a[2][MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[0][mt] = xb[(mt * G1_SUB + sl0) * 64 + g1_slot(lane >> 5, lane & 31, 0)];
#pragma unroll
        for (int u = 0; u < G1_UNROLL; ++u) {
            if (u + 1 < G1_UNROLL) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) a[(u + 1) & 1][mt] = xb[(mt * G1_SUB + sl0 + u + 1) * 64 + g1_slot(lane >> 5, lane & 31, u + 1)];
            }
            if (s0 + u < steps) {
                const g1z_pair &pr = W[u >> 1];
                const u32x4 b = (u & 1) ? g1z_operand<WIDE>(pr.lo.z, pr.lo.w, pr.c.y, (unsigned)(s0 + u), hd, lane)
                                        : g1z_operand<WIDE>(pr.lo.x, pr.lo.y, pr.c.x, (unsigned)(s0 + u), hd, lane);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = G1Mfma<DT>::mma(a[u & 1][mt], b, acc[mt]);
            }
        }
    };
    for (int st = 0; st < n_sub; ++st) {
        const u32x4 *xb = xl + (st & 1) * BUF;
        u32x4 val[NV];
        stage(st + 1, (st + 1) & 1, val, true);               // (past the last sub-tile: clamped loads of zeros nobody reads)
        w_load(B, 2 * st + 1);
        __builtin_amdgcn_sched_barrier(0);
        group(xb, 0, A, st * G1_SUB);
        __builtin_amdgcn_sched_barrier(0);
        w_load(A, 2 * st + 2);
        __builtin_amdgcn_sched_barrier(0);
        group(xb, G1_UNROLL, B, st * G1_SUB + G1_UNROLL);
        __builtin_amdgcn_sched_barrier(0);
        stage(st + 1, (st + 1) & 1, val, false);
        __syncthreads();
    }
    SJD_TR(3);
    if (!has_tile) return;
    float *o = out + ((size_t)chunk * (32 * MT)) * N + (size_t)t_out * 32 + (lane & 31);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            o[(size_t)m * N] = acc[mt][r];
        }
}

// x [M <= 128, K] bf16, wz / exc = ops.pack_weight_z(W [N_packed, K], KC, step_major) -> out fp32 [n_chunks, 32 * ceil(M / 32), N] for the N
// columns from 32 * tile0: what sjd_skinny_gemm_cols writes from the uncompressed packing of the same weight, bit for bit.  raw: the packing's
// raw units (include/sjd_hip.h); every branch below knows whether its kernel multiplies them itself or needs the fix-up launch behind it.
extern "C" int sjd_skinny_gemm_z(const void *x, const void *wz, const void *exc, int exc_cap, float *out, int M, int N, int K, int KC, int waves,
                                 int step_major, int dtype, int N_packed, int tile0, const sjd_raw_units *raw, void *stream)
{
    if (!(exc_cap == 32 || exc_cap == 64 || exc_cap == 128) || !g1_raw_desc_ok(raw)) return SJD_ERR_BAD_ARG;
    if (!x || !wz || !exc || !out || M < 1 || N < 32 || (N % 32) != 0 || (N_packed % 32) != 0 || (K % 16) != 0 || KC < 16 || (KC % 16) != 0)
        return SJD_ERR_BAD_ARG;
    if (waves < 1 || waves > 16) return SJD_ERR_BAD_ARG;
    if (dtype != SJD_DTYPE_BF16 || M > 128 || KC > 4096) return SJD_ERR_UNSUPPORTED;      // (the k-step of an exception is 7 + 1 bits of its position)
    const int n_out = N / 32, n_tiles = N_packed / 32, n_chunks = (K + KC - 1) / KC;
    if (tile0 < 0 || tile0 + n_out > n_tiles) return SJD_ERR_BAD_ARG;
    const int MT = (M + 31) / 32;
    const size_t lds = (size_t)MT * ((KC < K ? KC : K) / 16) * 1024;
    const dim3 grid((n_out + waves - 1) / waves, n_chunks), block(waves * 64);
    hipStream_t s = (hipStream_t)stream;
    const int rs = step_major ? n_tiles : 1;
    auto then_raw_fixup = [&](int rc) { return rc != SJD_OK ? rc : g1_raw_units_launch(x, raw, out, M, N, K, KC, tile0, s); };
    // 33..64 rows with FOUR column tiles per workgroup: kernel G1w's 12-bit form (csrc/sjd_gemm_wide.h, template parameter Z).  The one shape where it beats
    // the kernels below -- the o projection of a 64-row window, 9.3 against 10.7 us (profiles/r6_g1wz_sweep_64rows_emu3.jsonl); everywhere else it measured
    // slower and lives in the experimental library only.  It has no in-kernel path for raw units.
    if (MT == 2 && waves == 4)
        return then_raw_fixup(g1_wide_launch_z<2, 1, 4, 4, 3, 2, 2>(x, wz, exc, exc_cap, out, M, N, K, KC, n_tiles, step_major, tile0, s));
    if (MT > 2 || lds > 160 * 1024) {             // sub-tiled activation (65..128 rows, or a 64-row window with a tall K chunk): <= 8 waves, no raw path
        if (waves > 8) return SJD_ERR_BAD_ARG;
        const size_t lds_t = (size_t)2 * MT * G1_SUB * 1024;
#define SJD_G1ZT(MT_, W_) \
        return then_raw_fixup(g1_launch_kernel(g1z_skinny_gemm_tiled<MT_, W_>, grid, block, lds_t, s, x, wz, exc, out, M, N, K, KC, n_tiles, rs, tile0, waves | (exc_cap << 16)))
        if (exc_cap > 64) { if (MT == 2) SJD_G1ZT(2, true); else if (MT == 3) SJD_G1ZT(3, true); else if (MT == 4) SJD_G1ZT(4, true); else return SJD_ERR_UNSUPPORTED; }
        else { if (MT == 2) SJD_G1ZT(2, false); else if (MT == 3) SJD_G1ZT(3, false); else if (MT == 4) SJD_G1ZT(4, false); else return SJD_ERR_UNSUPPORTED; }
#undef SJD_G1ZT
    }
    // g1z_skinny_gemm multiplies raw units in the kernel
#define SJD_G1Z_LAUNCH_W(MT_, MAXT_, W_) \
    return g1_launch_kernel(g1z_skinny_gemm<MT_, MAXT_, W_>, grid, block, lds, s, x, wz, exc, out, M, N, K, KC, n_tiles, rs, tile0, waves | (exc_cap << 16))
#define SJD_G1Z_LAUNCH(MT_, MAXT_) do { if (exc_cap > 64) SJD_G1Z_LAUNCH_W(MT_, MAXT_, true); else SJD_G1Z_LAUNCH_W(MT_, MAXT_, false); } while (0)
    if (MT == 1) { if (waves <= 8) SJD_G1Z_LAUNCH(1, 512); else SJD_G1Z_LAUNCH(1, 1024); }
    else { if (waves <= 8) SJD_G1Z_LAUNCH(2, 512); else SJD_G1Z_LAUNCH(2, 1024); }
#undef SJD_G1Z_LAUNCH
#undef SJD_G1Z_LAUNCH_W
}

// G1p (csrc/sjd_gemm_prefill.h): y [M, N] = round16(row_scale[m] * x [M, K] @ W^T) over a packed copy, any M >= 1; see include/sjd_hip.h
extern "C" int sjd_prefill_gemm(const void *x, const void *w_packed, void *y, int M, int N, int K, int KC, int step_major, int dtype,
                                const float *row_scale, void *stream)
{
    if (!x || !w_packed || !y || M < 1) return SJD_ERR_BAD_ARG;
    return g1p_launch(x, w_packed, y, M, N, K, KC, step_major, dtype, row_scale, (hipStream_t)stream);
}

// out: fp32 [n_chunks, 32, N] partial products; the consumer sums the chunks.
template <int DT, int MT>
static int g1_launch(const void *x, const void *w_packed, float *out, int M, int N, int K, int KC, int waves, int step_major, hipStream_t s,
                     int n_tiles_packed, int tile0)
{
    const int n_out = N / 32, n_tiles = n_tiles_packed > 0 ? n_tiles_packed : n_out, n_chunks = (K + KC - 1) / KC;
    if (tile0 < 0 || tile0 + n_out > n_tiles) return SJD_ERR_BAD_ARG;
    const dim3 grid((n_out + waves - 1) / waves, n_chunks), block(waves * 64);
    const size_t lds_whole = (size_t)MT * ((KC < K ? KC : K) / 16) * 64 * 16;       // the whole activation chunk staged at once
    if constexpr (MT == 2) {
        // 33..64-row windows (Emu3's draft window of 32 with CFG; two prompts per forward) on the uncompressed stream, both 16-bit types: G1w with two
        // row tiles and the register budget of two workgroups per CU (late round 6) -- per launch at Emu3's shapes q|k|v 12.6 / 13.6 us, o 9.4 / 11.2,
        // gate|up 39.0 / 43.1, down 22.5 / 25.2 against the kernels below (profiles/r6_g1w_sweep_64rows_emu3.jsonl); `waves` = column tiles per
        // workgroup: 2, 3, 4, 6, 8.  Same chunking and accumulation order: bit-identical planes.
        if (M > 32) {
            const int rc = g1_wide_by_tiles<DT, MT, 2>(waves, x, w_packed, out, M, N, K, KC, n_tiles, step_major, tile0, s);
            if (rc != G1W_NO_FORM) return rc;          // (any other tile count: the kernels below)
        }
    }
    if constexpr (MT > 4) {      // 129..256-row windows (five to eight prompts per forward), both 16-bit types: G1w (sjd_gemm_wide.h, round 6).  `waves` = column tiles per
        // workgroup: 2, 3, 4 (one per wave) or 6, 8 (two per wave: every activation fragment read from LDS feeds two MFMAs); stages of four k-steps,
        // three ring slots (96 KiB + 1), weight ring of eight k-steps.
        const int rc = g1_wide_by_tiles<DT, MT, 1>(waves, x, w_packed, out, M, N, K, KC, n_tiles, step_major, tile0, s);
        return rc == G1W_NO_FORM ? SJD_ERR_BAD_ARG : rc;
    } else
    if constexpr (MT >= 2) if (MT > 2 || lds_whole > 160 * 1024) {     // sub-tiled activation: no limit on KC
        if (waves > 8) return SJD_ERR_BAD_ARG;
        if constexpr ((MT == 3 || MT == 4) && DT == SJD_DTYPE_BF16) {
            // 65..128-row windows (three / four prompts per forward) in bf16: G1w too (late round 6) -- with its own launch shapes it is 5-10 % faster per
            // launch than the sub-tiled kernels (profiles/r6_g1w_sweep_128rows.jsonl: q|k|v 23.1 / 24.5, o 11.6 / 12.4, gate|up 37.2 / 40.4, down 21.9 / 24.2 us);
            // `waves` = column tiles per workgroup: 2, 3, 4, 6, 8; any other count, or fp16, keeps the sub-tiled kernels below.
            // Same chunking and accumulation order: the planes are the sub-tiled kernels', bit for bit.
            if (M > 64) {          // (G1w has no two-tile form at three row tiles, only at four: the sub-tiled kernel keeps that shape)
                const int rc = g1_wide_by_tiles<DT, MT, 1>(waves, x, w_packed, out, M, N, K, KC, n_tiles, step_major, tile0, s);
                if (rc != G1W_NO_FORM) return rc;
            }
        }
        const int rs = step_major ? n_tiles : 1;
        if constexpr (MT > 2) {      // g1_skinny_gemm_tiled8 with 4 or 8 waves per workgroup: 8-step sub-tiles (4 waves: two workgroups per CU)
            const size_t lds_8 = (size_t)2 * MT * 8 * 1024;
            if (waves == 4) return g1_launch_kernel(g1_skinny_gemm_tiled8<DT, MT, 4>, grid, block, lds_8, s, x, w_packed, out, M, N, K, KC, n_tiles, rs, tile0);
            if (waves == 8) return g1_launch_kernel(g1_skinny_gemm_tiled8<DT, MT, 8>, grid, block, lds_8, s, x, w_packed, out, M, N, K, KC, n_tiles, rs, tile0);
        }
        return g1_launch_kernel(g1_skinny_gemm_tiled<DT, MT>, grid, block, (size_t)2 * MT * G1_SUB * 1024, s, x, w_packed, out, M, N, K, KC, n_tiles, rs, tile0, waves);
    }
    if constexpr (MT <= 2) {
        const size_t lds = lds_whole;
        const int rs = step_major ? n_tiles : 1;
        if (lds > 160 * 1024) return SJD_ERR_BAD_ARG;
        if (waves <= 8)
            return g1_launch_kernel(g1_skinny_gemm<DT, MT, 512>, grid, block, lds, s, x, w_packed, out, M, N, K, KC, n_tiles, rs, tile0, waves, nullptr, nullptr, nullptr);
        return g1_launch_kernel(g1_skinny_gemm<DT, MT, 1024>, grid, block, lds, s, x, w_packed, out, M, N, K, KC, n_tiles, rs, tile0, waves, nullptr, nullptr, nullptr);
    }
    return SJD_ERR_UNSUPPORTED;
}

// the (dtype, row tiles) ladder of the two entry points below, which have checked their arguments
static int g1_dispatch(const void *x, const void *w_packed, float *out, int M, int N, int K, int KC, int waves, int step_major, int dtype, int np, int tile0,
                       hipStream_t s)
{
    auto rows = [&](auto dt) {          // (both entries have checked M <= 256: eight row tiles at the most)
        return g1_by_row_tiles<1, 8>(M, [&](auto mt) {
            return g1_launch<decltype(dt)::value, decltype(mt)::value>(x, w_packed, out, M, N, K, KC, waves, step_major, s, np, tile0); });
    };
    if (dtype == SJD_DTYPE_BF16) return rows(std::integral_constant<int, SJD_DTYPE_BF16>{});
    if (dtype == SJD_DTYPE_F16) return rows(std::integral_constant<int, SJD_DTYPE_F16>{});
    return SJD_ERR_UNSUPPORTED;
}

// Column window of a packed weight: out[c, m, j] for the N = 32 * n columns [32 * tile0, 32 * tile0 + N) of a weight packed with N_packed columns.
extern "C" int sjd_skinny_gemm_cols(const void *x, const void *w_packed, float *out, int M, int N, int K, int KC, int waves, int step_major,
                                    int dtype, int N_packed, int tile0, void *stream)
{
    if (!x || !w_packed || !out || M < 1 || M > 256 || N < 32 || (N % 32) != 0 || (N_packed % 32) != 0 || (K % 16) != 0 || KC < 16 || (KC % 16) != 0)
        return SJD_ERR_BAD_ARG;
    if (waves < 1 || waves > 16) return SJD_ERR_BAD_ARG;
    if (g1_two_streams(dtype)) return SJD_ERR_BAD_ARG;          // one weight stream per call
    if (dtype & SJD_G1_W6_E2M3)                                            // w_packed = ops.pack_weight_q6: G1q6 (csrc/sjd_gemm_q6.h)
        return dtype == (SJD_DTYPE_BF16 | SJD_G1_W6_E2M3) ? g1q6_launch(x, w_packed, out, M, N, K, KC, waves, step_major, N_packed / 32, tile0, (hipStream_t)stream)
                                                          : SJD_ERR_UNSUPPORTED;
    if (dtype & SJD_G1_W4_MXFP4)                                           // w_packed = ops.pack_weight_q4: G1q4 (csrc/sjd_gemm_q4.h)
        return dtype == (SJD_DTYPE_BF16 | SJD_G1_W4_MXFP4) ? g1q4_launch(x, w_packed, out, M, N, K, KC, waves, step_major, N_packed / 32, tile0, (hipStream_t)stream)
                                                           : SJD_ERR_UNSUPPORTED;
    if (dtype & SJD_G1_W8_E4M3)                                            // w_packed = ops.pack_weight_q8: G1q (csrc/sjd_gemm_q8.h)
        return dtype == (SJD_DTYPE_BF16 | SJD_G1_W8_E4M3) ? g1q_launch(x, w_packed, out, M, N, K, KC, waves, step_major, N_packed / 32, tile0, (hipStream_t)stream)
                                                          : SJD_ERR_UNSUPPORTED;
    return g1_dispatch(x, w_packed, out, M, N, K, KC, waves, step_major, dtype, N_packed / 32, tile0, (hipStream_t)stream);
}

// the whole weight: the column window [0, N) of a weight packed with N columns
extern "C" int sjd_skinny_gemm(const void *x, const void *w_packed, float *out, int M, int N, int K, int KC, int waves, int step_major,
                               int dtype, void *stream)
{
    if (!x || !w_packed || !out || M < 1 || M > 256 || (N % 32) != 0 || (K % 16) != 0 || KC < 16 || (KC % 16) != 0) return SJD_ERR_BAD_ARG;
    if (waves < 1 || waves > 16) return SJD_ERR_BAD_ARG;       // (the staged activation chunk must fit in LDS: min(KC, K) <= 2560 / 1280)
    if (g1_two_streams(dtype)) return SJD_ERR_BAD_ARG;
    if (dtype & SJD_G1_W6_E2M3)
        return dtype == (SJD_DTYPE_BF16 | SJD_G1_W6_E2M3) ? g1q6_launch(x, w_packed, out, M, N, K, KC, waves, step_major, N / 32, 0, (hipStream_t)stream)
                                                          : SJD_ERR_UNSUPPORTED;
    if (dtype & SJD_G1_W4_MXFP4)
        return dtype == (SJD_DTYPE_BF16 | SJD_G1_W4_MXFP4) ? g1q4_launch(x, w_packed, out, M, N, K, KC, waves, step_major, N / 32, 0, (hipStream_t)stream)
                                                           : SJD_ERR_UNSUPPORTED;
    if (dtype & SJD_G1_W8_E4M3)
        return dtype == (SJD_DTYPE_BF16 | SJD_G1_W8_E4M3) ? g1q_launch(x, w_packed, out, M, N, K, KC, waves, step_major, N / 32, 0, (hipStream_t)stream)
                                                          : SJD_ERR_UNSUPPORTED;
    return g1_dispatch(x, w_packed, out, M, N, K, KC, waves, step_major, dtype, N / 32, 0, (hipStream_t)stream);
}

#ifdef SJD_EXPERIMENTAL        // G1 + F1r in one launch, the MLP pair, the loader / consumer engine, the G1w tuning entry
// G1 with F1r as its tail (see g1_reduce_tail): h [M, N] += dtype(x @ W^T) in place, sumsq [N / 512, 32] = per-slice sums of h^2 -- what
// sjd_skinny_gemm followed by sjd_residual_sumsq computes, bit for bit, in one launch.  `workspace`: fp32 [n_chunks, 32, N] (the planes
// still travel through memory, device-coherently); `ticket`: N / 512 * 32 zero-initialised uint32 that must not be shared with a launch
// that can run concurrently (it re-arms itself).  M <= 32, N % 512 == 0, waves in {2, 4, 8} with (N / 32) % waves == 0, at most 16 K chunks,
// enough workgroups per slice that each reduces at most waves / 2 rows (2 * ceil(32 / ((16 / waves) * n_chunks)) <= waves: SJD_ERR_UNSUPPORTED
// otherwise -- few-chunk toy shapes), and every workgroup of the launch resident at once: grid <= resident_limit (what the device holds).
extern "C" int sjd_skinny_gemm_reduce(const void *x, const void *w_packed, float *workspace, void *h, float *sumsq, unsigned *ticket, int M, int N,
                                      int K, int KC, int waves, int step_major, int dtype, int resident_limit, void *stream)
{
    if (!x || !w_packed || !workspace || !h || !sumsq || !ticket || M < 1 || M > 32 || N < 512 || (N % 512) != 0 || (K % 16) != 0 || KC < 16 || (KC % 16) != 0)
        return SJD_ERR_BAD_ARG;
    if (!(waves == 1 || waves == 2 || waves == 4 || waves == 8) || ((N / 32) % waves) != 0) return SJD_ERR_UNSUPPORTED;
    const int n_chunks = (K + KC - 1) / KC, n_out = N / 32;
    if (n_chunks > 16) return SJD_ERR_UNSUPPORTED;
    const dim3 grid(n_out / waves, n_chunks), block(waves * 64);
    if ((int)(grid.x * grid.y) > resident_limit) return SJD_ERR_UNSUPPORTED;
    {   // the workgroups of a slice share its 32 rows, two waves per row: a workgroup must have the waves for its share
        const int total = (16 / waves) * n_chunks, per = (32 + total - 1) / total;
        if (2 * per > waves) return SJD_ERR_UNSUPPORTED;
    }
    const size_t lds = (size_t)((KC < K ? KC : K) / 16) * 64 * 16;
    if (lds > 160 * 1024) return SJD_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int rs = step_major ? n_out : 1;
    if (dtype == SJD_DTYPE_BF16)
        return g1_launch_kernel(g1_skinny_gemm<SJD_DTYPE_BF16, 1, 512>, grid, block, lds, s, x, w_packed, workspace, M, N, K, KC, n_out, rs, 0, waves, h, sumsq, ticket);
    if (dtype == SJD_DTYPE_F16)
        return g1_launch_kernel(g1_skinny_gemm<SJD_DTYPE_F16, 1, 512>, grid, block, lds, s, x, w_packed, workspace, M, N, K, KC, n_out, rs, 0, waves, h, sumsq, ticket);
    return SJD_ERR_UNSUPPORTED;
}

// Kernel G1w over the 12-bit stream (late round 6 experiment, csrc/sjd_gemm_wide.h `Z`): bit-identical planes, measured SLOWER than what the product runs
// (the decode costs a one-wave-per-SIMD kernel more issue slots than the 25 % of weight bytes buy: 256 rows q|k|v 44.2 against 35.3 us on the uncompressed
// stream, gate|up 71.3 / 56.8; 64 rows: level with G1z except the o projection, 9.3 / 10.7 us; profiles/r6_g1wz_sweep_*.jsonl).  tiles: 2, 3, 4, 6, 8 column
// tiles per workgroup; 33..256 rows; raw units always through the fix-up launch behind the kernel.
extern "C" int sjd_skinny_gemm_z_wide(const void *x, const void *wz, const void *exc, int exc_cap, float *out, int M, int N, int K, int KC, int tiles,
                                      int step_major, int N_packed, int tile0, const sjd_raw_units *raw, void *stream)
{
    if (!(exc_cap == 32 || exc_cap == 64 || exc_cap == 128) || !g1_raw_desc_ok(raw)) return SJD_ERR_BAD_ARG;
    if (!x || !wz || !exc || !out || M < 33 || M > 256 || N < 32 || (N % 32) != 0 || (N_packed % 32) != 0 || (K % 16) != 0 || KC < 16 || (KC % 16) != 0 || KC > 4096)
        return SJD_ERR_BAD_ARG;
    const int waves = tiles, n_out = N / 32, n_tiles = N_packed / 32, MT = (M + 31) / 32;
    if (tile0 < 0 || tile0 + n_out > n_tiles) return SJD_ERR_BAD_ARG;
    if (!(waves == 2 || waves == 3 || waves == 4 || waves == 6 || waves == 8) || (MT == 3 && waves == 2)) return SJD_ERR_BAD_ARG;
    hipStream_t s_ = (hipStream_t)stream;
    auto then_raw_fixup = [&](int rc) { return rc != SJD_OK ? rc : g1_raw_units_launch(x, raw, out, M, N, K, KC, tile0, s_); };
#define SJD_G1WZ_T(MT_, WPS_) do { switch (waves) { \
        case 2: if constexpr (MT_ != 3) return then_raw_fixup(g1_wide_launch_z<MT_, 1, 2, 4, 3, 2, WPS_>(x, wz, exc, exc_cap, out, M, N, K, KC, n_tiles, step_major, tile0, s_)); else return SJD_ERR_BAD_ARG; \
        case 3: return then_raw_fixup(g1_wide_launch_z<MT_, 1, 3, 4, 3, 2, WPS_>(x, wz, exc, exc_cap, out, M, N, K, KC, n_tiles, step_major, tile0, s_)); \
        case 4: return then_raw_fixup(g1_wide_launch_z<MT_, 1, 4, 4, 3, 2, WPS_>(x, wz, exc, exc_cap, out, M, N, K, KC, n_tiles, step_major, tile0, s_)); \
        case 6: return then_raw_fixup(g1_wide_launch_z<MT_, 2, 3, 4, 3, 2, WPS_>(x, wz, exc, exc_cap, out, M, N, K, KC, n_tiles, step_major, tile0, s_)); \
        default: return then_raw_fixup(g1_wide_launch_z<MT_, 2, 4, 4, 3, 2, WPS_>(x, wz, exc, exc_cap, out, M, N, K, KC, n_tiles, step_major, tile0, s_)); } } while (0)
    switch (MT) {
    case 2: SJD_G1WZ_T(2, 2);
    case 3: SJD_G1WZ_T(3, 1);
    case 4: SJD_G1WZ_T(4, 1);
    case 5: SJD_G1WZ_T(5, 1);
    case 6: SJD_G1WZ_T(6, 1);
    case 7: SJD_G1WZ_T(7, 1);
    default: SJD_G1WZ_T(8, 1);
    }
#undef SJD_G1WZ_T
}

// G1w tuning entry (tools/g1w_bench.py): bf16; M <= 128 runs four row tiles, M <= 256 eight; tiles = column tiles per workgroup (2, 3, 4: one per
// wave; 6, 8: two per wave); variant = (stage k-steps, ring slots, weight ring stages): 0 (4, 3, 2) = the product's  1 (4, 4, 2)  10: eight waves with
// one tile each (tiles = 8, two waves per SIMD)  20: four row tiles in the register budget of two workgroups per CU.  ldx: row stride of x.
extern "C" int sjd_skinny_gemm_wide(const void *x, const void *w_packed, float *out, int M, int N, int K, int KC, int tiles, int step_major,
                                    int variant, int ldx, void *stream)
{
    if (!x || !w_packed || !out || M < 1 || M > 256 || N < 32 || (N % 32) != 0 || (K % 16) != 0 || KC < 16 || (KC % 16) != 0) return SJD_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nt = N / 32;
#define SJD_G1W_V(MT_, CT_, NW_, SUB_, NS_, RW_, WPS_) return g1_wide_launch<SJD_DTYPE_BF16, MT_, CT_, NW_, SUB_, NS_, RW_, WPS_>(x, w_packed, out, M, N, K, KC, nt, step_major, 0, s, ldx)
#define SJD_G1W_T(MT_, SUB_, NS_, RW_, WPS_) do { switch (tiles) { case 2: SJD_G1W_V(MT_, 1, 2, SUB_, NS_, RW_, WPS_); case 3: SJD_G1W_V(MT_, 1, 3, SUB_, NS_, RW_, WPS_); \
        case 4: SJD_G1W_V(MT_, 1, 4, SUB_, NS_, RW_, WPS_); case 6: SJD_G1W_V(MT_, 2, 3, SUB_, NS_, RW_, WPS_); case 8: SJD_G1W_V(MT_, 2, 4, SUB_, NS_, RW_, WPS_); \
        default: return SJD_ERR_BAD_ARG; } } while (0)
    if (M > 128) {
        switch (variant) {
        case 0: SJD_G1W_T(8, 4, 3, 2, 1);
        case 1: SJD_G1W_T(8, 4, 4, 2, 1);
        case 10: if (tiles == 8) SJD_G1W_V(8, 1, 8, 4, 3, 2, 2); return SJD_ERR_BAD_ARG;
        default: return SJD_ERR_BAD_ARG;
        }
    }
    if (M <= 64) {          // (late round 6: two row tiles -- Emu3's 64-row windows, two prompts per forward)
        switch (variant) {
        case 0: SJD_G1W_T(2, 4, 3, 2, 1);
        case 20: SJD_G1W_T(2, 4, 3, 2, 2);
        case 21: SJD_G1W_T(2, 8, 3, 1, 2);
        case 22: SJD_G1W_T(2, 4, 4, 2, 2);
        default: return SJD_ERR_BAD_ARG;
        }
    }
    switch (variant) {
    case 0: SJD_G1W_T(4, 4, 3, 2, 1);
    case 20: SJD_G1W_T(4, 4, 3, 2, 2);
    default: return SJD_ERR_BAD_ARG;
    }
#undef SJD_G1W_T
#undef SJD_G1W_V
}

// workgroups of a reducing launch that gave up waiting for their slice's ticket since the library was loaded (0 on a healthy device)
#include "sjd_gemm_pair.h"
#include "sjd_gemm_engine.h"

extern "C" int sjd_reduce_timeouts(void)
{
    unsigned v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g1_red_timeouts), sizeof(v), 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int)v;
}

#endif  // SJD_EXPERIMENTAL

#ifdef SJD_TRACE
extern "C" int sjd_debug_trace_g1(unsigned long long *host_out, int n_wg)
{
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_g1_trace), (size_t)n_wg * 8 * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

#ifdef SJD_EXPERIMENTAL
// ------------------------------------------------------------------------------------------------ round 6 gate probe (VERDICT r5 "next #4")
// "Let the o projection consume K1's split partials": the activation-staging prologue of every o-projection workgroup would merge the n_split
// partial triples (m, l, O[128]) of its K chunk's heads instead of reading the 32 KB of merged activations.  This kernel IS that prologue and
// nothing else, on the o projection's grid (22 column groups x 8 K chunks of 512 = 4 heads, 384 threads): for 32 window rows x 4 heads it reads
// 4 splits x (2 + 128) fp32 -- 266 KB per workgroup against 32 KB, the 22 column groups of a chunk re-merging the same heads -- merges them in
// k1_combine's order (max, exp2f weights, sum, one division) and leaves the bf16 tile in LDS.  mode 0: the same launch with an empty body.
// Timed in a hipGraph (tools/o_merge_probe.py): the prologue's cost is mode 1 - mode 0, to hold against k1_combine's 4.98 us + one kernel boundary.
__global__ __launch_bounds__(384) void o_merge_prologue_probe(const float *__restrict__ part, float *__restrict__ sink, int n_split, int rows, int mode)
{
    __shared__ unsigned short xs[32 * 512];
    if (mode == 0) { if (part == nullptr) sink[0] = 0.f; return; }
    const int chunk = blockIdx.y;                                   // heads 4 * chunk .. 4 * chunk + 3
    // part: [head 32][split n_split][row rows][2 + 128] fp32
    float keep = 0.f;
    for (int item = threadIdx.x; item < rows * 4 * 32; item += 384) {          // (row, head, four output columns)
        const int d4 = item & 31, hr = item >> 5, h = hr & 3, r = hr >> 2;
        const float *base = part + (((size_t)(4 * chunk + h) * n_split) * rows + r) * 130;
        float m[4], l[4];
        float4 o[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float *p = base + (size_t)min(s, n_split - 1) * rows * 130;
            m[s] = p[0]; l[s] = p[1];
            o[s] = *reinterpret_cast<const float4 *>(p + 2 + 4 * d4 + 2);      // (16-byte aligned: rows of 130 floats, +2 pad)
        }
        float M = m[0];
#pragma unroll
        for (int s = 1; s < 4; ++s) M = fmaxf(M, m[s]);
        float L = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float w = exp2f(m[s] - M);
            L += w * l[s]; a0 += w * o[s].x; a1 += w * o[s].y; a2 += w * o[s].z; a3 += w * o[s].w;
        }
        const float inv = 1.0f / L;
        unsigned short *dst = xs + r * 512 + h * 128 + 4 * d4;
        auto bf = [](float x) { unsigned u = __float_as_uint(x); u += 0x7fffu + ((u >> 16) & 1u); return (unsigned short)(u >> 16); };
        dst[0] = bf(a0 * inv); dst[1] = bf(a1 * inv); dst[2] = bf(a2 * inv); dst[3] = bf(a3 * inv);
        keep += a0;
    }
    __syncthreads();
    if (keep == 12345.678f) sink[blockIdx.x] = (float)xs[threadIdx.x];          // (keeps the LDS tile alive)
}

extern "C" int sjd_o_merge_prologue_probe(const float *part, float *sink, int n_split, int rows, int mode, void *stream)
{
    if (!part || !sink || n_split < 1 || n_split > 4 || rows < 1 || rows > 32) return SJD_ERR_BAD_ARG;
    return g1_launch_kernel(o_merge_prologue_probe, dim3(22, 8), dim3(384), 0, (hipStream_t)stream, part, sink, n_split, rows, mode);
}
#endif  // SJD_EXPERIMENTAL
