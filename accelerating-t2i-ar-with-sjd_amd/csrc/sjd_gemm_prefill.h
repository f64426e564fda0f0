// sjd_gemm_prefill.h -- G1p: the PREFILL projection over the packed weight copies of the window kernels, at any row count.  Included by sjd_gemm.hip
// behind sjd_gemm_q8.h / sjd_gemm_q4.h, whose operand decodes (g1q_operand, g1q4_operand, g1q4_scale) and whose byte layouts it reads as they are.
//
//   y[m, n] = round16(rs[m] * sum_k x[m, k] * W[n, k])          x [M, K] bf16, y [M, N] bf16, rs fp32 [M] or NULL (= 1)
//
// Three weight forms behind ONE body (template parameter FMT): 0 the plain packing (ops.pack_weight: 1-KiB records, one per k-step), 8 the e4m3 stream
// (ops.pack_weight_q8: record pairs + fp32 column scales), 4 the MXFP4 stream (ops.pack_weight_q4: records of four k-steps + one e8m0 scale dword per lane
// and trip of eight).  The copy is read with the chunk KC and the record order (tile-major / step-major) it was packed with; a gate|up copy is the same
// bytes as any other with KC = K / 2.  No second packing, no split-K planes, no fp32 workspace: at prefill row counts the ROWS supply the parallelism.
//
// Structure.  A workgroup of G1P_WAVES waves owns a block of G1P_ROWS rows x G1P_WAVES column tiles (one 32-column tile per wave, G1P_ROWS / 32 accumulator
// tiles each) and runs the WHOLE of K, chunk after chunk, in stages of up to eight k-steps (128 columns: one MXFP4 trip; a chunk of the other two forms is
// whole record pairs, so a stage is 2, 4, 6 or 8 k-steps).  The activation stage travels global -> registers -> LDS in G1's fragment-major order (g1_slot:
// both sides conflict-free) into one of two buffers; the next stage's activation and weight loads are issued in front of the current stage's MFMAs, one
// barrier per stage.  The weight records go global -> MFMA B registers directly (the packed stream IS the operand order) with plain cached loads: every
// row block re-reads them, so they are not marked non-temporal.
//
// Accumulation order: every output element is ONE fp32 MFMA accumulator chain over the k-steps in k order (chunk after chunk), started from zero -- it
// depends on k alone: not on the row's position in its block, not on M, not on which workgroup ran it, and not on the weight form (the quantised forms
// rebuild the bf16 operand bit for bit, so the output equals the plain form's on pack_weight(dequant()), bit for bit).  Rows >= M are staged as zeros and
// never stored.  The row scale multiplies the finished fp32 sum (F2 / F3's definition of the folded RMSNorm) in front of the one 16-bit rounding.
#pragma once

constexpr int G1P_ROWS = 128;          // rows of a workgroup's block (ops: LS.PREFILL_ROW_BLOCK)
constexpr int G1P_WAVES = 4;           // waves = column tiles per workgroup
constexpr int G1P_STAGE = 8;           // k-steps per activation stage

// the weight registers of one stage: FMT 0 eight records, FMT 8 four record pairs, FMT 4 two records and the trip's scale dword
template <int FMT> struct g1p_wstage {
    u32x4 r[FMT == 0 ? 8 : FMT == 8 ? 4 : 2];
    unsigned sd;
};

template <int FMT>
__global__ __launch_bounds__(64 * G1P_WAVES) void g1p_prefill_gemm(const unsigned short *__restrict__ x, const unsigned char *__restrict__ wq,
                                                                   const float *__restrict__ row_scale, unsigned short *__restrict__ y, int M, int N,
                                                                   int K, int KC, int n_tiles, int rec_stride)
{
    constexpr int DT = SJD_DTYPE_BF16;
    constexpr int MT = G1P_ROWS / 32, NT = 64 * G1P_WAVES;
    constexpr int PPR = 2 * G1P_STAGE;                             // 16-byte pieces per row and stage
    constexpr int PPT = G1P_ROWS * PPR / NT;                       // ... per thread and stage
    constexpr int BUF = MT * G1P_STAGE * 64;                       // u32x4 per buffer
    static_assert(NT % PPR == 0 && (G1P_ROWS * PPR) % NT == 0, "a thread keeps its piece column; its rows are NT / PPR apart");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4 *xl = reinterpret_cast<u32x4 *>(smem);
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int row0 = blockIdx.x * G1P_ROWS;
    const int t = blockIdx.y * G1P_WAVES + w;
    const bool has_tile = t < N / 32;
    const int n_chunks = (K + KC - 1) / KC;
    [[maybe_unused]] float sc8 = 0.f;                                                                // (FMT 8) this lane's fp32 column scale, from behind the records
    if constexpr (FMT == 8) sc8 = has_tile ? reinterpret_cast<const float *>(wq + (size_t)n_tiles * 32 * K)[32 * t + (lane & 31)] : 0.f;

    // this thread's pieces of a stage: column piece pj of rows pm0 + i * (NT / PPR)
    const int pj = threadIdx.x % PPR, pm0 = threadIdx.x / PPR;
    auto x_load = [&](u32x4 (&val)[PPT], int col0, int ns) {
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int m = row0 + pm0 + i * (NT / PPR);
            val[i] = (m < M && pj < 2 * ns) ? *reinterpret_cast<const u32x4 *>(x + (size_t)m * K + col0 + 8 * pj) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto x_store = [&](const u32x4 (&val)[PPT], int buf, int ns) {
        if (pj < 2 * ns) {
#pragma unroll
            for (int i = 0; i < PPT; ++i) {
                const int m = pm0 + i * (NT / PPR);
                xl[buf * BUF + ((m >> 5) * G1P_STAGE + (pj >> 1)) * 64 + g1_slot(pj & 1, m & 31, pj >> 1)] = val[i];
            }
        }
    };
    // the weight bytes of the stage at k-step s0 (a multiple of eight) of chunk c, ns k-steps: the layouts of pack_weight / pack_weight_q8 / pack_weight_q4
    auto w_load = [&](g1p_wstage<FMT> &ws, int c, int s0, int ns) {
        const int k0 = c * KC;
        const int steps = min(KC, K - k0) / 16;
        if constexpr (FMT == 0) {
            const size_t base = (size_t)c * n_tiles * (KC / 16);                                     // records in front of the chunk
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < ns) {
                    const size_t rec = base + (rec_stride == 1 ? (size_t)t * steps + (s0 + u) : (size_t)(s0 + u) * n_tiles + t);
                    ws.r[u] = *reinterpret_cast<const u32x4 *>(wq + rec * 1024 + (size_t)lane * 16);
                }
        } else if constexpr (FMT == 8) {
            const unsigned char *cb = wq + (size_t)k0 * ((size_t)n_tiles * 32);
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (2 * p < ns) {
                    const int pa = s0 / 2 + p;
                    const size_t off = rec_stride == 1 ? (size_t)t * steps * 512 + (size_t)pa * 1024 : ((size_t)pa * n_tiles + t) * 1024;
                    ws.r[p] = *reinterpret_cast<const u32x4 *>(cb + off + (size_t)lane * 16);
                }
        } else {
            const unsigned char *cb = wq + (size_t)k0 * ((size_t)n_tiles * 16);
            const unsigned char *sb = wq + (size_t)n_tiles * 16 * K + (size_t)k0 * (size_t)n_tiles;      // the e8m0 scale groups sit behind the records
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int ra = s0 / 4 + q;
                const size_t off = rec_stride == 1 ? (size_t)t * steps * 256 + (size_t)ra * 1024 : ((size_t)ra * n_tiles + t) * 1024;
                ws.r[q] = *reinterpret_cast<const u32x4 *>(cb + off + (size_t)lane * 16);
            }
            const int qa = s0 / 8;
            const size_t soff = rec_stride == 1 ? (size_t)t * steps * 16 + (size_t)qa * 128 : ((size_t)qa * n_tiles + t) * 128;
            ws.sd = *reinterpret_cast<const unsigned *>(sb + soff + (size_t)(lane & 31) * 4);
        }
    };
    // the MFMA B operand of k-step u of the stage
    auto operand = [&](const g1p_wstage<FMT> &ws, int u) -> u32x4 {
        if constexpr (FMT == 0) return ws.r[u];
        else if constexpr (FMT == 8) {
            const u32x4 &p = ws.r[u >> 1];
            return (u & 1) ? g1q_operand(p.z, p.w, sc8) : g1q_operand(p.x, p.y, sc8);
        } else {
            const u32x4 &rec = ws.r[u >> 2];
            const unsigned code = (u & 3) == 0 ? rec.x : (u & 3) == 1 ? rec.y : (u & 3) == 2 ? rec.z : rec.w;
            const float sc = (u >> 1) == 0 ? g1q4_scale<0>(ws.sd) : (u >> 1) == 1 ? g1q4_scale<1>(ws.sd) : (u >> 1) == 2 ? g1q4_scale<2>(ws.sd) : g1q4_scale<3>(ws.sd);
            return g1q4_operand(code, sc);
        }
    };

    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;

    // the stage walk: (c, s0) over the chunks and their stages of eight k-steps, in k order
    auto steps_of = [&](int c) { return min(KC, K - c * KC) / 16; };
    int c = 0, s0 = 0, ns = min(G1P_STAGE, steps_of(0));
    g1p_wstage<FMT> wcur, wnext;
    u32x4 val[PPT];
    x_load(val, 0, ns);
    if (has_tile) w_load(wcur, 0, 0, ns);
    x_store(val, 0, ns);
    __syncthreads();
    int buf = 0;
    for (;;) {
        int cn = c, sn = s0 + G1P_STAGE;
        if (sn >= steps_of(c)) { cn = c + 1; sn = 0; }
        const bool more = cn < n_chunks;                               // (uniform)
        const int nsn = more ? min(G1P_STAGE, steps_of(cn) - sn) : 0;
        if (more) {
            x_load(val, cn * KC + 16 * sn, nsn);
            if (has_tile) w_load(wnext, cn, sn, nsn);
        }
        if (has_tile) {
            const u32x4 *xb = xl + buf * BUF;
#pragma unroll
            for (int u = 0; u < G1P_STAGE; ++u)
                if (u < ns) {
                    const u32x4 b = operand(wcur, u);
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
                        acc[mt] = G1Mfma<DT>::mma(xb[(mt * G1P_STAGE + u) * 64 + g1_slot(lane >> 5, lane & 31, u)], b, acc[mt]);
                }
        }
        if (!more) break;
        x_store(val, buf ^ 1, nsn);
        __syncthreads();               // everybody's pieces of the next stage are in place; everybody is done reading this one
        wcur = wnext;
        buf ^= 1; c = cn; s0 = sn; ns = nsn;
    }
    if (!has_tile) return;
    unsigned short *o = y + (size_t)t * 32 + (lane & 31);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = row0 + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m < M) {
#pragma clang fp contract(off)
                const float v = row_scale ? acc[mt][r] * row_scale[m] : acc[mt][r];
                o[(size_t)m * N] = SjdAct<DT>::from_f(v);
            }
        }
}

// sjd_prefill_gemm, which has checked the pointers and M: everything the kernel does not serve is refused here, before any launch
static int g1p_launch(const void *x, const void *w_packed, void *y, int M, int N, int K, int KC, int step_major, int dtype, const float *row_scale,
                      hipStream_t s)
{
    if ((dtype & SJD_G1_W8_E4M3) && (dtype & SJD_G1_W4_MXFP4)) return SJD_ERR_BAD_ARG;          // one weight stream per call
    const int fmt = (dtype & SJD_G1_W4_MXFP4) ? 4 : (dtype & SJD_G1_W8_E4M3) ? 8 : 0;
    if ((dtype & ~(SJD_G1_W8_E4M3 | SJD_G1_W4_MXFP4)) != SJD_DTYPE_BF16) return SJD_ERR_UNSUPPORTED;      // bf16: the quantised streams are
    const int gran = fmt == 4 ? 128 : 32;                          // whole MXFP4 trips / whole record pairs
    if (N < 32 || (N % 32) != 0 || K < gran || (K % gran) != 0 || KC < gran || (KC % gran) != 0) return SJD_ERR_UNSUPPORTED;
    const int n_tiles = N / 32;
    const dim3 grid((M + G1P_ROWS - 1) / G1P_ROWS, (n_tiles + G1P_WAVES - 1) / G1P_WAVES), block(64 * G1P_WAVES);
    if (grid.y > 65535u) return SJD_ERR_UNSUPPORTED;
    constexpr size_t lds = (size_t)2 * (G1P_ROWS / 32) * G1P_STAGE * 1024;
    static_assert(lds <= 160 * 1024, "two activation buffers in LDS");
    const int rs = step_major ? n_tiles : 1;
    const unsigned char *wq = static_cast<const unsigned char *>(w_packed);
    if (fmt == 4) return g1_launch_kernel(g1p_prefill_gemm<4>, grid, block, lds, s, x, wq, row_scale, y, M, N, K, KC, n_tiles, rs);
    if (fmt == 8) return g1_launch_kernel(g1p_prefill_gemm<8>, grid, block, lds, s, x, wq, row_scale, y, M, N, K, KC, n_tiles, rs);
    return g1_launch_kernel(g1p_prefill_gemm<0>, grid, block, lds, s, x, wq, row_scale, y, M, N, K, KC, n_tiles, rs);
}
