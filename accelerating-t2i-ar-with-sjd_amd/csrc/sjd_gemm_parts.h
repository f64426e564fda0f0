// sjd_gemm_parts.h -- what the launchers and kernels of the G1 family share, once.  Included by sjd_gemm.hip behind g1_slot / G1Mfma / G1_STAGE.
//
//   G1S_RP, g1s_epilogue_lds   the row pitch of the gate|up epilogue's planes in LDS and the bytes they take: the gate|up kernels and their
//                              launchers read the same constant
//   g1s_row_sumsq_load, g1s_row_scale   the folded RMSNorm's row scale of the gate|up kernels: the eight loads every thread issues, and the finish
//   g1s_plane_store, g1s_finish         the gate|up epilogue: a wave's accumulators as a plane in LDS; planes summed in chunk order, SiLU * up, store
//   g1s_norm_args             sjd_row_norm unpacked into the four kernel arguments of the folded RMSNorm
//   g1_stream_launch           the launcher body of a quantised stream's whole-chunk kernel (G1q, G1q4, G1q6)
//   g1s_stream_launch          ... and of its 32-row gate|up kernel (G1sq, G1sq4, G1sq6)
// A new quantised stream supplies its kernels, its bytes per weight and its own refusals; the argument checks, the LDS limit, the grid and the
// (row tiles, threads) / phase-length ladders are here.
// Shared elsewhere, by TEMPLATE PARAMETER: the kernels of the two block-scaled streams (MXFP4, e2m3) are one whole-chunk and one gate|up template
// over a stream-traits struct (csrc/sjd_gemm_qblock.h).  The body stands in place, once; only the record type, its sizes, its load and its half
// trip come from the parameter, so an instantiation is the machine code of the copy it replaced.
// Of the DEVICE bodies the kernels repeat, the gate|up kernels' tail (row scale, plane store, finish) is here: it runs behind the weight stream or
// on cache hits, its 31 instantiations compile to other machine code than the copies did and were timed against them (DESIGN.md 4.2f;
// g1z_gateup_silu, the headline's kernel, keeps its copy).  The
// bodies ON the streaming path (whole-chunk staging, phase staging, g1_wide's plane store) are NOT gathered: as force-inlined functions they
// changed the machine code of every kernel that called them -- the optimiser simplifies a callee on its own before it inlines it, so operand
// orders and what is known about `lane` differ from the code written in place -- and each needs a timing of its own.  (A template over types
// and constants is not such a function: nothing is simplified apart from its caller.  That is how sjd_gemm_qblock.h shares whole kernels.)
// Not on the helpers: the raw gate|up fix-up (csrc/sjd_gemm_raw.h: planes [4][32][33], row scale read per thread, one tile pair per workgroup) and
// the MLP pair's gate|up phase (csrc/sjd_gemm_pair.h: workgroup index `bid`, write-through 8-byte stores) -- their indexing differs.
#pragma once

// The gate|up epilogue's eight planes (tile q x K half) go through LDS row-major, rows padded to G1S_RP floats: conflict-free both ways.
constexpr int G1S_RP = 36;
constexpr size_t g1s_epilogue_lds(int MT) { return (size_t)8 * 32 * MT * G1S_RP * sizeof(float); }      // (the launchers take the larger of this and the activation arena)

// ---- the tail of the gate|up kernels, once.  Everything here runs behind the weight stream or on cache hits; the BARRIERS around it (the one
// that frees the activation arena, the one between plane store and finish) stay in the kernels: where they sit is part of each kernel's schedule.
// The helpers derive lane and thread index from threadIdx.x themselves: passed in, `lane` is an opaque integer and the known-bits folds go.

// The per-slice sums of h^2 behind the row scale r = rsqrt(mean(h^2) + eps) of the folded RMSNorm (F1r wrote them as [slices][rs_rows]; at most
// eight slices).  Every thread issues the eight loads -- unconditional (no norm: they read x), so the waits around them stay exact.  The kernels
// call this BEHIND the first activation batch and ahead of the first weight loads: cache hits that cost the staging nothing (see g1_gateup_silu).
// R = rows of the window's tile (32 MT): thread -> row min(thread % R, rs_rows - 1), which is thread % R where rs_rows is the constant R.
template <int R>
__device__ __forceinline__ void g1s_row_sumsq_load(float (&ssv)[8], const unsigned short *__restrict__ x, const float *__restrict__ row_sumsq,
                                                   int rs_slices, int rs_rows)
{
    const float *ssp = row_sumsq ? row_sumsq : reinterpret_cast<const float *>(x);
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) ssv[qq] = ssp[(size_t)(row_sumsq ? min(qq, rs_slices - 1) : 0) * rs_rows + min((int)(threadIdx.x & (R - 1)), rs_rows - 1)];
}

// ... and the row scale from them, by the first R threads into rsc[R] (LDS): sjd_glue.hip row_sumsq_total -- one batch of eight in slice order,
// missing slices add zero.  No norm: 1.
template <int R>
__device__ __forceinline__ void g1s_row_scale(float *rsc, const float (&ssv)[8], const float *__restrict__ row_sumsq, int rs_slices,
                                              float rs_inv_hidden, float rs_eps)
{
    if (threadIdx.x < R) {
        float tsum = 0.f;
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) tsum += (qq < rs_slices) ? ssv[qq] : 0.f;
        rsc[threadIdx.x] = row_sumsq ? rsqrtf(__builtin_fmaf(tsum, rs_inv_hidden, rs_eps)) : 1.0f;
    }
}

// A wave's MT fp32 accumulators as plane `plane` of red[planes][32 MT rows][G1S_RP] (LDS).  The kernels number their planes chunk * 4 + q
// (q = 0, 1: the gate tiles, 2, 3: the up tiles of the same columns).
template <int MT>
__device__ __forceinline__ void g1s_plane_store(float *red, int plane, const f32x16 *acc)
{
    constexpr int R = 32 * MT;
    const int lane = threadIdx.x & 63;
    float *mine = red + (size_t)plane * R * G1S_RP + (lane & 31);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) mine[(32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * G1S_RP] = acc[mt][r];
}

// The finish over NC chunk planes per tile: MT passes of the 512 threads, each one (activation tile a, row m, four columns c4) -- F3's arithmetic:
// the gate and the up planes summed in chunk order starting from zero, sjd_silu_mul_elem (sjd_mlp_epilogue.h: the element arithmetic F3 uses,
// same bits), 8 bytes stored under m < M.  Bit-identical to G1 + F3.
template <int DT, int MT, int NC>
__device__ __forceinline__ void g1s_finish(const float *red, const float *rsc, unsigned short *__restrict__ y, int M, int I)
{
    constexpr int R = 32 * MT;
#pragma unroll
    for (int it = 0; it < MT; ++it) {
        const int idx = it * 512 + (int)threadIdx.x;
        const int a = idx / (8 * R), m = (idx >> 3) % R, c4 = (idx & 7) * 4;
        auto plane = [&](int c_, int q_) { return *reinterpret_cast<const float4 *>(red + ((size_t)(c_ * 4 + q_) * R + m) * G1S_RP + c4); };
        float gv[NC][4], uv[NC][4];
#pragma unroll
        for (int c = 0; c < NC; ++c) { const float4 g = plane(c, a); gv[c][0] = g.x; gv[c][1] = g.y; gv[c][2] = g.z; gv[c][3] = g.w; }
#pragma unroll
        for (int c = 0; c < NC; ++c) { const float4 u = plane(c, 2 + a); uv[c][0] = u.x; uv[c][1] = u.y; uv[c][2] = u.z; uv[c][3] = u.w; }
        const float rr = rsc[m];
        unsigned short o16[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gsum = 0.f, usum = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) gsum += gv[c][j];
#pragma unroll
            for (int c = 0; c < NC; ++c) usum += uv[c][j];
            o16[j] = sjd_silu_mul_elem<DT>(gsum, usum, rr);
        }
        if (m < M) {
            uint2 pk{(unsigned)o16[0] | ((unsigned)o16[1] << 16), (unsigned)o16[2] | ((unsigned)o16[3] << 16)};
            *reinterpret_cast<uint2 *>(y + (size_t)m * I + 32 * (2 * blockIdx.x + a) + c4) = pk;
        }
    }
}

// the four kernel arguments of a folded RMSNorm from the entry points' descriptor (NULL: no norm, the kernels scale by 1)
struct g1s_norm_args {
    const float *ss; int sl; float ih, eps;
    explicit g1s_norm_args(const sjd_row_norm *rn)
        : ss(rn ? rn->sumsq : nullptr), sl(rn ? rn->slices : 0), ih(rn ? 1.0f / (float)rn->hidden : 0.f), eps(rn ? rn->eps : 0.f) {}
};

// The launcher of a quantised stream's whole-chunk kernel (G1q, G1q4, G1q6) behind sjd_skinny_gemm / sjd_skinny_gemm_cols, which have checked the common
// arguments: M <= 64 with the activation chunk in LDS -- min(KC, K) <= 2560 up to 32 rows, <= 1280 at 33..64.
//   tile_k_bytes   the stream's record bytes per 32-column tile and column of K (32 at one byte per weight); the scales sit behind n_tiles * K of them
//   other_form()   the stream's own refusals (its K granule) and its forms for more rows: an SJD_* code, or G1_STREAM_GO for this launcher's shapes
//   launch(MT, MAXT, grid, block, lds, scales, rs)   names the kernel (MT, MAXT: std::integral_constant)
constexpr int G1_STREAM_GO = 1;          // internal, like G1W_NO_FORM: never leaves this translation unit
static_assert(G1_STREAM_GO != SJD_OK && G1_STREAM_GO != SJD_ERR_BAD_ARG && G1_STREAM_GO != SJD_ERR_UNSUPPORTED && G1_STREAM_GO != SJD_ERR_LAUNCH, "not a return code");
template <typename Other, typename Launch>
static int g1_stream_launch(const void *wq, int M, int N, int K, int KC, int waves, int step_major, int n_tiles, int tile0, int tile_k_bytes,
                            Other other_form, Launch launch)
{
    if (N < 32) return SJD_ERR_BAD_ARG;
    const int n_out = N / 32, n_chunks = (K + KC - 1) / KC;
    if (tile0 < 0 || tile0 + n_out > n_tiles) return SJD_ERR_BAD_ARG;
    if (const int rc = other_form(); rc != G1_STREAM_GO) return rc;
    const int MT = M <= 32 ? 1 : 2;
    const size_t lds = (size_t)MT * ((KC < K ? KC : K) / 16) * 1024;
    if (lds > 160 * 1024) return SJD_ERR_UNSUPPORTED;
    const unsigned char *scales = static_cast<const unsigned char *>(wq) + (size_t)n_tiles * tile_k_bytes * K;
    const dim3 grid((n_out + waves - 1) / waves, n_chunks), block(waves * 64);
    const int rs = step_major ? n_tiles : 1;
    using one = std::integral_constant<int, 1>; using two = std::integral_constant<int, 2>;
    using t512 = std::integral_constant<int, 512>; using t1024 = std::integral_constant<int, 1024>;
    if (MT == 1) return waves <= 8 ? launch(one{}, t512{}, grid, block, lds, scales, rs) : launch(one{}, t1024{}, grid, block, lds, scales, rs);
    return waves <= 8 ? launch(two{}, t512{}, grid, block, lds, scales, rs) : launch(two{}, t1024{}, grid, block, lds, scales, rs);
}

// ... and of its 32-row gate|up kernel (G1sq, G1sq4, G1sq6) behind sjd_gateup_silu: M <= 32; the packed weight is [Wg; Wu], 2 I / 32 tiles.
//   launch(SP, grid, block, lds, scales, rec_stride, norm)   names the kernel (SP = K / 64 k-steps per phase: std::integral_constant)
template <typename Launch>
static int g1s_stream_launch(const void *wq, int M, int I, int K, int step_major, int tile_k_bytes, const sjd_row_norm *rn, Launch launch)
{
    if (M > 32) return SJD_ERR_UNSUPPORTED;
    const int SP = K / 64;
    const dim3 grid(I / 64), block(512);
    const size_t lds_x = (size_t)2 * SP * 1024, lds_red = g1s_epilogue_lds(1);
    const size_t lds = lds_x > lds_red ? lds_x : lds_red;
    const int rec_stride = step_major ? 2 * (I / 32) : 1;
    const unsigned char *scales = static_cast<const unsigned char *>(wq) + (size_t)(2 * (I / 32)) * tile_k_bytes * K;
    const g1s_norm_args n(rn);
    if (SP == 8) return launch(std::integral_constant<int, 8>{}, grid, block, lds, scales, rec_stride, n);
    if (SP == 16) return launch(std::integral_constant<int, 16>{}, grid, block, lds, scales, rec_stride, n);
    if (SP == 32) return launch(std::integral_constant<int, 32>{}, grid, block, lds, scales, rec_stride, n);
    if (SP == 64) return launch(std::integral_constant<int, 64>{}, grid, block, lds, scales, rec_stride, n);
    return SJD_ERR_UNSUPPORTED;
}
