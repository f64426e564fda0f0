// sjd_gemm_parts.h -- what the launchers and kernels of the G1 family share, once.  Included by sjd_gemm.hip behind g1_slot / G1Mfma / G1_STAGE.
//
//   G1S_RP, g1s_epilogue_lds   the row pitch of the gate|up epilogue's planes in LDS and the bytes they take: the six gate|up kernels and their
//                              launchers read the same constant
//   g1s_norm_args              sjd_row_norm unpacked into the four kernel arguments of the folded RMSNorm
//   g1_stream_launch           the launcher body of a quantised stream's whole-chunk kernel (G1q, G1q4)
//   g1s_stream_launch          ... and of its 32-row gate|up kernel (G1sq, G1sq4)
// A new quantised stream supplies its kernels, its bytes per weight and its own refusals; the argument checks, the LDS limit, the grid and the
// (row tiles, threads) / phase-length ladders are here.
// The DEVICE bodies the kernels repeat (whole-chunk staging, plane store, phase staging, row scale, gate|up epilogue) are NOT gathered here:
// as force-inlined functions they changed the machine code of every kernel that called them -- the optimiser simplifies a
// callee on its own before it inlines it, so operand orders and what is known about `lane` differ from the code written in place.
#pragma once

// The gate|up epilogue's eight planes (tile q x K half) go through LDS row-major, rows padded to G1S_RP floats: conflict-free both ways.
constexpr int G1S_RP = 36;
constexpr size_t g1s_epilogue_lds(int MT) { return (size_t)8 * 32 * MT * G1S_RP * sizeof(float); }      // (the launchers take the larger of this and the activation arena)

// the four kernel arguments of a folded RMSNorm from the entry points' descriptor (NULL: no norm, the kernels scale by 1)
struct g1s_norm_args {
    const float *ss; int sl; float ih, eps;
    explicit g1s_norm_args(const sjd_row_norm *rn)
        : ss(rn ? rn->sumsq : nullptr), sl(rn ? rn->slices : 0), ih(rn ? 1.0f / (float)rn->hidden : 0.f), eps(rn ? rn->eps : 0.f) {}
};

// The launcher of a quantised stream's whole-chunk kernel (G1q, G1q4) behind sjd_skinny_gemm / sjd_skinny_gemm_cols, which have checked the common
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

// ... and of its 32-row gate|up kernel (G1sq, G1sq4) behind sjd_gateup_silu: M <= 32; the packed weight is [Wg; Wu], 2 I / 32 tiles.
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
