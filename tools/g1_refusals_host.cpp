// Host-side check of the projection entry points' refusals: every call below is refused BEFORE a launch, so the program needs no GPU.  It is meant to be
// compiled together with csrc/sjd_gemm.hip under the host sanitizers, which then watch the dispatch code itself (argument checks, the row-tile fold,
// the column-tile table):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/g1_refusals_host.cpp accelerating-t2i-ar-with-sjd_amd/csrc/sjd_gemm.hip -o /tmp/g1_refusals_host && /tmp/g1_refusals_host
// The expected codes are what the library returned before the launch ladders were gathered (g1_launch_kernel, g1_wide_by_tiles, g1_by_row_tiles).
#include <cstdio>
#include <cstdlib>

#include "../include/sjd_hip.h"

static int failures = 0;

static void expect(const char *what, int got, int want)
{
    std::printf("%-68s %3d%s\n", what, got, got == want ? "" : "   <-- MISMATCH");
    if (got != want) ++failures;
}

int main()
{
    static unsigned short x[16];          // never read: no call gets as far as a launch
    static unsigned char w[16];
    static float out[16], ss[16];
    static int exc[16];
    void *y = out;
    const int BF = SJD_DTYPE_BF16, F16 = SJD_DTYPE_F16, Q8 = SJD_DTYPE_BF16 | SJD_G1_W8_E4M3, BAD = SJD_ERR_BAD_ARG, UNS = SJD_ERR_UNSUPPORTED;
    // sjd_skinny_gemm(x, w, out, M, N, K, KC, waves, step_major, dtype, stream)
    expect("skinny_gemm: null x", sjd_skinny_gemm(nullptr, w, out, 32, 256, 512, 256, 4, 0, BF, nullptr), BAD);
    expect("skinny_gemm: M = 0", sjd_skinny_gemm(x, w, out, 0, 256, 512, 256, 4, 0, BF, nullptr), BAD);
    expect("skinny_gemm: M = 257", sjd_skinny_gemm(x, w, out, 257, 256, 512, 256, 4, 0, BF, nullptr), BAD);
    expect("skinny_gemm: N % 32", sjd_skinny_gemm(x, w, out, 32, 250, 512, 256, 4, 0, BF, nullptr), BAD);
    expect("skinny_gemm: KC % 16", sjd_skinny_gemm(x, w, out, 32, 256, 512, 250, 4, 0, BF, nullptr), BAD);
    expect("skinny_gemm: waves = 0", sjd_skinny_gemm(x, w, out, 32, 256, 512, 256, 0, 0, BF, nullptr), BAD);
    expect("skinny_gemm: waves = 17", sjd_skinny_gemm(x, w, out, 32, 256, 512, 256, 17, 0, BF, nullptr), BAD);
    for (int M : {1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256}) {
        char what[96];
        std::snprintf(what, sizeof what, "skinny_gemm: unknown dtype, M = %d", M);
        expect(what, sjd_skinny_gemm(x, w, out, M, 256, 512, 256, 4, 0, 7, nullptr), UNS);
    }
    expect("skinny_gemm: 32 rows, chunk of 4096 columns (bf16)", sjd_skinny_gemm(x, w, out, 32, 256, 8192, 4096, 4, 0, BF, nullptr), BAD);
    expect("skinny_gemm: 32 rows, chunk of 4096 columns (fp16)", sjd_skinny_gemm(x, w, out, 32, 256, 8192, 4096, 4, 0, F16, nullptr), BAD);
    expect("skinny_gemm: 64 rows, tall chunk, 9 waves (sub-tiled: <= 8)", sjd_skinny_gemm(x, w, out, 64, 256, 8192, 4096, 9, 0, BF, nullptr), BAD);
    expect("skinny_gemm: 65 rows, 9 waves", sjd_skinny_gemm(x, w, out, 65, 256, 512, 256, 9, 0, BF, nullptr), BAD);
    expect("skinny_gemm: 128 rows, 16 waves (fp16)", sjd_skinny_gemm(x, w, out, 128, 256, 512, 256, 16, 0, F16, nullptr), BAD);
    for (int M : {129, 160, 161, 192, 193, 224, 225, 256})
        for (int tiles : {1, 5, 7, 9, 16}) {
            char what[96];
            std::snprintf(what, sizeof what, "skinny_gemm: %d rows, %d column tiles (G1w takes 2 3 4 6 8)", M, tiles);
            expect(what, sjd_skinny_gemm(x, w, out, M, 256, 512, 256, tiles, 0, (M + tiles) % 2 ? BF : F16, nullptr), BAD);
        }
    expect("skinny_gemm (e4m3): fp16", sjd_skinny_gemm(x, w, out, 32, 256, 512, 256, 4, 1, F16 | SJD_G1_W8_E4M3, nullptr), UNS);
    expect("skinny_gemm (e4m3): N = 0", sjd_skinny_gemm(x, w, out, 32, 0, 512, 256, 4, 1, Q8, nullptr), BAD);
    expect("skinny_gemm (e4m3): 32 rows, chunk of 4096 columns", sjd_skinny_gemm(x, w, out, 32, 256, 8192, 4096, 4, 1, Q8, nullptr), UNS);
    expect("skinny_gemm (e4m3): 64 rows, chunk of 2048 columns", sjd_skinny_gemm(x, w, out, 64, 256, 4096, 2048, 4, 1, Q8, nullptr), UNS);
    expect("skinny_gemm (e4m3): 65 rows, two column tiles", sjd_skinny_gemm(x, w, out, 65, 256, 512, 256, 2, 1, Q8, nullptr), UNS);
    expect("skinny_gemm (e4m3): 96 rows, two column tiles", sjd_skinny_gemm(x, w, out, 96, 256, 512, 256, 2, 1, Q8, nullptr), UNS);
    expect("skinny_gemm (e4m3): 129 rows, five column tiles", sjd_skinny_gemm(x, w, out, 129, 256, 512, 256, 5, 1, Q8, nullptr), UNS);
    expect("skinny_gemm (e4m3): 256 rows, K % 32", sjd_skinny_gemm(x, w, out, 256, 256, 528, 256, 4, 1, Q8, nullptr), UNS);
    // sjd_skinny_gemm_cols(x, w, out, M, N, K, KC, waves, step_major, dtype, N_packed, tile0, stream)
    expect("skinny_gemm_cols: null out", sjd_skinny_gemm_cols(x, w, nullptr, 32, 256, 512, 256, 4, 1, BF, 512, 0, nullptr), BAD);
    expect("skinny_gemm_cols: N = 0", sjd_skinny_gemm_cols(x, w, out, 32, 0, 512, 256, 4, 1, BF, 512, 0, nullptr), BAD);
    expect("skinny_gemm_cols: N_packed % 32", sjd_skinny_gemm_cols(x, w, out, 32, 256, 512, 256, 4, 1, BF, 500, 0, nullptr), BAD);
    expect("skinny_gemm_cols: M = 257", sjd_skinny_gemm_cols(x, w, out, 257, 256, 512, 256, 4, 1, BF, 512, 0, nullptr), BAD);
    expect("skinny_gemm_cols: unknown dtype", sjd_skinny_gemm_cols(x, w, out, 32, 256, 512, 256, 4, 1, 9, 512, 0, nullptr), UNS);
    for (int M : {32, 64, 96, 128, 160, 256}) {
        char what[96];
        std::snprintf(what, sizeof what, "skinny_gemm_cols: window past the packed columns, M = %d", M);
        expect(what, sjd_skinny_gemm_cols(x, w, out, M, 256, 512, 256, 4, 1, M % 64 ? BF : F16, 512, 9, nullptr), BAD);
        std::snprintf(what, sizeof what, "skinny_gemm_cols: tile0 = -1, M = %d", M);
        expect(what, sjd_skinny_gemm_cols(x, w, out, M, 256, 512, 256, 4, 1, BF, 512, -1, nullptr), BAD);
    }
    expect("skinny_gemm_cols (e4m3): window past the packed columns", sjd_skinny_gemm_cols(x, w, out, 160, 256, 512, 256, 4, 1, Q8, 512, 9, nullptr), BAD);
    // sjd_skinny_gemm_z(x, wz, exc, exc_cap, out, M, N, K, KC, waves, step_major, dtype, N_packed, tile0, raw, stream)
    expect("skinny_gemm_z: exc_cap = 48", sjd_skinny_gemm_z(x, w, exc, 48, out, 32, 256, 512, 256, 4, 1, BF, 256, 0, nullptr, nullptr), BAD);
    expect("skinny_gemm_z: null exc", sjd_skinny_gemm_z(x, w, nullptr, 32, out, 32, 256, 512, 256, 4, 1, BF, 256, 0, nullptr, nullptr), BAD);
    expect("skinny_gemm_z: waves = 17", sjd_skinny_gemm_z(x, w, exc, 32, out, 32, 256, 512, 256, 17, 1, BF, 256, 0, nullptr, nullptr), BAD);
    expect("skinny_gemm_z: fp16", sjd_skinny_gemm_z(x, w, exc, 32, out, 32, 256, 512, 256, 4, 1, F16, 256, 0, nullptr, nullptr), UNS);
    expect("skinny_gemm_z: M = 129", sjd_skinny_gemm_z(x, w, exc, 32, out, 129, 256, 512, 256, 4, 1, BF, 256, 0, nullptr, nullptr), UNS);
    expect("skinny_gemm_z: KC = 4112", sjd_skinny_gemm_z(x, w, exc, 32, out, 32, 256, 8224, 4112, 4, 1, BF, 256, 0, nullptr, nullptr), UNS);
    expect("skinny_gemm_z: window past the packed columns", sjd_skinny_gemm_z(x, w, exc, 64, out, 32, 256, 512, 256, 4, 1, BF, 256, 1, nullptr, nullptr), BAD);
    expect("skinny_gemm_z: 96 rows, 9 waves", sjd_skinny_gemm_z(x, w, exc, 128, out, 96, 256, 512, 256, 9, 1, BF, 256, 0, nullptr, nullptr), BAD);
    sjd_raw_units bad_raw = {};
    bad_raw.n = 1;
    expect("skinny_gemm_z: raw units without records", sjd_skinny_gemm_z(x, w, exc, 32, out, 32, 256, 512, 256, 4, 1, BF, 256, 0, &bad_raw, nullptr), BAD);
    // sjd_gateup_silu(x, w, y, M, I, K, step_major, dtype, row_norm, stream)
    sjd_row_norm rn = {};
    rn.sumsq = ss; rn.slices = 9; rn.hidden = 4096; rn.eps = 1e-5f;
    expect("gateup_silu: null y", sjd_gateup_silu(x, w, nullptr, 32, 256, 4096, 1, BF, nullptr, nullptr), BAD);
    expect("gateup_silu: I = 32", sjd_gateup_silu(x, w, y, 32, 32, 4096, 1, BF, nullptr, nullptr), BAD);
    expect("gateup_silu: nine slices", sjd_gateup_silu(x, w, y, 32, 256, 4096, 1, BF, &rn, nullptr), UNS);
    expect("gateup_silu: M = 129", sjd_gateup_silu(x, w, y, 129, 256, 4096, 1, BF, nullptr, nullptr), UNS);
    expect("gateup_silu: K = 3072", sjd_gateup_silu(x, w, y, 32, 256, 3072, 1, BF, nullptr, nullptr), UNS);
    expect("gateup_silu: 64 rows at K = 512", sjd_gateup_silu(x, w, y, 64, 256, 512, 1, F16, nullptr, nullptr), UNS);
    expect("gateup_silu: 128 rows at K = 2048", sjd_gateup_silu(x, w, y, 128, 256, 2048, 1, BF, nullptr, nullptr), UNS);
    expect("gateup_silu: unknown dtype", sjd_gateup_silu(x, w, y, 32, 256, 4096, 1, 5, nullptr, nullptr), UNS);
    expect("gateup_silu (e4m3): 33 rows", sjd_gateup_silu(x, w, y, 33, 256, 4096, 1, Q8, nullptr, nullptr), UNS);
    expect("gateup_silu (e4m3): fp16", sjd_gateup_silu(x, w, y, 32, 256, 4096, 1, F16 | SJD_G1_W8_E4M3, nullptr, nullptr), UNS);
    // sjd_gateup_silu_z(x, wz, exc, exc_cap, y, M, I, K, step_major, dtype, row_norm, raw, stream)
    expect("gateup_silu_z: exc_cap = 16", sjd_gateup_silu_z(x, w, exc, 16, y, 32, 256, 4096, 1, BF, nullptr, nullptr, nullptr), BAD);
    expect("gateup_silu_z: raw units without records", sjd_gateup_silu_z(x, w, exc, 32, y, 32, 256, 4096, 1, BF, nullptr, &bad_raw, nullptr), BAD);
    expect("gateup_silu_z: nine slices", sjd_gateup_silu_z(x, w, exc, 32, y, 32, 256, 4096, 1, BF, &rn, nullptr, nullptr), UNS);
    expect("gateup_silu_z: M = 65", sjd_gateup_silu_z(x, w, exc, 32, y, 65, 256, 4096, 1, BF, nullptr, nullptr, nullptr), UNS);
    expect("gateup_silu_z: fp16", sjd_gateup_silu_z(x, w, exc, 32, y, 32, 256, 4096, 1, F16, nullptr, nullptr, nullptr), UNS);
    expect("gateup_silu_z: 64 rows at K = 512", sjd_gateup_silu_z(x, w, exc, 128, y, 64, 256, 512, 1, BF, nullptr, nullptr, nullptr), UNS);
    std::printf("%s: %d mismatch(es)\n", failures ? "FAILED" : "ok", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
