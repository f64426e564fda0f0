// sjd_attention.hip -- K1 draft-window attention + K3 KV append for gfx950 (CDNA4, wave64, MFMA 16x16x32).
//
// Data layout in HBM:  K/V cache per layer [B, H_kv, S_max, D] (one contiguous D-row per key, 256 B at D=128 bf16);
// q / out [B, n_rows, H, D] (the q_proj / o_proj activation layout, no transposes).
//
// K1 structure (memory-bound: intensity = L*H/H_kv flop/byte << ridge, judged on HBM GB/s):
//   grid = (n_chunks * n_split, H_kv, B), 256 threads = 4 wave64.
//   A workgroup owns one (batch, kv-head, 16-row query chunk, key split).  Wave w works for q-head (w % G) of the
//   kv-group (G = H/H_kv in {1,2,4}) on key tiles (w / G) + k * (4/G) of 32 keys.
//   Per 32-key tile and wave:
//     S^T = K Q^T   : 2 x (D/32) MFMA 16x16x32;  A operand = K rows loaded STRAIGHT from HBM in fragment layout
//                     (lane = key, 16 B = 8 consecutive d);  B operand = Q (kept in registers for the whole kernel).
//                     The "swapped" product puts a whole query row's scores in one lane column, so running max / sum /
//                     rescale are per-lane scalars + two xor-shuffles (16, 32).
//     O^T += V^T P^T: D/16 MFMA; B operand = P^T taken from the S^T accumulator registers as-is (the key permutation
//                     this implies is applied to the V operand instead, so P never goes through LDS);
//                     A operand = V^T via ds_read_b64_tr_b16 from a per-wave LDS tile filled with coalesced 16-B loads.
//   Next tile's K and V loads are issued before the current tile's math (register double buffer).
//   Split partials (m, l, O) go to an fp32 workspace; k1_combine merges them and writes bf16/f16.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <math.h>

#include "../../include/sjd_hip.h"
#include "sjd_coherent.h"
#include "sjd_switches.h"
#include "sjd_fp8.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

#define K1_WAVES 4
// Phase timestamps (tools/phase_trace.py builds with -DSJD_TRACE; compiled out otherwise): thread 0 of every workgroup records the
// 100 MHz wall clock at the phase boundaries of k1_partial.  This is how the 5.3 us merge epilogue and the serialised second key tile
// were found in round 2.
#ifdef SJD_TRACE
__device__ unsigned long long g_k1_trace[4096][8];
__device__ unsigned long long g_k1c_trace[4096][4];
#define SJD_TRC(i) do { if (threadIdx.x == 0) g_k1c_trace[((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) & 4095][i] = wall_clock64(); } while (0)
#define SJD_TR(i) do { if (threadIdx.x == 0) g_k1_trace[((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) & 4095][i] = wall_clock64(); } while (0)
#else
#define SJD_TR(i) do { } while (0)
#define SJD_TRC(i) do { } while (0)
#endif
#define K1_KT 32          // keys per wave tile
#define K1_ROWS 16        // query rows per chunk
#define K1_RPAD 4          // fp32 padding of a merge-buffer row: rows 16 banks apart instead of on the same bank
#define K1_MIN_TILES_PER_SPLIT 4   // a key split is only opened when it gets at least one tile per wave

// What an attention kernel of the window forward needs before it can compute a single address: kv_len / n_rows of its batch row (device
// blob) and the row's first visible key.  ONE scalar round trip: the three loads are issued together, as instructions (sjdi_kv_rows in
// the header explains why), at the top of the kernel next to the loads of the kernel arguments that did not fit the SGPR preload.
// Before: arguments -> batch_rows -> kv_len -> key_start, each waiting for the one before (ISA, late round 2).
__device__ __forceinline__ void k1_entry(const sjd_iter_params *params, const int *key_start, int b, int kv_len_arg, int n_rows_arg,
                                         int &kv_base, int &n_total, int &kstart)
{
    if (!params) {
        kv_base = kv_len_arg; n_total = n_rows_arg; kstart = key_start ? key_start[b] : 0;
        return;
    }
    const int *ksp = key_start ? key_start + b : reinterpret_cast<const int *>(params);        // (always a readable address)
    // both addresses are wave-uniform (kernel arguments and blockIdx); readfirstlane states it, so that the "s" operands below never
    // depend on what the uniformity analysis makes of the surrounding code (the -DSJD_TRACE build had the pointer in VGPRs)
    const unsigned long long pa = sjdi_uniform_u64(reinterpret_cast<unsigned long long>(params));
    const unsigned long long ka = sjdi_uniform_u64(reinterpret_cast<unsigned long long>(ksp));
    unsigned long long nk;
    int br, ks;
    __asm__ volatile("s_load_dwordx2 %0, %3, 0x0\n\ts_load_dword %1, %3, 0x14\n\ts_load_dword %2, %4, 0x0\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(nk), "=&s"(br), "=&s"(ks) : "s"(pa), "s"(ka) : "memory");
    kstart = key_start ? ks : 0;
    const int blob = br > 0 ? b / br : 0;
    if (blob == 0) { n_total = (int)(unsigned)(nk & 0xffffffffull); kv_base = (int)(unsigned)(nk >> 32); }
    else { kv_base = params[blob].kv_len; n_total = params[blob].n_rows; }
}

// Key-tile range [t_lo, t_hi) of a (batch row, chunk) and the number of splits actually used for it.  The launch grid
// is sized for n_split (static, hipGraph friendly); splits >= the effective count exit immediately and are skipped by
// the combine kernel, so short contexts do not pay for empty partials.
__device__ __forceinline__ void k1_tile_range(int kstart, int total, int n_split, int &t_lo, int &t_hi, int &eff_split, int &tps)
{
    t_lo = kstart / K1_KT;
    t_hi = (total + K1_KT - 1) / K1_KT;
    const int nt = max(t_hi - t_lo, 0);
    eff_split = min(n_split, max(1, (nt + K1_MIN_TILES_PER_SPLIT - 1) / K1_MIN_TILES_PER_SPLIT));
    tps = (nt + eff_split - 1) / eff_split;
    // no EMPTY split below the effective count: with tps rounded up the last splits may get no tile (129 tiles over 16 splits: 9 each, the
    // sixteenth none), and a kernel that skips its empty split would leave a partial the combine merges unwritten (round 4: found with the
    // allocator's free pool poisoned -- a fresh process reads zero pages there, which merge as a harmless (m = 0, l = 0) term)
    if (tps > 0) eff_split = (nt + tps - 1) / tps;
}

// the (m, l, O) of a split that saw no key: -inf, 0, zeros (O must be DEFINED: the merge multiplies it by exp(-inf) = 0).  Only the case of no
// visible key at all (eff_split == 1 with no tile: rows hidden in front of key_start) still reaches it.
template <int D>
__device__ __forceinline__ void k1_store_empty_partial(float *__restrict__ ws_o, float *__restrict__ ws_ml, size_t slot0, int c, int g)
{
#pragma unroll
    for (int db = 0; db < D / 16; ++db) *reinterpret_cast<f32x4 *>(ws_o + (slot0 + c) * D + 16 * db + 4 * g) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (g == 0) { ws_ml[(slot0 + c) * 2] = -INFINITY; ws_ml[(slot0 + c) * 2 + 1] = 0.f; }
}

template <int DT> struct Frag;
template <> struct Frag<SJD_DTYPE_BF16> {
    typedef bf16x8 vec;
    static __device__ __forceinline__ f32x4 mfma(vec a, vec b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ unsigned short cvt(float x)
    {   // round-to-nearest-even fp32 -> bf16 (v_cvt_pk_bf16_f32 on gfx950)
        const __bf16 h = (__bf16)x;
        return __builtin_bit_cast(unsigned short, h);
    }
};
template <> struct Frag<SJD_DTYPE_F16> {
    typedef f16x8 vec;
    static __device__ __forceinline__ f32x4 mfma(vec a, vec b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ unsigned short cvt(float x)
    {
        _Float16 h = (_Float16)x;
        return *reinterpret_cast<unsigned short *>(&h);
    }
};

template <typename V> __device__ __forceinline__ V as_frag(u32x4 x) { return __builtin_bit_cast(V, x); }

// two fp32 -> one dword of two 16-bit values (a in the low half), round-to-nearest-even: ONE v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32 instead of two
// conversions, a shift and an or -- the same bits as Frag<DT>::cvt of each
template <int DT> __device__ __forceinline__ unsigned k1_cvt_pk(float a, float b);
template <> __device__ __forceinline__ unsigned k1_cvt_pk<SJD_DTYPE_BF16>(float a, float b)
{
    typedef __attribute__((ext_vector_type(2))) float f32x2_;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_;
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_{a, b}), bf16x2_));
}
template <> __device__ __forceinline__ unsigned k1_cvt_pk<SJD_DTYPE_F16>(float a, float b)
{
    typedef __attribute__((ext_vector_type(2))) float f32x2_;
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_;
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_{a, b}), f16x2_));
}

// transpose read: the 16 lanes of a group fetch a [4 keys][16 d] block (lane i: 8 bytes at row i/4, cols 4*(i%4)..+3)
// and lane c receives column c (4 keys).
__device__ __forceinline__ u32x2 lds_tr_read(const unsigned short *p)
{
    typedef __attribute__((ext_vector_type(4))) short s16x4;
    s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(p));
    return __builtin_bit_cast(u32x2, r);
}

// Epilogue of k1_partial / k1_partial_fp8: merge the key-part states (m, l, O) of every head of the workgroup, which the waves have
// written to LDS, and publish the result -- the split partial (fp32 workspace) or, with ONE key split, the normalised 16-bit output.
// One thread per four output columns; its 8 (m, l) pairs and 8 O quads are read from LDS up front (16 independent reads, one round
// trip), then max / exp / weighted sums in key-part order.  In-kernel timestamps (round 2): the earlier form -- one element per thread,
// ~50 DEPENDENT LDS reads, rows of the buffer all on one bank -- took 5.3 us of a 14.6 us launch (3.6 us of them bank-conflicted writes
// and the dependent chain); this one 0.5 us + 0.5 us for the writes.
// Round 3: with `merge_out` the key SPLITS of a (batch, kv head, chunk) are merged here too, by whichever of their workgroups finishes
// LAST -- k1_combine, until now a graph node of its own behind every k1_partial (5.1 us + the node boundary), is gone for the
// multi-head window.  A workgroup publishes its partial with device-coherent (sc1) stores, waits for their acknowledgement and takes a
// ticket; the holder of the last ticket reads all partials back with device-coherent loads (one round trip: every split in flight) and
// runs k1_combine's arithmetic in split order -- the output bits are those of k1_partial + k1_combine.  Nobody waits for anybody (no
// spin, no residency assumption); the ticket re-arms itself.  One effective split (short contexts): the direct output, no exchange.
// one step of the online merge of split partials (m, l, O[N]) into (M, L, acc[N]) -- shared by k1_combine and by the in-kernel merge of
// k1_partial, written with explicit fma so that both give the same bits whatever the instruction selector makes of the code around it
template <int N>
__device__ __forceinline__ void k1_merge_step(float &M, float &L, float (&acc)[N], float m, float l, const float (&o)[N])
{
    const float Mn = fmaxf(M, m);
    const float Msafe = (Mn == -INFINITY) ? 0.0f : Mn;
    const float w0 = __expf(M - Msafe), w1 = __expf(m - Msafe);
    L = __builtin_fmaf(L, w0, l * w1);
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = __builtin_fmaf(acc[j], w0, o[j] * w1);
    M = Mn;
}

template <int DT, int D>
__device__ __forceinline__ void k1_merge_splits(const float *__restrict__ ws_o, const float *__restrict__ ws_ml, unsigned short *__restrict__ out,
                                                int G, int b, int H, int head0, int n_chunks, int chunk, int n_split, int eff_split,
                                                int row0, int n_rows, int n_total, int nthreads)
{
    constexpr int D4 = D / 4, CB = 8;
    for (int u = threadIdx.x; u < G * K1_ROWS * D4; u += nthreads) {
        const int hg = u / (K1_ROWS * D4), row = (u / D4) % K1_ROWS, d = (u % D4) * 4;
        const int grow = row0 + row;
        if (grow >= n_rows) continue;
        unsigned short *o = out + (((size_t)b * n_rows + grow) * H + (head0 + hg)) * D + d;
        if (grow >= n_total) { *reinterpret_cast<uint2 *>(o) = uint2{0u, 0u}; continue; }     // padding rows: defined (zero) output
        const size_t base = ((((size_t)b * H + (head0 + hg)) * n_chunks + chunk) * n_split) * K1_ROWS + row;
        float M = -INFINITY, L = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < eff_split; s0 += CB) {
            sjd_f4 ov[CB];
            sjd_f2 mv[CB];
#pragma unroll
            for (int q = 0; q < CB; ++q) {                         // every split of the batch in flight, then merged in split order;
                const size_t slot = base + (size_t)min(s0 + q, eff_split - 1) * K1_ROWS;      // unconditional (clamped) loads: counted waits
                ov[q] = sjd_ld_coherent_f4(ws_o + slot * D + d);
                mv[q] = sjd_ld_coherent_f2(ws_ml + slot * 2);
            }
#pragma unroll
            for (int q = 0; q < CB; ++q)
                if (s0 + q < eff_split) {                          // k1_combine's online merge, split order
                    const float ov4[4] = {ov[q].x, ov[q].y, ov[q].z, ov[q].w};
                    k1_merge_step<4>(M, L, acc, mv[q].x, mv[q].y, ov4);
                }
        }
        const float inv = L > 0.f ? 1.0f / L : 0.0f;
        uint2 pk;
        pk.x = (unsigned)Frag<DT>::cvt(acc[0] * inv) | ((unsigned)Frag<DT>::cvt(acc[1] * inv) << 16);
        pk.y = (unsigned)Frag<DT>::cvt(acc[2] * inv) | ((unsigned)Frag<DT>::cvt(acc[3] * inv) << 16);
        *reinterpret_cast<uint2 *>(o) = pk;
    }
}

template <int DT, int D, int NW>
__device__ __forceinline__ void k1_merge_publish(float (*red_o)[K1_ROWS][D + K1_RPAD], float (*red_ml)[K1_ROWS][2], int G, int kparts,
                                                 int b, int H, int head0, int n_chunks, int chunk, int n_split, int split, int row0, int n_rows,
                                                 int n_total, float *__restrict__ ws_o, float *__restrict__ ws_ml,
                                                 unsigned short *__restrict__ out_direct, unsigned short *__restrict__ merge_out = nullptr,
                                                 unsigned *__restrict__ ticket = nullptr, int eff_split = 0)
{
    constexpr int D4 = D / 4;
#ifndef SJD_EXPERIMENTAL      // (the in-kernel split merge is an experiment: libsjd_hip_exp.so -- the product kernels are compiled without it)
    merge_out = nullptr;
    ticket = nullptr;
#endif
    const bool merged = merge_out != nullptr;
    if (merged && eff_split == 1) out_direct = merge_out;          // one split in effect: this workgroup's state IS the result
    const bool coherent = merged && !out_direct;
    for (int u = threadIdx.x; u < G * K1_ROWS * D4; u += 64 * NW) {
        const int hg = u / (K1_ROWS * D4), row = (u / D4) % K1_ROWS, d = (u % D4) * 4;
        float mk[NW], lk[NW];
        float4 ok[NW];
#pragma unroll
        for (int kp = 0; kp < NW; ++kp) {                      // every LDS read of this thread is issued before the first use
            const bool on = kp < kparts;
            const int ww = on ? kp * G + hg : hg;
            const float2 v = *reinterpret_cast<const float2 *>(&red_ml[ww][row][0]);
            ok[kp] = *reinterpret_cast<const float4 *>(&red_o[ww][row][d]);
            mk[kp] = on ? v.x : -INFINITY;
            lk[kp] = v.y;
        }
        float M = -INFINITY;
#pragma unroll
        for (int kp = 0; kp < NW; ++kp) M = fmaxf(M, mk[kp]);
        const float Ms = (M == -INFINITY) ? 0.0f : M;
        float L = 0.f, O0 = 0.f, O1 = 0.f, O2 = 0.f, O3 = 0.f;
#pragma unroll
        for (int kp = 0; kp < NW; ++kp)
            if (kp < kparts) {
                const float wgt = __expf(mk[kp] - Ms);
                L += wgt * lk[kp];
                O0 += wgt * ok[kp].x; O1 += wgt * ok[kp].y; O2 += wgt * ok[kp].z; O3 += wgt * ok[kp].w;
            }
        if (out_direct) {
            // one key split (n_split == 1): this IS the attention output -- exactly what k1_combine makes of a single partial
            // (acc = 0 * exp(-inf) + O * exp(0), L likewise), written without the workspace round trip and the second launch
            const int grow = row0 + row;
            if (grow < n_rows) {
                const float inv = L > 0.f ? 1.0f / L : 0.0f;
                uint2 pk{0u, 0u};
                if (grow < n_total) {
                    pk.x = (unsigned)Frag<DT>::cvt(O0 * inv) | ((unsigned)Frag<DT>::cvt(O1 * inv) << 16);
                    pk.y = (unsigned)Frag<DT>::cvt(O2 * inv) | ((unsigned)Frag<DT>::cvt(O3 * inv) << 16);
                }
                *reinterpret_cast<uint2 *>(out_direct + (((size_t)b * n_rows + grow) * H + (head0 + hg)) * D + d) = pk;
            }
            continue;
        }
        const size_t slot = ((((size_t)b * H + (head0 + hg)) * n_chunks + chunk) * n_split + split) * K1_ROWS + row;
        if (coherent) {
            sjd_st_coherent_f4(ws_o + slot * D + d, O0, O1, O2, O3);
            if (d == 0) sjd_st_coherent_f2(ws_ml + slot * 2, M, L);
        } else {
            *reinterpret_cast<float4 *>(ws_o + slot * D + d) = float4{O0, O1, O2, O3};
            if (d == 0) { ws_ml[slot * 2] = M; ws_ml[slot * 2 + 1] = L; }
        }
    }
    if (!coherent) return;
    __shared__ unsigned last_s;
    __builtin_amdgcn_s_waitcnt(0x0F70);                            // vmcnt(0): this thread's partial is acknowledged (written through L2)
    __syncthreads();
    unsigned *tk = ticket + ((size_t)b * (H / G) + head0 / G) * n_chunks + chunk;
    if (threadIdx.x == 0) last_s = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (last_s != (unsigned)(eff_split - 1)) return;             // somebody else finishes later and merges
    if (threadIdx.x == 0) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // re-armed for the next launch
    k1_merge_splits<DT, D>(ws_o, ws_ml, merge_out, G, b, H, head0, n_chunks, chunk, n_split, eff_split, row0, n_rows, n_total, 64 * NW);
}

// NW wave64 per workgroup (4, or 8 for two waves per SIMD: twice the key tiles in flight per CU; the key-parts are merged in LDS)
// DL: the LOGICAL head dim of the softmax scale (SJD_K1_HEAD_DIM_100: heads stored D = 128 wide with zero pad columns, scale 1/sqrt(100))
template <int DT, int D, int NW, int DL = D>
__global__ __launch_bounds__(64 * NW) void k1_partial(
    const unsigned short *__restrict__ q, const unsigned short *__restrict__ kc, const unsigned short *__restrict__ vc,
    const sjd_iter_params *__restrict__ params, const int *__restrict__ key_start,        // (among the first 16 dwords: preloaded into SGPRs)
    float *__restrict__ ws_o, float *__restrict__ ws_ml, unsigned short *__restrict__ out_direct,   // (the pointer before the ints: no padding
    int n_rows, int H, int H_kv, int S_max, int kv_len_arg, int n_split, int n_chunks,              //  dword in the scalar load of the rest)
    unsigned short *__restrict__ merge_out = nullptr, unsigned *__restrict__ ticket = nullptr)
{
    typedef typename Frag<DT>::vec vec;
    constexpr int KS = D / 32;            // k-steps of the QK^T product
    constexpr int DB = D / 16;            // 16-wide d blocks of the output
    constexpr int VROW = D + 8;           // padded LDS row (elements): 16-B aligned rows, breaks the 256-B bank period
    // one LDS arena: the per-wave V tiles during the key loop, then (after a barrier) the fp32 merge buffers of the epilogue;
    // aliasing them keeps the workgroup at ~35 KB so that four workgroups fit on a CU
    constexpr int V_BYTES = NW * K1_KT * VROW * 2;
    constexpr int R_BYTES = NW * K1_ROWS * (D + K1_RPAD + 2) * 4;
    __shared__ __attribute__((aligned(16))) unsigned char arena[V_BYTES > R_BYTES ? V_BYTES : R_BYTES];
    unsigned short (*v_lds)[K1_KT * VROW] = reinterpret_cast<unsigned short (*)[K1_KT * VROW]>(arena);
    float (*red_o)[K1_ROWS][D + K1_RPAD] = reinterpret_cast<float (*)[K1_ROWS][D + K1_RPAD]>(arena);
    float (*red_ml)[K1_ROWS][2] = reinterpret_cast<float (*)[K1_ROWS][2]>(arena + NW * K1_ROWS * (D + K1_RPAD) * 4);

    SJD_TR(0);                    // entry
    int kv_base, n_total, kstart;                                 // valid rows of this call, first visible key: one scalar round trip
    k1_entry(params, key_start, blockIdx.z, kv_len_arg, n_rows, kv_base, n_total, kstart);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int G = H / H_kv;
    const int kparts = NW / G;
    const int head_in_group = w % G, kpart = w / G;
    const int chunk = blockIdx.x / n_split, split = blockIdx.x % n_split;
    const int hkv = blockIdx.y, b = blockIdx.z;
    const int head = hkv * G + head_in_group;

    const int row0 = chunk * K1_ROWS;
    const int n_c = min(K1_ROWS, n_total - row0);                 // may be <= 0 for padding chunks
    const int kv_len = kv_base + row0;                            // keys < kv_len are visible to every row of the chunk
    const int total = kv_len + max(n_c, 0);                       // keys >= total are not visible to any row
    const float scale = rsqrtf((float)DL);

    // tile range of this workgroup / wave
    int t_lo, t_hi, eff_split, tps;
    k1_tile_range(kstart, total, n_split, t_lo, t_hi, eff_split, tps);
    if (split >= eff_split) return;
    const int t_begin = t_lo + split * tps, t_end = min(t_hi, t_begin + tps);
    SJD_TR(1);                    // kv_len / key_start known

    // Q fragments (B operand): lane (row c, group g) holds Q[row0+c][head][32*ks + 8g .. +7]
    vec qf[KS];
    {
        const bool rv = (c < n_c);
        const unsigned short *qp = q + (((size_t)b * n_rows + (row0 + (rv ? c : 0))) * H + head) * D + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4 x = rv ? *reinterpret_cast<const u32x4 *>(qp + 32 * ks) : u32x4{0, 0, 0, 0};
            qf[ks] = as_frag<vec>(x);
        }
    }
    const unsigned short *kbase = kc + ((size_t)b * H_kv + hkv) * (size_t)S_max * D;
    const unsigned short *vbase = vc + ((size_t)b * H_kv + hkv) * (size_t)S_max * D;

    float m_run = -INFINITY, l_run = 0.0f;
    f32x4 o_acc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) o_acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 kreg[2][KS], kn[2][KS];
    u32x4 vstage[K1_KT * D / (64 * 8)];       // 16-B pieces per lane for one V tile
    constexpr int VP = K1_KT * D / (64 * 8);
    constexpr int LPR = D / 8;                // lanes per V row
    unsigned short *vl = v_lds[w];

    auto load_tile = [&](int t, u32x4 (&kd)[2][KS], u32x4 (&vd)[VP]) {
        const unsigned short *kt = kbase + (size_t)(t * K1_KT) * D;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                kd[kb][ks] = *reinterpret_cast<const u32x4 *>(kt + (size_t)(16 * kb + c) * D + 32 * ks + 8 * g);
        const unsigned short *vt = vbase + (size_t)(t * K1_KT) * D;
#pragma unroll
        for (int i = 0; i < VP; ++i) {
            int idx = i * 64 + lane;
            vd[i] = *reinterpret_cast<const u32x4 *>(vt + (size_t)(idx / LPR) * D + 8 * (idx % LPR));
        }
    };
    // V rows of keys >= total are never visible (p = 0) but 0 * NaN = NaN inside the MFMA: rows beyond the valid cache length
    // (padding rows of a shape-static window, stale data) are therefore zeroed while staging.
    auto store_v = [&](int t, u32x4 (&vd)[VP]) {
#pragma unroll
        for (int i = 0; i < VP; ++i) {
            int idx = i * 64 + lane;
            const bool live = (t * K1_KT + idx / LPR) < total;
            *reinterpret_cast<u32x4 *>(vl + (idx / LPR) * VROW + 8 * (idx % LPR)) = live ? vd[i] : u32x4{0u, 0u, 0u, 0u};
        }
    };

    // Two tiles of a wave are in flight before the first one is waited for (in-kernel timestamps, round 2: with one tile in flight a
    // wave that owns two or three tiles pays 3.4 us of HBM latency for each of them).
    u32x4 vstage2[VP];
    auto compute_tile = [&](int t) {

        // ---- S^T = K Q^T for the two 16-key blocks
        f32x4 st[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            st[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) st[kb] = Frag<DT>::mfma(as_frag<vec>(kreg[kb][ks]), qf[ks], st[kb]);
        }
        // ---- mask + online softmax (query row = c; this lane holds keys 16kb + 4g + r)
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int key = t * K1_KT + 16 * kb + 4 * g + r;
                bool vis = (key >= kstart) && (key <= kv_len + c) && (key < total);
                float s = vis ? st[kb][r] * scale : -INFINITY;
                st[kb][r] = s;
                mx = fmaxf(mx, s);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float m_safe = (m_new == -INFINITY) ? 0.0f : m_new;
        const float alpha = __expf(m_run - m_safe);
        float rs = 0.0f;
        unsigned short pb[8];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float pv = __expf(st[kb][r] - m_safe);
                rs += pv;
                pb[4 * kb + r] = Frag<DT>::cvt(pv);
            }
        rs += __shfl_xor(rs, 16);
        rs += __shfl_xor(rs, 32);
        l_run = l_run * alpha + rs;
        m_run = m_new;
        u32x4 pw;
        pw[0] = pb[0] | ((unsigned)pb[1] << 16);
        pw[1] = pb[2] | ((unsigned)pb[3] << 16);
        pw[2] = pb[4] | ((unsigned)pb[5] << 16);
        pw[3] = pb[6] | ((unsigned)pb[7] << 16);
        const vec pfrag = as_frag<vec>(pw);
        // ---- O^T = alpha * O^T + V^T P^T
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const unsigned short *a0 = vl + (4 * g + (c >> 2)) * VROW + 16 * db + 4 * (c & 3);
            u32x2 lo = lds_tr_read(a0);
            u32x2 hi = lds_tr_read(a0 + 16 * VROW);
            u32x4 vv{lo[0], lo[1], hi[0], hi[1]};
            f32x4 acc = o_acc[db];
            acc[0] *= alpha; acc[1] *= alpha; acc[2] *= alpha; acc[3] *= alpha;
            o_acc[db] = Frag<DT>::mfma(as_frag<vec>(vv), pfrag, acc);
        }
    };
    auto adopt_next = [&](int tn, u32x4 (&vd)[VP]) {
        store_v(tn, vd);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kreg[kb][ks] = kn[kb][ks];
    };
    int t = t_begin + kpart;
    if (t < t_end) {
        load_tile(t, kreg, vstage);
        if (t + kparts < t_end) {
            load_tile(t + kparts, kn, vstage2);
            store_v(t, vstage);
            SJD_TR(2);            // first tile arrived
            compute_tile(t);
            adopt_next(t + kparts, vstage2);
            t += kparts;
        } else {
            store_v(t, vstage);
            SJD_TR(2);
        }
    }
    for (; t < t_end; t += kparts) {
        const int tn = t + kparts;
        const bool has_next = tn < t_end;
        if (has_next) load_tile(tn, kn, vstage);
        compute_tile(t);
        if (has_next) adopt_next(tn, vstage);
    }

    SJD_TR(3);                    // key loop done
    // ---- merge the key-parts of each head inside the workgroup, then publish the split partial
    __syncthreads();
    SJD_TR(4);                    // all waves done            // every wave is done with its V tile: the arena is reused for the merge buffers
    if (g == 0) { red_ml[w][c][0] = m_run; red_ml[w][c][1] = l_run; }
#pragma unroll
    for (int db = 0; db < DB; ++db) *reinterpret_cast<f32x4 *>(&red_o[w][c][16 * db + 4 * g]) = o_acc[db];
    __syncthreads();
    SJD_TR(5);                    // merge buffers written
    k1_merge_publish<DT, D, NW>(red_o, red_ml, G, kparts, b, H, hkv * G, n_chunks, chunk, n_split, split, row0, n_rows, n_total, ws_o, ws_ml,
                                out_direct, merge_out, ticket, eff_split);
#ifdef SJD_TRACE
    SJD_TR(6);                    // merged, stores issued
    __builtin_amdgcn_s_waitcnt(0x0F70);
    SJD_TR(7);                    // stores acknowledged
#endif
}

#ifdef SJD_EXPERIMENTAL        // the round-3 shared-tile kernel (replaced by the ring kernel; SJD_K1_RING=0, sjd_switches.h): libsjd_hip_exp.so only
// ------------------------------------------------------------------------------------------------ K1 (shared tiles)
// Grouped-query attention and/or several 16-row chunks (Emu3: H/H_kv = 4, draft window 32): in k1_partial every (head, chunk) pair
// streams the same K/V tiles by itself, 8 times the bytes through L2/L1.  Here ONE workgroup owns a (batch, kv head, key split) and
// all its (head, chunk) pairs -- one wave each, up to 8 -- and the 32-key K and V tiles are fetched once per workgroup into a
// double-buffered LDS tile (K rows padded to 272 B: the fragment read "lane = key, 16 B" is conflict free; V as in k1_partial,
// read back transposed).  The next tile's loads are in flight while the current one is consumed; one barrier per tile.
// Same split / workspace layout as k1_partial (the waves of a pair cover all tiles of the split, so no LDS merge), k1_combine
// is unchanged.
// NSET key tiles travel at a time: 3.  Six (a register set is only 2 * MAXP 16-byte pieces) measured EQUAL in round 3
// -- 17.2 / 26.4 / 36.7 us per layer at kv 1024 / 4096 / 8192 against 16.9 / 25.5 / 36.3 (Emu3 shape, 16 splits, with k1_combine) -- so
// the bytes in flight are not what bounds this kernel: a tile costs 1.4-1.9 us whatever travels behind it (LDS fragment reads of eight
// waves, the dependent QK^T -> softmax -> PV chain of each, one workgroup barrier), profiles/r3_k1_microbench.jsonl.
template <int DT, int D, int NWV, int NSET = 3>          // NWV = waves per workgroup = (q head of the group, row chunk) pairs: 4 or 8
__global__ __launch_bounds__(64 * NWV) void k1_partial_shared(
    const unsigned short *__restrict__ q, const unsigned short *__restrict__ kc, const unsigned short *__restrict__ vc,
    const sjd_iter_params *__restrict__ params, const int *__restrict__ key_start,        // (among the first 16 dwords: preloaded into SGPRs)
    float *__restrict__ ws_o, float *__restrict__ ws_ml, int n_rows, int H, int H_kv, int S_max, int kv_len_arg, int n_split, int n_chunks)
{
    typedef typename Frag<DT>::vec vec;
    constexpr int KS = D / 32, DB = D / 16;
    constexpr int ROW = D + 8;                // padded LDS row (elements) for both tiles
    SJD_TR(0);
    constexpr int TILE = K1_KT * ROW;         // elements per K or V tile
    __shared__ __attribute__((aligned(16))) unsigned short tiles[2][2][TILE];     // [buffer][K, V]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int G = H / H_kv;
    const int head_in_group = w % G, chunk = w / G;           // wave = (q head of the group, 16-row chunk)
    const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
    const int head = hkv * G + head_in_group;
    int kv_base, n_total, kstart;
    k1_entry(params, key_start, b, kv_len_arg, n_rows, kv_base, n_total, kstart);
    const float scale = rsqrtf((float)D);

    // this wave's rows and tile range (identical to what k1_partial / k1_combine derive for its chunk)
    const int row0 = chunk * K1_ROWS;
    const int n_c = min(K1_ROWS, n_total - row0);
    const int kv_len = kv_base + row0;
    const int total = kv_len + max(n_c, 0);
    int t_lo, t_hi, eff_split, tps;
    k1_tile_range(kstart, total, n_split, t_lo, t_hi, eff_split, tps);
    const bool wave_on = split < eff_split;
    const int wt0 = wave_on ? t_lo + split * tps : 0, wt1 = wave_on ? min(t_hi, wt0 + tps) : 0;
    // the workgroup walks the union of its waves' ranges (they differ by at most a tile between the chunks)
    int bt0 = 1 << 30, bt1 = 0, total_max = 0;
    for (int ch = 0; ch < n_chunks; ++ch) {
        const int nc = min(K1_ROWS, n_total - ch * K1_ROWS), tot = kv_base + ch * K1_ROWS + max(nc, 0);
        int a, e, es, tp;
        k1_tile_range(kstart, tot, n_split, a, e, es, tp);
        if (split < es) { bt0 = min(bt0, a + split * tp); bt1 = max(bt1, min(e, a + split * tp + tp)); }
        total_max = max(total_max, tot);
    }
    if (bt1 <= bt0) {                         // no wave of this workgroup has a tile in this split
        if (wave_on) k1_store_empty_partial<D>(ws_o, ws_ml, ((((size_t)b * H + head) * n_chunks + chunk) * n_split + split) * K1_ROWS, c, g);
        return;
    }
    SJD_TR(1);                    // tile ranges known

    vec qf[KS];
    {
        const bool rv = (c < n_c);
        const unsigned short *qp = q + (((size_t)b * n_rows + (row0 + (rv ? c : 0))) * H + head) * D + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4 x = rv ? *reinterpret_cast<const u32x4 *>(qp + 32 * ks) : u32x4{0, 0, 0, 0};
            qf[ks] = as_frag<vec>(x);
        }
    }
    const unsigned short *kbase = kc + ((size_t)b * H_kv + hkv) * (size_t)S_max * D;
    const unsigned short *vbase = vc + ((size_t)b * H_kv + hkv) * (size_t)S_max * D;

    // cooperative tile fetch: K1_KT * D / 8 16-byte pieces per tensor, spread over the workgroup.  THREE tiles travel at a time, in three
    // register sets that rotate without copies (tile r of the workgroup's range lives in set r % 3); every load is unconditional (the
    // tile index is clamped), so the compiler's vmcnt at a stash leaves the two younger tiles in flight.  With one tile ahead a
    // workgroup moved 16 KB per HBM round trip: 1.1 TB/s at kv_len 4096 (round 2, 31 us per layer).
    constexpr int PIECES = K1_KT * D / 8, LPR = D / 8;
    constexpr int MAXP = PIECES / (64 * NWV);  // pieces per thread and tensor
    static_assert(MAXP * 64 * NWV == PIECES, "the workgroup covers a tile exactly");
    u32x4 kst[NSET][MAXP], vst[NSET][MAXP];
    auto fetch = [&](int t, auto set) {
        constexpr int S = decltype(set)::value;
        const int tc = min(t, bt1 - 1);
#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            const int idx = i * (64 * NWV) + (int)threadIdx.x;
            const size_t off = (size_t)(tc * K1_KT + idx / LPR) * D + 8 * (idx % LPR);
            kst[S][i] = *reinterpret_cast<const u32x4 *>(kbase + off);
            vst[S][i] = *reinterpret_cast<const u32x4 *>(vbase + off);
        }
    };
    auto stash = [&](int t, int buf, auto set) {        // rows of keys >= total_max are zeroed (0 * NaN inside the MFMA, see k1_partial)
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            const int idx = i * (64 * NWV) + (int)threadIdx.x;
            const bool live = (t * K1_KT + idx / LPR) < total_max;
            const int o = (idx / LPR) * ROW + 8 * (idx % LPR);
            *reinterpret_cast<u32x4 *>(&tiles[buf][0][o]) = live ? kst[S][i] : u32x4{0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4 *>(&tiles[buf][1][o]) = live ? vst[S][i] : u32x4{0u, 0u, 0u, 0u};
        }
    };

    float m_run = -INFINITY, l_run = 0.0f;
    f32x4 o_acc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) o_acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto compute_tile = [&](int t, int buf) {
        if (t >= wt0 && t < wt1) {
            const unsigned short *kl = tiles[buf][0], *vl = tiles[buf][1];
            f32x4 st[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                st[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const u32x4 kf = *reinterpret_cast<const u32x4 *>(kl + (16 * kb + c) * ROW + 32 * ks + 8 * g);
                    st[kb] = Frag<DT>::mfma(as_frag<vec>(kf), qf[ks], st[kb]);
                }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int key = t * K1_KT + 16 * kb + 4 * g + r;
                    bool vis = (key >= kstart) && (key <= kv_len + c) && (key < total);
                    float sv = vis ? st[kb][r] * scale : -INFINITY;
                    st[kb][r] = sv;
                    mx = fmaxf(mx, sv);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m_run, mx);
            const float m_safe = (m_new == -INFINITY) ? 0.0f : m_new;
            const float alpha = __expf(m_run - m_safe);
            float rs = 0.0f;
            unsigned short pb[8];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float pv = __expf(st[kb][r] - m_safe);
                    rs += pv;
                    pb[4 * kb + r] = Frag<DT>::cvt(pv);
                }
            rs += __shfl_xor(rs, 16);
            rs += __shfl_xor(rs, 32);
            l_run = l_run * alpha + rs;
            m_run = m_new;
            u32x4 pw;
            pw[0] = pb[0] | ((unsigned)pb[1] << 16);
            pw[1] = pb[2] | ((unsigned)pb[3] << 16);
            pw[2] = pb[4] | ((unsigned)pb[5] << 16);
            pw[3] = pb[6] | ((unsigned)pb[7] << 16);
            const vec pfrag = as_frag<vec>(pw);
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                const unsigned short *a0 = vl + (4 * g + (c >> 2)) * ROW + 16 * db + 4 * (c & 3);
                u32x2 lo = lds_tr_read(a0);
                u32x2 hi = lds_tr_read(a0 + 16 * ROW);
                u32x4 vv{lo[0], lo[1], hi[0], hi[1]};
                f32x4 acc = o_acc[db];
                acc[0] *= alpha; acc[1] *= alpha; acc[2] *= alpha; acc[3] *= alpha;
                o_acc[db] = Frag<DT>::mfma(as_frag<vec>(vv), pfrag, acc);
            }
        }
    };
    typedef std::integral_constant<int, 0> S0;
    typedef std::integral_constant<int, 1> S1;
    typedef std::integral_constant<int, 2> S2;
    typedef std::integral_constant<int, NSET == 6 ? 3 : 0> S3;
    typedef std::integral_constant<int, NSET == 6 ? 4 : 0> S4;
    typedef std::integral_constant<int, NSET == 6 ? 5 : 0> S5;
    fetch(bt0, S0{});
    fetch(bt0 + 1, S1{});
    fetch(bt0 + 2, S2{});
    if constexpr (NSET == 6) { fetch(bt0 + 3, S3{}); fetch(bt0 + 4, S4{}); fetch(bt0 + 5, S5{}); }
    stash(bt0, 0, S0{});
    __syncthreads();
    SJD_TR(2);                    // first tile in LDS
    // iteration of tile t (relative index r = t - bt0, r % NSET == k): request tile r + NSET into set k (tile r left it one iteration ago),
    // multiply tile r out of LDS buffer r & 1, move tile r + 1 from set (k + 1) % NSET into the other buffer
#define K1S_STEP(SA, SB)                                                          \
    fetch(t + NSET, SA{});                                                        \
    compute_tile(t, (t - bt0) & 1);                                               \
    if (t + 1 < bt1) stash(t + 1, ((t - bt0) & 1) ^ 1, SB{});                     \
    __syncthreads();                                                              \
    if (++t >= bt1) break;
    for (int t = bt0; t < bt1;) {
        if constexpr (NSET == 6) {
            K1S_STEP(S0, S1) K1S_STEP(S1, S2) K1S_STEP(S2, S3) K1S_STEP(S3, S4) K1S_STEP(S4, S5) K1S_STEP(S5, S0)
        } else {
            K1S_STEP(S0, S1) K1S_STEP(S1, S2) K1S_STEP(S2, S0)
        }
    }
#undef K1S_STEP
    SJD_TR(3);                    // key loop done
    if (!wave_on) return;
    // the wave covered every tile of its split: its (m, l, O) is the split partial
    const size_t slot0 = ((((size_t)b * H + head) * n_chunks + chunk) * n_split + split) * K1_ROWS;
#pragma unroll
    for (int db = 0; db < DB; ++db) *reinterpret_cast<f32x4 *>(ws_o + (slot0 + c) * D + 16 * db + 4 * g) = o_acc[db];
    if (g == 0) { ws_ml[(slot0 + c) * 2] = m_run; ws_ml[(slot0 + c) * 2 + 1] = l_run; }
#ifdef SJD_TRACE
    SJD_TR(4);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    SJD_TR(5);                    // partial stored
    SJD_TR(6); SJD_TR(7);
#endif
    (void)nw;
}
#endif  // SJD_EXPERIMENTAL

#include "sjd_attention_ring.h"

// RS (round 4 experiment): row blocks per 16-row chunk = workgroups per (batch, head, chunk).  RS = 2 gives Emu3's shape 256 workgroups instead
// of 128 (8 rows x 128 d each, one float4 per thread and split; the arithmetic per element is unchanged) -- and measured SLOWER (Emu3 pair 22.2 -> 24.8 us, Lumina 14.1 -> 14.8 us, profiles/r4_k1_combine_rs.txt: the launch is bound by its cold
// start and its one round trip, not by the CUs it covers), so RS = 1 is the only instantiation.
template <int DT, int D, int RS = 1>
__global__ __launch_bounds__(256) void k1_combine(const float *__restrict__ ws_o, const float *__restrict__ ws_ml,
                                                 unsigned short *__restrict__ out, int n_rows, int H, int n_split, int n_chunks,
                                                 const sjd_iter_params *__restrict__ params, const int *__restrict__ key_start,
                                                 int kv_len_arg)
{
    SJD_TRC(0);
    const int chunk = blockIdx.x / RS, rblock = blockIdx.x % RS, head = blockIdx.y, b = blockIdx.z;
    constexpr int PER = (K1_ROWS / RS) * D / 256;   // consecutive d per thread
    static_assert(PER >= 1 && PER * 256 == (K1_ROWS / RS) * D, "256 threads cover the row block exactly");
    const int row = rblock * (K1_ROWS / RS) + (threadIdx.x * PER) / D, d0 = (threadIdx.x * PER) % D;
    const int grow = chunk * K1_ROWS + row;
    const size_t base = (((size_t)b * H + head) * n_chunks + chunk) * n_split;
    // sixteen splits' (m, l, O) in flight at a time (the partials were written by the kernel that has just finished: cold -- every batch is
    // a full round trip; with batches of four, Emu3's 16 splits took four of them, 7.6 us), merged online in split order.
    // The first batch is requested for ALL n_split slots BEFORE the effective split count is known (it needs kv_len from the device blob:
    // a scalar round trip that used to sit in front of these loads); slots beyond the effective count hold stale partials and are not merged.
    constexpr int CB = 16;
    float ms[CB], ls[CB], os[CB][PER];
#pragma unroll
    for (int q = 0; q < CB; ++q)
        if (q < n_split) {
            const size_t slot = (base + q) * K1_ROWS + row;
            ms[q] = ws_ml[slot * 2];
            ls[q] = ws_ml[slot * 2 + 1];
#pragma unroll
            for (int j = 0; j < PER; ++j) os[q][j] = ws_o[slot * D + d0 + j];
        }
    int kv_base, n_total, kstart;
    k1_entry(params, key_start, b, kv_len_arg, n_rows, kv_base, n_total, kstart);
    int eff_split;
    {
        const int n_c = min(K1_ROWS, n_total - chunk * K1_ROWS);
        const int total = kv_base + chunk * K1_ROWS + max(n_c, 0);
        int t_lo, t_hi, tps;
        k1_tile_range(kstart, total, n_split, t_lo, t_hi, eff_split, tps);
    }
    if (grow >= n_rows) return;
    if (grow >= n_total) {        // padding rows of a shape-static window: defined (zero) output, never garbage
        unsigned short *oz = out + (((size_t)b * n_rows + grow) * H + head) * D + d0;
#pragma unroll
        for (int j = 0; j < PER; ++j) oz[j] = 0;
        return;
    }
    float M = -INFINITY, L = 0.f, acc[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) acc[j] = 0.f;
    for (int s0 = 0; s0 < eff_split; s0 += CB) {
        if (s0 > 0) {                               // (more than sixteen splits: further batches, now that the count is known)
#pragma unroll
            for (int q = 0; q < CB; ++q)
                if (s0 + q < eff_split) {
                    const size_t slot = (base + s0 + q) * K1_ROWS + row;
                    ms[q] = ws_ml[slot * 2];
                    ls[q] = ws_ml[slot * 2 + 1];
#pragma unroll
                    for (int j = 0; j < PER; ++j) os[q][j] = ws_o[slot * D + d0 + j];
                }
        }
#pragma unroll
        for (int q = 0; q < CB; ++q)
            if (s0 + q < eff_split) k1_merge_step<PER>(M, L, acc, ms[q], ls[q], os[q]);
    }
    const float inv = L > 0.f ? 1.0f / L : 0.0f;
    if (inv != 12345.678f) SJD_TRC(1);          // (partials arrived)
    unsigned short *o = out + (((size_t)b * n_rows + grow) * H + head) * D + d0;
#pragma unroll
    for (int j = 0; j < PER; ++j) o[j] = Frag<DT>::cvt(acc[j] * inv);
    SJD_TRC(2);
}

#ifdef SJD_EXPERIMENTAL        // K1F / K1Fs (rounds 2-3, measured no-go): libsjd_hip_exp.so only
// ------------------------------------------------------------------------------------------------ K1F (fused F2 + K1 + combine)
// rocprofv3, round 1: per layer the attention block is THREE dependent launches -- F2 (QK-norm + RoPE + KV append, 5.2 us), k1_partial
// (11.8 us at kv_len 100 ... 21 us at 1216) and k1_combine (4.6 us) -- each at its launch-latency floor, and the split partials make a
// round trip through HBM.  K1F does all of it in ONE launch for the multi-head-attention window (H == H_kv, <= 16 rows, D = 128):
//   grid = (H, B); one 512-thread workgroup = 8 wave64 owns a (batch, head) completely.
//   phase A  the 48 (row, q|k|v) head slices are spread over the waves (6 each): a wave sums the fp32 split-K partials of its slice
//            (lane l owns the rotate-half pair d = l, l + 64), applies the folded RMSNorm row scale, per-head LayerNorm, RoPE -- the
//            arithmetic and rounding points of F2 (sjd_glue.hip), so K/V rows are bit-identical -- and writes q to LDS, k / v into cache
//            rows [kv_len + row].  Waves whose first key tile lies wholly below kv_len have its K/V loads in flight meanwhile.
//   phase B  wave w walks key tiles t_lo + w, + 8, ... like k1_partial, two tiles in flight (K rows straight from HBM into MFMA fragments, V via a
//            per-wave LDS tile and ds_read_b64_tr_b16, online softmax in registers): 8 waves x 32 KB in flight per CU replace the four
//            4-wave workgroups of the split version, and the window's own K/V rows are read back by the workgroup that wrote them.
//   phase C  the 8 (m, l, O) states are merged through LDS (the arena of the V tiles, reused) and the normalised output goes straight
//            to out[B, n, H, D]: no workspace, no second kernel.
// 64 workgroups instead of 256: each CU has to pull ~0.6 MB at kv_len 1216, which 8 waves with two tiles each in flight have to sustain (~100 GB/s per CU).
#define K1F_WAVES 8           // 512 threads = 2 waves per SIMD = 256 registers per lane: room for TWO key tiles in flight per wave

template <int DT> __device__ __forceinline__ float k1f_round(float x);
template <> __device__ __forceinline__ float k1f_round<SJD_DTYPE_BF16>(float x)
{   // the round-to-nearest-even F2 uses (sjd_glue.hip Cvt<BF16>)
    unsigned u = __float_as_uint(x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return __uint_as_float(u & 0xffff0000u);
}
template <> __device__ __forceinline__ float k1f_round<SJD_DTYPE_F16>(float x) { return (float)((_Float16)x); }
template <int DT> __device__ __forceinline__ unsigned short k1f_bits(float x);       // x already representable
template <> __device__ __forceinline__ unsigned short k1f_bits<SJD_DTYPE_BF16>(float x) { return (unsigned short)(__float_as_uint(x) >> 16); }
template <> __device__ __forceinline__ unsigned short k1f_bits<SJD_DTYPE_F16>(float x) { _Float16 h = (_Float16)x; return *reinterpret_cast<unsigned short *>(&h); }
template <int DT> __device__ __forceinline__ float k1f_load16(const unsigned short *p);
template <> __device__ __forceinline__ float k1f_load16<SJD_DTYPE_BF16>(const unsigned short *p) { return __uint_as_float((unsigned)(*p) << 16); }
template <> __device__ __forceinline__ float k1f_load16<SJD_DTYPE_F16>(const unsigned short *p) { return (float)(*reinterpret_cast<const _Float16 *>(p)); }

__device__ __forceinline__ float k1f_wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int DT, int D>
__global__ __launch_bounds__(64 * K1F_WAVES) void k1f_qkv_attention(
    const float *__restrict__ part, int n_chunks, int prows, const unsigned short *__restrict__ qn_w, const unsigned short *__restrict__ qn_b,
    const unsigned short *__restrict__ kn_w, const unsigned short *__restrict__ kn_b, const float *__restrict__ inv_freq,
    const long *__restrict__ positions, const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden, float rs_eps,
    unsigned short *__restrict__ kc, unsigned short *__restrict__ vc, unsigned short *__restrict__ out, int n_rows, int H, int S_max,
    const int *__restrict__ key_start, const sjd_iter_params *__restrict__ params, int kv_len_arg,
    int n_split = 1, float *__restrict__ ws_o = nullptr, float *__restrict__ ws_ml = nullptr)
{
    // n_split > 1 (round 3, "K1Fs"): grid (H, B, n_split) -- the key tiles of a (batch, head) are split over n_split workgroups exactly as
    // k1_partial splits them (k1_tile_range, the effective count from the device-side kv_len), every workgroup derives q for itself (16 of
    // the 48 phase-A tasks), the workgroups whose tiles reach into the window's own rows also derive and append those K / V rows (identical
    // bytes if two of them do), and phase C publishes the split's (m, l, O) in k1_partial's workspace layout for k1_combine.  F2 + k1_partial
    // become ONE launch that fills the chip: the 64-workgroup form above streamed at 1.8 TB/s.
    typedef typename Frag<DT>::vec vec;
    static_assert(D == 128, "K1F is written for head_dim 128");
    constexpr int HALF = D / 2, KS = D / 32, DB = D / 16, VROW = D + 8;
    constexpr int V_BYTES = K1F_WAVES * K1_KT * VROW * 2;             // per-wave V tiles of the key loop
    constexpr int R_BYTES = K1F_WAVES * K1_ROWS * (D + 2) * 4;        // merge buffers of the epilogue (aliased)
    __shared__ __attribute__((aligned(16))) unsigned char arena[V_BYTES > R_BYTES ? V_BYTES : R_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned short q_lds[K1_ROWS][VROW];
    unsigned short (*v_lds)[K1_KT * VROW] = reinterpret_cast<unsigned short (*)[K1_KT * VROW]>(arena);
    float (*red_o)[K1_ROWS][D] = reinterpret_cast<float (*)[K1_ROWS][D]>(arena);
    float (*red_ml)[K1_ROWS][2] = reinterpret_cast<float (*)[K1_ROWS][2]>(arena + K1F_WAVES * K1_ROWS * D * 4);

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int head = blockIdx.x, b = blockIdx.y;
    int kv_len = kv_len_arg, n_total = n_rows;
    if (params) sjdi_kv_rows(params, b, &kv_len, &n_total);
    const int n_c = min(min(K1_ROWS, n_rows), n_total);
    const int total = kv_len + max(n_c, 0);
    const int kstart = key_start ? key_start[b] : 0;
    const float scale = rsqrtf((float)D);
    int t_lo, t_hi, eff_split, tps;
    k1_tile_range(kstart, total, n_split, t_lo, t_hi, eff_split, tps);
    const int split = blockIdx.z;
    if (split >= eff_split) return;
    t_lo += split * tps;                                                   // this workgroup's tiles
    t_hi = min(t_hi, t_lo + tps);
    const bool does_kv = t_hi * K1_KT > kv_len;                            // its tiles reach into the window's own rows: it appends (and reads) them
    unsigned short *kbase = kc + ((size_t)b * H + head) * (size_t)S_max * D;
    unsigned short *vbase = vc + ((size_t)b * H + head) * (size_t)S_max * D;

    // ---------------- phase A (round 3: rewritten for the memory system).  Wave w owns rows 2 w and 2 w + 1 of the window: their q slices
    // always, their k and v slices when this workgroup appends (does_kv).  In a slice lane l owns the rotate-half pair d = l, l + 64.  EVERY
    // load of a batch -- the row statistics, up to eight split-K planes of both rows, the norm gains, the rotation frequencies and positions
    // -- is unconditional (row / chunk indices clamped, values masked afterwards) and issued before the first use: one round trip per batch.
    // The first version walked six (row, tensor) tasks per wave with conditional loads, i.e. a dozen dependent round trips (K1Fs measured
    // 3.27 ms per step against 2.98 for F2 + K1 + combine).
    constexpr int RPW = K1_ROWS / K1F_WAVES;                      // rows per wave (2)
    static_assert(RPW * K1F_WAVES == K1_ROWS, "rows must divide evenly");
    const size_t ncol = (size_t)3 * H * D;
    const size_t cstride = (size_t)prows * ncol;
    int rowi[RPW], toki[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) { rowi[r] = w * RPW + r; toki[r] = b * n_rows + min(rowi[r], n_rows - 1); }
    // (slots beyond n_chunks re-read the last plane and are not added; with at most four planes -- the production q|k|v launch shape --
    // only four slots per slice are requested, so that q, k AND v of both rows fit into ONE batch under the 63-load vmcnt ceiling)
    const bool few = n_chunks <= 4;
    auto plane_loads = [&](int x, float (&v0)[RPW][8], float (&v1)[RPW][8]) {
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const float *p0 = part + (size_t)toki[r] * ncol + ((size_t)x * H + head) * D + lane;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float *pp = p0 + (size_t)min(q, n_chunks - 1) * cstride;
                v0[r][q] = pp[0];
                v1[r][q] = pp[HALF];
            }
            if (!few) {
#pragma unroll
                for (int q = 4; q < 8; ++q) {
                    const float *pp = p0 + (size_t)min(q, n_chunks - 1) * cstride;
                    v0[r][q] = pp[0];
                    v1[r][q] = pp[HALF];
                }
            } else {
#pragma unroll
                for (int q = 4; q < 8; ++q) { v0[r][q] = 0.f; v1[r][q] = 0.f; }
            }
        }
    };
    // the row statistics: lane q holds slice q (q < 8; further slices in the math below) -- ONE load per row instead of eight
    float ssl[RPW], qv0[RPW][8], qv1[RPW][8];
    {
        const float *ssp = row_sumsq ? row_sumsq : part;
#pragma unroll
        for (int r = 0; r < RPW; ++r) ssl[r] = ssp[(size_t)(row_sumsq ? min(lane & 7, rs_slices - 1) : 0) * prows + toki[r]];
    }
    plane_loads(0, qv0, qv1);
    float kv0[RPW][8], kv1[RPW][8], vv0[RPW][8], vv1[RPW][8];
    if (does_kv && few) { plane_loads(1, kv0, kv1); plane_loads(2, vv0, vv1); }          // everything this workgroup needs: one round trip
    float posf[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) posf[r] = (float)positions[toki[r]];
    const float ifr = inv_freq[lane];
    const unsigned short *wl = qn_w ? qn_w : reinterpret_cast<const unsigned short *>(part);       // (unconditional loads: any readable address)
    const unsigned short *bl = qn_b ? qn_b : reinterpret_cast<const unsigned short *>(part);
    const unsigned short *wk = kn_w ? kn_w : reinterpret_cast<const unsigned short *>(part);
    const unsigned short *bk = kn_b ? kn_b : reinterpret_cast<const unsigned short *>(part);
    const float qw0 = k1f_load16<DT>(wl + lane), qw1 = k1f_load16<DT>(wl + lane + HALF), qb0 = k1f_load16<DT>(bl + lane), qb1 = k1f_load16<DT>(bl + lane + HALF);
    const float kw0 = k1f_load16<DT>(wk + lane), kw1 = k1f_load16<DT>(wk + lane + HALF), kb0 = k1f_load16<DT>(bk + lane), kb1 = k1f_load16<DT>(bk + lane + HALF);

    // ---------------- key tiles.  A wave owns tiles t_lo + w, + 8, ...; TWO of them are in flight at any time (two register landing
    // zones of K fragments + V rows, 64 registers each): measured with one tile in flight and 12 waves, a CU pulled only ~40 GB/s -- the
    // per-wave load -> MFMA -> softmax -> LDS -> MFMA chain is latency bound -- and with 64 workgroups the kernel needs ~100 GB/s per CU
    // to beat four 4-wave workgroups per head.  Tiles that contain rows this workgroup is about to append are fetched after the barrier.
    u32x4 kA[2][KS], kB[2][KS];
    constexpr int VP = K1_KT * D / (64 * 8), LPR = D / 8;
    u32x4 vA[VP], vB[VP];
    unsigned short *vl = v_lds[w];
    auto load_k = [&](int t_, u32x4 (&kd)[2][KS]) {
        const unsigned short *kt = kbase + (size_t)(t_ * K1_KT) * D;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                kd[kb][ks] = *reinterpret_cast<const u32x4 *>(kt + (size_t)(16 * kb + c) * D + 32 * ks + 8 * g);
    };
    auto load_v = [&](int t_, u32x4 (&vd)[VP]) {
        const unsigned short *vt = vbase + (size_t)(t_ * K1_KT) * D;
#pragma unroll
        for (int i = 0; i < VP; ++i) {
            const int idx = i * 64 + lane;
            vd[i] = *reinterpret_cast<const u32x4 *>(vt + (size_t)(idx / LPR) * D + 8 * (idx % LPR));
        }
    };
    auto store_v = [&](int t_, u32x4 (&vd)[VP]) {                // rows of keys >= total are zeroed (0 * NaN inside the MFMA)
#pragma unroll
        for (int i = 0; i < VP; ++i) {
            const int idx = i * 64 + lane;
            const bool live = (t_ * K1_KT + idx / LPR) < total;
            *reinterpret_cast<u32x4 *>(vl + (idx / LPR) * VROW + 8 * (idx % LPR)) = live ? vd[i] : u32x4{0u, 0u, 0u, 0u};
        }
    };
    const int t0 = t_lo + w, t1 = t0 + K1F_WAVES;
    const bool early0 = (t0 < t_hi) && ((t0 + 1) * K1_KT <= kv_len);         // no window row inside: safe to fetch before the append
    const bool early1 = (t1 < t_hi) && ((t1 + 1) * K1_KT <= kv_len);
    if (early0) { load_k(t0, kA); load_v(t0, vA); }
    if (early1) { load_k(t1, kB); load_v(t1, vB); }

    // ---------------- phase A math: the arithmetic of f2_qknorm_rope_append, same rounding points.  (More than eight planes / slices: the
    // remaining ones in further batches, in order.)
    float rscale[RPW], csr[RPW], snr[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {                           // slice order, as row_sumsq_total (sjd_glue.hip)
            const float sq = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ssl[r]), q));
            t += (q < rs_slices) ? sq : 0.f;
        }
        for (int s0 = 8; s0 < rs_slices; s0 += 8) {
            float v8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v8[q] = (s0 + q < rs_slices) ? row_sumsq[(size_t)(s0 + q) * prows + toki[r]] : 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) t += v8[q];
        }
        rscale[r] = row_sumsq ? rsqrtf(t * rs_inv_hidden + rs_eps) : 1.0f;
        float sn, cs;
        sincosf(posf[r] * ifr, &sn, &cs);
        csr[r] = k1f_round<DT>(cs);
        snr[r] = k1f_round<DT>(sn);
    }
    // one (row, tensor) slice: sum of the planes in chunk order, row scale, rounding, [LayerNorm, RoPE] -> the two 16-bit values of this lane
    auto finish = [&](int x, int r, const float (&v0)[8], const float (&v1)[8], unsigned short &o0, unsigned short &o1) {
        float x0 = 0.f, x1 = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (q < n_chunks) { x0 += v0[q]; x1 += v1[q]; }
        for (int c0 = 8; c0 < n_chunks; ++c0) {
            const float *pp = part + (size_t)toki[r] * ncol + ((size_t)x * H + head) * D + lane + (size_t)c0 * cstride;
            x0 += pp[0];
            x1 += pp[HALF];
        }
        if (row_sumsq) { x0 *= rscale[r]; x1 *= rscale[r]; }
        x0 = k1f_round<DT>(x0);
        x1 = k1f_round<DT>(x1);
        if (x == 2) { o0 = k1f_bits<DT>(x0); o1 = k1f_bits<DT>(x1); return; }               // V: plain copy
        const bool normed = x == 0 ? qn_w != nullptr : kn_w != nullptr;
        if (normed) {                                                                         // per-head LayerNorm over head_dim (eps 1e-5)
            const float mean = k1f_wave_sum(x0 + x1) / (float)D;
            const float d0 = x0 - mean, d1 = x1 - mean;
            const float var = k1f_wave_sum(d0 * d0 + d1 * d1) / (float)D;
            const float inv = rsqrtf(var + 1e-5f);
            {
#pragma clang fp contract(off)
                // (as F2, sjd_glue.hip: in fp16 the compiler otherwise demotes dtype(n * gain) + bias to ONE half-precision FMA and the rounding of
                // the product is gone)
                const float n0 = k1f_round<DT>(d0 * inv), n1 = k1f_round<DT>(d1 * inv);
                x0 = k1f_round<DT>(k1f_round<DT>(n0 * (x == 0 ? qw0 : kw0)) + (x == 0 ? qb0 : kb0));
                x1 = k1f_round<DT>(k1f_round<DT>(n1 * (x == 0 ? qw1 : kw1)) + (x == 0 ? qb1 : kb1));
            }
        }
        {
#pragma clang fp contract(off)
            const float a0 = k1f_round<DT>(x0 * csr[r]), b0 = k1f_round<DT>(-x1 * snr[r]);
            const float a1 = k1f_round<DT>(x1 * csr[r]), b1 = k1f_round<DT>(x0 * snr[r]);
            o0 = k1f_bits<DT>(k1f_round<DT>(a0 + b0));
            o1 = k1f_bits<DT>(k1f_round<DT>(a1 + b1));
        }
    };
    if (does_kv && !few) plane_loads(1, kv0, kv1);                               // (more than four planes: k under the q math, v under the k math)
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        unsigned short o0, o1;
        finish(0, r, qv0[r], qv1[r], o0, o1);
        if (rowi[r] < n_rows) { q_lds[rowi[r]][lane] = o0; q_lds[rowi[r]][lane + HALF] = o1; }
    }
    if (does_kv) {
        if (!few) plane_loads(2, vv0, vv1);
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            unsigned short o0, o1;
            finish(1, r, kv0[r], kv1[r], o0, o1);
            const int rr = kv_len + rowi[r];
            if (rowi[r] < n_rows && rr < S_max) { kbase[(size_t)rr * D + lane] = o0; kbase[(size_t)rr * D + lane + HALF] = o1; }
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            unsigned short o0, o1;
            finish(2, r, vv0[r], vv1[r], o0, o1);
            const int rr = kv_len + rowi[r];
            if (rowi[r] < n_rows && rr < S_max) { vbase[(size_t)rr * D + lane] = o0; vbase[(size_t)rr * D + lane + HALF] = o1; }
        }
    }
    __syncthreads();            // q in LDS; this workgroup's K/V rows acknowledged by L2 (it is their only reader in this launch)

    // ---------------- phase B: the key loop of k1_partial with 8 key-parts, two tiles in flight per wave
    const bool rv = (c < n_c);
    float m_run = -INFINITY, l_run = 0.0f;
    f32x4 o_acc[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) o_acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t0 < t_hi && !early0) { load_k(t0, kA); load_v(t0, vA); }
    if (t1 < t_hi && !early1) { load_k(t1, kB); load_v(t1, vB); }
    // one tile: on entry kc_ / vc_ hold (or are about to receive) tile t_; the other pair holds tile t_ + 8.  As soon as a landing zone
    // has been consumed it is re-armed with tile t_ + 16.
    auto step = [&](int t_, u32x4 (&kc_)[2][KS], u32x4 (&vc_)[VP]) {
        const int t2 = t_ + 2 * K1F_WAVES;
        const bool more = t2 < t_hi;
        f32x4 st[2];
        st[0] = f32x4{0.f, 0.f, 0.f, 0.f};
        st[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {                        // Q fragments from LDS (4 ds_read_b128 per tile instead of 16 registers)
            const u32x4 qx = rv ? *reinterpret_cast<const u32x4 *>(&q_lds[c][32 * ks + 8 * g]) : u32x4{0, 0, 0, 0};
            st[0] = Frag<DT>::mfma(as_frag<vec>(kc_[0][ks]), as_frag<vec>(qx), st[0]);
            st[1] = Frag<DT>::mfma(as_frag<vec>(kc_[1][ks]), as_frag<vec>(qx), st[1]);
        }
        if (more) load_k(t2, kc_);
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = t_ * K1_KT + 16 * kb + 4 * g + r;
                const bool vis = (key >= kstart) && (key <= kv_len + c) && (key < total);
                const float sv = vis ? st[kb][r] * scale : -INFINITY;
                st[kb][r] = sv;
                mx = fmaxf(mx, sv);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float m_safe = (m_new == -INFINITY) ? 0.0f : m_new;
        const float alpha = __expf(m_run - m_safe);
        float rsum = 0.0f;
        unsigned short pb[8];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = __expf(st[kb][r] - m_safe);
                rsum += pv;
                pb[4 * kb + r] = Frag<DT>::cvt(pv);
            }
        rsum += __shfl_xor(rsum, 16);
        rsum += __shfl_xor(rsum, 32);
        l_run = l_run * alpha + rsum;
        m_run = m_new;
        u32x4 pw;
        pw[0] = pb[0] | ((unsigned)pb[1] << 16);
        pw[1] = pb[2] | ((unsigned)pb[3] << 16);
        pw[2] = pb[4] | ((unsigned)pb[5] << 16);
        pw[3] = pb[6] | ((unsigned)pb[7] << 16);
        const vec pfrag = as_frag<vec>(pw);
        store_v(t_, vc_);              // in-order LDS queue: the previous tile's transposed reads are done
        if (more) load_v(t2, vc_);
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const unsigned short *a0 = vl + (4 * g + (c >> 2)) * VROW + 16 * db + 4 * (c & 3);
            const u32x2 lo = lds_tr_read(a0), hi = lds_tr_read(a0 + 16 * VROW);
            const u32x4 vv{lo[0], lo[1], hi[0], hi[1]};
            f32x4 a = o_acc[db];
            a[0] *= alpha; a[1] *= alpha; a[2] *= alpha; a[3] *= alpha;
            o_acc[db] = Frag<DT>::mfma(as_frag<vec>(vv), pfrag, a);
        }
    };
    for (int t = t0; t < t_hi; t += 2 * K1F_WAVES) {
        step(t, kA, vA);
        if (t + K1F_WAVES < t_hi) step(t + K1F_WAVES, kB, vB);
    }

    // ---------------- phase C: merge the 16 key-parts and write the normalised rows
    __syncthreads();
    if (g == 0) { red_ml[w][c][0] = m_run; red_ml[w][c][1] = l_run; }
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) red_o[w][c][16 * db + 4 * g + r] = o_acc[db][r];
    __syncthreads();
    for (int idx = threadIdx.x; idx < K1_ROWS * D; idx += 64 * K1F_WAVES) {
        const int row = idx / D, d = idx % D;
        if (n_split > 1) {                                      // the split's partial in k1_partial's workspace layout (one 16-row chunk)
            float M = -INFINITY;
#pragma unroll
            for (int ww = 0; ww < K1F_WAVES; ++ww) M = fmaxf(M, red_ml[ww][row][0]);
            const float Ms = (M == -INFINITY) ? 0.0f : M;
            float L = 0.f, O = 0.f;
#pragma unroll
            for (int ww = 0; ww < K1F_WAVES; ++ww) {
                const float wgt = __expf(red_ml[ww][row][0] - Ms);
                L += wgt * red_ml[ww][row][1];
                O += wgt * red_o[ww][row][d];
            }
            const size_t slot = (((size_t)b * H + head) * n_split + split) * K1_ROWS + row;
            ws_o[slot * D + d] = O;
            if (d == 0) { ws_ml[slot * 2] = M; ws_ml[slot * 2 + 1] = L; }
            continue;
        }
        if (row >= n_rows) continue;
        unsigned short *o = out + (((size_t)b * n_rows + row) * H + head) * D + d;
        if (row >= n_total) { *o = 0; continue; }              // padding rows of a shape-static window: defined (zero) output
        float M = -INFINITY;
#pragma unroll
        for (int ww = 0; ww < K1F_WAVES; ++ww) M = fmaxf(M, red_ml[ww][row][0]);
        const float Ms = (M == -INFINITY) ? 0.0f : M;
        float L = 0.f, O = 0.f;
#pragma unroll
        for (int ww = 0; ww < K1F_WAVES; ++ww) {
            const float wgt = __expf(red_ml[ww][row][0] - Ms);
            L += wgt * red_ml[ww][row][1];
            O += wgt * red_o[ww][row][d];
        }
        *o = Frag<DT>::cvt(L > 0.f ? O / L : 0.0f);
    }
}

extern "C" int sjd_qkv_attention_fused(const float *part, int n_chunks, void *k_cache, void *v_cache, void *out, const void *qn_w,
                                       const void *qn_b, const void *kn_w, const void *kn_b, const float *inv_freq, const int64_t *positions,
                                       int B, int n_rows, int H, int D, int S_max, int dtype, const sjd_row_norm *row_norm,
                                       const int32_t *key_start, const sjd_iter_params *params, int kv_len, void *stream)
{
    if (!part || n_chunks < 1 || !k_cache || !v_cache || !out || !inv_freq || !positions || B < 1 || H < 1) return SJD_ERR_BAD_ARG;
    if (n_rows < 1 || n_rows > K1_ROWS || B * n_rows > 32 || (S_max % K1_KT) != 0) return SJD_ERR_BAD_ARG;
    if ((qn_w == nullptr) != (qn_b == nullptr) || (kn_w == nullptr) != (kn_b == nullptr)) return SJD_ERR_BAD_ARG;
    if (row_norm && (!row_norm->sumsq || row_norm->slices < 1 || row_norm->hidden < 1)) return SJD_ERR_BAD_ARG;
    if (D != 128) return SJD_ERR_UNSUPPORTED;
    const float *ss = row_norm ? row_norm->sumsq : nullptr;
    const int sl = row_norm ? row_norm->slices : 0;
    const float ih = row_norm ? 1.0f / (float)row_norm->hidden : 0.f, eps = row_norm ? row_norm->eps : 0.f;
    hipStream_t s = (hipStream_t)stream;
#define SJD_K1F_CASE(DT_)                                                                                                                  \
    if (dtype == DT_) {                                                                                                                    \
        hipLaunchKernelGGL((k1f_qkv_attention<DT_, 128>), dim3(H, B), dim3(64 * K1F_WAVES), 0, s, part, n_chunks, 32, (const unsigned short *)qn_w,   \
                           (const unsigned short *)qn_b, (const unsigned short *)kn_w, (const unsigned short *)kn_b, inv_freq,              \
                           (const long *)positions, ss, sl, ih, eps, (unsigned short *)k_cache, (unsigned short *)v_cache,                 \
                           (unsigned short *)out, n_rows, H, S_max, key_start, params, kv_len);                                           \
        return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;                                                                   \
    }
    SJD_K1F_CASE(SJD_DTYPE_BF16)
    SJD_K1F_CASE(SJD_DTYPE_F16)
#undef SJD_K1F_CASE
    return SJD_ERR_UNSUPPORTED;
}

// K1Fs: sjd_qkv_attention_fused with the key tiles split over n_split workgroups per (batch, head) + k1_combine: F2 and k1_partial in one
// launch that fills the chip.  workspace: sjd_attention_workspace_bytes(B, H, n_rows, D, n_split).  n_split == 1 is sjd_qkv_attention_fused.
extern "C" int sjd_qkv_attention_fused_split(const float *part, int n_chunks, void *k_cache, void *v_cache, void *out, const void *qn_w,
                                             const void *qn_b, const void *kn_w, const void *kn_b, const float *inv_freq,
                                             const int64_t *positions, int B, int n_rows, int H, int D, int S_max, int dtype,
                                             const sjd_row_norm *row_norm, const int32_t *key_start, const sjd_iter_params *params, int kv_len,
                                             int n_split, void *workspace, void *stream)
{
    if (n_split <= 1)
        return sjd_qkv_attention_fused(part, n_chunks, k_cache, v_cache, out, qn_w, qn_b, kn_w, kn_b, inv_freq, positions, B, n_rows, H, D, S_max,
                                       dtype, row_norm, key_start, params, kv_len, stream);
    if (!part || n_chunks < 1 || !k_cache || !v_cache || !out || !inv_freq || !positions || !workspace || B < 1 || H < 1 || n_split > 64) return SJD_ERR_BAD_ARG;
    if (n_rows < 1 || n_rows > K1_ROWS || B * n_rows > 32 || (S_max % K1_KT) != 0) return SJD_ERR_BAD_ARG;
    if ((qn_w == nullptr) != (qn_b == nullptr) || (kn_w == nullptr) != (kn_b == nullptr)) return SJD_ERR_BAD_ARG;
    if (row_norm && (!row_norm->sumsq || row_norm->slices < 1 || row_norm->hidden < 1)) return SJD_ERR_BAD_ARG;
    if (D != 128) return SJD_ERR_UNSUPPORTED;
    const float *ss = row_norm ? row_norm->sumsq : nullptr;
    const int sl = row_norm ? row_norm->slices : 0;
    const float ih = row_norm ? 1.0f / (float)row_norm->hidden : 0.f, eps = row_norm ? row_norm->eps : 0.f;
    hipStream_t s = (hipStream_t)stream;
    float *ws_o = (float *)workspace;
    float *ws_ml = ws_o + (size_t)B * H * n_split * K1_ROWS * D;           // (k1_partial's layout with one 16-row chunk)
#define SJD_K1FS_CASE(DT_)                                                                                                                 \
    if (dtype == DT_) {                                                                                                                    \
        hipLaunchKernelGGL((k1f_qkv_attention<DT_, 128>), dim3(H, B, n_split), dim3(64 * K1F_WAVES), 0, s, part, n_chunks, 32,              \
                           (const unsigned short *)qn_w, (const unsigned short *)qn_b, (const unsigned short *)kn_w,                        \
                           (const unsigned short *)kn_b, inv_freq, (const long *)positions, ss, sl, ih, eps, (unsigned short *)k_cache,    \
                           (unsigned short *)v_cache, (unsigned short *)out, n_rows, H, S_max, key_start, params, kv_len, n_split, ws_o,    \
                           ws_ml);                                                                                                         \
        hipLaunchKernelGGL((k1_combine<DT_, 128>), dim3(1, H, B), dim3(256), 0, s, ws_o, ws_ml, (unsigned short *)out, n_rows, H, n_split, 1,  \
                           params, key_start, kv_len);                                                                                     \
        return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;                                                                   \
    }
    SJD_K1FS_CASE(SJD_DTYPE_BF16)
    SJD_K1FS_CASE(SJD_DTYPE_F16)
#undef SJD_K1FS_CASE
    return SJD_ERR_UNSUPPORTED;
}

#endif  // SJD_EXPERIMENTAL
// ------------------------------------------------------------------------------------------------ K1 (fp8 KV)
// BASELINE config 5: the KV cache is stored as OCP fp8 e4m3 (value = fp8 * scale, one scale per tensor), which halves the
// bytes K1 streams, and both contractions run on v_mfma_f32_16x16x32_fp8_fp8:
//   S^T = K Q^T : K bytes go straight from HBM into the A operand (lane (key c, group g) takes the 16 bytes
//                 d = 64p + 16g .. +15 of its key row: first half = k-step 2p, second half = k-step 2p+1); q is converted to
//                 fp8 once, in the matching order;
//   O^T += V^T P^T : P is scaled by 256 and rounded to fp8 (keeps the softmax tail out of the e4m3 subnormals), V bytes
//                 pass through a per-wave LDS tile and come back transposed with ds_read_b64_tr_b8 (lane i of a 16-lane
//                 group points at row i/2, columns 8(i%2).. of an 8-key x 16-d byte block; lane c receives column c).
// Everything else (tile ranges, online softmax, masks, merge, workspace layout, k1_combine) is shared with k1_partial.
typedef __attribute__((ext_vector_type(2))) int i32x2;

// pack4_fp8: the bare conversion, for P (at most 256 by construction); pack4_fp8_sat: the saturating one (sjd_fp8.h), for what the outside
// world hands in -- the cache rows K3 writes and the q operand
__device__ __forceinline__ unsigned pack4_fp8(float a, float b, float c, float d) { return sjd_pack4_e4m3<false>(a, b, c, d); }
__device__ __forceinline__ unsigned pack4_fp8_sat(float a, float b, float c, float d) { return sjd_pack4_e4m3<true>(a, b, c, d); }
__device__ __forceinline__ long as_long(unsigned lo, unsigned hi) { return (long)(((unsigned long long)hi << 32) | lo); }

// ---- hi / lo operands (round 6; VERDICT r5 #2b).  The fp8 attention rounded FOUR things to e4m3's three mantissa bits: K and V (the cache: that is
// the format BASELINE config 5 names) and, on chip, Q and P -- although the matrix pipe is 2-5 % busy here.  Q and P now travel as TWO e4m3
// operands each: hi = fp8(x), lo = fp8(16 (x - hi)) (the residual of a rounding is at most 2^-4 of the value: scaled by 16 it uses the same
// binades), one more MFMA per product into an accumulator of its own, merged as hi + lo / 16.  What is left of the two on-chip roundings is
// 2^-8 relative -- bf16's own resolution.  -DK1_FP8_HILO=0: the round-5 arithmetic (A/B aid).
#ifndef K1_FP8_HILO
#define K1_FP8_HILO 1
#endif
#define K1_LO_SCALE 16.0f
// SAT (the q operand: q arrives unscaled, and an fp16 q without QK-norm can be anything up to 65504): hi = sat_e4m3(x), lo = sat_e4m3(16 (x - hi)),
// so a finite q of any magnitude gives finite scores -- above 448 the operand is hi + lo / 16 <= 476 by definition, and only |q| <= 448 is exact
// to 2^-8.  P's calls keep the bare form: the hot loop's instructions are unchanged.
template <bool SAT = false>
__device__ __forceinline__ void pack4_fp8_hilo(float a, float b, float c, float d, unsigned &hi, unsigned &lo)
{
    hi = sjd_pack4_e4m3<SAT>(a, b, c, d);
    const float ra = a - __builtin_amdgcn_cvt_f32_fp8((int)hi, 0), rb = b - __builtin_amdgcn_cvt_f32_fp8((int)hi, 1);
    const float rc = c - __builtin_amdgcn_cvt_f32_fp8((int)hi, 2), rd = d - __builtin_amdgcn_cvt_f32_fp8((int)hi, 3);
    lo = sjd_pack4_e4m3<SAT>(ra * K1_LO_SCALE, rb * K1_LO_SCALE, rc * K1_LO_SCALE, rd * K1_LO_SCALE);
}

template <int DT> __device__ __forceinline__ float k1_to_f32(unsigned short h);
template <> __device__ __forceinline__ float k1_to_f32<SJD_DTYPE_BF16>(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
template <> __device__ __forceinline__ float k1_to_f32<SJD_DTYPE_F16>(unsigned short h) { return (float)(*reinterpret_cast<_Float16 *>(&h)); }

template <int DT, int D, int NW>
__global__ __launch_bounds__(64 * NW) void k1_partial_fp8(
    const unsigned short *__restrict__ q, const unsigned char *__restrict__ kc, const unsigned char *__restrict__ vc,
    const sjd_iter_params *__restrict__ params, const int *__restrict__ key_start,        // (among the first 16 dwords: preloaded into SGPRs)
    float *__restrict__ ws_o, float *__restrict__ ws_ml, unsigned short *__restrict__ out_direct,
    int n_rows, int H, int H_kv, int S_max, int kv_len_arg, int n_split, int n_chunks, float k_scale, float v_scale,
    unsigned short *__restrict__ merge_out = nullptr, unsigned *__restrict__ ticket = nullptr)
{
    constexpr int KP = D / 64;            // 16-byte K pieces per key row and lane group = pairs of k-steps
    constexpr int DB = D / 16;            // 16-wide d blocks of the output
    constexpr int VROW = D + 16;          // padded LDS row in bytes (16-B aligned rows, breaks the 128-B bank period)
    constexpr float PSCALE = 256.0f;
    constexpr int V_BYTES = NW * K1_KT * VROW;
    constexpr int R_BYTES = NW * K1_ROWS * (D + K1_RPAD + 2) * 4;
    __shared__ __attribute__((aligned(16))) unsigned char arena[V_BYTES > R_BYTES ? V_BYTES : R_BYTES];
    float (*red_o)[K1_ROWS][D + K1_RPAD] = reinterpret_cast<float (*)[K1_ROWS][D + K1_RPAD]>(arena);
    float (*red_ml)[K1_ROWS][2] = reinterpret_cast<float (*)[K1_ROWS][2]>(arena + NW * K1_ROWS * (D + K1_RPAD) * 4);

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int G = H / H_kv;
    const int kparts = NW / G;
    const int head_in_group = w % G, kpart = w / G;
    const int chunk = blockIdx.x / n_split, split = blockIdx.x % n_split;
    const int hkv = blockIdx.y, b = blockIdx.z;
    const int head = hkv * G + head_in_group;
    unsigned char *vl = arena + (size_t)w * K1_KT * VROW;

    int kv_base, n_total, kstart;
    k1_entry(params, key_start, b, kv_len_arg, n_rows, kv_base, n_total, kstart);
    const int row0 = chunk * K1_ROWS;
    const int n_c = min(K1_ROWS, n_total - row0);
    const int kv_len = kv_base + row0;
    const int total = kv_len + max(n_c, 0);
    const float scale = rsqrtf((float)D) * k_scale;

    int t_lo, t_hi, eff_split, tps;
    k1_tile_range(kstart, total, n_split, t_lo, t_hi, eff_split, tps);
    if (split >= eff_split) return;
    const int t_begin = t_lo + split * tps, t_end = min(t_hi, t_begin + tps);

    // Q (B operand) as fp8: lane (row c, group g), pair p: d = 64p + 16g .. +15 -> two 8-byte k-step operands
    long qf[KP][2], qfl[KP][2];           // (qfl: the residual operand, K1_FP8_HILO)
    {
        const bool rv = (c < n_c);
        const unsigned short *qp = q + (((size_t)b * n_rows + (row0 + (rv ? c : 0))) * H + head) * D + 16 * g;
#pragma unroll
        for (int p = 0; p < KP; ++p) {
            unsigned wds[4] = {0u, 0u, 0u, 0u}, wdl[4] = {0u, 0u, 0u, 0u};
            if (rv) {
                const u32x4 lo = *reinterpret_cast<const u32x4 *>(qp + 64 * p), hi = *reinterpret_cast<const u32x4 *>(qp + 64 * p + 8);
                float f[16];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    f[2 * i] = k1_to_f32<DT>((unsigned short)(lo[i] & 0xffffu)); f[2 * i + 1] = k1_to_f32<DT>((unsigned short)(lo[i] >> 16));
                    f[8 + 2 * i] = k1_to_f32<DT>((unsigned short)(hi[i] & 0xffffu)); f[8 + 2 * i + 1] = k1_to_f32<DT>((unsigned short)(hi[i] >> 16));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) pack4_fp8_hilo<true>(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3], wds[i], wdl[i]);
            }
            qf[p][0] = as_long(wds[0], wds[1]);
            qf[p][1] = as_long(wds[2], wds[3]);
            qfl[p][0] = as_long(wdl[0], wdl[1]);
            qfl[p][1] = as_long(wdl[2], wdl[3]);
        }
    }
    const unsigned char *kbase = kc + ((size_t)b * H_kv + hkv) * (size_t)S_max * D;
    const unsigned char *vbase = vc + ((size_t)b * H_kv + hkv) * (size_t)S_max * D;

    float m_run = -INFINITY, l_run = 0.0f;
    f32x4 o_acc[DB], o_lo[DB];            // (o_lo: the products with P's residual operand)
#pragma unroll
    for (int db = 0; db < DB; ++db) { o_acc[db] = f32x4{0.f, 0.f, 0.f, 0.f}; o_lo[db] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    constexpr int VP = K1_KT * D / (64 * 16);     // 16-B pieces per lane for one V tile
    constexpr int LPR = D / 16;                   // lanes per V row
    u32x4 kreg[2][KP], kn[2][KP], vstage[VP];

    auto load_tile = [&](int t, u32x4 (&kd)[2][KP], u32x4 (&vd)[VP]) {
        const unsigned char *kt = kbase + (size_t)(t * K1_KT) * D;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int p = 0; p < KP; ++p)
                kd[kb][p] = *reinterpret_cast<const u32x4 *>(kt + (size_t)(16 * kb + c) * D + 64 * p + 16 * g);
        const unsigned char *vt = vbase + (size_t)(t * K1_KT) * D;
#pragma unroll
        for (int i = 0; i < VP; ++i) {
            int idx = i * 64 + lane;
            vd[i] = *reinterpret_cast<const u32x4 *>(vt + (size_t)(idx / LPR) * D + 16 * (idx % LPR));
        }
    };
    // bytes of keys >= total are never visible (p = 0) but may decode to NaN: zero them while staging
    auto store_v = [&](int t, u32x4 (&vd)[VP]) {
#pragma unroll
        for (int i = 0; i < VP; ++i) {
            int idx = i * 64 + lane;
            const bool live = (t * K1_KT + idx / LPR) < total;
            *reinterpret_cast<u32x4 *>(vl + (idx / LPR) * VROW + 16 * (idx % LPR)) = live ? vd[i] : u32x4{0u, 0u, 0u, 0u};
        }
    };
    // transposed V operand: element j of lane group g is key 16(j/4) + 4g + (j%4) (the order the S^T accumulators hold P in)
    const int jrow = c >> 1;
    const unsigned char *vrd = vl + (16 * (jrow >> 2) + 4 * g + (jrow & 3)) * VROW + 8 * (c & 1);

    // two tiles of a wave in flight before the first one is waited for (see k1_partial)
    u32x4 vstage2[VP];
    auto compute_tile = [&](int t) {

        f32x4 st[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            st[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#if K1_FP8_HILO
            f32x4 sl = f32x4{0.f, 0.f, 0.f, 0.f};
#endif
#pragma unroll
            for (int p = 0; p < KP; ++p) {
                st[kb] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(as_long(kreg[kb][p][0], kreg[kb][p][1]), qf[p][0], st[kb], 0, 0, 0);
                st[kb] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(as_long(kreg[kb][p][2], kreg[kb][p][3]), qf[p][1], st[kb], 0, 0, 0);
#if K1_FP8_HILO
                sl = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(as_long(kreg[kb][p][0], kreg[kb][p][1]), qfl[p][0], sl, 0, 0, 0);
                sl = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(as_long(kreg[kb][p][2], kreg[kb][p][3]), qfl[p][1], sl, 0, 0, 0);
#endif
            }
#if K1_FP8_HILO
            st[kb] += sl * (1.0f / K1_LO_SCALE);
#endif
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int key = t * K1_KT + 16 * kb + 4 * g + r;
                bool vis = (key >= kstart) && (key <= kv_len + c) && (key < total);
                float sv = vis ? st[kb][r] * scale : -INFINITY;
                st[kb][r] = sv;
                mx = fmaxf(mx, sv);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float m_safe = (m_new == -INFINITY) ? 0.0f : m_new;
        const float alpha = __expf(m_run - m_safe);
        float rs = 0.0f, pv[8];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __expf(st[kb][r] - m_safe);
                rs += e;
                pv[4 * kb + r] = e * PSCALE;
            }
        rs += __shfl_xor(rs, 16);
        rs += __shfl_xor(rs, 32);
        l_run = l_run * alpha + rs;
        m_run = m_new;
#if K1_FP8_HILO
        unsigned ph0, pl0, ph1, pl1;
        pack4_fp8_hilo(pv[0], pv[1], pv[2], pv[3], ph0, pl0);
        pack4_fp8_hilo(pv[4], pv[5], pv[6], pv[7], ph1, pl1);
        const long pfrag = as_long(ph0, ph1), pfrag_lo = as_long(pl0, pl1);
#else
        const long pfrag = as_long(pack4_fp8(pv[0], pv[1], pv[2], pv[3]), pack4_fp8(pv[4], pv[5], pv[6], pv[7]));
#endif
#pragma unroll
        for (int db = 0; db < DB; ++db) {
            const i32x2 vv = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2 *)(vrd + 16 * db));
            f32x4 acc = o_acc[db];
            acc[0] *= alpha; acc[1] *= alpha; acc[2] *= alpha; acc[3] *= alpha;
            o_acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(as_long((unsigned)vv[0], (unsigned)vv[1]), pfrag, acc, 0, 0, 0);
#if K1_FP8_HILO
            f32x4 al = o_lo[db];
            al[0] *= alpha; al[1] *= alpha; al[2] *= alpha; al[3] *= alpha;
            o_lo[db] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(as_long((unsigned)vv[0], (unsigned)vv[1]), pfrag_lo, al, 0, 0, 0);
#endif
        }
    };
    auto adopt_next = [&](int tn, u32x4 (&vd)[VP]) {
        store_v(tn, vd);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int p = 0; p < KP; ++p) kreg[kb][p] = kn[kb][p];
    };
    int t = t_begin + kpart;
    if (t < t_end) {
        load_tile(t, kreg, vstage);
        if (t + kparts < t_end) {
            load_tile(t + kparts, kn, vstage2);
            store_v(t, vstage);
            compute_tile(t);
            adopt_next(t + kparts, vstage2);
            t += kparts;
        } else {
            store_v(t, vstage);
        }
    }
    for (; t < t_end; t += kparts) {
        const int tn = t + kparts;
        const bool has_next = tn < t_end;
        if (has_next) load_tile(tn, kn, vstage);
        compute_tile(t);
        if (has_next) adopt_next(tn, vstage);
    }

    __syncthreads();
    const float oscale = v_scale / PSCALE;
    if (g == 0) { red_ml[w][c][0] = m_run; red_ml[w][c][1] = l_run; }
#pragma unroll
    for (int db = 0; db < DB; ++db) {
#if K1_FP8_HILO
        o_acc[db] += o_lo[db] * (1.0f / K1_LO_SCALE);
#endif
        *reinterpret_cast<f32x4 *>(&red_o[w][c][16 * db + 4 * g]) = o_acc[db] * oscale;
    }
    __syncthreads();
    k1_merge_publish<DT, D, NW>(red_o, red_ml, G, kparts, b, H, hkv * G, n_chunks, chunk, n_split, split, row0, n_rows, n_total, ws_o, ws_ml,
                                out_direct, merge_out, ticket, eff_split);
}

#include "sjd_attention_dsplit_fp8.h"

// K3 for an fp8 cache: rows [kv_len, kv_len + n) <- sat_e4m3(x * (1 / scale)) (beyond +-448: +-448, sjd_fp8.h); one thread converts 8 values
// (16 B in, 8 B out)
template <int DT>
__global__ void k3_kv_append_fp8(const u32x4 *__restrict__ k_new, const u32x4 *__restrict__ v_new, u32x2 *__restrict__ k_cache,
                                 u32x2 *__restrict__ v_cache, int B, int n_rows, int H_kv, int D8, int S_max,
                                 const sjd_iter_params *__restrict__ params, int kv_len_arg, float k_inv, float v_inv, int head_major)
{
    const size_t total = (size_t)B * n_rows * H_kv * D8;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int d = i % D8;
        const int h = (i / D8) % H_kv;
        const int r = (i / ((size_t)D8 * H_kv)) % n_rows;
        const int b = i / ((size_t)D8 * H_kv * n_rows);
        int kv_len = kv_len_arg, n_unused_ = 0;
        if (params) sjdi_kv_rows(params, b, &kv_len, &n_unused_);
        if (kv_len + r >= S_max) continue;
        const size_t dst = (((size_t)b * H_kv + h) * S_max + (kv_len + r)) * D8 + d;
        const size_t src = head_major ? (((size_t)b * H_kv + h) * n_rows + r) * D8 + d : i;     // [B, H_kv, n, D] or [B, n, H_kv, D]
        const u32x4 kv = k_new[src], vv = v_new[src];
        float kf[8], vf[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kf[2 * j] = k1_to_f32<DT>((unsigned short)(kv[j] & 0xffffu)) * k_inv; kf[2 * j + 1] = k1_to_f32<DT>((unsigned short)(kv[j] >> 16)) * k_inv;
            vf[2 * j] = k1_to_f32<DT>((unsigned short)(vv[j] & 0xffffu)) * v_inv; vf[2 * j + 1] = k1_to_f32<DT>((unsigned short)(vv[j] >> 16)) * v_inv;
        }
        k_cache[dst] = u32x2{pack4_fp8_sat(kf[0], kf[1], kf[2], kf[3]), pack4_fp8_sat(kf[4], kf[5], kf[6], kf[7])};
        v_cache[dst] = u32x2{pack4_fp8_sat(vf[0], vf[1], vf[2], vf[3]), pack4_fp8_sat(vf[4], vf[5], vf[6], vf[7])};
    }
}

// ------------------------------------------------------------------------------------------------ K1 (fp32)
// Exact-fp32 variant for small parity runs (reproducing the reference's fp32 CPU token sequences on the GPU): one wave64 per
// (batch, head, query row), two passes over the visible keys, fp32 FMA dot products.  Same visibility rule as k1_partial.
__global__ __launch_bounds__(64) void k1_f32(const float *__restrict__ q, const float *__restrict__ kc, const float *__restrict__ vc,
                                             float *__restrict__ out, int n_rows, int H, int H_kv, int D, int S_max,
                                             const int *__restrict__ key_start, const sjd_iter_params *__restrict__ params, int kv_len_arg)
{
    extern __shared__ float sc[];                     // scores of the visible keys
    const int row = blockIdx.x, head = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    int kv_len = kv_len_arg, n_total = n_rows;
    if (params) sjdi_kv_rows(params, b, &kv_len, &n_total);
    float *o = out + (((size_t)b * n_rows + row) * H + head) * D;
    if (row >= n_total) { for (int d = lane; d < D; d += 64) o[d] = 0.0f; return; }
    const int hkv = head / (H / H_kv);
    const int kstart = key_start ? key_start[b] : 0, kend = kv_len + row + 1;       // visible keys [kstart, kend)
    const float *qr = q + (((size_t)b * n_rows + row) * H + head) * D;
    const float *kb = kc + ((size_t)b * H_kv + hkv) * (size_t)S_max * D;
    const float *vb = vc + ((size_t)b * H_kv + hkv) * (size_t)S_max * D;
    const float scale = 1.0f / sqrtf((float)D);
    float mx = -INFINITY;
    for (int j = kstart + lane; j < kend; j += 64) {
        float s = 0.0f;
        for (int d = 0; d < D; ++d) s = fmaf(qr[d], kb[(size_t)j * D + d], s);
        s *= scale;
        sc[j - kstart] = s;
        mx = fmaxf(mx, s);
    }
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    float sum = 0.0f;
    for (int j = kstart + lane; j < kend; j += 64) { float e = expf(sc[j - kstart] - mx); sc[j - kstart] = e; sum += e; }
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    __syncthreads();
    const float inv = (kend > kstart && sum > 0.0f) ? 1.0f / sum : 0.0f;
    for (int d = lane; d < D; d += 64) {
        float acc = 0.0f;
        for (int j = kstart; j < kend; ++j) acc = fmaf(sc[j - kstart], vb[(size_t)j * D + d], acc);
        o[d] = acc * inv;
    }
}

// ------------------------------------------------------------------------------------------------ K3
__global__ void k3_kv_append(const u32x4 *__restrict__ k_new, const u32x4 *__restrict__ v_new, u32x4 *__restrict__ k_cache,
                             u32x4 *__restrict__ v_cache, int B, int n_rows, int H_kv, int D8, int S_max,
                             const sjd_iter_params *__restrict__ params, int kv_len_arg)
{
    const size_t total = (size_t)B * n_rows * H_kv * D8;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int d = i % D8;
        const int h = (i / D8) % H_kv;
        const int r = (i / ((size_t)D8 * H_kv)) % n_rows;
        const int b = i / ((size_t)D8 * H_kv * n_rows);
        int kv_len = kv_len_arg, n_unused_ = 0;
        if (params) sjdi_kv_rows(params, b, &kv_len, &n_unused_);
        if (kv_len + r >= S_max) continue;
        const size_t dst = (((size_t)b * H_kv + h) * S_max + (kv_len + r)) * D8 + d;
        k_cache[dst] = k_new[i];
        v_cache[dst] = v_new[i];
    }
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" int sjd_kv_append(const void *k_new, const void *v_new, void *k_cache, void *v_cache, int B, int n_rows, int H_kv, int D,
                             int S_max, int dtype, const sjd_iter_params *params, int kv_len, void *stream)
{
    if (!k_new || !v_new || !k_cache || !v_cache || B < 1 || n_rows < 1 || H_kv < 1 || (D % 8) != 0 || S_max < 1) return SJD_ERR_BAD_ARG;
    if (dtype == SJD_DTYPE_F32) D *= 2;              // rows are copied as 16-byte pieces: an fp32 row is 2x as many
    const size_t total = (size_t)B * n_rows * H_kv * (D / 8);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k3_kv_append, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const u32x4 *)k_new, (const u32x4 *)v_new,
                       (u32x4 *)k_cache, (u32x4 *)v_cache, B, n_rows, H_kv, D / 8, S_max, params, kv_len);
    return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
}

extern "C" int64_t sjd_attention_workspace_bytes(int B, int H, int n_rows, int D, int n_split)
{
    const int64_t n_chunks = (n_rows + K1_ROWS - 1) / K1_ROWS;
    return (int64_t)B * H * n_chunks * n_split * K1_ROWS * (D + 2) * (int64_t)sizeof(float);
}

// what follows K1's partial launch, over 16-bit and fp8 caches alike: nothing when the partial kernel wrote the output itself (one key split,
// or the splits merged by their last workgroup), else k1_combine.  ev1 closes the partial kernel's interval (sjd_draft_window_attention_ex).
template <int DT, int D>
static int k1_finish(bool out_written, const float *ws_o, const float *ws_ml, void *out, int B, int n_rows, int H, int n_chunks, int n_split,
                     const int32_t *key_start, const sjd_iter_params *params, int kv_len, hipStream_t stream, hipEvent_t ev1 = nullptr)
{
    if (ev1) (void)hipEventRecord(ev1, stream);
    if (hipGetLastError() != hipSuccess) return SJD_ERR_LAUNCH;
    if (out_written) return SJD_OK;
    hipLaunchKernelGGL((k1_combine<DT, D>), dim3(n_chunks, H, B), dim3(256), 0, stream, ws_o, ws_ml, (unsigned short *)out, n_rows, H,
                       n_split, n_chunks, params, key_start, kv_len);
    return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
}

// One ladder: the column split (k1_dsplit, chosen by the colsplit entry points) -> the LDS-DMA ring kernel for the shapes whose rows share
// key tiles (8 or 4 (head, chunk) pairs; four slots = three tiles of 16 KiB in flight per workgroup, profiles/r4_k1_ring_halves.txt) ->
// k1_partial with eight waves (two per SIMD, the eight key-parts merged in LDS: profiles/r2_k1_waves_splits.jsonl), then k1_finish.
// DL: the logical head dim of the softmax scale (SJD_K1_HEAD_DIM_100: D = 128 storage, DL = 100), passed through to every kernel.
// The experimental library keeps two alternative forms that tests compare against (sjd_switches.h).
template <int DT, int D, int DL = D>
static int launch_attention(const void *q, const void *kc, const void *vc, void *out, int B, int n_rows, int H, int H_kv, int S_max,
                            const int32_t *key_start, const sjd_iter_params *params, int kv_len, int n_split, void *workspace,
                            hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1, unsigned *ticket = nullptr, bool colsplit = false)
{
    static_assert(DL == D || D == 128, "a logical head dim is served at storage D = 128 only");
    const int n_chunks = (n_rows + K1_ROWS - 1) / K1_ROWS;
    float *ws_o = (float *)workspace;
    float *ws_ml = ws_o + (size_t)B * H * n_chunks * n_split * K1_ROWS * D;
    if (ev0) (void)hipEventRecord(ev0, stream);
    const int pairs = (H / H_kv) * n_chunks;           // (q head of a group, row chunk) pairs that read the same K/V tiles
    const bool shared = D == 128 && (pairs == 4 || pairs == 8) && (H / H_kv > 1 || n_chunks > 1);
    // a single key split needs no combine: k1_partial normalises and writes the 16-bit output directly
    bool one_split_direct = n_split == 1;
#ifdef SJD_EXPERIMENTAL
    if (sjd_switches::get().k1_no_direct) one_split_direct = false;
#endif
    unsigned short *direct = (!shared && one_split_direct) ? (unsigned short *)out : nullptr;
    // round 3: the splits are merged by the last of their workgroups to finish (k1_merge_publish): no k1_combine launch.  `ticket`: one
    // zero-initialised uint32 per (batch, kv head, chunk), handed over by the caller (sjd_draft_window_attention_merged); they re-arm themselves.
    unsigned short *merge_out = (ticket && !shared && !direct) ? (unsigned short *)out : nullptr;
    if (colsplit && !(D == 128 && H == H_kv)) return SJD_ERR_UNSUPPORTED;
    if (DL != D && H != H_kv) return SJD_ERR_UNSUPPORTED;
    if constexpr (D == 128) {
        // round 4: the multi-head window without key splits -- four workgroups per (batch, head) split the OUTPUT COLUMNS (k1_dsplit): one
        // launch, no workspace, no combine
        if (colsplit) {
            hipLaunchKernelGGL((k1_dsplit<DT, D, 8, 4, DL>), dim3(4 * n_chunks * H * B), dim3(512), 0, stream, (const unsigned short *)q,
                               (const unsigned short *)kc, (const unsigned short *)vc, params, key_start, (unsigned short *)out, n_rows, H, H_kv,
                               S_max, kv_len, n_chunks, B);
            if (ev1) (void)hipEventRecord(ev1, stream);
            return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
        }
        if (shared) {
#ifdef SJD_EXPERIMENTAL        // SJD_K1_RING=0: the round-3 shared-tile kernel the ring kernel replaced (its blob-array test runs it)
            if (!sjd_switches::get().k1_ring) {
                if constexpr (DL != D) return SJD_ERR_UNSUPPORTED;
                else if (pairs == 8)
                    hipLaunchKernelGGL((k1_partial_shared<DT, D, 8, 3>), dim3(n_split, H_kv, B), dim3(512), 0, stream, (const unsigned short *)q,
                                       (const unsigned short *)kc, (const unsigned short *)vc, params, key_start, ws_o, ws_ml, n_rows, H, H_kv, S_max,
                                       kv_len, n_split, n_chunks);
                else
                    hipLaunchKernelGGL((k1_partial_shared<DT, D, 4, 3>), dim3(n_split, H_kv, B), dim3(256), 0, stream, (const unsigned short *)q,
                                       (const unsigned short *)kc, (const unsigned short *)vc, params, key_start, ws_o, ws_ml, n_rows, H, H_kv, S_max,
                                       kv_len, n_split, n_chunks);
                return k1_finish<DT, D>(false, ws_o, ws_ml, out, B, n_rows, H, n_chunks, n_split, key_start, params, kv_len, stream, ev1);
            }
#endif
            // round 4: the LDS-DMA ring kernel (sjd_attention_ring.h); its LDS is the ring of four slots, then the waves' Q rows
            constexpr size_t ring = (size_t)4 * 2 * K1_KT * D * 2, lds8 = ring + (size_t)8 * K1_ROWS * D * 2, lds4 = ring + (size_t)4 * K1_ROWS * D * 2;
            if (pairs == 8) {
                (void)hipFuncSetAttribute((const void *)k1_partial_ring<DT, D, 8, 4, DL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds8);
                hipLaunchKernelGGL((k1_partial_ring<DT, D, 8, 4, DL>), dim3(n_split, H_kv, B), dim3(512), lds8, stream, (const unsigned short *)q,
                                   (const unsigned short *)kc, (const unsigned short *)vc, params, key_start, ws_o, ws_ml, n_rows, H, H_kv, S_max,
                                   kv_len, n_split, n_chunks, B);
            } else {
                (void)hipFuncSetAttribute((const void *)k1_partial_ring<DT, D, 4, 4, DL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds4);
                hipLaunchKernelGGL((k1_partial_ring<DT, D, 4, 4, DL>), dim3(n_split, H_kv, B), dim3(256), lds4, stream, (const unsigned short *)q,
                                   (const unsigned short *)kc, (const unsigned short *)vc, params, key_start, ws_o, ws_ml, n_rows, H, H_kv, S_max,
                                   kv_len, n_split, n_chunks, B);
            }
            return k1_finish<DT, D>(false, ws_o, ws_ml, out, B, n_rows, H, n_chunks, n_split, key_start, params, kv_len, stream, ev1);
        }
    }
    hipLaunchKernelGGL((k1_partial<DT, D, 8, DL>), dim3(n_chunks * n_split, H_kv, B), dim3(512), 0, stream, (const unsigned short *)q,
                       (const unsigned short *)kc, (const unsigned short *)vc, params, key_start, ws_o, ws_ml, direct, n_rows, H, H_kv, S_max,
                       kv_len, n_split, n_chunks, merge_out, ticket);
    return k1_finish<DT, D>(direct || merge_out, ws_o, ws_ml, out, B, n_rows, H, n_chunks, n_split, key_start, params, kv_len, stream, ev1);
}

static int k1_dispatch(const void *q, const void *k_cache, const void *v_cache, void *out, int B, int n_rows,
                       int H, int H_kv, int D, int S_max, int dtype, const int32_t *key_start,
                       const sjd_iter_params *params, int kv_len, int n_split, void *workspace, void *stream,
                       void *ev_start, void *ev_stop, unsigned *ticket, bool colsplit = false)
{
    // the mode bit of `dtype`: SJD_K1_HEAD_DIM_100 -- heads stored 128 wide with zero pad columns 100..127, softmax scale 1/sqrt(100)
    if (dtype & ~(SJD_DTYPE_MASK | SJD_K1_HEAD_DIM_100)) return SJD_ERR_UNSUPPORTED;
    const bool dl100 = (dtype & SJD_K1_HEAD_DIM_100) != 0;
    dtype &= SJD_DTYPE_MASK;
    if (dl100 && (D != 128 || H != H_kv || (dtype != SJD_DTYPE_BF16 && dtype != SJD_DTYPE_F16))) return SJD_ERR_UNSUPPORTED;
    if (!q || !k_cache || !v_cache || !out || (!workspace && !colsplit) || B < 1 || n_rows < 1 || H < 1 || H_kv < 1 || n_split < 1) return SJD_ERR_BAD_ARG;
    if (H % H_kv != 0 || (S_max % K1_KT) != 0) return SJD_ERR_BAD_ARG;
    if (dtype == SJD_DTYPE_F32) {
        if (colsplit) return SJD_ERR_UNSUPPORTED;
        if ((size_t)S_max * sizeof(float) > 160 * 1024) return SJD_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(k1_f32, dim3(n_rows, H, B), dim3(64), (size_t)S_max * sizeof(float), (hipStream_t)stream, (const float *)q,
                           (const float *)k_cache, (const float *)v_cache, (float *)out, n_rows, H, H_kv, D, S_max, key_start, params, kv_len);
        return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
    }
    const int G = H / H_kv;
    // group 8 (the 30B-class Chameleon, 64 / 8 heads): one draft window of <= 16 rows is 8 (head, chunk) pairs -- the LDS-DMA ring kernel with
    // eight waves; 17..32 rows (two chunks) run on k1_partial with eight waves, one per head of the group (key parts 1)
    if (!(G == 1 || G == 2 || G == 4 || G == 8)) return SJD_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (dl100) {
        if (dtype == SJD_DTYPE_BF16) return launch_attention<SJD_DTYPE_BF16, 128, 100>(q, k_cache, v_cache, out, B, n_rows, H, H_kv, S_max, key_start, params, kv_len, n_split, workspace, s, (hipEvent_t)ev_start, (hipEvent_t)ev_stop, ticket, colsplit);
        return launch_attention<SJD_DTYPE_F16, 128, 100>(q, k_cache, v_cache, out, B, n_rows, H, H_kv, S_max, key_start, params, kv_len, n_split, workspace, s, (hipEvent_t)ev_start, (hipEvent_t)ev_stop, ticket, colsplit);
    }
#define SJD_K1_CASE(DT_, D_) \
    if (dtype == DT_ && D == D_) return launch_attention<DT_, D_>(q, k_cache, v_cache, out, B, n_rows, H, H_kv, S_max, key_start, params, kv_len, n_split, workspace, s, (hipEvent_t)ev_start, (hipEvent_t)ev_stop, ticket, colsplit);
    SJD_K1_CASE(SJD_DTYPE_BF16, 128)
    SJD_K1_CASE(SJD_DTYPE_BF16, 64)
    SJD_K1_CASE(SJD_DTYPE_F16, 128)
    SJD_K1_CASE(SJD_DTYPE_F16, 64)
#undef SJD_K1_CASE
    return SJD_ERR_UNSUPPORTED;
}

extern "C" int sjd_draft_window_attention_ex(const void *q, const void *k_cache, const void *v_cache, void *out, int B, int n_rows,
                                             int H, int H_kv, int D, int S_max, int dtype, const int32_t *key_start,
                                             const sjd_iter_params *params, int kv_len, int n_split, void *workspace, void *stream,
                                             void *ev_start, void *ev_stop)
{
    return k1_dispatch(q, k_cache, v_cache, out, B, n_rows, H, H_kv, D, S_max, dtype, key_start, params, kv_len, n_split, workspace, stream,
                       ev_start, ev_stop, nullptr);
}

#ifdef SJD_EXPERIMENTAL        // round-3 option
// K1 in ONE launch: the key splits are merged by the last of their workgroups to finish instead of by a second kernel (k1_merge_publish).
// tickets: B * H_kv * ceil(n_rows / 16) zero-initialised uint32, private to launches that cannot overlap (they re-arm themselves).
// Grouped-query / multi-chunk shapes served by the shared-tile kernel keep the two-kernel form (tickets unused).
extern "C" int sjd_draft_window_attention_merged(const void *q, const void *k_cache, const void *v_cache, void *out, int B, int n_rows,
                                                 int H, int H_kv, int D, int S_max, int dtype, const int32_t *key_start,
                                                 const sjd_iter_params *params, int kv_len, int n_split, void *workspace, uint32_t *tickets,
                                                 void *stream, void *ev_start, void *ev_stop)
{
    if (!tickets) return SJD_ERR_BAD_ARG;
    return k1_dispatch(q, k_cache, v_cache, out, B, n_rows, H, H_kv, D, S_max, dtype, key_start, params, kv_len, n_split, workspace, stream,
                       ev_start, ev_stop, (unsigned *)tickets);
}

#endif  // SJD_EXPERIMENTAL
extern "C" int sjd_draft_window_attention(const void *q, const void *k_cache, const void *v_cache, void *out, int B, int n_rows, int H,
                                          int H_kv, int D, int S_max, int dtype, const int32_t *key_start,
                                          const sjd_iter_params *params, int kv_len, int n_split, void *workspace, void *stream)
{
    return sjd_draft_window_attention_ex(q, k_cache, v_cache, out, B, n_rows, H, H_kv, D, S_max, dtype, key_start, params, kv_len,
                                         n_split, workspace, stream, nullptr, nullptr);
}

// K1 without key splits (round 4): the four workgroups of a (batch, head) split the OUTPUT COLUMNS -- each scores all keys and multiplies
// them with its 32 columns of V -- and write the normalised output themselves: ONE launch, no workspace, no combine.  Multi-head attention
// (H == H_kv), D = 128, 16-bit caches; SJD_ERR_UNSUPPORTED otherwise.  Faster than the key split + combine while a CU's share of the K stream
// is short (kv_len below ~750 keys, profiles/r4_k1_dsplit_ab.txt); the caller picks per launch (sjd_amd.ops.HipWindowAttention.choose_regime).
extern "C" int sjd_draft_window_attention_colsplit(const void *q, const void *k_cache, const void *v_cache, void *out, int B, int n_rows, int H,
                                                   int H_kv, int D, int S_max, int dtype, const int32_t *key_start,
                                                   const sjd_iter_params *params, int kv_len, void *stream)
{
    return k1_dispatch(q, k_cache, v_cache, out, B, n_rows, H, H_kv, D, S_max, dtype, key_start, params, kv_len, 1, nullptr, stream, nullptr, nullptr,
                       nullptr, true);
}

extern "C" int sjd_kv_append_fp8(const void *k_new, const void *v_new, void *k_cache, void *v_cache, int B, int n_rows, int H_kv, int D,
                                 int S_max, int dtype, float k_scale, float v_scale, int head_major, const sjd_iter_params *params, int kv_len,
                                 void *stream)
{
    if (!k_new || !v_new || !k_cache || !v_cache || B < 1 || n_rows < 1 || H_kv < 1 || (D % 8) != 0 || S_max < 1 || !(k_scale > 0.f) || !(v_scale > 0.f))
        return SJD_ERR_BAD_ARG;
    const size_t total = (size_t)B * n_rows * H_kv * (D / 8);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SJD_DTYPE_BF16)
        hipLaunchKernelGGL(k3_kv_append_fp8<SJD_DTYPE_BF16>, dim3(blocks), dim3(256), 0, s, (const u32x4 *)k_new, (const u32x4 *)v_new, (u32x2 *)k_cache,
                           (u32x2 *)v_cache, B, n_rows, H_kv, D / 8, S_max, params, kv_len, 1.0f / k_scale, 1.0f / v_scale, head_major);
    else if (dtype == SJD_DTYPE_F16)
        hipLaunchKernelGGL(k3_kv_append_fp8<SJD_DTYPE_F16>, dim3(blocks), dim3(256), 0, s, (const u32x4 *)k_new, (const u32x4 *)v_new, (u32x2 *)k_cache,
                           (u32x2 *)v_cache, B, n_rows, H_kv, D / 8, S_max, params, kv_len, 1.0f / k_scale, 1.0f / v_scale, head_major);
    else return SJD_ERR_UNSUPPORTED;
    return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
}

template <int DT, int D>
static int launch_attention_fp8(const void *q, const void *kc, const void *vc, void *out, int B, int n_rows, int H, int H_kv, int S_max,
                                float k_scale, float v_scale, const int32_t *key_start, const sjd_iter_params *params, int kv_len, int n_split,
                                void *workspace, hipStream_t stream, unsigned *ticket = nullptr, bool colsplit = false)
{
    const int n_chunks = (n_rows + K1_ROWS - 1) / K1_ROWS;
    if (colsplit) {
        if constexpr (D == 128) {
            if (H != H_kv) return SJD_ERR_UNSUPPORTED;
            hipLaunchKernelGGL((k1_dsplit_fp8<DT, D, 8, 4>), dim3(4 * n_chunks * H * B), dim3(512), 0, stream, (const unsigned short *)q,
                               (const unsigned char *)kc, (const unsigned char *)vc, params, key_start, (unsigned short *)out, n_rows, H, H_kv,
                               S_max, kv_len, n_chunks, B, k_scale, v_scale);
            return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
        }
        return SJD_ERR_UNSUPPORTED;
    }
    float *ws_o = (float *)workspace;
    float *ws_ml = ws_o + (size_t)B * H * n_chunks * n_split * K1_ROWS * D;
    bool one_split_direct = n_split == 1;      // one key split: no combine launch
#ifdef SJD_EXPERIMENTAL
    if (sjd_switches::get().k1_no_direct) one_split_direct = false;
#endif
    unsigned short *direct = one_split_direct ? (unsigned short *)out : nullptr;
    unsigned short *merge_out = (ticket && !direct) ? (unsigned short *)out : nullptr;      // splits merged by their last workgroup
    hipLaunchKernelGGL((k1_partial_fp8<DT, D, 8>), dim3(n_chunks * n_split, H_kv, B), dim3(512), 0, stream, (const unsigned short *)q,
                       (const unsigned char *)kc, (const unsigned char *)vc, params, key_start, ws_o, ws_ml, direct, n_rows, H, H_kv, S_max,
                       kv_len, n_split, n_chunks, k_scale, v_scale, merge_out, ticket);
    return k1_finish<DT, D>(direct || merge_out, ws_o, ws_ml, out, B, n_rows, H, n_chunks, n_split, key_start, params, kv_len, stream);
}

static int k1_dispatch_fp8(const void *q, const void *k_cache, const void *v_cache, void *out, int B, int n_rows, int H,
                           int H_kv, int D, int S_max, int dtype, float k_scale, float v_scale, const int32_t *key_start,
                           const sjd_iter_params *params, int kv_len, int n_split, void *workspace, void *stream, unsigned *ticket,
                           bool colsplit = false)
{
    if (dtype & ~SJD_DTYPE_MASK) return SJD_ERR_UNSUPPORTED;      // (SJD_K1_HEAD_DIM_100 is served over 16-bit caches only)
    if (!q || !k_cache || !v_cache || !out || (!workspace && !colsplit) || B < 1 || n_rows < 1 || H < 1 || H_kv < 1 || n_split < 1) return SJD_ERR_BAD_ARG;
    if (H % H_kv != 0 || (S_max % K1_KT) != 0 || !(k_scale > 0.f) || !(v_scale > 0.f)) return SJD_ERR_BAD_ARG;
    const int G = H / H_kv;
    if (!(G == 1 || G == 2 || G == 4)) return SJD_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
#define SJD_K1F8_CASE(DT_, D_) \
    if (dtype == DT_ && D == D_) return launch_attention_fp8<DT_, D_>(q, k_cache, v_cache, out, B, n_rows, H, H_kv, S_max, k_scale, v_scale, key_start, params, kv_len, n_split, workspace, s, ticket, colsplit);
    SJD_K1F8_CASE(SJD_DTYPE_BF16, 128)
    SJD_K1F8_CASE(SJD_DTYPE_BF16, 64)
    SJD_K1F8_CASE(SJD_DTYPE_F16, 128)
    SJD_K1F8_CASE(SJD_DTYPE_F16, 64)
#undef SJD_K1F8_CASE
    return SJD_ERR_UNSUPPORTED;
}

extern "C" int sjd_draft_window_attention_fp8(const void *q, const void *k_cache, const void *v_cache, void *out, int B, int n_rows, int H,
                                              int H_kv, int D, int S_max, int dtype, float k_scale, float v_scale, const int32_t *key_start,
                                              const sjd_iter_params *params, int kv_len, int n_split, void *workspace, void *stream)
{
    return k1_dispatch_fp8(q, k_cache, v_cache, out, B, n_rows, H, H_kv, D, S_max, dtype, k_scale, v_scale, key_start, params, kv_len, n_split,
                           workspace, stream, nullptr);
}

#ifdef SJD_EXPERIMENTAL        // round-3 option
extern "C" int sjd_draft_window_attention_fp8_merged(const void *q, const void *k_cache, const void *v_cache, void *out, int B, int n_rows, int H,
                                                     int H_kv, int D, int S_max, int dtype, float k_scale, float v_scale, const int32_t *key_start,
                                                     const sjd_iter_params *params, int kv_len, int n_split, void *workspace, uint32_t *tickets,
                                                     void *stream)
{
    if (!tickets) return SJD_ERR_BAD_ARG;
    return k1_dispatch_fp8(q, k_cache, v_cache, out, B, n_rows, H, H_kv, D, S_max, dtype, k_scale, v_scale, key_start, params, kv_len, n_split,
                           workspace, stream, (unsigned *)tickets);
}

#endif  // SJD_EXPERIMENTAL
// sjd_draft_window_attention_colsplit over an fp8 (e4m3) cache: a key row is 128 bytes, so the column split stays ahead up to ~1500 keys
extern "C" int sjd_draft_window_attention_fp8_colsplit(const void *q, const void *k_cache, const void *v_cache, void *out, int B, int n_rows, int H,
                                                       int H_kv, int D, int S_max, int dtype, float k_scale, float v_scale,
                                                       const int32_t *key_start, const sjd_iter_params *params, int kv_len, void *stream)
{
    return k1_dispatch_fp8(q, k_cache, v_cache, out, B, n_rows, H, H_kv, D, S_max, dtype, k_scale, v_scale, key_start, params, kv_len, 1, nullptr,
                           stream, nullptr, true);
}

extern "C" void *sjd_event_create(void)
{
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? (void *)e : nullptr;
}
extern "C" void sjd_event_destroy(void *ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); }
extern "C" int sjd_event_synchronize(void *ev) { return hipEventSynchronize((hipEvent_t)ev) == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH; }
extern "C" float sjd_event_elapsed_ms(void *ev_start, void *ev_stop)
{
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, (hipEvent_t)ev_start, (hipEvent_t)ev_stop) != hipSuccess) return -1.0f;
    return ms;
}

#ifdef SJD_TRACE
extern "C" int sjd_debug_trace_k1c(unsigned long long *host_out, int n_wg)
{
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_k1c_trace), (size_t)n_wg * 4 * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
extern "C" int sjd_debug_trace_k1(unsigned long long *host_out, int n_wg)
{
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_k1_trace), (size_t)n_wg * 8 * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
