// sjd_glue.hip -- fused element-wise glue of the draft-window forward (gfx950).
//
// rocprofv3 of the first end-to-end bench (profiles/r1a_*) showed ~1300 tiny ATen element-wise launches per SJD
// iteration (RMSNorm as pow/mean/add/rsqrt/mul, per-head QK-LayerNorm, rotate_half RoPE as neg/cat/mul/mul/add, dtype
// copies, SiLU, residual adds) costing more wall time than the weight-streaming GEMMs.  These three kernels replace them:
//
//   F1 sjd_add_rmsnorm        h += delta (optional);  y = w * bf16(h * rsqrt(mean(h^2)+eps))
//                             <- ChameleonRMSNorm (reference modeling_chameleon.py:59-73) + the residual add of the
//                                decoder layer (:637, :643)
//   F2 sjd_qknorm_rope_append per (token, head): LayerNorm over head_dim with per-head gamma/beta (optional), RoPE
//                             (rotate-half form, fp32 angles), q -> q_out, k/v -> static KV cache rows [kv_len + i]
//                             <- ChameleonLayerNorm (:198-219), apply_rotary_pos_emb (:144-178), DynamicCache.update
//                                (:547);  this is K3 fused into the projection epilogue
//   F3 sjd_silu_mul           y = silu(gate) * up on a fused [M, 2I] gate|up projection  <- ChameleonMLP (:193-195)
//
// All are HBM/latency bound on [32 x 4096]-sized activations: 16-byte vector loads, one wave64 per row / head.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/sjd_hip.h"

// phase timestamps of the glue kernels (tools/phase_trace.py, -DSJD_TRACE; compiled out otherwise): slot 0 F1r, 1 F2, 2 F3
#ifdef SJD_TRACE
__device__ unsigned long long g_glue_trace[3][4096][4];
#define SJD_TRG(k, i) do { if (threadIdx.x == 0) g_glue_trace[k][((blockIdx.y * gridDim.x) + blockIdx.x) & 4095][i] = wall_clock64(); } while (0)
extern "C" int sjd_debug_trace_glue(int kind, unsigned long long *host_out, int n_wg)
{
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_glue_trace), (size_t)n_wg * 4 * sizeof(unsigned long long),
                               (size_t)kind * 4096 * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#else
#define SJD_TRG(k, i) do { } while (0)
#endif

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

#include "sjd_mlp_epilogue.h"
#include "sjd_fp8.h"
#ifdef SJD_EXPERIMENTAL
#include "sjd_l2_prefetch.h"
#endif

template <int DT> struct Cvt;
template <> struct Cvt<SJD_DTYPE_BF16> {
    static __device__ __forceinline__ float to_f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
    static __device__ __forceinline__ unsigned short from_f(float x)
    {
        unsigned u = __float_as_uint(x);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (unsigned short)(u >> 16);
    }
};
template <> struct Cvt<SJD_DTYPE_F16> {
    static __device__ __forceinline__ float to_f(unsigned short h) { return (float)(*reinterpret_cast<_Float16 *>(&h)); }
    static __device__ __forceinline__ unsigned short from_f(float x)
    {
        _Float16 h = (_Float16)x;
        return *reinterpret_cast<unsigned short *>(&h);
    }
};

template <int DT> __device__ __forceinline__ void unpack8(u32x4 v, float (&f)[8])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = Cvt<DT>::to_f((unsigned short)(v[i] & 0xffffu));
        f[2 * i + 1] = Cvt<DT>::to_f((unsigned short)(v[i] >> 16));
    }
}
template <int DT> __device__ __forceinline__ u32x4 pack8(const float (&f)[8])
{
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (unsigned)Cvt<DT>::from_f(f[2 * i]) | ((unsigned)Cvt<DT>::from_f(f[2 * i + 1]) << 16);
    return v;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ------------------------------------------------------------------------------------------------ F1
// one 256-thread workgroup per row; hidden % 8 == 0 and hidden <= 256*8*MAXV
// `part` (optional): fp32 split-K partials [n_chunks, 32, hidden] of the producing G1 projection; delta = dtype(sum_c part[c]).
// POST (swin-norm layers, ChameleonSwinDecoderLayer): the norm applies to the sublayer output, not to h --
//   h = dtype(h + dtype(w * dtype(delta * rsqrt(mean(delta^2) + eps))))   (delta or part required, y is not written)
template <int DT, bool POST = false>
__global__ __launch_bounds__(256) void f1_add_rmsnorm(unsigned short *__restrict__ h, const unsigned short *__restrict__ delta,
                                                      const unsigned short *__restrict__ w, unsigned short *__restrict__ y,
                                                      int hidden, float eps, const float *__restrict__ part, int n_chunks, int prows)
{
    __shared__ float red[4];
    const int row = blockIdx.x;
    unsigned short *hr = h + (size_t)row * hidden;
    const unsigned short *dr = delta ? delta + (size_t)row * hidden : nullptr;
    constexpr int MAXV = 4;
    float x[MAXV][8];
    float hp[POST ? MAXV : 1][8];                  // POST: h itself (x holds the rounded sublayer output)
    float ss = 0.f;
    int nv = 0;
    for (int c = threadIdx.x * 8; c < hidden && nv < MAXV; c += 256 * 8, ++nv) {
        unpack8<DT>(*reinterpret_cast<const u32x4 *>(hr + c), POST ? hp[POST ? nv : 0] : x[nv]);
        if (dr || part) {
            float d[8];
            if (part) {
#pragma unroll
                for (int j = 0; j < 8; ++j) d[j] = 0.f;
                const size_t cstride = (size_t)prows * hidden;
                const float *p0 = part + (size_t)row * hidden + c;
                int cc = 0;
                for (; cc + 4 <= n_chunks; cc += 4) {       // issue the loads of four chunks before any add (L2 latency overlap)
                    float4 a[4], b[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 *pp = reinterpret_cast<const float4 *>(p0 + (size_t)(cc + q) * cstride);
                        a[q] = pp[0]; b[q] = pp[1];
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        d[0] += a[q].x; d[1] += a[q].y; d[2] += a[q].z; d[3] += a[q].w;
                        d[4] += b[q].x; d[5] += b[q].y; d[6] += b[q].z; d[7] += b[q].w;
                    }
                }
                for (; cc < n_chunks; ++cc) {
                    const float4 *pp = reinterpret_cast<const float4 *>(p0 + (size_t)cc * cstride);
                    const float4 a = pp[0], b = pp[1];
                    d[0] += a.x; d[1] += a.y; d[2] += a.z; d[3] += a.w; d[4] += b.x; d[5] += b.y; d[6] += b.z; d[7] += b.w;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) d[j] = Cvt<DT>::to_f(Cvt<DT>::from_f(d[j]));     // the projection output rounds to the activation dtype
            } else {
                unpack8<DT>(*reinterpret_cast<const u32x4 *>(dr + c), d);
            }
            if constexpr (POST) {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[nv][j] = d[j];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[nv][j] = Cvt<DT>::to_f(Cvt<DT>::from_f(x[nv][j] + d[j]));   // residual add rounds to the activation dtype
                *reinterpret_cast<u32x4 *>(hr + c) = pack8<DT>(x[nv]);
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += x[nv][j] * x[nv][j];
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float tot = red[0] + red[1] + red[2] + red[3];
    const float inv = rsqrtf(tot / (float)hidden + eps);
    nv = 0;
    for (int c = threadIdx.x * 8; c < hidden && nv < MAXV; c += 256 * 8, ++nv) {
#pragma clang fp contract(off)
        // (fp16: the compiler otherwise demotes dtype(a * b) + c to ONE half-precision FMA and the documented rounding of the product is gone --
        // tests/test_gpu_glue_bounds.py)
        float wv[8], o[8];
        unpack8<DT>(*reinterpret_cast<const u32x4 *>(w + c), wv);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = wv[j] * Cvt<DT>::to_f(Cvt<DT>::from_f(x[nv][j] * inv));   // weight * hidden.to(dtype)
        if constexpr (POST) {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = Cvt<DT>::to_f(Cvt<DT>::from_f(hp[nv][j] + Cvt<DT>::to_f(Cvt<DT>::from_f(o[j]))));   // residual + norm, both rounded
            *reinterpret_cast<u32x4 *>(hr + c) = pack8<DT>(o);
        } else {
            *reinterpret_cast<u32x4 *>(y + (size_t)row * hidden + c) = pack8<DT>(o);
        }
    }
}

// F1 for a G1 producer: the residual delta arrives as fp32 split-K partials [n_chunks, 32, hidden].  Only `rows` (<= 32)
// workgroups exist, so the kernel is bound by how many loads ONE CU keeps in flight: 1024 threads, 4 columns each per 4096-column
// stripe, and all chunk loads of a stripe are issued before the first add.  POST: the swin-norm form of f1_add_rmsnorm (h is written last).
template <int DT, bool POST = false>
__global__ __launch_bounds__(1024) void f1p_add_rmsnorm(unsigned short *__restrict__ h, const float *__restrict__ part, int n_chunks,
                                                        const unsigned short *__restrict__ w, unsigned short *__restrict__ y,
                                                        int hidden, float eps, int prows)
{
    __shared__ float red[16];
    constexpr int MAXS = 4;                        // stripes of 4096 columns (hidden <= 16384)
    constexpr int MAXC = 16;
    const int row = blockIdx.x;
    unsigned short *hr = h + (size_t)row * hidden;
    const size_t cstride = (size_t)prows * hidden;
    float x[MAXS][4];
    uint2 hkeep[POST ? MAXS : 1];                  // POST: h as loaded (x holds the rounded sublayer output)
    float ss = 0.f;
    int ns = 0;
    for (int c = threadIdx.x * 4; c < hidden && ns < MAXS; c += 4096, ++ns) {
        const uint2 hv = *reinterpret_cast<const uint2 *>(hr + c);
        if constexpr (POST) hkeep[ns] = hv;
        const float *p0 = part + (size_t)row * hidden + c;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
        for (int c0 = 0; c0 < n_chunks; c0 += MAXC) {
            float4 v[MAXC];
#pragma unroll
            for (int q = 0; q < MAXC; ++q)
                if (c0 + q < n_chunks) v[q] = *reinterpret_cast<const float4 *>(p0 + (size_t)(c0 + q) * cstride);
#pragma unroll
            for (int q = 0; q < MAXC; ++q)
                if (c0 + q < n_chunks) { d0 += v[q].x; d1 += v[q].y; d2 += v[q].z; d3 += v[q].w; }
        }
        const float hx[4] = {Cvt<DT>::to_f((unsigned short)(hv.x & 0xffffu)), Cvt<DT>::to_f((unsigned short)(hv.x >> 16)),
                             Cvt<DT>::to_f((unsigned short)(hv.y & 0xffffu)), Cvt<DT>::to_f((unsigned short)(hv.y >> 16))};
        const float dd[4] = {d0, d1, d2, d3};
        if constexpr (POST) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[ns][j] = Cvt<DT>::to_f(Cvt<DT>::from_f(dd[j]));                         // the sublayer output rounds to the activation dtype
                ss += x[ns][j] * x[ns][j];
            }
            (void)hx;
            continue;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dj = Cvt<DT>::to_f(Cvt<DT>::from_f(dd[j]));                       // projection output rounds to the activation dtype
            x[ns][j] = Cvt<DT>::to_f(Cvt<DT>::from_f(hx[j] + dj));                        // residual add rounds too
            ss += x[ns][j] * x[ns][j];
        }
        uint2 ho;
        ho.x = (unsigned)Cvt<DT>::from_f(x[ns][0]) | ((unsigned)Cvt<DT>::from_f(x[ns][1]) << 16);
        ho.y = (unsigned)Cvt<DT>::from_f(x[ns][2]) | ((unsigned)Cvt<DT>::from_f(x[ns][3]) << 16);
        *reinterpret_cast<uint2 *>(hr + c) = ho;
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) tot += red[i];
    const float inv = rsqrtf(tot / (float)hidden + eps);
    ns = 0;
    for (int c = threadIdx.x * 4; c < hidden && ns < MAXS; c += 4096, ++ns) {
#pragma clang fp contract(off)
        // (fp16: the compiler otherwise demotes dtype(a * b) + c to ONE half-precision FMA and the documented rounding of the product is gone --
        // tests/test_gpu_glue_bounds.py)
        const uint2 wv = *reinterpret_cast<const uint2 *>(w + c);
        const float ww[4] = {Cvt<DT>::to_f((unsigned short)(wv.x & 0xffffu)), Cvt<DT>::to_f((unsigned short)(wv.x >> 16)),
                             Cvt<DT>::to_f((unsigned short)(wv.y & 0xffffu)), Cvt<DT>::to_f((unsigned short)(wv.y >> 16))};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ww[j] * Cvt<DT>::to_f(Cvt<DT>::from_f(x[ns][j] * inv));
        if constexpr (POST) {                      // h + dtype(gain * norm), rounded like the reference's residual add
            const uint2 hv = hkeep[ns];
            const float hx[4] = {Cvt<DT>::to_f((unsigned short)(hv.x & 0xffffu)), Cvt<DT>::to_f((unsigned short)(hv.x >> 16)),
                                 Cvt<DT>::to_f((unsigned short)(hv.y & 0xffffu)), Cvt<DT>::to_f((unsigned short)(hv.y >> 16))};
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = hx[j] + Cvt<DT>::to_f(Cvt<DT>::from_f(o[j]));
        }
        uint2 yo;
        yo.x = (unsigned)Cvt<DT>::from_f(o[0]) | ((unsigned)Cvt<DT>::from_f(o[1]) << 16);
        yo.y = (unsigned)Cvt<DT>::from_f(o[2]) | ((unsigned)Cvt<DT>::from_f(o[3]) << 16);
        *reinterpret_cast<uint2 *>((POST ? hr : y + (size_t)row * hidden) + c) = yo;
    }
}

// F1r: only the residual half of F1, spread over (row, 512-column slice) workgroups: h += dtype(sum_c part[c]) (part optional) and
// the slice's sum of h^2.  With the RMSNorm gain folded into the next projection's packed weight (W' = W diag(gamma)) the norm
// reduces to one scale per row, which commutes with the projection and is applied by its consumer (F2 / F3 `row_sumsq`):
//   gamma * (h * r) @ W^T  ==  r * (h @ (W diag(gamma))^T),   r = rsqrt(mean(h^2) + eps)
template <int DT>
__device__ __forceinline__ void f1r_body(unsigned short *__restrict__ h, const float *__restrict__ part, int n_chunks,
                                         int hidden, int prows, float *__restrict__ out_sumsq)
{
    SJD_TRG(0, 0);
    __shared__ float red[2];
    const int row = blockIdx.x, c = blockIdx.y * 512 + threadIdx.x * 4;
    float ss = 0.f;
    if (c < hidden) {
        unsigned short *hp = h + (size_t)row * hidden + c;
        const uint2 hv = *reinterpret_cast<const uint2 *>(hp);
        float hx[4] = {Cvt<DT>::to_f((unsigned short)(hv.x & 0xffffu)), Cvt<DT>::to_f((unsigned short)(hv.x >> 16)),
                       Cvt<DT>::to_f((unsigned short)(hv.y & 0xffffu)), Cvt<DT>::to_f((unsigned short)(hv.y >> 16))};
        if (part) {
            const size_t cstride = (size_t)prows * hidden;
            const float *p0 = part + (size_t)row * hidden + c;
            float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
            // UNCONDITIONAL loads (a missing chunk re-reads the last one, its value is not added): behind a conditional load the
            // compiler waits with vmcnt(0) -- round 3 found this kernel at 4.0 us instead of 3.0 after an unrelated edit had made it
            // reuse destination registers between the eight conditional loads, i.e. eight HBM round trips in a row, 0.06 ms per step.
            // 9..16 chunks (the down projection's 15): ONE batch of sixteen -- two batches of eight were two round trips; same order of adds.
            if (n_chunks > 8 && n_chunks <= 16) {
                float4 v[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q] = *reinterpret_cast<const float4 *>(p0 + (size_t)min(q, n_chunks - 1) * cstride);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const bool on = q < n_chunks;
                    d0 += on ? v[q].x : 0.f; d1 += on ? v[q].y : 0.f; d2 += on ? v[q].z : 0.f; d3 += on ? v[q].w : 0.f;
                }
            } else
            for (int c0 = 0; c0 < n_chunks; c0 += 8) {           // issue the loads of eight chunks before the first add
                float4 v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = *reinterpret_cast<const float4 *>(p0 + (size_t)min(c0 + q, n_chunks - 1) * cstride);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const bool on = c0 + q < n_chunks;
                    d0 += on ? v[q].x : 0.f; d1 += on ? v[q].y : 0.f; d2 += on ? v[q].z : 0.f; d3 += on ? v[q].w : 0.f;
                }
            }
            const float dd[4] = {d0, d1, d2, d3};
            if (dd[0] != 12345.678f) SJD_TRG(0, 1);          // (partials arrived)
            unsigned short o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = sjd_residual_elem<DT>(hx[j], dd[j]);      // projection output rounds to the activation dtype, the residual add again
                hx[j] = Cvt<DT>::to_f(o[j]);
            }
            uint2 ho;
            ho.x = (unsigned)o[0] | ((unsigned)o[1] << 16);
            ho.y = (unsigned)o[2] | ((unsigned)o[3] << 16);
            *reinterpret_cast<uint2 *>(hp) = ho;
        }
        ss = sjd_sumsq4(ss, hx[0], hx[1], hx[2], hx[3]);      // (shared with the reducing epilogue of G1: sjd_mlp_epilogue.h)
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) out_sumsq[(size_t)blockIdx.y * prows + row] = red[0] + red[1];
    SJD_TRG(0, 2);
}

template <int DT>
__global__ __launch_bounds__(128) void f1r_residual_sumsq(unsigned short *__restrict__ h, const float *__restrict__ part, int n_chunks,
                                                          int hidden, int prows, float *__restrict__ out_sumsq)
{
    f1r_body<DT>(h, part, n_chunks, hidden, prows, out_sumsq);
}

#ifdef SJD_EXPERIMENTAL        // round-5 experiment (measured no-go)
// F1r HOSTING the L2 head pull of the projection behind it (round 5, sjd_l2_prefetch.h): grid rows [0, n_slices) are F1r's own workgroups
// (dispatched first), the rows behind them pull.  `rows * n_slices` is a multiple of 8 (the launcher checks), so pulling workgroup j sits on
// XCD j mod 8.  The pull's arguments come after F1r's: the sixteen preloaded argument dwords are still F1r's own.
template <int DT>
__global__ __launch_bounds__(128) void f1r_residual_sumsq_pf(unsigned short *__restrict__ h, const float *__restrict__ part, int n_chunks,
                                                             int hidden, int prows, float *__restrict__ out_sumsq, int n_slices,
                                                             const sjd_l2_head pf)
{
    if ((int)blockIdx.y >= n_slices) {
        sjd_l2_head_pull(pf, ((int)blockIdx.y - n_slices) * (int)gridDim.x + (int)blockIdx.x, ((int)gridDim.y - n_slices) * (int)gridDim.x);
        return;
    }
    f1r_body<DT>(h, part, n_chunks, hidden, prows, out_sumsq);
}

#endif  // SJD_EXPERIMENTAL
// 1/rms of a row from the per-slice sums of squares F1r wrote (fixed order)
__device__ __forceinline__ float row_sumsq_total(const float *__restrict__ row_sumsq, int slices, int prows, int row)
{
    float t = 0.f;
    for (int s0 = 0; s0 < slices; s0 += 8) {          // eight independent loads in flight, then a fixed-order sum
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (s0 + q < slices) ? row_sumsq[(size_t)(s0 + q) * prows + row] : 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += v[q];
    }
    return t;
}

// ------------------------------------------------------------------------------------------------ F2
// qkv: [T, (H + 2*Hkv) * D] fused projection output (T = B*n tokens).  One wave64 per (token, head); D in {64,128}.
// Lane l owns the rotate-half pair (d = l', d + D/2) for l' = l (+64*k).  positions: int64 [T].
// KV8: the cache holds OCP fp8 e4m3 bytes (value = fp8 * scale); k/v rows are quantised on the way in (q stays 16-bit)
// TBL (SJD_F2_ROPE_TABLE, LlamaGen): the interleaved 2-D rotary of reference llamagen.py:457-467 -- lane l owns the pair (2l, 2l + 1), and
// `inv_freq` is an fp32 table [S_rows >= S_max, D/2, 2] of (cos, sin), row p serving position p (positions clamp to [0, S_max - 1]).  No QK-norm.
// DS (SJD_F2_HEAD_PAD128, LlamaGen GPT-3B): the STORAGE head dim of q_out and the caches where it differs from the source's D -- D = 100, DS = 128,
// table mode only.  Lanes 0..49 own the pairs of the 100-wide source head and of the [., 50, 2] table row exactly as above; lanes 50..63 store
// zeros into columns 100..127 of every row the kernel writes (q, k and v), so the pad columns never depend on what the buffers held.
// The byte stored is sat_e4m3(x * (1 / scale)): beyond +-448 (a key or value larger than the calibration prompt allowed for) it is +-448, not the
// NaN code the bare conversion gives (sjd_fp8.h).
__device__ __forceinline__ unsigned char f2_to_fp8(float x)
{
    x = sjd_e4m3_clamp(x);
    return (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(x, x, 0, false) & 0xff);
}

template <int DT, int D, bool KV8, bool TBL = false, int DS = D>
__global__ __launch_bounds__(256) void f2_qknorm_rope_append(
    const unsigned short *__restrict__ qkv, unsigned short *__restrict__ q_out, unsigned short *__restrict__ k_cache,
    unsigned short *__restrict__ v_cache, const unsigned short *__restrict__ qn_w, const unsigned short *__restrict__ qn_b,
    const unsigned short *__restrict__ kn_w, const unsigned short *__restrict__ kn_b, const float *__restrict__ inv_freq,
    const long *__restrict__ positions, int B, int n, int H, int H_kv, int S_max, const sjd_iter_params *__restrict__ params,
    int kv_len_arg, const float *__restrict__ part, int n_chunks, int prows, float k_inv, float v_inv,
    const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden, float rs_eps, int hps_q, int hps_k)
{
    SJD_TRG(1, 0);
    static_assert(DS == D || (TBL && !KV8 && DS == 128 && D < DS && (D % 2) == 0), "a padded head: table mode, 16-bit cache, 64 lanes cover the 128 stored columns");
    constexpr int HALF = D / 2;
    constexpr int PPL = HALF / 64 > 0 ? HALF / 64 : 1;       // pairs per lane (D=128: 1, D=64: lanes 32..63 idle)
    constexpr int EST = TBL ? 2 : 1, E1 = TBL ? 1 : HALF;    // the lane's pair: elements (EST * lane, EST * lane + E1)
    const int lane = threadIdx.x & 63;
    // the wave index as a SCALAR: everything derived from it (token, head, batch row) is uniform, so kv_len and the position come through
    // the scalar cache instead of as 64-lane vector loads the partial loads would queue behind
    const int gw = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // global wave id
    const int heads = H + 2 * H_kv;
    if (gw >= B * n * heads) return;
    const int tok = gw / heads, hh = gw % heads;
    const int b = tok / n, i = tok % n;
    const unsigned short *src = qkv + (size_t)tok * heads * D + (size_t)hh * D;
    const bool is_q = hh < H, is_k = !is_q && hh < H + H_kv;
    const int hl = is_q ? hh : (is_k ? hh - H : hh - H - H_kv);
    const float q8 = is_k ? k_inv : v_inv;
    const bool active = lane < HALF;
    float x0 = 0.f, x1 = 0.f;
    int kv_len = kv_len_arg;
    // Late round 6: the per-head norm's gain / bias, the rotary frequency and the position are requested HERE, in front of the partial planes, and held
    // (the empty asm below) -- by the ISA they used to be two more dependent round trips behind the plane sums: the norm parameters after the wave sums,
    // inv_freq / positions in front of the sincos.  Same values, same arithmetic.
    const unsigned short *gw_ = is_q ? qn_w : kn_w, *gb_ = is_q ? qn_b : kn_b;
    const bool has_norm = gw_ != nullptr && (is_q || is_k);           // (wave-uniform)
    const int la = active ? lane : 0;
    unsigned short nw0 = 0, nw1 = 0, nb0 = 0, nb1 = 0;
    if (has_norm) {
        const int hps = is_q ? hps_q : hps_k;                 // sharded gains ([mp, D], swin-norm checkpoints): row head / heads_per_shard
        const size_t nrow = hps ? (size_t)(hl / hps) * D : 0; //   (a scalar offset: the loads stay where they are)
        nw0 = gw_[nrow + la]; nw1 = gw_[nrow + la + HALF]; nb0 = gb_[nrow + la]; nb1 = gb_[nrow + la + HALF];
    }
    const long posv = positions[tok];
    float ifr, tsn = 0.f;                                     // TBL: (cos, sin) of the table row; the rotate-half form: the lane's frequency
    if constexpr (TBL) {
        const long prow = posv < 0 ? 0 : (posv < S_max ? posv : (long)S_max - 1);
        const float2 cs2 = reinterpret_cast<const float2 *>(inv_freq)[(size_t)prow * HALF + la];
        ifr = cs2.x;
        tsn = cs2.y;
    } else {
        ifr = inv_freq[la];
    }
    if (part) {                                               // fp32 split-K partials of the qkv projection (G1)
        // Entry sequence written for the memory system (ISA, late round 2: the kernel used to run through five dependent round trips --
        // two batches of kernel arguments, batch_rows, kv_len as a vector load with a full wait, the row statistics -- before the partial
        // loads went out).  Now: the row statistics and the first eight partial planes are requested back to back with unconditional
        // (clamped) loads, THEN kv_len is fetched (one scalar round trip, under the vector one), then the sums in the usual order.
        const size_t ncol = (size_t)heads * D, col = (size_t)hh * D + (active ? EST * lane : 0);
        float ssv[8], v0[8], v1[8];
        const float *ssp = row_sumsq ? row_sumsq : part;
#pragma unroll
        for (int q = 0; q < 8; ++q) ssv[q] = ssp[(size_t)(row_sumsq ? min(q, rs_slices - 1) : 0) * prows + tok];
        // (a batch of eight planes, or -- one uniform branch -- of the two / four a short split-K has: with the two planes of a 128-row q|k|v
        // launch six of the eight clamped loads re-read the last plane, 12 of a wave's 16 load instructions)
        if (n_chunks <= 2) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                v0[q] = 0.f; v1[q] = 0.f;
                if (q < 2) {
                    const float *pp = part + ((size_t)min(q, n_chunks - 1) * prows + tok) * ncol + col;
                    v0[q] = pp[0];
                    v1[q] = pp[E1];
                }
            }
        } else if (n_chunks <= 4) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                v0[q] = 0.f; v1[q] = 0.f;
                if (q < 4) {
                    const float *pp = part + ((size_t)min(q, n_chunks - 1) * prows + tok) * ncol + col;
                    v0[q] = pp[0];
                    v1[q] = pp[E1];
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float *pp = part + ((size_t)min(q, n_chunks - 1) * prows + tok) * ncol + col;
                v0[q] = pp[0];
                v1[q] = pp[E1];
            }
        }
        int n_unused_ = 0;
        if (params) sjdi_kv_rows(params, b, &kv_len, &n_unused_);
#ifndef F2_NO_PIN          // (A/B aid: without the pin the compiler sinks the early loads back to their uses -- the round-5 schedule)
        asm volatile("" :: "v"(nw0), "v"(nw1), "v"(nb0), "v"(nb1), "v"(ifr), "s"(posv));      // (keeps the early loads early: the compiler sinks them to their uses otherwise)
        if constexpr (TBL) asm volatile("" :: "v"(tsn));
#endif
        float ss_tot = 0.f;                                   // row_sumsq_total: batches of eight slices in order, missing slices add zero
#pragma unroll
        for (int q = 0; q < 8; ++q) ss_tot += (q < rs_slices) ? ssv[q] : 0.f;
        for (int s0 = 8; s0 < rs_slices; s0 += 8) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = (s0 + q < rs_slices) ? row_sumsq[(size_t)(s0 + q) * prows + tok] : 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) ss_tot += v[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (q < n_chunks) { x0 += v0[q]; x1 += v1[q]; }
        for (int c0 = 8; c0 < n_chunks; c0 += 8) {            // (more than eight planes: the old batched loop)
            float w0[8], w1[8];
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (c0 + q < n_chunks) {
                    const float *pp = part + ((size_t)(c0 + q) * prows + tok) * ncol + col;
                    w0[q] = pp[0];
                    w1[q] = pp[E1];
                }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (c0 + q < n_chunks) { x0 += w0[q]; x1 += w1[q]; }
        }
        if (row_sumsq) {                                      // the RMSNorm of the projection's input, applied on its output
            const float r = rsqrtf(ss_tot * rs_inv_hidden + rs_eps);
            x0 *= r;
            x1 *= r;
        }
        x0 = Cvt<DT>::to_f(Cvt<DT>::from_f(x0));
        x1 = Cvt<DT>::to_f(Cvt<DT>::from_f(x1));
        if (!active) { x0 = 0.f; x1 = 0.f; }
        if (x0 != 12345.678f) SJD_TRG(1, 1);                  // (partials + row statistics arrived)
    } else {
        if (params) kv_len = sjdi_params_of(params, b)->kv_len;
        if (active) {
            x0 = Cvt<DT>::to_f(src[EST * lane]);
            x1 = Cvt<DT>::to_f(src[EST * lane + E1]);
        }
    }
    // Where the row goes.  This used to sit -- with its early return for rows beyond the cache -- in front of the partial loads above,
    // which therefore could not be issued before kv_len had arrived.
    unsigned short *dst = nullptr;
    unsigned char *dst8 = nullptr;                            // KV8: byte rows of the fp8 cache
    if (is_q) dst = q_out + ((size_t)tok * H + hl) * DS;
    else {
        const int r = kv_len + i;
        if (r >= S_max) return;
        const size_t off = (((size_t)b * H_kv + hl) * S_max + r) * DS;
        if (KV8) dst8 = reinterpret_cast<unsigned char *>(is_k ? k_cache : v_cache) + off;
        else dst = (is_k ? k_cache : v_cache) + off;
    }
    if (!is_q && !is_k) {                                     // V: plain copy into the cache
        if constexpr (DS != D) {                              // (every lane stores: the pad lanes hold x0 = x1 = 0, written as zero bits)
            dst[2 * lane] = active ? Cvt<DT>::from_f(x0) : (unsigned short)0;
            dst[2 * lane + 1] = active ? Cvt<DT>::from_f(x1) : (unsigned short)0;
            return;
        }
        if (active) {
            if (KV8) { dst8[EST * lane] = f2_to_fp8(x0 * q8); dst8[EST * lane + E1] = f2_to_fp8(x1 * q8); }
            else { dst[EST * lane] = Cvt<DT>::from_f(x0); dst[EST * lane + E1] = Cvt<DT>::from_f(x1); }
        }
        return;
    }
    if (gw_ != nullptr) {                                     // per-head LayerNorm over head_dim (eps 1e-5)
        const float mean = wave_sum(active ? x0 + x1 : 0.f) / (float)D;
        const float d0 = x0 - mean, d1 = x1 - mean;
        const float var = wave_sum(active ? d0 * d0 + d1 * d1 : 0.f) / (float)D;
        const float inv = rsqrtf(var + 1e-5f);
        if (active) {
#pragma clang fp contract(off)
            // F.layer_norm output and the gamma/beta affine both round to the activation dtype in the reference (contraction off: in fp16 the
            // compiler otherwise demotes dtype(n * gain) + bias to ONE half-precision FMA and the rounding of the product is gone)
            const float n0 = Cvt<DT>::to_f(Cvt<DT>::from_f(d0 * inv)), n1 = Cvt<DT>::to_f(Cvt<DT>::from_f(d1 * inv));
            x0 = Cvt<DT>::to_f(Cvt<DT>::from_f(n0 * Cvt<DT>::to_f(nw0))) + Cvt<DT>::to_f(nb0);
            x1 = Cvt<DT>::to_f(Cvt<DT>::from_f(n1 * Cvt<DT>::to_f(nw1))) + Cvt<DT>::to_f(nb1);
            x0 = Cvt<DT>::to_f(Cvt<DT>::from_f(x0));
            x1 = Cvt<DT>::to_f(Cvt<DT>::from_f(x1));
        }
    }
    if constexpr (TBL) {
        if (active) {
#pragma clang fp contract(off)
            // out0 = x0 c - x1 s, out1 = x1 c + x0 s: each product and each sum rounded to fp32 as the separate ATen ops do, then ONE rounding
            // to the activation dtype (.type_as(x)); condition rows (c = s = 0) give zeros.  The pragma keeps the products out of an FMA (the
            // header's __fmul_rn / __fadd_rn are plain operators compiled under the file's contraction setting, and they fuse once inlined)
            const float o0 = x0 * ifr - x1 * tsn;
            const float o1 = x1 * ifr + x0 * tsn;
            dst[2 * lane] = Cvt<DT>::from_f(o0);
            dst[2 * lane + 1] = Cvt<DT>::from_f(o1);
        }
        if constexpr (DS != D) {
            if (!active) { dst[2 * lane] = 0; dst[2 * lane + 1] = 0; }      // pad columns D..DS-1 of the q / k row
        }
    } else if (active) {
#pragma clang fp contract(off)
        // (each product rounds before the sum: no half-precision FMA in fp16)
        const float ang = (float)posv * ifr;
        float sn, cs;
        sincosf(ang, &sn, &cs);
        cs = Cvt<DT>::to_f(Cvt<DT>::from_f(cs));              // cos/sin are cast to the activation dtype (:110)
        sn = Cvt<DT>::to_f(Cvt<DT>::from_f(sn));
        // (q*cos) + (rotate_half(q)*sin): each product and the sum round to the activation dtype, as the ATen ops do
        const float a0 = Cvt<DT>::to_f(Cvt<DT>::from_f(x0 * cs)), b0 = Cvt<DT>::to_f(Cvt<DT>::from_f(-x1 * sn));
        const float a1 = Cvt<DT>::to_f(Cvt<DT>::from_f(x1 * cs)), b1 = Cvt<DT>::to_f(Cvt<DT>::from_f(x0 * sn));
        if (KV8 && !is_q) {                                   // the 16-bit value the reference would cache, then fp8(x / scale)
            dst8[lane] = f2_to_fp8(Cvt<DT>::to_f(Cvt<DT>::from_f(a0 + b0)) * q8);
            dst8[lane + HALF] = f2_to_fp8(Cvt<DT>::to_f(Cvt<DT>::from_f(a1 + b1)) * q8);
        } else {
            dst[lane] = Cvt<DT>::from_f(a0 + b0);
            dst[lane + HALF] = Cvt<DT>::from_f(a1 + b1);
        }
    }
    SJD_TRG(1, 2);
    (void)PPL;
}

// ------------------------------------------------------------------------------------------------ F2 for many rows (round 6)
// The kernel above is written for the latency of a 32-row window: one wave per (token, head), two dword loads per plane and lane, and every wave
// computes the sin / cos of ITS token's rotary angles -- 48 (Emu3) or 96 (Lumina) times per token.  At the 256 rows of eight prompts that is
// 24576 waves of a few hundred bytes each: 17.2 us for 15.6 MB (profiles/r6_8prompts_by_shape.txt), three rounds of waves per CU, each a chain of
// dependent round trips.  Here a wave takes HPW consecutive heads of one kind (q, k or v) of its token: the planes of all HPW heads are requested
// together, the angle is computed once.  Element for element the arithmetic of f2_qknorm_rope_append (same sums in chunk order, same roundings),
// so q and the cache rows are bit-identical; used for windows of more than 64 rows read from split-K partials.
// SHARD (sharded QK-norm gains, [mp, D]): the HPW heads of a wave may belong to different shards, so each head loads its own row (all in
// the same early batch); without it one row serves the wave, as before.
// TBL (SJD_F2_ROPE_TABLE, LlamaGen's windows of 65..256 rows): lane l owns the interleaved pair (2l, 2l + 1) of each of its HPW heads -- one
// 8-byte load per plane and head, one packed 32-bit store per head -- and the (cos, sin) of its pair comes from row `position` of the table in
// `inv_freq`, read ONCE per wave.  The table row's address hangs on the position, so the order of requests is: position (scalar), the first
// four planes of all HPW heads (they do not need it), then the table row -- one vector round trip with the planes, not one in front of them.
// No QK-norm, no fp8 cache; the arithmetic of the one-head kernel's TBL branch element for element (no FMA contraction).
// DS (SJD_F2_HEAD_PAD128): see the one-head kernel -- 100-wide heads in the planes (400-byte head strides keep the 8-byte loads aligned), 128-wide
// rows out; lanes 50..63 store the zero pad columns of each of the wave's HPW heads.
template <int DT, int D, bool KV8, int HPW, bool SHARD = false, bool TBL = false, int DS = D>
__global__ __launch_bounds__(256) void f2_qknorm_rope_append_rows(
    unsigned short *__restrict__ q_out, unsigned short *__restrict__ k_cache, unsigned short *__restrict__ v_cache,
    const unsigned short *__restrict__ qn_w, const unsigned short *__restrict__ qn_b, const unsigned short *__restrict__ kn_w,
    const unsigned short *__restrict__ kn_b, const float *__restrict__ inv_freq, const long *__restrict__ positions, int B, int n, int H, int H_kv,
    int S_max, const sjd_iter_params *__restrict__ params, int kv_len_arg, const float *__restrict__ part, int n_chunks, int prows, float k_inv,
    float v_inv, const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden, float rs_eps, int hps_q, int hps_k)
{
    static_assert(DS == D || (TBL && !KV8 && DS == 128 && D < DS && (D % 4) == 0), "a padded head: table mode, 16-bit cache, 8-byte aligned head strides in the planes");
    constexpr int HALF = D / 2;
    constexpr int NG = SHARD ? HPW : 1;                       // gain / bias rows held per lane
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int heads = H + 2 * H_kv, groups = heads / HPW;
    if (gw >= B * n * groups) return;
    const int tok = gw / groups, hh0 = (gw % groups) * HPW;
    const int b = tok / n, i = tok % n;
    const bool is_q = hh0 < H, is_k = !is_q && hh0 < H + H_kv;
    const int hl0 = is_q ? hh0 : (is_k ? hh0 - H : hh0 - H - H_kv);
    const float q8 = is_k ? k_inv : v_inv;
    const bool active = lane < HALF;
    constexpr int EST = TBL ? 2 : 1;                          // the lane's pair starts at element EST * lane (TBL: (2l, 2l + 1); else (l, l + HALF))
    const size_t ncol = (size_t)heads * D, col = (size_t)hh0 * D + (active ? EST * lane : 0);
    // (the norm parameters, the rotary frequency and the position in front of the planes: see f2_qknorm_rope_append)
    const unsigned short *gw_ = is_q ? qn_w : kn_w, *gb_ = is_q ? qn_b : kn_b;
    const bool has_norm = gw_ != nullptr && (is_q || is_k);
    const int la = active ? lane : 0;
    unsigned short nw0[NG], nw1[NG], nb0[NG], nb1[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        nw0[j] = 0; nw1[j] = 0; nb0[j] = 0; nb1[j] = 0;
        if (has_norm) {
            const int hps = is_q ? hps_q : hps_k;
            const size_t nrow = (SHARD && hps) ? (size_t)((hl0 + j) / hps) * D : 0;
            nw0[j] = gw_[nrow + la]; nw1[j] = gw_[nrow + la + HALF]; nb0[j] = gb_[nrow + la]; nb1[j] = gb_[nrow + la + HALF];
        }
    }
    float ifr = 0.f, tsn = 0.f;                               // TBL: (cos, sin) of the table row; the rotate-half form: the lane's frequency
    if constexpr (!TBL) ifr = inv_freq[la];
    const long posv = positions[tok];
    float ssv[8];
    const float *ssp = row_sumsq ? row_sumsq : part;
#pragma unroll
    for (int q = 0; q < 8; ++q) ssv[q] = ssp[(size_t)(row_sumsq ? min(q, rs_slices - 1) : 0) * prows + tok];
    float x0[HPW], x1[HPW];
#pragma unroll
    for (int j = 0; j < HPW; ++j) { x0[j] = 0.f; x1[j] = 0.f; }
    for (int c0 = 0; c0 < n_chunks; c0 += 4) {                // four planes x HPW heads in flight, then the sums in chunk order
        float v0[4][HPW], v1[4][HPW];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float *pp = part + ((size_t)min(c0 + q, n_chunks - 1) * prows + tok) * ncol + col;
#pragma unroll
            for (int j = 0; j < HPW; ++j) {
                if constexpr (TBL) {
                    const float2 pr = *reinterpret_cast<const float2 *>(pp + j * D);
                    v0[q][j] = pr.x; v1[q][j] = pr.y;
                } else { v0[q][j] = pp[j * D]; v1[q][j] = pp[j * D + HALF]; }
            }
        }
        if constexpr (TBL) {
            if (c0 == 0) {                                    // the table row, behind the first batch of planes (positions clamp to the table)
                const long prow = posv < 0 ? 0 : (posv < S_max ? posv : (long)S_max - 1);
                const float2 cs2 = reinterpret_cast<const float2 *>(inv_freq)[(size_t)prow * HALF + la];
                ifr = cs2.x;
                tsn = cs2.y;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (c0 + q < n_chunks) {
#pragma unroll
                for (int j = 0; j < HPW; ++j) { x0[j] += v0[q][j]; x1[j] += v1[q][j]; }
            }
    }
    int kv_len = kv_len_arg, n_unused_ = 0;
    if (params) sjdi_kv_rows(params, b, &kv_len, &n_unused_);
#ifndef F2_NO_PIN
#pragma unroll
    for (int j = 0; j < NG; ++j) asm volatile("" :: "v"(nw0[j]), "v"(nw1[j]), "v"(nb0[j]), "v"(nb1[j]));
    asm volatile("" :: "v"(ifr), "s"(posv));
    if constexpr (TBL) asm volatile("" :: "v"(tsn));
#endif
    float ss_tot = 0.f;                                       // row_sumsq_total's order
#pragma unroll
    for (int q = 0; q < 8; ++q) ss_tot += (q < rs_slices) ? ssv[q] : 0.f;
    for (int s0 = 8; s0 < rs_slices; s0 += 8) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (s0 + q < rs_slices) ? row_sumsq[(size_t)(s0 + q) * prows + tok] : 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) ss_tot += v[q];
    }
    const float r = row_sumsq ? rsqrtf(ss_tot * rs_inv_hidden + rs_eps) : 1.0f;
#pragma unroll
    for (int j = 0; j < HPW; ++j) {
        if (row_sumsq) { x0[j] *= r; x1[j] *= r; }
        x0[j] = Cvt<DT>::to_f(Cvt<DT>::from_f(x0[j]));
        x1[j] = Cvt<DT>::to_f(Cvt<DT>::from_f(x1[j]));
        if (!active) { x0[j] = 0.f; x1[j] = 0.f; }
    }
    const int rrow = kv_len + i;
    if (!is_q && rrow >= S_max) return;
    if (!is_q && !is_k) {                                     // V: plain copy into the cache
        if (active || DS != D) {                              // (a padded head: every lane stores, the pad lanes zero bits)
#pragma unroll
            for (int j = 0; j < HPW; ++j) {
                const size_t off = (((size_t)b * H_kv + hl0 + j) * S_max + rrow) * DS;
                if constexpr (DS != D) {
                    *reinterpret_cast<unsigned *>(v_cache + off + 2 * lane) =
                        active ? (unsigned)Cvt<DT>::from_f(x0[j]) | ((unsigned)Cvt<DT>::from_f(x1[j]) << 16) : 0u;
                } else if constexpr (TBL) {
                    *reinterpret_cast<unsigned *>(v_cache + off + 2 * lane) =
                        (unsigned)Cvt<DT>::from_f(x0[j]) | ((unsigned)Cvt<DT>::from_f(x1[j]) << 16);
                } else if (KV8) {
                    unsigned char *d8 = reinterpret_cast<unsigned char *>(v_cache) + off;
                    d8[lane] = f2_to_fp8(x0[j] * q8); d8[lane + HALF] = f2_to_fp8(x1[j] * q8);
                } else { v_cache[off + lane] = Cvt<DT>::from_f(x0[j]); v_cache[off + lane + HALF] = Cvt<DT>::from_f(x1[j]); }
            }
        }
        return;
    }
    if (gw_ != nullptr) {                                     // per-head LayerNorm over head_dim (eps 1e-5)
#pragma unroll
        for (int j = 0; j < HPW; ++j) {
            const int jg = SHARD ? j : 0;
            const float w0 = Cvt<DT>::to_f(nw0[jg]), w1 = Cvt<DT>::to_f(nw1[jg]), b0 = Cvt<DT>::to_f(nb0[jg]), b1 = Cvt<DT>::to_f(nb1[jg]);
            const float mean = wave_sum(active ? x0[j] + x1[j] : 0.f) / (float)D;
            const float d0 = x0[j] - mean, d1 = x1[j] - mean;
            const float var = wave_sum(active ? d0 * d0 + d1 * d1 : 0.f) / (float)D;
            const float inv = rsqrtf(var + 1e-5f);
            if (active) {
#pragma clang fp contract(off)
                // (as in the one-head kernel: no half-precision FMA over the rounded product)
                const float n0 = Cvt<DT>::to_f(Cvt<DT>::from_f(d0 * inv)), n1 = Cvt<DT>::to_f(Cvt<DT>::from_f(d1 * inv));
                float y0 = Cvt<DT>::to_f(Cvt<DT>::from_f(n0 * w0)) + b0;
                float y1 = Cvt<DT>::to_f(Cvt<DT>::from_f(n1 * w1)) + b1;
                x0[j] = Cvt<DT>::to_f(Cvt<DT>::from_f(y0));
                x1[j] = Cvt<DT>::to_f(Cvt<DT>::from_f(y1));
            }
        }
    }
    if constexpr (TBL) {
        if (active) {
#pragma clang fp contract(off)
            // out0 = x0 c - x1 s, out1 = x1 c + x0 s: every product and sum rounded to fp32, ONE rounding to the activation dtype (see the
            // one-head kernel); condition rows (c = s = 0) give zeros
#pragma unroll
            for (int j = 0; j < HPW; ++j) {
                const float o0 = x0[j] * ifr - x1[j] * tsn;
                const float o1 = x1[j] * ifr + x0[j] * tsn;
                const unsigned pk = (unsigned)Cvt<DT>::from_f(o0) | ((unsigned)Cvt<DT>::from_f(o1) << 16);
                unsigned short *dst = is_q ? q_out + ((size_t)tok * H + hl0 + j) * DS
                                           : k_cache + (((size_t)b * H_kv + hl0 + j) * S_max + rrow) * DS;
                *reinterpret_cast<unsigned *>(dst + 2 * lane) = pk;
            }
        }
        if constexpr (DS != D) {
            if (!active) {                                    // pad columns D..DS-1 of the wave's q / k rows
#pragma unroll
                for (int j = 0; j < HPW; ++j) {
                    unsigned short *dst = is_q ? q_out + ((size_t)tok * H + hl0 + j) * DS
                                               : k_cache + (((size_t)b * H_kv + hl0 + j) * S_max + rrow) * DS;
                    *reinterpret_cast<unsigned *>(dst + 2 * lane) = 0u;
                }
            }
        }
    } else if (active) {
#pragma clang fp contract(off)
        // (each product rounds before the sum: no half-precision FMA in fp16)
        const float ang = (float)posv * ifr;
        float sn, cs;
        sincosf(ang, &sn, &cs);
        cs = Cvt<DT>::to_f(Cvt<DT>::from_f(cs));
        sn = Cvt<DT>::to_f(Cvt<DT>::from_f(sn));
#pragma unroll
        for (int j = 0; j < HPW; ++j) {
            const float a0 = Cvt<DT>::to_f(Cvt<DT>::from_f(x0[j] * cs)), c0_ = Cvt<DT>::to_f(Cvt<DT>::from_f(-x1[j] * sn));
            const float a1 = Cvt<DT>::to_f(Cvt<DT>::from_f(x1[j] * cs)), c1_ = Cvt<DT>::to_f(Cvt<DT>::from_f(x0[j] * sn));
            if (is_q) {
                unsigned short *dst = q_out + ((size_t)tok * H + hl0 + j) * D;
                dst[lane] = Cvt<DT>::from_f(a0 + c0_);
                dst[lane + HALF] = Cvt<DT>::from_f(a1 + c1_);
            } else {
                const size_t off = (((size_t)b * H_kv + hl0 + j) * S_max + rrow) * D;
                if (KV8) {
                    unsigned char *d8 = reinterpret_cast<unsigned char *>(k_cache) + off;
                    d8[lane] = f2_to_fp8(Cvt<DT>::to_f(Cvt<DT>::from_f(a0 + c0_)) * q8);
                    d8[lane + HALF] = f2_to_fp8(Cvt<DT>::to_f(Cvt<DT>::from_f(a1 + c1_)) * q8);
                } else {
                    k_cache[off + lane] = Cvt<DT>::from_f(a0 + c0_);
                    k_cache[off + lane + HALF] = Cvt<DT>::from_f(a1 + c1_);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ F3
template <int DT>
__global__ __launch_bounds__(256) void f3_silu_mul(const unsigned short *__restrict__ gu, unsigned short *__restrict__ y, int M, int I,
                                                   const float *__restrict__ part, int n_chunks, int prows,
                                                   const float *__restrict__ row_sumsq, int rs_slices, float rs_inv_hidden, float rs_eps)
{
    SJD_TRG(2, 0);
    const int per_row = I / 8;
    const size_t total = (size_t)M * per_row;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = idx / per_row, c = (idx % per_row) * 8;
        float g[8], u[8], o[8];
        if (part) {
            const float ss_tot = row_sumsq ? row_sumsq_total(row_sumsq, rs_slices, prows, row) : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) { g[j] = 0.f; u[j] = 0.f; }
            for (int c0 = 0; c0 < n_chunks; c0 += 4) {        // four chunks (16 loads) in flight, then the sum in chunk order
                float4 a[4], b[4], e[4], f[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (c0 + q < n_chunks) {
                        const float4 *pg = reinterpret_cast<const float4 *>(part + ((size_t)(c0 + q) * prows + row) * 2 * I + c);
                        const float4 *pu = reinterpret_cast<const float4 *>(part + ((size_t)(c0 + q) * prows + row) * 2 * I + I + c);
                        a[q] = pg[0]; b[q] = pg[1]; e[q] = pu[0]; f[q] = pu[1];
                    }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (c0 + q < n_chunks) {
                        g[0] += a[q].x; g[1] += a[q].y; g[2] += a[q].z; g[3] += a[q].w; g[4] += b[q].x; g[5] += b[q].y; g[6] += b[q].z; g[7] += b[q].w;
                        u[0] += e[q].x; u[1] += e[q].y; u[2] += e[q].z; u[3] += e[q].w; u[4] += f[q].x; u[5] += f[q].y; u[6] += f[q].z; u[7] += f[q].w;
                    }
            }
            const float r = row_sumsq ? rsqrtf(ss_tot * rs_inv_hidden + rs_eps) : 1.0f;
            if (g[0] + r != 12345.678f) SJD_TRG(2, 1);       // (partials + row statistics arrived)
            unsigned short ob[8];                // element arithmetic shared with g1_gateup_silu (sjd_mlp_epilogue.h): same bits
#pragma unroll
            for (int j = 0; j < 8; ++j) ob[j] = sjd_silu_mul_elem<DT>(g[j], u[j], r);
            *reinterpret_cast<u32x4 *>(y + (size_t)row * I + c) = u32x4{(unsigned)ob[0] | ((unsigned)ob[1] << 16), (unsigned)ob[2] | ((unsigned)ob[3] << 16),
                                                                      (unsigned)ob[4] | ((unsigned)ob[5] << 16), (unsigned)ob[6] | ((unsigned)ob[7] << 16)};
            continue;
        } else {
            unpack8<DT>(*reinterpret_cast<const u32x4 *>(gu + (size_t)row * 2 * I + c), g);
            unpack8<DT>(*reinterpret_cast<const u32x4 *>(gu + (size_t)row * 2 * I + I + c), u);
        }
        unsigned short ob[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) ob[j] = sjd_silu_mul_elem_rounded<DT>(g[j], u[j]);     // silu rounds to the activation dtype
        (void)o;
        *reinterpret_cast<u32x4 *>(y + (size_t)row * I + c) = u32x4{(unsigned)ob[0] | ((unsigned)ob[1] << 16), (unsigned)ob[2] | ((unsigned)ob[3] << 16),
                                                                  (unsigned)ob[4] | ((unsigned)ob[5] << 16), (unsigned)ob[6] | ((unsigned)ob[7] << 16)};
    }
    SJD_TRG(2, 2);
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" int sjd_add_rmsnorm(void *h, const void *delta, const void *weight, void *y, int rows, int hidden, float eps, int dtype,
                               const float *part, int n_chunks, void *stream)
{
    const int mode = dtype & ~SJD_DTYPE_MASK;
    dtype &= SJD_DTYPE_MASK;
    if (mode & ~SJD_F1_POST_NORM) return SJD_ERR_UNSUPPORTED;
    const bool post = (mode & SJD_F1_POST_NORM) != 0;
    if (part && (rows > 256 || n_chunks < 1)) return SJD_ERR_BAD_ARG;
    if (post && !delta && !part) return SJD_ERR_BAD_ARG;         // the post-norm form normalises the sublayer output: there must be one
    const int prows = ((rows + 31) / 32) * 32;      // row padding of the G1 partials
    // (hidden <= 8192 for the 256-thread kernel; the post-norm form of the 1024-thread plane kernel serves up to 16384)
    const int hidden_cap = (post && part) ? 16384 : 256 * 8 * 4;
    if (!h || !weight || (!y && !post) || rows < 1 || hidden < 8 || (hidden % 8) != 0 || hidden > hidden_cap) return SJD_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (part && (hidden % 4) == 0 && hidden <= 16384 && (dtype == SJD_DTYPE_BF16 || dtype == SJD_DTYPE_F16)) {
#define SJD_F1P(DT_, POST_) hipLaunchKernelGGL((f1p_add_rmsnorm<DT_, POST_>), dim3(rows), dim3(1024), 0, s, (unsigned short *)h, part, n_chunks, \
                                               (const unsigned short *)weight, (unsigned short *)y, hidden, eps, prows)
        if (dtype == SJD_DTYPE_BF16) { if (post) SJD_F1P(SJD_DTYPE_BF16, true); else SJD_F1P(SJD_DTYPE_BF16, false); }
        else { if (post) SJD_F1P(SJD_DTYPE_F16, true); else SJD_F1P(SJD_DTYPE_F16, false); }
#undef SJD_F1P
        return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
    }
#define SJD_F1(DT_, POST_) hipLaunchKernelGGL((f1_add_rmsnorm<DT_, POST_>), dim3(rows), dim3(256), 0, s, (unsigned short *)h,                \
                                              (const unsigned short *)delta, (const unsigned short *)weight, (unsigned short *)y, hidden, eps, \
                                              part, n_chunks, prows)
    if (dtype == SJD_DTYPE_BF16) { if (post) SJD_F1(SJD_DTYPE_BF16, true); else SJD_F1(SJD_DTYPE_BF16, false); }
    else if (dtype == SJD_DTYPE_F16) { if (post) SJD_F1(SJD_DTYPE_F16, true); else SJD_F1(SJD_DTYPE_F16, false); }
    else return SJD_ERR_UNSUPPORTED;
#undef SJD_F1
    return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
}

static int f2_launch(const void *qkv, void *q_out, void *k_cache, void *v_cache, const void *qn_w, const void *qn_b, const void *kn_w,
                     const void *kn_b, const float *inv_freq, const int64_t *positions, int B, int n, int H, int H_kv, int D, int S_max,
                     int dtype, const sjd_iter_params *params, int kv_len, const float *part, int n_chunks, bool kv8, float k_scale,
                     float v_scale, const sjd_row_norm *rn, void *stream)
{
    // the mode bits of `dtype`: SJD_QKN_SHARDS(mp) -- QK-norm gain / bias stored [mp, D], head h of q uses row h / (H / mp), of k h / (H_kv / mp);
    // SJD_F2_ROPE_TABLE -- LlamaGen's interleaved rotary from a (cos, sin) table in `inv_freq`
    // SJD_F2_HEAD_PAD128 -- with the table mode and D = 100: 100-wide source heads, 128-wide q_out / cache rows whose pad columns are written as zeros
    // SJD_F2_ONE_HEAD -- one head per wave even above 64 rows of split-K planes (the parity tests compare the two forms)
    if (dtype & ~(SJD_DTYPE_MASK | SJD_QKN_SHARDS_MASK | SJD_F2_ROPE_TABLE | SJD_F2_HEAD_PAD128 | SJD_F2_ONE_HEAD)) return SJD_ERR_UNSUPPORTED;
    const int shards = (dtype & SJD_QKN_SHARDS_MASK) >> SJD_QKN_SHARDS_SHIFT;
    const bool table = (dtype & SJD_F2_ROPE_TABLE) != 0, pad128 = (dtype & SJD_F2_HEAD_PAD128) != 0, one_head = (dtype & SJD_F2_ONE_HEAD) != 0;
    dtype &= SJD_DTYPE_MASK;
    if (pad128 && (!table || D != 100)) return SJD_ERR_UNSUPPORTED;
    if (table && (qn_w || qn_b || kn_w || kn_b)) return SJD_ERR_BAD_ARG;      // (LlamaGen has no QK-norm)
    // (table mode above 64 rows reads split-K planes only: the many-row windows come from G1; a dense source stays refused)
    if (table && (kv8 || (B * n > 64 && !part) || (D != 64 && D != 128 && !pad128))) return SJD_ERR_UNSUPPORTED;
    if (shards > 1 && (H % shards != 0 || H_kv % shards != 0)) return SJD_ERR_BAD_ARG;
    const int hps_q = shards > 1 ? H / shards : 0, hps_k = shards > 1 ? H_kv / shards : 0;     // heads per shard (0: one shared row)
    if (part && (B * n > 256 || n_chunks < 1)) return SJD_ERR_BAD_ARG;
    if (rn && (!part || !rn->sumsq || rn->slices < 1 || rn->hidden < 1)) return SJD_ERR_BAD_ARG;
    const int prows = ((B * n + 31) / 32) * 32;
    if ((!qkv && !part) || !q_out || !k_cache || !v_cache || !inv_freq || !positions || B < 1 || n < 1 || H < 1 || H_kv < 1) return SJD_ERR_BAD_ARG;
    if (kv8 && (!(k_scale > 0.f) || !(v_scale > 0.f))) return SJD_ERR_BAD_ARG;
    const int waves = B * n * (H + 2 * H_kv);
    const dim3 grid((waves + 3) / 4), block(256);
    hipStream_t s = (hipStream_t)stream;
    // more than 64 rows of split-K partials: HPW heads per wave (f2_qknorm_rope_append_rows) unless the caller asks for the one-head kernel
    if (!one_head && table && part && B * n > 64 && (H % 4) == 0 && (H_kv % 4) == 0) {      // (other head counts: the one-head table kernel below)
        const dim3 g2((B * n * ((H + 2 * H_kv) / 4) + 3) / 4);
#define SJD_F2RT_CASE(DT_, D_, DS_)                                                                                                        \
        if (dtype == DT_ && D == D_) {                                                                                                     \
            hipLaunchKernelGGL((f2_qknorm_rope_append_rows<DT_, D_, false, 4, false, true, DS_>), g2, block, 0, s, (unsigned short *)q_out,     \
                               (unsigned short *)k_cache, (unsigned short *)v_cache, nullptr, nullptr, nullptr, nullptr, inv_freq,         \
                               (const long *)positions, B, n, H, H_kv, S_max, params, kv_len, part, n_chunks, prows, 1.0f, 1.0f,           \
                               rn ? rn->sumsq : nullptr, rn ? rn->slices : 0, rn ? 1.0f / (float)rn->hidden : 0.f, rn ? rn->eps : 0.f, 0,  \
                               0);                                                                                                         \
            return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;                                                              \
        }
        SJD_F2RT_CASE(SJD_DTYPE_BF16, 128, 128)
        SJD_F2RT_CASE(SJD_DTYPE_F16, 128, 128)
        SJD_F2RT_CASE(SJD_DTYPE_BF16, 64, 64)
        SJD_F2RT_CASE(SJD_DTYPE_F16, 64, 64)
        SJD_F2RT_CASE(SJD_DTYPE_BF16, 100, 128)
        SJD_F2RT_CASE(SJD_DTYPE_F16, 100, 128)
#undef SJD_F2RT_CASE
        return SJD_ERR_UNSUPPORTED;
    }
    if (!one_head && !table && part && B * n > 64 && (H % 4) == 0 && (H_kv % 4) == 0 && D == 128 && dtype == SJD_DTYPE_BF16) {
        const dim3 g2((B * n * ((H + 2 * H_kv) / 4) + 3) / 4);
#define SJD_F2R(KV8_, SH_)                                                                                                                 \
        hipLaunchKernelGGL((f2_qknorm_rope_append_rows<SJD_DTYPE_BF16, 128, KV8_, 4, SH_>), g2, block, 0, s, (unsigned short *)q_out,      \
                           (unsigned short *)k_cache, (unsigned short *)v_cache, (const unsigned short *)qn_w, (const unsigned short *)qn_b, \
                           (const unsigned short *)kn_w, (const unsigned short *)kn_b, inv_freq, (const long *)positions, B, n, H, H_kv,    \
                           S_max, params, kv_len, part, n_chunks, prows, kv8 ? 1.0f / k_scale : 1.0f, kv8 ? 1.0f / v_scale : 1.0f,          \
                           rn ? rn->sumsq : nullptr, rn ? rn->slices : 0, rn ? 1.0f / (float)rn->hidden : 0.f, rn ? rn->eps : 0.f, hps_q, hps_k)
        if (shards > 1) { if (kv8) SJD_F2R(true, true); else SJD_F2R(false, true); }
        else { if (kv8) SJD_F2R(true, false); else SJD_F2R(false, false); }
#undef SJD_F2R
        return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
    }
#define SJD_F2_CASE(DT_, D_, KV8_)                                                                                                         \
    if (dtype == DT_ && D == D_ && kv8 == KV8_) {                                                                                          \
        hipLaunchKernelGGL((f2_qknorm_rope_append<DT_, D_, KV8_>), grid, block, 0, s, (const unsigned short *)qkv, (unsigned short *)q_out, \
                           (unsigned short *)k_cache, (unsigned short *)v_cache, (const unsigned short *)qn_w,                              \
                           (const unsigned short *)qn_b, (const unsigned short *)kn_w, (const unsigned short *)kn_b, inv_freq,              \
                           (const long *)positions, B, n, H, H_kv, S_max, params, kv_len, part, n_chunks, prows,                           \
                           kv8 ? 1.0f / k_scale : 1.0f, kv8 ? 1.0f / v_scale : 1.0f, rn ? rn->sumsq : nullptr, rn ? rn->slices : 0,         \
                           rn ? 1.0f / (float)rn->hidden : 0.f, rn ? rn->eps : 0.f, hps_q, hps_k);                                         \
        return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;                                                                   \
    }
    if (table) {
#define SJD_F2T_CASE(DT_, D_, DS_)                                                                                                         \
        if (dtype == DT_ && D == D_) {                                                                                                     \
            hipLaunchKernelGGL((f2_qknorm_rope_append<DT_, D_, false, true, DS_>), grid, block, 0, s, (const unsigned short *)qkv,              \
                               (unsigned short *)q_out, (unsigned short *)k_cache, (unsigned short *)v_cache, nullptr, nullptr, nullptr,   \
                               nullptr, inv_freq, (const long *)positions, B, n, H, H_kv, S_max, params, kv_len, part, n_chunks, prows,    \
                               1.0f, 1.0f, rn ? rn->sumsq : nullptr, rn ? rn->slices : 0, rn ? 1.0f / (float)rn->hidden : 0.f,             \
                               rn ? rn->eps : 0.f, 0, 0);                                                                                  \
            return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;                                                              \
        }
        SJD_F2T_CASE(SJD_DTYPE_BF16, 128, 128)
        SJD_F2T_CASE(SJD_DTYPE_F16, 128, 128)
        SJD_F2T_CASE(SJD_DTYPE_BF16, 64, 64)
        SJD_F2T_CASE(SJD_DTYPE_F16, 64, 64)
        SJD_F2T_CASE(SJD_DTYPE_BF16, 100, 128)
        SJD_F2T_CASE(SJD_DTYPE_F16, 100, 128)
#undef SJD_F2T_CASE
        return SJD_ERR_UNSUPPORTED;
    }
    SJD_F2_CASE(SJD_DTYPE_BF16, 128, false)
    SJD_F2_CASE(SJD_DTYPE_F16, 128, false)
    SJD_F2_CASE(SJD_DTYPE_BF16, 64, false)
    SJD_F2_CASE(SJD_DTYPE_F16, 64, false)
    SJD_F2_CASE(SJD_DTYPE_BF16, 128, true)
    SJD_F2_CASE(SJD_DTYPE_F16, 128, true)
    SJD_F2_CASE(SJD_DTYPE_BF16, 64, true)
    SJD_F2_CASE(SJD_DTYPE_F16, 64, true)
#undef SJD_F2_CASE
    return SJD_ERR_UNSUPPORTED;
}

extern "C" int sjd_qknorm_rope_append(const void *qkv, void *q_out, void *k_cache, void *v_cache, const void *qn_w, const void *qn_b,
                                      const void *kn_w, const void *kn_b, const float *inv_freq, const int64_t *positions, int B, int n,
                                      int H, int H_kv, int D, int S_max, int dtype, const sjd_iter_params *params, int kv_len,
                                      const float *part, int n_chunks, void *stream)
{
    return f2_launch(qkv, q_out, k_cache, v_cache, qn_w, qn_b, kn_w, kn_b, inv_freq, positions, B, n, H, H_kv, D, S_max, dtype, params, kv_len,
                     part, n_chunks, false, 1.0f, 1.0f, nullptr, stream);
}

extern "C" int sjd_qknorm_rope_append_fp8(const void *qkv, void *q_out, void *k_cache, void *v_cache, const void *qn_w, const void *qn_b,
                                          const void *kn_w, const void *kn_b, const float *inv_freq, const int64_t *positions, int B, int n,
                                          int H, int H_kv, int D, int S_max, int dtype, float k_scale, float v_scale,
                                          const sjd_iter_params *params, int kv_len, const float *part, int n_chunks, void *stream)
{
    return f2_launch(qkv, q_out, k_cache, v_cache, qn_w, qn_b, kn_w, kn_b, inv_freq, positions, B, n, H, H_kv, D, S_max, dtype, params, kv_len,
                     part, n_chunks, true, k_scale, v_scale, nullptr, stream);
}

extern "C" int sjd_qknorm_rope_append_ex(const void *qkv, void *q_out, void *k_cache, void *v_cache, const void *qn_w, const void *qn_b,
                                         const void *kn_w, const void *kn_b, const float *inv_freq, const int64_t *positions, int B, int n,
                                         int H, int H_kv, int D, int S_max, int dtype, int kv_fp8, float k_scale, float v_scale,
                                         const sjd_row_norm *row_norm, const sjd_iter_params *params, int kv_len, const float *part,
                                         int n_chunks, void *stream)
{
    return f2_launch(qkv, q_out, k_cache, v_cache, qn_w, qn_b, kn_w, kn_b, inv_freq, positions, B, n, H, H_kv, D, S_max, dtype, params, kv_len,
                     part, n_chunks, kv_fp8 != 0, k_scale, v_scale, row_norm, stream);
}

extern "C" int sjd_residual_sumsq(void *h, const float *part, int n_chunks, int rows, int hidden, int dtype, float *out_sumsq, void *stream)
{
    if (!h || !out_sumsq || rows < 1 || rows > 256 || (part && n_chunks < 1) || hidden < 4 || (hidden % 4) != 0) return SJD_ERR_BAD_ARG;
    const int prows = ((rows + 31) / 32) * 32;
    const dim3 grid(rows, (hidden + 511) / 512), block(128);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SJD_DTYPE_BF16)
        hipLaunchKernelGGL(f1r_residual_sumsq<SJD_DTYPE_BF16>, grid, block, 0, s, (unsigned short *)h, part, n_chunks, hidden, prows, out_sumsq);
    else if (dtype == SJD_DTYPE_F16)
        hipLaunchKernelGGL(f1r_residual_sumsq<SJD_DTYPE_F16>, grid, block, 0, s, (unsigned short *)h, part, n_chunks, hidden, prows, out_sumsq);
    else return SJD_ERR_UNSUPPORTED;
    return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
}

// F1r + the L2 head pull of the next projection in one launch.  pf_blocks: pulling workgroups of 128 threads (a multiple of 8 x rows / gcd...:
// the launcher rounds it to whole grid rows); head NULL or pf_blocks 0: plain sjd_residual_sumsq.
#ifdef SJD_EXPERIMENTAL        // round-5 experiment
extern "C" int sjd_residual_sumsq_pf(void *h, const float *part, int n_chunks, int rows, int hidden, int dtype, float *out_sumsq,
                                     const sjd_l2_head *head, int pf_blocks, void *stream)
{
    if (!head || pf_blocks < 1) return sjd_residual_sumsq(h, part, n_chunks, rows, hidden, dtype, out_sumsq, stream);
    if (!h || !out_sumsq || rows < 1 || rows > 256 || (part && n_chunks < 1) || hidden < 4 || (hidden % 4) != 0 || !head->wz) return SJD_ERR_BAD_ARG;
    const int prows = ((rows + 31) / 32) * 32, n_slices = (hidden + 511) / 512;
    // the pull's XCD arithmetic needs (i) F1r's own workgroup count and (ii) the pulling workgroup count to be multiples of 8
    int pf_rows = (pf_blocks + rows - 1) / rows;
    while ((pf_rows * rows) % 8) ++pf_rows;
    if ((rows * n_slices) % 8) return sjd_residual_sumsq(h, part, n_chunks, rows, hidden, dtype, out_sumsq, stream);
    const dim3 grid(rows, n_slices + pf_rows), block(128);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SJD_DTYPE_BF16)
        hipLaunchKernelGGL(f1r_residual_sumsq_pf<SJD_DTYPE_BF16>, grid, block, 0, s, (unsigned short *)h, part, n_chunks, hidden, prows, out_sumsq, n_slices, *head);
    else if (dtype == SJD_DTYPE_F16)
        hipLaunchKernelGGL(f1r_residual_sumsq_pf<SJD_DTYPE_F16>, grid, block, 0, s, (unsigned short *)h, part, n_chunks, hidden, prows, out_sumsq, n_slices, *head);
    else return SJD_ERR_UNSUPPORTED;
    return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
}
#endif  // SJD_EXPERIMENTAL

static int f3_launch(const void *gate_up, void *y, int rows, int inter, int dtype, const float *part, int n_chunks, const sjd_row_norm *rn,
                     void *stream)
{
    if (part && (rows > 256 || n_chunks < 1)) return SJD_ERR_BAD_ARG;
    if (rn && (!part || !rn->sumsq || rn->slices < 1 || rn->hidden < 1)) return SJD_ERR_BAD_ARG;
    const int prows = ((rows + 31) / 32) * 32;
    if ((!gate_up && !part) || !y || rows < 1 || inter < 8 || (inter % 8) != 0) return SJD_ERR_BAD_ARG;
    const size_t total = (size_t)rows * (inter / 8);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipStream_t s = (hipStream_t)stream;
    const float *ss = rn ? rn->sumsq : nullptr;
    const int sl = rn ? rn->slices : 0;
    const float ih = rn ? 1.0f / (float)rn->hidden : 0.f, eps = rn ? rn->eps : 0.f;
    if (dtype == SJD_DTYPE_BF16)
        hipLaunchKernelGGL(f3_silu_mul<SJD_DTYPE_BF16>, dim3(blocks), dim3(256), 0, s, (const unsigned short *)gate_up, (unsigned short *)y, rows, inter, part, n_chunks, prows, ss, sl, ih, eps);
    else if (dtype == SJD_DTYPE_F16)
        hipLaunchKernelGGL(f3_silu_mul<SJD_DTYPE_F16>, dim3(blocks), dim3(256), 0, s, (const unsigned short *)gate_up, (unsigned short *)y, rows, inter, part, n_chunks, prows, ss, sl, ih, eps);
    else return SJD_ERR_UNSUPPORTED;
    return hipGetLastError() == hipSuccess ? SJD_OK : SJD_ERR_LAUNCH;
}

extern "C" int sjd_silu_mul(const void *gate_up, void *y, int rows, int inter, int dtype, const float *part, int n_chunks, void *stream)
{
    return f3_launch(gate_up, y, rows, inter, dtype, part, n_chunks, nullptr, stream);
}

extern "C" int sjd_silu_mul_ex(const void *gate_up, void *y, int rows, int inter, int dtype, const float *part, int n_chunks,
                               const sjd_row_norm *row_norm, void *stream)
{
    return f3_launch(gate_up, y, rows, inter, dtype, part, n_chunks, row_norm, stream);
}
