// sjd_gemm_wide.h -- G1w: the weight-streaming projection for windows of 65..256 rows (three to eight prompts per forward), round 6.
// Included by sjd_gemm.hip (same packed weights, same fp32 split-K planes [n_chunks, 32 MT, N] as g1_skinny_gemm: bit for bit).
//
// Why a new structure (VERDICT r5 "next #1").  g1_skinny_gemm_tiled8 with eight row tiles ran at 0.27 of the HBM peak (48.5 us per launch at
// 256 rows): a wave owned ONE 32-column tile and read EIGHT activation fragments from LDS per weight record (8 KiB per 8 MFMAs: the LDS read
// port at its limit), the activation sub-tile travelled global -> VGPR -> ds_write_b128 -> barrier (64 KiB per eight k-steps through the
// 79 B/clk store path, interleaved loads do not hide it: MI355X_MICROARCH "LDS"), and a 128-column workgroup re-read the activation at
// TWICE the weight bytes.  Here:
//   * the activation never touches a VGPR on its way in: LDS-DMA (`buffer_load_dwordx4 ... offen lds`, 1 KiB per wave instruction) writes
//     stages of SUB k-steps x 32 MT rows straight into a ring of NS slots; NS - 1 stages are in flight per workgroup;
//   * the LDS image of a DMA is lane-linear (it cannot pad rows), so bank conflicts are avoided by permuting the SOURCE: 16-byte piece p of
//     row m lands at position p ^ swz(m) of the row, swz(m) = (m SUB / 8) mod 2 SUB -- the sixteen lanes of every ds_read_b128 lane group then
//     hit sixteen different 16-byte bank groups (checked for SUB = 2, 4, 8 against the lane groups of MI355X_MICROARCH's LDS table);
//   * a wave owns CT column tiles (CT = 2: every activation fragment read from LDS feeds two MFMAs -- half the LDS reads per flop) and all
//     MT row tiles; the weight records still go HBM -> MFMA B registers directly (the packed stream IS the operand order), through a ring of
//     R = (NS - 1) SUB k-steps per tile refilled in place;
//   * every load of the kernel is hand-written and hand-counted: the DMA has no destination register the compiler could wait for, and
//     the weight loads are `asm volatile` as well so that ONE in-order vmcnt sequence covers both.  The prologue issues exactly the
//     steady-state sequence (per k-step: the records of tiles 0 .. CT - 2 of the k-step R ahead, DPK DMA pieces of the stage NS - 1 ahead, the
//     record of the last tile -- each BETWEEN two MFMAs of the k-step, not in a burst behind the barrier), so the wait counts (N_W0, N_WL, N_A
//     in the kernel) are exact from the first stage on (a count larger than the number of younger operations would not wait at all);
//   * one raw s_barrier per stage: "my pieces of stage st landed" -> barrier (everybody's have; everybody is done with stage st - 1) ->
//     refill the slot stage st - 1 left -> SUB k-steps of MFMAs.
// Rows >= M and columns past the matrix read as zero through the buffer descriptor's range check; the columns past a ragged chunk's end are
// requested out of range (one compare + select per DMA piece), so the k-steps past the end multiply zero records by zero fragments: no branch.
// Same MFMA sequence per (column tile, K chunk, row tile) as g1_skinny_gemm: the planes are bit-identical to the 32-row kernel's
// (tests/test_gpu_glue.py::test_g1_skinny_gemm_five_to_eight_row_tiles compares them plane for plane).
#pragma once

template <int N> __device__ __forceinline__ void gw_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// the same, with the registers the wait makes valid passed THROUGH the statement: the compiler then cannot move a use above it
template <int N> __device__ __forceinline__ void gw_wait_regs(u32x4 &a) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void gw_wait_regs(u32x4 &a, u32x4 &b) { asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory"); }

// raw buffer descriptor over `bytes` bytes from `p` (wave-uniform); loads at or past `bytes` return zero without touching memory
__device__ __forceinline__ u32x4 gw_rsrc(const void *p, unsigned bytes)
{
    const unsigned long long a = (unsigned long long)p;
    u32x4 r;
    r[0] = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r[1] = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32)) & 0xffffu;       // stride 0: raw buffer
    r[2] = (unsigned)__builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = 0x00020000u;
    return r;
}

// one LDS-DMA piece: 64 lanes x 16 B from (descriptor base + voff + soff) to LDS bytes [lds_addr + 16 lane, + 16).  M0 is the compiler's: saved /
// restored inside the statement; the s_nop covers the M0 write -> LDS-DMA read hazard (sjd_attention_ring.h: k1r_dma16).
__device__ __forceinline__ void gw_dma16(u32x4 rsrc, unsigned voff, unsigned soff, unsigned lds_addr)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 2\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(rsrc), "s"(__builtin_amdgcn_readfirstlane((int)soff)), "s"(__builtin_amdgcn_readfirstlane((int)lds_addr))
                 : "memory");
}

// (12-bit form, late round 6) the waits that tie a record pair's registers / a unit header's registers
template <int N> __device__ __forceinline__ void gw_wait_regs(u32x4 &a, u32x2 &b) { asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void gw_wait_regs(u32x2 &a, u32x2 &b) { asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory"); }
// the codes of a record pair (64 lanes x 8 B), and one header entry per lane: like gw_wload, issued by hand and counted by hand
__device__ __forceinline__ u32x2 gw_wload2(u32x4 rsrc, unsigned voff, unsigned soff)
{
    u32x2 r;
    asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen nt" : "=v"(r) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
    return r;
}
__device__ __forceinline__ u32x2 gw_gload2(const void *p)
{
    u32x2 r;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}

// one weight record (1 KiB per wave) into B-operand registers, non-temporal (streamed once); NOT waited for by the compiler
__device__ __forceinline__ u32x4 gw_wload(u32x4 rsrc, unsigned voff, unsigned soff)
{
    u32x4 r;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen nt" : "=v"(r) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
    return r;
}

// (8-bit form) one fp32 column scale per lane, issued and counted by hand like the headers of the 12-bit form, and the wait that ties its register
__device__ __forceinline__ float gw_gload1(const void *p)
{
    float r;
    asm volatile("global_load_dword %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}
template <int N> __device__ __forceinline__ void gw_wait_regs(float &a) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(N) : "memory"); }
__device__ __forceinline__ u32x4 g1q_operand(unsigned b0, unsigned b1, float sc);        // csrc/sjd_gemm_q8.h
// (4-bit form) one scale dword (a trip's four e8m0 bytes) per lane through the unit's scale descriptor, and the wait that ties it with a record
__device__ __forceinline__ unsigned gw_wload1(u32x4 rsrc, unsigned voff, unsigned soff)
{
    unsigned r;
    asm volatile("buffer_load_dword %0, %1, %2, %3 offen nt" : "=v"(r) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
    return r;
}
template <int N> __device__ __forceinline__ void gw_wait_regs(u32x4 &a, unsigned &b) { asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory"); }
__device__ __forceinline__ u32x4 g1q4_operand(unsigned c, float sc);                      // csrc/sjd_gemm_q4.h
template <int B> __device__ __forceinline__ float g1q4_scale(unsigned sd);

__device__ __forceinline__ unsigned gw_lds_addr(const void *p)
{
    return (unsigned)(unsigned long)((__attribute__((address_space(3))) const unsigned char *)p);
}

// (timing probes, results invalid: -DGW_NO_MFMA the streams and the LDS traffic without the matrix cores, -DGW_NO_W no weight stream, -DGW_NO_DMA no
//  activation stream, -DGW_NO_STORE no partial planes, -DGW_NO_BARRIER no workgroup barrier)
#ifdef GW_NO_MFMA
template <int DT> __device__ __forceinline__ f32x16 gw_fake_mma(u32x4 a, u32x4 b, f32x16 c) { asm volatile("" ::"v"(a), "v"(b)); return c; }      // (operands kept alive, no instruction)
#define GW_MMA(a_, b_, c_) gw_fake_mma<DT>(a_, b_, c_)
#else
#define GW_MMA(a_, b_, c_) G1Mfma<DT>::mma(a_, b_, c_)
#endif
// MT row tiles (rows = 32 MT), CT column tiles per wave, NW waves (column groups) per workgroup, stages of SUB k-steps, NS ring slots,
// WPS = waves per SIMD the register budget is cut for (1: up to 512 registers; 2: 256 -- two workgroups of <= 4 waves per CU)
// Z (late round 6): the weights arrive as the LOSSLESS 12-bit stream of kernels G1z / G1sz (csrc/sjd_gemm.hip: 1536-byte record PAIRS of two k-steps --
// 64 lanes x 16 B of low bytes, 64 lanes x 8 B of codes -- and a header of exceptions per (chunk, tile) unit) and are decoded into the SAME B operands
// in front of their MFMAs (g1z_operand): bit-identical planes, 25 % fewer weight bytes.  One vector-memory operation per tile and k-step as before -- the
// low bytes of the pair R k-steps ahead behind an even k-step's last MFMA, its codes behind the odd one's -- so the hand counts stand; an even k-step
// decodes BOTH operands of its pair (its registers are then free for the refill) and waits one group less deep (the codes are one k-step younger than the
// low bytes); an odd k-step waits for nothing.  The unit headers are requested in front of the prologue and waited for behind it without draining it.
// WIDE: headers of 128 entries.  Raw units (a header count of -1) decode to garbage here: the entry points run the fix-up launch (sjd_gemm_raw.h) behind this one.
// Q ("G1wq"): the weights arrive as the 8-bit e4m3 stream of kernels G1q / G1sq (csrc/sjd_gemm_q8.h: 1024-byte record PAIRS of two k-steps, 64 lanes x
// 16 B, fp32 column scales behind the N_packed * K record bytes; K and KC multiples of 32, so every unit is whole pairs) and are rebuilt into the SAME B
// operands (g1q_operand: four conversions per k-step): the planes of the uncompressed form on pack_weight(dequant()), bit for bit, at half the weight
// bytes.  The ring is one u32x4 per tile and pair (R / 2 registers per tile); the pair R k-steps ahead is requested behind an even k-step's last MFMA, and
// an odd k-step issues an out-of-range DMA piece into the scratch KiB in its place (the prologue's trick: one instruction, no traffic, no register
// written), so every k-step still has one vector-memory operation per tile and N_W0 / N_WL / N_A stand as they are.  An even k-step waits for its pair
// (issued R k-steps earlier, at the same position: the plain counts) and decodes both operands; an odd one waits for nothing.  Pairs past a unit's end
// read as zero through the descriptor range, code 0 decodes to +0.0.  The scales are requested in front of the prologue and waited for behind it.
// Q && WIDE ("G1wq4"; WIDE has no other meaning without Z, and a new template parameter would rename every existing instantiation): the weights arrive
// as the MXFP4 stream of kernels G1q4 / G1sq4 (csrc/sjd_gemm_q4.h: 1024-byte RECORDS of four k-steps, 64 lanes x 16 B, dword i = the lane's eight codes
// of k-step 4 R + i; one e8m0 scale dword per lane and TRIP of eight k-steps behind the N_packed * K / 2 record bytes, laid out like the records; K and
// KC multiples of 128, so every unit is whole records and trips) and are rebuilt into the SAME B operands (g1q4_operand: four conversions per k-step, in
// front of the k-step's first MFMA): the planes of the uncompressed form on pack_weight(dequant()), bit for bit.  The ring R = 8 k-steps is exactly one
// trip: two record registers and one scale dword per tile.  One vector-memory operation per tile and k-step as before, in the tile's slot of ring k-step r:
//     r = 2  the NEXT trip's scale dword, into a landing register of its own (SDL; the current trip's dword was copied out of it at r = 0)
//     r = 3  the next trip's first record, into W[c][0] -- behind the last MFMA of the fourth and last k-step that register serves, whose operand was
//            decoded in front of that k-step's first MFMA: no load ever lands in a register that still holds undecoded codes
//     r = 7  the next trip's second record, into W[c][1], likewise
//     else   an out-of-range DMA piece into the scratch KiB (the Q form's odd k-steps)
// so N_W0 / N_WL / N_A stand.  A record is waited for at its first k-step (r = 0 / r = 4), FIVE k-steps behind its request at the same position of the
// group -- three groups less deep than the plain counts: N_WL - 3 GRP / N_W0 - 3 GRP younger operations.  The scale dword is requested one k-step BEFORE
// the trip's first record: vmcnt retires loads in order, so the wait for the record at r = 0 covers it (both registers ride through that wait).  Nothing
// is decoded ahead: per tile 8 (records) + 2 (scale dword, landing + current) + 4 (the operand, live for one tile's MFMAs) registers, against the Q
// form's 16 + 1 + 8.  Records and scale dwords past a unit's end read as zero through the descriptor ranges; code 0 decodes to +0.0 under any scale.
template <int DT, int MT, int CT, int NW, int SUB, int NS, int RW, int WPS, bool Z = false, bool WIDE = false, bool Q = false>
__global__ __launch_bounds__(64 * NW, WPS) void g1_wide(const unsigned short *__restrict__ x, const u32x4 *__restrict__ wp, float *__restrict__ out,
                                                        int M, int N, int K, int KC, int n_tiles, int rec_stride, int tile0, int ldx, int xmap,
                                                        const u32x2 *__restrict__ exc, int exc_cap)
{
    static_assert(!Z || (DT == SJD_DTYPE_BF16 && SUB % 2 == 0 && (RW * SUB) % 2 == 0), "the 12-bit stream: bf16, whole record pairs per stage and ring");
    static_assert(!Q || (!Z && DT == SJD_DTYPE_BF16 && SUB % 2 == 0 && (RW * SUB) % 2 == 0), "the 8-bit stream: bf16, whole record pairs per stage and ring");
    constexpr bool Q4 = Q && WIDE, Q8 = Q && !WIDE;          // the 4-bit / the 8-bit stream
    static_assert(!Q4 || RW * SUB == 8, "the 4-bit stream: the weight ring is exactly one trip of eight k-steps (two records, one scale dword)");
    static_assert(SUB == 2 || SUB == 4 || SUB == 8, "a stage is 2, 4 or 8 k-steps");
    static_assert(CT == 1 || CT == 2, "one or two column tiles per wave");
    // The weight ring is RW stages (R k-steps) deep, the activation ring LA = NS - 1 stages ahead.  LA > RW matters: vmcnt retires in order, so the
    // wait for the (L2-resident, fast) pieces of stage st also waits for every weight record issued before them -- with LA == RW those are the
    // records of stage st itself, i.e. the top of every stage drained the weight ring (the two streams alone cost +2.5 / +0.5 us over the
    // arithmetic, together +7.3: profiles/r6_g1w_probes.txt); with LA = RW + 1 they are the records of stage st - 1, consumed already.
    constexpr int LA = NS - 1, R = RW * SUB;
    static_assert(LA >= RW && RW >= 1, "the activation ring is at least as far ahead as the weight ring");
    constexpr int ROWB = SUB * 32;                // bytes per activation row and stage
    constexpr int LPR = SUB * 2;                  // 16-byte pieces (DMA lanes) per row
    constexpr int RPP = 64 / LPR;                 // rows per DMA piece (1 KiB)
    constexpr int P = MT * SUB;                   // DMA pieces per stage
    constexpr int DPK = (P + NW * SUB - 1) / (NW * SUB);      // ... per wave and k-step (the pieces of a stage are issued spread over the k-steps of a stage)
    constexpr int NA = DPK * SUB;                 // ... per wave and stage
    constexpr bool DUMMY = NA * NW != P;          // some wave's last pieces lie past the stage: issued out of range into a scratch KiB (uniform counts)
    constexpr int SLOT = P * 1024;
    constexpr int NM = MT * CT;                   // MFMAs per k-step, tile-major: MFMA i = (tile i / MT, row tile i % MT)
    // vector-memory operations of a k-step in issue order: [records of tiles 0 .. CT - 2] [DPK DMA pieces] [record of tile CT - 1]
    constexpr int GRP = CT + DPK;
    constexpr int D0 = MT * (CT - 1) + 1;         // the DMA pieces follow MFMA D0, D0 + DSTR, ...
    constexpr int DSTR = (D0 + 2 * (DPK - 1) < NM - 1) ? 2 : 1;
    // (the last piece may share the last MFMA's slot with the record reload of tile CT - 1: the piece is issued first there, the order the counts assume)
    static_assert(D0 + DSTR * (DPK - 1) <= NM - 1, "the DMA pieces fit between the record loads");
    // younger operations when tile c's records of k-step s are waited for (issued R k-steps earlier), and when the last piece of stage st is
    constexpr int N_WL = (R - 1) * GRP + (CT - 1);                       // the last tile's record closes its group; the earlier tiles' of THIS k-step are out again
    constexpr int N_W0 = (R - 1) * GRP + DPK + 1;                        // (CT = 2) tile 0: the pieces and the last record of its own group follow it
    constexpr int N_A = (LA - 1) * SUB * GRP + 1;
    static_assert(N_A <= 63 && N_WL <= 63 && N_W0 <= 63, "vmcnt is a 6-bit counter");
    // (Q4) a record is requested at ring k-step 3 / 7 and first used at 0 / 4 of the next trip: 5 k-steps, i.e. 4 whole groups and the same partial one
    constexpr int N_WL4 = N_WL - 3 * GRP, N_W04 = N_W0 - 3 * GRP;
    static_assert(!Q4 || (N_WL4 == 4 * GRP + (CT - 1) && N_W04 == 4 * GRP + DPK + 1), "five k-steps between a record's request and its first use");
    static_assert(NS >= 2, "at least two slots");
    extern __shared__ __attribute__((aligned(1024))) unsigned char gw_lds[];       // NS slots, then 1 KiB of scratch
    SJD_TR(0);
    SJD_TR_CLK(4);             // (shader-clock stamps next to the 100 MHz wall-clock ones: the clock the launch actually ran at)
    // XCD-aware (column group, K chunk) of this workgroup.  Workgroup L = x + gridDim.x * y runs on XCD L mod 8, and every XCD has its own L2: with the
    // plain (x, y) = (column group, chunk) map the workgroups of one chunk are spread over all eight XCDs, so every XCD's L2 holds the activation
    // columns of EVERY chunk -- 5.6 MB for the down projection at 256 rows against 4 MB of L2: PMC showed 45 MB of activation re-reads going to HBM
    // (profiles/g1w_traffic.json).  With a power-of-two chunk count the chunk follows the XCD instead (chunk = XCD mod n_chunks; sixteen and more
    // chunks: XCD + 8 * ...), an XCD then re-reads 1 / min(8, n_chunks) of the activation.  Which workgroup computes which (tile, chunk) does not
    // change any result.  xmap = 0: the plain map (four row tiles and below).
    int bx = blockIdx.x, chunk = blockIdx.y;
    {
        const int gx = gridDim.x, nc = gridDim.y;
        if (xmap && nc > 1 && (nc & (nc - 1)) == 0) {
            const int total = gx * nc, lin = bx + gx * chunk, full = total & ~7;
            if (nc <= 8) {
                const int per = 8 / nc, b0 = (full >> 3) * per;          // column groups covered by the whole rounds of eight workgroups
                if (lin < full) { const int xcd = lin & 7, slot = lin >> 3; chunk = xcd % nc; bx = slot * per + xcd / nc; }
                else { const int j = lin - full, rest = gx - b0; bx = b0 + j % rest; chunk = j / rest; }
            } else if (total == full) {
                const int q = nc >> 3, xcd = lin & 7, slot = lin >> 3;
                chunk = xcd + 8 * (slot % q); bx = slot / q;
            }
        }
    }
    const int k0 = chunk * KC;
    const int steps = min(KC, K - k0) / 16;
    const int n_stage = (steps + SUB - 1) / SUB;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned rsb = (unsigned)rec_stride * (Z ? 1536u : 1024u);
    [[maybe_unused]] const unsigned ssb = (unsigned)rec_stride * 128u;           // (Q4) bytes from a trip's scale group to the unit's next
    const int pairs = (steps + 1) / 2, pairs_full = (KC / 16 + 1) / 2;          // (Z) record pairs of this unit / of a full chunk's unit
    const size_t chunk_base = (size_t)chunk * n_tiles * (Z ? pairs_full : KC / 16);
    u32x4 wr[CT];
    [[maybe_unused]] u32x4 sr[CT];                                               // (Q4) the descriptor of the unit's scale groups
    int t_out[CT];
    [[maybe_unused]] u32x2 hra[CT], hrb[CT];                                     // (Z) this lane's header entries of the tiles' units
    [[maybe_unused]] float qs[CT];                                               // (Q) this lane's column scale of each tile
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        t_out[c] = (bx * NW + w) * CT + c;
        const bool has = t_out[c] < N / 32;
        const int t = tile0 + (has ? t_out[c] : 0);
        if constexpr (Z) {
            const size_t tile_off = (rec_stride == 1) ? (size_t)t * pairs : (size_t)t;
            wr[c] = gw_rsrc(reinterpret_cast<const unsigned char *>(wp) + (chunk_base + tile_off) * 1536, has ? (unsigned)(pairs - 1) * rsb + 1536u : 0u);
            const u32x2 *e = exc + ((size_t)chunk * n_tiles + t) * (size_t)exc_cap;
            hra[c] = gw_gload2(e + min(lane, exc_cap - 1));
            if constexpr (WIDE) hrb[c] = gw_gload2(e + 64 + lane); else hrb[c] = u32x2{0xffffffffu, 0xffffffffu};
        } else if constexpr (Q4) {         // a chunk starts at byte k0 * N_packed / 2 (scales: k0 * N_packed / 32); tile-major: a unit is steps * 256 (* 16) contiguous bytes
            const unsigned char *wq = reinterpret_cast<const unsigned char *>(wp);
            const unsigned char *sq = wq + (size_t)n_tiles * 16 * K;
            const size_t tile_off = (rec_stride == 1) ? (size_t)t * steps * 256 : (size_t)t * 1024;
            const size_t stile_off = (rec_stride == 1) ? (size_t)t * steps * 16 : (size_t)t * 128;
            wr[c] = gw_rsrc(wq + (size_t)k0 * ((size_t)n_tiles * 16) + tile_off, has ? (unsigned)(steps / 4 - 1) * rsb + 1024u : 0u);
            sr[c] = gw_rsrc(sq + (size_t)k0 * (size_t)n_tiles + stile_off, has ? (unsigned)(steps / 8 - 1) * ssb + 128u : 0u);
        } else if constexpr (Q) {          // a chunk starts at byte k0 * N_packed; tile-major: a unit is steps * 512 contiguous bytes, step-major: pair p of every tile
            const unsigned char *wq = reinterpret_cast<const unsigned char *>(wp);
            const size_t tile_off = (rec_stride == 1) ? (size_t)t * steps * 512 : (size_t)t * 1024;
            wr[c] = gw_rsrc(wq + (size_t)k0 * ((size_t)n_tiles * 32) + tile_off, has ? (unsigned)(pairs - 1) * rsb + 1024u : 0u);
            qs[c] = gw_gload1(reinterpret_cast<const float *>(wq + (size_t)n_tiles * 32 * K) + 32 * t + (lane & 31));
        } else {
            const size_t tile_off = (rec_stride == 1) ? (size_t)t * steps : (size_t)t;
#ifdef GW_NO_W            // (timing probe, results invalid: no weight stream -- every record out of range)
            wr[c] = gw_rsrc(wp + (chunk_base + tile_off) * 64, 0u);
#else
            wr[c] = gw_rsrc(wp + (chunk_base + tile_off) * 64, has ? (unsigned)(steps - 1) * rsb + 1024u : 0u);      // (no tile: every record reads as zero)
#endif
        }
    }
    const u32x4 xr = gw_rsrc(x, (unsigned)M * (unsigned)ldx * 2u);      // (ldx: row stride of x in elements, >= K)
    const unsigned lds0 = gw_lds_addr(gw_lds);
    // this wave's DMA pieces of a stage: piece j = w NA + i covers rows j RPP .. + RPP - 1; lane l -> row j RPP + l / LPR, position l % LPR of the
    // row, which receives source piece (l % LPR) ^ swz(row)
    unsigned xoff[NA], xcol[NA];          // byte offset of the lane's 16 bytes in x; its column inside the stage
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int j = w * NA + i;
        const int row = j * RPP + lane / LPR, pos = lane % LPR;
        const int p = pos ^ ((((row & 31) * SUB) >> 3) & (LPR - 1));
        xoff[i] = (!DUMMY || j < P) ? ((unsigned)row * (unsigned)ldx + (unsigned)(k0 + 8 * p)) * 2u : 0x7fff0000u;
        xcol[i] = (unsigned)(8 * p);
    }
    const int chunk_cols = steps * 16;
    // A-fragment read offsets inside a slot: lane (m = l & 31, h = l >> 5), k-step u of the stage: row m, piece (2 u + h) ^ swz(m)
    unsigned aoff[SUB];
    {
        const int m = lane & 31, h = lane >> 5;
        const int sw = ((m * SUB) >> 3) & (LPR - 1);
#pragma unroll
        for (int u = 0; u < SUB; ++u) aoff[u] = (unsigned)(m * ROWB + 16 * ((2 * u + h) ^ sw));
    }
    const unsigned wvoff = (unsigned)lane * 16u;
    const unsigned piece0 = lds0 + (unsigned)(w * NA) * 1024u;        // this wave's first piece inside slot 0
    const unsigned scratch = lds0 + (unsigned)(NS * SLOT);

    // piece d of k-step position u of activation stage `sa`, into the ring slot at LDS address `sb` (+ this wave's piece offset)
    auto dma_piece = [&](int sa, unsigned sb, int u, int d) {
#ifdef GW_NO_DMA          // (timing probe: the activation pieces are issued out of range -- same instructions, no traffic)
        const unsigned soff = 0x7fff0000u;
#else
        const unsigned soff = sa < n_stage ? (unsigned)sa * ROWB : 0x7fff0000u;       // past the chunk: out of range (zeros, no traffic)
#endif
        const int i = u * DPK + d;
        unsigned dst = sb + (unsigned)i * 1024u;
        if constexpr (DUMMY) dst = (w * NA + i < P) ? dst : scratch;
        // a column past a ragged chunk's end belongs to the next chunk (or the next row): it is fetched out of range, i.e. lands as zeros, and the
        // k-steps past the end multiply zero records by zero fragments (+0 added to an accumulator that is never -0 leaves every bit as it is)
        const unsigned voff = (int)xcol[i] < chunk_cols - sa * (SUB * 16) ? xoff[i] : 0x7fff0000u;
        gw_dma16(xr, voff, soff, dst);
    };
    u32x4 W[CT][Q4 ? R / 4 : (Z || Q) ? R / 2 : R];       // plain: one record per k-step of the ring; Z: the low bytes of one record pair per two k-steps; Q: the pair; Q4: the record of four
    [[maybe_unused]] unsigned SDL[CT], SDC[CT];            // (Q4) the scale dword of the next trip (landing) / of the current one
    [[maybe_unused]] u32x2 WC[CT][R / 2];    // (Z) ... and its codes
    [[maybe_unused]] u32x4 Bn[CT];           // (Z, Q) the odd k-step's operand, decoded with the even one's
    // (Z) record load of ring k-step ks: even -> the pair's low bytes, odd -> its codes
    auto z_load = [&](int c, int ks_ring, unsigned pair_abs) {
        if ((ks_ring & 1) == 0) W[c][ks_ring >> 1] = gw_wload(wr[c], wvoff, pair_abs * rsb);
        else WC[c][ks_ring >> 1] = gw_wload2(wr[c], 1024u + (unsigned)lane * 8u, pair_abs * rsb);
    };
    // (Q) record load of ring k-step ks: even -> the pair, odd -> an out-of-range piece into the scratch KiB (counted, no traffic, no register)
    auto q_load = [&](int c, int ks_ring, unsigned pair_abs) {
        if ((ks_ring & 1) == 0) W[c][ks_ring >> 1] = gw_wload(wr[c], wvoff, pair_abs * rsb);
        else gw_dma16(xr, 0x7fff0000u, 0u, scratch);
    };
    // (Q4) the load of ring k-step ks for the trip that holds k-step `tgt` (the same ring position, R k-steps on): see the table in the header comment
    [[maybe_unused]] const unsigned svoff = (unsigned)(lane & 31) * 4u;
    auto q4_load = [&](int c, int ks_ring, unsigned tgt) {
        if ((ks_ring & 7) == 2) SDL[c] = gw_wload1(sr[c], svoff, (tgt >> 3) * ssb);
        else if ((ks_ring & 3) == 3) W[c][(ks_ring >> 2) & 1] = gw_wload(wr[c], wvoff, (tgt >> 2) * rsb);
        else gw_dma16(xr, 0x7fff0000u, 0u, scratch);
    };
    f32x16 acc[CT][MT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][mt][r] = 0.0f;

    // ---- prologue: the steady-state issue sequence of the virtual stages -LA .. -1.  A record load whose k-step would be negative is replaced by an
    // out-of-range DMA piece into the scratch KiB: the counts stay uniform, and NO register is written -- a dummy register load would land
    // asynchronously in a register the compiler considers dead and has handed to somebody else by then (it did: wrong planes, first version)
#pragma unroll
    for (int v = 0; v < LA; ++v)
#pragma unroll
        for (int u = 0; u < SUB; ++u) {
            const int ks = (v - (LA - RW)) * SUB + u;         // k-step of this group's records
#pragma unroll
            for (int c = 0; c < CT - 1; ++c) {
                if (ks >= 0) { if constexpr (Z) z_load(c, ks, (unsigned)(ks >> 1)); else if constexpr (Q4) q4_load(c, ks, (unsigned)ks); else if constexpr (Q) q_load(c, ks, (unsigned)(ks >> 1)); else W[c][ks] = gw_wload(wr[c], wvoff, (unsigned)ks * rsb); }
                else gw_dma16(xr, 0x7fff0000u, 0u, scratch);
            }
#pragma unroll
            for (int d = 0; d < DPK; ++d) dma_piece(v, piece0 + (unsigned)(v * SLOT), u, d);
            if (ks >= 0) { if constexpr (Z) z_load(CT - 1, ks, (unsigned)(ks >> 1)); else if constexpr (Q4) q4_load(CT - 1, ks, (unsigned)ks); else if constexpr (Q) q_load(CT - 1, ks, (unsigned)(ks >> 1)); else W[CT - 1][ks] = gw_wload(wr[CT - 1], wvoff, (unsigned)ks * rsb); }
            else gw_dma16(xr, 0x7fff0000u, 0u, scratch);
        }
    // (Z) the unit headers: requested in front of the prologue, complete once no more than the prologue's own LA * SUB * GRP operations are outstanding
    [[maybe_unused]] g1z_hdr hd[CT];
    if constexpr (Z) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            gw_wait_regs<LA * SUB * GRP>(hra[c], hrb[c]);
            hd[c] = g1z_header<WIDE>(g1z_hraw{hra[c], hrb[c]}, lane, exc_cap);
        }
    }
    if constexpr (Q8) {        // the column scales: likewise
#pragma unroll
        for (int c = 0; c < CT; ++c) gw_wait_regs<LA * SUB * GRP>(qs[c]);
    }
    SJD_TR(1);
    // one k-step: the MFMAs in tile-major order, ONE other instruction group behind each of them (a single wave per SIMD issues in order: what is
    // not placed between two MFMAs is not hidden by them -- the first version issued its 16 MFMAs back to back and then ~45 other instructions:
    // 33 % of the wave's cycles were spent issuing while the matrix pipe idled, profiles/r6_g1w_first_pmc.txt):
    //   behind MFMA i < MT: the A fragment of row tile i for the NEXT k-step;  behind the last MFMA of tile c: its record R k-steps ahead;
    //   behind MFMA D0 + DSTR d: DMA piece d of the stage NS - 1 ahead;  in front of the first MFMA of tile c: the wait for its records.
    auto k_step = [&](const unsigned char *sl, int u, int r, int st, unsigned sb_refill, u32x4 (&a)[2][MT]) {
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            const int c = i / MT, mt = i % MT;
            u32x4 b;
            if constexpr (Z) {
                if (mt == 0 && (r & 1) == 0) {            // an even k-step: both loads of its pair have landed once one group fewer is outstanding
                    if (c == CT - 1) gw_wait_regs<N_WL - GRP>(W[c][r >> 1], WC[c][r >> 1]); else gw_wait_regs<N_W0 - GRP>(W[c][r >> 1], WC[c][r >> 1]);
                    const unsigned s_abs = (unsigned)(st * SUB + u);
                    Bn[c] = g1z_operand<WIDE>(W[c][r >> 1].z, W[c][r >> 1].w, WC[c][r >> 1].y, s_abs + 1u, hd[c], lane);
                    W[c][r >> 1] = g1z_operand<WIDE>(W[c][r >> 1].x, W[c][r >> 1].y, WC[c][r >> 1].x, s_abs, hd[c], lane);      // (held in the pair's own registers until its last MFMA)
                }
                b = (r & 1) == 0 ? W[c][r >> 1] : Bn[c];
            } else if constexpr (Q4) {
                if (mt == 0) {
                    if ((r & 3) == 0) {                   // a record's first k-step: requested five k-steps ago at this position (r = 0: the scale dword one more)
                        u32x4 &rec = W[c][(r >> 2) & 1];
                        if ((r & 7) == 0) {
                            if (c == CT - 1) gw_wait_regs<N_WL4>(rec, SDL[c]); else gw_wait_regs<N_W04>(rec, SDL[c]);
                            SDC[c] = SDL[c];              // (the landing register is free for the request at r = 2)
                        } else {
                            if (c == CT - 1) gw_wait_regs<N_WL4>(rec); else gw_wait_regs<N_W04>(rec);
                        }
                    }
                    const u32x4 &rec = W[c][(r >> 2) & 1];
                    const unsigned code = (r & 3) == 0 ? rec.x : (r & 3) == 1 ? rec.y : (r & 3) == 2 ? rec.z : rec.w;
                    const int sb = (r >> 1) & 3;
                    const float sc = sb == 0 ? g1q4_scale<0>(SDC[c]) : sb == 1 ? g1q4_scale<1>(SDC[c]) : sb == 2 ? g1q4_scale<2>(SDC[c]) : g1q4_scale<3>(SDC[c]);
                    Bn[c] = g1q4_operand(code, sc);       // (decoded in front of the k-step's first MFMA: behind its last one the record may be refilled)
                }
                b = Bn[c];
            } else if constexpr (Q) {
                if (mt == 0 && (r & 1) == 0) {            // an even k-step: its pair was requested R k-steps ago at this position
                    if (c == CT - 1) gw_wait_regs<N_WL>(W[c][r >> 1]); else gw_wait_regs<N_W0>(W[c][r >> 1]);
                    Bn[c] = g1q_operand(W[c][r >> 1].z, W[c][r >> 1].w, qs[c]);
                    W[c][r >> 1] = g1q_operand(W[c][r >> 1].x, W[c][r >> 1].y, qs[c]);      // (held in the pair's own register until its last MFMA)
                }
                b = (r & 1) == 0 ? W[c][r >> 1] : Bn[c];
            } else {
                if (mt == 0) {
                    if (c == CT - 1) gw_wait_regs<N_WL>(W[c][r]); else gw_wait_regs<N_W0>(W[c][r]);
                }
                b = W[c][r];
            }
            acc[c][mt] = GW_MMA(a[u & 1][mt], b, acc[c][mt]);
            if (i < MT && u + 1 < SUB) a[(u + 1) & 1][i] = *reinterpret_cast<const u32x4 *>(sl + i * (32 * ROWB) + aoff[u + 1]);
            if (i >= D0 && ((i - D0) % DSTR) == 0 && (i - D0) / DSTR < DPK) dma_piece(st + LA, sb_refill, u, (i - D0) / DSTR);
            if (mt == MT - 1) {
                if constexpr (Z) z_load(c, r, (unsigned)((st * SUB + u + R) >> 1));
                else if constexpr (Q4) q4_load(c, r, (unsigned)(st * SUB + u + R));
                else if constexpr (Q) q_load(c, r, (unsigned)((st * SUB + u + R) >> 1));
                else W[c][r] = gw_wload(wr[c], wvoff, (unsigned)(st * SUB + u + R) * rsb);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    int slot = 0, refill = LA;              // slot of stage st; slot stage st + LA goes into (= the one stage st - 1 has left)
    for (int st0 = 0; st0 < n_stage; st0 += RW) {
#pragma unroll
        for (int q = 0; q < RW; ++q) {
            const int st = st0 + q;
            if (st >= n_stage) break;
            gw_wait<N_A>();                       // this wave's pieces of stage st have landed
#ifndef GW_NO_BARRIER
            __builtin_amdgcn_s_barrier();         // ... everybody's; everybody is done reading stage st - 1
#endif
            const unsigned char *sl = gw_lds + slot * SLOT;
            const unsigned sb_refill = piece0 + (unsigned)(refill * SLOT);
            u32x4 a[2][MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[0][mt] = *reinterpret_cast<const u32x4 *>(sl + mt * (32 * ROWB) + aoff[0]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < SUB; ++u) k_step(sl, u, q * SUB + u, st, sb_refill, a);
            refill = slot;
            slot = slot + 1 == NS ? 0 : slot + 1;
        }
    }
    SJD_TR(3);
    SJD_TR_CLK(5);
    gw_wait<0>();          // (the tail's out-of-range pieces: nothing may still be writing this workgroup's LDS when it exits)
#ifdef GW_NO_STORE
    if (acc[0][0][0] != 12345.0f) return;
#endif
    // The fp16 forms with five to eight row tiles take the lane index for the plane stores from the hardware again here, behind the last wait (a volatile
    // statement stays behind gw_wait<0>, so nothing of it is live in the loop): carried from the top of the kernel, `lane & 31` is live across the whole main loop, and with eight row tiles x two column
    // tiles (256 accumulators + both rings) it was the one register too many -- stored to scratch in front of the loop and reloaded here.  (The bf16 forms
    // keep the carried index: their code objects are unchanged; the two with eight row tiles x two column tiles have that same store / reload pair outside
    // the loop)
    int el = lane;
    if constexpr (DT == SJD_DTYPE_F16 && MT > 4) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(el));
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        if (t_out[c] >= N / 32) continue;
        float *o = out + ((size_t)chunk * (32 * MT)) * N + (size_t)t_out[c] * 32 + (el & 31);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (el >> 5);
                o[(size_t)m * N] = acc[c][mt][r];
            }
    }
#ifdef SJD_TRACE
    SJD_TR(2);                    // plane stores issued
    __builtin_amdgcn_s_waitcnt(0x0F70);
    SJD_TR(6);                    // acknowledged
#endif
}

// LDS bytes of a g1_wide launch
template <int MT, int SUB, int NS> constexpr size_t g1_wide_lds() { return (size_t)NS * MT * SUB * 1024 + 1024; }

template <int DT, int MT, int CT, int NW, int SUB, int NS, int RW, int WPS>
static int g1_wide_launch(const void *x, const void *w_packed, float *out, int M, int N, int K, int KC, int n_tiles, int step_major, int tile0, hipStream_t s, int ldx = 0)
{
    const int n_out = N / 32, n_chunks = (K + KC - 1) / KC;
    const dim3 grid((n_out + NW * CT - 1) / (NW * CT), n_chunks), block(64 * NW);
    constexpr size_t lds = g1_wide_lds<MT, SUB, NS>();
    static_assert(lds <= 160 * 1024, "the activation ring must fit in LDS");
    // (the XCD-aware map pays where the activation outgrows an XCD's L2 share: eight prompts 6.75 -> 6.58 ms per step, two alternations on one box; at 128
    //  rows and below it is neutral end to end and costs the gate|up launch 3 us alone: plain map there.  profiles/r6_g1w_xmap_ab.txt)
    constexpr int xmap = MT > 4;
    return g1_launch_kernel(g1_wide<DT, MT, CT, NW, SUB, NS, RW, WPS>, grid, block, lds, s, x, w_packed, out, M, N, K, KC, n_tiles, step_major ? n_tiles : 1, tile0,
                            ldx > 0 ? ldx : K, xmap, nullptr, 0);
}

// the same over the 12-bit stream (wz: record pairs, exc: unit headers of exc_cap entries); bf16
template <int MT, int CT, int NW, int SUB, int NS, int RW, int WPS>
static int g1_wide_launch_z(const void *x, const void *wz, const void *exc, int exc_cap, float *out, int M, int N, int K, int KC, int n_tiles, int step_major, int tile0,
                            hipStream_t s)
{
    const int n_out = N / 32, n_chunks = (K + KC - 1) / KC;
    const dim3 grid((n_out + NW * CT - 1) / (NW * CT), n_chunks), block(64 * NW);
    constexpr size_t lds = g1_wide_lds<MT, SUB, NS>();
    static_assert(lds <= 160 * 1024, "the activation ring must fit in LDS");
    constexpr int xmap = MT > 4;
#define SJD_G1WZ(WIDE_) \
    return g1_launch_kernel(g1_wide<SJD_DTYPE_BF16, MT, CT, NW, SUB, NS, RW, WPS, true, WIDE_>, grid, block, lds, s, x, wz, out, M, N, K, KC, n_tiles, \
                            step_major ? n_tiles : 1, tile0, K, xmap, exc, exc_cap)
    if (exc_cap > 64) SJD_G1WZ(true); else SJD_G1WZ(false);
#undef SJD_G1WZ
}

// G1wq: the same over the 8-bit e4m3 stream (wq: record pairs, then the fp32 column scales at byte N_packed * K); bf16, K and KC multiples of 32
// G1wq4 (Q4 = true): the same over the MXFP4 stream (wq: records of four k-steps, then the e8m0 scale dwords at byte N_packed * K / 2); K and KC multiples of 128
template <int MT, int CT, int NW, int SUB, int NS, int RW, int WPS, bool Q4 = false>
static int g1_wide_launch_q(const void *x, const void *wq, float *out, int M, int N, int K, int KC, int n_tiles, int step_major, int tile0, hipStream_t s)
{
    const int n_out = N / 32, n_chunks = (K + KC - 1) / KC;
    const dim3 grid((n_out + NW * CT - 1) / (NW * CT), n_chunks), block(64 * NW);
    constexpr size_t lds = g1_wide_lds<MT, SUB, NS>();
    static_assert(lds <= 160 * 1024, "the activation ring must fit in LDS");
    constexpr int xmap = MT > 4;
    return g1_launch_kernel(g1_wide<SJD_DTYPE_BF16, MT, CT, NW, SUB, NS, RW, WPS, false, Q4, true>, grid, block, lds, s, x, wq, out, M, N, K, KC, n_tiles,
                            step_major ? n_tiles : 1, tile0, K, xmap, nullptr, 0);
}

// Column tiles per workgroup -> the G1w instantiation (stages of four k-steps, three ring slots, weight ring of two stages): 2, 3, 4 tiles run one per
// wave, 6 and 8 two per wave.  WPS: workgroups per SIMD the register budget allows; Q: 8 the e4m3 stream, 4 the MXFP4 stream (g1_wide_launch_q, bf16).  G1W_NO_FORM, with
// nothing launched, for a count kernel G1w does not take -- the caller falls back or refuses.
constexpr int G1W_NO_FORM = 1;          // internal: every caller maps it to an SJD_* code or a fall-back -- it must never leave this translation unit
static_assert(G1W_NO_FORM != SJD_OK && G1W_NO_FORM != SJD_ERR_BAD_ARG && G1W_NO_FORM != SJD_ERR_UNSUPPORTED && G1W_NO_FORM != SJD_ERR_LAUNCH, "not a return code");
template <int DT, int MT, int WPS, int Q = 0>
static int g1_wide_by_tiles(int tiles, const void *x, const void *w, float *out, int M, int N, int K, int KC, int n_tiles, int step_major, int tile0, hipStream_t s)
{
    auto launch = [&](auto ct, auto nw) {
        constexpr int CT = decltype(ct)::value, NW = decltype(nw)::value;
        if constexpr (Q != 0) return g1_wide_launch_q<MT, CT, NW, 4, 3, 2, WPS, Q == 4>(x, w, out, M, N, K, KC, n_tiles, step_major, tile0, s);
        else return g1_wide_launch<DT, MT, CT, NW, 4, 3, 2, WPS>(x, w, out, M, N, K, KC, n_tiles, step_major, tile0, s);
    };
    using one = std::integral_constant<int, 1>;
    using two = std::integral_constant<int, 2>;
    switch (tiles) {
    // (three row tiles x two waves: a k-step has too few MFMAs to carry its DMA pieces -- no two-tile form at three row tiles)
    case 2: if constexpr (MT != 3) return launch(one{}, two{}); else return G1W_NO_FORM;
    case 3: return launch(one{}, std::integral_constant<int, 3>{});
    case 4: return launch(one{}, std::integral_constant<int, 4>{});
    case 6: return launch(two{}, std::integral_constant<int, 3>{});
    case 8: return launch(two{}, std::integral_constant<int, 4>{});
    default: return G1W_NO_FORM;
    }
}

// f(std::integral_constant<int, MT>) for the row-tile count MT = ceil(M / 32) in [LO, HI]: the one place a row count becomes a template argument
template <int LO, int HI, typename F>
static int g1_by_row_tiles(int M, F &&f)
{
    if constexpr (LO < HI) { if (M > 32 * LO) return g1_by_row_tiles<LO + 1, HI>(M, f); }
    return f(std::integral_constant<int, LO>{});
}

// SJD_G1_W8_E4M3 at 65..256 rows (g1q_launch, which has checked the column window): `waves` = column tiles per workgroup, the template shapes of the
// uncompressed dispatch (g1_launch) per row-tile count.  Anything G1wq has no form for: SJD_ERR_UNSUPPORTED before a launch.
static int g1wq_launch(const void *x, const void *wq, float *out, int M, int N, int K, int KC, int waves, int step_major, int n_tiles, int tile0, hipStream_t s)
{
    if (M <= 64 || M > 256 || (K % 32) != 0 || (KC % 32) != 0) return SJD_ERR_UNSUPPORTED;
    const int rc = g1_by_row_tiles<3, 8>(M, [&](auto mt) {
        return g1_wide_by_tiles<SJD_DTYPE_BF16, decltype(mt)::value, 1, 8>(waves, x, wq, out, M, N, K, KC, n_tiles, step_major, tile0, s); });
    return rc == G1W_NO_FORM ? SJD_ERR_UNSUPPORTED : rc;
}

// SJD_G1_W4_MXFP4 at 65..256 rows (g1q4_launch, which has checked the column window): kernel G1wq4 on the same template shapes; K and KC whole trips.
static int g1wq4_launch(const void *x, const void *wq, float *out, int M, int N, int K, int KC, int waves, int step_major, int n_tiles, int tile0, hipStream_t s)
{
    if (M <= 64 || M > 256 || (K % 128) != 0 || (KC % 128) != 0) return SJD_ERR_UNSUPPORTED;
    const int rc = g1_by_row_tiles<3, 8>(M, [&](auto mt) {
        return g1_wide_by_tiles<SJD_DTYPE_BF16, decltype(mt)::value, 1, 4>(waves, x, wq, out, M, N, K, KC, n_tiles, step_major, tile0, s); });
    return rc == G1W_NO_FORM ? SJD_ERR_UNSUPPORTED : rc;
}
