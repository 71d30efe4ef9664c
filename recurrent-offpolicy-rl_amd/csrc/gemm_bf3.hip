// fp32 GEMM on the bf16 matrix cores of gfx950, second edition: the operands are split ONCE PER BLOCK, on their way into LDS.
//
//     C[b][m][n] = epi( sum_k A[b](m, k) * B[b](n, k) )          same contract and operand layouts as gemm_f32.hip
//
// Product formation (resel_gemm_f32 mode 6, gemm_f32.hip 'SPLIT'): every fp32 operand element x is written exactly as
// x1 + x2 + x3, three bf16 values obtained by truncation; a bf16 x bf16 product is exact in fp32 and v_mfma_f32_32x32x16_bf16
// accumulates the plane products in fp32.  Mode 6 keeps six of the nine plane products: it drops a2 b3, a3 b2, a3 b3 (each at
// most 2^-24 |a b|).  Mode 3 ("bf16x3", what torch.set_float32_matmul_precision('high') names) keeps two planes per operand -
// 16 significant bits - and the products a1 b1 + a1 b2 + a2 b1: every dropped term is at most 2^-16 |a b|; half the matrix
// instructions and two thirds of the split / LDS work of mode 6.  The first edition kept fp32 tiles in LDS and every wave split the fragments it read: with 2 x 2 waves
// per block each element was split twice, 352 vector instructions per wave and K step beside 48 matrix instructions - the
// vector pipe, not the matrix pipe, set the pace (PMC: matrix pipe 50 % busy, profiles/r02_gemm.md).  Here
//   * the thread that LOADS an element splits it (22 vector instructions per four elements, once) and stores the three planes
//     to LDS as bf16; fragments are read from LDS as finished MFMA operands (ds_read_b128 = 8 k of one plane);
//   * the block tile is 256 x 128 (8 waves as 4 x 2, wave tile 64 x 64 = four 32 x 32 tiles): a thread splits 24 elements per
//     K step (132 vector instructions) against 48 matrix instructions of 32 cycles - inside their shadow;
//   * LDS image per plane: [row][32 k] bf16 = 64 bytes per row, no padding; the 16-byte chunk index is XOR-ed with bits 2..3
//     of the row and rows 4..7 of every 8 swap inside their pairs, which makes the fragment reads (ds_read_b128), the
//     [rows][K] stores (ds_write_b64) and the transposed [K][rows] stores conflict-free or 2-way at worst;
//     2 stages x (3 x 16 KB + 3 x 8 KB) = 144 KB: one block of 512 threads per CU, two waves per SIMD.
// Pipeline per K step s (one barrier): MFMAs of k slab 0 | split + LDS stores of step s + 1 (its global loads were issued a step
// earlier) | fragment reads of slab 1 | global loads of step s + 2 | first half of slab 1's MFMAs | barrier | fragment reads of
// step s + 1's slab 0 under the second half of slab 1's MFMAs.
// A third edition for mode 2 (producer / consumer waves, `gemm_ws_kernel` further down) takes the shapes with whole K steps; this one keeps the rest.
// Blocks are persistent (256 = one per CU) and walk items exactly as in gemm_f32.hip: whole tiles, and K slices for the last
// partly filled round and for weight gradients, summed by a fix-up kernel in a fixed order (deterministic, no atomics): the item
// walk, the slice plan and the fix-up kernel are gemm_splitk.h, shared with gemm_f32.hip.
// SPLIT of gemm_bf3_kernel is 2, 3 or 6; gemm_ws_kernel is mode 2 only (EPI: 0 / 6 the plain epilogues, 4 / 5 the fused ones).
#include "gemm_splitk.h"
#include "gemm_call.h"

namespace {
using namespace resel;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int BM = 256, BN = 128;
constexpr int NTH = 512;
constexpr int GRID = 256;
constexpr int TILE = BM * BN;
constexpr int ROWB = 64;                         // bytes of one row of one plane: 32 k x bf16
constexpr int PLA = BM * ROWB, PLB = BN * ROWB;  // one plane of the A / B tile
constexpr int STAGE = 3 * PLA + 3 * PLB;         // 73 728 bytes

struct Params {
    const float *A, *B, *bias;
    float *C, *slab;
    int64_t lda, ldb, ldc, sA, sB, sC, sBias;
    int M, N, K;
    int act;
    int mt, nt;
    int nfull, nsplit, nsl, kslice;
    const float *amaxA, *amaxB;                  // mode 2: device scalars >= max |A|, max |B| (resel_amax); nullptr otherwise
    AmaxOut amaxC;                               // optional: publish max |C| (the values stored, after bias / activation / accumulate)
    int ntst;                                    // third edition: non-temporal C stores
    // fused epilogues of the third edition (resel_gemm_f32_dact / resel_gemm_f32_head, whole-K items only):
    //   act 4: C = product * elu'(Y) with Y the OUTPUT of the layer below (y > 0 ? 1 : y + 1); red = per-wave column sums of C
    //          [batch][2 mt][N] (the bias gradient of that layer, folded by colsum_kernel);
    //   act 5: C = a = elu(product + bias); red = per-wave row dots sum_n a[m][n] aux[z][n] over the wave's 64 columns [batch][2 nt][M]
    //          (the width-1 output layer of the critic head, folded by head_fold_kernel)
    const float* aux;
    int64_t ldaux, sAux;
    float* red;
    int redrows;                                 // act 4: partial rows per batch member in `red` (2 mt + one for the rows the host entry handles apart)
};

// byte offset of (row, 16-byte chunk c = k / 8) inside one plane
__device__ __forceinline__ int plane_off(int row, int c) {
    const int q = row >> 2;
    return ((row ^ (q & 1)) << 6) + ((c ^ (q & 3)) << 4);
}

// The third edition's image: the chunk permutation is (0, 3, 2, 1)[q & 3].  Its consumers read a 16-row tile of the 16x16x32 operand with one
// ds_read_b128 (row lane & 15, chunk lane >> 4), which the hardware serves in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...:
// rows of q = 0, 3 with chunk c and of q = 1, 2 with chunk c + 1 meet in one group, and `c ^ q` puts two of them on the same 16-byte slots
// (2-way); this permutation gives the four their own.  The producers' stores keep their bank sets (a row group's chunks are permuted among
// themselves), and the period stays 16 rows.
__device__ __forceinline__ int plane_off_ws(int row, int c) {
    const int q = row >> 2;
    return ((row ^ (q & 1)) << 6) + ((c ^ (-q & 3)) << 4);
}

// ---- four fp32 values -> three planes of four bf16 (8 bytes each).  NP = 2 (mode 3): the second plane is the residual ROUNDED to
// nearest even (v_cvt_pk_bf16_f32) instead of truncated - the dropped part is then unbiased and at most 2^-17 |x|
__device__ __forceinline__ uint32_t rne_pair(float lo, float hi) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
struct P3 { uint2 p1, p2, p3; };
template <int NP>
__device__ __forceinline__ P3 split4(const float4& v) {
#ifdef BF3_AB_NOSPLIT                  // ablation (wrong results): no vector work for the split
    return P3{make_uint2(__float_as_uint(v.x), __float_as_uint(v.y)), make_uint2(__float_as_uint(v.z), __float_as_uint(v.w)),
              make_uint2(__float_as_uint(v.x), __float_as_uint(v.w))};
#endif
    const float x[4] = {v.x, v.y, v.z, v.w};
    uint32_t w1[2], w2[2], w3[2] = {0u, 0u};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint32_t u0 = __float_as_uint(x[2 * q]), u1 = __float_as_uint(x[2 * q + 1]);
        w1[q] = __builtin_amdgcn_perm(u1, u0, 0x07060302u);        // {hi16(x[2q+1]), hi16(x[2q])}: element 2q in the low half
        const float r0 = x[2 * q] - __uint_as_float(u0 & 0xffff0000u), r1 = x[2 * q + 1] - __uint_as_float(u1 & 0xffff0000u);
        if (NP == 2) {
            w2[q] = rne_pair(r0, r1);
        } else {
            const uint32_t v0 = __float_as_uint(r0), v1 = __float_as_uint(r1);
            w2[q] = __builtin_amdgcn_perm(v1, v0, 0x07060302u);
            const float s0 = r0 - __uint_as_float(v0 & 0xffff0000u), s1 = r1 - __uint_as_float(v1 & 0xffff0000u);
            w3[q] = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
        }
    }
    return P3{make_uint2(w1[0], w1[1]), make_uint2(w2[0], w2[1]), make_uint2(w3[0], w3[1])};
}
struct P3h { uint32_t p1, p2, p3; };                 // two values -> three planes of two bf16
template <int NP>
__device__ __forceinline__ P3h split2(float x0, float x1) {
    const uint32_t u0 = __float_as_uint(x0), u1 = __float_as_uint(x1);
    P3h o;
    o.p1 = __builtin_amdgcn_perm(u1, u0, 0x07060302u);
    const float r0 = x0 - __uint_as_float(u0 & 0xffff0000u), r1 = x1 - __uint_as_float(u1 & 0xffff0000u);
    if (NP == 2) {
        o.p2 = rne_pair(r0, r1);
        o.p3 = 0u;
        return o;
    }
    const uint32_t v0 = __float_as_uint(r0), v1 = __float_as_uint(r1);
    o.p2 = __builtin_amdgcn_perm(v1, v0, 0x07060302u);
    const float s0 = r0 - __uint_as_float(v0 & 0xffff0000u), s1 = r1 - __uint_as_float(v1 & 0xffff0000u);
    o.p3 = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
    return o;
}

// ---- mode 2 ("f16x3"): fp16 planes of the SCALED operands, three plane products, one accumulator.  Each operand is multiplied by
// a power of two s that brings its largest magnitude into [2^14, 2^15) (resel_amax; exact), then
//   A (the wide-range operand: activations, gradients):  a1 = fp16(x s),  a2 = fp16(2^11 (x s - a1))        - two planes;
//   B (weights; the second operand of a weight gradient): b1 = fp16(x s),  b2 = fp16(x s - b1),  b1s = 2^-11 b1 - three planes;
//   C = (a1 b1 + a1 b2 + a2 b1s) / (sA sB):  the residuals are exact in fp32, every plane product is exact in fp32, the dropped
//   term a2 b2 is <= 2^-22 |a b|.  The 2^11 between the planes of one element sits on the A side for the a-residual (a2 is
//   normal down to |x| = 2^-29 max|A|) and on the B side for the b-residual (b2, b1s normal down to 2^-18 max|B|; below that
//   the element keeps 40 - d bits, d = log2(max|B| / |x|)) - a single fp16 accumulator scale cannot give both operands the
//   full range, two accumulator sets do not fit 256 registers beside the fragments (tried: 11-31 spilled dwords, slower than mode 6).
// sc = {s, 2048 s}.  7 vector instructions per element pair.
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
template <bool WIDE>
__device__ __forceinline__ void split_pair_f16(float x0, float x1, f32x2_t sc, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
#ifdef BF3_AB_NOSPLIT                  // ablation (wrong results)
    p1 = __float_as_uint(x0); p2 = __float_as_uint(x1); p3 = __float_as_uint(x0) ^ __float_as_uint(sc.x);
    return;
#endif
    const f32x2_t xs = {x0 * sc.x, x1 * sc.x};
    const f16x2_t h = __builtin_convertvector(xs, f16x2_t);
    p1 = __builtin_bit_cast(uint32_t, h);
    if (WIDE) {
        const f32x2_t r = {__builtin_fmaf((float)h.x, -2048.f, x0 * sc.y), __builtin_fmaf((float)h.y, -2048.f, x1 * sc.y)};
        p2 = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2_t));
        p3 = 0u;
    } else {
        const f32x2_t r = {xs.x - (float)h.x, xs.y - (float)h.y};
        p2 = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2_t));
        p3 = 0u;                                   // 2^-11 b1 is formed by the consumer of the fragment (mfma_lead_f16)
    }
}
template <bool WIDE>
__device__ __forceinline__ P3 split4_f16(const float4& v, f32x2_t sc) {
    P3 o;
    split_pair_f16<WIDE>(v.x, v.y, sc, o.p1.x, o.p2.x, o.p3.x);
    split_pair_f16<WIDE>(v.z, v.w, sc, o.p1.y, o.p2.y, o.p3.y);
    return o;
}
template <bool WIDE>
__device__ __forceinline__ P3h split2_f16(float x0, float x1, f32x2_t sc) {
    P3h o;
    split_pair_f16<WIDE>(x0, x1, sc, o.p1, o.p2, o.p3);
    return o;
}
// scale of an operand from its (upper bound of the) largest magnitude a: 2^(14 - floor(log2 a)), so a s is in [2^14, 2^15);
// a = 0 or tiny: a large finite scale (the operand is zero / negligible either way)
__device__ __forceinline__ float f16_scale(float amax) {
    const int f = (int)((__float_as_uint(amax) >> 23) & 0xffu);
    const int e = min(max(268 - f, 1), 240);         // 2048 s stays finite
    return __uint_as_float((uint32_t)e << 23);
}

// ---- one operand's share of a thread in a K step.
// KC (P[row][k]): NPC pieces, piece i = row (tid / 8 + 64 i), k = 4 (tid % 8) .. + 3 (one float4, 8 bytes per plane).
// !KC (P[k][row]), the 256-row operand: one 4 (k) x 4 (rows) patch, rows 4 g .., k = 4 k4 ..: four float4 along rows,
//   transposed in registers, four ds_write_b64 per plane.  tid = [g_lo:3][k4:3][g_hi:3]: a wave-load covers 8 k rows x 128 B.
// !KC, the 128-row operand: one 2 (k) x 4 (rows) patch, k = 2 k2 ..: two float4, four ds_write_b32 per plane.
//   tid = [g_lo:3][k2:4][g_hi:2].
// Rows beyond the operand's extent are read from row 0 (their products land in rows / columns that are never stored); k beyond
// the slice end contributes zeros (guarded loads on the last step of a K that is not a multiple of 32).
template <bool KC, int ROWS>
struct Src {
    static constexpr int NPC = ROWS / 64;          // KC pieces
    static constexpr bool is_kc = KC;
    static constexpr int NR = KC ? NPC : (ROWS == 256 ? 4 : 2);
    const char* base;
    const char* base0;                             // the tile's step at k = 0: always a whole, valid K step (K >= 32)
    uint32_t off[NR];
    uint32_t loff[KC ? NPC : 4];                   // LDS byte offsets inside a plane (KC: per piece; !KC: per patch row)
    int64_t step;
    int rl0, rlim, ld4, kofs4;                     // KC, third edition: this thread's row in piece 0, the last valid row of the tile (uniform),
                                                   // the row stride and this thread's k offset in bytes: offset of piece i = min(rl0 + 64 i, rlim) ld4 + kofs4
    int kofs;
    float4 r[NR];
    __device__ __forceinline__ void init(const float* P, int64_t ld, int rows, int r0, int k0, int tid) {
        if (KC) {
            kofs = 4 * (tid & 7);
            base = (const char*)(P + (int64_t)r0 * ld + k0);
            base0 = (const char*)(P + (int64_t)r0 * ld);
#pragma unroll
            for (int i = 0; i < NPC; ++i) {
                const int rl = (tid >> 3) + 64 * i;
                off[i] = (uint32_t)(((r0 + rl < rows ? rl : 0) * ld + kofs) * 4);
            }
            step = BK * 4;
            rl0 = tid >> 3;
            rlim = min(rows - 1 - r0, ROWS - 1);         // rows past the operand read its last row (their products are never stored)
            ld4 = (int)(ld * 4);
            kofs4 = kofs * 4;
        } else {
            const int g = ROWS == 256 ? (tid & 7) + 8 * (tid >> 6) : (tid & 7) + 8 * (tid >> 7);
            kofs = ROWS == 256 ? 4 * ((tid >> 3) & 7) : 2 * ((tid >> 3) & 15);
            base = (const char*)(P + (int64_t)k0 * ld + r0);
            base0 = (const char*)(P + r0);
            const int rl = 4 * g;
#pragma unroll
            for (int j = 0; j < NR; ++j) off[j] = (uint32_t)(((kofs + j) * ld + (r0 + rl < rows ? rl : 0)) * 4);
            step = (int64_t)BK * ld * 4;
        }
    }
    template <bool WS = false>                      // WS: the third edition's image (plane_off_ws)
    __device__ __forceinline__ void init_lds(int tid) {
        auto plane_off = [](int row, int c) { return WS ? plane_off_ws(row, c) : ::plane_off(row, c); };
        if (KC) {
#pragma unroll
            for (int i = 0; i < NPC; ++i) loff[i] = plane_off((tid >> 3) + 64 * i, (tid & 7) >> 1) + 8 * (tid & 1);
        } else if (ROWS == 256) {
            const int g = (tid & 7) + 8 * (tid >> 6), k4 = (tid >> 3) & 7;
#pragma unroll
            for (int j = 0; j < 4; ++j) loff[j] = plane_off(4 * g + j, k4 >> 1) + 8 * (k4 & 1);
        } else {
            const int g = (tid & 7) + 8 * (tid >> 7), k2 = (tid >> 3) & 15;
#pragma unroll
            for (int j = 0; j < 4; ++j) loff[j] = plane_off(4 * g + j, k2 >> 2) + 4 * (k2 & 3);
        }
    }
    // branch-free form for the scheduled region of the K loop: `full` (uniform) = a whole K step is due - load it and advance;
    // otherwise the same instructions re-read the tile's step at k = 0 (in bounds) and the caller's guarded `load` follows
    __device__ __forceinline__ void load_sched(bool full) {
#ifdef BF3_AB_NOLOAD                   // ablation (wrong results): the staging registers are never refreshed
        asm volatile("" : "+v"(r[0].x));
        return;
#endif
        const char* b = full ? base : base0;
#pragma unroll
        for (int i = 0; i < NR; ++i) r[i] = *reinterpret_cast<const float4*>(b + off[i]);
        if (full) base += step;
    }
    __device__ __forceinline__ void load(int k0, int kend) { load_to(r, k0, kend); }
    __device__ __forceinline__ void load_to(float4 (&r)[NR], int k0, int kend) {
#ifdef BF3_AB_NOLOAD
        asm volatile("" : "+v"(r[0].x));
        return;
#endif
        if (k0 + BK <= kend) {
#pragma unroll
            for (int i = 0; i < NR; ++i) r[i] = *reinterpret_cast<const float4*>(base + off[i]);
        } else {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                r[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k0 + kofs + (KC ? 0 : i) < kend) r[i] = *reinterpret_cast<const float4*>(base + off[i]);
            }
        }
        base += step;
    }
    // third edition (producer waves): one piece of a register set at a time, so that a register is reloaded for two K steps ahead
    // as soon as its values have been split (KC layouts; the transposed layouts need all NR registers of a patch together)
    __device__ __forceinline__ void load_piece(float4& v, int i, int k0, int kend) const {
#ifdef BF3_AB_NOLOAD
        asm volatile("" : "+v"(v.x));
        return;
#endif
        if (k0 + BK <= kend) {
            v = *reinterpret_cast<const float4*>(base + off[i]);
        } else {
            v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + kofs + (KC ? 0 : i) < kend) v = *reinterpret_cast<const float4*>(base + off[i]);
        }
    }
    __device__ __forceinline__ void advance() { base += step; }
    __device__ __forceinline__ uint32_t piece_off(int i) const {        // two vector instructions per piece instead of a register per piece
        return __umul24((uint32_t)min(rl0 + 64 * i, rlim), (uint32_t)ld4) + (uint32_t)kofs4;
    }
    template <int PL, int NP, int F16>
    __device__ __forceinline__ void store_piece(const float4& v, int i, char* pl, f32x2_t sc) const {
        static_assert(KC, "pieces exist in the [rows][K] layout only");
        const P3 s = F16 == 1 ? split4_f16<true>(v, sc) : F16 == 2 ? split4_f16<false>(v, sc) : split4<NP>(v);
        *reinterpret_cast<uint2*>(pl + loff[i]) = s.p1;
        *reinterpret_cast<uint2*>(pl + PL + loff[i]) = s.p2;
        if (NP == 3) *reinterpret_cast<uint2*>(pl + 2 * PL + loff[i]) = s.p3;
    }
    // split the staged values and store the planes of this thread's pieces into the plane set at `pl` (plane stride PL bytes)
    template <int PL, int NP, int F16 = 0>
    __device__ __forceinline__ void store(char* pl, f32x2_t sc = f32x2_t{1.f, 2048.f}) const { store_from<PL, NP, F16>(r, pl, sc); }
    template <int PL, int NP, int F16 = 0>
    __device__ __forceinline__ void store_from(const float4 (&r)[NR], char* pl, f32x2_t sc = f32x2_t{1.f, 2048.f}) const {
        if (KC) {
#pragma unroll
            for (int i = 0; i < NPC; ++i) {
                const P3 s = F16 == 1 ? split4_f16<true>(r[i], sc) : F16 == 2 ? split4_f16<false>(r[i], sc) : split4<NP>(r[i]);
                *reinterpret_cast<uint2*>(pl + loff[i]) = s.p1;
                *reinterpret_cast<uint2*>(pl + PL + loff[i]) = s.p2;
                if (NP == 3) *reinterpret_cast<uint2*>(pl + 2 * PL + loff[i]) = s.p3;
            }
        } else if (ROWS == 256) {
            const float c[4][4] = {{r[0].x, r[1].x, r[2].x, r[3].x}, {r[0].y, r[1].y, r[2].y, r[3].y},
                                   {r[0].z, r[1].z, r[2].z, r[3].z}, {r[0].w, r[1].w, r[2].w, r[3].w}};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 cj = make_float4(c[j][0], c[j][1], c[j][2], c[j][3]);
                const P3 s = F16 == 1 ? split4_f16<true>(cj, sc) : F16 == 2 ? split4_f16<false>(cj, sc) : split4<NP>(cj);
                *reinterpret_cast<uint2*>(pl + loff[j]) = s.p1;
                *reinterpret_cast<uint2*>(pl + PL + loff[j]) = s.p2;
                if (NP == 3) *reinterpret_cast<uint2*>(pl + 2 * PL + loff[j]) = s.p3;
            }
        } else {
            const float c[4][2] = {{r[0].x, r[1].x}, {r[0].y, r[1].y}, {r[0].z, r[1].z}, {r[0].w, r[1].w}};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const P3h s = F16 == 1 ? split2_f16<true>(c[j][0], c[j][1], sc) : F16 == 2 ? split2_f16<false>(c[j][0], c[j][1], sc) : split2<NP>(c[j][0], c[j][1]);
                *reinterpret_cast<uint32_t*>(pl + loff[j]) = s.p1;
                *reinterpret_cast<uint32_t*>(pl + PL + loff[j]) = s.p2;
                if (NP == 3) *reinterpret_cast<uint32_t*>(pl + 2 * PL + loff[j]) = s.p3;
            }
        }
    }
};

struct Frag { bf16x8 a[3][2], b[3][2]; };            // [plane][32-row tile] of one k slab (16 k)

__device__ __forceinline__ bf16x8 lds16(const char* p) { return *reinterpret_cast<const bf16x8*>(p); }
// fa / fb: this lane's fragment address of slab `s` in plane 0, tile 0 of the stage (byte pointers into LDS)
template <int NP>
__device__ __forceinline__ void read_a(Frag& f, const char* fa) {
#pragma unroll
    for (int pi = 0; pi < NP; ++pi)
#pragma unroll
        for (int t = 0; t < 2; ++t) f.a[pi][t] = lds16(fa + pi * PLA + t * 32 * ROWB);
}
template <int NP>
__device__ __forceinline__ void read_b(Frag& f, const char* fb) {
#pragma unroll
    for (int pi = 0; pi < NP; ++pi)
#pragma unroll
        for (int t = 0; t < 2; ++t) f.b[pi][t] = lds16(fb + pi * PLB + t * 32 * ROWB);
}
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <int P, int Q>
__device__ __forceinline__ void mfma_term_f16(f32x16 (&acc)[2][2], const Frag& f) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#ifdef BF3_AB_NOMFMA
            asm volatile("" :: "v"(f.a[P][a]), "v"(f.b[Q][b]));
#else
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, f.a[P][a]), __builtin_bit_cast(f16x8, f.b[Q][b]), acc[a][b], 0, 0, 0);
#endif
        }
}
template <int P, int Q>
__device__ __forceinline__ void mfma_term(f32x16 (&acc)[2][2], const Frag& f) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#ifdef BF3_AB_NOMFMA                   // ablation (wrong results): operands consumed, no matrix instruction
            asm volatile("" :: "v"(f.a[P][a]), "v"(f.b[Q][b]));
#elif defined(BF3_AB_M16)              // ablation (wrong results): the same matrix-pipe time as TWO v_mfma_f32_16x16x32_bf16 on accumulator quarters
            {
                typedef float f32x4v __attribute__((ext_vector_type(4)));
                constexpr int h = ((P + Q) & 1) * 2;
                f32x4v q0 = __builtin_shufflevector(acc[a][b], acc[a][b], 4 * h, 4 * h + 1, 4 * h + 2, 4 * h + 3);
                f32x4v q1 = __builtin_shufflevector(acc[a][b], acc[a][b], 4 * h + 4, 4 * h + 5, 4 * h + 6, 4 * h + 7);
                q0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[P][a], f.b[Q][b], q0, 0, 0, 0);
                q1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[P][a], f.b[Q][b], q1, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc[a][b][4 * h + e] = q0[e]; acc[a][b][4 * h + 4 + e] = q1[e]; }
            }
#else
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[P][a], f.b[Q][b], acc[a][b], 0, 0, 0);
#endif
        }
}
// the small terms are added first
template <int SPLIT>
__device__ __forceinline__ void mfma_small(f32x16 (&acc)[2][2], const Frag& f) {
    if (SPLIT == 3 || SPLIT == 2) return;           // two planes per operand: a1 b1 + a1 b2 + a2 b1 only (mfma_lead)
    mfma_term<2, 0>(acc, f); mfma_term<0, 2>(acc, f); mfma_term<1, 1>(acc, f);
}
__device__ __forceinline__ void mfma_lead(f32x16 (&acc)[2][2], const Frag& f) {
    mfma_term<1, 0>(acc, f); mfma_term<0, 1>(acc, f); mfma_term<0, 0>(acc, f);
}
// mode 2: a2 b1s + a1 b2 + a1 b1 (A planes {a1, a2}, B planes {b1, b2, b1s}), small terms first
// the third B "plane" 2^-11 b1 never goes through LDS: four packed fp16 multiplies per fragment (exact unless the product is subnormal -
// the same values the producer's packed multiply stored before), a fifth less fragment traffic and a plane less to store
__device__ __forceinline__ void mfma_lead_f16(f32x16 (&acc)[2][2], Frag& f) {
    const f16x8 k = {(_Float16)0.00048828125f, (_Float16)0.00048828125f, (_Float16)0.00048828125f, (_Float16)0.00048828125f,
                     (_Float16)0.00048828125f, (_Float16)0.00048828125f, (_Float16)0.00048828125f, (_Float16)0.00048828125f};
#pragma unroll
    for (int t = 0; t < 2; ++t) f.b[2][t] = __builtin_bit_cast(bf16x8, __builtin_bit_cast(f16x8, f.b[0][t]) * k);
    mfma_term_f16<1, 2>(acc, f); mfma_term_f16<0, 1>(acc, f); mfma_term_f16<0, 0>(acc, f);
}

#define BF3_FENCE() __builtin_amdgcn_sched_barrier(0)
#ifdef BF3_AB_CLOCK                    // diagnostic build: in-kernel clock = d(s_memtime) / d(s_memrealtime) x 100 MHz per block
__device__ unsigned long long g_bf3_clock[2 * GRID];
#endif

template <bool AKC, bool BKC, int SPLIT>
__global__ __launch_bounds__(NTH, 2) void gemm_bf3_kernel(Params p) {
    extern __shared__ __attribute__((aligned(16))) char lds[];           // 2 stages
    constexpr bool F16 = SPLIT == 2;                                     // fp16 planes of the scaled operands (f16x3)
    constexpr int NP = (SPLIT == 3 || SPLIT == 2) ? 2 : 3;               // planes per element of A
    constexpr int NPB = (SPLIT == 3 || SPLIT == 2) ? 2 : 3;              // planes of B in LDS (mode 2: b1, b2; 2^-11 b1 is formed from b1's fragment)
    f32x2_t scA = {1.f, 2048.f}, scB = {1.f, 2048.f};
    float unscale = 1.f;
    if (F16) {
        const float sa_ = f16_scale(amax_read(p.amaxA)), sb_ = f16_scale(amax_read(p.amaxB));
        scA = f32x2_t{sa_, 2048.f * sa_};
        scB = f32x2_t{sb_, 2048.f * sb_};
        unscale = (1.f / sa_) * (1.f / sb_);                             // powers of two: exact
    }
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = (w >> 1) * 64, wn = (w & 1) * 64;
    const int li = lane & 31, lh = lane >> 5;
    const int total = p.nfull + p.nsplit * p.nsl;
    const int G = gridDim.x;
    if ((int)blockIdx.x >= total) return;

    Src<AKC, BM> sa;
    Src<BKC, BN> sb;
    sa.init_lds(tid);
    sb.init_lds(tid);
    int p_item = blockIdx.x, p_k0, p_kend;
    bool p_live = true;
    auto p_open = [&]() {
        const Item it = decode<BM, BN>(p, p_item);
        sa.init(p.A + (int64_t)it.z * p.sA, p.lda, p.M, it.m0, it.kbeg, tid);
        sb.init(p.B + (int64_t)it.z * p.sB, p.ldb, p.N, it.n0, it.kbeg, tid);
        p_k0 = it.kbeg; p_kend = it.kend;
    };
    auto produce = [&]() {                          // global loads of the next K step in program order (also across items)
        if (!p_live) return;
        sa.load(p_k0, p_kend);
        sb.load(p_k0, p_kend);
        p_k0 += BK;
        if (p_k0 >= p_kend) {
            p_item += G;
            if (p_item < total) p_open(); else p_live = false;
        }
    };
    auto stage_store = [&](int st) {
        sa.template store<PLA, NP, F16 ? 1 : 0>(lds + st * STAGE, scA);
        sb.template store<PLB, NPB, F16 ? 2 : 0>(lds + st * STAGE + 3 * PLA, scB);
    };
    // fragment addresses: slab s of the lane = chunk 2 s + lh of row li of the wave's tile rows
    const char* fa[2];
    const char* fb[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        fa[s] = lds + wm * ROWB + plane_off(li, 2 * s + lh);
        fb[s] = lds + 3 * PLA + wn * ROWB + plane_off(li, 2 * s + lh);
    }

#ifdef BF3_AB_STAGGER                     // experiment: BF3_AB_STAGGER groups of CUs start a fraction of a tile time apart (write bursts desynchronised)
    {
        const int grp = ((int)blockIdx.x >> 3) % BF3_AB_STAGGER;
        const long long wait = (long long)((p.K + BK - 1) / BK) * 5300 * grp / BF3_AB_STAGGER;
        const long long t0 = __builtin_amdgcn_s_memtime();
        while ((long long)__builtin_amdgcn_s_memtime() - t0 < wait) __builtin_amdgcn_s_sleep(32);
    }
#endif
#ifdef BF3_AB_CLOCK
    const unsigned long long ck_t0 = __builtin_amdgcn_s_memtime(), ck_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    float cmax = 0.f;                               // max |C| over everything this lane stores (published once, at the end)
    Frag f0, f1;
    p_open();
    produce();
    stage_store(0);
    produce();
    __syncthreads();
    read_a<NP>(f0, fa[0]); read_b<NPB>(f0, fb[0]);
    int cur_st = 0;
    for (int c_item = blockIdx.x; c_item < total; c_item += G) {
        const Item cur = decode<BM, BN>(p, c_item);
        float zero = 0.f;
        asm volatile("" : "+v"(zero));              // opaque: or 64 registers of hoisted zeros stay live across the K loop
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = zero;
        float bv[2] = {0.f, 0.f};

        for (int c_k0 = cur.kbeg; c_k0 < cur.kend; c_k0 += BK) {
            const int so = cur_st * STAGE, sn = (cur_st ^ 1) * STAGE;
            const bool fast = p_live && p_k0 + BK <= p_kend;
            if (c_k0 + BK >= cur.kend && p.bias && !cur.split) {        // requested most of a step before the epilogue needs them
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int n = cur.n0 + wn + 32 * b + li;
                    bv[b] = p.bias[(int64_t)cur.z * p.sBias + (n < p.N ? n : 0)];
                }
            }
            BF3_FENCE();
            // ---- region A: 36 matrix instructions (two-plane modes: 12); in their shadow slab 1's fragment reads, the split + LDS stores of step
            // s + 1's tile and the global loads of step s + 2 into the registers the split has just released
            read_a<NP>(f1, fa[1] + so); read_b<NPB>(f1, fb[1] + so);
            mfma_small<SPLIT>(acc, f0);
            stage_store(cur_st ^ 1);
            if (F16) mfma_lead_f16(acc, f0); else mfma_lead(acc, f0);
            sa.load_sched(fast);
            sb.load_sched(fast);
            mfma_small<SPLIT>(acc, f1);
            if (SPLIT == 3 || SPLIT == 2) {         // 12 matrix instructions carry 8 (10) fragment reads, the split, 12 (14) LDS writes, the loads
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (i < 2 * (NP + NPB)) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                    if (i >= 4) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 36; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                 // one MFMA
                    if (i < 12) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // one LDS read
                    __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);     // vector instructions
                    if (i >= 4 && i < 4 + 18) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // one LDS write
                    if (i >= 36 - 8) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);           // one global load
                }
            }
            BF3_FENCE();
#ifdef BF3_AB_NOBAR                    // ablation (wrong results)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // stage s + 1 is complete; every wave has read stage s
#endif
            BF3_FENCE();
            // ---- region B: the leading terms of slab 1 with the fragment reads of step s + 1's slab 0
            read_a<NP>(f0, fa[0] + sn); read_b<NPB>(f0, fb[0] + sn);
            if (F16) mfma_lead_f16(acc, f1); else mfma_lead(acc, f1);
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (i < 2 * (NP + NPB)) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            BF3_FENCE();
            if (fast) {
                p_k0 += BK;
                if (p_k0 >= p_kend) {
                    p_item += G;
                    if (p_item < total) p_open(); else p_live = false;
                }
            } else {
                produce();
            }
            BF3_FENCE();
            cur_st ^= 1;
        }
        if (F16) {                                   // C = (a1 b1 + a1 b2 + a2 b1s) / (sA sB): powers of two, exact
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[a][b][e] *= unscale;
        }
#ifdef BF3_AB_NOEPI                    // ablation (wrong results): one store per wave and tile keeps the accumulators alive
        if (lane == 0) p.C[(int64_t)cur.m0 * p.ldc + cur.n0 + w] = acc[0][0][0] + acc[0][1][1] + acc[1][0][2] + acc[1][1][3];
        continue;
#endif
        // epilogue: D layout col = lane & 31 (n), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (m).  One dword per lane and store:
        // 32 consecutive n of one row = a full 128-byte line (x 2 rows per instruction).  The transposed form (B fragment as the
        // first MFMA operand: four consecutive n per lane, 16 float4 stores instead of 64 dword stores) was measured SLOWER
        // (583 -> 618 us at 66 752 x 2048 x 384): a store costs per line touched (32 rows x 32 bytes per instruction there).
        if (cur.split) {
            slab_store<BN>(p.slab + (int64_t)(cur.split - 1) * TILE + (wm + 4 * lh) * BN + wn + li, acc);
        } else {
            float* C = p.C + (int64_t)cur.z * p.sC;
            const bool full_m = cur.m0 + BM <= p.M;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int n = cur.n0 + wn + 32 * b + li;
                if (n >= p.N) continue;
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    float v[16];
#pragma unroll
                    for (int e = 0; e < 16; ++e) v[e] = acc[a][b][e] + bv[b];
                    if (p.act == 1) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) v[e] = elu1(v[e]);
                    }
                    if (p.act == 3) {                                // softplus (dt_proj of the Mamba mixer: the scan then reads delta itself)
#pragma unroll
                        for (int e = 0; e < 16; ++e) v[e] = softplus_nb(v[e]);
                    }
                    if (p.act >= 6) {                                // relu, leaky_relu, tanh, sigmoid (the dense stacks' other activations)
                        if (p.act == 6) {
#pragma unroll
                            for (int e = 0; e < 16; ++e) v[e] = relu_(v[e]);
                        } else if (p.act == 7) {
#pragma unroll
                            for (int e = 0; e < 16; ++e) v[e] = leaky_relu_(v[e]);
                        } else if (p.act == 8) {
#pragma unroll
                            for (int e = 0; e < 16; ++e) v[e] = tanh_(v[e]);
                        } else {
#pragma unroll
                            for (int e = 0; e < 16; ++e) v[e] = sigmoidf_(v[e]);
                        }
                    }
                    const int mb = cur.m0 + wm + 32 * a + 4 * lh;
                    float* crow = C + (int64_t)mb * p.ldc + n;
                    if (p.act == 2) {                                // C += product (the accumulating form of an input gradient)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const int dm = (e & 3) + 8 * (e >> 2);
                            if (mb + dm < p.M) v[e] += crow[(int64_t)dm * p.ldc];
                        }
                    }
                    if (full_m) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) crow[(int64_t)((e & 3) + 8 * (e >> 2)) * p.ldc] = v[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const int dm = (e & 3) + 8 * (e >> 2);
                            if (mb + dm < p.M) crow[(int64_t)dm * p.ldc] = v[e];
                        }
                    }
                    if (p.amaxC.slot) {              // rows past M repeat row 0's products: in range of the real data
#pragma unroll
                        for (int e = 0; e < 16; e += 2) cmax = fmaxf(cmax, fmaxf(__builtin_fabsf(v[e]), __builtin_fabsf(v[e + 1])));
                    }
                }
            }
        }
    }
    amax_publish_wave(cmax, p.amaxC);
#ifdef BF3_AB_CLOCK
    if (tid == 0) {
        g_bf3_clock[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - ck_t0;
        g_bf3_clock[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - ck_r0;
    }
#endif
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Third edition (mode 2, whole K steps): the same block tile, planes, LDS image and item walk, with the two jobs of a K step given to
// different waves.  In the second edition every wave loads, splits, stores planes, reads fragments, issues matrix instructions and stores
// C in program order - a wave parked on `vmcnt` issues no matrix instruction either - and its parts ADD (profiles/r04_gemm.md: data path
// 192 us + split 50 + C stores 113 + matrix instructions 158 = 513 against 455 measured at 66 752 x 2048 x 384).  Here, 512 threads:
//   * waves 0..3 (consumers, 2 x 2 over the 256 x 128 tile, wave tile 128 x 64 = 8 x 4 tiles of 16 x 16 on v_mfma_f32_16x16x32_f16, 128
//     accumulator registers) only read fragments (24 ds_read_b128 per K step: one read is a 16-row tile's whole 32-k step; B held per
//     step in one of two register sets, A tiles through a ring of two), issue matrix instructions and store C; they never wait for a
//     load.  2^-11 b1 - the third B "plane" of mode 2 - is formed from b1's fragments with sixteen packed fp16 multiplies per step (the
//     values the producer's packed multiply used to store): LDS holds two planes per operand, in this edition's own chunk
//     permutation (plane_off_ws: the 16-row reads are conflict-free);
//   * waves 4..7 (producers, one per SIMD) hold two register sets = two K steps of the fp32 tiles; ALL their tile loads are inline
//     assembly the compiler does not count, and every unit (a piece of a [rows][K] operand, an instance of a transposed one) waits for
//     ITS loads with a hand-written `s_waitcnt vmcnt(24 - n)` tied to its registers through "+v" operands (24 loads in flight, the
//     unit's n are the oldest; foreign vector-memory operations only make a wait stricter), splits, stores its planes and reloads its
//     registers for the step two further on.  Each producer thread does the work of second-edition threads t and t + 256 (same
//     addresses, same LDS image).  What hipcc does to a fine-grained load / split / store pipeline written in plain C++ - branches
//     per piece, `vmcnt(0)` after every barrier or in front of every load, whole register sets copied at loop edges (= read while
//     their loads are in flight) - is in profiles/r04_gemm.md; hence: a SCALAR role test (two separate paths to the waitcnt pass),
//     native 128-bit vectors as asm operands, ONE path through the steady-state loop, the tail behind a drain;
//   * one `s_barrier` per K step for all eight waves: stage s + 1 written, stage s read;
//   * whole C tiles leave through a wave-private 5 KB LDS scratch (the third A plane of the stages, unused in mode 2) as 16-byte
//     stores of eight whole 128-byte lines: 32 store instructions per wave and tile instead of 128 (a wave may have 63 in flight);
//     edge tiles and the accumulating form leave in the accumulator layout, as in the second edition;
//   * after the K loop a K slice goes to the slab and a whole-K item through ONE of three separate epilogues, chosen at compile time:
//     EPI 0 plain (bias, Params::act 0 .. 3), EPI 6 plain with act 6 .. 9 (relu, leaky_relu, tanh, sigmoid), EPI 4 dact (whole tiles only: the host entry refuses other shapes), EPI 5 head (bias, ELU,
//     row dots; whole and edge tiles).  Each spells out its own tile loop: see the note at EPI 0's whole-tile block.
// 256 registers, 24-32 bytes of scratch (EPI 5: 84-88, EPI 4: none), two waves per SIMD, one block per CU, persistent.  Measured against the second edition (same box,
// us): fwd [T,384] -> 256 77 -> 67, [T,256] -> 256 55 -> 48, [T,256] -> 1024 171 -> 150, [T,384] -> 2048 420 -> 365.
// The 16x16x32 consumers against the 32x32x16 ones on a box that holds the clock down: 357.8 -> 349.2 at [T,384] -> 2048, 53.1 -> 48.0 at [T,256] -> 256,
// level at K = 1024 and on fast-class boxes (profiles/r29_gemm_mfma16.md).
constexpr int NTH_WS = 512;
constexpr int WS_LDS = 2 * STAGE;
#define WS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

template <bool AKC, bool BKC, int EPI = 0>
__global__ __launch_bounds__(NTH_WS, 1) void gemm_ws_kernel(Params p) {
    static_assert(EPI == 0 || EPI == 4 || EPI == 5 || EPI == 6, "EPI: 0 plain, 6 plain with act 6 .. 9, 4 dact, 5 head (the act codes of the fused host entries)");
    extern __shared__ __attribute__((aligned(16))) char lds[];           // 2 stages
    const int tid = threadIdx.x;
    const int total = p.nfull + p.nsplit * p.nsl;
    const int G = gridDim.x;
    if ((int)blockIdx.x >= total) return;
    const float sa_ = f16_scale(amax_read(p.amaxA)), sb_ = f16_scale(amax_read(p.amaxB));
    asm volatile("" :: "v"(sa_), "v"(sb_));            // the scales have landed HERE: no compiler-counted load is pending inside the producers' loop

    if (__builtin_amdgcn_readfirstlane(tid) >= 256) {                   // a scalar condition: the two roles are separate paths to the compiler too
        // ------------------------------------------------------------------------------------------------ producers
        const int pt = tid - 256;
        const f32x2_t scA = {sa_, 2048.f * sa_}, scB = {sb_, 2048.f * sb_};
        typedef Src<AKC, BM> SA;
        typedef Src<BKC, BN> SB;
        SA a0, a1;
        SB b0, b1;
        a0.template init_lds<true>(pt); a1.template init_lds<true>(pt + 256);
        b0.template init_lds<true>(pt); b1.template init_lds<true>(pt + 256);
        // Register sets as native 128-bit values: they are operands of the inline assembly below.  ALL tile loads of this wave are inline
        // assembly the compiler does not count, and every unit (a piece of a [rows][K] operand, an instance of a transposed one) waits for
        // its own loads with a hand-written `s_waitcnt vmcnt(24 - n)` tied to its registers through "+v" operands (24 loads = two register
        // sets in flight; the n loads of the unit are the oldest), splits, stores its planes and reloads its registers for the step two
        // further on right away.  Issue order = unit order: a0, a1, b0, b1.  Whole K steps only (the host sends other shapes to edition 2).
        typedef float f32x4a __attribute__((ext_vector_type(4)));
        f32x4a ra[2][2][SA::NR], rb[2][2][SB::NR];                      // [register set][virtual thread]
        int nsteps = 0;
        for (int it = blockIdx.x; it < total; it += G) {
            const Item i = decode<BM, BN>(p, it);
            nsteps += (i.kend - i.kbeg + BK - 1) / BK;
        }
        int p_item = blockIdx.x, p_k0 = 0, p_kend = 0;
        bool p_live = true;
        auto p_open = [&]() {
            const Item it = decode<BM, BN>(p, p_item);
            const float* Ab = p.A + (int64_t)it.z * p.sA;
            const float* Bb = p.B + (int64_t)it.z * p.sB;
            a0.init(Ab, p.lda, p.M, it.m0, it.kbeg, pt); a1.init(Ab, p.lda, p.M, it.m0, it.kbeg, pt + 256);
            b0.init(Bb, p.ldb, p.N, it.n0, it.kbeg, pt); b1.init(Bb, p.ldb, p.N, it.n0, it.kbeg, pt + 256);
            p_k0 = it.kbeg; p_kend = it.kend;
        };
        auto advance = [&]() {
            a0.base += a0.step; a1.base += a1.step; b0.base += b0.step; b1.base += b1.step;
            p_k0 += BK;
            if (p_k0 >= p_kend) {
                p_item += G;
                if (p_item < total) p_open(); else p_live = false;
            }
        };
        auto aload = [&](f32x4a& r, const char* base, uint32_t off) {
#ifdef BF3_AB_NOLOAD
            asm volatile("" : "+v"(r) : "v"(off), "s"(base) : "memory");
#else
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(r) : "v"(off), "s"(base) : "memory");
#endif
        };
        auto issue_set = [&](auto SET) {                                // prologue: a whole step into set S
            constexpr int S = decltype(SET)::value;
            auto all = [&](auto& src, auto& regs) {
                typedef std::remove_reference_t<decltype(src)> ST;
#pragma unroll
                for (int i = 0; i < ST::NR; ++i) {
                    if constexpr (ST::is_kc) aload(regs[i], src.base, src.piece_off(i));
                    else aload(regs[i], src.base, src.off[i]);
                }
            };
            all(a0, ra[S][0]); all(a1, ra[S][1]); all(b0, rb[S][0]); all(b1, rb[S][1]);
            advance();
        };
        // MODE 0: steady state - two sets (24 loads) in flight, every unit waits for its own loads and reloads.  MODE 1: everything has
        // landed (tail): split and store only.  MODE 2: as 1, then reload the set and wait for it (a tail step that still has a successor).
        auto recycle = [&](auto SET, auto MODEC) {
            constexpr int S = decltype(SET)::value;
            constexpr int MODE = decltype(MODEC)::value;
            constexpr bool LOAD = MODE == 0;
            uint32_t st_off = S * STAGE;
            asm volatile("" : "+s"(st_off));               // opaque: the plane addresses are formed per piece (one add), not kept in eight registers across the loop
            char* st = lds + st_off;
            auto one = [&](auto& src, auto& regs, char* pl, f32x2_t sc, auto PLc, auto WIDEc) {      // WIDE: the A operand's planes (split_pair_f16)
                constexpr int PL = decltype(PLc)::value;
                constexpr bool WIDE = decltype(WIDEc)::value;
                typedef std::remove_reference_t<decltype(src)> ST;
                if constexpr (ST::is_kc) {
#pragma unroll
                    for (int i = 0; i < ST::NR; ++i) {
                        if (LOAD) asm volatile("s_waitcnt vmcnt(23)" : "+v"(regs[i]) :: "memory");
                        const float4 v = make_float4(regs[i].x, regs[i].y, regs[i].z, regs[i].w);
                        const P3 sp = split4_f16<WIDE>(v, sc);
                        char* d = pl + src.loff[0] + 4096 * i;
                        *reinterpret_cast<uint2*>(d) = sp.p1;
                        *reinterpret_cast<uint2*>(d + PL) = sp.p2;
                        if (MODE != 1) aload(regs[i], src.base, src.piece_off(i));
                    }
                } else {
                    float4 t[ST::NR];
                    if constexpr (ST::NR == 4) { if (LOAD) asm volatile("s_waitcnt vmcnt(20)" : "+v"(regs[0]), "+v"(regs[1]), "+v"(regs[2]), "+v"(regs[3]) :: "memory"); }
                    else { if (LOAD) asm volatile("s_waitcnt vmcnt(22)" : "+v"(regs[0]), "+v"(regs[1]) :: "memory"); }
#pragma unroll
                    for (int i = 0; i < ST::NR; ++i) t[i] = make_float4(regs[i].x, regs[i].y, regs[i].z, regs[i].w);
                    src.template store_from<PL, 2, WIDE ? 1 : 2>(t, pl, sc);
                    if (MODE != 1) {
#pragma unroll
                        for (int i = 0; i < ST::NR; ++i) aload(regs[i], src.base, src.off[i]);
                    }
                }
            };
            using IA = std::integral_constant<int, PLA>;
            using IB = std::integral_constant<int, PLB>;
            one(a0, ra[S][0], st, scA, IA{}, std::true_type{});
            one(a1, ra[S][1], st, scA, IA{}, std::true_type{});
            one(b0, rb[S][0], st + 3 * PLA, scB, IB{}, std::false_type{});
            one(b1, rb[S][1], st + 3 * PLA, scB, IB{}, std::false_type{});
            if (MODE != 1) advance();
        };
        auto landed = [&]() {                            // every load issued so far has landed, in every register of both sets
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int v = 0; v < 2; ++v) {
#pragma unroll
                    for (int i = 0; i < SA::NR; ++i) asm volatile("s_waitcnt vmcnt(0)" : "+v"(ra[q][v][i]) :: "memory");
#pragma unroll
                    for (int i = 0; i < SB::NR; ++i) asm volatile("s_waitcnt vmcnt(0)" : "+v"(rb[q][v][i]) :: "memory");
                }
        };
        using S0 = std::integral_constant<int, 0>;
        using S1 = std::integral_constant<int, 1>;
        using M0 = std::integral_constant<int, 0>;
        using M1 = std::integral_constant<int, 1>;
        using M2 = std::integral_constant<int, 2>;
        p_open();
        issue_set(S0{});                                // step 0
        if (nsteps > 1) issue_set(S1{});                // step 1
        int j = 0;
        // ONE path through the steady state (pairs of steps that both reload): the loop-carried registers keep their places - with
        // the tail's variants inside this loop hipcc copied whole register sets at the loop edges, i.e. read registers still in flight
        for (; j + 3 < nsteps; j += 2) {                // step j -> stage j & 1 from set j & 1, one K step ahead of the consumers
            recycle(S0{}, M0{});
            WS_BARRIER();
            recycle(S1{}, M0{});
            WS_BARRIER();
        }
        landed();
        for (; j < nsteps; ++j) {                       // at most three steps: synchronous
            const bool more = j + 2 < nsteps;
            if (j & 1) { if (more) recycle(S1{}, M2{}); else recycle(S1{}, M1{}); }
            else { if (more) recycle(S0{}, M2{}); else recycle(S0{}, M1{}); }
            if (more) landed();
            WS_BARRIER();
        }
        WS_BARRIER();
        return;
    }

    // ---------------------------------------------------------------------------------------------------- consumers
    // wave w: rows 128 (w >> 1) .. + 127, columns 64 (w & 1) .. + 63 of the 256 x 128 block tile = 8 x 4 tiles of 16 x 16 (v_mfma_f32_16x16x32_f16),
    // 128 accumulator registers: acc[i][j][r] is row 16 i + 4 (lane >> 4) + r, column 16 j + (lane & 15) of the wave tile.  An operand
    // fragment of a 16-row tile is ONE ds_read_b128 at chunk lane >> 4 of row lane & 15: the whole 32-k step (plane_off has a period of 16
    // rows, so tile t sits 16 t rows on).  Held per K step: B, 4 tiles x 2 planes (two sets: the next step's is read under this step's last
    // products), 2^-11 b1 (16 registers), and the A tiles streaming through a ring of two (2 planes x 4 registers each): 24 reads per step.
#ifdef BF3_AB_CLOCK
    const unsigned long long ck_t0 = __builtin_amdgcn_s_memtime(), ck_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    const float unscale = (1.f / sa_) * (1.f / sb_);
    const int lane = tid & 63, w = tid >> 6;
    const int wm = (w >> 1) * 128, wn = (w & 1) * 64;
    const int l15 = lane & 15, l4 = lane >> 4;
    const char* fa = lds + wm * ROWB + plane_off_ws(l15, l4);
    const char* fb = lds + 3 * PLA + wn * ROWB + plane_off_ws(l15, l4);
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    struct BF { f16x8 p[2][4]; };
    f16x8 ar[2][2];                                  // the A ring: [slot][plane]
    f32x4v acc[8][4];
    // the lane's 16 values of the 32 x 32 region (a, b) = a 2 x 2 group of accumulators, e = 8 ii + 4 jj + r: the exits walk these regions
#define WS_ACC(a, b, e) acc[2 * (a) + ((e) >> 3)][2 * (b) + (((e) >> 2) & 1)][(e) & 3]
#define WS_DROW(e) (16 * ((e) >> 3) + ((e) & 3))      /* row inside the region, less 4 (lane >> 4) */
#define WS_DCOL(e) (16 * (((e) >> 2) & 1))            /* column inside the region, less lane & 15 */
#define WS_BV(b, e) bv[2 * (b) + (((e) >> 2) & 1)]
    auto rdB = [&](BF& f, const char* pb) {
#pragma unroll
        for (int pi = 0; pi < 2; ++pi)
#pragma unroll
            for (int t = 0; t < 4; ++t) f.p[pi][t] = *reinterpret_cast<const f16x8*>(pb + pi * PLB + t * 16 * ROWB);
    };
    // one K step: a2 (2^-11 b1) + a1 b2 + a1 b1 per A tile, the small terms first, four independent accumulators between two products of
    // one.  Behind tile i's products the ring slot takes tile i + 2; behind tile 5's the stage has been read to the end, so the step's
    // barrier stands behind tile 6's products and the next stage's B set and first A tiles are read under tile 7's.
    auto step = [&](const BF& bc, BF& bn, const char* pa, const char* pan, const char* pbn, bool next) {
        const f16x8 k = {(_Float16)0.00048828125f, (_Float16)0.00048828125f, (_Float16)0.00048828125f, (_Float16)0.00048828125f,
                         (_Float16)0.00048828125f, (_Float16)0.00048828125f, (_Float16)0.00048828125f, (_Float16)0.00048828125f};
        f16x8 bs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bs[j] = bc.p[0][j] * k;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f16x8 a1 = ar[i & 1][0], a2 = ar[i & 1][1];
#ifdef BF3_AB_NOMFMA
            asm volatile("" :: "v"(a1), "v"(a2), "v"(bs[0]), "v"(bs[1]), "v"(bs[2]), "v"(bs[3]));
            asm volatile("" :: "v"(bc.p[0][0]), "v"(bc.p[0][1]), "v"(bc.p[0][2]), "v"(bc.p[0][3]), "v"(bc.p[1][0]), "v"(bc.p[1][1]), "v"(bc.p[1][2]), "v"(bc.p[1][3]));
#else
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, bs[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bc.p[1][j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bc.p[0][j], acc[i][j], 0, 0, 0);
#endif
            BF3_FENCE();
            if (i < 6) {
#pragma unroll
                for (int pi = 0; pi < 2; ++pi) ar[i & 1][pi] = *reinterpret_cast<const f16x8*>(pa + pi * PLA + (i + 2) * 16 * ROWB);
            } else if (i == 6) {
                WS_BARRIER();
                if (next) {
                    rdB(bn, pbn);
#pragma unroll
                    for (int pi = 0; pi < 2; ++pi) ar[0][pi] = *reinterpret_cast<const f16x8*>(pan + pi * PLA);
                }
            } else if (next) {
#pragma unroll
                for (int pi = 0; pi < 2; ++pi) ar[1][pi] = *reinterpret_cast<const f16x8*>(pan + pi * PLA + 16 * ROWB);
            }
            BF3_FENCE();
        }
    };
    // the first fragments of an item: its first stage's B set and A tiles 0 and 1
    auto rd_first = [&](BF& f, int so) {
        rdB(f, fb + so);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) ar[t][pi] = *reinterpret_cast<const f16x8*>(fa + so + pi * PLA + t * 16 * ROWB);
    };
    float cmax = 0.f;
    BF b0, b1;
    // EPI 4 keeps four tiles of Y in flight through its epilogue (64 registers): the first fragments of an item are then read at its start,
    // behind the epilogue of the one before, instead of under that item's last matrix instructions (their stage stays valid until this
    // wave passes the next barrier), and no fragment register is live across the epilogue
    constexpr bool DEFER_F0 = EPI == 4;
    WS_BARRIER();
    if (!DEFER_F0) rd_first(b0, 0);
    int cur_st = 0;
    for (int c_item = blockIdx.x; c_item < total; c_item += G) {
        const Item cur = decode<BM, BN>(p, c_item);
        if (DEFER_F0) rd_first(b0, cur_st * STAGE);
        float zero = 0.f;
        asm volatile("" : "+v"(zero));
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = zero;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        int c_k0 = cur.kbeg;
        auto one = [&](const BF& bc, BF& bn) {           // the B sets alternate from step to step
            const bool last = c_k0 + BK >= cur.kend;
            if (last && p.bias && !cur.split) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = cur.n0 + wn + 16 * j + l15;
                    bv[j] = p.bias[(int64_t)cur.z * p.sBias + (n < p.N ? n : 0)];
                }
            }
            const int so = cur_st * STAGE, sn = (cur_st ^ 1) * STAGE;
            BF3_FENCE();
            step(bc, bn, fa + so, fa + sn, fb + sn, !(DEFER_F0 && last));
            cur_st ^= 1;
            c_k0 += BK;
        };
        while (c_k0 + BK < cur.kend) { one(b0, b1); one(b1, b0); }
        if (c_k0 < cur.kend) {                           // an odd number of steps: the next item starts from set 0 again
            one(b0, b1);
            if (!DEFER_F0) b0 = b1;
        }
#ifdef BF3_AB_NOEPI
        if (lane == 0) p.C[(int64_t)cur.m0 * p.ldc + cur.n0 + w] = acc[0][0][0] + acc[3][1][1] + acc[4][2][2] + acc[7][3][3];
        continue;
#endif
        // every item: undo the operand scales (powers of two, exact).  A K slice then leaves for the slab; a whole-K item leaves through ONE
        // of three epilogues - plain (EPI 0), dact (EPI 4), head (EPI 5) - each ending the item
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] *= unscale;
        if (cur.split) {                                             // slab_store's twin (gemm_splitk.h): through the helper every EPI 0 instantiation changed
            float* o = p.slab + (int64_t)(cur.split - 1) * TILE + (wm + 4 * l4) * BN + wn + l15;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int e = 0; e < 16; ++e) o[(32 * a + WS_DROW(e)) * BN + 32 * b + WS_DCOL(e)] = WS_ACC(a, b, e);
            continue;
        }
        if constexpr (EPI == 0 || EPI == 6) {
            // ---- plain: bias, p.act (ELU / accumulate / softplus), exactly as before the fused forms existed.  EPI 6 is the same epilogue for
            // act 6 .. 9 (relu, leaky_relu, tanh, sigmoid): spelled as run-time branches next to act 1 / 3, even relu alone took the scratch of
            // every EPI 0 instantiation from 24-32 to 72-76 bytes (profiles/r30_dense_activations.md); compiled apart, EPI 0 is untouched.
            float* C = p.C + (int64_t)cur.z * p.sC;
            const bool full_m = cur.m0 + BM <= p.M;
            if (full_m && cur.n0 + BN <= p.N && p.act != 2) {
                // whole tiles: every 32 x 32 region (a 2 x 2 group of accumulators) is turned through a wave-private 5 KB LDS scratch (rows of 40
                // words; the two 16-lane row groups of a half-wave's dword write are 160 words apart: 2-way, 4 M of 53 M LDS cycles per launch
                // at 66 752 x 2048 x 384, profiles/r29_gemm_mfma16.md) and leaves as FOUR 16-byte-per-lane stores of eight whole 128-byte lines each - 32 store
                // instructions per wave and tile instead of 128: a wave may have 63 vector-memory operations in flight, and with four
                // consumer waves 128 dword stores each stalled on that limit (160 of 415 us at 66 752 x 2048 x 384).
                // Scratch: the third A plane of the stages, which mode 2 does not use (waves 0, 1 in stage 0's, 2, 3 in stage 1's).
                // Kept apart from head's whole-tile block (row tiles outermost there): through one shared loop every plain instantiation
                // changed and its scratch grew from 24 to 92 - 96 bytes.  The same holds for helper functions (profiles/r13_gemm_epilogues.md).
                char* sc = lds + (w >> 1) * STAGE + 2 * PLA + (w & 1) * 5120;
                float* wr = reinterpret_cast<float*>(sc) + (4 * l4) * 40 + l15;
                const float4* rdp = reinterpret_cast<const float4*>(sc + (lane >> 3) * 160 + (lane & 7) * 16);
#pragma unroll
                for (int b = 0; b < 2; ++b) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        float v[16];
#pragma unroll
                        for (int e = 0; e < 16; ++e) v[e] = WS_ACC(a, b, e) + WS_BV(b, e);
                        if (p.act == 1) {
#pragma unroll
                            for (int e = 0; e < 16; ++e) v[e] = elu1(v[e]);
                        }
                        if (p.act == 3) {
#pragma unroll
                            for (int e = 0; e < 16; ++e) v[e] = softplus_nb(v[e]);
                        }
                        if constexpr (EPI == 6) {                       // relu, leaky_relu, tanh, sigmoid: an instantiation of their own (note above)
                            if (p.act == 6) {
#pragma unroll
                                for (int e = 0; e < 16; ++e) v[e] = relu_(v[e]);
                            } else if (p.act == 7) {
#pragma unroll
                                for (int e = 0; e < 16; ++e) v[e] = leaky_relu_(v[e]);
                            } else if (p.act == 8) {
#pragma unroll
                                for (int e = 0; e < 16; ++e) v[e] = tanh_(v[e]);
                            } else {
#pragma unroll
                                for (int e = 0; e < 16; ++e) v[e] = sigmoidf_(v[e]);
                            }
                        }
                        if (p.amaxC.slot) {
#pragma unroll
                            for (int e = 0; e < 16; e += 2) cmax = fmaxf(cmax, fmaxf(__builtin_fabsf(v[e]), __builtin_fabsf(v[e + 1])));
                        }
#pragma unroll
                        for (int e = 0; e < 16; ++e) wr[WS_DROW(e) * 40 + WS_DCOL(e)] = v[e];
                        float* q = C + (int64_t)(cur.m0 + wm + 32 * a + (lane >> 3)) * p.ldc + cur.n0 + wn + 32 * b + 4 * (lane & 7);
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const float4 t = rdp[g * 8 * 10];                   // rows 8 g + (lane >> 3): 8 rows x 160 bytes = 80 float4
                            if (p.ntst) {                                       // streaming stores (RESEL_GEMM_NT): -4 % on the kernel alone at N = 2048
                                typedef float f4v __attribute__((ext_vector_type(4)));
                                __builtin_nontemporal_store(f4v{t.x, t.y, t.z, t.w}, reinterpret_cast<f4v*>(q + (int64_t)(8 * g) * p.ldc));
                            } else {
                                *reinterpret_cast<float4*>(q + (int64_t)(8 * g) * p.ldc) = t;
                            }
                        }
                    }
                }
                continue;
            }
            // edge tiles and the accumulating form: the accumulator layout goes out as it is - column n = lane & 15 of column tile j,
            // rows 4 (lane >> 4) + r of row tile i
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = cur.n0 + wn + 16 * j + l15;
                if (n >= p.N) continue;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] + bv[j];
                    if (p.act == 1) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = elu1(v[r]);
                    }
                    if (p.act == 3) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = softplus_nb(v[r]);
                    }
                    if constexpr (EPI == 6) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = p.act == 6 ? relu_(v[r]) : p.act == 7 ? leaky_relu_(v[r]) : p.act == 8 ? tanh_(v[r]) : sigmoidf_(v[r]);
                    }
                    const int mb = cur.m0 + wm + 16 * i + 4 * l4;
                    float* crow = C + (int64_t)mb * p.ldc + n;
                    if (p.act == 2) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (mb + r < p.M) v[r] += crow[(int64_t)r * p.ldc];
                    }
                    if (full_m) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) crow[(int64_t)r * p.ldc] = v[r];
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (mb + r < p.M) crow[(int64_t)r * p.ldc] = v[r];
                    }
                    if (p.amaxC.slot) cmax = fmaxf(fmaxf(cmax, fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1]))), fmaxf(__builtin_fabsf(v[2]), __builtin_fabsf(v[3])));
                }
            }
        } else if constexpr (EPI == 4) {
            // ---- dact: C = product * elu'(Y), column sums.  Whole tiles only (the host entry sends the rows past the last whole 256-row
            // tile elsewhere and refuses N % 128 != 0).  Two phases:
            //   A  the Y values are loaded IN THE ACCUMULATOR LAYOUT (column = lane & 15 of column tile j, rows 4 (lane >> 4) + r of row tile i: a dword load
            //      covers two whole 128-byte lines) and multiplied into the accumulators in place, tile by tile with PF tiles of loads in
            //      flight; column sums and the magnitude come from the same registers;
            //   B  the tiles leave exactly as in the plain epilogue (LDS turn, 16-byte full-line non-temporal stores).
            // No store is issued between the loads of an item: a wait for a load also waits for every OLDER store (one in-order counter
            // per wave), and with loads and stores interleaved per tile every tile waited for the write acknowledgements of the tiles
            // before it (measured: 650 us against 305 for the product alone; this form: see profiles/r05_gemm.md).  The loads are inline
            // assembly with a scalar base + ONE per-lane offset register (the compiler formed a 64-bit address pair per load and spilled
            // accumulators; every scratch reload is a vmcnt(0)); it does not count them: each tile waits for ITS sixteen loads with a
            // hand-written vmcnt = the loads issued since (foreign vector-memory operations only make a wait stricter).
            float* C = p.C + (int64_t)cur.z * p.sC;
            constexpr int PF = 3;
            // per-lane constants are formed HERE from the lane id (v_mbcnt) and the wave id in a scalar register: kept across the K loop
            // they were spilled
            const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            const int l15 = lane & 15, l4 = lane >> 4;
            const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
            const int wm = (w >> 1) * 128, wn = (w & 1) * 64;
            typedef float f32x4a __attribute__((ext_vector_type(4)));
            f32x4a yv[8][4];
            // Y travels as 16-byte loads of whole 128-byte lines (a lane: rows 8 g + (lane >> 3), columns 4 (lane & 7) .. + 3 - the form the C
            // tiles leave in) and is turned INTO the accumulator layout through the wave's LDS scratch: dword loads in the accumulator
            // layout cost four times the address work per byte (128 load instructions per item and wave; measured 542 us, this form: r05_gemm.md)
            char* sc = lds + (w >> 1) * STAGE + 2 * PLA + (w & 1) * 5120;
            float* wr = reinterpret_cast<float*>(sc) + (4 * l4) * 40 + l15;
            float4* rdp = reinterpret_cast<float4*>(sc + (lane >> 3) * 160 + (lane & 7) * 16);
            const uint32_t ylane = (uint32_t)(((lane >> 3) * (int)p.ldaux + 4 * (lane & 7)) * 4);
            const float* ybase = p.aux + (int64_t)cur.z * p.sAux + (int64_t)(cur.m0 + wm) * p.ldaux + cur.n0 + wn;
            auto yld = [](f32x4a& r, uint32_t off, const float* base) {        // (asm operands inside the generic lambdas below are not captured: a clang quirk)
                asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(r) : "v"(off), "s"(base) : "memory");
            };
            auto ywait = [](f32x4a& r0, f32x4a& r1, f32x4a& r2, f32x4a& r3, auto NC) {
                asm volatile("s_waitcnt vmcnt(%4)" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3) : "n"(decltype(NC)::value) : "memory");
            };
            auto yload = [&](auto TC) {
                constexpr int t = decltype(TC)::value;
                if constexpr (t < 8) {
                    const float* yb = ybase + (int64_t)(32 * (t >> 1)) * p.ldaux + 32 * (t & 1);
#pragma unroll
                    for (int g = 0; g < 4; ++g) yld(yv[t][g], ylane, yb + (int64_t)(8 * g) * p.ldaux);
                }
            };
            float cs[4] = {0.f, 0.f, 0.f, 0.f}, cmx = 0.f;
            auto mul = [&](auto TC) {
                constexpr int t = decltype(TC)::value;
                constexpr int a = t >> 1, b = t & 1;
                yload(std::integral_constant<int, t + PF>{});
                ywait(yv[t][0], yv[t][1], yv[t][2], yv[t][3], std::integral_constant<int, 4 * ((t + PF < 7 ? t + PF : 7) - t)>{});
#pragma unroll
                for (int g = 0; g < 4; ++g) rdp[g * 8 * 10] = make_float4(yv[t][g].x, yv[t][g].y, yv[t][g].z, yv[t][g].w);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float y = wr[WS_DROW(e) * 40 + WS_DCOL(e)];
                    const float v = WS_ACC(a, b, e) * (y > 0.f ? 1.f : y + 1.f);
                    WS_ACC(a, b, e) = v;
                    cs[2 * b + ((e >> 2) & 1)] += v;
                    cmx = fmaxf(cmx, __builtin_fabsf(v));
                }
            };
            yload(std::integral_constant<int, 0>{}); yload(std::integral_constant<int, 1>{}); yload(std::integral_constant<int, 2>{});
            static_assert(PF == 3, "the prologue issues PF tiles");
            mul(std::integral_constant<int, 0>{}); mul(std::integral_constant<int, 1>{}); mul(std::integral_constant<int, 2>{});
            mul(std::integral_constant<int, 3>{}); mul(std::integral_constant<int, 4>{}); mul(std::integral_constant<int, 5>{});
            mul(std::integral_constant<int, 6>{}); mul(std::integral_constant<int, 7>{});
            if (p.red) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float c = cs[j] + __shfl_xor(cs[j], 16, 64);             // the four row groups of the accumulator layout
                    c += __shfl_xor(c, 32, 64);
                    if (l4 == 0) p.red[((int64_t)cur.z * p.redrows + 2 * (cur.m0 / BM) + (w >> 1)) * p.N + cur.n0 + wn + 16 * j + l15] = c;
                }
            }
            amax_publish_wave(cmx, p.amaxC);                         // one conditional atomic per wave and item (a maximum carried across the K loops was spilled)
            // phase B
#pragma unroll
            for (int b = 0; b < 2; ++b) {
#pragma unroll
                for (int a = 0; a < 4; ++a) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) wr[WS_DROW(e) * 40 + WS_DCOL(e)] = WS_ACC(a, b, e);
                    float* q = C + (int64_t)(cur.m0 + wm + 32 * a + (lane >> 3)) * p.ldc + cur.n0 + wn + 32 * b + 4 * (lane & 7);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 t = rdp[g * 8 * 10];
                        typedef float f4v __attribute__((ext_vector_type(4)));
                        __builtin_nontemporal_store(f4v{t.x, t.y, t.z, t.w}, reinterpret_cast<f4v*>(q + (int64_t)(8 * g) * p.ldc));
                    }
                }
            }
        } else {
            // ---- head: C = a = elu(product + bias), row dots of a with the output layer's weights (aux)
            float* C = p.C + (int64_t)cur.z * p.sC;
            const bool full_m = cur.m0 + BM <= p.M;
            if (full_m && cur.n0 + BN <= p.N) {
                // whole tiles through the wave's LDS scratch, as in the plain epilogue
                char* sc = lds + (w >> 1) * STAGE + 2 * PLA + (w & 1) * 5120;
                float* wr = reinterpret_cast<float*>(sc) + (4 * l4) * 40 + l15;
                const float4* rdp = reinterpret_cast<const float4*>(sc + (lane >> 3) * 160 + (lane & 7) * 16);
                // one 32 x 32 tile (row tile a, column block b).  In the turned form a lane holds rows 8 g + (lane >> 3), columns 4 (lane & 7) .. + 3:
                // w3 = the output layer's weights of the lane's four columns, qr[g] += the lane's share of the row dots
                auto tile = [&](int a, int b, const float4& w3, float (&qr)[4]) {
                    float v[16];
#pragma unroll
                    for (int e = 0; e < 16; ++e) v[e] = WS_ACC(a, b, e) + WS_BV(b, e);
#pragma unroll
                    for (int e = 0; e < 16; ++e) v[e] = elu1(v[e]);
                    if (p.amaxC.slot) {
#pragma unroll
                        for (int e = 0; e < 16; e += 2) cmax = fmaxf(cmax, fmaxf(__builtin_fabsf(v[e]), __builtin_fabsf(v[e + 1])));
                    }
#pragma unroll
                    for (int e = 0; e < 16; ++e) wr[WS_DROW(e) * 40 + WS_DCOL(e)] = v[e];
                    float* q = C + (int64_t)(cur.m0 + wm + 32 * a + (lane >> 3)) * p.ldc + cur.n0 + wn + 32 * b + 4 * (lane & 7);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        float4 t = rdp[g * 8 * 10];
                        qr[g] += (t.x * w3.x + t.y * w3.y) + (t.z * w3.z + t.w * w3.w);
                        if (p.ntst) {                                       // streaming stores (RESEL_GEMM_NT): -4 % on the kernel alone at N = 2048
                            typedef float f4v __attribute__((ext_vector_type(4)));
                            __builtin_nontemporal_store(f4v{t.x, t.y, t.z, t.w}, reinterpret_cast<f4v*>(q + (int64_t)(8 * g) * p.ldc));
                        } else {
                            *reinterpret_cast<float4*>(q + (int64_t)(8 * g) * p.ldc) = t;
                        }
                    }
                };
                // row tiles outermost: the row dots of a tile's 32 rows complete after its two column blocks (4 registers instead of 16)
                float4 w3[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) w3[b] = ld4(p.aux + (int64_t)cur.z * p.sAux + cur.n0 + wn + 32 * b + 4 * (lane & 7));
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    float qr[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int b = 0; b < 2; ++b) tile(a, b, w3[b], qr);
                    // fold the eight column groups (lane bits 0..2): lanes with (lane & 7) == 0 hold a row's dot
                    float* qp = p.red + ((int64_t)cur.z * 2 * p.nt + 2 * (cur.n0 / BN) + (w & 1)) * p.M + cur.m0 + wm + 32 * a + (lane >> 3);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        float r = qr[g];
                        r += __shfl_xor(r, 1, 64); r += __shfl_xor(r, 2, 64); r += __shfl_xor(r, 4, 64);
                        if ((lane & 7) == 0) qp[8 * g] = r;
                    }
                }
                continue;
            }
            // edge tiles: the accumulator layout goes out as it is - column n = lane & 15 of column tile j, rows 4 (lane >> 4) + r of row tile i
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float qe[4] = {0.f, 0.f, 0.f, 0.f};
                const int mb = cur.m0 + wm + 16 * i + 4 * l4;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = cur.n0 + wn + 16 * j + l15;
                    if (n >= p.N) continue;
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = elu1(acc[i][j][r] + bv[j]);
                    const float w3 = p.aux[(int64_t)cur.z * p.sAux + n];
#pragma unroll
                    for (int r = 0; r < 4; ++r) qe[r] += v[r] * w3;
                    float* crow = C + (int64_t)mb * p.ldc + n;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (full_m || mb + r < p.M) crow[(int64_t)r * p.ldc] = v[r];
                    if (p.amaxC.slot) cmax = fmaxf(fmaxf(cmax, fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1]))), fmaxf(__builtin_fabsf(v[2]), __builtin_fabsf(v[3])));
                }
                float* qp = p.red + ((int64_t)cur.z * 2 * p.nt + 2 * (cur.n0 / BN) + (w & 1)) * p.M;     // a row's 64 columns of a wave sit in 16 lanes, four per lane
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float q = qe[r];
#pragma unroll
                    for (int o = 1; o < 16; o <<= 1) q += __shfl_xor(q, o, 64);
                    if (l15 == 0 && mb + r < p.M) qp[mb + r] = q;
                }
            }
        }
    }
#undef WS_ACC
#undef WS_DROW
#undef WS_DCOL
#undef WS_BV
    amax_publish_wave(cmax, p.amaxC);
#ifdef BF3_AB_CLOCK
    if (tid == 0) {
        g_bf3_clock[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - ck_t0;
        g_bf3_clock[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - ck_r0;
    }
#endif
}

// one flag table per kernel instantiation (launch_big_lds)
template <bool AKC, bool BKC, int SP>
int launch_one(const Params& p, dim3 grid, hipStream_t s) {
    static std::atomic<bool> attr_set[64];
    return launch_big_lds(gemm_bf3_kernel<AKC, BKC, SP>, attr_set, grid, dim3(NTH), 2 * STAGE, s, p);
}
template <bool AKC, bool BKC, int EPI = 0>
int launch_ws(const Params& p, dim3 grid, hipStream_t s) {
    static std::atomic<bool> attr_set[64];
    return launch_big_lds(gemm_ws_kernel<AKC, BKC, EPI>, attr_set, grid, dim3(NTH_WS), WS_LDS, s, p);
}

constexpr int g_nt = 1;               // non-temporal C stores of the third edition: 23.43 -> 23.30 ms per update, same box

}  // namespace

#ifdef BF3_AB_CLOCK
extern "C" int resel_bf3_debug_clock(unsigned long long* host_out) {
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_bf3_clock), sizeof(unsigned long long) * 2 * GRID);
}
#endif

namespace resel {

size_t gemm_bf3_workspace_bytes(int M, int N, int K, int batch) {
    const Plan pl = make_plan<BM, BN, GRID>(M, N, K, batch);
    return (size_t)pl.nsplit * pl.nsl * TILE * sizeof(float);
}

// whole K steps, also per K slice: what the third edition's (producer / consumer waves, mode 2) items must be
inline bool whole_k_steps(int K, int kslice) { return K % BK == 0 && kslice % BK == 0; }

// the fused epilogues (act 4 / 5) exist on the third edition, for whole-K items (one slice = K): mode 2, M > 128
bool gemm_bf3_fused_ok(int M, int N, int K) { return M > 128 && N >= 4 && K >= BK && whole_k_steps(K, K); }

int gemm_bf3_launch(const GemmCall& c, int split, const GemmFused& fused) {
    if (split == 2 && (!c.amax_a || !c.amax_b)) return RESEL_EINVAL;
    const int M = c.M, N = c.N, K = c.K, act = c.act;
    Plan pl = make_plan<BM, BN, GRID>(M, N, K, c.batch);
    if (act == 4 || act == 5) {                      // every tile whole: the epilogue reductions are written per (tile, wave), no K slices
        if (split != 2 || !gemm_bf3_fused_ok(M, N, K) || !fused.aux) return RESEL_EINVAL;
        if (act == 4 && (M % BM || N % BN)) return RESEL_EINVAL;          // the act 4 epilogue has no edge form (resel_gemm_f32_dact splits the rows)
        if (!c.a_kcontig) return RESEL_EINVAL;                            // the layouts the trainer uses: A [rows][K]; B either way
        const long nbt = (long)((M + BM - 1) / BM) * ((N + BN - 1) / BN) * c.batch;
        pl = Plan{(int)nbt, 0, 1, (K + BK - 1) / BK * BK};
    }
    if (pl.nsplit && (!c.workspace || !aligned16(c.workspace))) return RESEL_EINVAL;
    Params p{(const float*)c.A, c.B, c.bias, (float*)c.C, (float*)c.workspace, c.lda, c.ldb, c.ldc, c.strideA, c.strideB, c.strideC, c.strideBias,
             M, N, K, act, (M + BM - 1) / BM, (N + BN - 1) / BN, pl.nfull, pl.nsplit, pl.nsl, pl.kslice, c.amax_a, c.amax_b,
             AmaxOut{c.amax_c, c.amax_epoch}, g_nt, fused.aux, fused.ldaux, fused.strideAux, fused.red, fused.redrows};
    dim3 grid((unsigned)std::min<int64_t>((int64_t)pl.nfull + (int64_t)pl.nsplit * pl.nsl, GRID));
    const bool third = split == 2 && whole_k_steps(K, pl.kslice);
    const int rc = with_layout(c.a_kcontig, c.b_kcontig, [&](auto akc, auto bkc) {
        constexpr bool AKC = akc.value, BKC = bkc.value;
        if constexpr (AKC) {
            if (act == 4 || act == 5) return act == 4 ? launch_ws<true, BKC, 4>(p, grid, c.s) : launch_ws<true, BKC, 5>(p, grid, c.s);
        }
        if (third) return act >= 6 ? launch_ws<AKC, BKC, 6>(p, grid, c.s) : launch_ws<AKC, BKC>(p, grid, c.s);
        if (split == 3) return launch_one<AKC, BKC, 3>(p, grid, c.s);
        if (split == 2) return launch_one<AKC, BKC, 2>(p, grid, c.s);
        return launch_one<AKC, BKC, 6>(p, grid, c.s);
    });
    if (rc != RESEL_OK) return rc;
    if (pl.nsplit) hipLaunchKernelGGL((gemm_fixup_kernel<BM, BN, Params>), dim3(TILE / 4 / 64, pl.nsplit), dim3(64, 4), 0, c.s, p);
#ifdef BF3_AB_FIXUP2                    // ablation (right results): every fix-up launched TWICE - what the 86 fix-up launches of an update cost, measured
    if (pl.nsplit && act != 2) hipLaunchKernelGGL((gemm_fixup_kernel<BM, BN, Params>), dim3(TILE / 4 / 64, pl.nsplit), dim3(64, 4), 0, c.s, p);   // with the data left intact
#endif                                  // (skipping the fix-up instead leaves garbage tiles: the degenerate data lowers the chip's power draw, its clock
                                        //  rises and EVERY kernel of the update runs 5-13 % faster - profiles/r06_gemm.md)
    return launch_status();
}

}  // namespace resel
