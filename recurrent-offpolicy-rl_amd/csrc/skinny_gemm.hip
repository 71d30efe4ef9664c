// C = W^T N over a very long reduction dimension: the weight-gradient GEMMs of the narrow Mamba projections
//   d(dt_proj.weight)[Di, R]    = ddelta[M, Di]^T  x_dbl[M, :R]         (R = 16)
//   d(x_proj.weight)[R+2N, Di]  = dx_dbl[M, R+2N]^T xc[M, Di]           (R + 2N = 80)
// with M = rows * T' = 66 752 tokens at config 2 (reference: autograd of the three F.linear calls in
// mamba_ssm/ops/selective_scan_interface_new.py:261-335).  The outputs are tiny (8 K / 41 K floats), the reduction is 66 752
// long: the library's kernels for these shapes reach 7 - 70 TFLOP/s (149 / 77 us); the operation is bound by reading the wide
// operand once (137 MB ~ 25 us at HBM speed).
//
// Layout trick: v_mfma_f32_32x32x2_f32 wants lane l to hold operand element [l % 32][k = l / 32].  Both operands are row-major
// [k][column], so a half-wave reads 32 consecutive columns of row k - and if every lane reads a float4 (4 consecutive columns)
// the four components are the A operands of FOUR output tiles whose rows are the columns 4 i + e (a permutation of the 128
// columns the wave owns).  One 16-byte load per lane feeds four MFMAs; no LDS, no transposes.  The reduction dimension is
// split over the grid; partial tiles go to a workspace in the FINAL layout and are summed in a fixed order (colsum_kernel),
// so the result is bitwise reproducible.
#include <type_traits>
#include "resel_common.h"

namespace {
using namespace resel;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// C row of accumulator register r of lane l in a 32x32 tile (column = l % 32)
__device__ __forceinline__ int acc_row(int r, int half) { return (r >> 2) * 8 + half * 4 + (r & 3); }

// grid (ksplit, ceil(Wd / 512)); 256 threads = 4 waves x 128 wide columns.  NT = number of 32-column tiles of the narrow operand.
template <int NT>
__global__ __launch_bounds__(256) void atb_kernel(const float* __restrict__ Wm, int64_t ldw, int Wd, const float* __restrict__ Nm,
                                                  int64_t ldn, int Nd, float* __restrict__ part, int64_t K, int rows_per,
                                                  int transposed) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int wb = blockIdx.y * 512 + wave * 128;
    if (wb >= Wd) return;
    const int64_t k0 = (int64_t)blockIdx.x * rows_per;
    const int64_t k1 = k0 + rows_per < K ? k0 + rows_per : K;
    f32x16 acc[4][NT];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[e][t][r] = 0.f;
    const int wc = wb + 4 * col;
    const bool w_ok = wc < Wd;                                   // Wd % 4 == 0: a float4 is inside or outside as a whole
    bool n_ok[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) n_ok[t] = 32 * t + col < Nd;
    constexpr int UN = NT == 1 ? 8 : 4;                          // k-pairs in flight per iteration
    for (int64_t k = k0; k < k1; k += 2 * UN) {
        float4 a[UN];
        float b[UN][NT];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int64_t kr = k + 2 * u + half;
            const bool ok = kr < k1;
            a[u] = (ok && w_ok) ? ld4(Wm + kr * ldw + wc) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < NT; ++t) b[u][t] = (ok && n_ok[t]) ? Nm[kr * ldn + 32 * t + col] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < UN; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc[0][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].x, b[u][t], acc[0][t], 0, 0, 0);
                acc[1][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].y, b[u][t], acc[1][t], 0, 0, 0);
                acc[2][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].z, b[u][t], acc[2][t], 0, 0, 0);
                acc[3][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].w, b[u][t], acc[3][t], 0, 0, 0);
            }
    }
    // partial slab of this k-split in the final layout: C[w][n] (ld Nd) or, transposed, C[n][w] (ld Wd)
    float* dst = part + (int64_t)blockIdx.x * Wd * Nd;
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = 32 * t + col;
            if (n >= Nd) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int w = wb + 4 * acc_row(r, half) + e;
                if (w < Wd) dst[transposed ? (int64_t)n * Wd + w : (int64_t)w * Nd + n] = acc[e][t][r];
            }
        }
}

// ---- products with one side at most 48 wide (the rank-16 time-step projection of the Mamba mixer and its gradients) -------------------
// Each needs ~1 GFLOP and moves 137 MB at the flagship shape: one pass over the wide side is the whole cost, the fp32 instruction is
// fast enough, and neither the 256 x 128 tiles nor the operand split of the big GEMM help.
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float2 ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }

// ELU with expm1's accuracy near zero (exp(x) - 1 cancels there): Taylor to x^9 on [-0.5, 0], remainder 0.5^10 / 10! = 2.7e-10.
// Both sides are computed and selected: no divergent branch in the store loop.
__device__ __forceinline__ float elu_acc(float x) {
    float p = 1.f / 362880.f;
    p = __builtin_fmaf(p, x, 1.f / 40320.f);
    p = __builtin_fmaf(p, x, 1.f / 5040.f);
    p = __builtin_fmaf(p, x, 1.f / 720.f);
    p = __builtin_fmaf(p, x, 1.f / 120.f);
    p = __builtin_fmaf(p, x, 1.f / 24.f);
    p = __builtin_fmaf(p, x, 1.f / 6.f);
    p = __builtin_fmaf(p, x, 0.5f);
    p = __builtin_fmaf(p, x, 1.f);
    const float neg = x > -0.5f ? p * x : fast_exp(x) - 1.f;
    return x > 0.f ? x : neg;
}

// C[M, N] = act(A[M, :K] W[N, K]^T + bias), K <= 4 KQ <= 48.  A wave owns 128 output columns and keeps their weight rows in registers
// (8 KQ of them); 32-token tiles stream through.  The atb layout turned round: lane (col, half) holds W[n0 + 4 col + e][k] as the B operand
// of four 32x32x2 products e = 0..3, so the four accumulators of a lane are four CONSECUTIVE output columns of one row - every store
// instruction writes two whole 512-byte row segments as float4s, no LDS turn needed.  Any assignment of k to (step, half) is allowed as
// long as both operands use it: k = 4 q + 2 half + c lets both load float2s.
// The loop has no branch around a load or a product (the compiler waits for EVERY outstanding store at such a join, which undoes the
// prefetch): rows past M and steps past K read a clamped, valid address - the rows are never stored, the steps meet zero weights.
// grid (token groups, column groups); 4 waves = wn column chunks x 4 / wn token tiles.  ACT: the GEMM epilogue codes 0 / 1 (ELU) / 3 (softplus).
template <int KQ, int ACT>
__global__ __launch_bounds__(256) void narrow_k_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ W, int64_t ldw,
                                                       const float* __restrict__ bias, float* __restrict__ C, int64_t ldc, int64_t M, int N,
                                                       int K, int wn, int64_t ntiles, AmaxOut amax) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int cw = wave & (wn - 1), tw = wave / wn, TW = 4 / wn;
    const int nb = (blockIdx.y * wn + cw) * 128;
    if (nb >= N) return;
    const int n0 = nb + 4 * col;
    const bool n_ok = n0 < N;                                    // N % 4 == 0: a lane's four columns are inside or outside together
    const int nr = n_ok ? n0 : 0;
    int kc[KQ];
#pragma unroll
    for (int q = 0; q < KQ; ++q) kc[q] = (4 * q < K ? 4 * q : 0) + 2 * half;
    float2 wr[KQ][4];
#pragma unroll
    for (int q = 0; q < KQ; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float2 w = ld2(W + (int64_t)(nr + e) * ldw + kc[q]);
            wr[q][e] = (n_ok && 4 * q < K) ? w : make_float2(0.f, 0.f);
        }
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bias != nullptr) {
        bv = make_float4(bias[nr], bias[nr + 1], bias[nr + 2], bias[nr + 3]);
        if (!n_ok) bv = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float mx = 0.f;
    int64_t tile = (int64_t)blockIdx.x * TW + tw;
    const int64_t tstep = (int64_t)gridDim.x * TW;
    float2 a[KQ];
    {
        int64_t t = tile * 32 + col;
        t = t < M ? t : M - 1;
#pragma unroll
        for (int q = 0; q < KQ; ++q) a[q] = ld2(A + t * lda + kc[q]);
    }
    // one tile: prefetch the next, multiply, store.  MASKED = false: every row and every lane's columns are inside - the stores are
    // unconditional, so the wait for the prefetched rows can leave them in flight (a store under a lane mask sits behind a branch, and
    // at its join the compiler waits for everything outstanding)
    auto do_tile = [&](auto masked_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        float2 an[KQ];                                           // the next tile's rows are on their way while this one multiplies and stores
        {
            int64_t t = (tile + tstep) * 32 + col;
            t = t < M ? t : M - 1;
#pragma unroll
            for (int q = 0; q < KQ; ++q) an[q] = ld2(A + t * lda + kc[q]);
        }
        f32x16 acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[e][r] = 0.f;
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, wr[q][e].x, acc[e], 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, wr[q][e].y, acc[e], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = tile * 32 + acc_row(r, half);
            float4 v = make_float4(acc[0][r] + bv.x, acc[1][r] + bv.y, acc[2][r] + bv.z, acc[3][r] + bv.w);
            if (ACT == 3) v = make_float4(softplus_nb(v.x), softplus_nb(v.y), softplus_nb(v.z), softplus_nb(v.w));
            if (ACT == 1) v = make_float4(elu_acc(v.x), elu_acc(v.y), elu_acc(v.z), elu_acc(v.w));
            if (!MASKED || (row < M && n_ok)) {
                st4(C + row * ldc + n0, v);
                mx = amax4(mx, v);
            }
        }
#pragma unroll
        for (int q = 0; q < KQ; ++q) a[q] = an[q];
    };
    // (first tile outside the loop: both ways into the loop head then have the 16 stores behind the prefetch, and the wait there is
    // vmcnt(16), not the vmcnt(0) a store-free entry edge would force)
    if (nb + 128 <= N && (tile + 1) * 32 <= M) {                 // wave-uniform: all 128 columns of the chunk exist
        do_tile(std::false_type{});
        for (tile += tstep; (tile + 1) * 32 <= M; tile += tstep) do_tile(std::false_type{});
    }
    for (; tile < ntiles; tile += tstep) do_tile(std::true_type{});           // the ragged last tile; chunks cut by N
    amax_publish_wave(mx, amax);
}

// One pass over a wide G[M, Wd <= 512]: dX[M, Nn] = G W[Wd, Nn] and dW[Wd, Nn] = G^T X[M, Nn], Nn <= 16 NT <= 48, on the 16x16x4 fp32
// instruction (no idle half tile at Nn = 16).  grid = slices of `rows_per` rows; 4 waves x 128 columns of G; 16-row blocks.
//  - A block is loaded once, as float4s along the rows: lane (i, kq) gets G[4 s + kq][64 h + 4 i + e] - directly the A operand of the
//    dW tiles (rows w = 64 h + 4 i + e, reduction over the block's rows), accumulated over the slice and written as a partial slab.
//  - For dX the reduction runs along the row, so the block is turned through the wave's own LDS tile: lane (i, kq) reads row i, columns
//    16 q + 4 kq + c, against the wave's resident part of W.  The four waves' partial sums meet in LDS and are added in wave order.
// Both outputs are sums in a fixed order: bitwise reproducible.
template <int NT, bool DX, bool DW>
__global__ __launch_bounds__(256) void narrow_n_pair_kernel(const float* __restrict__ G, int64_t ldg, int Wd, const float* __restrict__ Wm,
                                                            int64_t ldw, const float* __restrict__ X, int64_t ldx, int Nn,
                                                            float* __restrict__ dX, int64_t lddx, float* __restrict__ part, int64_t M,
                                                            int rows_per) {
    __shared__ float s_g[DX ? 4 : 1][16][132];                   // row stride 132: the turned float4 reads spread over all banks
    __shared__ float s_px[DX ? 2 : 1][4][16][16 * NT];           // partial dX per wave; two copies: one barrier per block
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, kq = lane >> 4;
    const int wb = wave * 128;
    if (!DX && wb >= Wd) return;
    const int64_t k0 = (int64_t)blockIdx.x * rows_per;
    const int64_t k1 = k0 + rows_per < M ? k0 + rows_per : M;
    const int nblk = (int)((k1 - k0 + 15) / 16);
    bool n_ok[NT], w_ok[2];
#pragma unroll
    for (int t = 0; t < NT; ++t) n_ok[t] = 16 * t + i16 < Nn;
#pragma unroll
    for (int h = 0; h < 2; ++h) w_ok[h] = wb + 64 * h + 4 * i16 < Wd;      // Wd % 4 == 0
    // no branch around a load (the compiler would wait for every outstanding access at the join): what lies outside reads a clamped,
    // valid address and is replaced by zero
    int nc[NT], gc[2];
#pragma unroll
    for (int t = 0; t < NT; ++t) nc[t] = n_ok[t] ? 16 * t + i16 : 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) gc[h] = w_ok[h] ? wb + 64 * h + 4 * i16 : 0;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool fast = wb + 128 <= Wd && Nn == 16 * NT && ((k1 - k0) & 15) == 0;      // wave-uniform
    float wr[DX ? 8 : 1][4][NT];
    auto load_w = [&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int w = wb + 16 * q + 4 * kq + c;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float v = Wm[(int64_t)(FAST || w < Wd ? w : 0) * ldw + nc[t]];
                    wr[q][c][t] = (FAST || (w < Wd && n_ok[t])) ? v : 0.f;
                }
            }
    };
    if (DX) {
        if (fast) load_w(std::true_type{});
        else load_w(std::false_type{});
    }
    f32x4 accW[2][4][NT];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < NT; ++t) accW[h][e][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 g[4][2];
    float xb[4][NT];
    // rows [m0, m0 + 16) of the wave's columns (and of X).  FAST: the slice is whole blocks and all of the wave's columns and all 16 NT narrow
    // columns exist - plain loads (a block past the slice re-reads its last row and is never used).  Otherwise what lies outside reads a
    // clamped, valid address and is replaced by zero.
    auto load_block = [&](auto fast_tag, int64_t m0, float4 (&gd)[4][2], float (&xd)[4][NT]) {
        constexpr bool FAST = decltype(fast_tag)::value;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t m = m0 + 4 * s + kq, mr = m < k1 ? m : k1 - 1;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float4 v = ld4(G + mr * ldg + gc[h]);
                gd[s][h] = (FAST || (m < k1 && w_ok[h])) ? v : zero4;
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float v = DW ? X[mr * ldx + nc[t]] : 0.f;
                xd[s][t] = (FAST || (m < k1 && n_ok[t])) ? v : 0.f;
            }
        }
    };
    if (fast) load_block(std::true_type{}, k0, g, xb);
    else load_block(std::false_type{}, k0, g, xb);
    // one 16-row block.  No load and (FAST) no store sits behind a branch: at such a join the compiler waits for everything outstanding,
    // which would put the dX stores of the block before in front of every block
    auto do_block = [&](auto fast_tag, int b) {
        constexpr bool FAST = decltype(fast_tag)::value;
        const int64_t m0 = k0 + 16 * (int64_t)b;
        float4 gn[4][2];                                         // the next block is in flight while this one is multiplied
        float xn[4][NT];
        load_block(fast_tag, m0 + 16, gn, xn);
        if (DW) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        accW[h][0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[s][h].x, xb[s][t], accW[h][0][t], 0, 0, 0);
                        accW[h][1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[s][h].y, xb[s][t], accW[h][1][t], 0, 0, 0);
                        accW[h][2][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[s][h].z, xb[s][t], accW[h][2][t], 0, 0, 0);
                        accW[h][3][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[s][h].w, xb[s][t], accW[h][3][t], 0, 0, 0);
                    }
        }
        if (DX) {
            float (*sg)[132] = s_g[DX ? wave : 0];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int h = 0; h < 2; ++h) st4(&sg[4 * s + kq][64 * h + 4 * i16], g[s][h]);
            // the tile is this wave's own and LDS serves a wave in order: a wave-level fence is all the turn needs
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            f32x4 accX[NT], accY[NT];                              // two chains (even / odd q): dependent MFMAs do not queue behind each other
#pragma unroll
            for (int t = 0; t < NT; ++t) accX[t] = accY[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 8; q += 2) {
                const float4 a = ld4(&sg[i16][16 * q + 4 * kq]);
                const float4 c = ld4(&sg[i16][16 * q + 16 + 4 * kq]);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    accX[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wr[q][0][t], accX[t], 0, 0, 0);
                    accY[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.x, wr[q + 1][0][t], accY[t], 0, 0, 0);
                    accX[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wr[q][1][t], accX[t], 0, 0, 0);
                    accY[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.y, wr[q + 1][1][t], accY[t], 0, 0, 0);
                    accX[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wr[q][2][t], accX[t], 0, 0, 0);
                    accY[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.z, wr[q + 1][2][t], accY[t], 0, 0, 0);
                    accX[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wr[q][3][t], accX[t], 0, 0, 0);
                    accY[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.w, wr[q + 1][3][t], accY[t], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) accX[t] += accY[t];
            float (*px)[16][16 * NT] = s_px[DX ? (b & 1) : 0];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) px[wave][4 * kq + r][16 * t + i16] = accX[t][r];      // D: row 4 (lane / 16) + r, column lane % 16
            __syncthreads();
            const int row = threadIdx.x >> 4, nn = threadIdx.x & 15;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int n = 16 * t + nn;
                if (FAST || (n < Nn && m0 + row < k1))
                    dX[(m0 + row) * lddx + n] = ((px[0][row][n] + px[1][row][n]) + px[2][row][n]) + px[3][row][n];
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int h = 0; h < 2; ++h) g[s][h] = gn[s][h];
#pragma unroll
            for (int t = 0; t < NT; ++t) xb[s][t] = xn[s][t];
        }
    };
    // (both forms have one barrier per block, so the waves of a workgroup may differ in theirs; the first block stands outside the loop so
    // that both ways into the loop head have the same accesses behind the prefetch)
    if (fast) {
        do_block(std::true_type{}, 0);
        for (int b = 1; b < nblk; ++b) do_block(std::true_type{}, b);
    } else {
        for (int b = 0; b < nblk; ++b) do_block(std::false_type{}, b);
    }
    if (DW) {                                                    // partial slab of this slice in the final layout [Wd][Nn]
        float* dst = part + (int64_t)blockIdx.x * Wd * Nn;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int w = wb + 64 * h + 4 * (4 * kq + r) + e;
                        if (w < Wd && n_ok[t]) dst[(int64_t)w * Nn + 16 * t + i16] = accW[h][e][t][r];
                    }
    }
}

inline int pick_ksplit(int64_t K, int Wd, int Nd) {
    // enough workgroups to pull HBM bandwidth, partial slabs bounded to ~16 MB
    int64_t ks = (int64_t)(16 << 20) / ((int64_t)Wd * Nd * 4);
    if (ks > 512) ks = 512;
    if (ks < 32) ks = 32;
    if (ks > (K + 1) / 2) ks = (K + 1) / 2;
    return (int)(ks < 1 ? 1 : ks);
}

inline int pair_rows_per(int64_t M, int Wd, int Nn) {
    const int ks = pick_ksplit(M, Wd, Nn);
    const int64_t r = (M + ks - 1) / ks;
    return (int)((r + 15) / 16 * 16);                            // whole 16-row blocks: at most pick_ksplit slices
}
template <int NT>
void launch_pair(dim3 grid, hipStream_t s, bool dx, bool dw, const float* G, int64_t ldg, int Wd, const float* Wm, int64_t ldw, const float* X,
                 int64_t ldx, int Nn, float* dX, int64_t lddx, float* part, int64_t M, int rows_per) {
    const dim3 block(256);
    if (dx && dw) hipLaunchKernelGGL((narrow_n_pair_kernel<NT, true, true>), grid, block, 0, s, G, ldg, Wd, Wm, ldw, X, ldx, Nn, dX, lddx, part, M, rows_per);
    else if (dx) hipLaunchKernelGGL((narrow_n_pair_kernel<NT, true, false>), grid, block, 0, s, G, ldg, Wd, Wm, ldw, X, ldx, Nn, dX, lddx, part, M, rows_per);
    else hipLaunchKernelGGL((narrow_n_pair_kernel<NT, false, true>), grid, block, 0, s, G, ldg, Wd, Wm, ldw, X, ldx, Nn, dX, lddx, part, M, rows_per);
}
}  // namespace

extern "C" {

size_t resel_atb_workspace_bytes(int64_t K, int Wd, int Nd) {
    return (size_t)pick_ksplit(K, Wd, Nd) * Wd * Nd * sizeof(float);
}

int resel_atb(const float* wide, int64_t ldw, int Wd, const float* narrow, int64_t ldn, int Nd, float* out, int transposed,
              void* workspace, int64_t K, resel_stream_t stream) {
    if (!wide || !narrow || !out || !workspace || K <= 0 || Wd <= 0 || Nd <= 0) return RESEL_EINVAL;
    if (Nd > 96 || (Wd & 3) || (ldw & 3) || !aligned16(wide)) return RESEL_EINVAL;
    const int ks = pick_ksplit(K, Wd, Nd);
    int rows_per = (int)((K + ks - 1) / ks);
    rows_per += rows_per & 1;                                    // k-pairs never straddle two splits
    const int nsplit = (int)((K + rows_per - 1) / rows_per);
    const dim3 grid(nsplit, (Wd + 511) / 512), block(256);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    const int NT = (Nd + 31) / 32;
    switch (NT) {
        case 1: hipLaunchKernelGGL(atb_kernel<1>, grid, block, 0, s, wide, ldw, Wd, narrow, ldn, Nd, part, K, rows_per, transposed); break;
        case 2: hipLaunchKernelGGL(atb_kernel<2>, grid, block, 0, s, wide, ldw, Wd, narrow, ldn, Nd, part, K, rows_per, transposed); break;
        default: hipLaunchKernelGGL(atb_kernel<3>, grid, block, 0, s, wide, ldw, Wd, narrow, ldn, Nd, part, K, rows_per, transposed); break;
    }
    launch_colsum(part, (int64_t)Wd * Nd, nsplit, Wd * Nd, out, s);
    return launch_status();
}

int resel_narrow_k(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, float* C, int64_t ldc, int64_t M, int N,
                   int K, int act, void* amax_out, unsigned amax_epoch, resel_stream_t stream) {
    if (!A || !W || !C || M <= 0 || N <= 0 || K < 4 || K > 48 || (K & 3) || (N & 3)) return RESEL_EINVAL;
    if (act != 0 && act != 1 && act != 3) return RESEL_EINVAL;
    if ((lda & 1) || (ldw & 1) || (ldc & 3) || lda < K || ldw < K || ldc < N) return RESEL_EINVAL;
    if ((reinterpret_cast<uintptr_t>(A) & 7u) || (reinterpret_cast<uintptr_t>(W) & 7u) || !aligned16(C)) return RESEL_EINVAL;
    const int nchunks = (N + 127) / 128;
    const int wn = nchunks >= 4 ? 4 : (nchunks >= 2 ? 2 : 1);
    const int gy = (nchunks + wn - 1) / wn;
    const int64_t ntiles = (M + 31) / 32;
    const int64_t iters = (ntiles + 4 / wn - 1) / (4 / wn);
    const int slots = 256 * (K <= 16 ? 2 : 1);                   // workgroups the chip holds at once (register-bound: 2 or 1 per CU)
    const int64_t maxwg = gy >= slots ? 1 : slots / gy;          // all resident together; each strides over the token tiles
    const dim3 grid((unsigned)(iters < maxwg ? iters : maxwg), gy), block(256);
    hipStream_t s = (hipStream_t)stream;
    const AmaxOut ao{(unsigned long long*)amax_out, amax_epoch};
#define RESEL_NK_LAUNCH(KQ, ACT) \
    hipLaunchKernelGGL((narrow_k_kernel<KQ, ACT>), grid, block, 0, s, A, lda, W, ldw, bias, C, ldc, M, N, K, wn, ntiles, ao)
#define RESEL_NK_ACT(KQ) \
    do { if (act == 3) RESEL_NK_LAUNCH(KQ, 3); else if (act == 1) RESEL_NK_LAUNCH(KQ, 1); else RESEL_NK_LAUNCH(KQ, 0); } while (0)
    if (K <= 16) RESEL_NK_ACT(4);
    else if (K <= 32) RESEL_NK_ACT(8);
    else RESEL_NK_ACT(12);
#undef RESEL_NK_ACT
#undef RESEL_NK_LAUNCH
    return launch_status();
}

size_t resel_narrow_n_pair_workspace_bytes(int64_t M, int Wd, int Nn) {
    return (size_t)pick_ksplit(M, Wd, Nn) * Wd * Nn * sizeof(float);
}

int resel_narrow_n_pair(const float* G, int64_t ldg, int Wd, const float* W, int64_t ldw, const float* X, int64_t ldx, int Nn, float* dX,
                        int64_t lddx, float* dW, void* workspace, int64_t M, resel_stream_t stream) {
    if (!G || M <= 0 || Wd <= 0 || Wd > 512 || (Wd & 3) || Nn <= 0 || Nn > 48 || (ldg & 3) || ldg < Wd || !aligned16(G)) return RESEL_EINVAL;
    if (!dX && !dW) return RESEL_EINVAL;
    if (dX && (!W || ldw < Nn || lddx < Nn)) return RESEL_EINVAL;
    if (dW && (!X || !workspace || ldx < Nn)) return RESEL_EINVAL;
    const int rows_per = pair_rows_per(M, Wd, Nn);
    const int nsplit = (int)((M + rows_per - 1) / rows_per);
    const dim3 grid(nsplit);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    switch ((Nn + 15) / 16) {
        case 1: launch_pair<1>(grid, s, dX != nullptr, dW != nullptr, G, ldg, Wd, W, ldw, X, ldx, Nn, dX, lddx, part, M, rows_per); break;
        case 2: launch_pair<2>(grid, s, dX != nullptr, dW != nullptr, G, ldg, Wd, W, ldw, X, ldx, Nn, dX, lddx, part, M, rows_per); break;
        default: launch_pair<3>(grid, s, dX != nullptr, dW != nullptr, G, ldg, Wd, W, ldw, X, ldx, Nn, dX, lddx, part, M, rows_per); break;
    }
    if (dW) launch_colsum(part, (int64_t)Wd * Nn, nsplit, Wd * Nn, dW, s);
    return launch_status();
}

}  // extern "C"
