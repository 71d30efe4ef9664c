// Tiling and split-K code of the persistent fp32 GEMM kernels (gemm_f32.hip: 128 x 128 tiles; gemm_bf3.hip: 256 x 128 tiles).
// Blocks walk items: whole output tiles, and K slices of the tiles of the last, partly filled round (and of weight gradients: few
// tiles, K = 66 752) whose partial sums go to a workspace slab; a fix-up kernel adds the slices in a fixed order (deterministic, no
// atomics) and applies bias / activation.  Templated on the block tile <BM, BN> and on the file's parameter struct P, which has
// A, B, bias, C, slab, ld*, s*, M, N, K, act, mt, nt, nfull, nsplit, nsl, kslice, amaxC (GemmParams / Params: each file keeps its own,
// the kernels receive it by value).
#pragma once
#include "resel_common.h"
#include <algorithm>
#include <atomic>

namespace resel {

constexpr int BK = 32;                 // K step of every kernel that walks these items

__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : fast_exp(x) - 1.f; }

// Partial sums of a K slice: the wave's NA x 2 accumulator tiles (D layout: column = lane & 31, rows (e & 3) + 8 (e >> 2) + 4 (lane >> 5))
// -> the item's dense slab tile of BN columns; o = the lane's place in the wave's first tile.  gemm_ws_kernel keeps its own copy.
template <int BN, typename ACC, int NA>
__device__ __forceinline__ void slab_store(float* o, const ACC (&acc)[NA][2]) {
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[(32 * a + (e & 3) + 8 * (e >> 2)) * BN + 32 * b] = acc[a][b][e];
}

// tile t (member-major) -> member z, tile origin (m0, n0).  XCD-aware: the tiles of one XCD (ids congruent mod 8) walk the
// n-tiles of one m-tile after another.
template <int BM, int BN, typename P>
__device__ __forceinline__ void tile_origin(const P& p, int t, int& z, int& m0, int& n0) {
    const int ntile = p.mt * p.nt;
    z = t / ntile;
    const int tt = t - z * ntile;
    const int q = ntile / 8, r = ntile % 8, x = tt & 7, j = tt >> 3;
    const int bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
    m0 = (bid / p.nt) * BM;
    n0 = (bid % p.nt) * BN;
}

struct Item { int m0, n0, z, kbeg, kend, split; };     // split: index of the slab tile + 1, 0 for a whole tile
template <int BM, int BN, typename P>
__device__ __forceinline__ Item decode(const P& p, int it) {
    Item o;
    int t = it;
    o.kbeg = 0; o.kend = p.K; o.split = 0;
    if (it >= p.nfull) {
        const int idx = it - p.nfull, tr = idx / p.nsl, sl = idx - tr * p.nsl;
        t = p.nfull + tr;
        o.kbeg = sl * p.kslice; o.kend = min(p.K, o.kbeg + p.kslice); o.split = idx + 1;
    }
    tile_origin<BM, BN>(p, t, o.z, o.m0, o.n0);
    return o;
}

// C tile = epi(sum over the K slices of a split tile).  Fixed summation order (deterministic): four interleaved slice groups
// (threadIdx.y) accumulate slices q, q + 4, ... each, then ((g0 + g1) + (g2 + g3)).  grid (BM * BN / 4 / 64, split tiles), block (64, 4).
template <int BM, int BN, typename P>
__global__ __launch_bounds__(256) void gemm_fixup_kernel(P p) {
    static_assert(BN == 128, "a slab row is 32 float4");
    constexpr int TILE = BM * BN;
    __shared__ float4 part[3][64];
    const int tr = blockIdx.y, q = threadIdx.y;
    const int e = blockIdx.x * 64 + threadIdx.x, ml = e >> 5, nl = 4 * (e & 31);
    const float* s = p.slab + (int64_t)tr * p.nsl * TILE + ml * BN + nl;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int i = q;
    for (; i + 12 < p.nsl; i += 16) {                     // four loads in flight per thread
        const float4 u0 = ld4(s + (int64_t)i * TILE), u1 = ld4(s + (int64_t)(i + 4) * TILE);
        const float4 u2 = ld4(s + (int64_t)(i + 8) * TILE), u3 = ld4(s + (int64_t)(i + 12) * TILE);
        v.x = (((v.x + u0.x) + u1.x) + u2.x) + u3.x; v.y = (((v.y + u0.y) + u1.y) + u2.y) + u3.y;
        v.z = (((v.z + u0.z) + u1.z) + u2.z) + u3.z; v.w = (((v.w + u0.w) + u1.w) + u2.w) + u3.w;
    }
    for (; i < p.nsl; i += 4) {
        const float4 u = ld4(s + (int64_t)i * TILE);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    if (q) part[q - 1][threadIdx.x] = v;
    __syncthreads();
    if (q) return;
    const float4 g1 = part[0][threadIdx.x], g2 = part[1][threadIdx.x], g3 = part[2][threadIdx.x];
    float o[4] = {(v.x + g1.x) + (g2.x + g3.x), (v.y + g1.y) + (g2.y + g3.y), (v.z + g1.z) + (g2.z + g3.z), (v.w + g1.w) + (g2.w + g3.w)};
    int z, m0, n0;
    tile_origin<BM, BN>(p, p.nfull + tr, z, m0, n0);
    const int m = m0 + ml, n = n0 + nl;
    float cmax = 0.f;
    if (m < p.M && n < p.N) {
        float* c = p.C + (int64_t)z * p.sC + (int64_t)m * p.ldc + n;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (n + j >= p.N) break;
            float x = o[j] + (p.bias ? p.bias[(int64_t)z * p.sBias + n + j] : 0.f);
            if (p.act == 1) x = elu1(x);
            if (p.act == 3) x = softplus_nb(x);
            if (p.act >= 6) x = p.act == 6 ? relu_(x) : p.act == 7 ? leaky_relu_(x) : p.act == 8 ? tanh_(x) : sigmoidf_(x);
            if (p.act == 2) x += c[j];
            c[j] = x;
            cmax = fmaxf(cmax, __builtin_fabsf(x));
        }
    }
    amax_publish_wave(cmax, p.amaxC);                // q == 0: one whole wave (threadIdx.y selects the wave)
}

// How the output tiles become items: whole tiles for the full rounds of the GRID block slots; the remaining r tiles are cut
// into K slices so that they fill the slots once more (at least two K steps per slice), also when r is everything (weight
// gradients: 6 tiles, K = 66 752).  r > GRID / 2 tiles are left whole (a split could not even double the blocks).
struct Plan { int nfull, nsplit, nsl, kslice; };
// K slices for the tiles of a partly filled last round pay a fix-up launch (~6 us) and the slab round trip: only worth it when a whole
// tile's K loop is long
constexpr int g_split_min_ksteps = 4;   // thresholds 12 / 20 / 40 measured equal or slower on the whole update (profiles/r05_gemm.md)
template <int BM, int BN, int GRID>
inline Plan make_plan(int M, int N, int K, int batch) {
    const long nbt = (long)((M + BM - 1) / BM) * ((N + BN - 1) / BN) * batch;
    const int ksteps = (K + BK - 1) / BK;
    Plan pl{(int)nbt, 0, 1, ksteps * BK};
    const int r = (int)(nbt % GRID);
    if (r == 0 || r > GRID / 2 || ksteps < g_split_min_ksteps) return pl;
    int s = std::min(GRID / r, ksteps / 2);
    const int per = (ksteps + s - 1) / s;           // K steps per slice
    s = (ksteps + per - 1) / per;                   // no empty slices
    if (s < 2) return pl;
    pl.nfull = (int)(nbt - r); pl.nsplit = r; pl.nsl = s; pl.kslice = per * BK;
    return pl;
}

// Launch of a kernel that needs more dynamic LDS than the default limit.  The attribute is per device (and the first call may come from
// any thread): `attr_set` is the caller's table of one flag per device id - one table per kernel instantiation - set after the call succeeds.
template <typename K, typename P>
inline int launch_big_lds(K kernel, std::atomic<bool> (&attr_set)[64], dim3 grid, dim3 block, int lds, hipStream_t s, const P& p) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return RESEL_ELAUNCH;
    if (!attr_set[dev].load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return RESEL_ELAUNCH;
        attr_set[dev].store(true, std::memory_order_release);
    }
    launch_timed(RESEL_PROF_GEMM, kernel, grid, block, (size_t)lds, s, p);
    return RESEL_OK;
}

}  // namespace resel
