// LayerNorm over a token's E segments of C floats (the `ln+<act>` / `eln-<E>+<act>` tails of the dense stacks), forward and backward.
//
// A "row" is one token: E segments of C contiguous floats, segment e of token m at  base + m * ld_m + e * ld_e.  One kernel pair so
// serves the token-major [M, E C] output of a shared-input EnsembleLinear (ld_e = C, ld_m = E C), the member-major [E, M, C] output of
// the deeper layers (ld_e = M C, ld_m = C) and, with E = 1, the plain row norm - read and written where the producer / consumer GEMMs
// keep them: no transpose, no densifying copy.  Weight / bias are [E, C] dense: float4 j of the row (j = e C/4 + c) is float4 j of them.
//
// HBM-bound, built like add_layernorm.hip: 16 B per lane per access (a 256-wide segment is one float4 per lane, i.e. 1 KiB per wave
// instruction), the whole token in registers, one pass over memory.  Tokens of up to 512 floats get one wave each, statistics by
// wave-level xor reductions (no LDS).  Wider tokens (the published critic: 8 x 256) get one workgroup each - a wave per token would
// hold 8 float4 of every operand per lane, 256 VGPRs in the backward, one wave per SIMD and nothing to hide a load behind - with the
// four waves' partial sums meeting in LDS.  The mean is taken around the token's first element (mean = x0 + sum(x - x0) / N): a
// constant token gives x - mean == 0 exactly instead of a rounding residue that rstd = eps^-1/2 would amplify.  The backward is
// persistent: it keeps the weight / bias gradients of the tokens it visits in registers and leaves one partial row per workgroup;
// colsum_kernel sums the rows in a fixed order (no atomics, bitwise reproducible).
#include "resel_common.h"

namespace {
using namespace resel;

__device__ __forceinline__ float elu1(float y) { return y > 0.f ? y : expm1f(y); }         // ELU, alpha = 1 (torch's expm1 form)
__device__ __forceinline__ float delu1(float y) { return y > 0.f ? 1.f : expf(y); }         // its derivative from the pre-activation

constexpr int WAVES = 4;            // per block: tokens in flight (wave per token) / parts of one token (workgroup per token)
constexpr int BWD_BLOCKS = 2048;    // persistent backward, wave per token: 8 per CU (two loads in flight per wave at 256 wide: it takes the waves)
constexpr int BWD_BLOCKS_WIDE = 1024;   // ... workgroup per token: 4 per CU, 16 KiB of loads in flight each at 8 x 256
constexpr int WAVE_ROW = 512;       // E * C up to which a token is one wave's
constexpr int MAX_ROW = 2048;       // E * C: 2 float4 per thread of a workgroup

// offset (in floats) of float4 j of a token inside the token: segment j / c4, column 4 (j % c4)
__device__ __forceinline__ int64_t seg_off(int j, int c4, int64_t ld_e) { const int e = j / c4; return (int64_t)e * ld_e + (int64_t)(j - e * c4) * 4; }

template <int VPL>                  // float4 per lane: E * C <= VPL * 256; one wave per token
__global__ __launch_bounds__(WAVES * 64) void mln_fwd_kernel(const float* __restrict__ x, int64_t ldx_e, int64_t ldx_m,
                                                             const float* __restrict__ w, const float* __restrict__ b,
                                                             float* __restrict__ y, int64_t ldy_e, int64_t ldy_m,
                                                             float* __restrict__ stats, int M, int E, int C, float eps, int act, AmaxOut amax,
                                                             const float* __restrict__ res, float* __restrict__ xsum) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (row >= M) return;
    const int c4 = C / 4, n4 = E * c4;
    const float inv_n = 1.f / (float)(E * C);
    const float* xr = x + (int64_t)row * ldx_m;
    float* yr = y + (int64_t)row * ldy_m;
    // residual form (res != nullptr): the token normalised is x + res, both in x's layout; the sum is left in xsum (same layout) for the backward
    const float* rr = res ? res + (int64_t)row * ldx_m : nullptr;
    float* sr = res ? xsum + (int64_t)row * ldx_m : nullptr;
    const float x0 = rr ? xr[0] + rr[0] : xr[0];        // wave-uniform: the shift of the mean
    float4 v[VPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int j = i * 64 + lane;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < n4) {
            float4 t = ld4(xr + seg_off(j, c4, ldx_e));
            if (rr) {
                const float4 r = ld4(rr + seg_off(j, c4, ldx_e));
                t.x += r.x; t.y += r.y; t.z += r.z; t.w += r.w;
                st4(sr + seg_off(j, c4, ldx_e), t);
            }
            v[i] = make_float4(t.x - x0, t.y - x0, t.z - x0, t.w - x0);
        }
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float dm = wave_sum(s) * inv_n;               // mean - x0
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int j = i * 64 + lane;
        if (j < n4) {
            v[i].x -= dm; v[i].y -= dm; v[i].z -= dm; v[i].w -= dm;
            q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
        }
    }
    const float rstd = rsqrtf(wave_sum(q) * inv_n + eps);
    if (lane == 0) { stats[2 * (int64_t)row] = x0 + dm; stats[2 * (int64_t)row + 1] = rstd; }
    float wmax = 0.f, bmax = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int j = i * 64 + lane;
        if (j < n4) {
            const float4 wv = reinterpret_cast<const float4*>(w)[j];
            float4 o;
            o.x = v[i].x * rstd * wv.x; o.y = v[i].y * rstd * wv.y; o.z = v[i].z * rstd * wv.z; o.w = v[i].w * rstd * wv.w;
            if (b) {
                const float4 bb = reinterpret_cast<const float4*>(b)[j];
                o.x += bb.x; o.y += bb.y; o.z += bb.z; o.w += bb.w;
                bmax = amax4(bmax, bb);
            }
            if (act) { o.x = elu1(o.x); o.y = elu1(o.y); o.z = elu1(o.z); o.w = elu1(o.w); }      // |elu(y)| <= |y|: the bound below still holds
            st4(yr + seg_off(j, c4, ldy_e), o);
            wmax = amax4(wmax, wv);
        }
    }
    // Magnitude of the output for the GEMM that reads it (mode 2), as resel_add_layernorm_fwd publishes it: a normalised token obeys
    // |x_i - mean| * rstd <= sqrt(E C), so sqrt(E C) max|w| + max|b| bounds every |y| - no per-token work, ONE wave publishes it.
    if (amax.slot != nullptr && row == 0) {
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) { wmax = fmaxf(wmax, __shfl_xor(wmax, sh, 64)); bmax = fmaxf(bmax, __shfl_xor(bmax, sh, 64)); }
        amax_publish_wave(sqrtf((float)(E * C)) * wmax + bmax, amax);
    }
}

template <int VPL, bool ACT>          // ACT: the forward stored elu(y) (a compile-time switch, as in add_layernorm.hip)
__global__ __launch_bounds__(WAVES * 64) void mln_bwd_kernel(const float* __restrict__ dy, int64_t ldg_e, int64_t ldg_m,
                                                             const float* __restrict__ x, int64_t ldx_e, int64_t ldx_m,
                                                             const float* __restrict__ w, const float* __restrict__ b,
                                                             const float* __restrict__ stats, float* __restrict__ dx, int64_t ldd_e, int64_t ldd_m,
                                                             float* __restrict__ dw_part, float* __restrict__ db_part,
                                                             int M, int E, int C, AmaxOut amax) {
    __shared__ __attribute__((aligned(16))) float s_acc[2][WAVES][VPL * 256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c4 = C / 4, n4 = E * c4, N = E * C;
    const float inv_n = 1.f / (float)N;
    float4 dwa[VPL], dba[VPL], wreg[VPL], breg[ACT ? VPL : 1];
    int ox[VPL], og[VPL], od[VPL];                      // per-lane offsets inside a token (the entry checks that a token spans < 2^31 floats): formed once, the waves are persistent
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        dwa[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        dba[i] = dwa[i];
        const int j = i * 64 + lane;
        const bool in = j < n4;
        wreg[i] = in ? reinterpret_cast<const float4*>(w)[j] : dwa[i];
        if constexpr (ACT) breg[i] = (b && in) ? reinterpret_cast<const float4*>(b)[j] : dwa[i];
        ox[i] = in ? (int)seg_off(j, c4, ldx_e) : 0;
        og[i] = in ? (int)seg_off(j, c4, ldg_e) : 0;
        od[i] = in ? (int)seg_off(j, c4, ldd_e) : 0;
    }
    float dxmax = 0.f;
    for (int row = blockIdx.x * WAVES + wv; row < M; row += gridDim.x * WAVES) {
        const float mean = stats[2 * (int64_t)row], rstd = stats[2 * (int64_t)row + 1];
        const float* xr = x + (int64_t)row * ldx_m;
        const float* gr = dy + (int64_t)row * ldg_m;
        float* dr = dx + (int64_t)row * ldd_m;
        float4 xh[VPL], g[VPL];
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            xh[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            g[i] = xh[i];
            if (i * 64 + lane < n4) {
                const float4 r = ld4(xr + ox[i]);
                float4 d = ld4(gr + og[i]);
                xh[i].x = (r.x - mean) * rstd; xh[i].y = (r.y - mean) * rstd; xh[i].z = (r.z - mean) * rstd; xh[i].w = (r.w - mean) * rstd;
                if constexpr (ACT) {          // the forward stored elu(y), y = xh w + b: its derivative from the recomputed y (1 for y > 0, e^y below)
                    d.x *= delu1(xh[i].x * wreg[i].x + breg[i].x); d.y *= delu1(xh[i].y * wreg[i].y + breg[i].y);
                    d.z *= delu1(xh[i].z * wreg[i].z + breg[i].z); d.w *= delu1(xh[i].w * wreg[i].w + breg[i].w);
                }
                dwa[i].x += d.x * xh[i].x; dwa[i].y += d.y * xh[i].y; dwa[i].z += d.z * xh[i].z; dwa[i].w += d.w * xh[i].w;
                dba[i].x += d.x; dba[i].y += d.y; dba[i].z += d.z; dba[i].w += d.w;
                g[i].x = d.x * wreg[i].x; g[i].y = d.y * wreg[i].y; g[i].z = d.z * wreg[i].z; g[i].w = d.w * wreg[i].w;
                c1 += (g[i].x * xh[i].x + g[i].y * xh[i].y) + (g[i].z * xh[i].z + g[i].w * xh[i].w);
                c2 += (g[i].x + g[i].y) + (g[i].z + g[i].w);
            }
        }
        c1 = wave_sum(c1) * inv_n;
        c2 = wave_sum(c2) * inv_n;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            if (i * 64 + lane < n4) {
                float4 o;
                o.x = (g[i].x - (xh[i].x * c1 + c2)) * rstd; o.y = (g[i].y - (xh[i].y * c1 + c2)) * rstd;
                o.z = (g[i].z - (xh[i].z * c1 + c2)) * rstd; o.w = (g[i].w - (xh[i].w * c1 + c2)) * rstd;
                st4(dr + od[i], o);
                dxmax = amax4(dxmax, o);
            }
        }
    }
    amax_publish_wave(dxmax, amax);                  // persistent waves: one publication each (dx feeds the gradient GEMMs of the layer in front)
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        st4(&s_acc[0][wv][(i * 64 + lane) * 4], dwa[i]);
        st4(&s_acc[1][wv][(i * 64 + lane) * 4], dba[i]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < N; c += WAVES * 64) {
        float a = 0.f, bq = 0.f;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) { a += s_acc[0][k][c]; bq += s_acc[1][k][c]; }
        dw_part[(int64_t)blockIdx.x * N + c] = a;
        db_part[(int64_t)blockIdx.x * N + c] = bq;
    }
}

// sum over the workgroup of a value that is already summed over each wave: lane 0 of every wave leaves it in `slot`, one barrier
__device__ __forceinline__ float block_sum(float wave_total, float* slot, int lane, int wv) {
    if (lane == 0) slot[wv] = wave_total;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

template <int VW>                   // float4 per thread: E * C <= VW * 1024; one workgroup per token
__global__ __launch_bounds__(WAVES * 64) void mln_fwd_wide_kernel(const float* __restrict__ x, int64_t ldx_e, int64_t ldx_m,
                                                                  const float* __restrict__ w, const float* __restrict__ b,
                                                                  float* __restrict__ y, int64_t ldy_e, int64_t ldy_m,
                                                                  float* __restrict__ stats, int M, int E, int C, float eps, int act, AmaxOut amax,
                                                                  const float* __restrict__ res, float* __restrict__ xsum) {
    __shared__ float s_red[4][WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row = blockIdx.x;                         // grid = M
    const int c4 = C / 4, n4 = E * c4;
    const float inv_n = 1.f / (float)(E * C);
    const float* xr = x + (int64_t)row * ldx_m;
    float* yr = y + (int64_t)row * ldy_m;
    const float* rr = res ? res + (int64_t)row * ldx_m : nullptr;      // residual form, see mln_fwd_kernel
    float* sr = res ? xsum + (int64_t)row * ldx_m : nullptr;
    const float x0 = rr ? xr[0] + rr[0] : xr[0];
    float4 v[VW];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VW; ++i) {
        const int j = i * (WAVES * 64) + tid;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < n4) {
            float4 t = ld4(xr + seg_off(j, c4, ldx_e));
            if (rr) {
                const float4 r = ld4(rr + seg_off(j, c4, ldx_e));
                t.x += r.x; t.y += r.y; t.z += r.z; t.w += r.w;
                st4(sr + seg_off(j, c4, ldx_e), t);
            }
            v[i] = make_float4(t.x - x0, t.y - x0, t.z - x0, t.w - x0);
        }
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float dm = block_sum(wave_sum(s), s_red[0], lane, wv) * inv_n;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VW; ++i) {
        if (i * (WAVES * 64) + tid < n4) {
            v[i].x -= dm; v[i].y -= dm; v[i].z -= dm; v[i].w -= dm;
            q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
        }
    }
    const float rstd = rsqrtf(block_sum(wave_sum(q), s_red[1], lane, wv) * inv_n + eps);
    if (tid == 0) { stats[2 * (int64_t)row] = x0 + dm; stats[2 * (int64_t)row + 1] = rstd; }
    float wmax = 0.f, bmax = 0.f;
#pragma unroll
    for (int i = 0; i < VW; ++i) {
        const int j = i * (WAVES * 64) + tid;
        if (j < n4) {
            const float4 wq = reinterpret_cast<const float4*>(w)[j];
            float4 o;
            o.x = v[i].x * rstd * wq.x; o.y = v[i].y * rstd * wq.y; o.z = v[i].z * rstd * wq.z; o.w = v[i].w * rstd * wq.w;
            if (b) {
                const float4 bb = reinterpret_cast<const float4*>(b)[j];
                o.x += bb.x; o.y += bb.y; o.z += bb.z; o.w += bb.w;
                bmax = amax4(bmax, bb);
            }
            if (act) { o.x = elu1(o.x); o.y = elu1(o.y); o.z = elu1(o.z); o.w = elu1(o.w); }
            st4(yr + seg_off(j, c4, ldy_e), o);
            wmax = amax4(wmax, wq);
        }
    }
    if (amax.slot != nullptr && row == 0) {             // the bound of mln_fwd_kernel, from the maxima over all four waves (block-uniform branch)
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) { wmax = fmaxf(wmax, __shfl_xor(wmax, sh, 64)); bmax = fmaxf(bmax, __shfl_xor(bmax, sh, 64)); }
        if (lane == 0) { s_red[2][wv] = wmax; s_red[3][wv] = bmax; }
        __syncthreads();
        if (wv == 0) {
            wmax = fmaxf(fmaxf(s_red[2][0], s_red[2][1]), fmaxf(s_red[2][2], s_red[2][3]));
            bmax = fmaxf(fmaxf(s_red[3][0], s_red[3][1]), fmaxf(s_red[3][2], s_red[3][3]));
            amax_publish_wave(sqrtf((float)(E * C)) * wmax + bmax, amax);
        }
    }
}

// persistent workgroups, one token at a time: every thread owns VW float4 columns of the token for the whole launch, so the weight /
// bias gradients it accumulates go straight to its block's partial row (no LDS pass at the end)
template <int VW, bool ACT>
__global__ __launch_bounds__(WAVES * 64) void mln_bwd_wide_kernel(const float* __restrict__ dy, int64_t ldg_e, int64_t ldg_m,
                                                                  const float* __restrict__ x, int64_t ldx_e, int64_t ldx_m,
                                                                  const float* __restrict__ w, const float* __restrict__ b,
                                                                  const float* __restrict__ stats, float* __restrict__ dx, int64_t ldd_e, int64_t ldd_m,
                                                                  float* __restrict__ dw_part, float* __restrict__ db_part,
                                                                  int M, int E, int C, AmaxOut amax) {
    __shared__ float s_red[2][2][WAVES];                // [token parity][c1 | c2][wave]: one barrier per token
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c4 = C / 4, n4 = E * c4, N = E * C;
    const float inv_n = 1.f / (float)N;
    float4 dwa[VW], dba[VW], wreg[VW], breg[ACT ? VW : 1];
    int ox[VW], og[VW], od[VW];
#pragma unroll
    for (int i = 0; i < VW; ++i) {
        dwa[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        dba[i] = dwa[i];
        const int j = i * (WAVES * 64) + tid;
        const bool in = j < n4;
        wreg[i] = in ? reinterpret_cast<const float4*>(w)[j] : dwa[i];
        if constexpr (ACT) breg[i] = (b && in) ? reinterpret_cast<const float4*>(b)[j] : dwa[i];
        ox[i] = in ? (int)seg_off(j, c4, ldx_e) : 0;
        og[i] = in ? (int)seg_off(j, c4, ldg_e) : 0;
        od[i] = in ? (int)seg_off(j, c4, ldd_e) : 0;
    }
    float dxmax = 0.f;
    int par = 0;
    for (int row = blockIdx.x; row < M; row += gridDim.x, par ^= 1) {       // block-uniform trip count: the barrier below is reached by all
        const float mean = stats[2 * (int64_t)row], rstd = stats[2 * (int64_t)row + 1];
        const float* xr = x + (int64_t)row * ldx_m;
        const float* gr = dy + (int64_t)row * ldg_m;
        float* dr = dx + (int64_t)row * ldd_m;
        float4 xh[VW], g[VW];
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int i = 0; i < VW; ++i) {
            xh[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            g[i] = xh[i];
            if (i * (WAVES * 64) + tid < n4) {
                const float4 r = ld4(xr + ox[i]);
                float4 d = ld4(gr + og[i]);
                xh[i].x = (r.x - mean) * rstd; xh[i].y = (r.y - mean) * rstd; xh[i].z = (r.z - mean) * rstd; xh[i].w = (r.w - mean) * rstd;
                if constexpr (ACT) {
                    d.x *= delu1(xh[i].x * wreg[i].x + breg[i].x); d.y *= delu1(xh[i].y * wreg[i].y + breg[i].y);
                    d.z *= delu1(xh[i].z * wreg[i].z + breg[i].z); d.w *= delu1(xh[i].w * wreg[i].w + breg[i].w);
                }
                dwa[i].x += d.x * xh[i].x; dwa[i].y += d.y * xh[i].y; dwa[i].z += d.z * xh[i].z; dwa[i].w += d.w * xh[i].w;
                dba[i].x += d.x; dba[i].y += d.y; dba[i].z += d.z; dba[i].w += d.w;
                g[i].x = d.x * wreg[i].x; g[i].y = d.y * wreg[i].y; g[i].z = d.z * wreg[i].z; g[i].w = d.w * wreg[i].w;
                c1 += (g[i].x * xh[i].x + g[i].y * xh[i].y) + (g[i].z * xh[i].z + g[i].w * xh[i].w);
                c2 += (g[i].x + g[i].y) + (g[i].z + g[i].w);
            }
        }
        c1 = wave_sum(c1);
        c2 = wave_sum(c2);
        // the slots of this parity were last read two tokens ago, in front of the barrier of the token in between
        if (lane == 0) { s_red[par][0][wv] = c1; s_red[par][1][wv] = c2; }
        __syncthreads();
        c1 = ((s_red[par][0][0] + s_red[par][0][1]) + (s_red[par][0][2] + s_red[par][0][3])) * inv_n;
        c2 = ((s_red[par][1][0] + s_red[par][1][1]) + (s_red[par][1][2] + s_red[par][1][3])) * inv_n;
#pragma unroll
        for (int i = 0; i < VW; ++i) {
            if (i * (WAVES * 64) + tid < n4) {
                float4 o;
                o.x = (g[i].x - (xh[i].x * c1 + c2)) * rstd; o.y = (g[i].y - (xh[i].y * c1 + c2)) * rstd;
                o.z = (g[i].z - (xh[i].z * c1 + c2)) * rstd; o.w = (g[i].w - (xh[i].w * c1 + c2)) * rstd;
                st4(dr + od[i], o);
                dxmax = amax4(dxmax, o);
            }
        }
    }
    amax_publish_wave(dxmax, amax);
#pragma unroll
    for (int i = 0; i < VW; ++i) {
        const int j = i * (WAVES * 64) + tid;
        if (j < n4) {
            st4(dw_part + (int64_t)blockIdx.x * N + 4 * j, dwa[i]);
            st4(db_part + (int64_t)blockIdx.x * N + 4 * j, dba[i]);
        }
    }
}

inline bool wide(int E, int C) { return E * C > WAVE_ROW; }
inline int bwd_blocks(int M, int E, int C) {
    if (wide(E, C)) return M < BWD_BLOCKS_WIDE ? M : BWD_BLOCKS_WIDE;
    const int need = (M + WAVES - 1) / WAVES;
    return need < BWD_BLOCKS ? need : BWD_BLOCKS;
}
inline bool shape_ok(int M, int E, int C) { return M > 0 && E > 0 && C > 0 && C % 4 == 0 && (int64_t)E * C <= MAX_ROW; }
// a (segment, token) stride pair the kernels can address with 16-byte accesses (the segment stride of a single segment is never used)
inline bool ld_ok(int64_t ld_e, int64_t ld_m, int E, int M) {
    return (E == 1 || (ld_e > 0 && ld_e % 4 == 0 && ld_e < ((int64_t)1 << 31) / E)) && (M == 1 || (ld_m > 0 && ld_m % 4 == 0));
}

}  // namespace

static int mln_fwd_run(const float* x, const float* res, float* xsum, int64_t ldx_e, int64_t ldx_m, const float* w, const float* b,
                       float* y, int64_t ldy_e, int64_t ldy_m, float* stats, int M, int E, int C, float eps, int act,
                       void* amax_y, unsigned amax_epoch, resel_stream_t stream) {
    if (!x || !w || !y || !stats || !shape_ok(M, E, C) || (act != 0 && act != 1) || (reinterpret_cast<uintptr_t>(amax_y) & 7u)) return RESEL_EINVAL;
    if (!ld_ok(ldx_e, ldx_m, E, M) || !ld_ok(ldy_e, ldy_m, E, M)) return RESEL_EINVAL;
    if (!aligned16(x) || !aligned16(y) || !aligned16(w) || (b && !aligned16(b))) return RESEL_EINVAL;
    const AmaxOut ao{(unsigned long long*)amax_y, amax_epoch};
    hipStream_t s = (hipStream_t)stream;
    const int N = E * C;
    dim3 grid(wide(E, C) ? M : (M + WAVES - 1) / WAVES), blk(WAVES * 64);
#define MLN_FWD(K) hipLaunchKernelGGL(K, grid, blk, 0, s, x, ldx_e, ldx_m, w, b, y, ldy_e, ldy_m, stats, M, E, C, eps, act, ao, res, xsum)
    if (N <= 256) MLN_FWD(mln_fwd_kernel<1>);
    else if (N <= WAVE_ROW) MLN_FWD(mln_fwd_kernel<2>);
    else if (N <= 1024) MLN_FWD(mln_fwd_wide_kernel<1>);
    else MLN_FWD(mln_fwd_wide_kernel<2>);
#undef MLN_FWD
    return launch_status();
}

extern "C" int resel_member_layernorm_fwd(const float* x, int64_t ldx_e, int64_t ldx_m, const float* w, const float* b,
                                          float* y, int64_t ldy_e, int64_t ldy_m, float* stats, int M, int E, int C, float eps, int act,
                                          void* amax_y, unsigned amax_epoch, resel_stream_t stream) {
    return mln_fwd_run(x, nullptr, nullptr, ldx_e, ldx_m, w, b, y, ldy_e, ldy_m, stats, M, E, C, eps, act, amax_y, amax_epoch, stream);
}

// y = act(LN_[E, C](x + res)), xsum = x + res: the closing residual add + joint member LayerNorm of the ensemble feed-forward block
// (elru-<E>) in one pass.  x, res, xsum share one stride pair.  The backward is resel_member_layernorm_bwd on xsum: its dx is the
// gradient of both addends.
extern "C" int resel_member_add_layernorm_fwd(const float* x, const float* res, float* xsum, int64_t ldx_e, int64_t ldx_m,
                                              const float* w, const float* b, float* y, int64_t ldy_e, int64_t ldy_m, float* stats,
                                              int M, int E, int C, float eps, int act, void* amax_y, unsigned amax_epoch,
                                              resel_stream_t stream) {
    if (!res || !xsum || !aligned16(res) || !aligned16(xsum)) return RESEL_EINVAL;
    return mln_fwd_run(x, res, xsum, ldx_e, ldx_m, w, b, y, ldy_e, ldy_m, stats, M, E, C, eps, act, amax_y, amax_epoch, stream);
}

extern "C" size_t resel_member_layernorm_bwd_workspace_bytes(int M, int E, int C) {
    if (!shape_ok(M, E, C)) return 0;
    return (size_t)2 * bwd_blocks(M, E, C) * E * C * sizeof(float);
}

extern "C" int resel_member_layernorm_bwd(const float* dy, int64_t ldg_e, int64_t ldg_m, const float* x, int64_t ldx_e, int64_t ldx_m,
                                          const float* w, const float* b, const float* stats, float* dx, int64_t ldd_e, int64_t ldd_m,
                                          float* dw, float* db, void* workspace, int M, int E, int C, int act,
                                          void* amax_dx, unsigned amax_epoch, resel_stream_t stream) {
    if (!dy || !x || !w || !stats || !dx || !dw || !workspace || !shape_ok(M, E, C) || (reinterpret_cast<uintptr_t>(amax_dx) & 7u)) return RESEL_EINVAL;
    if ((act != 0 && act != 1) || (b && !aligned16(b)) || (db && !b)) return RESEL_EINVAL;
    if (!ld_ok(ldg_e, ldg_m, E, M) || !ld_ok(ldx_e, ldx_m, E, M) || !ld_ok(ldd_e, ldd_m, E, M)) return RESEL_EINVAL;
    if (!aligned16(dy) || !aligned16(x) || !aligned16(w) || !aligned16(dx) || !aligned16(workspace)) return RESEL_EINVAL;
    const AmaxOut ao{(unsigned long long*)amax_dx, amax_epoch};
    hipStream_t s = (hipStream_t)stream;
    const int N = E * C, nblk = bwd_blocks(M, E, C);
    float* dw_part = (float*)workspace;
    float* db_part = dw_part + (size_t)nblk * N;
#define MLN_BWD(K, V) do { if (act) hipLaunchKernelGGL((K<V, true>), grid, blk, 0, s, dy, ldg_e, ldg_m, x, ldx_e, ldx_m, w, b, stats, dx, ldd_e, ldd_m, dw_part, db_part, M, E, C, ao); \
                           else hipLaunchKernelGGL((K<V, false>), grid, blk, 0, s, dy, ldg_e, ldg_m, x, ldx_e, ldx_m, w, b, stats, dx, ldd_e, ldd_m, dw_part, db_part, M, E, C, ao); } while (0)
    dim3 grid(nblk), blk(WAVES * 64);
    if (N <= 256) MLN_BWD(mln_bwd_kernel, 1);
    else if (N <= WAVE_ROW) MLN_BWD(mln_bwd_kernel, 2);
    else if (N <= 1024) MLN_BWD(mln_bwd_wide_kernel, 1);
    else MLN_BWD(mln_bwd_wide_kernel, 2);
#undef MLN_BWD
    launch_colsum(dw_part, N, nblk, N, dw, s);
    if (db) launch_colsum(db_part, N, nblk, N, db, s);
    return launch_status();
}
