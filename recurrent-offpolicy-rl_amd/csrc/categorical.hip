// Categorical action head (reference policy_value_models/contextual_sac_discrete_policy.py:106-121): the four steps of
// `process_model_out` - softmax, probability floor, two renormalisations - and their log.  Both forms below take the row arithmetic
// from ONE device function (`row_norm` / `RowNorm::prob`), so they cannot drift apart.
//   step (one policy step): also the mode and one inverse-CDF sample per row, in ONE launch.  One wave64 per row, four rows per
//     256-thread block; lane l owns the actions l, l + 64, ... .  A row is read from global memory only (A <= 64: once, into one
//     register per lane; wider rows are re-read per pass, they stay in cache); the sums are wave reductions, the CDF a wave prefix
//     sum with a carry between 64-wide chunks, and a 64-bit ballot picks the first lane past u.
//   fwd / bwd (whole-row passes of the update, 10^4 .. 10^5 rows of 2 .. 18 actions): a row gets W = the next power of two at or
//     above A lanes (at most 64) and a wave holds 64 / W rows; the reductions are xor-shuffles inside the aligned W-lane group.
//     A > 64 keeps the chunked loop of the step kernel (W = 64).  The backward recomputes softmax and p from the logits.
// No LDS, no atomics, nothing read from the host: capturable.
#include "resel_common.h"

namespace {
using namespace resel;

template <int W>
__device__ __forceinline__ float seg_max(float v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// inclusive prefix sum over the 64 lanes
__device__ __forceinline__ float wave_scan(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// The normalisers of one row: max, sum exp(x - max), sum (softmax + floor), sum of the renormalised row (1 up to rounding).
struct RowNorm {
    float mx, s1, s2, s3, floor_p;
    __device__ __forceinline__ float soft(float x) const { return expf(x - mx) / s1; }
    __device__ __forceinline__ float prob(float x) const { return ((expf(x - mx) / s1 + floor_p) / s2) / s3; }
};

// W lanes share the row x[0 .. A); `lane` in [0, W) owns the entries lane, lane + W, ... .  ONE: A <= W - every loop runs once and the
// row lives in one register per lane.  A = 0 (a group past the last row) reads nothing and only keeps its lanes in the shuffles.
// NaN anywhere in a row makes its first sum NaN and with it every p and logp of the row.
template <int W, bool ONE>
__device__ __forceinline__ RowNorm row_norm(const float* __restrict__ x, int A, int lane, float floor_p) {
    const int nch = ONE ? 1 : (A + W - 1) / W;
    RowNorm r;
    r.floor_p = floor_p;
    float mx = -INFINITY;
    for (int c = 0; c < nch; ++c) {
        const int i = c * W + lane;
        if (i < A) mx = fmaxf(mx, x[i]);
    }
    r.mx = seg_max<W>(mx);
    float s1 = 0.f;                                       // sum exp(x - max)
    for (int c = 0; c < nch; ++c) {
        const int i = c * W + lane;
        if (i < A) s1 += expf(x[i] - r.mx);
    }
    r.s1 = seg_sum<W>(s1);
    float s2 = 0.f;                                       // sum (softmax + floor)
    for (int c = 0; c < nch; ++c) {
        const int i = c * W + lane;
        if (i < A) s2 += expf(x[i] - r.mx) / r.s1 + floor_p;
    }
    r.s2 = seg_sum<W>(s2);
    float s3 = 0.f;                                       // sum of the renormalised row (1 up to rounding)
    for (int c = 0; c < nch; ++c) {
        const int i = c * W + lane;
        if (i < A) s3 += (expf(x[i] - r.mx) / r.s1 + floor_p) / r.s2;
    }
    r.s3 = seg_sum<W>(s3);
    return r;
}

// every lane holds the largest p among its own entries and its lowest index (0x7fffffff: none) -> the row's lowest argmax; no
// comparison with NaN is true, so a NaN row falls back to 0
template <int W>
__device__ __forceinline__ int row_mode(float best, int best_i, int A) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {                 // largest p, lowest index among equals
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(best_i, o, 64);
        if (ov > best || (ov == best && oi < best_i)) { best = ov; best_i = oi; }
    }
    return best_i < A ? best_i : 0;
}

// A NaN row: mode 0 and sample A - 1.
template <bool ONE>
__global__ __launch_bounds__(256) void categorical_step_kernel(const float* __restrict__ logits, int64_t ld_x, const float* __restrict__ u,
                                                               float floor_p, float* __restrict__ logp, int64_t ld_lp,
                                                               float* __restrict__ mode, float* __restrict__ sample, int64_t ld_idx,
                                                               int M, int A) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;                                   // whole waves leave together: the shuffles below see full waves
    const float* x = logits + (int64_t)m * ld_x;
    float* lp = logp + (int64_t)m * ld_lp;
    const int nch = ONE ? 1 : (A + 63) >> 6;
    const RowNorm r = row_norm<64, ONE>(x, A, lane, floor_p);

    const float uu = u[m];
    float best = -1.f, carry = 0.f;
    int best_i = 0x7fffffff, pick = -1;
    for (int c = 0; c < nch; ++c) {
        const int i = c * 64 + lane;
        float p = 0.f;
        if (i < A) {
            p = r.prob(x[i]);
            lp[i] = logf(p);
            if (p > best) { best = p; best_i = i; }      // a lane's indices ascend: strict > keeps its lowest maximum
        }
        const float cdf = carry + wave_scan(p, lane);
        const unsigned long long past = __ballot(i < A && uu < cdf);
        if (pick < 0 && past != 0ull) pick = c * 64 + __ffsll((long long)past) - 1;
        carry = __shfl(cdf, 63, 64);
    }
    const int mi = row_mode<64>(best, best_i, A);
    if (lane == 0) {
        mode[(int64_t)m * ld_idx] = (float)mi;
        sample[(int64_t)m * ld_idx] = (float)(pick >= 0 ? pick : A - 1);
    }
}

// Row m of a dense [M, A] block belongs to lane group (threadIdx.x & 63) / W of wave (blockIdx.x * 4 + threadIdx.x / 64).  Groups past
// the last row run with an empty row: nothing is read or written, their lanes only take part in the shuffles.
template <int W>
__device__ __forceinline__ int64_t packed_row() {
    return ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / W) + ((threadIdx.x & 63) / W);
}

template <int W, bool ONE>
__global__ __launch_bounds__(256) void categorical_fwd_kernel(const float* __restrict__ logits, float floor_p, float* __restrict__ logp,
                                                              float* __restrict__ probs, float* __restrict__ mode, int M, int A) {
    const int lane = threadIdx.x & (W - 1);
    const int64_t m = packed_row<W>();
    const int n = m < M ? A : 0;
    const int64_t row = (m < M ? m : 0) * A;
    const float* x = logits + row;
    const RowNorm r = row_norm<W, ONE>(x, n, lane, floor_p);
    const int nch = ONE ? 1 : (n + W - 1) / W;
    float best = -1.f;
    int best_i = 0x7fffffff;
    for (int c = 0; c < nch; ++c) {
        const int i = c * W + lane;
        if (i < n) {
            const float p = r.prob(x[i]);
            logp[row + i] = logf(p);
            probs[row + i] = p;
            if (p > best) { best = p; best_i = i; }
        }
    }
    const int mi = row_mode<W>(best, best_i, A);
    if (lane == 0 && m < M) mode[m] = (float)mi;
}

// g_i = dprobs_i + dlogp_i / p_i;  dp_i = g_i - sum_j g_j p_j;  ds_i = dp_i / S2;  dx_i = s_i (ds_i - sum_j ds_j s_j)
// (p = t / sum t is invariant to the scale of t = s + floor, so the Jacobian of the second renormalisation collapses into the first
// projection).  A = 1: p = s = 1 exactly, so dp and dx are exactly 0.
template <int W, bool ONE>
__global__ __launch_bounds__(256) void categorical_bwd_kernel(const float* __restrict__ logits, float floor_p, const float* __restrict__ dlogp,
                                                              const float* __restrict__ dprobs, float* __restrict__ dlogits, int M, int A) {
    const int lane = threadIdx.x & (W - 1);
    const int64_t m = packed_row<W>();
    const int n = m < M ? A : 0;
    const int64_t row = (m < M ? m : 0) * A;
    const float* x = logits + row;
    const RowNorm r = row_norm<W, ONE>(x, n, lane, floor_p);
    const int nch = ONE ? 1 : (n + W - 1) / W;
    float t1 = 0.f;                                       // sum g p
    for (int c = 0; c < nch; ++c) {
        const int i = c * W + lane;
        if (i < n) {
            const float p = r.prob(x[i]);
            const float g = (dprobs ? dprobs[row + i] : 0.f) + (dlogp ? dlogp[row + i] / p : 0.f);
            t1 += g * p;
        }
    }
    t1 = seg_sum<W>(t1);
    float t2 = 0.f;                                       // sum ds s
    for (int c = 0; c < nch; ++c) {
        const int i = c * W + lane;
        if (i < n) {
            const float p = r.prob(x[i]);
            const float g = (dprobs ? dprobs[row + i] : 0.f) + (dlogp ? dlogp[row + i] / p : 0.f);
            t2 += ((g - t1) / r.s2) * r.soft(x[i]);
        }
    }
    t2 = seg_sum<W>(t2);
    for (int c = 0; c < nch; ++c) {
        const int i = c * W + lane;
        if (i < n) {
            const float p = r.prob(x[i]);
            const float g = (dprobs ? dprobs[row + i] : 0.f) + (dlogp ? dlogp[row + i] / p : 0.f);
            dlogits[row + i] = r.soft(x[i]) * ((g - t1) / r.s2 - t2);
        }
    }
}

// one launch of KERNEL<W, ONE> over M packed rows: W = row_lanes(A) lanes per row, 4 * (64 / W) rows per 256-thread block
#define RESEL_LAUNCH_PACKED(KERNEL, M, A, stream, ...)                                                                            \
    do {                                                                                                                            \
        const int w_ = row_lanes(A);                                                                                                \
        const int64_t rpb_ = 4 * (64 / w_);                                                                                         \
        const dim3 grid_((unsigned)(((int64_t)(M) + rpb_ - 1) / rpb_)), block_(256);                                               \
        if ((A) > 64) hipLaunchKernelGGL((KERNEL<64, false>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);               \
        else switch (w_) {                                                                                                          \
            case 1: hipLaunchKernelGGL((KERNEL<1, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__); break;            \
            case 2: hipLaunchKernelGGL((KERNEL<2, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__); break;            \
            case 4: hipLaunchKernelGGL((KERNEL<4, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__); break;            \
            case 8: hipLaunchKernelGGL((KERNEL<8, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__); break;            \
            case 16: hipLaunchKernelGGL((KERNEL<16, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__); break;          \
            case 32: hipLaunchKernelGGL((KERNEL<32, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__); break;          \
            default: hipLaunchKernelGGL((KERNEL<64, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__); break;          \
        }                                                                                                                           \
    } while (0)

}  // namespace

extern "C" int resel_categorical_step(const float* logits, int64_t ld_logits, const float* u, float floor, float* logp, int64_t ld_logp,
                                      float* mode, float* sample, int64_t ld_idx, int M, int A, resel_stream_t stream) {
    if (!logits || !u || !logp || !mode || !sample) return RESEL_EINVAL;
    if (A < 1 || A > RESEL_CATEGORICAL_MAX_ACTIONS || M < 0 || ld_logits < A || ld_logp < A || ld_idx < 1) return RESEL_EINVAL;
    if (M == 0) return RESEL_OK;
    const dim3 grid((unsigned)(((int64_t)M + 3) / 4)), block(256);
    if (A <= 64)
        hipLaunchKernelGGL(categorical_step_kernel<true>, grid, block, 0, (hipStream_t)stream, logits, ld_logits, u, floor, logp, ld_logp,
                           mode, sample, ld_idx, M, A);
    else
        hipLaunchKernelGGL(categorical_step_kernel<false>, grid, block, 0, (hipStream_t)stream, logits, ld_logits, u, floor, logp, ld_logp,
                           mode, sample, ld_idx, M, A);
    return launch_status();
}

extern "C" int resel_categorical_fwd(const float* logits, float floor, float* logp, float* probs, float* mode, int M, int A,
                                     resel_stream_t stream) {
    if (!logits || !logp || !probs || !mode) return RESEL_EINVAL;
    if (A < 1 || A > RESEL_CATEGORICAL_MAX_ACTIONS || M < 0) return RESEL_EINVAL;
    if (M == 0) return RESEL_OK;
    RESEL_LAUNCH_PACKED(categorical_fwd_kernel, M, A, stream, logits, floor, logp, probs, mode, M, A);
    return launch_status();
}

extern "C" int resel_categorical_bwd(const float* logits, float floor, const float* dlogp, const float* dprobs, float* dlogits, int M, int A,
                                     resel_stream_t stream) {
    if (!logits || !dlogits || (!dlogp && !dprobs)) return RESEL_EINVAL;
    if (A < 1 || A > RESEL_CATEGORICAL_MAX_ACTIONS || M < 0) return RESEL_EINVAL;
    if (M == 0) return RESEL_OK;
    RESEL_LAUNCH_PACKED(categorical_bwd_kernel, M, A, stream, logits, floor, dlogp, dprobs, dlogits, M, A);
    return launch_status();
}
