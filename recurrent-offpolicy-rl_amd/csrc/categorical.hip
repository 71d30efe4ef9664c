// Categorical action head of one policy step (reference policy_value_models/contextual_sac_discrete_policy.py:106-121): the four steps
// of `process_model_out` - softmax, probability floor, two renormalisations - their log, the mode and one inverse-CDF sample per
// row, in ONE launch.  One wave64 per row, four rows per 256-thread block; lane l owns the actions l, l + 64, ... .  A row is read
// from global memory only (A <= 64: once, into one register per lane; wider rows are re-read per pass, they stay in cache); the
// sums are wave reductions, the CDF a wave prefix sum with a carry between 64-wide chunks, and a 64-bit ballot picks the first lane
// past u.  No LDS, no atomics, nothing read from the host: capturable.
#include "resel_common.h"

namespace {
using namespace resel;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
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

// ONE: A <= 64 - every loop below runs once and the row lives in one register per lane.
// NaN anywhere in a row makes its first sum NaN and with it every p and logp of the row; no comparison with NaN is true, so the
// mode falls back to 0 and the sample to A - 1.
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

    float mx = -INFINITY;
    for (int c = 0; c < nch; ++c) {
        const int i = c * 64 + lane;
        if (i < A) mx = fmaxf(mx, x[i]);
    }
    mx = wave_max(mx);
    float s1 = 0.f;                                       // sum exp(x - max)
    for (int c = 0; c < nch; ++c) {
        const int i = c * 64 + lane;
        if (i < A) s1 += expf(x[i] - mx);
    }
    s1 = wave_sum(s1);
    float s2 = 0.f;                                       // sum (softmax + floor)
    for (int c = 0; c < nch; ++c) {
        const int i = c * 64 + lane;
        if (i < A) s2 += expf(x[i] - mx) / s1 + floor_p;
    }
    s2 = wave_sum(s2);
    float s3 = 0.f;                                       // sum of the renormalised row (1 up to rounding)
    for (int c = 0; c < nch; ++c) {
        const int i = c * 64 + lane;
        if (i < A) s3 += (expf(x[i] - mx) / s1 + floor_p) / s2;
    }
    s3 = wave_sum(s3);

    const float uu = u[m];
    float best = -1.f, carry = 0.f;
    int best_i = 0x7fffffff, pick = -1;
    for (int c = 0; c < nch; ++c) {
        const int i = c * 64 + lane;
        float p = 0.f;
        if (i < A) {
            p = ((expf(x[i] - mx) / s1 + floor_p) / s2) / s3;
            lp[i] = logf(p);
            if (p > best) { best = p; best_i = i; }      // a lane's indices ascend: strict > keeps its lowest maximum
        }
        const float cdf = carry + wave_scan(p, lane);
        const unsigned long long past = __ballot(i < A && uu < cdf);
        if (pick < 0 && past != 0ull) pick = c * 64 + __ffsll((long long)past) - 1;
        carry = __shfl(cdf, 63, 64);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                    // largest p, lowest index among equals
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(best_i, o, 64);
        if (ov > best || (ov == best && oi < best_i)) { best = ov; best_i = oi; }
    }
    if (lane == 0) {
        mode[(int64_t)m * ld_idx] = (float)(best_i < A ? best_i : 0);
        sample[(int64_t)m * ld_idx] = (float)(pick >= 0 ? pick : A - 1);
    }
}

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
