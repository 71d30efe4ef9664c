// Packed full-trajectory batch assembled ON THE DEVICE from a device-resident replay ring.
//
// The host keeps the trajectory bookkeeping and the sampling RNG (reference nested_replay_memory.py:103-185 - the numpy
// call order is contractual) and ships only a PLAN: one int4 per sampled trajectory = (batch row, first slot, length
// including the `skip` leading slots, first transition index in the ring).  Three HBM-bound passes then build exactly
// the array the host path builds (bit-exact: it is all copies and flag writes):
//   init     out[r, t, :] = 0, start = 1                      (padding is "start" everywhere)
//   segments slots [pos, pos+skip-1): start = 1; slot pos+skip-1 (PRE-STEP): next_state <- s_0, reward <- r_in0,
//            state <- last_state_0 (column pairs passed by the host), start = 1; slots [pos+skip, pos+n): the transitions,
//            validity column W <- their mask; with a selection bitmap (`sel`, randomised loss masks: the host draws which positions
//            keep their loss mask - reference :165-168 - and ships one bit per data position with the plan) the mask column of a
//            position whose bit is 0 becomes 0, validity keeps the stored mask
//   flags    column W+1 = validity extended one slot earlier, column W+2 = start with the last 1 before data cleared
//            (the target pass's flags, reference sac_full_length_rnn_ensembleQ.py:338-342), done <- 0 where timeout > 0
// One float per thread along the contiguous column axis: every wave access is a fully used row segment.
#include "resel_common.h"

namespace {
using namespace resel;

__global__ void gather_init_kernel(float* __restrict__ out, int64_t ntok, int WO, int c_start) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntok * WO) return;
    out[i] = (int)(i % WO) == c_start ? 1.f : 0.f;
}

// grid = (ceil(maxlen * W / 256), nseg); sel (or null) = [nseg word offsets | bitmap words], sel_words ints in all
__global__ void gather_segments_kernel(const float* __restrict__ buffer, int W, int64_t capacity, const int* __restrict__ seg, int skip,
                                       int rows, int Tp, int c_mask, int c_start, const int* __restrict__ pre_pairs, int npairs,
                                       const int* __restrict__ sel, int sel_words, float* __restrict__ out) {
    const int4 sg = reinterpret_cast<const int4*>(seg)[blockIdx.y];       // row, pos, n, first transition
    // a plan entry that does not fit the output / the ring is dropped (its slots stay padding) instead of written out of bounds
    if (sg.x < 0 || sg.x >= rows || sg.y < 0 || sg.z < skip || (int64_t)sg.y + sg.z > Tp || sg.w < 0 ||
        (int64_t)sg.w + (sg.z - skip) > capacity || (sg.z > skip ? false : sg.w >= capacity)) return;
    const int WO = W + 3;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= sg.z * W) return;
    const int i = e / W, col = e % W;
    float* dst = out + ((int64_t)sg.x * Tp + sg.y + i) * WO;
    if (i >= skip) {
        const float v = buffer[(int64_t)(sg.w + i - skip) * W + col];
        float m = v;
        if (col == c_mask) {
            dst[W] = v;
            if (sel) {
                // a bitmap that would reach outside the words part keeps every mask of its segment instead of reading out of bounds
                const int nseg = (int)gridDim.y, p = i - skip, off = sel[blockIdx.y];
                if (off >= 0 && (int64_t)off + ((sg.z - skip + 31) >> 5) <= (int64_t)sel_words - nseg &&
                    !((sel[nseg + off + (p >> 5)] >> (p & 31)) & 1))
                    m = 0.f;
            }
        }
        dst[col] = m;
    } else if (i == skip - 1) {
        float v = col == c_start ? 1.f : 0.f;
        const float* first = buffer + (int64_t)sg.w * W;
        for (int k = 0; k < npairs; ++k)
            if (pre_pairs[2 * k] == col) v = first[pre_pairs[2 * k + 1]];
        dst[col] = v;
    } else if (col == c_start) {
        dst[col] = 1.f;
    }
}

__global__ void gather_flags_kernel(float* __restrict__ out, int rows, int Tp, int W, int c_start, int c_done, int c_timeout) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * Tp) return;
    const int t = (int)(i % Tp);
    const int WO = W + 3;
    float* p = out + i * WO;
    const float v = p[W], st = p[c_start];
    float tv = v, ts = st;
    if (t + 1 < Tp) {
        if (p[WO + W] - v == 1.f) tv = 1.f;
        if (p[WO + c_start] - st == -1.f) ts = 0.f;
    }
    p[W + 1] = tv;
    p[W + 2] = ts;
    if (c_timeout >= 0 && p[c_timeout] > 0.f) p[c_done] = 0.f;
}

// Transition batches (the memoryless trainers): out[n, :] = buffer[rows[p, n], :].  One wave per batch row, its lanes across the W columns
// (plain 4-byte loads and stores: W is whatever the environment makes it and rows are 4-byte aligned only); a block is four rows.  The
// pass p comes from the device word when there is one, so that one captured launch serves every pass of an update.  A pass outside
// [0, passes) or a row index outside [0, capacity) gives a zero row and reads nothing behind the table.
__global__ __launch_bounds__(256) void gather_transitions_kernel(const float* __restrict__ buffer, int W, int64_t capacity,
                                                                 const int* __restrict__ rows, int passes, int batch, int p_arg,
                                                                 const int* __restrict__ pass_word, int c_done, int c_timeout,
                                                                 float* __restrict__ out) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= batch) return;
    const int p = pass_word ? pass_word[0] : p_arg;
    int64_t r = -1;
    if (p >= 0 && p < passes) r = rows[(int64_t)p * batch + n];
    const bool ok = r >= 0 && r < capacity;
    const float* src = buffer + (ok ? r : 0) * W;
    float* dst = out + (int64_t)n * W;
    const bool timed_out = ok && c_timeout >= 0 && src[c_timeout] > 0.f;      // time-limit terminations bootstrap
    for (int col = lane; col < W; col += 64) {
        float v = ok ? src[col] : 0.f;
        if (col == c_done && timed_out) v = 0.f;
        dst[col] = v;
    }
}

// Slice batches (the slice trainer): out[b, 0, :] = the PRE-STEP row of slice b's first transition (zero but for the column pairs),
// out[b, 1 .. n, :] = ring rows row0 .. row0 + n - 1 with done <- 0 where the row timed out, out[b, n + 1 .. L, :] = 0; (row0, n) =
// plan[p, b].  grid = (batch, ceil((L + 1) W / 256)): one float per thread along the contiguous (slot, column) axis of a slice - the n
// ring rows of a slice are contiguous too, so every wave access is a fully used row segment (plain 4-byte loads and stores: W is whatever
// the environment makes it).  EVERY element of out is written.  The pass p comes from the device word when there is one.  A pass outside
// [0, passes), row0 < 0, n < 1, n > L or row0 + n > capacity gives an all-zero slice and reads nothing of the ring; a pair whose source
// column is outside [0, W) is skipped.
__global__ __launch_bounds__(256) void gather_slices_kernel(const float* __restrict__ buffer, int W, int64_t capacity,
                                                            const int* __restrict__ plan, int passes, int batch, int L, int p_arg,
                                                            const int* __restrict__ pass_word, int c_done, int c_timeout,
                                                            const int* __restrict__ pre_pairs, int npairs, float* __restrict__ out) {
    const int b = blockIdx.x;
    const int e = blockIdx.y * blockDim.x + threadIdx.x;
    if (b >= batch || e >= (L + 1) * W) return;
    const int p = pass_word ? pass_word[0] : p_arg;
    int row0 = -1, n = 0;
    if (p >= 0 && p < passes) {
        const int* entry = plan + ((int64_t)p * batch + b) * 2;
        row0 = entry[0];
        n = entry[1];
    }
    const bool ok = row0 >= 0 && n >= 1 && n <= L && (int64_t)row0 + n <= capacity;
    const int slot = e / W, col = e - slot * W;
    float v = 0.f;
    if (ok && slot == 0) {
        const float* first = buffer + (int64_t)row0 * W;
        for (int k = 0; k < npairs; ++k) {
            const int src = pre_pairs[2 * k + 1];
            if (pre_pairs[2 * k] == col && src >= 0 && src < W) v = first[src];
        }
    } else if (ok && slot <= n) {
        const float* src = buffer + ((int64_t)row0 + slot - 1) * W;
        v = src[col];
        if (col == c_done && c_timeout >= 0 && src[c_timeout] > 0.f) v = 0.f;      // time-limit terminations bootstrap
    }
    out[(int64_t)b * (L + 1) * W + e] = v;
}

}  // namespace

extern "C" int resel_gather_slices(const float* buffer, int W, int64_t capacity, const int* plan, int passes, int batch, int L, int p,
                                   const int* pass_word, int c_done, int c_timeout, const int* pre_pairs, int npairs, float* out,
                                   resel_stream_t stream) {
    if (!buffer || !plan || !out || W <= 0 || capacity <= 0 || passes <= 0 || batch <= 0 || L <= 0) return RESEL_EINVAL;
    if (c_done < 0 || c_done >= W || c_timeout >= W || npairs < 0 || (npairs > 0 && !pre_pairs)) return RESEL_EINVAL;
    if (!pass_word && (p < 0 || p >= passes)) return RESEL_EINVAL;
    const int64_t per_slice = ((int64_t)L + 1) * W, chunks = (per_slice + 255) / 256;
    if (chunks > 65535) return RESEL_EINVAL;          // (grid.y; per_slice then fits an int with room to spare)
    hipLaunchKernelGGL(gather_slices_kernel, dim3((unsigned)batch, (unsigned)chunks), dim3(256), 0, (hipStream_t)stream, buffer, W, capacity,
                       plan, passes, batch, L, p, pass_word, c_done, c_timeout, pre_pairs, npairs, out);
    return launch_status();
}

extern "C" int resel_gather_transitions(const float* buffer, int W, int64_t capacity, const int* rows, int passes, int batch, int p,
                                        const int* pass_word, int c_done, int c_timeout, float* out, resel_stream_t stream) {
    if (!buffer || !rows || !out || W <= 0 || capacity <= 0 || passes <= 0 || batch <= 0) return RESEL_EINVAL;
    if (c_done < 0 || c_done >= W || c_timeout >= W || (!pass_word && (p < 0 || p >= passes))) return RESEL_EINVAL;
    hipLaunchKernelGGL(gather_transitions_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)stream, buffer, W, capacity,
                       rows, passes, batch, p, pass_word, c_done, c_timeout, out);
    return launch_status();
}

extern "C" int resel_gather_trajs_sel(const float* buffer, int W, int64_t capacity, const int* segments, int nseg, int max_len, int skip, int rows,
                                      int Tp, int c_mask, int c_start, int c_done, int c_timeout, const int* pre_pairs, int npairs,
                                      const int* sel, int sel_words, float* out, resel_stream_t stream) {
    if (!buffer || !segments || !out || W <= 0 || capacity <= 0 || nseg <= 0 || max_len <= 0 || skip < 1 || rows <= 0 || Tp <= 0) return RESEL_EINVAL;
    if (c_mask < 0 || c_mask >= W || c_start < 0 || c_start >= W || c_done < 0 || c_done >= W || c_timeout >= W || (npairs > 0 && !pre_pairs))
        return RESEL_EINVAL;
    if (!aligned16(segments) || (sel && sel_words < nseg)) return RESEL_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int WO = W + 3;
    const int64_t ntok = (int64_t)rows * Tp;
    hipLaunchKernelGGL(gather_init_kernel, dim3((unsigned)((ntok * WO + 255) / 256)), dim3(256), 0, s, out, ntok, WO, c_start);
    hipLaunchKernelGGL(gather_segments_kernel, dim3((unsigned)(((int64_t)max_len * W + 255) / 256), nseg), dim3(256), 0, s, buffer, W,
                       capacity, segments, skip, rows, Tp, c_mask, c_start, pre_pairs, npairs, sel, sel_words, out);
    hipLaunchKernelGGL(gather_flags_kernel, dim3((unsigned)((ntok + 255) / 256)), dim3(256), 0, s, out, rows, Tp, W, c_start, c_done,
                       c_timeout);
    return launch_status();
}

extern "C" int resel_gather_trajs(const float* buffer, int W, int64_t capacity, const int* segments, int nseg, int max_len, int skip, int rows, int Tp,
                                  int c_mask, int c_start, int c_done, int c_timeout, const int* pre_pairs, int npairs,
                                  float* out, resel_stream_t stream) {
    return resel_gather_trajs_sel(buffer, W, capacity, segments, nseg, max_len, skip, rows, Tp, c_mask, c_start, c_done, c_timeout, pre_pairs,
                                  npairs, nullptr, 0, out, stream);
}
