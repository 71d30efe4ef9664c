// Packing / unpacking of the tokens of a PADDED sequence description (cgpt under shape-bucketed update graphs,
// algorithm/graphed_update.py `seq_buckets`).  The index table has a bucketed length T; how many of its entries are real is a device
// word (cu_seqlens[Sb] of the padded table), so one recorded launch serves every batch of the bucket:
//     pack:    out[t]  = t < n ? src[idx[t]] : 0                                  (index_select + a zero tail)
//     unpack:  dst[m]  = packed[t] if idx[t] == m for some t < n, else 0          (zeros.index_copy without the memset)
// Both are copy kernels (HBM-bound): float4 accesses, at most 2048 workgroups of 256 threads striding over the rows.  A row is served
// by a group of G = 2^k <= 64 consecutive lanes (G >= C / 4 where that fits a wave), so the row's index - and, in the unpack, the
// binary search for it - is a wave-coalesced read of one address per group and not one per float4.
// The unpack goes over the DESTINATION rows: every row is written exactly once (no memset in front, no write race, the same bits
// on every run); it finds its source by a lower-bound search over the strictly increasing real prefix of idx.
#include "resel_common.h"

namespace {
using namespace resel;

__device__ __forceinline__ int real_count(const int32_t* n_dev, int T) { return min(max(*n_dev, 0), T); }

__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ src, int64_t ld_src, const int64_t* __restrict__ idx,
                                                        const int32_t* __restrict__ n_dev, float* __restrict__ out, int64_t ld_out,
                                                        int T, int C4, int gshift) {
    const int n = real_count(n_dev, T);
    const int G = 1 << gshift, c0 = threadIdx.x & (G - 1);
    const int64_t step = ((int64_t)gridDim.x * blockDim.x) >> gshift;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> gshift; t < T; t += step) {
        float* o = out + t * ld_out;
        if (t < n) {
            const float* s = src + idx[t] * ld_src;
            for (int c = c0; c < C4; c += G) st4(o + 4 * c, ld4(s + 4 * c));
        } else {
            for (int c = c0; c < C4; c += G) st4(o + 4 * c, make_float4(0.f, 0.f, 0.f, 0.f));
        }
    }
}

__global__ __launch_bounds__(256) void unpack_rows_kernel(const float* __restrict__ packed, int64_t ld, const int64_t* __restrict__ idx,
                                                          const int32_t* __restrict__ n_dev, float* __restrict__ dst, int64_t ld_dst,
                                                          int M, int T, int C4, int gshift) {
    const int n = real_count(n_dev, T);
    const int G = 1 << gshift, c0 = threadIdx.x & (G - 1);
    const int64_t step = ((int64_t)gridDim.x * blockDim.x) >> gshift;
    for (int64_t m = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> gshift; m < M; m += step) {
        int lo = 0, hi = n;                                      // lower bound of m in idx[0, n)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (idx[mid] < m) lo = mid + 1; else hi = mid;
        }
        float* o = dst + m * ld_dst;
        if (lo < n && idx[lo] == m) {
            const float* s = packed + (int64_t)lo * ld;
            for (int c = c0; c < C4; c += G) st4(o + 4 * c, ld4(s + 4 * c));
        } else {
            for (int c = c0; c < C4; c += G) st4(o + 4 * c, make_float4(0.f, 0.f, 0.f, 0.f));
        }
    }
}

// Head-width padding of the cgpt attention operands: [rows][hd] bf16 <-> [rows][hdp] bf16 with a zero tail, rows = T * n * H, hd and
// hdp multiples of 8 (a row is a whole number of 16-byte pieces on both sides).  One thread per 16-byte piece of the DESTINATION,
// which is written exactly once; at most 2048 workgroups striding over the pieces.  No device-side count: the token tail of a
// padded problem is zero on the way in (pack_rows) and is written as zero by the attention entries on the way out.
__global__ __launch_bounds__(256) void head_pad_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t rows, int c_src, int c_dst) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = rows * c_dst;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t row = i / c_dst;
        const int c = (int)(i - row * c_dst);
        dst[i] = c < c_src ? src[row * c_src + c] : make_uint4(0u, 0u, 0u, 0u);       // unpad: c_dst < c_src, every piece is a copy
    }
}
inline int head_pad_launch(const void* src, void* dst, int64_t rows, int c_src, int c_dst, resel_stream_t stream) {
    const int64_t blocks = (rows * c_dst + 255) / 256;
    hipLaunchKernelGGL(head_pad_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream,
                       (const uint4*)src, (uint4*)dst, rows, c_src, c_dst);
    return launch_status();
}
inline bool head_pad_ok(const void* a, const void* b, int T, int n, int H, int hd, int hdp) {
    return a && b && aligned16(a) && aligned16(b) && T >= 0 && n > 0 && H > 0 && hd > 0 && (hd & 7) == 0 && hdp >= hd && (hdp & 7) == 0;
}

inline int group_shift(int C4) {                                // smallest 2^k >= C4, at most a wave
    int k = 0;
    while ((1 << k) < C4 && k < 6) ++k;
    return k;
}
inline int grid_for(int64_t rows, int gshift) {
    const int64_t blocks = ((rows << gshift) + 255) / 256;
    return (int)(blocks < 2048 ? blocks : 2048);
}
inline bool rows_ok(const void* p, int64_t ld, int C) { return p && aligned16(p) && ld >= C && (ld & 3) == 0; }

}  // namespace

extern "C" int resel_pack_rows(const float* src, int64_t ld_src, const int64_t* idx, const int32_t* n_dev, float* out, int64_t ld_out,
                               int T, int C, resel_stream_t stream) {
    if (!idx || !n_dev || T < 0 || C <= 0 || (C & 3) || !rows_ok(src, ld_src, C) || !rows_ok(out, ld_out, C)) return RESEL_EINVAL;
    if (T == 0) return RESEL_OK;
    const int gs = group_shift(C / 4);
    hipLaunchKernelGGL(pack_rows_kernel, dim3(grid_for(T, gs)), dim3(256), 0, (hipStream_t)stream, src, ld_src, idx, n_dev, out, ld_out, T, C / 4, gs);
    return launch_status();
}

extern "C" int resel_unpack_rows(const float* packed, int64_t ld, const int64_t* idx, const int32_t* n_dev, float* dst, int64_t ld_dst,
                                 int M, int T, int C, resel_stream_t stream) {
    if (!idx || !n_dev || M < 0 || T < 0 || C <= 0 || (C & 3) || !rows_ok(dst, ld_dst, C) || (T > 0 && !rows_ok(packed, ld, C))) return RESEL_EINVAL;
    if (M == 0) return RESEL_OK;
    const int gs = group_shift(C / 4);
    hipLaunchKernelGGL(unpack_rows_kernel, dim3(grid_for(M, gs)), dim3(256), 0, (hipStream_t)stream, packed, ld, idx, n_dev, dst, ld_dst, M, T, C / 4, gs);
    return launch_status();
}

extern "C" int resel_head_pad(const uint16_t* src, uint16_t* dst, int T, int n, int H, int hd, int hdp, resel_stream_t stream) {
    if (!head_pad_ok(src, dst, T, n, H, hd, hdp)) return RESEL_EINVAL;
    if (T == 0) return RESEL_OK;
    return head_pad_launch(src, dst, (int64_t)T * n * H, hd / 8, hdp / 8, stream);
}

extern "C" int resel_head_unpad(const uint16_t* src, uint16_t* dst, int T, int n, int H, int hd, int hdp, resel_stream_t stream) {
    if (!head_pad_ok(src, dst, T, n, H, hd, hdp)) return RESEL_EINVAL;
    if (T == 0) return RESEL_OK;
    return head_pad_launch(src, dst, (int64_t)T * n * H, hdp / 8, hd / 8, stream);
}
