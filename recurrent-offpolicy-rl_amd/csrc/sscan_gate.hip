// State groups of the selective scan (d_state > 64, include/resel_hip.h "state groups").  States meet only in <C, h>, so a scan over N states
// is G scans over column groups of (A, B, C) with z == NULL and D == NULL, each on a native kernel, and what the groups share is done here:
//   gate_fwd      out = (sum_g part_g + D u) * silu(z)                                        (max |out| published as the scan forward does)
//   gate_bwd      g = dout * silu(z)  - the `dout` every group's backward takes -,  dz = dout * silu'(z) * (sum_g part_g + D u),
//                 dD[c] = sum_rows g u   (per-wave row partials -> colsum_kernel: fixed order, no atomics; max |dz| published)
//   group_reduce  du = sum_g du_g + D g,  ddelta = sum_g ddelta_g,  ddelta_bias = sum_g ddelta_bias_g   (max |ddelta| published)
// All three are HBM-bound single passes: one float4 per lane, token-major, unit stride on channels, groups summed in index order.
#include "resel_common.h"

namespace {
using namespace resel;

constexpr int GATE_ROWS = 128;       // rows per gate_bwd block: 4 waves x 32 rows, one dD partial row per wave

struct Parts { const float* p[RESEL_SSCAN_MAX_GROUPS]; };

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 c) {
    return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
template <int G>
__device__ __forceinline__ float4 sum_groups(const Parts& q, int64_t off) {
    float4 acc = ld4(q.p[0] + off);
#pragma unroll
    for (int g = 1; g < G; ++g) acc = add4(acc, ld4(q.p[g] + off));
    return acc;
}

// one float4 of one token per lane; every lane of a wave reaches the publish
template <int G>
__global__ __launch_bounds__(256) void sscan_gate_fwd_kernel(Parts parts, const float* __restrict__ u, int64_t ld_u, const float* __restrict__ D,
                                                             const float* __restrict__ z, int64_t ld_z, float* __restrict__ out, int64_t ld_out,
                                                             int64_t M, int Di, AmaxOut amax) {
    const int c4n = Di / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float m = 0.f;
    if (i < M * c4n) {
        const int64_t r = i / c4n;
        const int c = (int)(i % c4n) * 4;
        float4 y = sum_groups<G>(parts, r * Di + c);
        if (D) y = fma4(ld4(D + c), ld4(u + r * ld_u + c), y);
        if (z) {
            const float4 zv = ld4(z + r * ld_z + c);
            y.x *= silu_nb(zv.x); y.y *= silu_nb(zv.y); y.z *= silu_nb(zv.z); y.w *= silu_nb(zv.w);
        }
        st4(out + r * ld_out + c, y);
        m = amax4(0.f, y);
    }
    amax_publish_wave(m, amax);
}

// grid = (column blocks of 256 floats, row blocks of GATE_ROWS); 256 threads = 64 float4 columns x 4 waves, wave w takes rows w, w + 4, ...
template <int G>
__global__ __launch_bounds__(256) void sscan_gate_bwd_kernel(const float* __restrict__ dout, int64_t ld_dout, Parts parts, const float* __restrict__ u,
                                                             int64_t ld_u, const float* __restrict__ D, const float* __restrict__ z, int64_t ld_z,
                                                             float* __restrict__ gout, int64_t ld_g, float* __restrict__ dz, int64_t ld_dz,
                                                             float* __restrict__ dD_part, int64_t M, int Di, AmaxOut amax) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * 4;
    const int64_t r0 = (int64_t)blockIdx.y * GATE_ROWS;
    const int64_t r1 = r0 + GATE_ROWS < M ? r0 + GATE_ROWS : M;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float m = 0.f;
    if (c < Di) {
        const float4 Dv = D ? ld4(D + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t r = r0 + w; r < r1; r += 4) {
            float4 gv = ld4(dout + r * ld_dout + c);
            float4 uv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (D) uv = ld4(u + r * ld_u + c);
            if (z) {
                const float4 zv = ld4(z + r * ld_z + c);
                const float4 y = fma4(Dv, uv, sum_groups<G>(parts, r * Di + c));      // the pre-gate output
                const float4 dzv = make_float4(gv.x * dsiluf_(zv.x) * y.x, gv.y * dsiluf_(zv.y) * y.y, gv.z * dsiluf_(zv.z) * y.z,
                                               gv.w * dsiluf_(zv.w) * y.w);
                st4(dz + r * ld_dz + c, dzv);
                m = amax4(m, dzv);
                gv = make_float4(gv.x * siluf_(zv.x), gv.y * siluf_(zv.y), gv.z * siluf_(zv.z), gv.w * siluf_(zv.w));
                st4(gout + r * ld_g + c, gv);
            }
            acc = fma4(gv, uv, acc);
        }
        if (dD_part) st4(dD_part + ((int64_t)blockIdx.y * 4 + w) * Di + c, acc);
    }
    amax_publish_wave(m, amax);
}

template <int G>
__global__ __launch_bounds__(256) void sscan_group_reduce_kernel(Parts du_parts, Parts dd_parts, const float* __restrict__ db_parts,
                                                                 const float* __restrict__ g, int64_t ld_g, const float* __restrict__ D,
                                                                 float* __restrict__ du, int64_t ld_du, float* __restrict__ ddelta, int64_t ld_dd,
                                                                 float* __restrict__ dbias, int64_t M, int Di, AmaxOut amax) {
    const int c4n = Di / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float m = 0.f;
    if (i < M * c4n) {
        const int64_t r = i / c4n;
        const int c = (int)(i % c4n) * 4;
        float4 a = sum_groups<G>(du_parts, r * Di + c);
        if (D) a = fma4(ld4(D + c), ld4(g + r * ld_g + c), a);                      // the skip term's share: D * (pre-gate gradient)
        st4(du + r * ld_du + c, a);
        const float4 b = sum_groups<G>(dd_parts, r * Di + c);
        st4(ddelta + r * ld_dd + c, b);
        m = amax4(0.f, b);
        if (dbias && r == 0) {
            float4 s = ld4(db_parts + c);
#pragma unroll
            for (int k = 1; k < G; ++k) s = add4(s, ld4(db_parts + (int64_t)k * Di + c));
            st4(dbias + c, s);
        }
    }
    amax_publish_wave(m, amax);
}

inline Parts make_parts(const float* base, int64_t stride_g, int G) {
    Parts q;
    for (int g = 0; g < RESEL_SSCAN_MAX_GROUPS; ++g) q.p[g] = base ? base + (g < G ? g : 0) * stride_g : nullptr;
    return q;
}
inline bool rows_ok(const float* p, int64_t ld, int Di) { return p && aligned16(p) && ld % 4 == 0 && ld >= Di; }
inline bool shape_ok(int64_t M, int Di, int G) { return M > 0 && Di > 0 && Di % 4 == 0 && G >= 1 && G <= RESEL_SSCAN_MAX_GROUPS; }
inline bool parts_ok(const float* p, int64_t stride_g, int64_t M, int Di, int G) {
    return p && aligned16(p) && stride_g % 4 == 0 && (G == 1 || stride_g >= M * Di);
}
inline bool amax_ok(const void* h) { return (reinterpret_cast<uintptr_t>(h) & 7u) == 0; }

#define GROUPS_DISPATCH(G, CALL) do { switch (G) { case 1: { constexpr int GG = 1; CALL; } break; case 2: { constexpr int GG = 2; CALL; } break; \
                                                   case 3: { constexpr int GG = 3; CALL; } break; default: { constexpr int GG = 4; CALL; } break; } } while (0)

}  // namespace

extern "C" int resel_sscan_gate_fwd(const float* parts, int64_t stride_g, int G, const float* u, int64_t ld_u, const float* D,
                                    const float* z, int64_t ld_z, float* out, int64_t ld_out, int64_t M, int Di,
                                    void* amax_out, unsigned amax_epoch, resel_stream_t stream) {
    if (!shape_ok(M, Di, G) || !parts_ok(parts, stride_g, M, Di, G) || !rows_ok(out, ld_out, Di) || !amax_ok(amax_out)) return RESEL_EINVAL;
    if (D && (!aligned16(D) || !rows_ok(u, ld_u, Di))) return RESEL_EINVAL;
    if (z && !rows_ok(z, ld_z, Di)) return RESEL_EINVAL;
    const int64_t n4 = M * (Di / 4);
    const Parts q = make_parts(parts, stride_g, G);
    const AmaxOut ao{(unsigned long long*)amax_out, amax_epoch};
    hipStream_t s = (hipStream_t)stream;
    GROUPS_DISPATCH(G, (launch_timed(RESEL_PROF_SSCAN_GATE_FWD, sscan_gate_fwd_kernel<GG>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                                     q, u, ld_u, D, z, ld_z, out, ld_out, M, Di, ao)));
    return launch_status();
}

extern "C" size_t resel_sscan_gate_bwd_workspace_bytes(int64_t M, int Di) {
    if (M <= 0 || Di <= 0) return 0;
    return (size_t)((M + GATE_ROWS - 1) / GATE_ROWS) * 4 * (size_t)Di * sizeof(float);
}

extern "C" int resel_sscan_gate_bwd(const float* dout, int64_t ld_dout, const float* parts, int64_t stride_g, int G,
                                    const float* u, int64_t ld_u, const float* D, const float* z, int64_t ld_z,
                                    float* g, int64_t ld_g, float* dz, int64_t ld_dz, float* dD, void* workspace, int64_t M, int Di,
                                    void* amax_dz, unsigned amax_epoch, resel_stream_t stream) {
    if (!shape_ok(M, Di, G) || !rows_ok(dout, ld_dout, Di) || !amax_ok(amax_dz)) return RESEL_EINVAL;
    if (!z && !D) return RESEL_EINVAL;                                         // nothing to form: the pre-gate gradient is dout itself
    if ((D != nullptr) != (dD != nullptr) || (z != nullptr) != (dz != nullptr) || (z != nullptr) != (g != nullptr)) return RESEL_EINVAL;
    if (D && (!aligned16(D) || !rows_ok(u, ld_u, Di) || !workspace || !aligned16(workspace))) return RESEL_EINVAL;
    if (z && (!rows_ok(z, ld_z, Di) || !rows_ok(g, ld_g, Di) || !rows_ok(dz, ld_dz, Di) || !parts_ok(parts, stride_g, M, Di, G)))
        return RESEL_EINVAL;
    const Parts q = make_parts(z ? parts : nullptr, stride_g, G);
    const AmaxOut ao{(unsigned long long*)amax_dz, amax_epoch};
    const int64_t nrb = (M + GATE_ROWS - 1) / GATE_ROWS;
    if (nrb > 65535) return RESEL_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((Di / 4 + 63) / 64), (unsigned)nrb);
    float* part = D ? (float*)workspace : nullptr;
    GROUPS_DISPATCH(G, (launch_timed(RESEL_PROF_SSCAN_GATE_BWD, sscan_gate_bwd_kernel<GG>, grid, dim3(256), 0, s,
                                     dout, ld_dout, q, u, ld_u, D, z, ld_z, g, ld_g, dz, ld_dz, part, M, Di, ao)));
    if (D) launch_colsum(part, Di, (int)(nrb * 4), Di, dD, s);
    return launch_status();
}

extern "C" int resel_sscan_group_reduce(const float* du_parts, const float* ddelta_parts, int64_t stride_g, const float* dbias_parts, int G,
                                        const float* g, int64_t ld_g, const float* D, float* du, int64_t ld_du,
                                        float* ddelta, int64_t ld_ddelta, float* dbias, int64_t M, int Di,
                                        void* amax_ddelta, unsigned amax_epoch, resel_stream_t stream) {
    if (!shape_ok(M, Di, G) || !parts_ok(du_parts, stride_g, M, Di, G) || !parts_ok(ddelta_parts, stride_g, M, Di, G)) return RESEL_EINVAL;
    if (!rows_ok(du, ld_du, Di) || !rows_ok(ddelta, ld_ddelta, Di) || !amax_ok(amax_ddelta)) return RESEL_EINVAL;
    if (D && (!aligned16(D) || !rows_ok(g, ld_g, Di))) return RESEL_EINVAL;
    if ((dbias != nullptr) != (dbias_parts != nullptr) || (dbias && (!aligned16(dbias) || !aligned16(dbias_parts)))) return RESEL_EINVAL;
    const int64_t n4 = M * (Di / 4);
    const Parts qu = make_parts(du_parts, stride_g, G), qd = make_parts(ddelta_parts, stride_g, G);
    const AmaxOut ao{(unsigned long long*)amax_ddelta, amax_epoch};
    hipStream_t s = (hipStream_t)stream;
    GROUPS_DISPATCH(G, (launch_timed(RESEL_PROF_SSCAN_GROUP_REDUCE, sscan_group_reduce_kernel<GG>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                                     qu, qd, dbias_parts, g, ld_g, D, du, ld_du, ddelta, ld_ddelta, dbias, M, Di, ao)));
    return launch_status();
}
