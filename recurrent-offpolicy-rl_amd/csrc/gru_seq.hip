// GRU recurrence on a hoisted input projection (gi = x W_ih^T + b_ih), forward and backward.
//
// The recurrence is T-sequential and each step needs every hidden unit of the previous step.  Two drivers share the same
// per-step arithmetic: (a) the PERSISTENT kernels further down - one launch per pass, the 16 unit-slice workgroups of a row
// group hand h_t (backward: the carry) to each other through tagged 8-byte granules, 3.0 / 3.9 us per step forward /
// backward and no per-step host work - used whenever the whole grid is co-resident (<= 256 workgroups); (b) one small
// launch per step enqueued back-to-back from C (a dependent kernel boundary, ~1.5 us, is cheaper than a full software
// grid barrier, 4-7 us, MI355X_MICROARCH "barrier-xcd"), 4.4 / 6.8 us per step, for larger grids.  Either way the
// LATENCY of one step is what matters, so the step is spread over the whole chip and keeps its operands close:
//   grid = (H/16 hidden-unit slices) x (B/4 row groups)  [16 x 16 = 256 workgroups at H = 256, B = 64: one per CU];
//   thread (j, kq) of a workgroup owns output unit j of the slice and the kq-th 1/16 of the reduction axis, and holds
//   that piece of W_hh for all three gates IN REGISTERS (3H/16 <= 192 floats, fetched with fully coalesced float4 loads
//   from a copy laid out once per call as [slice][float4 chunk][thread]); the 4 rows of h_{t-1} (forward) / of the gate
//   gradients (backward) sit in LDS and are read as broadcast float4s; the 16 partial sums of an output meet in LDS.
// A third entry, resel_gru_multi_fwd, runs up to four INDEPENDENT recurrences of equal shape through the same two drivers in one launch
// (network = outermost grid index; residency rule of its own, see multi_resident_cap): the trainer's concurrent embedding passes share the
// chip without a stream each, so that the update is a single-stream launch sequence.  The step bodies are device functions shared by the
// single- and multi-network kernels.  The backward has no multi form (the backward recurrences of an update sit in different optimizer steps).
// All arithmetic is exact fp32 FMA (parity target 1e-4 against ATen's CPU GRU).  [First version: 64 workgroups with
// the W slice and 16 rows in LDS, every thread a full-length dot product - LDS-read bound at 9 us (fwd) / 23 us (bwd)
// per step.]  Neither roofline is tight for this layer; the reported figure is the achieved step rate.
#include "resel_common.h"
#include <cstdlib>
#include <type_traits>

namespace {
using namespace resel;

// gate non-linearities on v_exp_f32 / v_rcp_f32 (1 ulp each: 2e-7 on a gate, parity bar 1e-4).  They sit on the serial chain of
// every step - 64 threads, everyone else waiting at a barrier - where libm's expf / tanhf cost ~0.25 us of a 3.4 us step.
__device__ __forceinline__ float gru_tanh(float x) {
    const float e = fast_exp(-2.0f * fabsf(x));                 // tanh|x| = (1 - e) / (1 + e)
    return copysignf((1.0f - e) * fast_rcp(1.0f + e), x);
}

constexpr int US = 16;    // hidden units per block
constexpr int RG = 4;     // batch rows per block
constexpr int KQMAX = 16; // reduction-axis pieces: H = KC * KQ with KQ <= 16; a block has 16 * KQ threads
constexpr int HMAX = 1024;

// forward copy: thread (kq, j) of slice s needs W_hh[g*H + s*16 + j][kq*KC + i], g < 3, i < KC = H/16, as 3*KC/4 float4s
//   wf[((s * NC + c) * NT + tid) * 4 + e]   with chunk c = g * (KC/4) + i/4, e = i % 4, tid = kq * 16 + j, NT = 16 KQ
__device__ __forceinline__ void gru_layout_fwd_elem(const float* __restrict__ w_hh, float* __restrict__ wf, int H, int KQ) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)3 * H * H) return;
    const int KC = H / KQ, NC = 3 * KC / 4, NT = 16 * KQ;
    const int e = i & 3;
    int64_t r = i >> 2;
    const int tid = r % NT; r /= NT;
    const int c = r % NC;
    const int s = r / NC;
    const int g = c / (KC / 4), i4 = c % (KC / 4);
    const int kq = tid >> 4, j = tid & 15;
    wf[i] = w_hh[((int64_t)g * H + s * 16 + j) * H + kq * KC + i4 * 4 + e];
}
__global__ void gru_layout_fwd_kernel(const float* __restrict__ w_hh, float* __restrict__ wf, int H, int KQ) {
    gru_layout_fwd_elem(w_hh, wf, H, KQ);
}
constexpr int NNET = 4;   // networks one multi launch takes
struct GruLayoutMulti {
    const float* w_hh[NNET];
    float* wf[NNET];
};
__global__ void gru_layout_fwd_multi_kernel(GruLayoutMulti m, int H, int KQ) {    // network in grid.y
    gru_layout_fwd_elem(m.w_hh[blockIdx.y], m.wf[blockIdx.y], H, KQ);
}
// backward copy: thread (kq, j) needs W_hh[q][s*16 + j] for the kq-th 1/16 of the 3H gate rows q: RC = 3H/16 values
//   wb[((s * NC + c) * NT + tid) * 4 + e]   with q = kq * RC + c * 4 + e
__global__ void gru_layout_bwd_kernel(const float* __restrict__ w_hh, float* __restrict__ wb, int H, int KQ) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)3 * H * H) return;
    const int RC = 3 * H / KQ, NC = RC / 4, NT = 16 * KQ;
    const int e = i & 3;
    int64_t r = i >> 2;
    const int tid = r % NT; r /= NT;
    const int c = r % NC;
    const int s = r / NC;
    const int kq = tid >> 4, j = tid & 15;
    wb[i] = w_hh[((int64_t)kq * RC + c * 4 + e) * H + s * 16 + j];
}

struct GruFwd {
    const float *gi, *wf, *b_hh, *h0;
    float *h_all, *gates;
    int B, L, H, t;
};

// One step of one network for the workgroup (unit slice s, rows b0 .. b0 + RG): the body of the launch-per-step kernels, single
// and multi-network alike.
template <int KC>                                    // KC = H / 16: reduction elements per thread and gate
__device__ __forceinline__ void gru_fwd_step_body(const GruFwd& p, const int s, const int b0) {
    constexpr int NC = 3 * KC / 4;
    __shared__ __attribute__((aligned(16))) float s_h[RG][KC * KQMAX];
    __shared__ float s_p[KQMAX][RG * 3][US + 1];
    const int tid = threadIdx.x, NT = blockDim.x, KQ = NT >> 4, H = p.H;
    const int j = tid & 15, kq = tid >> 4;
    // this thread's piece of W_hh (registers) and the gate inputs of its output (issued first: longest latency)
    float4 w[NC];
    const float4* wsrc = reinterpret_cast<const float4*>(p.wf) + (size_t)s * NC * NT + tid;
#pragma unroll
    for (int c = 0; c < NC; ++c) w[c] = wsrc[(size_t)c * NT];
    const int ro = tid >> 4, uo = s * US + j;        // output mapping of the first RG*16 threads: (row ro, unit uo)
    const bool out_thr = tid < RG * US && b0 + ro < p.B;
    float gir = 0.f, giz = 0.f, gin = 0.f, br = 0.f, bz = 0.f, bn = 0.f;
    if (out_thr) {
        const float* g = p.gi + ((int64_t)(b0 + ro) * p.L + p.t) * 3 * H;
        gir = g[uo]; giz = g[H + uo]; gin = g[2 * H + uo];
        br = p.b_hh[uo]; bz = p.b_hh[H + uo]; bn = p.b_hh[2 * H + uo];
    }
    for (int i = tid; i < RG * H / 4; i += NT) {
        const int r = i / (H / 4), c4 = (i % (H / 4)) * 4;
        const int b = b0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < p.B) {
            if (p.t > 0) v = ld4(p.h_all + ((int64_t)b * p.L + (p.t - 1)) * H + c4);
            else if (p.h0) v = ld4(p.h0 + (int64_t)b * H + c4);
        }
        st4(&s_h[r][c4], v);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RG; ++r) {
        float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int i4 = 0; i4 < KC / 4; ++i4) {
            const float4 hv = ld4(&s_h[r][kq * KC + i4 * 4]);
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const float4 wv = w[g * (KC / 4) + i4];
                a[g] = __builtin_fmaf(hv.x, wv.x, a[g]); a[g] = __builtin_fmaf(hv.y, wv.y, a[g]);
                a[g] = __builtin_fmaf(hv.z, wv.z, a[g]); a[g] = __builtin_fmaf(hv.w, wv.w, a[g]);
            }
        }
        s_p[kq][r * 3 + 0][j] = a[0];
        s_p[kq][r * 3 + 1][j] = a[1];
        s_p[kq][r * 3 + 2][j] = a[2];
    }
    __syncthreads();
    if (out_thr) {
        float ar = 0.f, az = 0.f, an = 0.f;
        for (int q = 0; q < KQ; ++q) { ar += s_p[q][ro * 3][j]; az += s_p[q][ro * 3 + 1][j]; an += s_p[q][ro * 3 + 2][j]; }
        const int64_t tok = (int64_t)(b0 + ro) * p.L + p.t;
        const float rg = sigmoidf_(gir + ar + br);
        const float zg = sigmoidf_(giz + az + bz);
        const float hn = an + bn;
        const float ng = gru_tanh(gin + rg * hn);
        const float hp = s_h[ro][uo];
        p.h_all[tok * H + uo] = (1.f - zg) * ng + zg * hp;
        if (p.gates) {
            float* o = p.gates + tok * 4 * H;
            o[uo] = rg; o[H + uo] = zg; o[2 * H + uo] = ng; o[3 * H + uo] = hn;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Persistent forward: ONE launch walks all L steps.  The 16 unit-slice workgroups of a row group exchange h_t through 8-byte
// {tag = step + 1, value} granules in global memory (cdna_hip_programming.md section 6 Guideline 16, form R2: the data is
// the flag - relaxed agent-scope 8-byte atomic stores are write-through, the consumer re-reads its granules with relaxed
// agent-scope loads until every tag matches; no flag word, no fence, placement-independent).  Two granule buffers
// alternate by step parity: a workgroup can publish h_{t+1} only after it has read every slice of h_t, so a slow reader
// of h_t is never overtaken by more than one step.  W_hh pieces stay in registers for the whole sequence and the host
// issues one launch instead of L.  All workgroups must be resident (they are tiny: the launcher caps the grid); every spin
// is bounded and raises `err` instead of hanging.
typedef unsigned long long u64;
#define RESEL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
constexpr unsigned SPIN_LIMIT = 1u << 22;

// ids congruent mod 8 share an XCD (round-robin dispatch): give a row group's slices one XCD when the grid allows it
__device__ __forceinline__ int gru_xcd_remap(int id, const int total) {
    if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
    return id;
}

// All L steps of one network for the workgroup with (remapped) index `id` inside that network's H/16 x ceil(B/4) workgroups: the
// body of the single-network persistent kernel and of the multi-network one (which picks the network from the outermost part
// of the index), so that a network's arithmetic does not depend on how many others share the launch.
template <int KC>
__device__ __forceinline__ void gru_fwd_persistent_body(const GruFwd& p, u64* __restrict__ xchg, int* __restrict__ err, const int id) {
    constexpr int NC = 3 * KC / 4;
    __shared__ __attribute__((aligned(16))) float s_h[RG][KC * KQMAX];
    __shared__ float s_p[KQMAX][RG * 3][US + 1];
    __shared__ int s_fail;
    const int tid = threadIdx.x, NT = blockDim.x, KQ = NT >> 4, H = p.H;
    const int nslice = H / US;
    const int s = id % nslice, rg = id / nslice, b0 = rg * RG;
    const int j = tid & 15, kq = tid >> 4;
    float4 w[NC];
    const float4* wsrc = reinterpret_cast<const float4*>(p.wf) + (size_t)s * NC * NT + tid;
#pragma unroll
    for (int c = 0; c < NC; ++c) w[c] = wsrc[(size_t)c * NT];
    const int ro = tid >> 4, uo = s * US + j;
    const bool out_thr = tid < RG * US && b0 + ro < p.B;
    float br = 0.f, bz = 0.f, bn = 0.f;
    if (out_thr) { br = p.b_hh[uo]; bz = p.b_hh[H + uo]; bn = p.b_hh[2 * H + uo]; }
    u64* xg = xchg + (size_t)rg * 2 * RG * H;        // [2][RG][H] granules of this row group
    if (tid == 0) s_fail = 0;
    __syncthreads();
    for (int t = 0; t < p.L; ++t) {
        float gir = 0.f, giz = 0.f, gin = 0.f;
        if (out_thr) {                               // independent of the recurrence: in flight during the wait below
            const float* g = p.gi + ((int64_t)(b0 + ro) * p.L + t) * 3 * H;
            gir = g[uo]; giz = g[H + uo]; gin = g[2 * H + uo];
        }
        if (t == 0) {
            for (int i = tid; i < RG * H; i += NT) {
                const int r = i / H, u = i % H;
                s_h[r][u] = (p.h0 && b0 + r < p.B) ? p.h0[(int64_t)(b0 + r) * H + u] : 0.f;
            }
        } else {
            const u64* src = xg + (size_t)((t - 1) & 1) * RG * H;
            const unsigned epoch = (unsigned)t;      // h_{t-1} was published with tag t
            // all granules of this thread are requested before the first tag is looked at: one L2 round trip in the common
            // case instead of one per granule (the polls were the longest part of a step)
            constexpr int NPOLL = (RG * KC + 15) / 16;           // = RG * H / NT  (H = KC * KQ, NT = 16 * KQ)
            u64 xv[NPOLL];
            // The first poll is held back by ~770 cycles where a step is long enough (H >= 256): h_{t-1} of the other slices becomes
            // visible 0.4-0.5 us after this workgroup's own publish, and a poll that arrives in L2 before the data costs a whole second
            // round trip.  B = 64, H = 256, same box, us per step: no delay 2.70; s_sleep 2 / 4 / 8 / 12 / 16 / 20 / 24 / 32: 2.61 / 2.62 /
            // 2.65 / 2.20 / 2.24 / 2.35 / 2.46 / 2.67.  B = 32: 2.58 -> 2.15.  H = 128: no change; H = 64: 2.08 -> 2.25 (no delay there).
            // (The backward's poll already sits behind the loads of its carry-independent operands: any delay there measured slower.)
            if (KC >= 16) __builtin_amdgcn_s_sleep(12);
#pragma unroll
            for (int q = 0; q < NPOLL; ++q) {
                const int i = tid + q * NT;
                xv[q] = i < RG * H ? __hip_atomic_load(src + i, RESEL_RLX_AGENT) : 0;
            }
#pragma unroll
            for (int q = 0; q < NPOLL; ++q) {
                const int i = tid + q * NT;
                if (i >= RG * H) continue;
                u64 x = xv[q];
                unsigned spins = 0;
                while ((unsigned)(x >> 32) != epoch) {
                    if (++spins > SPIN_LIMIT) { s_fail = 1; break; }
                    __builtin_amdgcn_s_sleep(1);
                    x = __hip_atomic_load(src + i, RESEL_RLX_AGENT);
                }
                (&s_h[0][0])[(i / H) * (KC * KQMAX) + (i % H)] = __uint_as_float((unsigned)x);
            }
        }
        __syncthreads();
        if (s_fail) {                                // uniform: written before the barrier.  Fail LOUDLY: poison the output
            if (tid == 0) atomicExch(err, 1);
            if (out_thr) p.h_all[((int64_t)(b0 + ro) * p.L + t) * H + uo] = __builtin_nanf("");
            return;
        }
#pragma unroll
        for (int r = 0; r < RG; ++r) {
            float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int i4 = 0; i4 < KC / 4; ++i4) {
                const float4 hv = ld4(&s_h[r][kq * KC + i4 * 4]);
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    const float4 wv = w[g * (KC / 4) + i4];
                    a[g] = __builtin_fmaf(hv.x, wv.x, a[g]); a[g] = __builtin_fmaf(hv.y, wv.y, a[g]);
                    a[g] = __builtin_fmaf(hv.z, wv.z, a[g]); a[g] = __builtin_fmaf(hv.w, wv.w, a[g]);
                }
            }
            s_p[kq][r * 3 + 0][j] = a[0];
            s_p[kq][r * 3 + 1][j] = a[1];
            s_p[kq][r * 3 + 2][j] = a[2];
        }
        // h_{t-1} of the owned unit is fetched on THIS side of the barrier: behind it nothing reads s_h any more, so the next step's
        // poll may overwrite it while slower waves still finish this step - one barrier per step less
        const float hp = tid < RG * US ? s_h[ro][uo] : 0.f;
        __syncthreads();
        if (tid < RG * US) {
            float hnew = 0.f;
            if (out_thr) {
                float ar = 0.f, az = 0.f, an = 0.f;
                for (int q = 0; q < KQ; ++q) { ar += s_p[q][ro * 3][j]; az += s_p[q][ro * 3 + 1][j]; an += s_p[q][ro * 3 + 2][j]; }
                const int64_t tok = (int64_t)(b0 + ro) * p.L + t;
                const float rgt = sigmoidf_(gir + ar + br);
                const float zg = sigmoidf_(giz + az + bz);
                const float hn = an + bn;
                const float ng = gru_tanh(gin + rgt * hn);
                hnew = (1.f - zg) * ng + zg * hp;
                // publish FIRST (the other slices wait for it), the step's outputs behind it
                __hip_atomic_store(xg + (size_t)(t & 1) * RG * H + (size_t)ro * H + uo, ((u64)(unsigned)(t + 1) << 32) | __float_as_uint(hnew),
                                   RESEL_RLX_AGENT);
                p.h_all[tok * H + uo] = hnew;
                if (p.gates) {
                    float* o = p.gates + tok * 4 * H;
                    o[uo] = rgt; o[H + uo] = zg; o[2 * H + uo] = ng; o[3 * H + uo] = hn;
                }
            } else {
                // rows past B publish zeros so that every granule of the row group gets its tag
                __hip_atomic_store(xg + (size_t)(t & 1) * RG * H + (size_t)ro * H + uo, ((u64)(unsigned)(t + 1) << 32), RESEL_RLX_AGENT);
            }
        }
        // A third barrier is not needed for correctness any more (nothing behind the second one reads s_h; s_p is rewritten behind the
        // next step's first barrier) but the forward is FASTER with it: 2.71 against 3.00 us per step on the same box - the waves stay in
        // step for the next poll.  (The backward is faster without: 3.35 against 3.44.)
#ifndef GRU_AB_NOB3
        __syncthreads();
#endif
    }
}

template <int KC>
__global__ __launch_bounds__(256) void gru_fwd_step_kernel(GruFwd p) {
    gru_fwd_step_body<KC>(p, blockIdx.x, blockIdx.y * RG);
}
template <int KC>
__global__ __launch_bounds__(256) void gru_fwd_persistent_kernel(GruFwd p, u64* __restrict__ xchg, int* __restrict__ err) {
    gru_fwd_persistent_body<KC>(p, xchg, err, gru_xcd_remap(blockIdx.x, gridDim.x));
}

// ---------------------------------------------------------------------------------------------------------------------
// N independent recurrences (same B, L, H) in ONE launch: what three streams bought the gru trainer - latency-bound recurrences
// sharing the chip - as a property of the kernel, so that the update is a single-stream launch sequence a hipGraph capture
// takes.  The argument struct holds every network's pointers BY VALUE (host arrays are read by the C entry: no device-side
// pointer table, no copy).  Persistent form: grid = n_net x (H/16) x ceil(B/4) workgroups, network = outermost part of the
// XCD-remapped index (a row group's 16 slices stay on one XCD while total / 8 is a multiple of H/16); every network has its own
// granules and error word.  Per-step form: network in grid.z.
struct GruFwdMulti {
    GruFwd net[NNET];
    u64* xchg[NNET];
    int* err[NNET];
    int per_net;                                     // workgroups per network (persistent form)
};
template <int KC>
__global__ __launch_bounds__(256) void gru_fwd_multi_step_kernel(GruFwdMulti m) {
    gru_fwd_step_body<KC>(m.net[blockIdx.z], blockIdx.x, blockIdx.y * RG);
}
template <int KC>
__global__ __launch_bounds__(256) void gru_fwd_multi_persistent_kernel(GruFwdMulti m) {
    const int id = gru_xcd_remap(blockIdx.x, gridDim.x);
    const int n = id / m.per_net;
    gru_fwd_persistent_body<KC>(m.net[n], m.xchg[n], m.err[n], id - n * m.per_net);
}

struct GruBwd {
    const float *wb, *h0, *h_all, *gates, *dh_all, *carry_in;
    float *carry_out, *dgi, *dgh;
    int B, L, H, t;
};

template <int KC>
__global__ __launch_bounds__(256) void gru_bwd_step_kernel(GruBwd p) {
    constexpr int RC = 3 * KC;                       // gate rows per thread (3H / KQ)
    constexpr int NC = RC / 4;
    __shared__ __attribute__((aligned(16))) float s_gbuf[RG * 3 * KC * KQMAX];   // [RG][3H]: (dr | dz | dhn) of the RG rows, all H units
    __shared__ float s_dz[RG][US];                                    // dh * z of the owned units
    __shared__ float s_p[KQMAX][RG][US + 1];
    const int tid = threadIdx.x, NT = blockDim.x, KQ = NT >> 4, H = p.H;
    auto s_g = [&](int r) { return s_gbuf + (size_t)r * 3 * H; };
    const int s = blockIdx.x, b0 = blockIdx.y * RG;
    const int j = tid & 15, kq = tid >> 4;
    float4 w[NC];
    const float4* wsrc = reinterpret_cast<const float4*>(p.wb) + (size_t)s * NC * NT + tid;
#pragma unroll
    for (int c = 0; c < NC; ++c) w[c] = wsrc[(size_t)c * NT];
    // gate gradients for the RG rows x all H units (recomputed by every unit slice of the row group: elementwise)
    for (int i = tid; i < RG * H; i += NT) {
        const int r = i / H, u = i % H;
        const int b = b0 + r;
        float dr_ = 0.f, dz_ = 0.f, dn_ = 0.f, dhn = 0.f, dhz = 0.f;
        if (b < p.B) {
            const int64_t tok = (int64_t)b * p.L + p.t;
            const float dh = p.dh_all[tok * H + u] + p.carry_in[(int64_t)b * H + u];
            const float* g = p.gates + tok * 4 * H;
            const float rg = g[u], zg = g[H + u], ng = g[2 * H + u], hn = g[3 * H + u];
            const float hp = p.t > 0 ? p.h_all[(tok - 1) * H + u] : (p.h0 ? p.h0[(int64_t)b * H + u] : 0.f);
            const float dn = dh * (1.f - zg);
            dz_ = dh * (hp - ng) * zg * (1.f - zg);
            dn_ = dn * (1.f - ng * ng);
            dr_ = dn_ * hn * rg * (1.f - rg);
            dhn = dn_ * rg;
            dhz = dh * zg;
            if (u / US == s) {                       // owned slice: publish the projection gradients once
                float* o1 = p.dgi + tok * 3 * H;
                float* o2 = p.dgh + tok * 3 * H;
                o1[u] = dr_; o1[H + u] = dz_; o1[2 * H + u] = dn_;
                o2[u] = dr_; o2[H + u] = dz_; o2[2 * H + u] = dhn;
            }
        }
        s_g(r)[u] = dr_;
        s_g(r)[H + u] = dz_;
        s_g(r)[2 * H + u] = dhn;
        if (u / US == s) s_dz[r][u % US] = dhz;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RG; ++r) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float4 gv = ld4(s_g(r) + kq * RC + c * 4);
            acc = __builtin_fmaf(gv.x, w[c].x, acc); acc = __builtin_fmaf(gv.y, w[c].y, acc);
            acc = __builtin_fmaf(gv.z, w[c].z, acc); acc = __builtin_fmaf(gv.w, w[c].w, acc);
        }
        s_p[kq][r][j] = acc;
    }
    __syncthreads();
    if (tid < RG * US) {
        const int r = tid >> 4;
        const int b = b0 + r;
        float acc = s_dz[r][j];
        for (int q = 0; q < KQ; ++q) acc += s_p[q][r][j];
        if (b < p.B) p.carry_out[(int64_t)b * H + s * US + j] = acc;
    }
}

// Persistent backward: same exchange protocol as the forward; step t publishes the carry d h_{t-1} (its 16 units x RG rows)
// with tag (L - t), the step for t-1 collects all H units of its rows.  The gate-gradient operands of the NEXT step do not
// depend on the carry and are loaded before the wait.
template <int KC>
__global__ __launch_bounds__(256) void gru_bwd_persistent_kernel(GruBwd p, u64* __restrict__ xchg, int* __restrict__ err) {
    constexpr int RC = 3 * KC;
    constexpr int NC = RC / 4;
    constexpr int PER = (RG * KC * KQMAX + 255) / 256;       // (row, unit) items per thread at the widest block
    __shared__ __attribute__((aligned(16))) float s_gbuf[RG * 3 * KC * KQMAX];
    __shared__ float s_dz[RG][US], s_dn[RG][US];
    __shared__ float s_p[KQMAX][RG][US + 1];
    __shared__ int s_fail;
    const int tid = threadIdx.x, NT = blockDim.x, KQ = NT >> 4, H = p.H;
    auto s_g = [&](int r) { return s_gbuf + (size_t)r * 3 * H; };
    const int nslice = H / US;
    int id = blockIdx.x;
    const int total = gridDim.x;
    if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
    const int s = id % nslice, rg = id / nslice, b0 = rg * RG;
    const int j = tid & 15, kq = tid >> 4;
    float4 w[NC];
    const float4* wsrc = reinterpret_cast<const float4*>(p.wb) + (size_t)s * NC * NT + tid;
#pragma unroll
    for (int c = 0; c < NC; ++c) w[c] = wsrc[(size_t)c * NT];
    u64* xg = xchg + (size_t)rg * 2 * RG * H;
    if (tid == 0) s_fail = 0;
    __syncthreads();
    for (int t = p.L - 1, k = 0; t >= 0; --t, ++k) {          // k = steps already done; the carry consumed here has tag k
        // operands that do not depend on the carry
        float dho[PER], rgv[PER], zgv[PER], ngv[PER], hnv[PER], hpv[PER];
#pragma unroll
        for (int n = 0; n < PER; ++n) {
            const int i = tid + n * NT;
            dho[n] = rgv[n] = zgv[n] = ngv[n] = hnv[n] = hpv[n] = 0.f;
            if (i < RG * H && b0 + i / H < p.B) {
                const int r = i / H, u = i % H;
                const int64_t tok = (int64_t)(b0 + r) * p.L + t;
                const float* g = p.gates + tok * 4 * H;
                dho[n] = p.dh_all[tok * H + u];
                rgv[n] = g[u]; zgv[n] = g[H + u]; ngv[n] = g[2 * H + u]; hnv[n] = g[3 * H + u];
                hpv[n] = t > 0 ? p.h_all[(tok - 1) * H + u] : (p.h0 ? p.h0[(int64_t)(b0 + r) * H + u] : 0.f);
            }
        }
        const u64* src = xg + (size_t)((k - 1) & 1) * RG * H;
        u64 xv[PER];                                             // every carry granule requested before the first tag check
#pragma unroll
        for (int n = 0; n < PER; ++n) {
            const int i = tid + n * NT;
            xv[n] = (k > 0 && i < RG * H) ? __hip_atomic_load(src + i, RESEL_RLX_AGENT) : 0;
        }
#pragma unroll
        for (int n = 0; n < PER; ++n) {
            const int i = tid + n * NT;
            if (i >= RG * H) continue;
            const int r = i / H, u = i % H;
            float carry = 0.f;
            if (k > 0) {
                u64 x = xv[n];
                unsigned spins = 0;
                while ((unsigned)(x >> 32) != (unsigned)k) {
                    if (++spins > SPIN_LIMIT) { s_fail = 1; break; }
                    __builtin_amdgcn_s_sleep(1);
                    x = __hip_atomic_load(src + i, RESEL_RLX_AGENT);
                }
                carry = __uint_as_float((unsigned)x);
            }
            float dr_ = 0.f, dz_ = 0.f, dn_ = 0.f, dhn = 0.f, dhz = 0.f;
            if (b0 + r < p.B) {
                const float dh = dho[n] + carry;
                const float rgt = rgv[n], zg = zgv[n], ng = ngv[n], hn = hnv[n];
                const float dn = dh * (1.f - zg);
                dz_ = dh * (hpv[n] - ng) * zg * (1.f - zg);
                dn_ = dn * (1.f - ng * ng);
                dr_ = dn_ * hn * rgt * (1.f - rgt);
                dhn = dn_ * rgt;
                dhz = dh * zg;
            }
            s_g(r)[u] = dr_;
            s_g(r)[H + u] = dz_;
            s_g(r)[2 * H + u] = dhn;
            if (u / US == s) { s_dz[r][u % US] = dhz; s_dn[r][u % US] = dn_; }
        }
        __syncthreads();
        if (s_fail) {                                // fail loudly: poison this step's projection gradients
            if (tid == 0) atomicExch(err, 2);
            if (tid < RG * US && b0 + (tid >> 4) < p.B) p.dgi[((int64_t)(b0 + (tid >> 4)) * p.L + t) * 3 * H + s * US + j] = __builtin_nanf("");
            return;
        }
#pragma unroll
        for (int r = 0; r < RG; ++r) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float4 gv = ld4(s_g(r) + kq * RC + c * 4);
                acc = __builtin_fmaf(gv.x, w[c].x, acc); acc = __builtin_fmaf(gv.y, w[c].y, acc);
                acc = __builtin_fmaf(gv.z, w[c].z, acc); acc = __builtin_fmaf(gv.w, w[c].w, acc);
            }
            s_p[kq][r][j] = acc;
        }
        // read on this side of the barrier (as h_{t-1} in the forward): dh z of the owned unit, and the owned projection gradients, which
        // are stored BEHIND the publish (24 stores of one quarter-wave used to sit in front of the first barrier of every step)
        float dz_own = 0.f, o_dr = 0.f, o_dz = 0.f, o_dhn = 0.f, o_dn = 0.f;
        if (tid < RG * US) {
            const int r = tid >> 4, u = s * US + j;
            dz_own = s_dz[r][j]; o_dn = s_dn[r][j];
            o_dr = s_g(r)[u]; o_dz = s_g(r)[H + u]; o_dhn = s_g(r)[2 * H + u];
        }
        __syncthreads();
        if (tid < RG * US) {
            const int r = tid >> 4;
            float acc = dz_own;
            for (int q = 0; q < KQ; ++q) acc += s_p[q][r][j];
            if (b0 + r >= p.B) acc = 0.f;
            if (t == 0) { if (b0 + r < p.B) p.carry_out[(int64_t)(b0 + r) * H + s * US + j] = acc; }     // d h_0 (unused by the caller)
            else __hip_atomic_store(xg + (size_t)(k & 1) * RG * H + (size_t)r * H + s * US + j,
                                    ((u64)(unsigned)(k + 1) << 32) | __float_as_uint(acc), RESEL_RLX_AGENT);
            if (b0 + r < p.B) {
                const int u = s * US + j;
                const int64_t tok = (int64_t)(b0 + r) * p.L + t;
                float* o1 = p.dgi + tok * 3 * H;
                float* o2 = p.dgh + tok * 3 * H;
                o1[u] = o_dr; o1[H + u] = o_dz; o1[2 * H + u] = o_dn;
                o2[u] = o_dr; o2[H + u] = o_dz; o2[2 * H + u] = o_dhn;
            }
        }
        // no third barrier: s_g / s_dz are rewritten before, s_p behind the next step's first barrier - neither is read above (3.44 -> 3.35 us per step)
    }
}

// H = KC * KQ with KC in {4, 8, 12, 16, 24, 32} (templated) and 4 <= KQ <= 16: every multiple of 16 up to 256, and
// 288 / 320 / 336 / 352 / 384 / 416 / 448 / 480 / 512 above.  640 / 768 / 896 / 1024 are named one by one (KQ = 16, KC = 40 / 48 / 56 / 64): the accepted set is a
// list, not whatever factors (a KC of 40 in the candidates would let 200 = 40 x 5 in).
inline int pick_kc(int H) {
    const int cand[6] = {4, 8, 12, 16, 24, 32};
    for (int kc : cand)
        if (H % kc == 0 && H / kc <= KQMAX && H / kc >= 4) return kc;
    if (H == 640 || H == 768 || H == 896 || H == 1024) return H / KQMAX;
    return 0;
}
// The run-time KC as a template argument: f(std::integral_constant<int, KC>) for the ten instantiations, RESEL_EINVAL for any other KC.
template <typename F>
inline int with_kc(int KC, F&& f) {
    switch (KC) {
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 12: return f(std::integral_constant<int, 12>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 24: return f(std::integral_constant<int, 24>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 40: return f(std::integral_constant<int, 40>{});
        case 48: return f(std::integral_constant<int, 48>{});
        case 56: return f(std::integral_constant<int, 56>{});
        case 64: return f(std::integral_constant<int, 64>{});
    }
    return RESEL_EINVAL;
}
inline bool gru_ok(int B, int L, int H) { return B > 0 && L > 0 && H > 0 && H % 16 == 0 && H <= HMAX && pick_kc(H) > 0; }
inline int gru_workgroups(int B, int H) { return (H / US) * ((B + RG - 1) / RG); }     // of one network: unit slices x row groups

// Workspace of one call on n networks (the single-network entries: n = 1):
//   [n x W copy (3 H H floats each) | carry (2 B H floats; single-network entries only) | n x (exchange granules, 8 bytes each; error word in 64 bytes)]
// The granule / error blocks of all networks are contiguous: one memset clears them.
struct GruWorkspace {
    char* base;
    size_t n, w_bytes, carry_bytes, granule_bytes;
    GruWorkspace(void* workspace, int n_net, int B, int H, bool with_carry)
        : base((char*)workspace), n((size_t)n_net), w_bytes((size_t)3 * H * H * sizeof(float)),
          carry_bytes(with_carry ? (size_t)2 * B * H * sizeof(float) : 0), granule_bytes((size_t)((B + RG - 1) / RG) * 2 * RG * H * sizeof(u64)) {}
    size_t sync_bytes() const { return granule_bytes + 64; }                            // per network
    size_t bytes() const { return n * (w_bytes + sync_bytes()) + carry_bytes; }
    float* wcopy(int k = 0) const { return (float*)(base + k * w_bytes); }
    float* carry() const { return (float*)(base + n * w_bytes); }
    char* sync(int k = 0) const { return base + n * w_bytes + carry_bytes + k * sync_bytes(); }
    u64* xchg(int k = 0) const { return (u64*)sync(k); }
    int* err(int k = 0) const { return (int*)(sync(k) + granule_bytes); }
};

// RESEL_GRU_PERSISTENT=0 forces the launch-per-step form (read once per process)
inline bool gru_persistent_allowed() {
    static const int mode = getenv("RESEL_GRU_PERSISTENT") ? atoi(getenv("RESEL_GRU_PERSISTENT")) : 1;
    return mode != 0;
}
// persistent form: all workgroups must be co-resident.  The backward kernel runs at 2 waves per SIMD (2 workgroups per CU),
// so the grid is capped at one workgroup per CU of the smallest configuration this library targets (256 CUs); larger
// problems keep the launch-per-step form.
// (the multi-network forward below has its own residency rule: its grid is up to four times as large)
inline bool persistent_ok(int B, int H) { return gru_persistent_allowed() && gru_workgroups(B, H) <= 256; }
// gfx950 build of the widths above 512 (KC 40 / 48 / 56 / 64; 256 threads, so one workgroup per CU needs <= 512 registers per lane):
//   forward persistent 216 / 245 / 277 / 311 registers, 23-29 KB of LDS, no scratch: resident at one per CU, rule above holds;
//   backward persistent 430 / 512 / 512 / 512 registers, 35-53 KB of LDS, and 352 / 676 bytes of scratch per lane at KC 56 / 64
//   (the carry-independent operands of a step, 8 registers per (row, unit) item and RG * KC / 16 items, on top of 3 KC of W_hh).
// A step that spills cannot keep the 3.9 us the persistent form is there for, so those two widths take the per-step backward
// (200 / 224 registers, no scratch) whatever the grid; everything else is routed as before.
constexpr int BWD_PERSISTENT_KC_MAX = 48;
inline bool bwd_persistent_ok(int B, int H) { return persistent_ok(B, H) && pick_kc(H) <= BWD_PERSISTENT_KC_MAX; }

}  // namespace

extern "C" size_t resel_gru_workspace_bytes(int B, int L, int H) {
    (void)L;
    return GruWorkspace(nullptr, 1, B, H, true).bytes();
}

extern "C" int resel_gru_seq_fwd(const float* gi, const float* w_hh, const float* b_hh, const float* h0,
                                 float* h_all, float* gates, void* workspace, int B, int L, int H, resel_stream_t stream) {
    if (!gi || !w_hh || !b_hh || !h_all || !workspace || !gru_ok(B, L, H)) return RESEL_EINVAL;
    if (!aligned16(h_all) || !aligned16(workspace) || (h0 && !aligned16(h0))) return RESEL_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const GruWorkspace ws(workspace, 1, B, H, true);
    const int64_t nw = (int64_t)3 * H * H;
    const int KC = pick_kc(H), KQ = H / KC;
    hipLaunchKernelGGL(gru_layout_fwd_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, w_hh, ws.wcopy(), H, KQ);
    GruFwd p{gi, ws.wcopy(), b_hh, h0, h_all, gates, B, L, H, 0};
    if (persistent_ok(B, H)) {
        if (hipMemsetAsync(ws.sync(), 0, ws.sync_bytes(), s) != hipSuccess) return RESEL_ELAUNCH;
        const dim3 pgrid(gru_workgroups(B, H));
        return with_kc(KC, [&](auto kc) {
            launch_timed(RESEL_PROF_GRU_FWD, gru_fwd_persistent_kernel<decltype(kc)::value>, pgrid, dim3(16 * KQ), 0, s, p, ws.xchg(), ws.err());
            return launch_status();
        });
    }
    dim3 grid(H / US, (B + RG - 1) / RG);
    return with_kc(KC, [&](auto kc) {
        for (int t = 0; t < L; ++t) {
            p.t = t;
            launch_timed(RESEL_PROF_GRU_FWD, gru_fwd_step_kernel<decltype(kc)::value>, grid, dim3(16 * KQ), 0, s, p);
        }
        return launch_status();
    });
}

// ---- multi-network forward ------------------------------------------------------------------------------------------
// workspace: GruWorkspace without a carry; sized n x the single-network size (rounded to 16 bytes), so that a caller may size either way.
extern "C" size_t resel_gru_multi_workspace_bytes(int n_net, int B, int L, int H) {
    if (n_net < 1) n_net = 1;
    return (size_t)n_net * ((resel_gru_workspace_bytes(B, L, H) + 15) & ~(size_t)15);
}

// Workgroups of gru_fwd_multi_persistent_kernel<KC> the device keeps resident at once.  Chosen source: the kernel's OWN resource
// numbers (hipFuncGetAttributes: registers per lane, static LDS), not hipOccupancyMaxActiveBlocksPerMultiprocessor - that call is
// advisory and over-reports by one block per CU for 256-thread kernels with 82+ SGPRs (this one: 87-95), and "API minus one"
// would be a correction that is right only while that quirk lasts.  A SIMD holds 512 registers per lane in 8-register granules
// and at most 8 waves; a workgroup here has at most 4 waves, one per SIMD, so workgroups per CU = waves per SIMD, further bounded
// by 160 KB of LDS and by 7 (the SGPR rule for 82-96 SGPRs).  gfx950 build of this file: KC 4 / 8 / 12 / 16 / 24 / 32 use
// 60 / 78 / 98 / 124 / 154 / 184 VGPRs, 73-84 SGPRs, no scratch, 14-21 KB of LDS -> 7 / 6 / 4 / 4 / 3 / 2 workgroups per CU (H = 256: 4,
// H = 384: 3, H = 512: 2; the compiler's own `Occupancy [waves/SIMD]` remark says 8 / 6 / 4 / 4 / 3 / 2).  KC 40 / 48 / 56 / 64: below.
// Cached per instantiation; 0 when no device answers (the per-step form needs no residency).
template <int KC>
inline int multi_resident_cap() {
    static const int cap = [] {
        hipFuncAttributes fa;
        hipDeviceProp_t prop;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess ||
            hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(gru_fwd_multi_persistent_kernel<KC>)) != hipSuccess) {
            (void)hipGetLastError();
            return 0;
        }
        const int regs = ((fa.numRegs > 0 ? fa.numRegs : 512) + 7) & ~7;
        int per_cu = 512 / regs;
        const int lds = (int)fa.sharedSizeBytes > 0 ? (160 * 1024) / (int)fa.sharedSizeBytes : 8;
        if (per_cu > lds) per_cu = lds;
        if (per_cu > 7) per_cu = 7;
        // KC 40 / 48 / 56 / 64 (H = 640 .. 1024): 214 / 243 / 274 / 309 registers (the last two 256 + 18 / 53 accumulation registers) -> 2 / 2 /
        // 1 / 1 per CU.  Held to the compiler's figure whatever the runtime reports for a kernel that uses both register files.
        constexpr int known = KC >= 56 ? 1 : (KC >= 40 ? 2 : 7);
        if (per_cu > known) per_cu = known;
        return per_cu * prop.multiProcessorCount;
    }();
    return cap;
}
inline int multi_cap(int KC) {
    const int cap = with_kc(KC, [](auto kc) { return multi_resident_cap<decltype(kc)::value>(); });
    return cap > 0 ? cap : 0;                            // no instantiation for this KC: nothing is resident
}
inline bool multi_persistent_ok(int n_net, int B, int H) {
    return gru_persistent_allowed() && n_net * gru_workgroups(B, H) <= multi_cap(pick_kc(H));
}

extern "C" int resel_gru_multi_form(int n_net, int B, int H) {
    if (n_net < 1 || n_net > NNET || !gru_ok(B, 1, H)) return RESEL_EINVAL;
    return multi_persistent_ok(n_net, B, H) ? 1 : 0;
}

extern "C" int resel_gru_multi_fwd(int n_net, const float* const* gi, const float* const* w_hh, const float* const* b_hh,
                                   const float* const* h0, float* const* h_all, float* const* gates, void* workspace,
                                   int B, int L, int H, resel_stream_t stream) {
    if (n_net < 1 || n_net > NNET || !gi || !w_hh || !b_hh || !h_all || !workspace || !gru_ok(B, L, H)) return RESEL_EINVAL;
    if (!aligned16(workspace)) return RESEL_EINVAL;
    for (int n = 0; n < n_net; ++n) {
        if (!gi[n] || !w_hh[n] || !b_hh[n] || !h_all[n] || !aligned16(h_all[n]) || (h0 && h0[n] && !aligned16(h0[n]))) return RESEL_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const GruWorkspace ws(workspace, n_net, B, H, false);
    const int64_t nw = (int64_t)3 * H * H;
    const int KC = pick_kc(H), KQ = H / KC;
    GruLayoutMulti lay{};
    GruFwdMulti m{};
    for (int n = 0; n < n_net; ++n) {
        lay.w_hh[n] = w_hh[n];
        lay.wf[n] = ws.wcopy(n);
        m.net[n] = GruFwd{gi[n], ws.wcopy(n), b_hh[n], h0 ? h0[n] : nullptr, h_all[n], gates ? gates[n] : nullptr, B, L, H, 0};
        m.xchg[n] = ws.xchg(n);
        m.err[n] = ws.err(n);
    }
    m.per_net = gru_workgroups(B, H);
    hipLaunchKernelGGL(gru_layout_fwd_multi_kernel, dim3((unsigned)((nw + 255) / 256), n_net), dim3(256), 0, s, lay, H, KQ);
    // the error words are cleared in either form: callers read them after the pass
    if (hipMemsetAsync(ws.sync(), 0, (size_t)n_net * ws.sync_bytes(), s) != hipSuccess) return RESEL_ELAUNCH;
    if (multi_persistent_ok(n_net, B, H)) {
        const dim3 pgrid((unsigned)(n_net * m.per_net));
        return with_kc(KC, [&](auto kc) {
            launch_timed(RESEL_PROF_GRU_FWD, gru_fwd_multi_persistent_kernel<decltype(kc)::value>, pgrid, dim3(16 * KQ), 0, s, m);
            return launch_status();
        });
    }
    const dim3 grid(H / US, (B + RG - 1) / RG, n_net);
    return with_kc(KC, [&](auto kc) {
        for (int t = 0; t < L; ++t) {
            for (int n = 0; n < n_net; ++n) m.net[n].t = t;
            launch_timed(RESEL_PROF_GRU_FWD, gru_fwd_multi_step_kernel<decltype(kc)::value>, grid, dim3(16 * KQ), 0, s, m);
        }
        return launch_status();
    });
}

extern "C" int resel_gru_seq_bwd(const float* w_hh, const float* h0, const float* h_all, const float* gates,
                                 const float* dh_all, float* dgi, float* dgh, void* workspace,
                                 int B, int L, int H, resel_stream_t stream) {
    if (!w_hh || !h_all || !gates || !dh_all || !dgi || !dgh || !workspace || !gru_ok(B, L, H)) return RESEL_EINVAL;
    if (!aligned16(workspace)) return RESEL_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const GruWorkspace ws(workspace, 1, B, H, true);
    float* carry = ws.carry();
    const int64_t nw = (int64_t)3 * H * H;
    const int KC = pick_kc(H), KQ = H / KC;
    hipLaunchKernelGGL(gru_layout_bwd_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, w_hh, ws.wcopy(), H, KQ);
    if (hipMemsetAsync(carry, 0, ws.carry_bytes, s) != hipSuccess) return RESEL_ELAUNCH;
    GruBwd p{ws.wcopy(), h0, h_all, gates, dh_all, nullptr, nullptr, dgi, dgh, B, L, H, 0};
    if (bwd_persistent_ok(B, H)) {
        if (hipMemsetAsync(ws.sync(), 0, ws.sync_bytes(), s) != hipSuccess) return RESEL_ELAUNCH;
        p.carry_out = carry;
        const dim3 pgrid(gru_workgroups(B, H));
        return with_kc(KC, [&](auto kc) {
            if constexpr (decltype(kc)::value <= BWD_PERSISTENT_KC_MAX) {        // the spilling instantiations are not even built
                launch_timed(RESEL_PROF_GRU_BWD, gru_bwd_persistent_kernel<decltype(kc)::value>, pgrid, dim3(16 * KQ), 0, s, p, ws.xchg(), ws.err());
                return launch_status();
            } else {
                return (int)RESEL_EINVAL;
            }
        });
    }
    dim3 grid(H / US, (B + RG - 1) / RG);
    return with_kc(KC, [&](auto kc) {
        for (int t = L - 1; t >= 0; --t) {
            p.t = t;
            p.carry_in = carry + (size_t)((t + 1) & 1) * B * H;
            p.carry_out = carry + (size_t)(t & 1) * B * H;
            launch_timed(RESEL_PROF_GRU_BWD, gru_bwd_step_kernel<decltype(kc)::value>, grid, dim3(16 * KQ), 0, s, p);
        }
        return launch_status();
    });
}

// ---- widths that are not native: zero padding per gate block ----------------------------------------------------------
// One launch moves up to four tensors (segment in grid.y).  A segment is seen as [outer][G][width][inner]: the padded side has
// width Hk and inner `inner_k`, the true side width H and inner `inner_t` (W_hh: inner H / Hk, everything else equal inners).
namespace {
struct GruPadSeg {
    const float* src;
    float* dst;
    int outer, G, inner_t, inner_k;
    int n;                                           // elements of dst
};
struct GruPadArgs {
    GruPadSeg seg[4];
    int H, Hk;
};
template <bool WIDEN>
__global__ __launch_bounds__(256) void gru_pad_kernel(GruPadArgs a) {
    const GruPadSeg sg = a.seg[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= sg.n) return;
    const int wd = WIDEN ? a.Hk : a.H, inn = WIDEN ? sg.inner_k : sg.inner_t;      // dst geometry
    const int c = i % inn;
    int r = i / inn;
    const int j = r % wd; r /= wd;                   // r = outer * G + g
    if (WIDEN) sg.dst[i] = (j < a.H && c < sg.inner_t) ? sg.src[((int64_t)r * a.H + j) * sg.inner_t + c] : 0.f;
    else sg.dst[i] = sg.src[((int64_t)r * a.Hk + j) * sg.inner_k + c];
}
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool pad_widths_ok(int H, int Hk) { return gru_ok(1, 1, Hk) && H >= 1 && H < Hk; }

template <bool WIDEN>
inline int gru_pad_launch(GruPadArgs& a, int nseg, hipStream_t s) {
    int nmax = 0;
    for (int k = 0; k < nseg; ++k) {
        GruPadSeg& sg = a.seg[k];
        const int64_t n = (int64_t)sg.outer * sg.G * (WIDEN ? a.Hk : a.H) * (WIDEN ? sg.inner_k : sg.inner_t);
        const int64_t nk = (int64_t)sg.outer * sg.G * a.Hk * sg.inner_k;
        if (!sg.src || !sg.dst || !aligned4(sg.src) || !aligned4(sg.dst) || n < 1 || nk >= ((int64_t)1 << 31) - 256) return RESEL_EINVAL;
        sg.n = (int)n;
        if (sg.n > nmax) nmax = sg.n;
    }
    hipLaunchKernelGGL(gru_pad_kernel<WIDEN>, dim3((unsigned)((nmax + 255) / 256), nseg), dim3(256), 0, s, a);
    return launch_status();
}
template <bool WIDEN>
inline int gru_pad_params(const float* w_ih, const float* b_ih, const float* w_hh, const float* b_hh,
                          float* o_w_ih, float* o_b_ih, float* o_w_hh, float* o_b_hh, int n_in, int H, int Hk, hipStream_t s) {
    if (!pad_widths_ok(H, Hk)) return RESEL_EINVAL;
    const bool none_ih = !w_ih && !b_ih && !o_w_ih && !o_b_ih;
    if (!none_ih && n_in < 1) return RESEL_EINVAL;
    GruPadArgs a{};
    a.H = H; a.Hk = Hk;
    int k = 0;
    a.seg[k++] = GruPadSeg{w_hh, o_w_hh, 1, 3, H, Hk, 0};
    a.seg[k++] = GruPadSeg{b_hh, o_b_hh, 1, 3, 1, 1, 0};
    if (!none_ih) {                                  // a partly given pair fails the NULL check of the launch
        a.seg[k++] = GruPadSeg{w_ih, o_w_ih, 1, 3, n_in, n_in, 0};
        a.seg[k++] = GruPadSeg{b_ih, o_b_ih, 1, 3, 1, 1, 0};
    }
    return gru_pad_launch<WIDEN>(a, k, s);
}
template <bool WIDEN>
inline int gru_pad_rows(const float* src, float* dst, long long rows, int G, int H, int Hk, hipStream_t s) {
    if (!pad_widths_ok(H, Hk) || rows < 1 || G < 1 || G > 4 || rows >= (1ll << 31) || rows * G * (long long)Hk >= (1ll << 31) - 256) return RESEL_EINVAL;
    GruPadArgs a{};
    a.H = H; a.Hk = Hk;
    a.seg[0] = GruPadSeg{src, dst, (int)rows, G, 1, 1, 0};
    return gru_pad_launch<WIDEN>(a, 1, s);
}
}  // namespace

extern "C" int resel_gru_pad_params(const float* w_ih, const float* b_ih, const float* w_hh, const float* b_hh,
                                    float* w_ih_k, float* b_ih_k, float* w_hh_k, float* b_hh_k, int n_in, int H, int Hk, resel_stream_t stream) {
    return gru_pad_params<true>(w_ih, b_ih, w_hh, b_hh, w_ih_k, b_ih_k, w_hh_k, b_hh_k, n_in, H, Hk, (hipStream_t)stream);
}
extern "C" int resel_gru_unpad_params(const float* dw_ih_k, const float* db_ih_k, const float* dw_hh_k, const float* db_hh_k,
                                      float* dw_ih, float* db_ih, float* dw_hh, float* db_hh, int n_in, int H, int Hk, resel_stream_t stream) {
    return gru_pad_params<false>(dw_ih_k, db_ih_k, dw_hh_k, db_hh_k, dw_ih, db_ih, dw_hh, db_hh, n_in, H, Hk, (hipStream_t)stream);
}
extern "C" int resel_gru_pad_rows(const float* src, float* dst, long long rows, int G, int H, int Hk, resel_stream_t stream) {
    return gru_pad_rows<true>(src, dst, rows, G, H, Hk, (hipStream_t)stream);
}
extern "C" int resel_gru_unpad_rows(const float* src, float* dst, long long rows, int G, int H, int Hk, resel_stream_t stream) {
    return gru_pad_rows<false>(src, dst, rows, G, H, Hk, (hipStream_t)stream);
}
