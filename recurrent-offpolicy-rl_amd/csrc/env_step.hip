// Environment step inside a graphed policy step: the T-Maze memory task (reference envs/memory_envs/tmaze.py, `TMazeBase` with
// ambiguous positions; host twin: offpolicy_rnn/env_utils/tmaze.py) for the B rows of a batched evaluation, as the LAST node of the
// step's graph.  The kernel is the per-row body of the evaluation scheduler (utility/policy_eval.py `run_episodes` and its
// `begin()`): it reads the action index the categorical head just wrote, steps the row's environment, and writes the next
// step's input row and reset flag into the step's device block, so an evaluation is back-to-back graph replays with no host
// round trip.  One thread per row, 64-thread blocks, a few dozen scalar operations: latency of one launch, nothing to tune.
// No LDS, no atomics, nothing read from the host, no allocation: capturable.
#include "resel_common.h"

namespace {
using namespace resel;

enum { SX = 0, SY, SGOAL, SVISITED, ST, SLEN, SSTARTED, SRUNNING };       // words of a row of env_state

// Observation of the cell (x, y): the oracle at x = 0 shows the goal side once per episode.
__device__ __forceinline__ void observe(const resel_tmaze_cfg_t& cfg, int32_t* st, float* obs) {
    const int x = st[SX];
    if (x == 0) {
        obs[0] = 0.f;
        obs[1] = st[SVISITED] ? 0.f : (float)st[SGOAL];
        st[SVISITED] = 1;
    } else if (x < cfg.oracle_length + cfg.corridor_length) {
        obs[0] = 0.f;
        obs[1] = 0.f;
    } else {
        obs[0] = 1.f;
        obs[1] = (float)st[SY];
    }
}

// `begin()` of the scheduler for one row: zero last state / last action / reward, flag set, and either the reset observation of
// episode j or, when the row has run all of its episodes, a zero state and an idle row.
__device__ __forceinline__ void begin_row(const resel_tmaze_cfg_t& cfg, int j, int n, const int32_t* goals_row, int32_t* st, double* ret,
                                          float* in, int A, int32_t* flag) {
    for (int c = 2; c < 4 + A + 1; ++c) in[c] = 0.f;
    *flag = 1;
    *ret = 0.0;
    st[SLEN] = 0;
    if (j < n) {
        st[SX] = cfg.oracle_length;
        st[SY] = 0;
        st[SGOAL] = goals_row[j];
        st[SVISITED] = 0;
        st[ST] = 0;
        st[SSTARTED] = j + 1;
        st[SRUNNING] = 1;
        observe(cfg, st, in);
    } else {
        st[SRUNNING] = 0;
        in[0] = 0.f;
        in[1] = 0.f;
    }
}

__global__ __launch_bounds__(64) void tmaze_step_kernel(resel_tmaze_cfg_t cfg, int init, const float* __restrict__ action, int64_t ld_action,
                                                        const int32_t* __restrict__ goals, int64_t ld_goals,
                                                        const int32_t* __restrict__ n_episodes, int J, int32_t* __restrict__ env_state,
                                                        double* __restrict__ ret_acc, double* __restrict__ ep_ret,
                                                        int32_t* __restrict__ ep_len, int64_t ld_ep, float* __restrict__ in_block,
                                                        int64_t ld_in, int A, int32_t* __restrict__ flags, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int32_t* st = env_state + (int64_t)b * RESEL_TMAZE_STATE_WORDS;
    float* in = in_block + (int64_t)b * ld_in;
    const int32_t* goals_row = goals + (int64_t)b * ld_goals;
    const int n = min(max(n_episodes[b], 0), J);        // never past the row's J goals / result slots
    if (init) {
        for (int w = 0; w < RESEL_TMAZE_STATE_WORDS; ++w) st[w] = 0;
        begin_row(cfg, 0, n, goals_row, st, ret_acc + b, in, A, flags + b);
        return;
    }
    if (!st[SRUNNING]) {                                  // idle: zeros with the flag set, so a cgpt position never runs away
        for (int c = 0; c < 4 + A + 1; ++c) in[c] = 0.f;
        flags[b] = 1;
        return;
    }
    const float af = action[(int64_t)b * ld_action];
    const int a = af >= 3.f ? 3 : (af >= 0.f ? (int)af : 0);             // clamp into [0, 4); NaN fails both tests: 0
    const int t = st[ST] + 1;
    int x = st[SX], y = st[SY];
    const int nx = x + (a == 0) - (a == 2), ny = y + (a == 1) - (a == 3);
    const int end = cfg.oracle_length + cfg.corridor_length;
    if ((ny == 0 && nx >= 0 && nx <= end) || (nx == end && (ny == 1 || ny == -1))) {
        x = nx;
        y = ny;
    }
    st[ST] = t;
    st[SX] = x;
    st[SY] = y;
    const bool done = t >= cfg.episode_length;
    double r;                                             // the host twin's expressions, one rounding each (no contraction): -0.0 survives
    if (done) {
        r = __dmul_rn(y == st[SGOAL] ? 1.0 : 0.0, cfg.goal_reward);
    } else {
        r = __dmul_rn(x < t - cfg.oracle_length ? 1.0 : 0.0, cfg.penalty);
        if (x == 0) r = __dadd_rn(r, cfg.distract_reward);
    }
    in[2] = in[0];
    in[3] = in[1];
    observe(cfg, st, in);
    for (int c = 0; c < A; ++c) in[4 + c] = c == a ? 1.f : 0.f;
    in[4 + A] = (float)r;
    const double ret = __dadd_rn(ret_acc[b], r);
    ret_acc[b] = ret;
    const int len = st[SLEN] + 1;
    st[SLEN] = len;
    flags[b] = 0;
    if (done) {
        const int j = st[SSTARTED] - 1;
        if (j >= 0 && j < J) {                            // always true behind an init call
            ep_ret[(int64_t)b * ld_ep + j] = ret;
            ep_len[(int64_t)b * ld_ep + j] = len;
        }
        begin_row(cfg, j + 1, n, goals_row, st, ret_acc + b, in, A, flags + b);
    }
}

}  // namespace

extern "C" {

int resel_tmaze_step(resel_tmaze_cfg_t cfg, int init, const float* action, int64_t ld_action, const int32_t* goals, int64_t ld_goals,
                     const int32_t* n_episodes, int J, int32_t* env_state, double* ret_acc, double* ep_ret, int32_t* ep_len, int64_t ld_ep,
                     float* in_block, int64_t ld_in, int A, int32_t* flags, int B, resel_stream_t stream) {
    if (!action || !goals || !n_episodes || !env_state || !ret_acc || !ep_ret || !ep_len || !in_block || !flags) return RESEL_EINVAL;
    if (A != 4 || B < 0 || ld_in < 2 * 2 + A + 1 || ld_action < 1 || J < 1 || ld_goals < J || ld_ep < J) return RESEL_EINVAL;
    if (cfg.corridor_length < 1 || cfg.oracle_length < 0 || cfg.episode_length < 1 || !(cfg.penalty <= 0.0)) return RESEL_EINVAL;
    if (B == 0) return RESEL_OK;
    hipLaunchKernelGGL(tmaze_step_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cfg, init, action, ld_action, goals,
                       ld_goals, n_episodes, J, env_state, ret_acc, ep_ret, ep_len, ld_ep, in_block, ld_in, A, flags, B);
    return launch_status();
}

}  // extern "C"
