// Environment step inside a graphed policy step: the T-Maze memory task (reference envs/memory_envs/tmaze.py, `TMazeBase` with
// ambiguous positions; host twin: offpolicy_rnn/env_utils/tmaze.py) for the B rows of a batched evaluation, as the LAST node of the
// step's graph.  The kernel is the per-row body of the evaluation scheduler (utility/policy_eval.py `run_episodes` and its
// `begin()`): it reads the action index the categorical head just wrote, steps the row's environment, and writes the next
// step's input row and reset flag into the step's device block, so an evaluation is back-to-back graph replays with no host
// round trip.  One thread per row, 64-thread blocks, a few dozen scalar operations: latency of one launch, nothing to tune.
// No LDS, no atomics, nothing read from the host, no allocation: capturable.
// The training rollout has a kernel of the same shape (`tmaze_collect_kernel`, the per-row body of one iteration of `SAC._train_loop`):
// the same move / reward / observation functions on the SAMPLED index, plus the transition row the replay ring stores.
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

// The action index as the head kernel wrote it (fp32), clamped into [0, 4); NaN fails both tests: 0.
__device__ __forceinline__ int clamp_action(float af) { return af >= 3.f ? 3 : (af >= 0.f ? (int)af : 0); }

// One move of `TMaze.step`: the clock advances, the agent moves unless the target cell is off the map.  -> done
__device__ __forceinline__ bool move(const resel_tmaze_cfg_t& cfg, int32_t* st, int a) {
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
    return t >= cfg.episode_length;
}

// Reward of the step `move` just made: the host twin's expressions, one rounding each (no contraction): -0.0 survives.
__device__ __forceinline__ double reward(const resel_tmaze_cfg_t& cfg, const int32_t* st, bool done) {
    if (done) return __dmul_rn(st[SY] == st[SGOAL] ? 1.0 : 0.0, cfg.goal_reward);
    double r = __dmul_rn(st[SX] < st[ST] - cfg.oracle_length ? 1.0 : 0.0, cfg.penalty);
    if (st[SX] == 0) r = __dadd_rn(r, cfg.distract_reward);
    return r;
}

// The input row of the next policy step: lst_state <- state, state <- the new observation, lst_action <- one-hot(a), reward <- (float)r.
__device__ __forceinline__ void feed_back(const resel_tmaze_cfg_t& cfg, int32_t* st, float* in, int a, int A, double r) {
    in[2] = in[0];
    in[3] = in[1];
    observe(cfg, st, in);
    for (int c = 0; c < A; ++c) in[4 + c] = c == a ? 1.f : 0.f;
    in[4 + A] = (float)r;
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
    const int a = clamp_action(action[(int64_t)b * ld_action]);
    const bool done = move(cfg, st, a);
    const double r = reward(cfg, st, done);
    feed_back(cfg, st, in, a, A, r);
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

// ---- training rollout: one iteration of `SAC._train_loop` per replay ---------------------------------------------------------
// Columns the transition row needs: the furthest end of a present field (widths: observations 2, last action A, scalars 1).
// `action` is one column (an index) unless the caller says otherwise (a continuous action: A columns).
__device__ __host__ inline int layout_need(const resel_collect_layout_t& lay, int A, int action_width = 1) {
    const int off[11] = {lay.state, lay.last_state, lay.last_action, lay.action, lay.next_state, lay.reward,
                         lay.mask,  lay.start,      lay.done,        lay.reward_input, lay.timeout};
    const int wid[11] = {2, 2, A, action_width, 2, 1, 1, 1, 1, 1, 1};
    int need = 0;
    for (int f = 0; f < 11; ++f)
        if (off[f] >= 0 && off[f] + wid[f] > need) need = off[f] + wid[f];
    return need;
}

__device__ __forceinline__ void put(float* row, int off, const float* v, int w) {
    if (off < 0) return;                                  // a field the ring does not store
    for (int c = 0; c < w; ++c) row[off + c] = v[c];
}

__device__ __forceinline__ void put1(float* row, int off, float v) {
    if (off >= 0) row[off] = v;
}

__global__ __launch_bounds__(64) void tmaze_collect_kernel(resel_tmaze_cfg_t cfg, resel_collect_layout_t lay, int init,
                                                           const float* __restrict__ action, int64_t ld_action,
                                                           const int32_t* __restrict__ goal, int32_t* __restrict__ env_state,
                                                           double* __restrict__ ret_acc, float* __restrict__ traj, int T_cap, int64_t ld_row,
                                                           int max_episode_steps, float* __restrict__ in_block, int64_t ld_in, int B) {
    constexpr int A = 4;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int32_t* st = env_state + (int64_t)b * RESEL_TMAZE_STATE_WORDS;
    float* in = in_block + (int64_t)b * ld_in;
    if (init) {                                           // `env_reset()`: the reset observation, zero last state / last action / reward
        for (int w = 0; w < RESEL_TMAZE_STATE_WORDS; ++w) st[w] = 0;
        for (int c = 2; c < 4 + A + 1; ++c) in[c] = 0.f;
        ret_acc[b] = 0.0;
        st[SX] = cfg.oracle_length;
        st[SGOAL] = goal[b];
        st[SSTARTED] = 1;
        st[SRUNNING] = 1;
        observe(cfg, st, in);
        return;
    }
    if (!st[SRUNNING]) return;                            // the episode is over: the row waits for the host's next init, untouched
    const int a = clamp_action(action[(int64_t)b * ld_action]);
    const int len = st[SLEN];
    float before[4 + A + 1];                              // state | last_state | last_action | reward_input as the policy just saw them
    for (int c = 0; c < 4 + A + 1; ++c) before[c] = in[c];
    const bool done = move(cfg, st, a);
    const double r = reward(cfg, st, done);
    feed_back(cfg, st, in, a, A, r);
    if (len >= 0 && len < T_cap && layout_need(lay, A) <= ld_row) {       // what `SAC._push` stores, at row `len` of the episode block
        float* row = traj + ((int64_t)b * T_cap + len) * ld_row;
        put(row, lay.state, before, 2);
        put(row, lay.last_state, before + 2, 2);
        put(row, lay.last_action, before + 4, A);
        put1(row, lay.action, (float)a);
        put(row, lay.next_state, in, 2);
        put1(row, lay.reward, (float)r);
        put1(row, lay.mask, 1.f);
        put1(row, lay.start, len == 0 ? 1.f : 0.f);
        put1(row, lay.done, done ? 1.f : 0.f);
        put1(row, lay.reward_input, before[4 + A]);
        put1(row, lay.timeout, len + 1 >= max_episode_steps ? 1.f : 0.f);
    }
    ret_acc[b] = __dadd_rn(ret_acc[b], r);
    st[SLEN] = len + 1;
    if (done) st[SRUNNING] = 0;
}

// ---- Wind-v0 (reference envs/meta/toy_navigation/wind.py behind VariBadWrapper; host twin offpolicy_rnn/env_utils/wind.py) ----------
// The same two kernels for a continuous-action environment: position and wind are doubles, the action is the row's two fp32 values.
// Every operation of a step is one rounding of the width the host arithmetic has there; `contract(off)` keeps the products and sums apart.
enum { PX = 0, PY, PWX, PWY, PLX, PLY };                                  // doubles of a row of env_pos
enum { WT = 0, WLEN, WSTARTED, WRUNNING };                                // words of a row of env_words
constexpr int WA = 2, WIN = 2 * 2 + WA + 1;                               // action width; state[2] | lst_state[2] | lst_action[2] | reward[1]

// numpy's clip, minimum(maximum(x, lo), hi): a NaN fails both comparisons and passes through.
__device__ __forceinline__ double np_clip(double x, double lo, double hi) {
    x = x < lo ? lo : x;
    return x > hi ? hi : x;
}

// One component of `env.step(unorm_act(a, env.action_space))`: the new coordinate.  Plain operators: the pragma governs what is
// written here, not the bodies of the __d*_rn helpers, which would come back contractable after inlining.
__device__ __forceinline__ double wind_move(const resel_wind_cfg_t& cfg, double p, float a, double wind) {
#pragma clang fp contract(off)
    const float t = (a + 1.0f) * 0.5f;                                    // (a + 1) / 2 in fp32
    const double u = (double)t * cfg.out_span + cfg.out_low;
    const double c = np_clip(u, -1.0, 1.0);
    double v = cfg.act_low + ((c + 1.0) * 0.5) * cfg.act_span;
    v = np_clip(v, cfg.act_low, cfg.act_high);
    return (p + v) + wind;
}

// `Wind.last_reward`: 1.0 inside the goal ball; a NaN coordinate fails the comparison.
__device__ __forceinline__ double wind_reward(const resel_wind_cfg_t& cfg, const double* ps) {
#pragma clang fp contract(off)
    const double dx = ps[PX] - cfg.goal_x, dy = ps[PY] - cfg.goal_y;
    const double d = __dsqrt_rn(dx * dx + dy * dy);
    return d <= cfg.goal_radius ? 1.0 : 0.0;
}

// One `Wind.step`: the position moves, the clock advances.  -> done; *r: the reward
__device__ __forceinline__ bool wind_env_step(const resel_wind_cfg_t& cfg, double* ps, int32_t* w, const float* a, double* r) {
    ps[PLX] = ps[PX];
    ps[PLY] = ps[PY];
    ps[PX] = wind_move(cfg, ps[PX], a[0], ps[PWX]);
    ps[PY] = wind_move(cfg, ps[PY], a[1], ps[PWY]);
    const int t = w[WT] + 1;
    w[WT] = t;
    *r = wind_reward(cfg, ps);
    return t >= cfg.episode_length;
}

// The input row of the next policy step: lst_state <- state, state <- (float)position, lst_action <- a as read, reward <- (float)r.
__device__ __forceinline__ void wind_feed_back(const double* ps, float* in, const float* a, double r) {
    in[2] = in[0];
    in[3] = in[1];
    in[0] = (float)ps[PX];
    in[1] = (float)ps[PY];
    in[4] = a[0];
    in[5] = a[1];
    in[6] = (float)r;
}

// `reset(task)`: the position (and the one before it) at the origin, the episode's wind, the clock at 0.
__device__ __forceinline__ void wind_reset(const double* wind, double* ps, int32_t* w, int started) {
    ps[PX] = ps[PY] = ps[PLX] = ps[PLY] = 0.0;
    ps[PWX] = wind[0];
    ps[PWY] = wind[1];
    w[WT] = 0;
    w[WSTARTED] = started;
    w[WRUNNING] = 1;
}

// `begin()` of the scheduler for one row, as `begin_row` above: the reset observation is (0, 0) either way.
__device__ __forceinline__ void wind_begin_row(int j, int n, const double* winds_row, double* ps, int32_t* w, double* ret, float* in,
                                               int32_t* flag) {
    for (int c = 0; c < WIN; ++c) in[c] = 0.f;
    *flag = 1;
    *ret = 0.0;
    w[WLEN] = 0;
    if (j < n)
        wind_reset(winds_row + 2 * j, ps, w, j + 1);
    else
        w[WRUNNING] = 0;
}

__global__ __launch_bounds__(64) void wind_step_kernel(resel_wind_cfg_t cfg, int init, const float* __restrict__ action, int64_t ld_action,
                                                       const double* __restrict__ winds, int64_t ld_winds,
                                                       const int32_t* __restrict__ n_episodes, int J, double* __restrict__ env_pos,
                                                       int32_t* __restrict__ env_words, double* __restrict__ ret_acc,
                                                       double* __restrict__ ep_ret, int32_t* __restrict__ ep_len, int64_t ld_ep,
                                                       float* __restrict__ in_block, int64_t ld_in, int32_t* __restrict__ flags, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double* ps = env_pos + (int64_t)b * RESEL_WIND_STATE_DOUBLES;
    int32_t* w = env_words + (int64_t)b * RESEL_WIND_STATE_WORDS;
    float* in = in_block + (int64_t)b * ld_in;
    const double* winds_row = winds + (int64_t)b * ld_winds;
    const int n = min(max(n_episodes[b], 0), J);          // never past the row's J winds / result slots
    if (init) {
        for (int c = 0; c < RESEL_WIND_STATE_DOUBLES; ++c) ps[c] = 0.0;
        for (int c = 0; c < RESEL_WIND_STATE_WORDS; ++c) w[c] = 0;
        wind_begin_row(0, n, winds_row, ps, w, ret_acc + b, in, flags + b);
        return;
    }
    if (!w[WRUNNING]) {                                   // idle: zeros with the flag set
        for (int c = 0; c < WIN; ++c) in[c] = 0.f;
        flags[b] = 1;
        return;
    }
    const float a[WA] = {action[(int64_t)b * ld_action], action[(int64_t)b * ld_action + 1]};
    double r;
    const bool done = wind_env_step(cfg, ps, w, a, &r);
    wind_feed_back(ps, in, a, r);
    const double ret = __dadd_rn(ret_acc[b], r);
    ret_acc[b] = ret;
    const int len = w[WLEN] + 1;
    w[WLEN] = len;
    flags[b] = 0;
    if (done) {
        const int j = w[WSTARTED] - 1;
        if (j >= 0 && j < J) {                            // always true behind an init call
            ep_ret[(int64_t)b * ld_ep + j] = ret;
            ep_len[(int64_t)b * ld_ep + j] = len;
        }
        wind_begin_row(j + 1, n, winds_row, ps, w, ret_acc + b, in, flags + b);
    }
}

__global__ __launch_bounds__(64) void wind_collect_kernel(resel_wind_cfg_t cfg, resel_collect_layout_t lay, int init,
                                                          const float* __restrict__ action, int64_t ld_action,
                                                          const double* __restrict__ wind, double* __restrict__ env_pos,
                                                          int32_t* __restrict__ env_words, double* __restrict__ ret_acc,
                                                          float* __restrict__ traj, int T_cap, int64_t ld_row, int max_episode_steps,
                                                          float* __restrict__ in_block, int64_t ld_in, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double* ps = env_pos + (int64_t)b * RESEL_WIND_STATE_DOUBLES;
    int32_t* w = env_words + (int64_t)b * RESEL_WIND_STATE_WORDS;
    float* in = in_block + (int64_t)b * ld_in;
    if (init) {                                           // `env_reset()`: the reset observation, zero last state / last action / reward
        for (int c = 0; c < RESEL_WIND_STATE_WORDS; ++c) w[c] = 0;
        for (int c = 0; c < WIN; ++c) in[c] = 0.f;
        ret_acc[b] = 0.0;
        wind_reset(wind + (int64_t)b * 2, ps, w, 1);
        return;
    }
    if (!w[WRUNNING]) return;                             // the episode is over: the row waits for the host's next init, untouched
    const float a[WA] = {action[(int64_t)b * ld_action], action[(int64_t)b * ld_action + 1]};
    const int len = w[WLEN];
    float before[WIN];                                    // state | last_state | last_action | reward_input as the policy just saw them
    for (int c = 0; c < WIN; ++c) before[c] = in[c];
    double r;
    const bool done = wind_env_step(cfg, ps, w, a, &r);
    wind_feed_back(ps, in, a, r);
    if (len >= 0 && len < T_cap && layout_need(lay, WA, WA) <= ld_row) {   // what `SAC._push` stores, at row `len` of the episode block
        float* row = traj + ((int64_t)b * T_cap + len) * ld_row;
        put(row, lay.state, before, 2);
        put(row, lay.last_state, before + 2, 2);
        put(row, lay.last_action, before + 4, WA);
        put(row, lay.action, a, WA);
        put(row, lay.next_state, in, 2);
        put1(row, lay.reward, (float)r);
        put1(row, lay.mask, 1.f);
        put1(row, lay.start, len == 0 ? 1.f : 0.f);
        put1(row, lay.done, done ? 1.f : 0.f);
        put1(row, lay.reward_input, before[4 + WA]);
        put1(row, lay.timeout, len + 1 >= max_episode_steps ? 1.f : 0.f);
    }
    ret_acc[b] = __dadd_rn(ret_acc[b], r);
    w[WLEN] = len + 1;
    if (done) w[WRUNNING] = 0;
}

// A cfg the Wind entries refuse: a NaN anywhere fails its comparison.
inline bool wind_cfg_bad(const resel_wind_cfg_t& c) {
    return c.episode_length < 1 || !(c.goal_radius >= 0.0) || !(c.act_low <= c.act_high) || c.goal_x != c.goal_x || c.goal_y != c.goal_y ||
           c.act_span != c.act_span || c.out_low != c.out_low || c.out_span != c.out_span;
}

}  // namespace

extern "C" {

int resel_tmaze_collect_step(resel_tmaze_cfg_t cfg, resel_collect_layout_t lay, int init, const float* action, int64_t ld_action,
                             const int32_t* goal, int32_t* env_state, double* ret_acc, float* traj, int T_cap, int64_t ld_row,
                             int max_episode_steps, float* in_block, int64_t ld_in, int A, int B, resel_stream_t stream) {
    if (!action || !goal || !env_state || !ret_acc || !traj || !in_block) return RESEL_EINVAL;
    if (A != 4 || B < 0 || ld_in < 2 * 2 + A + 1 || ld_action < 1 || T_cap < 1 || max_episode_steps < 1) return RESEL_EINVAL;
    if (cfg.corridor_length < 1 || cfg.oracle_length < 0 || cfg.episode_length < 1 || !(cfg.penalty <= 0.0)) return RESEL_EINVAL;
    if (lay.logp >= 0 || ld_row < 1 || layout_need(lay, A) > ld_row) return RESEL_EINVAL;
    if (B == 0) return RESEL_OK;
    hipLaunchKernelGGL(tmaze_collect_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cfg, lay, init, action, ld_action,
                       goal, env_state, ret_acc, traj, T_cap, ld_row, max_episode_steps, in_block, ld_in, B);
    return launch_status();
}

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

int resel_wind_step(resel_wind_cfg_t cfg, int init, const float* action, int64_t ld_action, const double* winds, int64_t ld_winds,
                    const int32_t* n_episodes, int J, double* env_pos, int32_t* env_words, double* ret_acc, double* ep_ret, int32_t* ep_len,
                    int64_t ld_ep, float* in_block, int64_t ld_in, int A, int32_t* flags, int B, resel_stream_t stream) {
    if (!action || !winds || !n_episodes || !env_pos || !env_words || !ret_acc || !ep_ret || !ep_len || !in_block || !flags) return RESEL_EINVAL;
    if (A != WA || B < 0 || ld_in < WIN || ld_action < WA || J < 1 || ld_winds < 2 * (int64_t)J || ld_ep < J) return RESEL_EINVAL;
    if (wind_cfg_bad(cfg)) return RESEL_EINVAL;
    if (B == 0) return RESEL_OK;
    hipLaunchKernelGGL(wind_step_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cfg, init, action, ld_action, winds, ld_winds,
                       n_episodes, J, env_pos, env_words, ret_acc, ep_ret, ep_len, ld_ep, in_block, ld_in, flags, B);
    return launch_status();
}

int resel_wind_collect_step(resel_wind_cfg_t cfg, resel_collect_layout_t lay, int init, const float* action, int64_t ld_action,
                            const double* wind, double* env_pos, int32_t* env_words, double* ret_acc, float* traj, int T_cap, int64_t ld_row,
                            int max_episode_steps, float* in_block, int64_t ld_in, int A, int B, resel_stream_t stream) {
    if (!action || !wind || !env_pos || !env_words || !ret_acc || !traj || !in_block) return RESEL_EINVAL;
    if (A != WA || B < 0 || ld_in < WIN || ld_action < WA || T_cap < 1 || max_episode_steps < 1) return RESEL_EINVAL;
    if (wind_cfg_bad(cfg)) return RESEL_EINVAL;
    if (lay.logp >= 0 || ld_row < 1 || layout_need(lay, WA, WA) > ld_row) return RESEL_EINVAL;
    if (B == 0) return RESEL_OK;
    hipLaunchKernelGGL(wind_collect_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cfg, lay, init, action, ld_action, wind,
                       env_pos, env_words, ret_acc, traj, T_cap, ld_row, max_episode_steps, in_block, ld_in, B);
    return launch_status();
}

}  // extern "C"
