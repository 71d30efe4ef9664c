// Environment step inside a graphed policy step, as the LAST node of the step's graph: the kernel reads the action the policy head just
// wrote, steps the row's environment, and writes the next step's input row into the step's device block, so an evaluation or a rollout
// is back-to-back graph replays with no host round trip.  Two kernel templates over an environment record:
//   `eval_step_kernel`     the per-row body of the evaluation scheduler (utility/policy_eval.py `run_episodes` and its `begin()`);
//   `collect_step_kernel`  the per-row body of one iteration of `SAC._train_loop`: the same step on the SAMPLED action, plus the
//                          transition row the replay ring stores.
// A record (`TMazeEnv`, `WindEnv`, `CatchEnv`) holds what is specific to one environment - state, payload, action, arithmetic, widths -
// and no scheduling.  One thread per row, 64-thread blocks, a few dozen scalar operations plus the row's columns (9 or 7 floats, 102 for
// Catch): latency of one launch, nothing to tune.  No LDS, no atomics, nothing read from the host, no allocation: capturable.
//
// Adding an environment: one record below with the members the three here have, two `extern "C"` entries that instantiate the templates
// (prototypes, cfg struct and state-size constants in include/resel_hip.h, mirrored in hip/_lib.py), two wrappers in hip/ops.py, a
// record in env_utils/device_env.py, and a host twin to compare against bit for bit.  `Env::step` sees the state and the cfg only: an
// environment that needs its payload in mid-episode (Catch) copies it into its state in `reset`.  NPAY is a compile-time constant: a
// payload of varying length is a fixed-capacity row with an unused tail.
#include "resel_common.h"

namespace {
using namespace resel;

// The three words every environment keeps next to its own state, consecutive int32 at `Env::book(state)`.
enum { BLEN = 0, BSTARTED, BRUNNING };                                    // steps of the episode, episodes started, running

// ---- T-Maze memory task (reference envs/memory_envs/tmaze.py, `TMazeBase` with ambiguous positions; host twin env_utils/tmaze.py) -------
struct TMazeEnv {
    using Cfg = resel_tmaze_cfg_t;
    using State = int32_t*;                                               // base of env_state, or one row of it
    using Payload = int32_t;                                              // the goal side of an episode
    using Action = int;                                                   // the clamped index
    static constexpr int NPAY = 1, OBS = 2, LAST_ACTION = 4, ACTION = 1, IN = 2 * OBS + LAST_ACTION + 1;
    enum { SX = 0, SY, SGOAL, SVISITED, ST, SBOOK };                      // words of a row of env_state; SBOOK: the bookkeeping trio

    static bool cfg_bad(const Cfg& c) { return c.corridor_length < 1 || c.oracle_length < 0 || c.episode_length < 1 || !(c.penalty <= 0.0); }
    static bool null(State s) { return !s; }
    __device__ static State row(State base, int b) { return base + (int64_t)b * RESEL_TMAZE_STATE_WORDS; }
    __device__ static int32_t* book(State st) { return st + SBOOK; }

    __device__ static void clear(State st) {
        for (int w = 0; w < RESEL_TMAZE_STATE_WORDS; ++w) st[w] = 0;
    }

    // `reset()`: the agent at the corridor's start, the oracle unvisited, the clock at 0.
    __device__ static void reset(const Cfg& cfg, State st, const Payload* goal, int started) {
        st[SX] = cfg.oracle_length;
        st[SY] = 0;
        st[SGOAL] = goal[0];
        st[SVISITED] = 0;
        st[ST] = 0;
        st[SBOOK + BSTARTED] = started;
        st[SBOOK + BRUNNING] = 1;
    }

    // Observation of the cell (x, y): the oracle at x = 0 shows the goal side once per episode.
    __device__ static void observe(const Cfg& cfg, State st, float* obs) {
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
    __device__ static int clamp_action(float af) { return af >= 3.f ? 3 : (af >= 0.f ? (int)af : 0); }
    __device__ static Action read_action(const float* a) { return clamp_action(a[0]); }

    // One move of `TMaze.step`: the clock advances, the agent moves unless the target cell is off the map.  -> done
    __device__ static bool move(const Cfg& cfg, State st, int a) {
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
    __device__ static double reward(const Cfg& cfg, const int32_t* st, bool done) {
        if (done) return __dmul_rn(st[SY] == st[SGOAL] ? 1.0 : 0.0, cfg.goal_reward);
        double r = __dmul_rn(st[SX] < st[ST] - cfg.oracle_length ? 1.0 : 0.0, cfg.penalty);
        if (st[SX] == 0) r = __dadd_rn(r, cfg.distract_reward);
        return r;
    }

    __device__ static bool step(const Cfg& cfg, State st, Action a, double* r) {
        const bool done = move(cfg, st, a);
        *r = reward(cfg, st, done);
        return done;
    }

    __device__ static void last_action(Action a, float* out) {           // one-hot(a)
        for (int c = 0; c < LAST_ACTION; ++c) out[c] = c == a ? 1.f : 0.f;
    }
    __device__ static void ring_action(Action a, float* out) { out[0] = (float)a; }
};

// ---- Wind-v0 (reference envs/meta/toy_navigation/wind.py behind VariBadWrapper; host twin env_utils/wind.py) -----------------------
// A continuous-action environment: position and wind are doubles, the action is the row's two fp32 values.  Every operation of a step
// is one rounding of the width the host arithmetic has there; `contract(off)` keeps the products and sums apart.
struct WindEnv {
    using Cfg = resel_wind_cfg_t;
    struct State {                                                        // bases of env_pos and env_words, or one row of each
        double* ps;
        int32_t* w;
    };
    using Payload = double;                                               // the wind vector of an episode
    struct Action {                                                       // the two values as read (bits kept)
        float v[2];
    };
    static constexpr int NPAY = 2, OBS = 2, LAST_ACTION = 2, ACTION = 2, IN = 2 * OBS + LAST_ACTION + 1;
    enum { PX = 0, PY, PWX, PWY, PLX, PLY };                              // doubles of a row of env_pos
    enum { WT = 0, WBOOK };                                               // words of a row of env_words; WBOOK: the bookkeeping trio

    // A cfg the entries refuse: a NaN anywhere fails its comparison.
    static bool cfg_bad(const Cfg& c) {
        return c.episode_length < 1 || !(c.goal_radius >= 0.0) || !(c.act_low <= c.act_high) || c.goal_x != c.goal_x || c.goal_y != c.goal_y ||
               c.act_span != c.act_span || c.out_low != c.out_low || c.out_span != c.out_span;
    }
    static bool null(State s) { return !s.ps || !s.w; }
    __device__ static State row(State base, int b) {
        return {base.ps + (int64_t)b * RESEL_WIND_STATE_DOUBLES, base.w + (int64_t)b * RESEL_WIND_STATE_WORDS};
    }
    __device__ static int32_t* book(State st) { return st.w + WBOOK; }

    __device__ static void clear(State st) {
        for (int c = 0; c < RESEL_WIND_STATE_DOUBLES; ++c) st.ps[c] = 0.0;
        for (int c = 0; c < RESEL_WIND_STATE_WORDS; ++c) st.w[c] = 0;
    }

    // `reset(task)`: the position (and the one before it) at the origin, the episode's wind, the clock at 0.
    __device__ static void reset(const Cfg&, State st, const Payload* wind, int started) {
        double* ps = st.ps;
        ps[PX] = ps[PY] = ps[PLX] = ps[PLY] = 0.0;
        ps[PWX] = wind[0];
        ps[PWY] = wind[1];
        st.w[WT] = 0;
        st.w[WBOOK + BSTARTED] = started;
        st.w[WBOOK + BRUNNING] = 1;
    }

    __device__ static void observe(const Cfg&, State st, float* obs) {   // (float)position
        obs[0] = (float)st.ps[PX];
        obs[1] = (float)st.ps[PY];
    }

    __device__ static Action read_action(const float* a) { return {{a[0], a[1]}}; }

    // numpy's clip, minimum(maximum(x, lo), hi): a NaN fails both comparisons and passes through.
    __device__ static double np_clip(double x, double lo, double hi) {
        x = x < lo ? lo : x;
        return x > hi ? hi : x;
    }

    // One component of `env.step(unorm_act(a, env.action_space))`: the new coordinate.  Plain operators: the pragma governs what is
    // written here, not the bodies of the __d*_rn helpers, which would come back contractable after inlining.
    __device__ static double wind_move(const Cfg& cfg, double p, float a, double wind) {
#pragma clang fp contract(off)
        const float t = (a + 1.0f) * 0.5f;                                // (a + 1) / 2 in fp32
        const double u = (double)t * cfg.out_span + cfg.out_low;
        const double c = np_clip(u, -1.0, 1.0);
        double v = cfg.act_low + ((c + 1.0) * 0.5) * cfg.act_span;
        v = np_clip(v, cfg.act_low, cfg.act_high);
        return (p + v) + wind;
    }

    // `Wind.last_reward`: 1.0 inside the goal ball; a NaN coordinate fails the comparison.
    __device__ static double wind_reward(const Cfg& cfg, const double* ps) {
#pragma clang fp contract(off)
        const double dx = ps[PX] - cfg.goal_x, dy = ps[PY] - cfg.goal_y;
        const double d = __dsqrt_rn(dx * dx + dy * dy);
        return d <= cfg.goal_radius ? 1.0 : 0.0;
    }

    // One `Wind.step`: the position moves, the clock advances.  -> done; *r: the reward
    __device__ static bool step(const Cfg& cfg, State st, Action a, double* r) {
        double* ps = st.ps;
        ps[PLX] = ps[PX];
        ps[PLY] = ps[PY];
        ps[PX] = wind_move(cfg, ps[PX], a.v[0], ps[PWX]);
        ps[PY] = wind_move(cfg, ps[PY], a.v[1], ps[PWY]);
        const int t = st.w[WT] + 1;
        st.w[WT] = t;
        *r = wind_reward(cfg, ps);
        return t >= cfg.episode_length;
    }

    __device__ static void last_action(Action a, float* out) {
        out[0] = a.v[0];
        out[1] = a.v[1];
    }
    __device__ static void ring_action(Action a, float* out) { last_action(a, out); }
};

// ---- Catch-<runs>-v0 (reference envs/credit_assign/catch.py `DelayedCatch`; host twin env_utils/catch.py) ------------------------------
// Integer state, a 49-wide observation, and a per-episode payload that is a table: the fruit and basket columns of every run.
// `step` sees no payload, so `reset` copies the episode's draws into the row's state and a soft reset reads them from there.
struct CatchEnv {
    using Cfg = resel_catch_cfg_t;
    using State = int32_t*;                                               // base of env_state, or one row of it
    using Payload = int32_t;                                              // ns[MAX_RUNS] | ms[MAX_RUNS] of an episode
    using Action = int;                                                   // the clamped index
    static constexpr int GRID = 7, MAX_RUNS = RESEL_CATCH_MAX_RUNS;
    static constexpr int NPAY = 2 * MAX_RUNS, OBS = GRID * GRID, LAST_ACTION = 3, ACTION = 1, IN = 2 * OBS + LAST_ACTION + 1;
    // words of a row of env_state; SBOOK: the bookkeeping trio, SPAD keeps the row a multiple of 8 bytes
    enum { SROW = 0, SCOL, SBASKET, SCOUNT, ST, SACC, SBOOK, SPAD = SBOOK + 3, SNS, SMS = SNS + MAX_RUNS, SWORDS = SMS + MAX_RUNS };
    static_assert(SWORDS == RESEL_CATCH_STATE_WORDS && SWORDS % 2 == 0, "the header's row of state words");

    static bool cfg_bad(const Cfg& c) {
        return c.num_catches < 1 || c.num_catches > MAX_RUNS || c.episode_length != GRID * c.num_catches - 1;
    }
    static bool null(State s) { return !s; }
    __device__ static State row(State base, int b) { return base + (int64_t)b * SWORDS; }
    __device__ static int32_t* book(State st) { return st + SBOOK; }
    __device__ static int cell(int v) { return min(max(v, 0), GRID - 1); }       // a row / column of the grid, whatever the word holds

    __device__ static void clear(State st) {
        for (int w = 0; w < SWORDS; ++w) st[w] = 0;
    }

    // `reset()`: the episode's draws into the state, the first fruit and basket in place, nothing caught, the clock at 0.
    __device__ static void reset(const Cfg&, State st, const Payload* draws, int started) {
        for (int k = 0; k < NPAY; ++k) st[SNS + k] = draws[k];
        st[SROW] = 0;
        st[SCOL] = draws[0];
        st[SBASKET] = draws[MAX_RUNS];
        st[SCOUNT] = 1;
        st[ST] = 0;
        st[SACC] = 0;
        st[SBOOK + BSTARTED] = started;
        st[SBOOK + BRUNNING] = 1;
    }

    // The flattened canvas: -1 at the fruit, then +1 at the basket in the last row (it covers a fruit in its cell).
    __device__ static void observe(const Cfg&, State st, float* obs) {
#pragma unroll
        for (int c = 0; c < OBS; ++c) obs[c] = 0.f;
        obs[GRID * cell(st[SROW]) + cell(st[SCOL])] = -1.f;
        obs[GRID * (GRID - 1) + cell(st[SBASKET])] = 1.f;
    }

    // The action index as the head kernel wrote it (fp32), clamped into [0, 3); NaN fails both tests: 0.
    __device__ static int clamp_action(float af) { return af >= 2.f ? 2 : (af >= 0.f ? (int)af : 0); }
    __device__ static Action read_action(const float* a) { return clamp_action(a[0]); }

    // One `DelayedCatch.step`: the clock advances; a fruit in the last row is replaced (the action is ignored), any other falls one
    // row while the basket moves.  Every reward but the last step's is 0; the last pays the catches.  -> done
    __device__ static bool step(const Cfg& cfg, State st, Action a, double* r) {
        const int t = st[ST] + 1;
        st[ST] = t;
        *r = 0.0;
        if (st[SROW] >= GRID - 1) {                       // soft reset; the count is clamped: a corrupted word reads inside the draws
            const int k = min(max(st[SCOUNT], 0), cfg.num_catches - 1);
            st[SROW] = 0;
            st[SCOL] = st[SNS + k];
            st[SBASKET] = st[SMS + k];
            st[SCOUNT] = k + 1;
            return false;
        }
        const int basket = cell(st[SBASKET] + a - 1), fruit_row = st[SROW] + 1;
        st[SBASKET] = basket;
        st[SROW] = fruit_row;
        int acc = st[SACC];
        if (fruit_row == GRID - 1 && st[SCOL] == basket) st[SACC] = ++acc;
        const bool done = t >= cfg.episode_length;
        if (done) *r = (double)acc;
        return done;
    }

    __device__ static void last_action(Action a, float* out) {           // one-hot(a)
        for (int c = 0; c < LAST_ACTION; ++c) out[c] = c == a ? 1.f : 0.f;
    }
    __device__ static void ring_action(Action a, float* out) { out[0] = (float)a; }
};

// ---- what the two kernels share ---------------------------------------------------------------------------------------------------
// One environment step of a running row and the input row of the next policy step: lst_state <- state, state <- the new observation,
// lst_action <- the action in the environment's form, reward <- (float)r.  -> done
template <class Env>
__device__ __forceinline__ bool step_row(const typename Env::Cfg& cfg, typename Env::State st, typename Env::Action a, float* in, double* r) {
    const bool done = Env::step(cfg, st, a, r);
#pragma unroll
    for (int c = 0; c < Env::OBS; ++c) in[Env::OBS + c] = in[c];
    Env::observe(cfg, st, in);
    Env::last_action(a, in + 2 * Env::OBS);
    in[Env::IN - 1] = (float)*r;
    return done;
}

// ---- evaluation: `begin()` of the scheduler for one row: zero last state / last action / reward, flag set, and either the reset
// observation of episode j or, when the row has run all of its episodes, a zero state and an idle row.
template <class Env>
__device__ __forceinline__ void begin_row(const typename Env::Cfg& cfg, int j, int n, const typename Env::Payload* payload_row,
                                          typename Env::State st, double* ret, float* in, int32_t* flag) {
#pragma unroll
    for (int c = Env::OBS; c < Env::IN; ++c) in[c] = 0.f;
    *flag = 1;
    *ret = 0.0;
    int32_t* book = Env::book(st);
    book[BLEN] = 0;
    if (j < n) {
        Env::reset(cfg, st, payload_row + Env::NPAY * j, j + 1);
        Env::observe(cfg, st, in);
    } else {
        book[BRUNNING] = 0;
#pragma unroll
        for (int c = 0; c < Env::OBS; ++c) in[c] = 0.f;
    }
}

template <class Env>
__global__ __launch_bounds__(64) void eval_step_kernel(typename Env::Cfg cfg, int init, const float* __restrict__ action, int64_t ld_action,
                                                       const typename Env::Payload* __restrict__ payload, int64_t ld_payload,
                                                       const int32_t* __restrict__ n_episodes, int J, typename Env::State state,
                                                       double* __restrict__ ret_acc, double* __restrict__ ep_ret,
                                                       int32_t* __restrict__ ep_len, int64_t ld_ep, float* __restrict__ in_block,
                                                       int64_t ld_in, int32_t* __restrict__ flags, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const typename Env::State st = Env::row(state, b);
    int32_t* book = Env::book(st);
    float* in = in_block + (int64_t)b * ld_in;
    const typename Env::Payload* payload_row = payload + (int64_t)b * ld_payload;
    const int n = min(max(n_episodes[b], 0), J);          // never past the row's J payloads / result slots
    if (init) {
        Env::clear(st);
        begin_row<Env>(cfg, 0, n, payload_row, st, ret_acc + b, in, flags + b);
        return;
    }
    if (!book[BRUNNING]) {                                // idle: zeros with the flag set, so a cgpt position never runs away
#pragma unroll
        for (int c = 0; c < Env::IN; ++c) in[c] = 0.f;
        flags[b] = 1;
        return;
    }
    double r;
    const bool done = step_row<Env>(cfg, st, Env::read_action(action + (int64_t)b * ld_action), in, &r);
    const double ret = __dadd_rn(ret_acc[b], r);
    ret_acc[b] = ret;
    const int len = book[BLEN] + 1;
    book[BLEN] = len;
    flags[b] = 0;
    if (done) {
        const int j = book[BSTARTED] - 1;
        if (j >= 0 && j < J) {                            // always true behind an init call
            ep_ret[(int64_t)b * ld_ep + j] = ret;
            ep_len[(int64_t)b * ld_ep + j] = len;
        }
        begin_row<Env>(cfg, j + 1, n, payload_row, st, ret_acc + b, in, flags + b);
    }
}

// ---- training rollout: one iteration of `SAC._train_loop` per replay ---------------------------------------------------------
// Columns the transition row needs: the furthest end of a present field (widths: observations, last action and action of Env, scalars 1).
template <class Env>
__device__ __host__ inline int layout_need(const resel_collect_layout_t& lay) {
    const int off[11] = {lay.state, lay.last_state, lay.last_action, lay.action, lay.next_state, lay.reward,
                         lay.mask,  lay.start,      lay.done,        lay.reward_input, lay.timeout};
    const int wid[11] = {Env::OBS, Env::OBS, Env::LAST_ACTION, Env::ACTION, Env::OBS, 1, 1, 1, 1, 1, 1};
    int need = 0;
    for (int f = 0; f < 11; ++f)
        if (off[f] >= 0 && off[f] + wid[f] > need) need = off[f] + wid[f];
    return need;
}

template <int W>
__device__ __forceinline__ void put(float* row, int off, const float* v) {
    if (off < 0) return;                                  // a field the ring does not store
#pragma unroll
    for (int c = 0; c < W; ++c) row[off + c] = v[c];
}

__device__ __forceinline__ void put1(float* row, int off, float v) {
    if (off >= 0) row[off] = v;
}

template <class Env>
__global__ __launch_bounds__(64) void collect_step_kernel(typename Env::Cfg cfg, resel_collect_layout_t lay, int init,
                                                          const float* __restrict__ action, int64_t ld_action,
                                                          const typename Env::Payload* __restrict__ payload, typename Env::State state,
                                                          double* __restrict__ ret_acc, float* __restrict__ traj, int T_cap, int64_t ld_row,
                                                          int max_episode_steps, float* __restrict__ in_block, int64_t ld_in, int B) {
    constexpr int OBS = Env::OBS, IN = Env::IN;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const typename Env::State st = Env::row(state, b);
    int32_t* book = Env::book(st);
    float* in = in_block + (int64_t)b * ld_in;
    if (init) {                                           // `env_reset()`: the reset observation, zero last state / last action / reward
        Env::clear(st);
#pragma unroll
        for (int c = OBS; c < IN; ++c) in[c] = 0.f;
        ret_acc[b] = 0.0;
        Env::reset(cfg, st, payload + (int64_t)b * Env::NPAY, 1);
        Env::observe(cfg, st, in);
        return;
    }
    if (!book[BRUNNING]) return;                          // the episode is over: the row waits for the host's next init, untouched
    const typename Env::Action a = Env::read_action(action + (int64_t)b * ld_action);
    const int len = book[BLEN];
    float before[IN];                                     // state | last_state | last_action | reward_input as the policy just saw them
#pragma unroll
    for (int c = 0; c < IN; ++c) before[c] = in[c];
    double r;
    const bool done = step_row<Env>(cfg, st, a, in, &r);
    if (len >= 0 && len < T_cap && layout_need<Env>(lay) <= ld_row) {     // what `SAC._push` stores, at row `len` of the episode block
        float* row = traj + ((int64_t)b * T_cap + len) * ld_row;
        float act[Env::ACTION];
        Env::ring_action(a, act);
        put<OBS>(row, lay.state, before);
        put<OBS>(row, lay.last_state, before + OBS);
        put<Env::LAST_ACTION>(row, lay.last_action, before + 2 * OBS);
        put<Env::ACTION>(row, lay.action, act);
        put<OBS>(row, lay.next_state, in);
        put1(row, lay.reward, (float)r);
        put1(row, lay.mask, 1.f);
        put1(row, lay.start, len == 0 ? 1.f : 0.f);
        put1(row, lay.done, done ? 1.f : 0.f);
        put1(row, lay.reward_input, before[IN - 1]);
        put1(row, lay.timeout, len + 1 >= max_episode_steps ? 1.f : 0.f);
    }
    ret_acc[b] = __dadd_rn(ret_acc[b], r);
    book[BLEN] = len + 1;
    if (done) book[BRUNNING] = 0;
}

// ---- the entries: argument checks, then one launch ----------------------------------------------------------------------------------
// What every entry refuses: a null row block, a width or stride the environment cannot step with, a bad cfg.
template <class Env>
bool rows_bad(const typename Env::Cfg& cfg, const float* action, const void* payload, typename Env::State state, const double* ret_acc,
              const float* in_block, int64_t ld_action, int64_t ld_in, int A, int B) {
    return !action || !payload || Env::null(state) || !ret_acc || !in_block || A != Env::LAST_ACTION || B < 0 || ld_in < Env::IN ||
           ld_action < Env::ACTION || Env::cfg_bad(cfg);
}

template <class Env>
int eval_step(typename Env::Cfg cfg, int init, const float* action, int64_t ld_action, const typename Env::Payload* payload,
              int64_t ld_payload, const int32_t* n_episodes, int J, typename Env::State state, double* ret_acc, double* ep_ret,
              int32_t* ep_len, int64_t ld_ep, float* in_block, int64_t ld_in, int A, int32_t* flags, int B, resel_stream_t stream) {
    if (rows_bad<Env>(cfg, action, payload, state, ret_acc, in_block, ld_action, ld_in, A, B)) return RESEL_EINVAL;
    if (!n_episodes || !ep_ret || !ep_len || !flags || J < 1 || ld_payload < Env::NPAY * (int64_t)J || ld_ep < J) return RESEL_EINVAL;
    if (B == 0) return RESEL_OK;
    hipLaunchKernelGGL(eval_step_kernel<Env>, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cfg, init, action, ld_action, payload,
                       ld_payload, n_episodes, J, state, ret_acc, ep_ret, ep_len, ld_ep, in_block, ld_in, flags, B);
    return launch_status();
}

template <class Env>
int collect_step(typename Env::Cfg cfg, resel_collect_layout_t lay, int init, const float* action, int64_t ld_action,
                 const typename Env::Payload* payload, typename Env::State state, double* ret_acc, float* traj, int T_cap, int64_t ld_row,
                 int max_episode_steps, float* in_block, int64_t ld_in, int A, int B, resel_stream_t stream) {
    if (rows_bad<Env>(cfg, action, payload, state, ret_acc, in_block, ld_action, ld_in, A, B)) return RESEL_EINVAL;
    if (!traj || T_cap < 1 || max_episode_steps < 1 || lay.logp >= 0 || ld_row < 1 || layout_need<Env>(lay) > ld_row) return RESEL_EINVAL;
    if (B == 0) return RESEL_OK;
    hipLaunchKernelGGL(collect_step_kernel<Env>, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, cfg, lay, init, action, ld_action,
                       payload, state, ret_acc, traj, T_cap, ld_row, max_episode_steps, in_block, ld_in, B);
    return launch_status();
}

}  // namespace

extern "C" {

int resel_tmaze_step(resel_tmaze_cfg_t cfg, int init, const float* action, int64_t ld_action, const int32_t* goals, int64_t ld_goals,
                     const int32_t* n_episodes, int J, int32_t* env_state, double* ret_acc, double* ep_ret, int32_t* ep_len, int64_t ld_ep,
                     float* in_block, int64_t ld_in, int A, int32_t* flags, int B, resel_stream_t stream) {
    return eval_step<TMazeEnv>(cfg, init, action, ld_action, goals, ld_goals, n_episodes, J, env_state, ret_acc, ep_ret, ep_len, ld_ep,
                               in_block, ld_in, A, flags, B, stream);
}

int resel_tmaze_collect_step(resel_tmaze_cfg_t cfg, resel_collect_layout_t lay, int init, const float* action, int64_t ld_action,
                             const int32_t* goal, int32_t* env_state, double* ret_acc, float* traj, int T_cap, int64_t ld_row,
                             int max_episode_steps, float* in_block, int64_t ld_in, int A, int B, resel_stream_t stream) {
    return collect_step<TMazeEnv>(cfg, lay, init, action, ld_action, goal, env_state, ret_acc, traj, T_cap, ld_row, max_episode_steps,
                                  in_block, ld_in, A, B, stream);
}

int resel_wind_step(resel_wind_cfg_t cfg, int init, const float* action, int64_t ld_action, const double* winds, int64_t ld_winds,
                    const int32_t* n_episodes, int J, double* env_pos, int32_t* env_words, double* ret_acc, double* ep_ret, int32_t* ep_len,
                    int64_t ld_ep, float* in_block, int64_t ld_in, int A, int32_t* flags, int B, resel_stream_t stream) {
    return eval_step<WindEnv>(cfg, init, action, ld_action, winds, ld_winds, n_episodes, J, {env_pos, env_words}, ret_acc, ep_ret, ep_len,
                              ld_ep, in_block, ld_in, A, flags, B, stream);
}

int resel_wind_collect_step(resel_wind_cfg_t cfg, resel_collect_layout_t lay, int init, const float* action, int64_t ld_action,
                            const double* wind, double* env_pos, int32_t* env_words, double* ret_acc, float* traj, int T_cap, int64_t ld_row,
                            int max_episode_steps, float* in_block, int64_t ld_in, int A, int B, resel_stream_t stream) {
    return collect_step<WindEnv>(cfg, lay, init, action, ld_action, wind, {env_pos, env_words}, ret_acc, traj, T_cap, ld_row,
                                 max_episode_steps, in_block, ld_in, A, B, stream);
}

int resel_catch_step(resel_catch_cfg_t cfg, int init, const float* action, int64_t ld_action, const int32_t* draws, int64_t ld_draws,
                     const int32_t* n_episodes, int J, int32_t* env_state, double* ret_acc, double* ep_ret, int32_t* ep_len, int64_t ld_ep,
                     float* in_block, int64_t ld_in, int A, int32_t* flags, int B, resel_stream_t stream) {
    return eval_step<CatchEnv>(cfg, init, action, ld_action, draws, ld_draws, n_episodes, J, env_state, ret_acc, ep_ret, ep_len, ld_ep,
                               in_block, ld_in, A, flags, B, stream);
}

int resel_catch_collect_step(resel_catch_cfg_t cfg, resel_collect_layout_t lay, int init, const float* action, int64_t ld_action,
                             const int32_t* draws, int32_t* env_state, double* ret_acc, float* traj, int T_cap, int64_t ld_row,
                             int max_episode_steps, float* in_block, int64_t ld_in, int A, int B, resel_stream_t stream) {
    return collect_step<CatchEnv>(cfg, lay, init, action, ld_action, draws, env_state, ret_acc, traj, T_cap, ld_row, max_episode_steps,
                                  in_block, ld_in, A, B, stream);
}

}  // extern "C"
