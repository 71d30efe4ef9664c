"""Policy evaluation during training: N deterministic episodes, `rows` of them at a time through ONE graphed policy step.

The reference snapshots the policy at the start of every iteration and runs `test_nprocess x test_nrollout` episodes in CPU worker
processes (utility/sample_utility.py:38-131, algorithm/sac.py:284-300,364-379).  This build has no CPU forward, so the same loop
runs on the device: `rows` environments share one `GraphedPolicyStep(..., row_reset=True)` - one H2D, one graph replay and one D2H
per environment step for all of them - and an episode that ends hands its row to the next one (the row's recurrent state and cgpt
position are reset inside the graph, hip/graph_step.py).

`run_episodes` is the scheduler (host only, numpy in / numpy out); `BatchedPolicyEval` owns the graph, the environments and a private
random stream, and leaves every global generator as it found it.

An environment that exists as a kernel (env_utils/device_env.py: the discrete T-Maze, `ops.tmaze_step`; Wind-v0, `ops.wind_step`; Catch up to 40
runs, `ops.catch_step`) is stepped INSIDE the graph:
`DeviceEnvEval` appends the environment step to the policy step as its last node, so an evaluation is `waves x episode_length`
back-to-back replays behind one init call, with one D2H at the end and no host round trip per step.  `RESEL_DEVICE_ENV=0` keeps
such an environment on the host loop."""
import os
import random
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from .sample_utility import unorm_act


def run_episodes(step: Callable, envs: List, n_episodes: int, obs_dim: int, act_dim: int, reset_env: Callable, discrete: bool = False):
    """The reference's `policy_eval` loop (sample_utility.py:50-100) over len(envs) rows at once.

    step(state, lst_state, lst_action, reward, reset) -> action means [rows, act_dim]; `reset` [rows] bool marks the rows that start
    an episode on this step.  Episodes 0 .. n_episodes - 1 are handed to rows in index order as rows become free (lowest free row
    first), environments are reset in that order too, and no environment is stepped between its `done` and its next reset.  A row's
    first step sees zero last state / last action / reward (:59-61).  A row without an episode is fed zeros with its flag set on every
    step (a cgpt position never runs away); what the step returns for it is ignored.
    discrete (reference :75-76,82-84): step returns the action indices [rows, 1] instead, the environment gets `int(index)` and the
    next step's lst_action is the one-hot of it over act_dim actions.
    -> ({'EpRetTest': [...], 'EpLenTest': [...], '<key>Test': [...]} in episode order, [row that ran each episode]); an info entry
    holds, per episode that reported the key, the value of its last report (the reference keeps the last report only, :93-96)."""
    rows = len(envs)
    state, lst_state = np.zeros((rows, obs_dim)), np.zeros((rows, obs_dim))
    lst_action, reward = np.zeros((rows, act_dim)), np.zeros((rows, 1))
    reset = np.ones(rows, dtype=bool)
    episode = [-1] * rows                                  # episode index a row is running; -1: idle
    ep_ret, ep_len, ep_row = [0.0] * n_episodes, [0] * n_episodes, [-1] * n_episodes
    ep_info = [dict() for _ in range(n_episodes)]
    handed = 0

    def begin(r):
        nonlocal handed
        lst_state[r], lst_action[r], reward[r], reset[r] = 0.0, 0.0, 0.0, True
        if handed < n_episodes:
            episode[r], ep_row[handed] = handed, r
            handed += 1
            state[r] = np.asarray(reset_env(envs[r])).reshape(-1)
        else:
            episode[r] = -1
            state[r] = 0.0

    for r in range(rows):
        begin(r)
    while any(k >= 0 for k in episode):
        mean = np.asarray(step(state, lst_state, lst_action, reward, reset)).reshape(rows, 1 if discrete else act_dim)
        reset[:] = False
        for r in range(rows):
            k = episode[r]
            if k < 0:
                reset[r] = True
                continue
            if discrete:
                index = int(unorm_act(mean[r, 0], envs[r].action_space))
                act = np.zeros(act_dim)
                act[index] = 1
                next_state, rew, done, info = envs[r].step(index)
            else:
                act = mean[r].copy()
                next_state, rew, done, info = envs[r].step(unorm_act(act, envs[r].action_space))
            lst_state[r] = state[r]
            state[r] = np.asarray(next_state).reshape(-1)
            reward[r], lst_action[r] = rew, act
            for key, v in (info or {}).items():
                try:
                    ep_info[k][key + 'Test'] = float(v)
                except Exception:
                    continue
            ep_ret[k] += rew
            ep_len[k] += 1
            if done:
                begin(r)
    out = {'EpRetTest': ep_ret, 'EpLenTest': ep_len}
    for key in sorted({key for d in ep_info for key in d}):
        out[key] = [d[key] for d in ep_info if key in d]
    return out, ep_row


DEVICE_ENV_DEFAULT = '1'                                   # RESEL_DEVICE_ENV when the variable is not set


def device_env_enabled() -> bool:
    return os.environ.get('RESEL_DEVICE_ENV', DEVICE_ENV_DEFAULT) != '0'


class DeviceEnvEval:
    """`run_episodes` for `rows` environments of one kind that exists as a kernel (env_utils/device_env.py: the discrete T-Maze, Wind-v0, Catch),
    with the environment step inside the graphed policy step.

    All episodes have the same length T, so the host scheduler runs episode k on row k % rows as that row's (k // rows)-th episode and
    takes ceil(n / rows) * T steps; this object does the same with one init call of the kind's evaluation entry, that many
    `replay_device()` calls, one D2H of the per-episode results and one synchronise.  What an episode starts from - the T-Maze's goal side,
    Wind's wind vector, Catch's fruit and basket columns - comes from the kind's `eval_payloads`, which draws as the host loop would: the
    T-Maze and Catch from the per-row host environments (`TMaze.draw_goal`, `Catch.draw_fruits`: the draws their `reset()` makes), a meta
    environment one task per episode through `draw_task`.
    The hook runs in the warm-up and in the capture too, on whatever the buffers hold: every buffer is (re)initialised by the init
    call of each evaluation, never at capture."""

    def __init__(self, policy, envs: List, device, draw_task: Optional[Callable] = None):
        from ..env_utils.device_env import device_env_kind
        from ..hip.graph_step import GraphedPolicyStep
        self.envs, self.rows, self.device, self.draw_task = envs, len(envs), torch.device(device), draw_task
        self.kind = kind = device_env_kind(envs[0])
        self.cfg = envs[0].device_config()
        assert all(device_env_kind(e) is kind and e.device_config() == self.cfg for e in envs), 'one graph steps one kind of environment'
        self.T, self.obs_dim, self.act_dim = kind.episode_length(self.cfg), kind.obs_dim, kind.act_dim
        self.step = GraphedPolicyStep(policy, self.device, batch_size=self.rows, row_reset=True, after_step=self._env_step)
        self.J = 0
        dev = self.device
        self._env_state = kind.state_views(torch.zeros(self.rows * kind.state_bytes, dtype=torch.uint8, device=dev), self.rows)
        self._ret_acc = torch.zeros(self.rows, dtype=torch.float64, device=dev)

    def _ensure(self, J: int):
        """Tables for J episodes per row.  Their addresses are part of the captured graph: growing them captures again."""
        if J <= self.J:
            return
        B, dev, kind = self.rows, self.device, self.kind
        w = kind.payload_width
        pay = B * J * w * torch.empty((), dtype=kind.payload_dtype).element_size()
        self._tab_host = torch.zeros(pay + 4 * B, dtype=torch.uint8).pin_memory()         # payloads [B, J, w] | n_episodes int32 [B]: one H2D
        self._tab_dev = torch.zeros(pay + 4 * B, dtype=torch.uint8, device=dev)
        self._payload, self._n_ep = self._tab_dev[:pay].view(kind.payload_dtype).view(B, J, w), self._tab_dev[pay:].view(torch.int32)
        self._payload_np, self._n_ep_np = self._tab_host.numpy()[:pay].view(kind.payload_np).reshape(B, J, w), self._tab_host.numpy()[pay:].view(np.int32)
        self._res_dev = torch.zeros(B * J * 12, dtype=torch.uint8, device=dev)            # ep_ret fp64 [B, J] | ep_len int32 [B, J]: one D2H
        self._res_host = torch.zeros(B * J * 12, dtype=torch.uint8).pin_memory()
        self._ep_ret, self._ep_len = self._res_dev[:B * J * 8].view(torch.float64).view(B, J), self._res_dev[B * J * 8:].view(torch.int32).view(B, J)
        self.J = J
        self.step.invalidate()

    def _launch(self, init: bool):
        from ..hip import ops
        step = self.step
        self.kind.eval_step(ops, self.cfg, init, self.kind.action(step._out_dev, False), self._payload, self._n_ep, self._env_state,
                            self._ret_acc, self._ep_ret, self._ep_len, step._in_dev, step._flags_dev)

    def _env_step(self, step):
        self._launch(False)

    def invalidate(self):
        self.step.invalidate()

    @torch.no_grad()
    def run(self, n_episodes: int):
        """-> what `run_episodes` returns for these environments: ({'EpRetTest': [...], 'EpLenTest': [...], ...}, [row of each episode])."""
        n, B, T, step = int(n_episodes), self.rows, self.T, self.step
        if n <= 0:
            return {'EpRetTest': [], 'EpLenTest': []}, []
        waves = -(-n // B)
        self._ensure(waves)
        J = self.J
        step.capture(self.obs_dim, self.act_dim)
        for ip in step._counters():                                          # what `__call__` raises at the step that would overrun
            if T > ip.max_seqlen:
                raise RuntimeError(f'cgpt rollout: KV cache is full (row 0: {ip.max_seqlen} tokens, max_seqlen {ip.max_seqlen})')
        per_row = [len(range(r, n, B)) for r in range(B)]                    # ceil((n - r) / rows)
        self._tab_host.zero_()
        for k, payload in enumerate(self.kind.eval_payloads(self.envs, n, self.draw_task)):      # drawn in the host loop's order
            self._payload_np[k % B, k // B] = payload
        self._n_ep_np[:] = per_row
        self._tab_dev.copy_(self._tab_host, non_blocking=True)
        self._launch(True)
        for _ in range(waves * T):
            step.replay_device()
        self._res_host.copy_(self._res_dev, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        # the host mirrors of the cgpt positions, as the same schedule through `__call__` leaves them: a row of the last wave is
        # T tokens into its episode, a row that went idle earlier was fed one flagged step after another (position 0, then 1)
        step._row_pos = np.array([T if per_row[r] == waves else 1 for r in range(B)], dtype=np.int64)
        for ip in step._counters():
            ip.seqlen_offset = int(step._row_pos.max())
        res = self._res_host.numpy()
        ep_ret, ep_len = res[:B * J * 8].view(np.float64).reshape(B, J), res[B * J * 8:].view(np.int32).reshape(B, J)
        out = {'EpRetTest': [float(ep_ret[k % B, k // B]) for k in range(n)], 'EpLenTest': [int(ep_len[k % B, k // B]) for k in range(n)]}
        out.update(self.kind.eval_extras(n))
        return out, [k % B for k in range(n)]


def _is_training(policy) -> bool:
    mods = getattr(policy, 'contextual_modules', None)
    if mods:
        return bool(next(iter(mods.values())).training)
    return bool(getattr(policy, 'training', False))


class BatchedPolicyEval:
    """`rows` evaluation environments behind one graphed policy step.  Everything is created at the first `evaluate`:
    the `GraphedPolicyStep(policy, device, batch_size=rows, row_reset=True)`, the environments (`env_factory()` each, seeded from the
    private stream the way the reference's `eval_inprocess` seeds its own, sample_utility.py:127-129) and nothing else.

    eval_tasks: task list of a meta environment (reference :53-56) - a reset draws one from the private stream.
    discrete: a categorical policy - act_dim actions, the step's first output is the mode index (`run_episodes(discrete=True)`).
    step: a replacement for the graphed step with the same call signature (host tests)."""

    def __init__(self, policy, env_factory: Callable, act_dim: int, rows: int, device, seed: int = 0, eval_tasks=None,
                 step: Optional[Callable] = None, discrete: bool = False):
        assert rows > 0
        self.policy, self.env_factory, self.act_dim, self.rows = policy, env_factory, act_dim, int(rows)
        self.device = torch.device(device)
        self.eval_tasks, self.discrete = eval_tasks, bool(discrete)
        self.rs = np.random.RandomState(seed)
        self.step, self.envs, self.env_seeds = step, None, []
        self._host_only = step is not None                 # a replacement step is a host callable: never the in-graph environment
        self.device_env: Optional[DeviceEnvEval] = None
        self.last_rows: List[int] = []                     # row that ran each episode of the last evaluation

    def invalidate(self):
        """After anything that re-allocates the policy's parameters (`load`, `.to`): capture again at the next evaluation."""
        if hasattr(self.step, 'invalidate'):
            self.step.invalidate()
        if self.device_env is not None:
            self.device_env.invalidate()

    def _draw_task(self):
        """The task of a meta environment's next evaluation episode: one draw from the private stream (reference :53-56)."""
        return self.eval_tasks[self.rs.randint(0, len(self.eval_tasks))]

    def _reset_env(self, env):
        if hasattr(env, 'meta_env_flag') and getattr(env, 'n_tasks', None) is not None:
            return env.reset(self._draw_task())
        return env.reset()

    def _make(self):
        if self.envs is None:
            self.envs = []
            for _ in range(self.rows):
                env, seed = self.env_factory(), int(self.rs.randint(0, 10000000))
                env.seed(seed + 5)
                env.action_space.seed(seed + 6)
                env.observation_space.seed(seed + 7)
                self.envs.append(env)
                self.env_seeds.append(seed)
        if self._on_device():
            if self.device_env is None:
                self.device_env = DeviceEnvEval(self.policy, self.envs, self.device, draw_task=self._draw_task)
            return
        if self.step is None:
            from ..hip.graph_step import GraphedPolicyStep
            self.step = GraphedPolicyStep(self.policy, self.device, batch_size=self.rows, row_reset=True)

    def _on_device(self) -> bool:
        """The in-graph environment step: environments of one kind that has a kernel (env_utils/device_env.py) behind the policy head that
        kernel reads, on a CUDA device, unless RESEL_DEVICE_ENV=0."""
        from ..env_utils.device_env import device_env_kind
        kind = device_env_kind(self.envs[0])
        return (not self._host_only and kind is not None and self.discrete == kind.categorical and self.device.type == 'cuda'
                and device_env_enabled() and kind.policy_ok(self.policy) and all(device_env_kind(e) is kind for e in self.envs))

    def evaluate(self, n_episodes: int) -> Dict[str, list]:
        """n_episodes deterministic episodes (action = the policy's mean) of the current parameters, which the graph reads through
        their storage.  The step is captured and replayed with the policy in eval mode; its previous mode comes back afterwards, and
        so does the state of Python's, numpy's and torch's CPU and device generators (the graph's unused action-noise draws - or a categorical
        head's uniform draws - advance the device generator; reading its state is one device sync)."""
        cuda = self.device.type == 'cuda'
        saved = (random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state(self.device) if cuda else None)
        was_training = _is_training(self.policy) if self.policy is not None else False
        try:
            if self.policy is not None:
                self.policy.eval()
            self._make()
            if self._on_device():
                out, self.last_rows = self.device_env.run(int(n_episodes))
                return out
            obs_dim = self.envs[0].observation_space.shape[0]

            def step(state, lst_state, lst_action, reward, reset):
                return self.step(state, lst_state, lst_action, reward, reset=reset)[0]

            out, self.last_rows = run_episodes(step, self.envs, int(n_episodes), obs_dim, self.act_dim, self._reset_env,
                                               discrete=self.discrete)
            return out
        finally:
            if self.policy is not None:
                self.policy.train(was_training)
            random.setstate(saved[0])
            np.random.set_state(saved[1])
            torch.set_rng_state(saved[2])
            if cuda:
                torch.cuda.set_rng_state(saved[3], self.device)
