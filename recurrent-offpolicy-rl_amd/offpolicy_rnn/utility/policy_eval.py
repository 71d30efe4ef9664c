"""Policy evaluation during training: N deterministic episodes, `rows` of them at a time through ONE graphed policy step.

The reference snapshots the policy at the start of every iteration and runs `test_nprocess x test_nrollout` episodes in CPU worker
processes (utility/sample_utility.py:38-131, algorithm/sac.py:284-300,364-379).  This build has no CPU forward, so the same loop
runs on the device: `rows` environments share one `GraphedPolicyStep(..., row_reset=True)` - one H2D, one graph replay and one D2H
per environment step for all of them - and an episode that ends hands its row to the next one (the row's recurrent state and cgpt
position are reset inside the graph, hip/graph_step.py).

`run_episodes` is the scheduler (host only, numpy in / numpy out); `BatchedPolicyEval` owns the graph, the environments and a private
random stream, and leaves every global generator as it found it."""
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
        self.last_rows: List[int] = []                     # row that ran each episode of the last evaluation

    def invalidate(self):
        """After anything that re-allocates the policy's parameters (`load`, `.to`): capture again at the next evaluation."""
        if hasattr(self.step, 'invalidate'):
            self.step.invalidate()

    def _reset_env(self, env):
        if hasattr(env, 'meta_env_flag') and getattr(env, 'n_tasks', None) is not None:
            return env.reset(self.eval_tasks[self.rs.randint(0, len(self.eval_tasks))])
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
        if self.step is None:
            from ..hip.graph_step import GraphedPolicyStep
            self.step = GraphedPolicyStep(self.policy, self.device, batch_size=self.rows, row_reset=True)

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
