"""The episode scheduler of the batched policy evaluation (offpolicy_rnn/utility/policy_eval.py) on the host: a fake numpy step
function stands in for the graphed policy step and records what it is fed."""
import random

import numpy as np
import torch

from offpolicy_rnn.env_utils.make_env import Box
from offpolicy_rnn.utility.policy_eval import BatchedPolicyEval

HORIZONS = [3, 7, 5, 7, 2, 4]
OBS, ACT, ROWS = 3, 2, 4


class Scripted:
    """Episode k (the k-th reset over all environments of one `episodes` counter) lasts HORIZONS[k] steps; observation t of episode k
    is k + t / 10 everywhere, the reward is k + 1.  Stepping after `done` without a reset fails."""

    def __init__(self, episodes):
        self.observation_space = Box(-np.inf, np.inf, (OBS,))
        self.action_space = Box(-2.0, 4.0, (ACT,))               # not the unit box: unorm_act must be applied
        self.episodes, self.k, self.t, self.live = episodes, None, 0, False
        self.seeds, self.actions = [], []

    def seed(self, s):
        self.seeds.append(s)

    def reset(self):
        self.k, self.t, self.live = self.episodes[0], 0, True
        self.episodes[0] += 1
        return np.full(OBS, float(self.k))

    def step(self, action):
        assert self.live, 'environment stepped between done and reset'
        self.t += 1
        self.actions.append((self.k, np.asarray(action).copy()))
        done = self.t >= HORIZONS[self.k]
        self.live = not done
        return np.full(OBS, self.k + self.t / 10), float(self.k + 1), done, {'progress': self.t, 'name': 'not a number'}


class FakeStep:
    """mean[r] = 0.05 * (state[r, 0] + 1) in both action columns (inside the unit box for the episodes above); records its inputs."""

    def __init__(self):
        self.calls = []

    def __call__(self, state, lst_state, lst_action, reward, reset=None):
        self.calls.append(tuple(np.array(a, copy=True) for a in (state, lst_state, lst_action, reward, reset)))
        mean = np.repeat(0.05 * (np.asarray(state)[:, :1] + 1), ACT, axis=1).astype(np.float32)
        return mean, mean, np.zeros((len(mean), 1), dtype=np.float32)


def _run(n_episodes=6, rows=ROWS):
    episodes, step = [0], FakeStep()
    ev = BatchedPolicyEval(None, lambda: Scripted(episodes), ACT, rows, 'cpu', seed=11, step=step)
    return ev, step, ev.evaluate(n_episodes)


def _expected_schedule():
    """(row, first step, last step) of each episode: free rows take the next episodes, lowest row first."""
    free_at, out = [0] * ROWS, []
    for k, h in enumerate(HORIZONS):
        r = min(range(ROWS), key=lambda i: (free_at[i], i))
        out.append((r, free_at[r], free_at[r] + h - 1))
        free_at[r] += h
    return out


def test_results_come_in_episode_order():
    ev, step, out = _run()
    assert out['EpLenTest'] == HORIZONS
    assert out['EpRetTest'] == [float(h * (k + 1)) for k, h in enumerate(HORIZONS)]
    assert out['progressTest'] == [float(h) for h in HORIZONS] and 'nameTest' not in out     # last report of each episode; floats only
    sched = _expected_schedule()
    assert ev.last_rows == [r for r, _, _ in sched] == [0, 1, 2, 3, 0, 0]
    assert len(step.calls) == max(last for _, _, last in sched) + 1 == 9


def test_reset_flags_and_zero_inputs():
    ev, step, _ = _run()
    sched = _expected_schedule()
    n = len(step.calls)
    busy = np.zeros((n, ROWS), dtype=bool)
    starts = np.zeros((n, ROWS), dtype=bool)
    for k, (r, first, last) in enumerate(sched):
        busy[first:last + 1, r] = True
        starts[first, r] = True
    for t, (state, lst_state, lst_action, reward, reset) in enumerate(step.calls):
        np.testing.assert_array_equal(np.asarray(reset).astype(bool), starts[t] | ~busy[t], err_msg=f'step {t}')
        for r in range(ROWS):
            if starts[t, r] or not busy[t, r]:                   # an episode's first step and idle rows: zero recurrent inputs
                assert not lst_state[r].any() and not lst_action[r].any() and not reward[r].any(), (t, r)
            if not busy[t, r]:
                assert not state[r].any(), (t, r)
    for k, (r, first, last) in enumerate(sched):
        for t in range(first, last + 1):
            state, lst_state, lst_action, reward, _ = step.calls[t]
            i = t - first
            np.testing.assert_allclose(state[r], k + i / 10)
            if i > 0:
                np.testing.assert_allclose(lst_state[r], k + (i - 1) / 10)
                np.testing.assert_allclose(lst_action[r], 0.05 * (k + (i - 1) / 10 + 1), rtol=1e-6)      # the NORMALISED mean
                np.testing.assert_allclose(reward[r], k + 1)
    # the environment received the un-normalised action: (a + 1) / 2 * (high - low) + low
    for env in ev.envs:
        for k, act in env.actions:
            assert -2.0 <= act.min() and act.max() <= 4.0
    k, first_act = ev.envs[1].actions[0]
    np.testing.assert_allclose(first_act, (0.05 * (k + 1) + 1) / 2 * 6.0 - 2.0, rtol=1e-6)


def test_more_rows_than_episodes_and_a_single_row():
    ev, step, out = _run(n_episodes=2)
    assert out['EpLenTest'] == HORIZONS[:2] and ev.last_rows == [0, 1]
    for state, _, _, _, reset in step.calls:                       # rows 2 and 3 never get an episode
        assert reset[2] and reset[3] and not state[2:].any()
    assert [e.k for e in ev.envs] == [0, 1, None, None]
    ev, step, out = _run(n_episodes=6, rows=1)
    assert out['EpLenTest'] == HORIZONS and len(step.calls) == sum(HORIZONS)


def test_environments_are_seeded_from_the_private_stream_only():
    ev, _, _ = _run()
    rs = np.random.RandomState(11)
    want = [int(rs.randint(0, 10000000)) for _ in range(ROWS)]
    assert ev.env_seeds == want
    assert [e.seeds for e in ev.envs] == [[s + 5] for s in want]           # reference eval_inprocess: env.seed(seed + 5)
    envs = ev.envs
    envs[0].episodes[0] = 0                                          # the scripted episodes start over
    ev.evaluate(3)                                                   # created once: the same environments, not seeded again
    assert ev.envs is envs and [e.seeds for e in ev.envs] == [[s + 5] for s in want]


def test_global_generators_are_left_as_found():
    class Noisy(Scripted):                                          # an environment that draws from every global stream
        def step(self, action):
            random.random(), np.random.rand(), torch.rand(1)
            return super().step(action)

    random.seed(5), np.random.seed(6), torch.manual_seed(7)
    before = (random.getstate(), np.random.get_state(), torch.get_rng_state().clone())
    episodes = [0]
    ev = BatchedPolicyEval(None, lambda: Noisy(episodes), ACT, ROWS, 'cpu', step=FakeStep())
    ev.evaluate(6)
    assert random.getstate() == before[0]
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), before[1]))
    assert torch.equal(torch.get_rng_state(), before[2])

