"""Discrete actions without a GPU: the argument checks of `resel_categorical_step` that return before the device is touched, and the
discrete form of the evaluation scheduler (`run_episodes(discrete=True)`) behind a stub step and scripted environments."""
import ctypes
import os

import numpy as np
import pytest

from offpolicy_rnn.env_utils.make_env import Box, Discrete
from offpolicy_rnn.utility.policy_eval import BatchedPolicyEval, run_episodes

RESEL_EINVAL = -1
HORIZONS = [3, 7, 5, 7, 2, 4]
OBS, NACT, ROWS = 3, 4, 4


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.fixture(scope='module')
def lib():
    from offpolicy_rnn.hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    h.resel_categorical_step.restype, h.resel_categorical_step.argtypes = _lib.SIGNATURES['resel_categorical_step']
    return h


def test_categorical_step_rejects_bad_arguments_before_touching_the_device(lib):
    """Nothing here is a device pointer: a call that got past the argument checks would fault, not return."""
    fake = 0x1000

    def call(M=3, A=5, logits=fake, u=fake, logp=fake, mode=fake, sample=fake, ld_x=None, ld_lp=None, ld_idx=1):
        return lib.resel_categorical_step(logits, A if ld_x is None else ld_x, u, 0.01, logp, A if ld_lp is None else ld_lp, mode, sample,
                                          ld_idx, M, A, None)

    assert call(A=0) == RESEL_EINVAL
    assert call(A=4097) == RESEL_EINVAL
    assert call(M=-1) == RESEL_EINVAL
    for name in ('logits', 'u', 'logp', 'mode', 'sample'):
        assert call(**{name: None}) == RESEL_EINVAL, name
    assert call(ld_x=4) == RESEL_EINVAL and call(ld_lp=4) == RESEL_EINVAL          # a row stride below A
    assert call(ld_idx=0) == RESEL_EINVAL
    assert call(M=0) == 0 and call(M=0, A=4096) == 0                               # nothing to do: nothing launched


def test_abi_version_is_11(lib):
    from offpolicy_rnn.hip import _lib
    lib.resel_abi_version.restype = ctypes.c_int
    assert lib.resel_abi_version() == _lib.ABI_VERSION == 11


# ------------------------------------------------------------------------------------------------ the scheduler, discrete form
class ScriptedDiscrete:
    """Episode k (the k-th reset over all environments of one `episodes` counter) lasts HORIZONS[k] steps; observation t of episode k
    is k + t / 10 everywhere, the reward is k + 1.  Records what `step` is handed; stepping after `done` without a reset fails."""

    def __init__(self, episodes):
        self.observation_space, self.action_space = Box(-np.inf, np.inf, (OBS,)), Discrete(NACT)
        self.episodes, self.k, self.t, self.live = episodes, None, 0, False
        self.actions = []

    def seed(self, s):
        pass

    def reset(self):
        self.k, self.t, self.live = self.episodes[0], 0, True
        self.episodes[0] += 1
        return np.full(OBS, float(self.k))

    def step(self, action):
        assert self.live, 'environment stepped between done and reset'
        self.t += 1
        self.actions.append((self.k, action))
        done = self.t >= HORIZONS[self.k]
        self.live = not done
        return np.full(OBS, self.k + self.t / 10), float(self.k + 1), done, {}


def _index(state_row):
    """The stub policy: the action index a row's observation k + t / 10 maps to - it changes along an episode and between episodes."""
    return int(round(state_row[0] * 10)) % NACT


class FakeDiscreteStep:
    """(mode, sample, logp) of a categorical step: mode [rows, 1] int64; records its inputs."""

    def __init__(self):
        self.calls = []

    def __call__(self, state, lst_state, lst_action, reward, reset=None):
        self.calls.append(tuple(np.array(a, copy=True) for a in (state, lst_state, lst_action, reward, reset)))
        mode = np.array([[_index(s)] for s in np.asarray(state)], dtype=np.int64)
        return mode, mode, np.zeros((len(mode), NACT), dtype=np.float32)


def _expected_schedule():
    free_at, out = [0] * ROWS, []
    for k, h in enumerate(HORIZONS):
        r = min(range(ROWS), key=lambda i: (free_at[i], i))
        out.append((r, free_at[r], free_at[r] + h - 1))
        free_at[r] += h
    return out


def test_run_episodes_discrete():
    episodes, step = [0], FakeDiscreteStep()
    ev = BatchedPolicyEval(None, lambda: ScriptedDiscrete(episodes), NACT, ROWS, 'cpu', seed=11, step=step, discrete=True)
    out = ev.evaluate(6)
    sched = _expected_schedule()
    # episode order and row hand-over: as in the continuous form (tests/test_policy_eval_host.py)
    assert out['EpLenTest'] == HORIZONS
    assert out['EpRetTest'] == [float(h * (k + 1)) for k, h in enumerate(HORIZONS)]
    assert ev.last_rows == [r for r, _, _ in sched] == [0, 1, 2, 3, 0, 0]
    assert len(step.calls) == max(last for _, _, last in sched) + 1 == 9
    # environments receive Python ints: the index of the step's mode
    for env in ev.envs:
        for k, act in env.actions:
            assert type(act) is int and 0 <= act < NACT
    for k, (r, first, last) in enumerate(sched):
        got = [a for kk, a in ev.envs[r].actions if kk == k]
        assert got == [_index(np.full(OBS, k + i / 10)) for i in range(last - first + 1)], k
    # lst_action: zeros on a row's first step, then the one-hot of the previous index
    seen = set()
    for k, (r, first, last) in enumerate(sched):
        for t in range(first, last + 1):
            state, lst_state, lst_action, reward, reset = step.calls[t]
            assert lst_action.shape == (ROWS, NACT)
            i = t - first
            if i == 0:
                assert reset[r] and not lst_action[r].any() and not lst_state[r].any() and not reward[r].any()
            else:
                want = np.zeros(NACT)
                want[_index(np.full(OBS, k + (i - 1) / 10))] = 1
                np.testing.assert_array_equal(lst_action[r], want, err_msg=f'episode {k} step {i}')
                np.testing.assert_allclose(lst_state[r], k + (i - 1) / 10)
                np.testing.assert_allclose(reward[r], k + 1)
                assert not reset[r]
                seen.add(int(want.argmax()))
    assert len(seen) == NACT                                         # every index was fed back at least once


def test_run_episodes_without_the_keyword_is_the_continuous_form():
    """tests/test_policy_eval_host.py `test_reset_flags_and_zero_inputs`, restated: the mean goes back as lst_action, the environment
    gets the un-normalised action."""
    ACT = 2

    class Cont(ScriptedDiscrete):
        def __init__(self, episodes):
            super().__init__(episodes)
            self.action_space = Box(-2.0, 4.0, (ACT,))

    calls = []

    def step(state, lst_state, lst_action, reward, reset):
        calls.append((np.array(lst_action, copy=True), np.array(reset, copy=True)))
        return np.repeat(0.05 * (np.asarray(state)[:, :1] + 1), ACT, axis=1).astype(np.float32)

    episodes = [0]
    envs = [Cont(episodes) for _ in range(ROWS)]
    out, rows = run_episodes(step, envs, 6, OBS, ACT, lambda e: e.reset())
    assert out['EpLenTest'] == HORIZONS and rows == [0, 1, 2, 3, 0, 0]
    for k, (r, first, last) in enumerate(_expected_schedule()):
        for t in range(first, last + 1):
            lst_action, reset = calls[t]
            i = t - first
            if i == 0:
                assert reset[r] and not lst_action[r].any()
            else:
                np.testing.assert_allclose(lst_action[r], 0.05 * (k + (i - 1) / 10 + 1), rtol=1e-6)      # the NORMALISED mean
    k, first_act = envs[1].actions[0]
    np.testing.assert_allclose(first_act, (0.05 * (k + 1) + 1) / 2 * 6.0 - 2.0, rtol=1e-6)
