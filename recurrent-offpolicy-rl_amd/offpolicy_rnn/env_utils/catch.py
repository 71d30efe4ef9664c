"""Catch-<runs>-v0, the delayed-reward credit-assignment task (reference envs/credit_assign/catch.py `DelayedCatch`, registered in
envs/credit_assign/__init__.py for runs in {1, 2, 5, 10, 20, 40}) without gym.

A fruit falls down a 7 x 7 grid, one row per step; a basket in the last row moves left / stays / moves right.  Seven steps make a
run: six falling steps, then (except behind the last run) one soft-reset step that ignores the action and puts the next fruit and
basket in place.  An episode is `runs` runs, 7 * runs - 1 steps; every reward is withheld until the last step, which pays the
number of fruits caught.  Everything random - the fruit columns `ns` and the basket start columns `ms` - is drawn at `reset()`.

The same step runs as a kernel at the end of a graphed policy step (`ops.catch_step`, csrc/env_step.hip); `device_config()` is
what that kernel takes, and `Catch.step` is what it is tested against bit for bit."""
import re

import numpy as np

GRID = 7
MAX_DEVICE_RUNS = 40                                   # RESEL_CATCH_MAX_RUNS of include/resel_hip.h: the kernel's payload row holds 40 draws
_NAME = re.compile(r'^Catch-(\d+)-v0$')


class Catch:
    def __init__(self, runs: int, seed: int = 0):
        from .make_env import Box, Discrete
        assert runs >= 1
        self.runs = int(runs)
        self.episode_length = GRID * self.runs - 1
        self.observation_space = Box(-1.0, 1.0, (GRID * GRID,))
        self.action_space = Discrete(3)
        self._rs = np.random.RandomState(seed)
        self.ns, self.ms = np.zeros(self.runs, dtype=np.int64), np.ones(self.runs, dtype=np.int64)
        self.fruit_row, self.fruit_col, self.basket = 0, 0, 1
        self.catch_count, self.accumulated, self.time_step = 1, 0, 0

    def seed(self, s):
        self._rs = np.random.RandomState(s)

    def device_config(self) -> dict:
        """What `ops.catch_step` needs to run this environment on the device."""
        return dict(num_catches=self.runs, episode_length=self.episode_length)

    def draw_fruits(self):
        """(ns, ms) of the next episode - fruit columns in [0, 6), basket start columns in [1, 5) - from the private stream: the two
        draws `reset()` makes, in its order."""
        ns = self._rs.randint(0, GRID - 1, size=self.runs)
        ms = self._rs.randint(1, GRID - 2, size=self.runs)
        return ns, ms

    def _obs(self):
        canvas = np.zeros(GRID * GRID, dtype=np.float32)
        canvas[GRID * self.fruit_row + self.fruit_col] = -1          # the fruit,
        canvas[GRID * (GRID - 1) + self.basket] = 1                  # then the basket: it covers a fruit in its cell
        return canvas

    def reset(self, fruits=None):
        ns, ms = self.draw_fruits() if fruits is None else fruits
        self.ns, self.ms = np.array(ns, dtype=np.int64).reshape(-1), np.array(ms, dtype=np.int64).reshape(-1)
        assert self.ns.shape == self.ms.shape == (self.runs,)
        self.fruit_row, self.fruit_col, self.basket = 0, int(self.ns[0]), int(self.ms[0])
        self.catch_count, self.accumulated, self.time_step = 1, 0, 0
        return self._obs()

    def step(self, action):
        action = int(action)
        assert 0 <= action < 3, action
        self.time_step += 1
        if self.fruit_row == GRID - 1:                   # soft reset: the action is ignored, the next fruit and basket appear
            self.fruit_row, self.fruit_col, self.basket = 0, int(self.ns[self.catch_count]), int(self.ms[self.catch_count])
            self.catch_count += 1
            return self._obs(), 0.0, False, {}
        self.basket = min(max(0, self.basket + action - 1), GRID - 1)
        self.fruit_row += 1
        if self.fruit_row == GRID - 1 and self.fruit_col == self.basket:
            self.accumulated += 1
        return self._obs(), self.last_reward(), self.time_step >= self.episode_length, {}

    def last_reward(self) -> float:
        """The reward of the step that led to the current state - a function of (time_step, accumulated) alone."""
        return float(self.accumulated) if self.time_step >= self.episode_length else 0.0


def parse_name(env_name: str):
    """'Catch-<runs>-v0' with runs >= 1 -> Catch keyword arguments, or None."""
    m = _NAME.match(env_name)
    if not m or int(m.group(1)) < 1:
        return None
    return dict(runs=int(m.group(1)))


def device_steppable(env) -> bool:
    """True for the environments `ops.catch_step` implements: a Catch whose draws fit the kernel's payload row."""
    return isinstance(env, Catch) and env.runs <= MAX_DEVICE_RUNS
