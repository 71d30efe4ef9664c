"""Wind-v0 meta-RL task (reference envs/meta/toy_navigation/wind.py `WindEnv` behind envs/meta/wrappers.py `VariBadWrapper` with
`episodes_per_task = 1`, no oracle and no done flag in the observation; configured in envs/pomdp_config.py) without gym.

A point on the plane starts at (0, 0) and moves by `action + wind` per step; the wind is fixed per task and hidden, the reward is 1.0
inside a ball of radius 0.03 around (0, 1) and 0.0 elsewhere, an episode lasts `_max_episode_steps` = 75 steps.  The `n_tasks` winds come
from `RandomState(1337)`, two uniform draws in [-0.08, 0.08] per task, x first.

`step` takes the normalised action: clip to [-1, 1], rescale to the inner bounds - float32 +-0.1, promoted to double where they meet a
double, as in the reference -, clip again, then `state = state + action + wind` in float64.  The outward action space is Box(-1, 1) with
float64 bounds, as the reference's `regularize_space` sets it.

The same step runs as a kernel at the end of a graphed policy step (`ops.wind_step` / `ops.wind_collect_step`, csrc/env_step.hip);
`device_config()` is what those kernels take and `Wind.step` is what they are tested against bit for bit, so every expression here is
spelled as one rounding per operation: the distance test is sqrt(dx * dx + dy * dy) <= r, not a library norm."""
import math

import numpy as np

GOAL = (0.0, 1.0)


class Wind:
    meta_env_flag = True

    def __init__(self, n_tasks: int = 60, max_episode_steps: int = 75, goal_radius: float = 0.03, seed: int = 0):
        from .make_env import Box
        assert n_tasks >= 1 and max_episode_steps >= 1
        self.n_tasks, self._max_episode_steps, self.goal_radius = int(n_tasks), int(max_episode_steps), float(goal_radius)
        self.horizon_bamdp = self._max_episode_steps             # episodes_per_task = 1
        self.np_random = np.random.RandomState(seed=1337)
        self.winds = [[self.np_random.uniform(-0.08, 0.08), self.np_random.uniform(-0.08, 0.08)] for _ in range(self.n_tasks)]
        self._goal = np.array(GOAL)
        self._lb, self._ub = np.full((2,), -0.1, dtype=np.float32), np.full((2,), 0.1, dtype=np.float32)     # the inner action bounds
        self.observation_space = Box(-np.inf, np.inf, (2,), dtype=np.float64)
        self.action_space = Box(-1.0, 1.0, (2,), dtype=np.float64)
        self._wind = np.array(self.winds[0])
        self._state, self.step_count, self.done_mdp = np.array([0.0, 0.0]), 0, True
        self.seed(seed)

    def seed(self, s):
        self.np_random.seed(s)

    def get_all_task_idx(self):
        return range(len(self.winds))

    def get_current_task(self):
        return self._wind.copy()

    def device_config(self) -> dict:
        """What `ops.wind_step` needs to run this environment on the device: every bound as the double the host arithmetic meets."""
        space = self.action_space
        return dict(episode_length=self._max_episode_steps, goal_x=float(self._goal[0]), goal_y=float(self._goal[1]),
                    goal_radius=self.goal_radius, act_low=float(self._lb[0]), act_high=float(self._ub[0]),
                    act_span=float((self._ub - self._lb)[0]), out_low=float(space.low[0]), out_span=float((space.high - space.low)[0]))

    def set_wind(self, wind):
        """A wind that is not one of the tasks' (the reference's `set_goal`)."""
        self._wind = np.array(wind, dtype=np.float64)

    def reset(self, task=None):
        if task is not None:                                     # None keeps the current wind, as the reference's reset_task(None)
            self._wind = np.array(self.winds[task])
        self._state, self.step_count, self.done_mdp = np.array([0.0, 0.0]), 0, False
        return np.copy(self._state)

    def step(self, action):
        action = np.clip(action, -1, 1)
        lb, ub = self._lb, self._ub
        action = lb + (action + 1.0) * 0.5 * (ub - lb)
        action = np.clip(action, lb, ub)
        self._state = self._state + action + self._wind
        self.step_count += 1
        self.done_mdp = self.step_count >= self._max_episode_steps
        return np.copy(self._state), self.last_reward(), self.done_mdp, {'done_mdp': self.done_mdp}

    def last_reward(self) -> float:
        """The reward of the step that led to the current state - a function of the state alone."""
        dx, dy = float(self._state[0]) - float(self._goal[0]), float(self._state[1]) - float(self._goal[1])
        return 1.0 if math.sqrt(dx * dx + dy * dy) <= self.goal_radius else 0.0


def device_steppable(env) -> bool:
    """True for the environments `ops.wind_step` implements."""
    return isinstance(env, Wind)
