"""T-Maze memory task (reference envs/memory_envs/tmaze.py: `TMazeBase` with ambiguous positions, as `TMazeClassicPassive` /
`TMazeClassicActive` configure it; ids and constants of envs/memory_envs/configs/tmaze_{passive,active}.py) without gym.

    o--s------------j      cells (x, 0) for 0 <= x <= o + L, and the two goal candidates (o + L, +1), (o + L, -1)
                           o: oracle at x = 0, s: start at x = o, j: junction at x = o + L

An episode lasts `episode_length` steps (passive: o = 0, L + 1 steps; active: o = 1, L + 3).  The goal side is shown once, the
first time the agent is observed at x = 0, so the last step's turn has to be remembered.  Walking right on every step and turning
to the goal side on the last one returns exactly 1.0; every step behind that schedule costs `penalty` = -1 / L.

The same step runs as a kernel at the end of a graphed policy step (`ops.tmaze_step`, csrc/env_step.hip); `device_config()` is
what that kernel takes, and `TMaze.step` is what it is tested against bit for bit - the reward arithmetic is kept literally,
signed zeros included."""
import re

import numpy as np

MOVES = ((1, 0), (0, 1), (-1, 0), (0, -1))
_NAME = re.compile(r'^Mem-T-(passive|active)-(\d+)(-cont-act)?-v0$')


class TMaze:
    def __init__(self, corridor_length: int, oracle_length: int = 0, goal_reward: float = 1.0, penalty: float = 0.0,
                 distract_reward: float = 0.0, continuous_act_space: bool = False, seed: int = 0):
        from .make_env import Box, Discrete
        assert corridor_length >= 1 and oracle_length >= 0 and penalty <= 0.0
        self.corridor_length, self.oracle_length = int(corridor_length), int(oracle_length)
        self.episode_length = self.corridor_length + 2 * self.oracle_length + 1
        self.goal_reward, self.penalty, self.distract_reward = float(goal_reward), float(penalty), float(distract_reward)
        self.continuous_act_space = bool(continuous_act_space)
        self.observation_space = Box(-1.0, 1.0, (2,))
        self.action_space = Box(-1.0, 1.0, (4,)) if self.continuous_act_space else Discrete(4)
        self._rs = np.random.RandomState(seed)
        self.x, self.y, self.goal_y, self.time_step, self.oracle_visited = self.oracle_length, 0, 1, 0, False

    def seed(self, s):
        self._rs = np.random.RandomState(s)

    def device_config(self) -> dict:
        """What `ops.tmaze_step` needs to run this environment on the device."""
        return dict(corridor_length=self.corridor_length, oracle_length=self.oracle_length, episode_length=self.episode_length,
                    goal_reward=self.goal_reward, penalty=self.penalty, distract_reward=self.distract_reward)

    def draw_goal(self) -> int:
        """The goal side of the next episode, -1 / +1, from the private stream: one draw, the one `reset()` makes."""
        return int(self._rs.choice([-1, 1]))

    def _on_map(self, x, y):
        end = self.oracle_length + self.corridor_length
        return (y == 0 and 0 <= x <= end) or (x == end and y in (-1, 1))

    def _obs(self):
        if self.x == 0:                                  # the oracle shows the goal side once per episode
            e = 0 if self.oracle_visited else self.goal_y
            self.oracle_visited = True
            return np.array([0, e], dtype=np.float32)
        if self.x < self.oracle_length + self.corridor_length:
            return np.array([0, 0], dtype=np.float32)
        return np.array([1, self.y], dtype=np.float32)

    def reset(self, goal=None):
        self.x, self.y = self.oracle_length, 0
        self.goal_y = self.draw_goal() if goal is None else int(goal)
        self.oracle_visited, self.time_step = False, 0
        return self._obs()

    def step(self, action):
        self.time_step += 1
        if self.continuous_act_space:
            action = int(np.argmax(np.reshape(action, (-1,))))        # first maximum on ties
        else:
            action = int(action)
            assert 0 <= action < 4, action
        mx, my = MOVES[action]
        if self._on_map(self.x + mx, self.y + my):
            self.x, self.y = self.x + mx, self.y + my
        done = self.time_step >= self.episode_length
        return self._obs(), self.last_reward(), done, {}

    def last_reward(self) -> float:
        """The reward of the step that led to the current (x, y, time_step) - a function of these alone."""
        if self.time_step >= self.episode_length:
            return float(self.y == self.goal_y) * self.goal_reward
        # behind the schedule x = t - o: -0.0 when it is not, kept as the reference forms it
        rew = float(self.x < self.time_step - self.oracle_length) * self.penalty
        if self.x == 0:
            rew = rew + self.distract_reward
        return rew


def parse_name(env_name: str):
    """'Mem-T-<passive|active>-<L>[-cont-act]-v0' -> TMaze keyword arguments (the reference's registration values), or None."""
    m = _NAME.match(env_name)
    if not m or int(m.group(2)) < 1:
        return None
    L = int(m.group(2))
    return dict(corridor_length=L, oracle_length=1 if m.group(1) == 'active' else 0, goal_reward=1.0, penalty=-1.0 / L,
                distract_reward=0.0, continuous_act_space=m.group(3) is not None)


def device_steppable(env) -> bool:
    """True for the environments `ops.tmaze_step` implements: a T-Maze with discrete actions."""
    return isinstance(env, TMaze) and not env.continuous_act_space
