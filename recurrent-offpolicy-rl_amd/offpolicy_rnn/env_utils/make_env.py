"""Environment factory (reference offpolicy_rnn/env_utils/make_env.py:41-72).

The simulator zoo of the reference (`envs/`) is out of scope.  Names of the form
`synthetic-o<obs>-a<act>-T<len>` (or `-d<n>-` for n discrete actions) build the Gaussian environment used by the benchmark / tests;
`Mem-T-{passive,active}-<L>[-cont-act]-v0` build the T-Maze memory task (env_utils/tmaze.py); `Wind-v0` builds the meta-RL task of
env_utils/wind.py with the reference's task split; `Catch-<runs>-v0` builds the delayed-reward task of env_utils/catch.py; anything
else - the other meta names included - is handed to `gym.make` when gym is installed and fails loudly otherwise."""
import re

import numpy as np


class Box:
    def __init__(self, low, high, shape, dtype=np.float32):
        self.low = np.full(shape, low, dtype=dtype)
        self.high = np.full(shape, high, dtype=dtype)
        self.shape = tuple(shape)
        self._rs = np.random.RandomState(0)

    def seed(self, s):
        self._rs = np.random.RandomState(s)

    def sample(self):
        return self._rs.uniform(-1, 1, self.shape)


class Discrete:
    def __init__(self, n):
        self.n, self.shape = n, ()
        self._rs = np.random.RandomState(0)

    def seed(self, s):
        self._rs = np.random.RandomState(s)

    def sample(self):
        return int(self._rs.randint(self.n))


class SyntheticEnv:
    """i.i.d. Gaussian observations / rewards, fixed horizon: the synthetic workload of BASELINE.json configs 2-4.
    `discrete=True`: `act_dim` discrete actions instead of a Box."""

    def __init__(self, obs_dim, act_dim, horizon, seed=0, discrete=False):
        self.observation_space = Box(-np.inf, np.inf, (obs_dim,))
        self.action_space = Discrete(act_dim) if discrete else Box(-1.0, 1.0, (act_dim,))
        self.horizon, self.t = horizon, 0
        self._rs = np.random.RandomState(seed)

    def seed(self, s):
        self._rs = np.random.RandomState(s)

    def reset(self, *a):
        self.t = 0
        return self._rs.randn(self.observation_space.shape[0])

    def step(self, action):
        self.t += 1
        return self._rs.randn(self.observation_space.shape[0]), float(self._rs.randn()), self.t >= self.horizon, {}


_SYN = re.compile(r'^synthetic-o(\d+)-([ad])(\d+)-T(\d+)$')          # a<n>: Box(n) actions, d<n>: n discrete actions


WIND_TASKS, WIND_TRAIN_TASKS, WIND_EVAL_TASKS = 60, 40, 20            # reference envs/pomdp_config.py 'Wind-v0'


def _make_wind(seed: int) -> dict:
    """Wind-v0 as reference envs/make_pomdp_env.py builds a meta environment: 60 tasks, shuffled by the permutation the reference draws
    under `fixed_seed(seed)` - `RandomState(seed).permutation(60)`, the global numpy stream stays as it is -, the first 40 for training
    and the last 20 for evaluation; one rollout per task, 75 steps.  The reference shares ONE object between `train_env` and `eval_env`
    (seeded `seed`, then `seed + 1`); this build keeps its convention of two objects, seeded `seed` and `seed + 1`: the environment has
    no random draw of its own after construction, so the two conventions behave alike."""
    from .wind import Wind
    env, eval_env = Wind(n_tasks=WIND_TASKS, seed=seed), Wind(n_tasks=WIND_TASKS, seed=seed + 1)
    shuffled = np.random.RandomState(seed).permutation(WIND_TASKS)
    return dict(train_env=env, eval_env=eval_env, train_tasks=shuffled[:WIND_TRAIN_TASKS], eval_tasks=shuffled[-WIND_EVAL_TASKS:],
                max_rollouts_per_task=1, max_trajectory_len=env.horizon_bamdp, obs_dim=2, act_dim=2, act_continuous=True, seed=seed,
                multiagent=False)


def make_env(env_name: str, seed: int) -> dict:
    m = _SYN.match(env_name)
    if m:
        obs, act, T = int(m.group(1)), int(m.group(3)), int(m.group(4))
        disc = m.group(2) == 'd'
        return dict(train_env=SyntheticEnv(obs, act, T, seed, disc), eval_env=SyntheticEnv(obs, act, T, seed + 1, disc), train_tasks=[],
                    eval_tasks=[None], max_rollouts_per_task=1, max_trajectory_len=T, obs_dim=obs, act_dim=act,
                    act_continuous=not disc, seed=seed, multiagent=False)
    from .tmaze import TMaze, parse_name
    kw = parse_name(env_name)
    if kw is not None:                                   # Mem-T-{passive,active}-<L>[-cont-act]-v0: the reference's T-Maze ids
        env, eval_env = TMaze(seed=seed, **kw), TMaze(seed=seed + 1, **kw)
        return dict(train_env=env, eval_env=eval_env, train_tasks=[], eval_tasks=[None], max_rollouts_per_task=1,
                    max_trajectory_len=env.episode_length, obs_dim=2, act_dim=4, act_continuous=env.continuous_act_space, seed=seed,
                    multiagent=False)
    if env_name == 'Wind-v0':
        return _make_wind(seed)
    from . import catch
    kw = catch.parse_name(env_name)
    if kw is not None:                                   # Catch-<runs>-v0: the reference's delayed-reward task
        env, eval_env = catch.Catch(seed=seed, **kw), catch.Catch(seed=seed + 1, **kw)
        return dict(train_env=env, eval_env=eval_env, train_tasks=[], eval_tasks=[None], max_rollouts_per_task=1,
                    max_trajectory_len=env.episode_length, obs_dim=49, act_dim=3, act_continuous=False, seed=seed, multiagent=False)
    try:
        import gym
    except ImportError as e:
        raise ImportError(f'environment {env_name!r} needs `gym` and the reference env zoo, which are outside this build; '
                          f'use synthetic-o<obs>-a<act>-T<len>') from e
    env, eval_env = gym.make(env_name), gym.make(env_name)
    T = getattr(env, '_max_episode_steps', 1000)
    cont = hasattr(env.action_space, 'low')
    return dict(train_env=env, eval_env=eval_env, train_tasks=[], eval_tasks=[None], max_rollouts_per_task=1,
                max_trajectory_len=T, obs_dim=env.observation_space.shape[0],
                act_dim=env.action_space.shape[0] if cont else env.action_space.n, act_continuous=cont, seed=seed, multiagent=False)
