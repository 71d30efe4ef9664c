#!/usr/bin/env python3
"""Record the reference's Wind-v0 (envs/meta/toy_navigation/wind.py `WindEnv` behind envs/meta/wrappers.py `VariBadWrapper`, built the
way envs/meta/make_env.py and envs/make_pomdp_env.py build a meta environment from the 'Wind-v0' entry of envs/pomdp_config.py) into
tests/golden/wind_v0.npz.  Run by hand where the reference is checked out:

    RESEL_REFERENCE=<checkout of the reference> python tests/golden/generate_wind_golden.py           # writes tests/golden/wind_v0.npz

The two modules are loaded by path behind a `gym` stub - `Env`, a `Wrapper` that forwards attributes, `spaces.Box` - and
`matplotlib` is not needed.  The fixture holds recorded data only.  For each of the seeds 1 and 3: the 60 winds, the train / eval split,
and for three tasks (two training tasks, one evaluation task) two scripted episodes of 75 steps each - the normalised actions fed
(float64: as the script produced them, so that float32 scripts stay float32 values) and the observations (reset first), rewards and
done flags that came back, in float64 / bool:
  noise: uniform in [-1.5, 1.5], so that the clip to [-1, 1] and the clip to the inner bounds both act;
  seek:  clip((goal - state - wind) / 0.1, -1, 1) cast to float32 - it reaches the goal ball, so the rewards are not all zero."""
import importlib.util
import os
import random
import sys
import types

import numpy as np

REF = os.environ.get('RESEL_REFERENCE')
OUT = os.path.dirname(os.path.abspath(__file__))
SEEDS, N_TASKS, N_TRAIN, N_EVAL, EPISODES_PER_TASK = (1, 3), 60, 40, 20, 1          # envs/pomdp_config.py 'Wind-v0'


def load_reference():
    if not REF:
        sys.exit('set RESEL_REFERENCE to a checkout of the reference')
    gym = types.ModuleType('gym')

    class Env:
        def seed(self, seed=None):
            return [seed]

        @property
        def unwrapped(self):
            return self

    class Wrapper(Env):
        def __init__(self, env):
            self.env = env

        def __getattr__(self, name):                         # only what the wrapper itself does not have
            if name.startswith('_') and name != '_max_episode_steps':
                raise AttributeError(name)
            return getattr(self.env, name)

        def seed(self, seed=None):
            return self.env.seed(seed)

        @property
        def unwrapped(self):
            return self.env.unwrapped

    class Box:
        def __init__(self, low=None, high=None, shape=None, dtype=np.float32):
            shape = tuple(shape) if shape is not None else np.shape(low)
            self.low, self.high = np.full(shape, low, dtype=dtype), np.full(shape, high, dtype=dtype)
            self.shape, self.dtype, self.np_random = shape, np.dtype(dtype), np.random.RandomState()

    spaces = types.ModuleType('gym.spaces')
    spaces.Box = Box
    registration = types.ModuleType('gym.envs.registration')
    registration.load = registration.register = lambda *a, **k: None
    envs = types.ModuleType('gym.envs')
    envs.registration = registration
    gym.Env, gym.Wrapper, gym.spaces, gym.envs = Env, Wrapper, spaces, envs
    gym.make = lambda *a, **k: sys.exit('the stub builds no environment by name')
    sys.modules.update({'gym': gym, 'gym.spaces': spaces, 'gym.envs': envs, 'gym.envs.registration': registration})
    pkg = types.ModuleType('ref_meta')                       # a package around envs/meta, so that the wrapper's relative import resolves
    pkg.__path__ = [os.path.join(REF, 'envs', 'meta')]
    sys.modules['ref_meta'] = pkg

    def load(name, *path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, 'envs', 'meta', *path))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    return load('ref_meta.toy_navigation_wind', 'toy_navigation', 'wind.py'), load('ref_meta.wrappers', 'wrappers.py'), Box


def make(ref_wind, ref_wrappers, Box, seed):
    """envs/meta/make_env.py `make_env` + the meta branch of envs/make_pomdp_env.py `_make_pomdp_env` + `regularize_space`, under the
    `fixed_seed(seed)` of offpolicy_rnn/env_utils/make_env.py - with the class built directly where they go through `gym.make`."""
    saved = np.random.get_state(), random.getstate()
    np.random.seed(seed)
    random.seed(seed)
    try:
        inner = np.random.get_state(), random.getstate()     # the inner fixed_seed(seed) around the construction
        np.random.seed(seed)
        random.seed(seed)
        env = ref_wind.WindEnv(n_tasks=N_TASKS)
        np.random.set_state(inner[0])
        random.setstate(inner[1])
        env.seed(seed)
        env.action_space.np_random.seed(seed)
        env = ref_wrappers.VariBadWrapper(env=env, episodes_per_task=EPISODES_PER_TASK, oracle=False)
        env.seed(seed + 1)                                   # eval_env is the same object
        shuffled = np.random.permutation(env.get_all_task_idx())
    finally:
        np.random.set_state(saved[0])
        random.setstate(saved[1])
    env.action_space = Box(low=-np.ones((2,)), high=np.ones((2,)), dtype=np.float64)
    return env, shuffled[:N_TRAIN], shuffled[-N_EVAL:]


def episode(env, task, script, rs):
    wind, goal = np.array(env.winds[task]), np.array([0.0, 1.0])
    ob = env.reset(task=task)
    actions, obs, rewards, dones = [], [ob], [], []
    for _ in range(env.horizon_bamdp):
        if script == 'noise':
            a = rs.uniform(-1.5, 1.5, 2)
        else:
            a = np.clip((goal - ob - wind) / 0.1, -1, 1).astype(np.float32)
        ob, r, d, info = env.step(a)
        assert info == {'done_mdp': d} and isinstance(r, float) and ob.dtype == np.float64
        actions.append(np.asarray(a, dtype=np.float64))
        obs.append(ob)
        rewards.append(r)
        dones.append(d)
    assert d and not any(dones[:-1])
    return np.array(actions), np.array(obs), np.array(rewards), np.array(dones)


def main():
    ref_wind, ref_wrappers, Box = load_reference()
    out, returns = {}, []
    for seed in SEEDS:
        env, train, evals = make(ref_wind, ref_wrappers, Box, seed)
        assert env.meta_env_flag and env.n_tasks == N_TASKS and env.horizon_bamdp == 75 and env.action_space.low.dtype == np.float64
        tasks = [int(train[0]), int(train[-1]), int(evals[0])]
        out.update({f's{seed}_winds': np.array(env.winds, dtype=np.float64), f's{seed}_train_tasks': np.asarray(train, dtype=np.int64),
                    f's{seed}_eval_tasks': np.asarray(evals, dtype=np.int64), f's{seed}_tasks': np.array(tasks, dtype=np.int64)})
        for script in ('noise', 'seek'):
            rs = np.random.RandomState(1000 * seed + len(script))
            rec = [episode(env, t, script, rs) for t in tasks]
            for k, name in enumerate(('actions', 'obs', 'reward', 'done')):
                out[f's{seed}_{script}_{name}'] = np.stack([r[k] for r in rec])
            returns.append((seed, script, [float(r[2].sum()) for r in rec]))
            if script == 'noise':
                a = out[f's{seed}_noise_actions']
                assert (np.abs(a) > 1).any() and (np.abs(a) < 1).any()
            else:
                assert all(r[2].sum() > 0 for r in rec), 'the goal-seeking script reaches the goal ball'
    path = os.path.join(OUT, 'wind_v0.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes; returns {returns}')


if __name__ == '__main__':
    main()
