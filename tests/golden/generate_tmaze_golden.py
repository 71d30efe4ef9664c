#!/usr/bin/env python3
"""Record the reference's T-Maze (envs/memory_envs/tmaze.py: TMazeClassicPassive / TMazeClassicActive, with the registration values
of envs/memory_envs/configs/tmaze_{passive,active}.py) into tests/golden/tmaze.npz.  Run by hand where the reference is checked out:

    RESEL_REFERENCE=<checkout of the reference> python tests/golden/generate_tmaze_golden.py          # writes tests/golden/tmaze.npz

The module is loaded by path; `gym` and `matplotlib.pyplot`, which it imports and the build does not have, are replaced by small
stubs, the way generate_golden.py replaces its missing imports.  The fixture holds recorded data only: per episode the variant,
corridor length, numpy seed and the goal side that seed drew, the actions fed, and the observations, rewards (float64: the
reference's -0.0 on unpenalised steps survives) and done flags that came back."""
import importlib.util
import os
import sys
import types

import numpy as np

REF = os.environ.get('RESEL_REFERENCE')
OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference():
    if not REF:
        sys.exit('set RESEL_REFERENCE to a checkout of the reference')
    gym = types.ModuleType('gym')

    class Env:
        pass

    class Box:
        def __init__(self, low=None, high=None, shape=None, dtype=np.float32):
            self.shape = tuple(shape) if shape is not None else np.shape(low)

    class Discrete:
        def __init__(self, n):
            self.n = n

        def contains(self, a):
            return int(a) == a and 0 <= a < self.n

    gym.Env, gym.spaces = Env, types.SimpleNamespace(Box=Box, Discrete=Discrete)
    mpl, plt = types.ModuleType('matplotlib'), types.ModuleType('matplotlib.pyplot')
    mpl.pyplot = plt
    sys.modules.update({'gym': gym, 'matplotlib': mpl, 'matplotlib.pyplot': plt})
    spec = importlib.util.spec_from_file_location('ref_tmaze', os.path.join(REF, 'envs', 'memory_envs', 'tmaze.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    meta, actions, obs, rewards, dones = [], [], [], [], []
    seen = dict(wall=0, vertical_in_corridor=0, oracle_twice=0, goal_up=0, goal_down=0)
    for active, lengths in ((0, (1, 3, 10)), (1, (1, 4))):
        for L in lengths:
            cls = ref.TMazeClassicActive if active else ref.TMazeClassicPassive
            env = cls(corridor_length=L, penalty=-1.0 / L, distract_reward=0.0)
            T, o = env.episode_length, env.oracle_length
            for goal in (-1, 1):
                seed = 0
                while True:                                  # the first numpy seed whose reset draws this goal side
                    np.random.seed(seed)
                    env.reset()
                    if env.goal_y == goal:
                        break
                    seed += 1
                turn = 1 if goal == 1 else 3
                optimal = [2] * o + [0] * (o + L) + [turn]
                wrong = optimal[:-1] + [4 - turn]
                probe = ([2, 2, 1, 3] + [0] * T)[:T - 1] + [turn]        # wall at x = 0, x = 0 seen again, vertical moves in the corridor
                rs = np.random.RandomState(7919 * (active + 1) + 31 * L + goal)
                scripts = [optimal, wrong, probe] + [[int(a) for a in rs.randint(0, 4, T)] for _ in range(5)]
                scripts.append([int(a) for a in rs.choice([0, 0, 0, 1, 3], T)])      # mostly right: reaches the junction and a goal cell
                for acts in scripts:
                    assert len(acts) == T
                    np.random.seed(seed)
                    ob = env.reset()
                    assert env.goal_y == goal
                    meta.append((active, L, seed, goal, T))
                    obs.append(ob)
                    at_oracle = int(env.x == 0)
                    for a in acts:
                        before = (env.x, env.y)
                        ob, r, d, info = env.step(a)
                        assert info == {} and isinstance(r, float)
                        seen['wall'] += (env.x, env.y) == before
                        seen['vertical_in_corridor'] += a in (1, 3) and before[0] < o + L
                        at_oracle += env.x == 0
                        actions.append(a)
                        obs.append(ob)
                        rewards.append(r)
                        dones.append(d)
                    assert d and not any(dones[-T:-1])
                    seen['oracle_twice'] += at_oracle >= 2
                    seen['goal_up'] += env.y == 1
                    seen['goal_down'] += env.y == -1
    assert all(v > 0 for v in seen.values()), seen
    out = dict(meta=np.array(meta, dtype=np.int64), actions=np.array(actions, dtype=np.int64), obs=np.array(obs, dtype=np.float32),
               rewards=np.array(rewards, dtype=np.float64), dones=np.array(dones, dtype=bool))
    assert np.signbit(out['rewards'][out['rewards'] == 0]).any(), 'the reference produces -0.0 on unpenalised steps'
    path = os.path.join(OUT, 'tmaze.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {len(meta)} episodes, {len(actions)} steps, {os.path.getsize(path)} bytes; coverage {seen}')


if __name__ == '__main__':
    main()
