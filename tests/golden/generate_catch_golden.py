#!/usr/bin/env python3
"""Record the reference's delayed Catch (envs/credit_assign/catch.py `DelayedCatch`, as `Catch-<runs>-v0` registers it: delay =
7 * (runs - 1) + 6, flattened image, integer actions) into tests/golden/catch.npz.  Run by hand where the reference is checked out:

    RESEL_REFERENCE=<checkout of the reference> python tests/golden/generate_catch_golden.py          # writes tests/golden/catch.npz

The module is loaded by path; `gym`, which it imports and the build does not have, is replaced by a small stub, the way
generate_tmaze_golden.py replaces its missing imports.  The fixture holds recorded data only: per episode the number of runs, the
numpy seed and the fruit / basket columns that seed drew (`ns`, `ms`), the actions fed, and the observations (int8: the canvas holds
-1, 0 and 1 only), rewards, done flags and `info['reward']` that came back."""
import importlib.util
import os
import sys
import types

import numpy as np

REF = os.environ.get('RESEL_REFERENCE')
OUT = os.path.dirname(os.path.abspath(__file__))
GRID = 7


def load_reference():
    if not REF:
        sys.exit('set RESEL_REFERENCE to a checkout of the reference')
    gym = types.ModuleType('gym')

    class Env:
        pass

    class Discrete:
        def __init__(self, n):
            self.n = n

    class MultiDiscrete:
        def __init__(self, nvec):
            self.nvec = np.asarray(nvec)

    gym.Env, gym.spaces = Env, types.SimpleNamespace(Discrete=Discrete, MultiDiscrete=MultiDiscrete)
    sys.modules.update({'gym': gym})
    spec = importlib.util.spec_from_file_location('ref_catch', os.path.join(REF, 'envs', 'credit_assign', 'catch.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def greedy(env, rs, p_random=0.0):
    """Towards the fruit's column; with probability p_random a random action instead."""
    _, col, basket = env.state[0]
    if rs.uniform() < p_random:
        return int(rs.randint(0, 3))
    return int(np.sign(col - basket)) + 1


def scripts_for(runs, rs):
    """[(name, seed, actions or a callable env -> action)]: about ten per runs."""
    T = GRID * runs - 1
    out = [('greedy', 0, lambda env: greedy(env, rs)), ('greedy', 1, lambda env: greedy(env, rs)),
           ('left', 2, [0] * T), ('right', 3, [2] * T), ('stay', 4, [1] * T)]
    out += [('random', 5 + k, [int(a) for a in rs.randint(0, 3, T)]) for k in range(4)]
    if runs > 1:                                         # two scripts that differ on the soft-reset steps t = 7k only
        base = [int(a) for a in rs.randint(0, 3, T)]
        other = [(a + 1 + (s // GRID) % 2) % 3 if (s + 1) % GRID == 0 else a for s, a in enumerate(base)]
        assert base != other
        out += [('soft-a', 9, base), ('soft-b', 9, other)]
    return out


def main():
    ref = load_reference()
    meta, ns_all, ms_all, actions, obs, rewards, dones, info_rewards = [], [], [], [], [], [], [], []
    seen = dict(catch=0, miss=0, clipped_left=0, clipped_right=0, single_entry=0, soft_pairs=0)
    rs = np.random.RandomState(20251)
    plans = [(runs, scripts_for(runs, rs)) for runs in (1, 2, 5)] + [(40, [('mostly-greedy', 11, lambda env: greedy(env, rs, 0.3))])]
    for runs, scripts in plans:
        env = ref.DelayedCatch(GRID * (runs - 1) + 6)
        T = env.delay
        assert env.num_catches == runs and T == GRID * runs - 1
        records = {}
        for name, seed, script in scripts:
            np.random.seed(seed)
            ob = env.reset()
            assert env.ns.shape == env.ms.shape == (runs,) and ob.shape == (GRID * GRID,)
            meta.append((runs, seed, T))
            ns_all.extend(int(v) for v in env.ns)
            ms_all.extend(int(v) for v in env.ms)
            first = len(obs)
            obs.append(ob)
            caught = 0
            for s in range(T):
                a = script(env) if callable(script) else script[s]
                soft = env.state[0, 0] == GRID - 1
                basket = int(env.state[0, 2])
                ob, r, d, info = env.step(a)
                assert set(info) == {'reward'} and ob.shape == (GRID * GRID,) and set(np.unique(ob)) <= {-1.0, 0.0, 1.0}
                assert soft == ((s + 1) % GRID == 0)
                if not soft:
                    seen['clipped_left'] += a == 0 and basket == 0
                    seen['clipped_right'] += a == 2 and basket == GRID - 1
                    if env.state[0, 0] == GRID - 1:
                        caught += info['reward']
                        seen['catch'] += info['reward'] == 1
                        seen['miss'] += info['reward'] == 0
                seen['single_entry'] += np.count_nonzero(ob) == 1
                actions.append(a)
                obs.append(ob)
                rewards.append(float(r))
                dones.append(bool(d))
                info_rewards.append(int(info['reward']))
            assert d and not any(dones[-T:-1]) and not any(rewards[-T:-1]) and rewards[-1] == caught
            if name == 'greedy':
                assert caught == runs
            if name.startswith('soft-'):
                records[name] = (np.array(obs[first:]), rewards[-T:], dones[-T:], info_rewards[-T:])
        if records:
            a, b = records['soft-a'], records['soft-b']
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
            seen['soft_pairs'] += 1
    assert all(v > 0 for v in seen.values()), seen
    obs = np.array(obs)
    assert np.array_equal(obs.astype(np.int8), obs)
    out = dict(meta=np.array(meta, dtype=np.int64), ns=np.array(ns_all, dtype=np.int64), ms=np.array(ms_all, dtype=np.int64),
               actions=np.array(actions, dtype=np.int64), obs=obs.astype(np.int8), rewards=np.array(rewards, dtype=np.float64),
               dones=np.array(dones, dtype=bool), info_rewards=np.array(info_rewards, dtype=np.int64))
    path = os.path.join(OUT, 'catch.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {len(meta)} episodes, {len(actions)} steps, {os.path.getsize(path)} bytes; coverage {seen}')


if __name__ == '__main__':
    main()
