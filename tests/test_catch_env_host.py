"""Catch without a GPU: the host environment (env_utils/catch.py) against what the reference's DelayedCatch recorded
(tests/golden/catch.npz, generate_catch_golden.py), hand-checked steps, the `make_env` names, the device record, the evaluation
scheduler over host environments, `train()` on the CPU op table, and the argument checks of `resel_catch_step` /
`resel_catch_collect_step` that return before the device is touched.  The environment is integer-valued: every comparison is exact."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from conftest import load_golden
from offpolicy_rnn.env_utils.catch import Catch, device_steppable, parse_name
from offpolicy_rnn.env_utils.make_env import Box, Discrete, make_env
from offpolicy_rnn.utility.policy_eval import run_episodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESEL_EINVAL = -1


def _episodes():
    g = load_golden('catch.npz')
    a0 = o0 = d0 = 0
    for runs, seed, T in g['meta'].tolist():
        yield (runs, seed, T, g['ns'][d0:d0 + runs], g['ms'][d0:d0 + runs], g['actions'][a0:a0 + T], g['obs'][o0:o0 + T + 1],
               g['rewards'][a0:a0 + T], g['dones'][a0:a0 + T], g['info_rewards'][a0:a0 + T])
        a0, o0, d0 = a0 + T, o0 + T + 1, d0 + runs
    assert a0 == len(g['actions']) and o0 == len(g['obs']) and d0 == len(g['ns']) == len(g['ms'])


def _greedy(env):
    return int(np.sign(env.fruit_col - env.basket)) + 1


# ------------------------------------------------------------------------------------------------ against the reference's record
def test_fixture_covers_what_it_should():
    eps = list(_episodes())
    assert sorted({e[0] for e in eps}) == [1, 2, 5, 40] and sum(e[0] == 40 for e in eps) == 1
    assert all(sum(e[0] == runs for e in eps) >= 9 for runs in (1, 2, 5))
    g = load_golden('catch.npz')
    assert g['obs'].dtype == np.int8 and g['obs'].shape[1] == 49 and set(np.unique(g['obs'])) == {-1, 0, 1}
    catch = miss = left = right = single = 0
    for runs, seed, T, ns, ms, actions, obs, rewards, dones, info in eps:
        assert T == 7 * runs - 1 and (0 <= ns).all() and (ns < 6).all() and (1 <= ms).all() and (ms < 5).all()
        assert not rewards[:-1].any() and rewards[-1] == info.sum() and dones.tolist() == [False] * (T - 1) + [True]
        for s in range(T):
            basket_before, basket = int(np.argmax(obs[s][42:])), int(np.argmax(obs[s + 1][42:]))
            if (s + 1) % 7 == 0:                                  # a soft reset reports nothing
                assert info[s] == 0
                continue
            left += actions[s] == 0 and basket_before == 0 and basket == 0
            right += actions[s] == 2 and basket_before == 6 and basket == 6
            if (s + 1) % 7 == 6:                                  # the fruit has reached the last row
                catch += info[s] == 1
                miss += info[s] == 0
                assert (np.count_nonzero(obs[s + 1]) == 1) == (info[s] == 1)
                single += np.count_nonzero(obs[s + 1]) == 1
    assert min(catch, miss, left, right, single) > 0
    pairs = 0                                                    # two scripts that differ on the soft-reset steps only: identical records
    for a in eps:
        for b in eps:
            if a is not b and a[:3] == b[:3] and not np.array_equal(a[5], b[5]):
                differ = np.nonzero(a[5] != b[5])[0]
                if ((differ + 1) % 7 == 0).all():
                    assert all(np.array_equal(x, y) for x, y in zip(a[6:], b[6:]))
                    pairs += 1
    assert pairs >= 2
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', 'catch.npz')) < 100 * 1024


@pytest.mark.parametrize('explicit', [True, False])
def test_host_env_equals_the_reference_record(explicit):
    """explicit False: `seed(s)` + `reset()` draws what the reference drew from numpy's global stream seeded with s."""
    n = 0
    for runs, seed, T, ns, ms, actions, obs, rewards, dones, info in _episodes():
        env = make_env(f'Catch-{runs}-v0', 0)['train_env']
        assert env.episode_length == T
        if explicit:
            ob = env.reset(fruits=(ns, ms))
        else:
            env.seed(seed)
            ob = env.reset()
        assert np.array_equal(env.ns, ns) and np.array_equal(env.ms, ms)
        got_obs, got_rew, got_done = [ob], [], []
        for s, a in enumerate(actions):
            before = env.accumulated
            ob, r, d, extra = env.step(int(a))
            assert type(r) is float and type(d) is bool and extra == {} and ob.dtype == np.float32 and ob.shape == (49,)
            assert env.accumulated - before == info[s]           # what the reference reports as info['reward']
            got_obs.append(ob)
            got_rew.append(r)
            got_done.append(d)
        assert np.array_equal(np.array(got_obs), obs.astype(np.float32)), (runs, seed)
        assert np.array_equal(np.array(got_rew), rewards) and got_done == dones.tolist(), (runs, seed)
        n += 1
    assert n == 32


def test_reset_draws_from_the_private_stream_only():
    state = np.random.get_state()
    env = Catch(5)
    env.seed(4)
    env.reset()
    a = (env.ns.tolist(), env.ms.tolist())
    env.seed(4)
    ns, ms = env.draw_fruits()
    assert a == (ns.tolist(), ms.tolist())
    rs = np.random.RandomState(4)                                # exactly the reference's two calls
    assert a == (rs.randint(0, 6, size=5).tolist(), rs.randint(1, 5, size=5).tolist())
    after, mine = rs.get_state(), env._rs.get_state()
    assert np.array_equal(after[1], mine[1]) and after[2] == mine[2]
    now = np.random.get_state()
    assert now[0] == state[0] and np.array_equal(now[1], state[1]) and now[2:] == state[2:]


def test_the_object_pickles():
    env = Catch(2, seed=3)
    env.reset()
    env.step(2)
    twin = pickle.loads(pickle.dumps(env))
    for a in (0, 1, 2, 2, 0, 1, 1, 0, 2, 1, 0, 2):
        x, y = env.step(a), twin.step(a)
        assert np.array_equal(x[0], y[0]) and x[1:] == y[1:]
    assert x[2] and np.array_equal(env.draw_fruits(), twin.draw_fruits())


# ------------------------------------------------------------------------------------------------ hand-checked steps
def test_runs_1_by_hand():
    env = Catch(1)
    ob = env.reset(fruits=([4], [2]))
    assert env.episode_length == 6 and np.nonzero(ob)[0].tolist() == [4, 44] and ob[4] == -1.0 and ob[44] == 1.0
    for s, a in enumerate((2, 2, 1, 1, 0, 2)):                   # right, right, stay, stay, left (to 3), right (to 4): under the fruit
        ob, r, d, _ = env.step(a)
        if s < 5:
            assert r == 0.0 and not d and ob[7 * (s + 1) + 4] == -1.0
    assert r == 1.0 and d and np.nonzero(ob)[0].tolist() == [46] and ob[46] == 1.0           # the basket covers the fruit
    env.reset(fruits=([0], [1]))
    for a in (0, 0, 0, 2, 2, 2):                                 # clipped at column 0, then away from the fruit
        ob, r, d, _ = env.step(a)
    assert r == 0.0 and d and np.nonzero(ob)[0].tolist() == [42, 45] and env.basket == 3
    with pytest.raises(AssertionError):
        env.step(3)


@pytest.mark.parametrize('runs', [1, 2, 5, 40])
def test_greedy_catcher_returns_exactly_runs(runs):
    env = Catch(runs, seed=runs)
    for _ in range(3):
        env.reset()
        ret, done, steps = 0.0, False, 0
        while not done:
            _, r, done, _ = env.step(_greedy(env))
            ret += r
            steps += 1
        assert ret == float(runs) and steps == 7 * runs - 1


# ------------------------------------------------------------------------------------------------ make_env
@pytest.mark.parametrize('runs', [1, 2, 40])
def test_make_env_names(runs):
    c = make_env(f'Catch-{runs}-v0', seed=3)
    assert c['obs_dim'] == 49 and c['act_dim'] == 3 and c['max_trajectory_len'] == 7 * runs - 1 and c['act_continuous'] is False
    assert c['train_env'] is not c['eval_env'] and isinstance(c['train_env'], Catch) and isinstance(c['eval_env'], Catch)
    assert c['eval_tasks'] == [None] and c['train_tasks'] == [] and c['seed'] == 3 and not c['multiagent'] and c['max_rollouts_per_task'] == 1
    env = c['train_env']
    assert isinstance(env.observation_space, Box) and env.observation_space.shape == (49,)
    assert isinstance(env.action_space, Discrete) and env.action_space.n == 3
    assert env.device_config() == dict(num_catches=runs, episode_length=7 * runs - 1) and device_steppable(env)
    twin, twin_eval = Catch(runs, seed=3), Catch(runs, seed=4)   # train / eval objects are seeded seed / seed + 1
    for got, want in ((c['train_env'], twin), (c['eval_env'], twin_eval)):
        for _ in range(4):
            assert [v.tolist() for v in got.draw_fruits()] == [v.tolist() for v in want.draw_fruits()]


def test_names_that_are_not_catches_still_fail_loudly():
    assert parse_name('Catch-5-v0') == dict(runs=5) and parse_name('Catch-0-v0') is None and parse_name('Catch-5-v1') is None
    for name in ('Catch-0-v0', 'Catch-5-v1', 'KeytoDoor-SR-v0'):
        with pytest.raises(ImportError):
            make_env(name, 0)


# ------------------------------------------------------------------------------------------------ the per-environment record
def test_record_of_the_device_environment():
    from offpolicy_rnn.env_utils.device_env import GRID_KINDS, KINDS, CatchKind, TMazeKind, WindKind, device_env_kind
    from offpolicy_rnn.hip import _lib
    assert device_env_kind(make_env('Catch-5-v0', 0)['train_env']) is CatchKind
    assert device_env_kind(make_env('Catch-40-v0', 0)['train_env']) is CatchKind
    assert device_env_kind(make_env('Catch-41-v0', 0)['train_env']) is None and not device_steppable(Catch(41))
    assert KINDS == (TMazeKind, WindKind) and GRID_KINDS == (CatchKind,)
    assert (CatchKind.obs_dim, CatchKind.act_dim, CatchKind.categorical) == (49, 3, True)
    assert CatchKind.MAX_RUNS == _lib.CATCH_MAX_RUNS and CatchKind.STATE_WORDS == _lib.CATCH_STATE_WORDS
    assert CatchKind.state_bytes == 4 * _lib.CATCH_STATE_WORDS and CatchKind.state_bytes % 8 == 0
    assert CatchKind.payload_width == _lib.CATCH_PAYLOAD_WORDS == 80 and CatchKind.book_offset == 24 and CatchKind.eval_extras(2) == {}
    # payloads: each row's own stream, in the row's episode order, padded to 80
    envs, twins = [Catch(2, seed=r) for r in range(3)], [Catch(2, seed=r) for r in range(3)]
    pay = CatchKind.eval_payloads(envs, 7, None)
    for k in range(7):                                           # rows 0, 1, 2, 0, 1, 2, 0
        ns, ms = twins[k % 3].draw_fruits()
        assert pay[k].dtype == np.int32 and pay[k].shape == (80,)
        assert pay[k][:2].tolist() == ns.tolist() and pay[k][40:42].tolist() == ms.tolist() and not pay[k][2:40].any() and not pay[k][42:].any()
    # the training environment: the draw is recorded in the object, and the state words bring every field back
    alg = type('A', (), dict(env=Catch(2, seed=9)))
    row = CatchKind.next_payload(alg)
    assert row[:2].tolist() == alg.env.ns.tolist() and row[40:42].tolist() == alg.env.ms.tolist()
    assert np.array_equal(CatchKind.current_payload(alg.env), row)
    assert CatchKind.behind_reset(Catch(2)) and alg.env.reset() is not None and CatchKind.behind_reset(alg.env)
    alg.env.step(1)
    assert not CatchKind.behind_reset(alg.env)


# ------------------------------------------------------------------------------------------------ the scheduler over host environments
@pytest.mark.parametrize('runs, n', [(1, 5), (2, 7)])
def test_run_episodes_with_a_scripted_catcher_reaches_runs(runs, n):
    rows = 3
    envs = [Catch(runs, seed=10 + r) for r in range(rows)]

    def step(state, lst_state, lst_action, reward, reset):
        """Reads the canvas: towards the fruit's column (anything on a soft-reset step, whose fruit the basket covers or has missed)."""
        mode = np.ones((rows, 1), dtype=np.int64)
        for r in range(rows):
            fruit, basket = np.nonzero(state[r] == -1)[0], np.nonzero(state[r] == 1)[0]
            if len(fruit) and len(basket):
                mode[r, 0] = int(np.sign(fruit[0] % 7 - basket[0] % 7)) + 1
        return mode

    out, ep_rows = run_episodes(step, envs, n, 49, 3, lambda e: e.reset(), discrete=True)
    assert list(out) == ['EpRetTest', 'EpLenTest']
    assert out['EpRetTest'] == [float(runs)] * n and out['EpLenTest'] == [7 * runs - 1] * n
    assert ep_rows == [k % rows for k in range(n)]


def test_train_runs_on_a_catch_name(oracle_ops, tmp_path, monkeypatch):
    """`alg.train()` with the discrete SAC trainer, one host environment per step (test_train_runs_on_a_tmaze_name's settings)."""
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    alg = alg_init(make_parameter('gru', env='Catch-2-v0', total_iteration=2, step_per_iteration=20, random_num=30,
                                  start_train_num=26, update_interval=5, sac_batch_size=26))
    assert alg.discrete_env and alg.obs_dim == 49 and alg.act_dim == 3 and isinstance(alg.env, Catch) and alg.env is not alg.eval_env
    assert alg.max_episode_steps == 13
    alg.train()
    assert alg.sample_num >= 30 + 40 and alg.grad_num >= 4 and len(alg.replay_buffer) >= 4       # thirteen-step episodes
    pickle.loads(pickle.dumps(alg.env))


# ------------------------------------------------------------------------------------------------ argument checks of the kernel entries
@pytest.fixture(scope='module')
def lib():
    from offpolicy_rnn.hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('resel_catch_step', 'resel_catch_collect_step'):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


def _cfg(runs=2, T=None):
    from offpolicy_rnn.hip._lib import CatchCfg
    return CatchCfg(runs, 7 * runs - 1 if T is None else T)


BAD_CFGS = [(0, -1), (0, 6), (41, 286), (41, 279), (2, 12), (2, 14), (40, 278)]


def test_catch_step_rejects_bad_arguments_before_touching_the_device(lib):
    """Nothing here is a device pointer: a call that got past the argument checks would fault, not return."""
    fake = 0x1000
    ptrs = ('action', 'draws', 'n_episodes', 'env_state', 'ret_acc', 'ep_ret', 'ep_len', 'in_block', 'flags')

    def call(B=3, A=3, J=2, ld_action=5, ld_draws=160, ld_ep=2, ld_in=102, init=0, cfg=None, **p):
        q = {k: p.get(k, fake) for k in ptrs}
        return lib.resel_catch_step(cfg or _cfg(), init, q['action'], ld_action, q['draws'], ld_draws, q['n_episodes'], J, q['env_state'],
                                    q['ret_acc'], q['ep_ret'], q['ep_len'], ld_ep, q['in_block'], ld_in, A, q['flags'], B, None)

    for name in ptrs:
        assert call(**{name: None}) == RESEL_EINVAL, name
        assert call(init=1, **{name: None}) == RESEL_EINVAL, name
    assert call(A=4) == RESEL_EINVAL and call(A=2) == RESEL_EINVAL and call(B=-1) == RESEL_EINVAL
    assert call(ld_in=101) == RESEL_EINVAL and call(ld_action=0) == RESEL_EINVAL
    assert call(J=0) == RESEL_EINVAL and call(ld_draws=159) == RESEL_EINVAL and call(ld_ep=1) == RESEL_EINVAL
    for runs, T in BAD_CFGS:
        assert call(cfg=_cfg(runs, T)) == RESEL_EINVAL, (runs, T)
    assert call(B=0) == 0 and call(B=0, init=1, cfg=_cfg(40)) == 0 and call(B=0, cfg=_cfg(1)) == 0      # nothing to do: nothing launched


def test_catch_collect_step_rejects_bad_arguments_before_touching_the_device(lib):
    from offpolicy_rnn.hip._lib import COLLECT_FIELDS, CollectLayout
    fake = 0x1000
    ptrs = ('action', 'draws', 'env_state', 'ret_acc', 'traj', 'in_block')
    widths = dict(state=49, last_state=49, last_action=3, next_state=49, logp=0)

    def layout(**over):
        lay, off = CollectLayout(), 0
        for name in COLLECT_FIELDS:
            w = widths.get(name, 1)
            setattr(lay, name, off if w else -1)
            off += w
        for k, v in over.items():
            setattr(lay, k, v)
        return lay, off

    assert layout()[1] == 157 and layout()[0].timeout == 156 and layout()[0].logp == -1 and layout()[0].next_state == 102

    def call(B=2, A=3, ld_action=5, T_cap=13, ld_row=157, steps=13, ld_in=102, init=0, cfg=None, lay=None, **p):
        q = {k: p.get(k, fake) for k in ptrs}
        return lib.resel_catch_collect_step(cfg or _cfg(), lay or layout()[0], init, q['action'], ld_action, q['draws'], q['env_state'],
                                            q['ret_acc'], q['traj'], T_cap, ld_row, steps, q['in_block'], ld_in, A, B, None)

    for name in ptrs:
        assert call(**{name: None}) == RESEL_EINVAL, name
        assert call(init=1, **{name: None}) == RESEL_EINVAL, name
    assert call(A=4) == RESEL_EINVAL and call(B=-1) == RESEL_EINVAL and call(T_cap=0) == RESEL_EINVAL and call(steps=0) == RESEL_EINVAL
    assert call(ld_in=101) == RESEL_EINVAL and call(ld_action=0) == RESEL_EINVAL and call(ld_row=156) == RESEL_EINVAL
    assert call(lay=layout(logp=3)[0]) == RESEL_EINVAL
    for field in ('state', 'last_state', 'next_state'):          # a 49-wide field that ends past ld_row: 109 + 49 > 157
        assert call(lay=layout(**{field: 109})[0]) == RESEL_EINVAL, field
        assert call(B=0, lay=layout(**{field: 108})[0]) == 0, field
    assert call(lay=layout(last_action=155)[0]) == RESEL_EINVAL  # three columns wide: 155 + 3 > 157
    for runs, T in BAD_CFGS:
        assert call(cfg=_cfg(runs, T)) == RESEL_EINVAL, (runs, T)
    assert call(B=0) == 0 and call(B=0, init=1) == 0 and call(B=0, lay=layout(timeout=-1)[0], ld_row=156) == 0


def test_cfg_struct_state_words_and_prototypes_match_the_header():
    from offpolicy_rnn.hip import _lib
    assert ctypes.sizeof(_lib.CatchCfg) == 8 and _lib.CatchCfg.num_catches.offset == 0 and _lib.CatchCfg.episode_length.offset == 4
    header = open(os.path.join(ROOT, 'include', 'resel_hip.h')).read()
    assert int(re.search(r'#define\s+RESEL_CATCH_MAX_RUNS\s+(\d+)', header).group(1)) == _lib.CATCH_MAX_RUNS == 40
    words = int(re.search(r'#define\s+RESEL_CATCH_STATE_WORDS\s+(\d+)', header).group(1))
    assert words == _lib.CATCH_STATE_WORDS == 6 + 3 + 1 + 2 * _lib.CATCH_MAX_RUNS and words % 2 == 0            # 8-byte aligned rows
    assert re.search(r'typedef struct \{ int32_t num_catches, episode_length; \} resel_catch_cfg_t;', header)
    from test_host_logic import test_ctypes_signatures_match_the_header_prototypes
    assert 'resel_catch_step' in _lib.SIGNATURES and 'resel_catch_collect_step' in _lib.SIGNATURES
    test_ctypes_signatures_match_the_header_prototypes()         # the generic check covers the two new prototypes
