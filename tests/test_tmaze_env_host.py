"""T-Maze without a GPU: the host environment (env_utils/tmaze.py) against what the reference's TMazeClassicPassive / TMazeClassicActive
recorded (tests/golden/tmaze.npz, generate_tmaze_golden.py) - exact, signed zeros included -, hand-checked steps, the four `make_env`
names, the evaluation scheduler over host T-Mazes, and the argument checks of `resel_tmaze_step` that return before the device is
touched."""
import ctypes
import os

import numpy as np
import pytest

from conftest import load_golden
from offpolicy_rnn.env_utils.make_env import Box, Discrete, make_env
from offpolicy_rnn.env_utils.tmaze import TMaze, device_steppable
from offpolicy_rnn.utility.policy_eval import run_episodes

RESEL_EINVAL = -1


def _episodes():
    g = load_golden('tmaze.npz')
    a0 = o0 = 0
    for active, L, seed, goal, T in g['meta'].tolist():
        yield (active, L, seed, goal, T, g['actions'][a0:a0 + T], g['obs'][o0:o0 + T + 1], g['rewards'][a0:a0 + T], g['dones'][a0:a0 + T])
        a0, o0 = a0 + T, o0 + T + 1
    assert a0 == len(g['actions']) and o0 == len(g['obs'])


def _env(active, L):
    return make_env(f'Mem-T-{"active" if active else "passive"}-{L}-v0', 0)['train_env']


# ------------------------------------------------------------------------------------------------ against the reference's record
def test_fixture_covers_what_it_should():
    eps = list(_episodes())
    assert {(a, L) for a, L, *_ in eps} == {(0, 1), (0, 3), (0, 10), (1, 1), (1, 4)}
    assert {g for _, _, _, g, *_ in eps} == {-1, 1}
    rew = np.concatenate([e[7] for e in eps])
    assert np.signbit(rew[rew == 0]).any() and (~np.signbit(rew[rew == 0])).any()      # both zeros occur
    assert any(e[7][-1] == 1.0 for e in eps) and any(e[7][-1] == 0.0 for e in eps)
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', 'tmaze.npz')) < 100 * 1024


@pytest.mark.parametrize('explicit_goal', [True, False])
def test_host_env_equals_the_reference_record(explicit_goal):
    """explicit_goal False: `seed(s)` + `reset()` draws what the reference drew from numpy's global stream seeded with s."""
    n = 0
    for active, L, seed, goal, T, actions, obs, rewards, dones in _episodes():
        env = _env(active, L)
        assert env.episode_length == T
        if explicit_goal:
            ob = env.reset(goal=goal)
        else:
            env.seed(seed)
            ob = env.reset()
        assert env.goal_y == goal
        got_obs, got_rew, got_done = [ob], [], []
        for a in actions:
            ob, r, d, info = env.step(int(a))
            assert type(r) is float and info == {} and ob.dtype == np.float32 and ob.shape == (2,)
            got_obs.append(ob)
            got_rew.append(r)
            got_done.append(d)
        got_obs, got_rew = np.array(got_obs), np.array(got_rew, dtype=np.float64)
        assert np.array_equal(got_obs, obs) and np.array_equal(np.signbit(got_obs), np.signbit(obs)), (active, L, seed)
        assert np.array_equal(got_rew, rewards) and np.array_equal(np.signbit(got_rew), np.signbit(rewards)), (active, L, seed)
        assert got_done == dones.tolist()
        n += 1
    assert n == 90


def test_reset_draws_from_the_private_stream_only():
    state = np.random.get_state()
    env = _env(0, 3)
    env.seed(4)
    a = [env.reset()[1] for _ in range(20)]
    env.seed(4)
    b = [float(env.draw_goal()) for _ in range(20)]
    assert a == b and set(a) == {-1.0, 1.0}
    now = np.random.get_state()
    assert now[0] == state[0] and np.array_equal(now[1], state[1]) and now[2:] == state[2:]


# ------------------------------------------------------------------------------------------------ hand-checked steps
def test_passive_l1_by_hand():
    env = _env(0, 1)
    assert env.reset(goal=-1).tolist() == [0.0, -1.0]
    ob, r, d, _ = env.step(1)                                     # up from the start: off the map, behind the schedule
    assert (env.x, env.y) == (0, 0) and ob.tolist() == [0.0, 0.0] and not np.signbit(ob[1]) and r == -1.0 and not d
    ob, r2, d, _ = env.step(3)
    assert r2 == 0.0 and d and r + r2 == -1.0


def test_active_l2_by_hand():
    env = _env(1, 2)
    assert env.episode_length == 5 and env.reset(goal=-1).tolist() == [0.0, 0.0]
    rews = []
    for a in (1, 3, 0, 0, 3):
        ob, r, d, _ = env.step(a)
        rews.append(r)
    assert rews[:4] == [0.0] * 4 and all(np.signbit(r) for r in rews[:4]) and rews[4] == 1.0 and d
    assert ob.tolist() == [1.0, -1.0]


def test_optimal_return_is_exactly_one():
    for active, L in ((0, 1), (0, 7), (1, 1), (1, 5), (0, 1000)):
        for goal in (-1, 1):
            env = _env(active, L)
            env.reset(goal=goal)
            o, ret = env.oracle_length, 0.0
            for a in [2] * o + [0] * (o + L) + [1 if goal == 1 else 3]:
                _, r, d, _ = env.step(a)
                ret += r
            assert d and ret == 1.0


# ------------------------------------------------------------------------------------------------ make_env
@pytest.mark.parametrize('name, T, cont', [('Mem-T-passive-3-v0', 4, False), ('Mem-T-active-3-v0', 6, False),
                                           ('Mem-T-passive-10-cont-act-v0', 11, True), ('Mem-T-active-1-cont-act-v0', 4, True)])
def test_make_env_names(name, T, cont):
    c = make_env(name, seed=3)
    assert c['obs_dim'] == 2 and c['act_dim'] == 4 and c['max_trajectory_len'] == T and c['act_continuous'] is cont
    assert c['train_env'] is not c['eval_env'] and isinstance(c['train_env'], TMaze) and isinstance(c['eval_env'], TMaze)
    assert c['eval_tasks'] == [None] and c['train_tasks'] == [] and c['seed'] == 3 and not c['multiagent']
    env = c['train_env']
    assert isinstance(env.observation_space, Box) and env.observation_space.shape == (2,)
    assert isinstance(env.action_space, Box if cont else Discrete)
    assert env.penalty == -1.0 / env.corridor_length and env.goal_reward == 1.0 and env.distract_reward == 0.0
    assert device_steppable(env) is (not cont)
    # train / eval objects are seeded seed / seed + 1
    twin, twin_eval = TMaze(env.corridor_length, seed=3), TMaze(env.corridor_length, seed=4)
    assert [c['train_env'].draw_goal() for _ in range(16)] == [twin.draw_goal() for _ in range(16)]
    assert [c['eval_env'].draw_goal() for _ in range(16)] == [twin_eval.draw_goal() for _ in range(16)]


def test_names_that_are_not_tmazes_still_fail_loudly():
    for name in ('Mem-T-passive-0-v0', 'Mem-T-sideways-3-v0', 'Mem-T-passive-3-v1'):
        with pytest.raises(ImportError):
            make_env(name, 0)


def test_continuous_variant_takes_the_first_maximum():
    env = make_env('Mem-T-passive-3-cont-act-v0', 0)['train_env']
    env.reset(goal=1)
    env.step(np.array([0.5, 0.5, -1.0, 0.5]))                    # tie between 0, 1 and 3: action 0, one cell to the right
    assert (env.x, env.y) == (1, 0)
    env.step(np.array([-1.0, -1.0, -1.0, -1.0]))                 # all equal: action 0 again
    assert (env.x, env.y) == (2, 0)
    env.step(np.array([[-0.2, 0.1, 0.3, 0.3]]))                  # any shape, flattened: action 2
    assert (env.x, env.y) == (1, 0)


# ------------------------------------------------------------------------------------------------ the scheduler over host T-Mazes
@pytest.mark.parametrize('active, L, n', [(0, 3, 7), (1, 2, 5)])
def test_run_episodes_with_a_memory_policy_is_optimal(active, L, n):
    rows = 3
    envs = [_env(active, L) for _ in range(rows)]
    for r, e in enumerate(envs):
        e.seed(10 + r)
    o, T = envs[0].oracle_length, envs[0].episode_length
    memory, t = np.zeros(rows), np.zeros(rows, dtype=np.int64)

    def step(state, lst_state, lst_action, reward, reset):
        """Left to the oracle, remember what it shows, right along the corridor, turn to the remembered side on the last step."""
        mode = np.zeros((rows, 1), dtype=np.int64)
        for r in range(rows):
            if reset[r]:
                memory[r], t[r] = 0.0, 0
            if state[r, 0] == 0 and state[r, 1] != 0:
                memory[r] = state[r, 1]
            mode[r, 0] = 2 if t[r] < o else (0 if t[r] < T - 1 else (1 if memory[r] > 0 else 3))
            t[r] += 1
        return mode

    out, ep_rows = run_episodes(step, envs, n, 2, 4, lambda e: e.reset(), discrete=True)
    assert out['EpRetTest'] == [1.0] * n and out['EpLenTest'] == [T] * n
    assert ep_rows == [k % rows for k in range(n)]               # equal lengths: episode k runs on row k % rows


def test_train_runs_on_a_tmaze_name(oracle_ops, tmp_path, monkeypatch):
    """`alg.train()` with the discrete SAC trainer, one host environment per step (tests/test_host_logic.py::test_train_loop_end_to_end's
    settings on the CPU op table)."""
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    alg = alg_init(make_parameter('gru', env='Mem-T-passive-3-v0', total_iteration=2, step_per_iteration=20, random_num=30,
                                  start_train_num=24, update_interval=5, sac_batch_size=24))
    assert alg.discrete_env and alg.obs_dim == 2 and alg.act_dim == 4 and isinstance(alg.env, TMaze) and alg.env is not alg.eval_env
    alg.train()
    assert alg.sample_num >= 30 + 40 and alg.grad_num >= 4 and len(alg.replay_buffer) >= 10      # four-step episodes


# ------------------------------------------------------------------------------------------------ argument checks of the kernel entry
@pytest.fixture(scope='module')
def lib():
    from offpolicy_rnn.hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    h.resel_tmaze_step.restype, h.resel_tmaze_step.argtypes = _lib.SIGNATURES['resel_tmaze_step']
    return h


def test_tmaze_step_rejects_bad_arguments_before_touching_the_device(lib):
    """Nothing here is a device pointer: a call that got past the argument checks would fault, not return."""
    from offpolicy_rnn.hip._lib import TMazeCfg
    fake = 0x1000
    ptrs = ('action', 'goals', 'n_episodes', 'env_state', 'ret_acc', 'ep_ret', 'ep_len', 'in_block', 'flags')

    def call(B=3, A=4, J=2, ld_action=6, ld_goals=2, ld_ep=2, ld_in=9, L=3, o=0, T=4, penalty=-1.0 / 3, init=0, **p):
        q = {k: p.get(k, fake) for k in ptrs}
        cfg = TMazeCfg(L, o, T, 1.0, penalty, 0.0)
        return lib.resel_tmaze_step(cfg, init, q['action'], ld_action, q['goals'], ld_goals, q['n_episodes'], J, q['env_state'], q['ret_acc'],
                                    q['ep_ret'], q['ep_len'], ld_ep, q['in_block'], ld_in, A, q['flags'], B, None)

    for name in ptrs:
        assert call(**{name: None}) == RESEL_EINVAL, name
        assert call(init=1, **{name: None}) == RESEL_EINVAL, name
    assert call(A=3) == RESEL_EINVAL and call(A=5, ld_in=16) == RESEL_EINVAL
    assert call(B=-1) == RESEL_EINVAL
    assert call(ld_in=8) == RESEL_EINVAL                           # below 2 * 2 + A + 1
    assert call(ld_action=0) == RESEL_EINVAL
    assert call(J=0) == RESEL_EINVAL and call(ld_goals=1) == RESEL_EINVAL and call(ld_ep=1) == RESEL_EINVAL
    assert call(L=0) == RESEL_EINVAL and call(T=0) == RESEL_EINVAL and call(o=-1) == RESEL_EINVAL
    assert call(penalty=0.25) == RESEL_EINVAL
    assert call(B=0) == 0 and call(B=0, init=1, penalty=0.0) == 0     # nothing to do: nothing launched


def test_cfg_struct_matches_the_header_layout():
    from offpolicy_rnn.hip._lib import TMAZE_STATE_WORDS, TMazeCfg
    assert ctypes.sizeof(TMazeCfg) == 40 and TMazeCfg.goal_reward.offset == 16 and TMazeCfg.distract_reward.offset == 32
    assert TMAZE_STATE_WORDS == 8
