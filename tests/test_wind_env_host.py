"""Wind-v0 without a GPU: the host environment (env_utils/wind.py) against what the reference's `WindEnv` behind `VariBadWrapper`
recorded (tests/golden/wind_v0.npz, generate_wind_golden.py) - every array, exactly -, `make_env('Wind-v0', seed)`, the trainer's task
draw in `env_reset`, the evaluation scheduler over host environments, and the argument checks of the two kernel entries that return
before the device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from offpolicy_rnn.env_utils.make_env import Box, make_env
from offpolicy_rnn.env_utils.wind import Wind, device_steppable
from offpolicy_rnn.utility.policy_eval import BatchedPolicyEval, run_episodes
from offpolicy_rnn.utility.sample_utility import unorm_act

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESEL_EINVAL = -1
SEEDS, SCRIPTS = (1, 3), ('noise', 'seek')


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ against the reference's record
def test_fixture_covers_what_it_should():
    g = load_golden('wind_v0.npz')
    for s in SEEDS:
        assert g[f's{s}_winds'].shape == (60, 2) and g[f's{s}_train_tasks'].shape == (40,) and g[f's{s}_eval_tasks'].shape == (20,)
        assert len(g[f's{s}_tasks']) >= 3
        noise, seek = g[f's{s}_noise_actions'], g[f's{s}_seek_actions']
        assert noise.shape == seek.shape == (len(g[f's{s}_tasks']), 75, 2)
        assert (np.abs(noise) > 1).any() and (np.abs(noise) < 1).any()                       # the outer clip acts, and does not
        assert _same(seek, seek.astype(np.float32).astype(np.float64))                       # a float32 script
        assert (g[f's{s}_seek_reward'].sum(axis=1) >= 30).all() and not g[f's{s}_noise_reward'].any()
        for script in SCRIPTS:
            assert g[f's{s}_{script}_obs'].dtype == np.float64 and g[f's{s}_{script}_reward'].dtype == np.float64
            assert g[f's{s}_{script}_done'].dtype == bool


@pytest.mark.parametrize('seed', SEEDS)
def test_host_env_equals_the_reference_record(seed):
    g = load_golden('wind_v0.npz')
    info = make_env('Wind-v0', seed)
    env = info['train_env']
    assert _same(np.array(env.winds, dtype=np.float64), g[f's{seed}_winds'])
    assert _same(np.asarray(info['train_tasks'], dtype=np.int64), g[f's{seed}_train_tasks'])
    assert _same(np.asarray(info['eval_tasks'], dtype=np.int64), g[f's{seed}_eval_tasks'])
    for script in SCRIPTS:
        for i, task in enumerate(g[f's{seed}_tasks'].tolist()):
            actions = g[f's{seed}_{script}_actions'][i]
            if script == 'seek':
                actions = actions.astype(np.float32)             # as the script fed them: the rescaling then runs in float32
            obs, rewards, dones = [env.reset(task)], [], []
            assert _same(env.get_current_task(), g[f's{seed}_winds'][task])
            for a in actions:
                ob, r, d, inf = env.step(a)
                assert type(r) is float and inf == {'done_mdp': d} and r == env.last_reward()
                obs.append(ob)
                rewards.append(r)
                dones.append(d)
            assert _same(np.array(obs), g[f's{seed}_{script}_obs'][i]), (script, task)
            assert _same(np.array(rewards), g[f's{seed}_{script}_reward'][i]), (script, task)
            assert _same(np.array(dones), g[f's{seed}_{script}_done'][i]), (script, task)


def test_reset_none_keeps_the_wind_and_short_episodes():
    env = Wind(n_tasks=5, max_episode_steps=3, seed=0)
    assert env.meta_env_flag and env.n_tasks == 5 and env.horizon_bamdp == env._max_episode_steps == 3
    assert list(env.get_all_task_idx()) == [0, 1, 2, 3, 4] and device_steppable(env)
    env.reset(4)
    wind = env.get_current_task()
    assert _same(wind, np.array(env.winds[4]))
    env.step(np.zeros(2))
    assert _same(env.reset(), np.zeros(2)) and _same(env.get_current_task(), wind)           # `reset_task(None)` of the reference
    dones = [env.step(np.zeros(2))[2] for _ in range(3)]
    assert dones == [False, False, True]
    assert _same(env._state, (wind + wind) + wind)                # a zero action is exactly the middle of the inner bounds: +0.0
    env.seed(9)
    assert _same(np.array(Wind(n_tasks=5, seed=7).winds), np.array(env.winds))               # the winds do not depend on the seed


def test_outward_box_is_float64_and_keeps_a_small_action():
    env = make_env('Wind-v0', 0)['train_env']
    space = env.action_space
    assert space.low.dtype == space.high.dtype == np.float64 and space.shape == (2,) and (space.low == -1).all() and (space.high == 1).all()
    assert Box(-1.0, 1.0, (2,)).low.dtype == np.float32          # the default stays: every other environment is unchanged
    a = np.array([0.3, -1e-8], dtype=np.float32)                 # what the graphed step returns: the outward box decides the width of the
    wide, narrow = unorm_act(a, space), unorm_act(a, Box(-1.0, 1.0, (2,)))                   # action the environment rescales
    assert wide.dtype == np.float64 and narrow.dtype == np.float32
    assert _same(wide, ((a + np.float32(1)) / np.float32(2)).astype(np.float64) * 2.0 - 1.0)  # (a + 1) / 2 in float32, the rest in double
    one, other = Wind(n_tasks=2), Wind(n_tasks=2)
    assert not _same(one.step(wide)[0], other.step(narrow)[0])   # a float32 action is rescaled in float32: another position
    cfg = env.device_config()
    assert cfg['act_low'] == float(np.float32(-0.1)) and cfg['act_high'] == float(np.float32(0.1)) and cfg['act_span'] == float(np.float32(0.2))
    assert cfg['out_low'] == -1.0 and cfg['out_span'] == 2.0 and cfg['episode_length'] == 75 and cfg['goal_radius'] == 0.03


# ------------------------------------------------------------------------------------------------ make_env
@pytest.mark.parametrize('seed', [0, 1, 3])
def test_make_env_fields_and_global_stream(seed):
    np.random.seed(77)
    before = np.random.get_state()
    info = make_env('Wind-v0', seed)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    perm = np.random.RandomState(seed).permutation(60)
    assert list(info['train_tasks']) == list(perm[:40]) and list(info['eval_tasks']) == list(perm[-20:])
    assert info['max_rollouts_per_task'] == 1 and info['max_trajectory_len'] == 75 and info['obs_dim'] == info['act_dim'] == 2
    assert info['act_continuous'] is True and info['seed'] == seed and info['multiagent'] is False
    env, eval_env = info['train_env'], info['eval_env']
    assert isinstance(env, Wind) and isinstance(eval_env, Wind) and env is not eval_env and env.n_tasks == 60
    assert env.observation_space.shape == (2,) and env._max_episode_steps == 75


@pytest.mark.parametrize('name', ['PointRobotSparse-v0', 'AntDir-v0', 'Wind-v1'])
def test_other_meta_names_still_fail_loudly(name):
    with pytest.raises(ImportError):
        make_env(name, 0)


# ------------------------------------------------------------------------------------------------ the trainer's task draw
def test_env_reset_draws_one_training_task(oracle_ops, tmp_path, monkeypatch):
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    alg = alg_init(make_parameter('gru', env='Wind-v0', seed=3))
    assert not alg.discrete_env and alg.obs_dim == 2 and alg.act_dim == 2 and isinstance(alg.env, Wind) and alg.max_episode_steps == 75
    train = list(alg.env_info['train_tasks'])
    for s in (5, 6, 7):
        np.random.seed(s)
        want = train[np.random.randint(0, len(train))]
        after_one = np.random.get_state()[1].copy(), np.random.get_state()[2]
        np.random.seed(s)
        alg.env_reset()
        got = np.random.get_state()
        assert np.array_equal(got[1], after_one[0]) and got[2] == after_one[1]               # exactly one draw
        assert _same(alg.env.get_current_task(), np.array(alg.env.winds[want])) and _same(alg.state_np, np.zeros((1, 2)))
    maze = alg_init(make_parameter('gru', env='Mem-T-passive-3-v0', seed=3))
    np.random.seed(5)
    before = np.random.get_state()
    maze.env_reset()
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2] == after[2]                     # no draw from the global stream


def test_train_runs_on_wind(oracle_ops, tmp_path, monkeypatch):
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    alg = alg_init(make_parameter('gru', env='Wind-v0', total_iteration=1, step_per_iteration=80, random_num=75, start_train_num=150,
                                  update_interval=50, sac_batch_size=150))
    alg.train()
    assert alg.sample_num == 75 + 80 and alg.grad_num == 1 and len(alg.replay_buffer) == 2   # 75-step episodes
    assert alg.env.step_count == 5 and alg.state_np.dtype == np.float64 and alg.last_action_np.shape == (1, 2)


# ------------------------------------------------------------------------------------------------ the scheduler over host environments
def test_run_episodes_with_a_scripted_step_reaches_the_goal():
    rows, n = 3, 7
    info = make_env('Wind-v0', 2)
    ev = BatchedPolicyEval(None, lambda: make_env('Wind-v0', 2)['eval_env'], 2, rows, 'cpu', seed=4, eval_tasks=info['eval_tasks'],
                           step=lambda *a, **k: None)
    ev._make()
    assert ev.device_env is None and not ev._on_device()

    def step(state, lst_state, lst_action, reward, reset):
        """Goal seeking on what the policy sees plus the hidden wind (a scripted oracle): float32 means, as the graphed step returns them."""
        wind = np.array([e.get_current_task() for e in ev.envs])
        return np.clip((np.array([0.0, 1.0]) - state - wind) / 0.1, -1, 1).astype(np.float32)

    rs = np.random.RandomState(4)
    for _ in range(rows):
        rs.randint(0, 10000000)                                  # the environments' seeds come first
    tasks = [info['eval_tasks'][rs.randint(0, 20)] for _ in range(n)]
    out, ep_rows = run_episodes(step, ev.envs, n, 2, 2, ev._reset_env)
    assert list(out) == ['EpRetTest', 'EpLenTest', 'done_mdpTest']
    assert out['EpLenTest'] == [75] * n and out['done_mdpTest'] == [1.0] * n and ep_rows == [k % rows for k in range(n)]
    assert all(30.0 <= r <= 70.0 and r == int(r) for r in out['EpRetTest'])
    after = ev.rs.get_state()
    assert np.array_equal(after[1], rs.get_state()[1]) and after[2] == rs.get_state()[2]     # exactly n draws, one per episode
    for r in range(rows):                                        # the last episode of each row ran on the task drawn for it
        k = max(k for k in range(n) if k % rows == r)
        assert _same(ev.envs[r].get_current_task(), np.array(ev.envs[r].winds[tasks[k]]))


# ------------------------------------------------------------------------------------------------ the per-environment record
def test_records_of_the_two_device_environments():
    from offpolicy_rnn.env_utils.device_env import KINDS, TMazeKind, WindKind, device_env_kind
    assert device_env_kind(make_env('Wind-v0', 0)['train_env']) is WindKind
    assert device_env_kind(make_env('Mem-T-passive-3-v0', 0)['train_env']) is TMazeKind
    assert device_env_kind(make_env('Mem-T-passive-3-cont-act-v0', 0)['train_env']) is None
    assert device_env_kind(make_env('synthetic-o2-a2-T75', 0)['train_env']) is None
    for kind in KINDS:
        assert kind.state_bytes % 8 == 0 and kind.obs_dim == 2
    assert (WindKind.act_dim, WindKind.categorical) == (2, False) and (TMazeKind.act_dim, TMazeKind.categorical) == (4, True)
    assert WindKind.eval_extras(2) == {'done_mdpTest': [1.0, 1.0]} and TMazeKind.eval_extras(2) == {}


# ------------------------------------------------------------------------------------------------ argument checks of the kernel entries
@pytest.fixture(scope='module')
def lib():
    from offpolicy_rnn.hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('resel_wind_step', 'resel_wind_collect_step'):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


def _cfg(**over):
    from offpolicy_rnn.hip._lib import WIND_CFG_DOUBLES, WindCfg
    cfg = dict(Wind(n_tasks=2, max_episode_steps=4).device_config(), **over)
    return WindCfg(int(cfg['episode_length']), *[float(cfg[k]) for k in WIND_CFG_DOUBLES])


def test_wind_step_rejects_bad_arguments_before_touching_the_device(lib):
    """Nothing here is a device pointer: a call that got past the argument checks would fault, not return."""
    fake = 0x1000
    ptrs = ('action', 'winds', 'n_episodes', 'env_pos', 'env_words', 'ret_acc', 'ep_ret', 'ep_len', 'in_block', 'flags')

    def call(B=3, A=2, J=2, ld_action=5, ld_winds=4, ld_ep=2, ld_in=7, init=0, cfg=None, **p):
        q = {k: p.get(k, fake) for k in ptrs}
        return lib.resel_wind_step(cfg or _cfg(), init, q['action'], ld_action, q['winds'], ld_winds, q['n_episodes'], J, q['env_pos'],
                                   q['env_words'], q['ret_acc'], q['ep_ret'], q['ep_len'], ld_ep, q['in_block'], ld_in, A, q['flags'], B, None)

    for name in ptrs:
        assert call(**{name: None}) == RESEL_EINVAL, name
        assert call(init=1, **{name: None}) == RESEL_EINVAL, name
    assert call(A=1) == RESEL_EINVAL and call(A=4, ld_in=16) == RESEL_EINVAL and call(B=-1) == RESEL_EINVAL
    assert call(ld_in=6) == RESEL_EINVAL and call(ld_action=1) == RESEL_EINVAL
    assert call(J=0) == RESEL_EINVAL and call(ld_winds=3) == RESEL_EINVAL and call(ld_ep=1) == RESEL_EINVAL
    for bad in (dict(episode_length=0), dict(goal_radius=-1.0), dict(goal_radius=float('nan')), dict(act_low=0.2), dict(out_span=float('nan'))):
        assert call(cfg=_cfg(**bad)) == RESEL_EINVAL, bad
    assert call(B=0) == 0 and call(B=0, init=1) == 0             # nothing to do: nothing launched


def test_wind_collect_step_rejects_bad_arguments_before_touching_the_device(lib):
    from offpolicy_rnn.hip._lib import COLLECT_FIELDS, CollectLayout
    fake = 0x1000
    ptrs = ('action', 'wind', 'env_pos', 'env_words', 'ret_acc', 'traj', 'in_block')
    widths = dict(state=2, last_state=2, last_action=2, action=2, next_state=2, logp=0)

    def layout(**over):
        lay, off = CollectLayout(), 0
        for name in COLLECT_FIELDS:
            w = widths.get(name, 1)
            setattr(lay, name, off if w else -1)
            off += w
        for k, v in over.items():
            setattr(lay, k, v)
        return lay, off

    assert layout()[1] == 16 and layout()[0].timeout == 15 and layout()[0].logp == -1

    def call(B=2, A=2, ld_action=5, T_cap=4, ld_row=16, steps=4, ld_in=7, init=0, cfg=None, lay=None, **p):
        q = {k: p.get(k, fake) for k in ptrs}
        return lib.resel_wind_collect_step(cfg or _cfg(), lay or layout()[0], init, q['action'], ld_action, q['wind'], q['env_pos'],
                                           q['env_words'], q['ret_acc'], q['traj'], T_cap, ld_row, steps, q['in_block'], ld_in, A, B, None)

    for name in ptrs:
        assert call(**{name: None}) == RESEL_EINVAL, name
    assert call(A=4) == RESEL_EINVAL and call(B=-1) == RESEL_EINVAL and call(T_cap=0) == RESEL_EINVAL and call(steps=0) == RESEL_EINVAL
    assert call(ld_in=6) == RESEL_EINVAL and call(ld_action=1) == RESEL_EINVAL and call(ld_row=15) == RESEL_EINVAL
    assert call(lay=layout(logp=3)[0]) == RESEL_EINVAL
    assert call(lay=layout(action=15)[0]) == RESEL_EINVAL        # the action field is two columns wide here: 15 + 2 > 16
    assert call(cfg=_cfg(episode_length=0)) == RESEL_EINVAL
    assert call(B=0) == 0 and call(B=0, lay=layout(timeout=-1)[0], ld_row=15) == 0           # an absent field needs no column


def test_cfg_struct_and_prototypes_match_the_header():
    from offpolicy_rnn.hip import _lib
    assert ctypes.sizeof(_lib.WindCfg) == 72 and _lib.WindCfg.goal_x.offset == 8 and _lib.WindCfg.out_span.offset == 64
    header = open(os.path.join(ROOT, 'include', 'resel_hip.h')).read()
    assert int(re.search(r'#define\s+RESEL_WIND_STATE_DOUBLES\s+(\d+)', header).group(1)) == _lib.WIND_STATE_DOUBLES == 6
    assert int(re.search(r'#define\s+RESEL_WIND_STATE_WORDS\s+(\d+)', header).group(1)) == _lib.WIND_STATE_WORDS == 4
    fields = re.search(r'typedef struct \{ int32_t episode_length; double ([^;]*); \} resel_wind_cfg_t;', header).group(1)
    assert tuple(f.strip() for f in fields.split(',')) == _lib.WIND_CFG_DOUBLES
    from test_host_logic import test_ctypes_signatures_match_the_header_prototypes
    assert 'resel_wind_step' in _lib.SIGNATURES and 'resel_wind_collect_step' in _lib.SIGNATURES
    test_ctypes_signatures_match_the_header_prototypes()         # the generic check covers the two new prototypes
