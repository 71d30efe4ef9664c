"""T-Maze on the GPU: the environment-step kernel (`ops.tmaze_step`, csrc/env_step.hip) against a host replica built on the host
environment (env_utils/tmaze.py) - every buffer after every step, floats through their bits -, its capture into a graph, the
evaluator with the environment step inside the policy-step graph against the host loop (`RESEL_DEVICE_ENV=0`), and `train()`.
Everything is integer logic plus a handful of doubles: every comparison is exact."""
import random

import numpy as np
import pytest
import torch

from offpolicy_rnn.env_utils.tmaze import TMaze

pytestmark = pytest.mark.gpu
J = 3
WIDTH = 9                                                       # state[2] | lst_state[2] | lst_action[4] | reward[1]
LD_IN, LD_ACTION = 12, 7                                        # wider than the rows: the gaps must stay as they were
GAP = 7.5
LAYERS = ['gru', 'smamba_s8_c4_b2_nln', 'cgpt_h1_l2_p0_ml32']
TRAIN_SHORT = dict(total_iteration=1, step_per_iteration=20, random_num=30, start_train_num=24, update_interval=5, sac_batch_size=24)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def _clamp(a):
    return 3 if a >= 3 else (int(a) if a >= 0 else 0)           # NaN fails both comparisons: 0


class Replica:
    """What the kernel is specified to do (include/resel_hip.h `resel_tmaze_step`), on numpy buffers, with one host TMaze per row."""

    def __init__(self, B, active, L, goals, n_episodes):
        self.B, self.goals, self.n = B, goals, np.clip(n_episodes, 0, J)
        self.envs = [TMaze(L, oracle_length=active, penalty=-1.0 / L) for _ in range(B)]
        self.cfg = self.envs[0].device_config()
        self.in_block = np.full((B, LD_IN), GAP, dtype=np.float32)
        self.flags = np.full(B, -3, dtype=np.int32)
        self.state = np.full((B, 8), -9, dtype=np.int32)
        self.ret_acc = np.full(B, 0.125)
        self.ep_ret, self.ep_len = np.full((B, J), -77.0), np.full((B, J), -77, dtype=np.int32)

    def buffers(self):
        return dict(in_block=self.in_block, flags=self.flags, env_state=self.state, ret_acc=self.ret_acc, ep_ret=self.ep_ret, ep_len=self.ep_len)

    def _sync(self, b):
        e = self.envs[b]
        self.state[b, :5] = (e.x, e.y, e.goal_y, int(e.oracle_visited), e.time_step)

    def _begin(self, b, j):
        self.in_block[b, 2:WIDTH] = 0.0
        self.flags[b], self.ret_acc[b], self.state[b, 5] = 1, 0.0, 0
        if j < self.n[b]:
            self.in_block[b, :2] = self.envs[b].reset(goal=int(self.goals[b, j]))
            self._sync(b)
            self.state[b, 6], self.state[b, 7] = j + 1, 1
        else:
            self.state[b, 7] = 0
            self.in_block[b, :2] = 0.0

    def init(self):
        self.state[:] = 0
        for b in range(self.B):
            self._begin(b, 0)

    def step(self, action):
        for b in range(self.B):
            if not self.state[b, 7]:
                self.in_block[b, :WIDTH], self.flags[b] = 0.0, 1
                continue
            a = _clamp(action[b])
            obs, r, done, _ = self.envs[b].step(a)
            self._sync(b)
            row = self.in_block[b]
            row[2:4] = row[0:2]
            row[0:2] = obs
            row[4:8] = np.eye(4, dtype=np.float32)[a]
            row[8] = np.float32(r)
            self.ret_acc[b] += r
            self.state[b, 5] += 1
            self.flags[b] = 0
            if done:
                j = self.state[b, 6] - 1
                self.ep_ret[b, j], self.ep_len[b, j] = self.ret_acc[b], self.state[b, 5]
                self._begin(b, j + 1)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _case(B, seed):
    rs = np.random.RandomState(seed)
    goals = rs.choice([-1, 1], size=(B, J)).astype(np.int32)
    n = rs.randint(0, J + 1, size=B).astype(np.int32)
    n[0] = J                                                    # row 0 runs throughout: it is the one fed NaN / -1 / 7
    if B >= 5:
        n[1], n[2] = 0, 1                                       # idle from the start, idle after one episode
    return rs, goals, n


def _device(rep, goals, n):
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in rep.buffers().items()}
    dev['goals'], dev['n_episodes'] = torch.from_numpy(goals).cuda(), torch.from_numpy(n).cuda()
    return dev


def _call(ops, cfg, init, action_block, d):
    ops.tmaze_step(cfg, init, action_block[:, 0], d['goals'], d['n_episodes'], d['env_state'], d['ret_acc'], d['ep_ret'], d['ep_len'],
                   d['in_block'][:, :WIDTH], d['flags'])


def _assert_equal(rep, d, what):
    for k, want in rep.buffers().items():
        got = d[k].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (what, k, got, want)


# ------------------------------------------------------------------------------------------------ 1. kernel against the host environment
@pytest.mark.parametrize('L', [1, 3])
@pytest.mark.parametrize('active', [0, 1])
@pytest.mark.parametrize('B', [1, 5, 64, 70])
def test_kernel_equals_the_host_environment(ops, B, active, L):
    rs, goals, n = _case(B, 100 * B + 10 * active + L)
    rep = Replica(B, active, L, goals, n)
    d = _device(rep, goals, n)
    T = rep.cfg['episode_length']
    assert T == L + 1 + 2 * active
    _call(ops, rep.cfg, True, torch.full((B, LD_ACTION), float('nan'), device='cuda'), d)       # init reads no action
    rep.init()
    _assert_equal(rep, d, 'init')
    steps = J * T + 2                                           # two more than the longest row needs: every row idle at the end
    finished = 0
    for s in range(steps):
        block = np.full((B, LD_ACTION), GAP, dtype=np.float32)
        block[:, 0] = rs.randint(0, 4, size=B)
        if s < 3:
            block[0, 0] = (np.nan, -1.0, 7.0)[s]
        dev_block = torch.from_numpy(block).cuda()
        _call(ops, rep.cfg, False, dev_block, d)
        rep.step(block[:, 0])
        _assert_equal(rep, d, f'step {s}')
        assert np.array_equal(_bits(dev_block.cpu().numpy()), _bits(block))                    # the action block is read only
        finished = int((rep.ep_len > 0).sum())
    assert finished == int(n.sum()) and not rep.state[:, 7].any() and (rep.flags == 1).all()
    assert (rep.ep_len[rep.ep_len > 0] == T).all() and (rep.in_block[:, WIDTH:] == GAP).all()
    if B >= 5:
        assert (rep.ep_len[1] == -77).all() and (rep.ep_len[2, 1:] == -77).all()               # slots nobody ran stay untouched


def test_clamped_indices_move_as_0_0_3(ops):
    """Passive L = 3 from the start (0, 0): NaN -> 0 (right), -1 -> 0 (right), 7 -> 3 (down: off the map)."""
    goals, n = np.ones((1, J), dtype=np.int32), np.full(1, 1, dtype=np.int32)
    rep = Replica(1, 0, 3, goals, n)
    d = _device(rep, goals, n)
    block = torch.zeros((1, LD_ACTION), device='cuda')
    _call(ops, rep.cfg, True, block, d)
    seen = []
    for a in (float('nan'), -1.0, 7.0):
        block[0, 0] = a
        _call(ops, rep.cfg, False, block, d)
        seen.append((d['env_state'][0, :2].tolist(), d['in_block'][0, 4:8].tolist()))
    assert seen == [([1, 0], [1.0, 0, 0, 0]), ([2, 0], [1.0, 0, 0, 0]), ([2, 0], [0, 0, 0, 1.0])]


# ------------------------------------------------------------------------------------------------ 2. capturability
def test_init_and_steps_capture_into_a_graph(ops):
    B, active, L, nsteps = 70, 1, 1, 6
    rs, goals, n = _case(B, 5)
    rep = Replica(B, active, L, goals, n)
    actions = torch.from_numpy(rs.randint(0, 4, size=(nsteps, B, LD_ACTION)).astype(np.float32)).cuda()

    def sequence(d):
        _call(ops, rep.cfg, True, actions[0], d)
        for s in range(nsteps):
            _call(ops, rep.cfg, False, actions[s], d)

    eager, graphed = _device(rep, goals, n), _device(rep, goals, n)
    sequence(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sequence(graphed)
    for k in rep.buffers():                                     # capture ran nothing; poison what a replay must rewrite
        graphed[k].copy_(torch.from_numpy(rep.buffers()[k]).cuda())
    g.replay()
    torch.cuda.synchronize()
    rep.init()
    for s in range(nsteps):
        rep.step(actions[s, :, 0].cpu().numpy())
    _assert_equal(rep, eager, 'eager')
    _assert_equal(rep, graphed, 'replay')
    g.replay()                                                  # the init call makes the sequence restartable
    torch.cuda.synchronize()
    _assert_equal(rep, graphed, 'second replay')


# ------------------------------------------------------------------------------------------------ 3. the evaluator
def _alg(rnn, env):
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    alg = alg_init(make_parameter(rnn, env=env, cuda_inference=True))
    assert alg.discrete_env and alg.act_dim == 4 and alg.obs_dim == 2 and alg.policy.categorical
    return alg


def _flat(store):
    if hasattr(store, 'flat_views'):
        return torch.cat([v.detach().reshape(-1) for _, v in sorted(store.flat_views().items())]).clone()
    return store.flat.detach().clone()


def _generators(dev):
    return (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state().clone(), torch.cuda.get_rng_state(dev).clone())


def _same_generators(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


@pytest.mark.parametrize('env', ['Mem-T-passive-3-v0', 'Mem-T-active-2-v0'])
@pytest.mark.parametrize('rnn', LAYERS)
def test_device_evaluation_equals_the_host_loop(ops, rnn, env, monkeypatch):
    from offpolicy_rnn.env_utils.make_env import make_env
    from offpolicy_rnn.utility.policy_eval import BatchedPolicyEval
    alg = _alg(rnn, env)
    dev, T = alg.sample_device, make_env(env, 0)['max_trajectory_len']
    factory = lambda: make_env(env, 0)['eval_env']
    results = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('RESEL_DEVICE_ENV', mode)
        ev = BatchedPolicyEval(alg.policy, factory, 4, 4, dev, seed=3, discrete=True)
        runs = []
        for n, training in ((7, True), (3, False), (8, True)):  # two waves with an idle row in the last; one wave with an idle row; full waves
            alg.policy.train(training)
            before, gens = _flat(alg.policy.store), _generators(dev)
            out = ev.evaluate(n)
            assert torch.equal(_flat(alg.policy.store), before)
            assert _same_generators(_generators(dev), gens)
            mods = alg.policy.contextual_modules
            assert all(m.training is training for m in mods.values())
            assert list(out) == ['EpRetTest', 'EpLenTest'] and out['EpLenTest'] == [T] * n
            assert all(type(v) is float for v in out['EpRetTest']) and all(type(v) is int for v in out['EpLenTest'])
            assert (ev.device_env is not None) == (mode == '1') and (ev.step is None) == (mode == '1')
            step = ev.device_env.step if mode == '1' else ev.step
            runs.append((out['EpRetTest'], out['EpLenTest'], list(ev.last_rows), step._row_pos.tolist(),     # and the cgpt positions:
                         [ip.seqlen_offset for ip in step._counters()], [ip.device_offset.tolist() for ip in step._counters()]))
        results[mode] = runs
    assert results['1'] == results['0']
    assert results['1'][0][2] == [0, 1, 2, 3, 0, 1, 2] and results['1'][1][2] == [0, 1, 2]
    assert results['1'][0][3] == [T, T, T, 1] and results['1'][1][3] == [T, T, T, 1] and results['1'][2][3] == [T] * 4
    if rnn.startswith('cgpt'):
        first = results['1'][0]                                 # one KV cache per attention layer
        assert first[4] and all(v == T for v in first[4]) and all(off == [T, T, T, 1] for off in first[5])


def test_fallbacks_take_the_host_loop(ops, monkeypatch):
    """A continuous-action T-Maze and any other environment never reach the in-graph step, whatever the switch says."""
    from offpolicy_rnn.env_utils.make_env import make_env
    from offpolicy_rnn.utility.policy_eval import BatchedPolicyEval
    monkeypatch.setenv('RESEL_DEVICE_ENV', '1')
    alg = _alg('gru', 'Mem-T-passive-3-v0')
    ev = BatchedPolicyEval(alg.policy, lambda: make_env('synthetic-o2-d4-T4', 0)['eval_env'], 4, 2, alg.sample_device, seed=3, discrete=True)
    assert ev.evaluate(3)['EpLenTest'] == [4] * 3 and ev.device_env is None and ev.step is not None
    from offpolicy_rnn.env_utils.tmaze import device_steppable
    assert not device_steppable(make_env('Mem-T-passive-3-cont-act-v0', 0)['eval_env'])


def test_cgpt_cache_shorter_than_an_episode_raises_before_any_replay(ops, monkeypatch):
    from offpolicy_rnn.env_utils.make_env import make_env
    from offpolicy_rnn.hip.graph_step import GraphedPolicyStep
    from offpolicy_rnn.utility.policy_eval import BatchedPolicyEval
    env = 'Mem-T-passive-10-v0'                                 # 11 steps into a cache of 8
    alg = _alg('cgpt_h1_l2_p0_ml8', env)
    replays = []
    monkeypatch.setattr(GraphedPolicyStep, 'replay_device', lambda self: replays.append(1))
    monkeypatch.setenv('RESEL_DEVICE_ENV', '1')
    ev = BatchedPolicyEval(alg.policy, lambda: make_env(env, 0)['eval_env'], 4, 4, alg.sample_device, seed=3, discrete=True)
    with pytest.raises(RuntimeError, match='KV cache is full'):
        ev.evaluate(7)
    assert ev.device_env is not None and not replays


# ------------------------------------------------------------------------------------------------ 4. train()
def test_train_logs_tmaze_evaluations(ops, tmp_path, monkeypatch):
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('RESEL_DEVICE_ENV', raising=False)
    alg = alg_init(make_parameter('gru', env='Mem-T-passive-3-v0', cuda_inference=True, test_nprocess=5, test_nrollout=1, **TRAIN_SHORT))
    logged, add = [], alg.logger.add_tabular_data

    def record(tb_prefix=None, **kw):
        logged.append((tb_prefix, {k: v for k, v in kw.items() if k.endswith('Test')}))
        return add(tb_prefix=tb_prefix, **kw)

    monkeypatch.setattr(alg.logger, 'add_tabular_data', record)
    alg.train()
    perf = [kw for prefix, kw in logged if prefix == 'performance']
    assert len(perf) == 1 and perf[0]['EpLenTest'] == [4] * 5 and len(perf[0]['EpRetTest']) == 5
    assert all(-1.0 <= v <= 1.0 for v in perf[0]['EpRetTest'])
    from offpolicy_rnn.utility.policy_eval import device_env_enabled
    assert alg.evaluator.rows == 5 and (alg.evaluator.device_env is not None) == device_env_enabled()
    assert alg.grad_num >= 1
