"""Wind-v0 on the GPU: the two environment kernels (`ops.wind_step`, `ops.wind_collect_step`, csrc/env_step.hip) against replicas built on
the host environment (env_utils/wind.py) and the trainer's own `_push` / `env_step` - every buffer after every step, floats through their
bits -, their capture into a graph, the evaluator and `train()` with the environment inside the policy step's graph against the host
loops (`RESEL_DEVICE_ENV=0`, `RESEL_DEVICE_COLLECT=0`), and the refusals.  Both sides execute the same correctly rounded operations in
the same order, so every comparison is exact: there is no tolerance anywhere in this file."""
import ctypes
import random
import types

import numpy as np
import pytest
import torch

from offpolicy_rnn.algorithm.sac import SAC
from offpolicy_rnn.buffers.transition_buffer.replay_memory import MemoryArray, Transition
from offpolicy_rnn.env_utils.wind import Wind
from offpolicy_rnn.utility.sample_utility import unorm_act

pytestmark = pytest.mark.gpu
J = 3
WIDTH = 7                                                       # state[2] | lst_state[2] | lst_action[2] | reward[1]
LD_IN, LD_ACTION = 10, 7                                        # wider than the rows: the gaps must stay as they were
GAP = 7.5
NAN, INF = float('nan'), float('inf')
# the first steps of row 0: signed zeros, values the fp32 `a + 1` rounds away, the clip's edges and beyond, infinities
SPECIAL = [(0.0, -0.0), (1e-8, -1e-8), (1.5, -2.0), (1.0, -1.0), (INF, -INF), (-1.0 + 2.0 ** -24, 1.0 - 2.0 ** -25)]


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _host_step(env, a):
    """The environment step of both host loops on the fp32 action the graphed step returns."""
    return env.step(unorm_act(np.asarray(a, dtype=np.float32), env.action_space))


class Replica:
    """What the evaluation kernel is specified to do (include/resel_hip.h `resel_wind_step`), on numpy buffers, one host `Wind` per row."""

    def __init__(self, B, T, winds, n_episodes):
        self.B, self.winds, self.n = B, winds, np.clip(n_episodes, 0, J)
        self.envs = [Wind(n_tasks=2, max_episode_steps=T) for _ in range(B)]
        self.cfg = self.envs[0].device_config()
        self.in_block = np.full((B, LD_IN), GAP, dtype=np.float32)
        self.flags = np.full(B, -3, dtype=np.int32)
        self.pos, self.words = np.full((B, 6), -9.5), np.full((B, 4), -9, dtype=np.int32)
        self.ret_acc = np.full(B, 0.125)
        self.ep_ret, self.ep_len = np.full((B, J), -77.0), np.full((B, J), -77, dtype=np.int32)

    def buffers(self):
        return dict(in_block=self.in_block, flags=self.flags, env_pos=self.pos, env_words=self.words, ret_acc=self.ret_acc, ep_ret=self.ep_ret,
                    ep_len=self.ep_len)

    def _begin(self, b, j):
        self.in_block[b, :WIDTH] = 0.0
        self.flags[b], self.ret_acc[b], self.words[b, 1] = 1, 0.0, 0
        if j < self.n[b]:
            env = self.envs[b]
            env.set_wind(self.winds[b, j])
            assert not env.reset().any()
            self.pos[b] = (0.0, 0.0, self.winds[b, j, 0], self.winds[b, j, 1], 0.0, 0.0)
            self.words[b, 0], self.words[b, 2], self.words[b, 3] = 0, j + 1, 1
        else:
            self.words[b, 3] = 0

    def init(self):
        self.pos[:], self.words[:] = 0.0, 0
        for b in range(self.B):
            self._begin(b, 0)

    def step(self, action):
        for b in range(self.B):
            if not self.words[b, 3]:
                self.in_block[b, :WIDTH], self.flags[b] = 0.0, 1
                continue
            env, row = self.envs[b], self.in_block[b]
            self.pos[b, 4:6] = self.pos[b, 0:2]
            obs, r, done, _ = _host_step(env, action[b])
            self.pos[b, 0:2], self.words[b, 0] = obs, env.step_count
            row[2:4] = row[0:2]
            row[0:2] = obs.astype(np.float32)
            row[4:6] = action[b]
            row[6] = np.float32(r)
            self.ret_acc[b] += r
            self.words[b, 1] += 1
            self.flags[b] = 0
            if done:
                j = self.words[b, 2] - 1
                self.ep_ret[b, j], self.ep_len[b, j] = self.ret_acc[b], self.words[b, 1]
                self._begin(b, j + 1)


def _case(B, seed):
    rs = np.random.RandomState(seed)
    winds = rs.uniform(-0.08, 0.08, size=(B, J, 2))
    n = rs.randint(0, J + 1, size=B).astype(np.int32)
    n[0] = J                                                    # row 0 runs throughout: it is the one fed the special values
    if B >= 5:
        n[1], n[2] = 0, 1                                       # idle from the start, idle after one episode
    return rs, winds, n


def _device(rep, winds, n):
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in rep.buffers().items()}
    dev['winds'], dev['n_episodes'] = torch.from_numpy(winds.copy()).cuda(), torch.from_numpy(n).cuda()
    return dev


def _call(ops, cfg, init, action_block, d):
    ops.wind_step(cfg, init, action_block[:, 1:3], d['winds'], d['n_episodes'], d['env_pos'], d['env_words'], d['ret_acc'], d['ep_ret'],
                  d['ep_len'], d['in_block'][:, :WIDTH], d['flags'])


def _assert_equal(rep, d, what):
    for k, want in rep.buffers().items():
        got = d[k].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (what, k, got, want)


def _seek(rep):
    """clip((goal - state - wind) / 0.1, -1, 1) cast to float32, per row, on the replica's current positions."""
    return np.clip((np.array([0.0, 1.0]) - rep.pos[:, 0:2] - rep.pos[:, 2:4]) / 0.1, -1, 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. evaluation kernel against the twin
@pytest.mark.parametrize('T', [1, 4])
@pytest.mark.parametrize('B', [1, 5, 64, 70])
def test_kernel_equals_the_host_environment(ops, B, T):
    rs, winds, n = _case(B, 100 * B + T)
    rep = Replica(B, T, winds, n)
    d = _device(rep, winds, n)
    _call(ops, rep.cfg, True, torch.full((B, LD_ACTION), NAN, device='cuda'), d)                # init reads no action
    rep.init()
    _assert_equal(rep, d, 'init')
    steps = J * T + 2                                           # two more than the longest row needs: every row idle at the end
    for s in range(steps):
        block = np.full((B, LD_ACTION), GAP, dtype=np.float32)
        block[:, 1:3] = rs.uniform(-1.5, 1.5, size=(B, 2)) if s % 2 == 0 else _seek(rep)        # both scripts, in turn
        if s < len(SPECIAL):
            block[0, 1:3] = SPECIAL[s]
        dev_block = torch.from_numpy(block).cuda()
        _call(ops, rep.cfg, False, dev_block, d)
        rep.step(block[:, 1:3])
        _assert_equal(rep, d, f'step {s}')
        assert np.array_equal(_bits(dev_block.cpu().numpy()), _bits(block))                    # the action block is read only
    assert int((rep.ep_len > 0).sum()) == int(n.sum()) and not rep.words[:, 3].any() and (rep.flags == 1).all()
    assert (rep.ep_len[rep.ep_len > 0] == T).all() and (rep.in_block[:, WIDTH:] == GAP).all()
    if B >= 5:
        assert (rep.ep_len[1] == -77).all() and (rep.ep_len[2, 1:] == -77).all()               # slots nobody ran stay untouched


def test_kernel_follows_a_trajectory_through_the_goal_ball(ops):
    """Whole 75-step episodes of the goal-seeking script: every row enters the ball, so rewards of 1.0 and the distance test were compared."""
    B, T = 5, 75
    winds = np.zeros((B, J, 2))
    winds[:, 0] = np.array(Wind(n_tasks=60).winds)[[0, 7, 19, 33, 59]]
    n = np.ones(B, dtype=np.int32)
    rep = Replica(B, T, winds, n)
    d = _device(rep, winds, n)
    block = torch.zeros((B, LD_ACTION), device='cuda')
    _call(ops, rep.cfg, True, block, d)
    rep.init()
    inside = np.zeros(B, dtype=np.int64)
    for s in range(T):
        a = _seek(rep)
        block[:, 1:3] = torch.from_numpy(a).cuda()
        _call(ops, rep.cfg, False, block, d)
        rep.step(a)
        inside += rep.in_block[:, 6] == 1.0
        _assert_equal(rep, d, f'step {s}')
    assert (rep.ep_ret[:, 0] >= 30).all() and (rep.ep_ret[:, 0] < T).all() and (rep.ep_len[:, 0] == T).all()
    assert (inside > 0).all()


def test_a_nan_action_takes_numpy_s_branch(ops):
    """numpy's clip lets a NaN through: that component of the position is NaN for the rest of the episode, the reward 0.0, the clock runs on."""
    winds, n = np.full((1, J, 2), 0.01), np.array([1], dtype=np.int32)
    rep = Replica(1, 3, winds, n)
    d = _device(rep, winds, n)
    block = torch.zeros((1, LD_ACTION), device='cuda')
    _call(ops, rep.cfg, True, block, d)
    rep.init()
    for s, a in enumerate([(NAN, 0.5), (0.25, 0.5)]):
        block[0, 1], block[0, 2] = a
        _call(ops, rep.cfg, False, block, d)
        rep.step(np.array([a], dtype=np.float32))
        for k, want in rep.buffers().items():
            got = d[k].cpu().numpy()
            assert np.array_equal(got, want, equal_nan=k in ('in_block', 'env_pos')), (s, k, got, want)
        pos = d['env_pos'][0].cpu().numpy()
        assert np.isnan(pos[0]) and np.isfinite(pos[1]) and d['in_block'][0, 6].item() == 0.0 and d['env_words'][0, 0].item() == s + 1


# ------------------------------------------------------------------------------------------------ 2. rollout kernel against `SAC._push`
def _ring_layout():
    """name2range / width of the ring as the trainer's first `_push` on Wind fixes them (16 columns: logp has none)."""
    m = MemoryArray(20, 6)
    z2 = np.zeros((1, 2))
    m.mem_push(Transition(state=z2, last_state=z2, last_action=z2, action=z2, next_state=z2, reward=0.0, logp=None, mask=1, done=True,
                          timeout=True, start=True, reward_input=np.zeros((1, 1))))
    return dict(m.name2range), m.width


def _permuted_layout():
    """Fields in another order, `timeout` absent (an empty range), no gaps: 15 columns."""
    widths = dict(state=2, last_state=2, last_action=2, action=2, next_state=2, reward=1, logp=0, mask=1, start=1, done=1, reward_input=1, timeout=0)
    order = ['done', 'next_state', 'reward_input', 'last_action', 'logp', 'state', 'mask', 'action', 'timeout', 'start', 'reward', 'last_state']
    out, off = {}, 0
    for name in order:
        out[name] = (off, off + widths[name])
        off += widths[name]
    return out, off


class Twin(types.SimpleNamespace):
    """One row of the host loop: a `Wind`, the trainer's own `_push` / `env_step` on the rollout mirrors, and a ring that records rows."""

    def __init__(self, T, name2range, width):
        ring = MemoryArray(20, 10)
        ring.name2range, ring.width = name2range, width
        super().__init__(env=Wind(n_tasks=2, max_episode_steps=T), ring=ring, rows=[], discrete_env=False, act_dim=2, obs_dim=2,
                         max_episode_steps=T, running=False, ret=0.0, len=0, wind=np.zeros(2))
        self.replay_buffer = self

    def mem_push(self, transition):
        self.rows.append(self.ring.transition_to_array(transition)[0])

    def env_reset(self):                                        # at `done` the device row stops; its reset is the host's next init call
        pass

    def begin(self, wind):
        self.env.set_wind(wind)
        self.state_np = np.asarray(self.env.reset()).reshape((1, -1))
        self.last_action_np, self.last_state_np, self.reward_np = np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 1))
        self.running, self.ret, self.len, self.wind = True, 0.0, 0, np.asarray(wind)

    def step(self, a):
        if not self.running:
            return None
        act = np.asarray(a, dtype=np.float32).reshape(1, -1)
        next_state, reward, done, _ = _host_step(self.env, act[0])
        self.ret += reward
        self.len += 1
        SAC._push(self, act, next_state, reward, done, self.len)
        SAC.env_step(self, next_state, act, reward, done)
        self.running = not done
        return self.rows[-1]

    def in_row(self):
        return np.concatenate([self.state_np, self.last_state_np, self.last_action_np, self.reward_np], axis=1).astype(np.float32)[0]

    def pos(self):
        return np.concatenate([self.state_np[0], self.wind, self.last_state_np[0]])

    def words(self):
        return [self.env.step_count, self.len, 1, int(self.running)]


@pytest.mark.parametrize('short', [0, 1], ids=['cap=T', 'cap=T-1'])
@pytest.mark.parametrize('layout', ['ring', 'permuted'])
@pytest.mark.parametrize('B', [1, 3])
def test_collect_kernel_equals_the_host_twin(ops, B, layout, short):
    T = 4
    name2range, width = _ring_layout() if layout == 'ring' else _permuted_layout()
    ld_row = width if layout == 'ring' else width + 4           # permuted: canary columns behind every row as well
    assert (width, name2range['logp'][1] - name2range['logp'][0]) == ((16, 0) if layout == 'ring' else (15, 0))
    twins = [Twin(T, name2range, width) for _ in range(B)]
    cfg, T_cap = twins[0].env.device_config(), T - short
    cuda = lambda a: torch.from_numpy(a).cuda()
    rs = np.random.RandomState(40 + B)
    winds = rs.uniform(-0.08, 0.08, size=(B, 2))
    exp_traj = np.full((B * T_cap + 2) * ld_row, GAP, dtype=np.float32)
    exp_in = np.full((B, LD_IN), GAP, dtype=np.float32)
    exp_pos, exp_words, exp_ret = np.full((B, 6), -9.5), np.full((B, 4), -9, dtype=np.int32), np.full(B, 0.125)
    traj_all, in_all, pos, words, ret = cuda(exp_traj.copy()), cuda(exp_in.copy()), cuda(exp_pos.copy()), cuda(exp_words.copy()), cuda(exp_ret.copy())
    traj = traj_all[:B * T_cap * ld_row].view(B, T_cap, ld_row)[:, :, :width]
    wind = cuda(winds.copy())
    block = np.full((B, LD_ACTION), GAP, dtype=np.float32)

    def call(init):
        dev_block = cuda(block.copy())
        ops.wind_collect_step(cfg, name2range, init, dev_block[:, 3:5], wind, pos, words, ret, traj, T, in_all[:, :WIDTH])
        assert np.array_equal(_bits(dev_block.cpu().numpy()), _bits(block))                     # the action block is read only

    def check(what):
        for b, tw in enumerate(twins):
            exp_in[b, :WIDTH], exp_pos[b], exp_words[b], exp_ret[b] = tw.in_row(), tw.pos(), tw.words(), tw.ret
        for name, got, want in (('traj', traj_all, exp_traj), ('in_block', in_all, exp_in), ('env_pos', pos, exp_pos),
                                ('env_words', words, exp_words), ('ret', ret, exp_ret)):
            got = got.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), (what, name, got, want)

    block[:, 3:5] = NAN                                         # init reads no action
    call(True)
    for b, tw in enumerate(twins):
        tw.begin(winds[b])
    check('init')                                               # and the episode block is untouched: all canaries
    exp3 = exp_traj[:B * T_cap * ld_row].reshape(B, T_cap, ld_row)
    for s in range(T + 2):                                      # the last two on rows that have stopped
        block[:, 3:5] = rs.uniform(-1.5, 1.5, size=(B, 2))
        if s < len(SPECIAL):
            block[0, 3:5] = SPECIAL[s]
        call(False)
        for b, tw in enumerate(twins):
            row = tw.step(block[b, 3:5])
            assert (row is None) == (s >= T)
            if row is not None and s < T_cap:                   # a step at or behind T_cap stores no row; everything else proceeds
                exp3[b, s, :width] = row
        check(f'step {s}')
    assert all(not tw.running and tw.len == T for tw in twins)
    assert (exp_traj[B * T_cap * ld_row:] == GAP).all() and (exp_in[:, WIDTH:] == GAP).all()
    if ld_row > width:
        assert (exp3[:, :, width:] == GAP).all()
    done, act = name2range['done'][0], name2range['action'][0]
    assert [r[done] for r in twins[0].rows] == [0.0] * (T - 1) + [1.0]
    assert _bits(np.asarray(twins[0].rows[0][act:act + 2])).tolist() == _bits(np.array(SPECIAL[0], dtype=np.float32)).tolist()    # -0.0 kept


def test_wrapper_refuses_a_ring_of_other_widths(ops):
    name2range, width = _ring_layout()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device='cuda')
    cfg = Wind(n_tasks=2, max_episode_steps=4).device_config()
    args = lambda n2r, w: (cfg, n2r, False, z(1, 6)[:, 2:4], z(1, 2, dt=torch.float64), z(1, 6, dt=torch.float64), z(1, 4, dt=torch.int32),
                           z(1, dt=torch.float64), z(1, 4, w), 4, z(1, WIDTH))
    ops.wind_collect_step(*args(name2range, width))             # stopped row: a no-op
    with pytest.raises(AssertionError, match='logp'):
        ops.wind_collect_step(*args(dict(name2range, logp=(width, width + 1)), width + 1))
    with pytest.raises(AssertionError, match='action'):
        ops.wind_collect_step(*args(dict(name2range, action=(name2range['action'][0], name2range['action'][0] + 1)), width))
    with pytest.raises(AssertionError, match='timeout'):
        ops.wind_collect_step(*args(name2range, width - 1))


def test_invalid_arguments_return_einval_and_touch_nothing(ops):
    from offpolicy_rnn.hip import _lib
    B = 2
    z = lambda *s, dt=torch.float32: torch.full(s, 3, dtype=dt, device='cuda')
    t = dict(action=z(B, 2), winds=z(B, J, 2, dt=torch.float64), n=z(B, dt=torch.int32), pos=z(B, 6, dt=torch.float64), words=z(B, 4, dt=torch.int32),
             ret=z(B, dt=torch.float64), ep_ret=z(B, J, dt=torch.float64), ep_len=z(B, J, dt=torch.int32), in_block=z(B, WIDTH), flags=z(B, dt=torch.int32))
    before = {k: v.clone() for k, v in t.items()}
    cfg = Wind(n_tasks=2, max_episode_steps=4).device_config()
    p = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(ld_in=WIDTH, ld_action=2, A=2, J_=J, cfg=cfg):
        c = _lib.WindCfg(int(cfg['episode_length']), *[float(cfg[k]) for k in _lib.WIND_CFG_DOUBLES])
        return _lib.lib().resel_wind_step(c, 0, p(t['action']), ld_action, p(t['winds']), 2 * J, p(t['n']), J_, p(t['pos']), p(t['words']), p(t['ret']),
                                          p(t['ep_ret']), p(t['ep_len']), J, p(t['in_block']), ld_in, A, p(t['flags']), B, None)

    assert call(ld_in=WIDTH - 1) == -1 and call(ld_action=1) == -1 and call(A=4) == -1 and call(J_=0) == -1 and call(J_=J + 1) == -1
    assert call(cfg=dict(cfg, episode_length=0)) == -1 and call(cfg=dict(cfg, goal_radius=NAN)) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(t[k], before[k]) for k in t)


# ------------------------------------------------------------------------------------------------ 3. capturability
def test_init_and_steps_capture_into_a_graph(ops):
    B, T, nsteps = 70, 2, 6
    rs, winds, n = _case(B, 5)
    rep = Replica(B, T, winds, n)
    actions = torch.from_numpy(rs.uniform(-1.5, 1.5, size=(nsteps, B, LD_ACTION)).astype(np.float32)).cuda()

    def sequence(d):
        _call(ops, rep.cfg, True, actions[0], d)
        for s in range(nsteps):
            _call(ops, rep.cfg, False, actions[s], d)

    eager, graphed = _device(rep, winds, n), _device(rep, winds, n)
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
        rep.step(actions[s, :, 1:3].cpu().numpy())
    _assert_equal(rep, eager, 'eager')
    _assert_equal(rep, graphed, 'replay')
    g.replay()                                                  # the init call makes the sequence restartable
    torch.cuda.synchronize()
    _assert_equal(rep, graphed, 'second replay')


# ------------------------------------------------------------------------------------------------ 4. the evaluator
def _flat(store):
    if hasattr(store, 'flat_views'):
        return torch.cat([v.detach().reshape(-1) for _, v in sorted(store.flat_views().items())]).clone()
    return store.flat.detach().clone()


def _generators(dev):
    return (random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2], torch.get_rng_state().tolist(),
            torch.cuda.get_rng_state(dev).tolist())


@pytest.mark.parametrize('rnn', ['gru', 'smamba_s8_c5_b1_ff'])
def test_device_evaluation_equals_the_host_loop(ops, rnn, tmp_path, monkeypatch):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.env_utils.make_env import make_env
    from offpolicy_rnn.utility.policy_eval import BatchedPolicyEval
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    rows, n = 5, 7
    alg = alg_init(make_parameter(rnn, D=32, env='Wind-v0', cuda_inference=True, test_nprocess=n, test_nrollout=1))
    assert not alg.discrete_env and alg.act_dim == 2 and alg.obs_dim == 2 and not getattr(alg.policy, 'categorical', False)
    dev = alg.sample_device
    results = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('RESEL_DEVICE_ENV', mode)
        alg.evaluator = BatchedPolicyEval(alg.policy, lambda: make_env('Wind-v0', alg.env_info['seed'])['eval_env'], alg.act_dim, rows, dev,
                                          seed=alg.parameter.seed, eval_tasks=alg.env_info['eval_tasks'], discrete=False)
        runs = []
        for training in (True, False):                          # two evaluations: the second starts from the first one's streams
            alg.policy.train(training)
            before, gens = _flat(alg.policy.store), _generators(dev)
            out = alg.evaluate()
            assert torch.equal(_flat(alg.policy.store), before) and _generators(dev) == gens
            assert all(m.training is training for m in alg.policy.contextual_modules.values())
            ev = alg.evaluator
            assert (ev.device_env is not None) == (mode == '1') and (ev.step is None) == (mode == '1')
            assert list(out) == ['EpRetTest', 'EpLenTest', 'done_mdpTest'] and out['EpLenTest'] == [75] * n and out['done_mdpTest'] == [1.0] * n
            assert all(type(v) is float for v in out['EpRetTest']) and all(type(v) is int for v in out['EpLenTest'])
            if mode == '1':                                     # where each row's last episode ended, and on which wind
                ps = ev.device_env._env_state[0].cpu().numpy()
                ends, winds = ps[:, 0:2], ps[:, 2:4]
            else:
                ends, winds = np.array([e._state for e in ev.envs]), np.array([e.get_current_task() for e in ev.envs])
            runs.append((out, list(ev.last_rows), _bits(ends).tolist(), _bits(winds).tolist(), ev.rs.get_state()[1].tolist(), ev.rs.get_state()[2]))
        results[mode] = runs
    assert results['1'] == results['0']
    assert results['1'][0][1] == [0, 1, 2, 3, 4, 0, 1]
    assert np.abs(np.array(results['1'][0][2]).view(np.float64)).max() > 0.1                    # the policy moved the rows: positions were compared


# ------------------------------------------------------------------------------------------------ 5. train()
def _run(monkeypatch, tmp_path, device_collect, rnn='gru', algo='sac', **over):
    """One trainer from the seeds of its parameter, `train()`, and everything the two paths must agree on."""
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('RESEL_DEVICE_COLLECT', '1' if device_collect else '0')
    monkeypatch.delenv('RESEL_GRAPH_ROLLOUT', raising=False)
    monkeypatch.delenv('RESEL_GRAPH_UPDATE', raising=False)
    alg = alg_init(make_parameter(rnn, D=32, algo=algo, env='Wind-v0', cuda_inference=True, **over))
    logged, add = [], alg.logger.add_tabular_data

    def record(tb_prefix=None, **kw):
        if tb_prefix == 'Train':
            logged.append((kw['EpRet'], kw['EpLength']))
        return add(tb_prefix=tb_prefix, **kw)

    monkeypatch.setattr(alg.logger, 'add_tabular_data', record)
    alg.train()
    torch.cuda.synchronize()
    ring, e, dev = alg.replay_buffer, alg.env, alg.sample_device
    out = dict(
        ring=_bits(ring.memory_buffer).copy(),
        tables=(list(ring.trajectory_start), list(ring.trajectory_length), ring.ptr, ring.transition_count, len(ring.memory)),
        pending=[_bits(ring.transition_to_array(tr)).tolist() for tr in ring.memory],            # the open episode, as the ring would store it
        logged=[(np.float64(r).view(np.int64).item(), n) for r, n in logged], log_types=sorted({(type(r), type(n)) for r, n in logged}, key=str),
        mirrors=[(a.dtype, a.shape, _bits(a.astype(a.dtype)).tolist()) for a in (alg.state_np, alg.last_state_np, alg.last_action_np, alg.reward_np)],
        env=(_bits(e._state).tolist(), _bits(e._wind).tolist(), e.step_count, e.done_mdp, e._state.dtype, e._wind.dtype),
        hidden=[t.detach().cpu().numpy().view(np.int32).tolist() for t in alg.graph_step._state_tensors()],
        generators=_generators(dev), counts=(alg.sample_num, alg.grad_num),
        policy=_flat(alg.policy.store).cpu().numpy().view(np.int32), values=[_flat(v.store).cpu().numpy().view(np.int32) for v in alg.values],
        targets=[_flat(v.store).cpu().numpy().view(np.int32) for v in alg.target_values], alpha=alg.log_sac_alpha.detach().cpu().numpy().view(np.int32),
    )
    return alg, out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (what, k)
        elif isinstance(a[k], list) and a[k] and isinstance(a[k][0], np.ndarray):
            assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


# three episodes and 20 steps of a fourth behind a one-episode warm-up: `train()` returns inside an episode
TRAIN = dict(random_num=75, total_iteration=1, step_per_iteration=3 * 75 + 20, test_nprocess=0, test_nrollout=0, sac_batch_size=150)


@pytest.mark.parametrize('rnn', ['gru', 'smamba_s8_c5_b1_ff'])
def test_train_without_updates_equals_the_host_loop(ops, rnn, tmp_path, monkeypatch):
    over = dict(TRAIN, start_train_num=10 ** 9)
    host, want = _run(monkeypatch, tmp_path, False, rnn, **over)
    alg, got = _run(monkeypatch, tmp_path, True, rnn, **over)
    assert host.collector is None and host.graph_step._graph is not None
    c = alg.collector
    assert c is not None and alg.graph_step._graph is None      # one graph only: the B = 1 host step was never captured
    _assert_same(got, want, ('no updates', rnn))
    assert want['counts'] == (75 + 245, 0) and want['env'][2] == 20 and len(want['logged']) == 3 and [n for _, n in want['logged']] == [75] * 3
    assert want['tables'][1] == [75] * 4 and len(want['pending']) == 20
    assert c.replays == 245 and c.episode_syncs == 3 and c.init_launches == 4
    train = [alg.env.winds[k] for k in alg.env_info['train_tasks']]
    assert any(np.array_equal(alg.env.get_current_task(), np.array(w)) for w in train)          # the open episode runs on a training task


def test_train_with_two_updates_equals_the_host_loop(ops, tmp_path, monkeypatch):
    """Updates at steps 150 and 225 - the first steps of the second and third collected episode.  The host loop runs twice as a control: the
    update's sums run in a fixed order, so its two runs agree bit for bit, and the device path must equal them."""
    over = dict(TRAIN, start_train_num=150, update_interval=75, step_per_iteration=3 * 75 - 1)
    _, first = _run(monkeypatch, tmp_path, False, **over)
    _, second = _run(monkeypatch, tmp_path, False, **over)
    assert first['counts'] == (75 + 224, 2)
    _assert_same(first, second, 'control: two runs of the host loop')
    alg, got = _run(monkeypatch, tmp_path, True, **over)
    assert alg.collector is not None and alg.collector.replays == 224
    _assert_same(got, first, 'two updates')


# ------------------------------------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize('algo,rollout,reason', [('td3', None, 'tanh-Gaussian'), ('sac', '0', 'RESEL_GRAPH_ROLLOUT=0')])
def test_refusals_name_their_reason(ops, algo, rollout, reason, tmp_path, monkeypatch):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.utility import device_collect
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('RESEL_DEVICE_COLLECT', '1')
    monkeypatch.setenv('RESEL_DEVICE_ENV', '1')
    if rollout is None:
        monkeypatch.delenv('RESEL_GRAPH_ROLLOUT', raising=False)
    else:
        monkeypatch.setenv('RESEL_GRAPH_ROLLOUT', rollout)

    def never(self, alg):
        raise AssertionError('the collector must not be built')

    monkeypatch.setattr(device_collect.DeviceCollector, '__init__', never)
    alg = alg_init(make_parameter('gru', D=32, algo=algo, env='Wind-v0', cuda_inference=True, random_num=75, start_train_num=10 ** 9,
                                  total_iteration=1, step_per_iteration=8, test_nprocess=0, test_nrollout=0))
    said, call = [], type(alg.logger).__call__
    monkeypatch.setattr(type(alg.logger), '__call__', lambda self, *a, **k: (said.append(' '.join(map(str, a))), call(self, *a, **k))[1])
    alg.train()
    why = [s for s in said if 'collected through the host loop' in s]
    assert len(why) == 1 and reason in why[0] and alg.collector is None and alg.sample_num == 75 + 8
    if algo == 'td3':                                           # and its evaluation keeps the host loop as well
        alg.parameter.test_nprocess, alg.parameter.test_nrollout = 2, 1
        out = alg.evaluate()
        assert alg.evaluator.device_env is None and out['EpLenTest'] == [75, 75] and out['done_mdpTest'] == [1.0, 1.0]
