"""Catch on the GPU: the two environment-step kernels (`ops.catch_step`, `ops.catch_collect_step`, csrc/env_step.hip `CatchEnv`) against
replicas built on the host environment (env_utils/catch.py) - every buffer after every call, floats through their bits -, the scheduler's
edge counts, capture into a graph, the evaluator and `train()` with the environment step inside the policy-step graph against the host
loops, a run state taken in mid-episode, and the fall-backs.  The environment is integer-valued: every comparison is exact."""
import gc
import types

import numpy as np
import pytest
import torch

from offpolicy_rnn.algorithm.sac import SAC
from offpolicy_rnn.buffers.transition_buffer.replay_memory import MemoryArray, Transition
from offpolicy_rnn.env_utils.catch import Catch
from test_tmaze_env_gpu import _bits, _flat, _generators, _same_generators

pytestmark = pytest.mark.gpu
J = 3
OBS, A, WIDTH, WORDS, PAY = 49, 3, 102, 90, 80                  # state[49] | lst_state[49] | lst_action[3] | reward[1]; state words; payload
LD_IN, LD_ACTION = 106, 7                                       # wider than the rows: the gaps must stay as they were
GAP = 7.5
NAN = float('nan')


@pytest.fixture(autouse=True)
def no_dead_graphs():
    """A trainer or an evaluator that a test drops is a dead cycle (the step object and its `after_step` hook) that owns a captured graph;
    `torch.cuda.graph` no longer collects before it captures, and a graph finalised INSIDE the next capture ends the process.  So the
    cycles go here, and between the trainers of one test (`gc.collect()` there), never at a moment the allocator picks."""
    gc.collect()
    yield
    gc.collect()


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def _clamp(a):
    return 2 if a >= 2 else (int(a) if a >= 0 else 0)           # NaN fails both comparisons: 0


def _words(env):
    return (env.fruit_row, env.fruit_col, env.basket, env.catch_count, env.time_step, env.accumulated)


def _draws(rs, runs, *lead):
    """Payload rows as the host sends them: ns[40] | ms[40], zeros behind the runs."""
    out = np.zeros(lead + (PAY,), dtype=np.int32)
    out[..., :runs] = rs.randint(0, 6, size=lead + (runs,))
    out[..., 40:40 + runs] = rs.randint(1, 5, size=lead + (runs,))
    return out


def _fruits(row, runs):
    return row[:runs], row[40:40 + runs]


class Replica:
    """What the kernel is specified to do (include/resel_hip.h `resel_catch_step`), on numpy buffers, with one host Catch per row."""

    def __init__(self, B, runs, draws, n_episodes):
        self.B, self.runs, self.draws, self.J = B, runs, draws, draws.shape[1]
        self.n = np.clip(n_episodes, 0, self.J)
        self.envs = [Catch(runs) for _ in range(B)]
        self.cfg = self.envs[0].device_config()
        self.in_block = np.full((B, LD_IN), GAP, dtype=np.float32)
        self.flags = np.full(B, -3, dtype=np.int32)
        self.state = np.full((B, WORDS), -9, dtype=np.int32)
        self.ret_acc = np.full(B, 0.125)
        self.ep_ret, self.ep_len = np.full((B, self.J), -77.0), np.full((B, self.J), -77, dtype=np.int32)

    def buffers(self):
        return dict(in_block=self.in_block, flags=self.flags, env_state=self.state, ret_acc=self.ret_acc, ep_ret=self.ep_ret, ep_len=self.ep_len)

    def _begin(self, b, j):
        self.in_block[b, OBS:WIDTH] = 0.0
        self.flags[b], self.ret_acc[b], self.state[b, 6] = 1, 0.0, 0
        if j < self.n[b]:
            self.in_block[b, :OBS] = self.envs[b].reset(fruits=_fruits(self.draws[b, j], self.runs))
            self.state[b, :6], self.state[b, 10:] = _words(self.envs[b]), self.draws[b, j]
            self.state[b, 7], self.state[b, 8] = j + 1, 1
        else:
            self.state[b, 8] = 0
            self.in_block[b, :OBS] = 0.0

    def init(self):
        self.state[:] = 0
        for b in range(self.B):
            self._begin(b, 0)

    def step(self, action):
        for b in range(self.B):
            if not self.state[b, 8]:
                self.in_block[b, :WIDTH], self.flags[b] = 0.0, 1
                continue
            a = _clamp(action[b])
            obs, r, done, _ = self.envs[b].step(a)
            self.state[b, :6] = _words(self.envs[b])
            row = self.in_block[b]
            row[OBS:2 * OBS] = row[:OBS]
            row[:OBS] = obs
            row[2 * OBS:2 * OBS + A] = np.eye(A, dtype=np.float32)[a]
            row[WIDTH - 1] = np.float32(r)
            self.ret_acc[b] += r
            self.state[b, 6] += 1
            self.flags[b] = 0
            if done:
                j = self.state[b, 7] - 1
                self.ep_ret[b, j], self.ep_len[b, j] = self.ret_acc[b], self.state[b, 6]
                self._begin(b, j + 1)


def _case(B, runs, seed, J=J):
    rs = np.random.RandomState(seed)
    draws = _draws(rs, runs, B, J)
    n = rs.randint(0, J + 1, size=B).astype(np.int32)
    n[0] = J                                                    # row 0 runs throughout: it is the one fed NaN / -1 / 7
    if B >= 5:
        n[1], n[2] = 0, 1                                       # idle from the start, idle after one episode
    return rs, draws, n


def _device(rep, draws, n):
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in rep.buffers().items()}
    dev['draws'], dev['n_episodes'] = torch.from_numpy(draws).cuda(), torch.from_numpy(n).cuda()
    return dev


def _call(ops, cfg, init, action_block, d):
    ops.catch_step(cfg, init, action_block[:, 0], d['draws'], d['n_episodes'], d['env_state'], d['ret_acc'], d['ep_ret'], d['ep_len'],
                   d['in_block'][:, :WIDTH], d['flags'])


def _assert_equal(rep, d, what):
    for k, want in rep.buffers().items():
        got = d[k].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (what, k, np.argwhere(_bits(got) != _bits(want))[:8])


# ------------------------------------------------------------------------------------------------ 1. evaluation kernel against the host environment
@pytest.mark.parametrize('runs', [1, 2])
@pytest.mark.parametrize('B', [1, 5, 64, 70])
def test_kernel_equals_the_host_environment(ops, B, runs):
    rs, draws, n = _case(B, runs, 100 * B + runs)
    rep = Replica(B, runs, draws, n)
    d = _device(rep, draws, n)
    T = rep.cfg['episode_length']
    assert T == 7 * runs - 1
    _call(ops, rep.cfg, True, torch.full((B, LD_ACTION), NAN, device='cuda'), d)                # init reads no action
    rep.init()
    _assert_equal(rep, d, 'init')
    for s in range(J * T + 2):                                  # two more than the longest row needs: every row idle at the end
        block = np.full((B, LD_ACTION), GAP, dtype=np.float32)
        block[:, 0] = rs.randint(0, 3, size=B)
        if s < 3:
            block[0, 0] = (NAN, -1.0, 7.0)[s]
        dev_block = torch.from_numpy(block).cuda()
        _call(ops, rep.cfg, False, dev_block, d)
        rep.step(block[:, 0])
        _assert_equal(rep, d, f'step {s}')
        assert np.array_equal(_bits(dev_block.cpu().numpy()), _bits(block))                    # the action block is read only
    assert int((rep.ep_len > 0).sum()) == int(n.sum()) and not rep.state[:, 8].any() and (rep.flags == 1).all()
    assert (rep.ep_len[rep.ep_len > 0] == T).all() and (rep.in_block[:, WIDTH:] == GAP).all()
    done = rep.ep_ret[rep.ep_len > 0]
    assert ((0 <= done) & (done <= runs) & (done == np.floor(done))).all()
    if B >= 5:
        assert (rep.ep_len[1] == -77).all() and (rep.ep_len[2, 1:] == -77).all()               # slots nobody ran stay untouched


def test_clamped_indices_move_as_0_0_2(ops):
    """From basket column 3: NaN -> 0 (left), -1 -> 0 (left), 7 -> 2 (right)."""
    draws, n = np.zeros((1, J, PAY), dtype=np.int32), np.ones(1, dtype=np.int32)
    draws[0, 0, 0], draws[0, 0, 40] = 5, 3
    rep = Replica(1, 1, draws, n)
    d = _device(rep, draws, n)
    block = torch.zeros((1, LD_ACTION), device='cuda')
    _call(ops, rep.cfg, True, block, d)
    seen = []
    for a in (NAN, -1.0, 7.0):
        block[0, 0] = a
        _call(ops, rep.cfg, False, block, d)
        seen.append((d['env_state'][0, :3].tolist(), d['in_block'][0, 2 * OBS:2 * OBS + A].tolist()))
    assert seen == [([1, 5, 2], [1.0, 0, 0]), ([2, 5, 1], [1.0, 0, 0]), ([3, 5, 2], [0, 0, 1.0])]


def test_forty_runs_read_the_last_payload_slot(ops):
    """runs = 40, B = 3, a greedy catcher: the soft reset of run 39 reads ns[39] / ms[39], the last words of the payload and of the state row."""
    B, runs = 3, 40
    rs = np.random.RandomState(11)
    draws, n = _draws(rs, runs, B, J), np.array([1, 1, 1], dtype=np.int32)
    draws[:, 0, 39], draws[:, 0, 79] = (5, 0, 3), (1, 4, 3)     # the last fruit / basket of each row
    rep = Replica(B, runs, draws, n)
    d = _device(rep, draws, n)
    _call(ops, rep.cfg, True, torch.zeros((B, LD_ACTION), device='cuda'), d)
    rep.init()
    for s in range(rep.cfg['episode_length']):
        block = np.full((B, LD_ACTION), GAP, dtype=np.float32)
        block[:, 0] = [int(np.sign(e.fruit_col - e.basket)) + 1 for e in rep.envs]
        block[2, 0] = rs.randint(0, 3)                          # row 2 plays at random
        _call(ops, rep.cfg, False, torch.from_numpy(block).cuda(), d)
        rep.step(block[:, 0])
        if s == 272:                                            # t = 273 = 7 * 39: the last soft reset
            assert [e.catch_count for e in rep.envs] == [40] * 3 and [e.fruit_col for e in rep.envs] == [5, 0, 3]
        if s % 40 == 0 or s >= 270:
            _assert_equal(rep, d, f'step {s}')
    _assert_equal(rep, d, 'end')
    assert rep.ep_len[:, 0].tolist() == [279] * 3 and rep.ep_ret[:2, 0].tolist() == [40.0, 40.0] and 0 <= rep.ep_ret[2, 0] < 40


def test_a_caught_fruit_is_covered_by_the_basket(ops):
    draws, n = np.zeros((1, J, PAY), dtype=np.int32), np.ones(1, dtype=np.int32)
    draws[0, 0, :2], draws[0, 0, 40:42] = (2, 0), (2, 4)        # the first fruit falls onto a basket that stays, the second beside it
    rep = Replica(1, 2, draws, n)
    d = _device(rep, draws, n)
    block = torch.ones((1, LD_ACTION), device='cuda')
    _call(ops, rep.cfg, True, block, d)
    rep.init()
    for s in range(13):
        _call(ops, rep.cfg, False, block, d)
        rep.step([1.0])
        _assert_equal(rep, d, f'step {s}')
        row = d['in_block'][0].cpu().numpy()
        if s == 5:                                              # the fruit in the basket's cell: one entry, +1; the catch is not paid yet
            assert np.nonzero(row[:OBS])[0].tolist() == [44] and row[44] == 1.0 and np.nonzero(row[OBS:2 * OBS])[0].tolist() == [37, 44]
            assert row[WIDTH - 1] == 0.0 and d['env_state'][0, 5].item() == 1 and d['ret_acc'][0].item() == 0.0
        if s == 6:                                              # the soft reset
            assert np.nonzero(row[:OBS])[0].tolist() == [0, 46]
    assert d['ep_ret'][0, 0].item() == 1.0 and d['ep_len'][0, 0].item() == 13 and not row[:WIDTH].any()    # paid at the end; the row went idle


def test_a_row_idle_from_init_next_to_a_row_clamped_to_J(ops):
    B, J2, runs = 3, 2, 1
    T = 7 * runs - 1
    rs = np.random.RandomState(7)
    n = np.array([0, J2 + 2, 1], dtype=np.int32)                # idle from the start | more than its J payloads | idle after one episode
    draws = _draws(rs, runs, B, J2)
    rep = Replica(B, runs, draws, n)
    assert rep.n.tolist() == [0, J2, 1]
    d = _device(rep, draws, n)                                  # the device sees the counts as asked for
    _call(ops, rep.cfg, True, torch.full((B, LD_ACTION), NAN, device='cuda'), d)
    rep.init()
    _assert_equal(rep, d, 'init')
    running = []
    for s in range(J2 * T + 2):
        block = np.full((B, LD_ACTION), GAP, dtype=np.float32)
        block[:, 0] = rs.randint(0, 3, size=B)
        _call(ops, rep.cfg, False, torch.from_numpy(block).cuda(), d)
        rep.step(block[:, 0])
        _assert_equal(rep, d, f'step {s}')
        running.append((rep.flags == 0).tolist())
    assert not any(r[0] for r in running) and (rep.ep_len[0] == -77).all()                     # row 0 never ran, its slots untouched
    assert (rep.ep_len[1] == T).all() and sum(r[1] for r in running) == J2 * T - J2            # row 1: exactly J episodes, then idle
    assert rep.ep_len[2].tolist() == [T, -77] and (rep.flags == 1).all()


def test_init_and_steps_capture_into_a_graph(ops):
    B, runs, nsteps = 70, 1, 8
    rs, draws, n = _case(B, runs, 5)
    rep = Replica(B, runs, draws, n)
    actions = torch.from_numpy(rs.randint(0, 3, size=(nsteps, B, LD_ACTION)).astype(np.float32)).cuda()

    def sequence(d):
        _call(ops, rep.cfg, True, actions[0], d)
        for s in range(nsteps):
            _call(ops, rep.cfg, False, actions[s], d)

    eager, graphed = _device(rep, draws, n), _device(rep, draws, n)
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


# ------------------------------------------------------------------------------------------------ 2. rollout kernel against `SAC._push`
_WIDTHS = dict(state=OBS, last_state=OBS, last_action=A, action=1, next_state=OBS, reward=1, logp=0, mask=1, start=1, done=1, reward_input=1, timeout=1)


def _ring_layout():
    """name2range / width of the ring as the trainer's first `_push` on Catch fixes them (157 columns: logp has none)."""
    m = MemoryArray(20, 6)
    zo, za = np.zeros((1, OBS), dtype=np.float32), np.zeros((1, A))
    m.mem_push(Transition(state=zo, last_state=zo, last_action=za, action=np.zeros((1, 1), dtype=np.int64), next_state=zo, reward=0.0, logp=None,
                          mask=1, done=True, timeout=True, start=True, reward_input=np.zeros((1, 1))))
    return dict(m.name2range), m.width


def _permuted_layout():
    """Fields in another order, `timeout` absent (an empty range), no gaps: 156 columns."""
    widths = dict(_WIDTHS, timeout=0)
    order = ['done', 'next_state', 'reward_input', 'last_action', 'logp', 'state', 'mask', 'action', 'timeout', 'start', 'reward', 'last_state']
    out, off = {}, 0
    for name in order:
        out[name] = (off, off + widths[name])
        off += widths[name]
    return out, off


class Twin(types.SimpleNamespace):
    """One row of the host loop: a `Catch`, the trainer's own `_push` / `env_step` on the rollout mirrors, and a ring that records rows."""

    def __init__(self, runs, name2range, width):
        env = Catch(runs)
        ring = MemoryArray(20, 10)
        ring.name2range, ring.width = name2range, width
        super().__init__(env=env, ring=ring, rows=[], discrete_env=True, act_dim=A, obs_dim=OBS, max_episode_steps=env.episode_length,
                         running=False, ret=0.0, len=0, draws=np.zeros(PAY, dtype=np.int32))
        self.replay_buffer = self

    def mem_push(self, transition):
        self.rows.append(self.ring.transition_to_array(transition)[0])

    def env_reset(self):                                        # at `done` the device row stops; its reset is the host's next init call
        pass

    def begin(self, draws):
        self.draws = draws
        self.state_np = np.asarray(self.env.reset(fruits=_fruits(draws, self.env.runs))).reshape((1, -1))
        self.last_action_np, self.last_state_np, self.reward_np = np.zeros((1, A)), np.zeros((1, OBS)), np.zeros((1, 1))
        self.running, self.ret, self.len = True, 0.0, 0

    def step(self, word):
        """-> the transition row this step stores, or None for a stopped row."""
        if not self.running:
            return None
        a = _clamp(word)
        act = np.array([[a]], dtype=np.int64)
        next_state, reward, done, _ = self.env.step(a)
        self.ret += reward
        self.len += 1
        SAC._push(self, act, next_state, reward, done, self.len)
        SAC.env_step(self, next_state, act, reward, done)
        self.running = not done
        return self.rows[-1]

    def in_row(self):
        return np.concatenate([self.state_np, self.last_state_np, self.last_action_np, self.reward_np], axis=1).astype(np.float32)[0]

    def words(self):
        return list(_words(self.env)) + [self.len, 1, int(self.running), 0] + self.draws.tolist()


@pytest.mark.parametrize('short', [0, 1], ids=['cap=T', 'cap=T-1'])
@pytest.mark.parametrize('layout', ['ring', 'permuted'])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('runs', [1, 2])
def test_collect_kernel_equals_the_host_twin(ops, runs, B, layout, short):
    name2range, width = _ring_layout() if layout == 'ring' else _permuted_layout()
    ld_row = width if layout == 'ring' else width + 4           # permuted: canary columns behind every row as well
    assert (width, name2range['logp'][1] - name2range['logp'][0]) == ((157, 0) if layout == 'ring' else (156, 0))
    twins = [Twin(runs, name2range, width) for _ in range(B)]
    cfg, T = twins[0].env.device_config(), twins[0].env.episode_length
    T_cap = T - short
    cuda = lambda a: torch.from_numpy(a).cuda()
    rs = np.random.RandomState(40 + 10 * runs + B)
    draws = _draws(rs, runs, B)
    draws[0, 0], draws[0, 40] = 3, 3                            # row 0: the fruit above the basket, which the script below leaves there
    # the episode block with two canary rows behind it, the input block with canary columns, state words that an init must overwrite
    exp_traj = np.full((B * T_cap + 2) * ld_row, GAP, dtype=np.float32)
    exp_in = np.full((B, LD_IN), GAP, dtype=np.float32)
    exp_state, exp_ret = np.full((B, WORDS), -9, dtype=np.int32), np.full(B, 0.125)
    traj_all, in_all, state, ret = cuda(exp_traj.copy()), cuda(exp_in.copy()), cuda(exp_state.copy()), cuda(exp_ret.copy())
    traj = traj_all[:B * T_cap * ld_row].view(B, T_cap, ld_row)[:, :, :width]
    dev_draws = cuda(draws.copy())
    block = np.full((B, LD_ACTION), GAP, dtype=np.float32)
    block[:, 0] = 2.0                                           # the mode column: never read

    def call(init):
        dev_block = cuda(block.copy())
        ops.catch_collect_step(cfg, name2range, init, dev_block[:, 1], dev_draws, state, ret, traj, T, in_all[:, :WIDTH])
        assert np.array_equal(_bits(dev_block.cpu().numpy()), _bits(block))                     # the action block is read only

    def check(what):
        for b, tw in enumerate(twins):
            exp_in[b, :WIDTH], exp_state[b], exp_ret[b] = tw.in_row(), tw.words(), tw.ret
        for name, got, want in (('traj', traj_all, exp_traj), ('in_block', in_all, exp_in), ('env_state', state, exp_state), ('ret', ret, exp_ret)):
            got = got.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), (what, name, np.argwhere(_bits(got) != _bits(want))[:8])

    block[:, 1] = NAN                                           # init reads no action
    call(True)
    for b, tw in enumerate(twins):
        tw.begin(draws[b])
    check('init')                                               # and the episode block is untouched: all canaries
    exp3 = exp_traj[:B * T_cap * ld_row].reshape(B, T_cap, ld_row)
    special = (NAN, 7.0, -1.0, 2.0)                             # row 0: left, right, left, right - back under the fruit -, then it stays
    for s in range(T + 2):                                      # the last two on rows that have stopped
        block[:, 1] = rs.randint(0, 3, size=B)
        block[0, 1] = special[s] if s < len(special) else 1.0
        call(False)
        for b, tw in enumerate(twins):
            row = tw.step(block[b, 1])
            assert (row is None) == (s >= T)
            if row is not None and s < T_cap:                   # a step at or behind T_cap stores no row; everything else proceeds
                exp3[b, s, :width] = row
        check(f'step {s}')
    assert all(not tw.running and tw.len == T for tw in twins)
    assert (exp_traj[B * T_cap * ld_row:] == GAP).all() and (exp_in[:, WIDTH:] == GAP).all()
    if ld_row > width:
        assert (exp3[:, :, width:] == GAP).all()
    done, rew, nxt = name2range['done'][0], name2range['reward'][0], name2range['next_state'][0]
    assert [r[done] for r in twins[0].rows] == [0.0] * (T - 1) + [1.0]
    assert not any(r[rew] for r in twins[0].rows[:-1]) and twins[0].rows[-1][rew] == twins[0].ret >= 1.0      # row 0 caught its first fruit
    assert np.count_nonzero(twins[0].rows[5][nxt:nxt + OBS]) == 1                                 # and the basket covered it


def test_wrapper_refuses_a_ring_of_other_widths(ops):
    name2range, width = _ring_layout()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device='cuda')
    args = lambda n2r, w: (dict(num_catches=1, episode_length=6), n2r, False, z(1, 6)[:, 1], z(1, PAY, dt=torch.int32), z(1, WORDS, dt=torch.int32),
                           z(1, dt=torch.float64), z(1, 6, w), 6, z(1, WIDTH))
    ops.catch_collect_step(*args(name2range, width))            # stopped row: a no-op
    with pytest.raises(AssertionError, match='logp'):
        ops.catch_collect_step(*args(dict(name2range, logp=(width, width + 1)), width + 1))
    with pytest.raises(AssertionError, match='state'):
        ops.catch_collect_step(*args(dict(name2range, state=(0, 2)), width))
    with pytest.raises(AssertionError, match='timeout'):
        ops.catch_collect_step(*args(name2range, width - 1))


# ------------------------------------------------------------------------------------------------ 3. the evaluator
ENV = 'Catch-2-v0'
T2 = 13


@pytest.mark.parametrize('rnn', ['gru', 'smamba_s8_c4_b2_nln'])
def test_device_evaluation_equals_the_host_loop(ops, rnn, tmp_path, monkeypatch):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.env_utils.make_env import make_env
    from offpolicy_rnn.utility.policy_eval import BatchedPolicyEval
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    alg = alg_init(make_parameter(rnn, env=ENV, cuda_inference=True))
    assert alg.discrete_env and alg.act_dim == 3 and alg.obs_dim == 49 and alg.policy.categorical
    dev = alg.sample_device
    results = {}
    ev = None
    for mode in ('1', '0'):
        monkeypatch.setenv('RESEL_DEVICE_ENV', mode)
        del ev
        gc.collect()                                            # the other mode's evaluator and its graph go before the next capture
        ev = BatchedPolicyEval(alg.policy, lambda: make_env(ENV, 0)['eval_env'], 3, 4, dev, seed=3, discrete=True)
        runs = []
        for n, training in ((7, True), (3, False)):             # two waves with an idle row in the last; one wave with an idle row
            alg.policy.train(training)
            before, gens = _flat(alg.policy.store), _generators(dev)
            out = ev.evaluate(n)
            assert torch.equal(_flat(alg.policy.store), before) and _same_generators(_generators(dev), gens)
            assert all(m.training is training for m in alg.policy.contextual_modules.values())
            assert list(out) == ['EpRetTest', 'EpLenTest'] and out['EpLenTest'] == [T2] * n
            assert all(type(v) is float and v in (0.0, 1.0, 2.0) for v in out['EpRetTest']) and all(type(v) is int for v in out['EpLenTest'])
            assert (ev.device_env is not None) == (mode == '1') and (ev.step is None) == (mode == '1')
            streams = [(e._rs.get_state()[1].tolist(), e._rs.get_state()[2]) for e in ev.envs]    # every row drew its episodes' fruits, no more
            runs.append((out['EpRetTest'], out['EpLenTest'], list(ev.last_rows), streams, ev.rs.get_state()[1].tolist(), ev.rs.get_state()[2]))
        results[mode] = runs
    assert results['1'] == results['0']
    assert results['1'][0][2] == [0, 1, 2, 3, 0, 1, 2] and results['1'][1][2] == [0, 1, 2]


# ------------------------------------------------------------------------------------------------ 4. train()
TRAIN = dict(random_num=26, update_interval=13, total_iteration=2, step_per_iteration=20, test_nprocess=1, test_nrollout=2, sac_batch_size=26)


def _run(monkeypatch, tmp_path, device_collect, graph_update=None, env=ENV, **over):
    """One trainer from the seeds of its parameter, `train()` -> (trainer, its snapshot with the training episodes it logged)."""
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    from test_run_state_host import snapshot
    gc.collect()                                                # the trainer before this one, with its graphs
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('RESEL_DEVICE_COLLECT', '1' if device_collect else '0')
    monkeypatch.delenv('RESEL_GRAPH_ROLLOUT', raising=False)
    monkeypatch.delenv('RESEL_CHECKPOINT_DIR', raising=False)
    if graph_update is None:
        monkeypatch.delenv('RESEL_GRAPH_UPDATE', raising=False)
    else:
        monkeypatch.setenv('RESEL_GRAPH_UPDATE', graph_update)
    alg = alg_init(make_parameter('gru', env=env, cuda_inference=True, **dict(TRAIN, **over)))
    logged, add = [], alg.logger.add_tabular_data

    def record(tb_prefix=None, **kw):
        if tb_prefix == 'Train':
            logged.append((np.float64(kw['EpRet']).view(np.int64).item(), type(kw['EpRet']), kw['EpLength'], type(kw['EpLength'])))
        return add(tb_prefix=tb_prefix, **kw)

    monkeypatch.setattr(alg.logger, 'add_tabular_data', record)
    alg.train()
    snap = snapshot(alg)
    # the open episode is compared as the rows the ring would store (`pending`); as objects the two paths' transitions differ by design:
    # `sync_host` rebuilds them from those fp32 rows, the host loop holds what `_push` was given (an int64 action, float64 zeros)
    del snap['pending_types']
    snap['logged'] = logged
    return alg, snap


def test_train_without_updates_equals_the_host_loop(ops, tmp_path, monkeypatch):
    """Two iterations of 20 steps on thirteen-step episodes: the second evaluation falls inside an episode, and so does the end."""
    from test_run_state_host import assert_same
    over = dict(start_train_num=10 ** 9)
    host, want = _run(monkeypatch, tmp_path, False, **over)
    alg, got = _run(monkeypatch, tmp_path, True, **over)
    assert host.collector is None and host.graph_step._graph is not None and host.evaluator is not None and alg.evaluator is not None
    c = alg.collector
    assert c is not None and alg.graph_step._graph is None      # one graph only: the B = 1 host step was never captured
    assert_same(got, want, 'no updates')
    assert want['counts'] == (26 + 40, 0, 2) and want['episode'][1] == 40 % T2 == len(want['pending']) and len(want['logged']) == 40 // T2
    assert [n for _, _, n, _ in want['logged']] == [T2] * 3 and want['tables'][1] == [T2] * 5
    assert c.replays == 40 and c.episode_syncs == 3 and c.init_launches == 4
    assert alg.env.time_step == 1 and alg.env.ns.shape == (2,) and alg.env.ns.dtype == np.int64


def test_train_with_two_updates_equals_the_host_loop(ops, tmp_path, monkeypatch):
    """Eager updates at steps 26 and 39 - the first steps of the first and second collected episode.  The host loop runs twice as a
    control: the update's sums run in a fixed order, so its two runs agree bit for bit, and the device path must equal them."""
    from test_run_state_host import assert_same
    over = dict(start_train_num=26, total_iteration=1, step_per_iteration=2 * T2 - 1, test_nprocess=0, test_nrollout=0)
    _, first = _run(monkeypatch, tmp_path, False, '0', **over)
    _, second = _run(monkeypatch, tmp_path, False, '0', **over)
    assert first['counts'] == (26 + 25, 2, 1)
    assert_same(first, second, 'control: two runs of the host loop')
    alg, got = _run(monkeypatch, tmp_path, True, '0', **over)
    assert alg.collector is not None and alg.collector.replays == 25
    assert_same(got, first, 'two updates')


def test_a_run_state_taken_in_mid_episode_continues_bit_for_bit(ops, tmp_path, monkeypatch):
    """Four iterations of 20 steps without updates; the state of iteration 2 falls one step into a thirteen-step episode.  The resumed run
    finishes that episode through the host loop - on the fruits, basket and count that `sync_env` brought back from the state words - and
    the collector takes over behind its `env_reset()`."""
    import os
    from test_run_state_gpu import NO_UPDATES, _only_state
    from test_run_state_gpu import _run as run
    from test_run_state_host import assert_same
    kw = dict(NO_UPDATES, collect=True, random_num=26, total_iteration=4)
    # (a) without a checkpoint directory, (b) with a state every two iterations, (c) a fresh trainer that finds only `state-000002`
    _, want, logged = run(monkeypatch, tmp_path, 'gru', ENV, **kw)
    gc.collect()
    _, with_states, _ = run(monkeypatch, tmp_path, 'gru', ENV, ckpt_dir=tmp_path / 'b', **kw)
    gc.collect()
    assert sorted(os.listdir(tmp_path / 'b')) == ['state-000002', 'state-000004']
    alg, got, tail = run(monkeypatch, tmp_path, 'gru', ENV, ckpt_dir=_only_state(tmp_path / 'b', tmp_path / 'c', 'state-000002'), **kw)
    assert want['counts'] == (26 + 80, 0, 4) and len(logged) == 80 // T2
    assert_same(with_states, want, 'states written on the way')
    assert_same(got, want, 'resumed from iteration 2')
    assert tail == logged[-len(tail):] and len(tail) == 80 // T2 - 40 // T2
    c = alg.collector
    host_steps = T2 - 40 % T2                                   # the steps that finished the open episode
    assert c is not None and host_steps == 12 and c.replays == 40 - host_steps and alg.graph_step._graph is not None
    assert c.episode_syncs == (40 - host_steps) // T2 and c.init_launches == c.episode_syncs + 1


# ------------------------------------------------------------------------------------------------ 5. fall-backs
@pytest.mark.parametrize('env,switch,rollout,reason', [('Catch-41-v0', '1', None, 'no device step'), (ENV, '0', None, 'RESEL_DEVICE_COLLECT=0'),
                                                       (ENV, '1', '0', 'RESEL_GRAPH_ROLLOUT=0')])
def test_fallbacks_take_the_host_loop_and_say_why_once(ops, env, switch, rollout, reason, tmp_path, monkeypatch):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.utility import device_collect
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('RESEL_DEVICE_COLLECT', switch)
    monkeypatch.setenv('RESEL_DEVICE_ENV', switch)
    if rollout is None:
        monkeypatch.delenv('RESEL_GRAPH_ROLLOUT', raising=False)
    else:
        monkeypatch.setenv('RESEL_GRAPH_ROLLOUT', rollout)

    def never(self, alg):
        raise AssertionError('the collector must not be built')

    monkeypatch.setattr(device_collect.DeviceCollector, '__init__', never)
    T = 7 * int(env.split('-')[1]) - 1
    alg = alg_init(make_parameter('gru', env=env, cuda_inference=True, random_num=T, start_train_num=10 ** 9, total_iteration=1,
                                  step_per_iteration=8, test_nprocess=0, test_nrollout=0))
    said, call = [], type(alg.logger).__call__
    monkeypatch.setattr(type(alg.logger), '__call__', lambda self, *a, **k: (said.append(' '.join(map(str, a))), call(self, *a, **k))[1])
    alg.train()
    alg.train()
    why = [s for s in said if 'collected through the host loop' in s]
    assert len(why) == 1 and reason in why[0] and alg.collector is None and alg.sample_num == 2 * (T + 8)
    if rollout is None:                                         # and the evaluation keeps the host loop as well
        alg.parameter.test_nprocess, alg.parameter.test_nrollout = 2, 1
        out = alg.evaluate()
        assert alg.evaluator.device_env is None and alg.evaluator.step is not None and out['EpLenTest'] == [T, T]


def test_td3_never_reaches_the_device_paths(ops, tmp_path, monkeypatch):
    """TD3 has no discrete-action form, so no TD3 trainer exists on a Catch name; a policy that is not a categorical one - TD3's has a
    `sample_std` and no `categorical` - is refused by the record, with the reason the trainer would log."""
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.env_utils.device_env import CatchKind
    from offpolicy_rnn.utility.device_collect import DeviceCollector
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('RESEL_DEVICE_COLLECT', '1')
    with pytest.raises(NotImplementedError, match='TD3 has no discrete-action form'):
        alg_init(make_parameter('gru', algo='td3', env=ENV, cuda_inference=True))
    td3_like = types.SimpleNamespace(sample_std=0.1)
    assert not CatchKind.policy_ok(td3_like) and CatchKind.policy_ok(types.SimpleNamespace(categorical=True))
    stub = types.SimpleNamespace(env=Catch(2), sample_device=torch.device('cuda'), policy=td3_like)
    assert 'not a categorical one' in DeviceCollector.refusal(stub)
