"""Training rollouts of a discrete T-Maze on the device (utility/device_collect.py, `ops.tmaze_collect_step`, csrc/env_step.hip):
1. the kernel against the host twin - `TMaze.step`, `SAC._push` (`Transition` + `transition_to_array`) and `SAC.env_step` - after every step;
2. the collector against the host loop with frozen parameters; 3. `train()` end to end, without and with updates; 4. the fall-backs.
Both sides execute the same arithmetic, so every comparison is on bit patterns (an int32 view of fp32: -0.0 counts)."""
import random
import types

import numpy as np
import pytest
import torch

from offpolicy_rnn.algorithm.sac import SAC
from offpolicy_rnn.buffers.transition_buffer.replay_memory import MemoryArray, Transition, tuplenames
from offpolicy_rnn.env_utils.tmaze import TMaze

pytestmark = pytest.mark.gpu
GAP = 7.5                                                       # canary value of every column / row the kernel must not touch
LD_IN, LD_ACTION = 12, 6
NAN = float('nan')
HOST_RUNS_DIFFER = 'two runs of the host loop do not agree bit for bit on this GPU'


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _clamp(a):
    return 3 if a >= 3 else (int(a) if a >= 0 else 0)           # NaN fails both comparisons: 0


# ------------------------------------------------------------------------------------------------ 1. kernel against the host twin
def _ring_layout():
    """name2range / width of the ring as the trainer's first `_push` fixes them (17 columns: logp has none)."""
    m = MemoryArray(20, 6)
    z2, z4 = np.zeros((1, 2), dtype=np.float32), np.zeros((1, 4))
    m.mem_push(Transition(state=z2, last_state=z2, last_action=z4, action=np.zeros((1, 1), dtype=np.int64), next_state=z2, reward=0.0, logp=None,
                          mask=1, done=True, timeout=True, start=True, reward_input=np.zeros((1, 1))))
    return dict(m.name2range), m.width


def _permuted_layout():
    """Fields in another order, `timeout` absent (an empty range), no gaps: 16 columns."""
    widths = dict(_WIDTHS, timeout=0)
    order = ['done', 'next_state', 'reward_input', 'last_action', 'logp', 'state', 'mask', 'action', 'timeout', 'start', 'reward', 'last_state']
    out, off = {}, 0
    for name in order:
        out[name] = (off, off + widths[name])
        off += widths[name]
    return out, off


_WIDTHS = dict(state=2, last_state=2, last_action=4, action=1, next_state=2, reward=1, logp=0, mask=1, start=1, done=1, reward_input=1, timeout=1)
# index words as the head kernel could leave them in the block; per environment one script per row, T steps each
SCRIPTS = {
    # passive L = 3: start (0, 0) at the oracle, junction x = 3, T = 4
    ('passive', 3): [[2.0, 0.0, 2.0, NAN],                     # left into the wall, right, back onto x = 0 (seen before: no goal shown), NaN -> right
                     [7.0, 1.0, 0.0, 3.0],                      # 7 -> down into the wall, up into the wall, right, down into the wall
                     [-1.0, 0.0, 0.0, 1.0]],                    # -1 -> right, right, right to the junction, up onto a goal cell
    # active L = 2: start (1, 0), oracle at x = 0, junction x = 3, T = 5
    ('active', 2): [[2.0, 2.0, 0.0, 2.0, NAN],                  # onto the oracle, into the wall, right, back onto x = 0, NaN -> right
                    [0.0, 0.0, 3.0, 1.0, 7.0],                  # to the junction, down onto a goal cell, up, 7 -> down again
                    [-3.0, 1.0, 2.0, 2.0, 0.0]],
}
GOALS = [1, -1, 1]


class Twin(types.SimpleNamespace):
    """One row of the host loop: a `TMaze`, the trainer's own `_push` / `env_step` on the rollout mirrors, and a ring that records rows."""

    def __init__(self, kind, L, name2range, width):
        env = TMaze(L, oracle_length=int(kind == 'active'), penalty=-1.0 / L)
        ring = MemoryArray(20, 10)
        ring.name2range, ring.width = name2range, width
        super().__init__(env=env, ring=ring, rows=[], discrete_env=True, act_dim=4, obs_dim=2, max_episode_steps=env.episode_length,
                         running=False, ret=0.0, len=0)
        self.replay_buffer = self

    def mem_push(self, transition):
        self.rows.append(self.ring.transition_to_array(transition)[0])

    def env_reset(self):                                        # at `done` the device row stops; its reset is the host's next init call
        pass

    def begin(self, goal):
        self.state_np = np.asarray(self.env.reset(goal=goal)).reshape((1, -1))
        self.last_action_np, self.last_state_np, self.reward_np = np.zeros((1, 4)), np.zeros((1, 2)), np.zeros((1, 1))
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
        e = self.env
        return [e.x, e.y, e.goal_y, int(e.oracle_visited), e.time_step, self.len, 1, int(self.running)]


@pytest.mark.parametrize('short', [0, 2], ids=['cap=T', 'cap=T-2'])
@pytest.mark.parametrize('layout', ['ring', 'permuted'])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('kind,L', [('passive', 3), ('active', 2)])
def test_kernel_equals_the_host_twin(ops, kind, L, B, layout, short):
    name2range, width = _ring_layout() if layout == 'ring' else _permuted_layout()
    ld_row = width if layout == 'ring' else width + 4           # permuted: canary columns behind every row as well
    assert (width, name2range['logp'][1] - name2range['logp'][0]) == ((17, 0) if layout == 'ring' else (16, 0))
    twins = [Twin(kind, L, name2range, width) for _ in range(B)]
    cfg, T = twins[0].env.device_config(), twins[0].env.episode_length
    assert T == len(SCRIPTS[kind, L][0]) == (4 if kind == 'passive' else 5)
    T_cap = T - short
    cuda = lambda a: torch.from_numpy(a).cuda()
    # the episode block with two canary rows behind it, the input block with canary columns, state words that an init must overwrite
    exp_traj = np.full((B * T_cap + 2) * ld_row, GAP, dtype=np.float32)
    exp_in = np.full((B, LD_IN), GAP, dtype=np.float32)
    exp_state, exp_ret = np.full((B, 8), -9, dtype=np.int32), np.full(B, 0.125)
    traj_all, in_all, state, ret = cuda(exp_traj.copy()), cuda(exp_in.copy()), cuda(exp_state.copy()), cuda(exp_ret.copy())
    traj = traj_all[:B * T_cap * ld_row].view(B, T_cap, ld_row)[:, :, :width]
    goal = cuda(np.array(GOALS[:B], dtype=np.int32))
    block = np.full((B, LD_ACTION), GAP, dtype=np.float32)
    block[:, 0] = 2.0                                           # the mode column: never read

    def call(init):
        dev_block = cuda(block.copy())
        ops.tmaze_collect_step(cfg, name2range, init, dev_block[:, 1], goal, state, ret, traj, T, in_all[:, :9])
        assert np.array_equal(_bits(dev_block.cpu().numpy()), _bits(block))                     # the action block is read only

    def check(what):
        for b, tw in enumerate(twins):
            exp_in[b, :9], exp_state[b], exp_ret[b] = tw.in_row(), tw.words(), tw.ret
        for name, got, want in (('traj', traj_all, exp_traj), ('in_block', in_all, exp_in), ('env_state', state, exp_state), ('ret', ret, exp_ret)):
            got = got.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), (what, name, got, want)

    block[:, 1] = NAN                                           # init reads no action
    call(True)
    for b, tw in enumerate(twins):
        tw.begin(GOALS[b])
    check('init')                                               # and the episode block is untouched: all canaries
    exp3 = exp_traj[:B * T_cap * ld_row].reshape(B, T_cap, ld_row)
    for s in range(T_cap + short + 2):                          # T + 2 steps: the last two on rows that have stopped
        for b in range(B):
            block[b, 1] = SCRIPTS[kind, L][b][s] if s < T else float(s % 4)
        call(False)
        for b, tw in enumerate(twins):
            row = tw.step(block[b, 1])
            assert (row is None) == (s >= T)
            if row is not None and s < T_cap:                   # a step at or behind T_cap stores no row; everything else proceeds
                exp3[b, s, :width] = row
        check(f'step {s}')
    assert all(not tw.running and tw.len == T for tw in twins)
    assert (exp_traj[B * T_cap * ld_row:] == GAP).all() and (exp_in[:, 9:] == GAP).all()
    if ld_row > width:
        assert (exp3[:, :, width:] == GAP).all()
    if kind == 'passive':                                       # the scripts did what their comments say: walls, a second visit of x = 0
        assert [twins[0].rows[k][name2range['next_state'][0] + 1] for k in range(3)] == [0.0, 0.0, 0.0]
    done = name2range['done'][0]
    assert [r[done] for r in twins[0].rows] == [0.0] * (T - 1) + [1.0]
    if B == 3:                                                  # rows 1 / 2 keep the schedule at first: a -0.0 reward was compared
        assert any((_bits(np.asarray(tw.rows)) == np.float32(-0.0).view(np.int32)).any() for tw in twins)


def test_wrapper_refuses_a_ring_of_other_widths(ops):
    name2range, width = _ring_layout()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device='cuda')
    args = lambda n2r, w: (dict(corridor_length=3, oracle_length=0, episode_length=4, goal_reward=1.0, penalty=-1 / 3, distract_reward=0.0), n2r,
                           False, z(1, 6)[:, 1], z(1, dt=torch.int32), z(1, 8, dt=torch.int32), z(1, dt=torch.float64), z(1, 4, w), 4, z(1, 9))
    ops.tmaze_collect_step(*args(name2range, width))            # stopped row: a no-op
    wide = dict(name2range, logp=(width, width + 1))
    with pytest.raises(AssertionError, match='logp'):
        ops.tmaze_collect_step(*args(wide, width + 1))
    with pytest.raises(AssertionError, match='timeout'):
        ops.tmaze_collect_step(*args(name2range, width - 1))


# ------------------------------------------------------------------------------------------------ 2. / 3. collector against the host loop
def _flat(store):
    if hasattr(store, 'flat_views'):
        return torch.cat([v.detach().reshape(-1) for _, v in sorted(store.flat_views().items())]).clone()
    return store.flat.detach().clone()


def _run(monkeypatch, tmp_path, device_collect, rnn, env, graph_update=None, **over):
    """One trainer from the seeds of its parameter, `train()`, and everything the two paths must agree on."""
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.hip.graph_step import GraphedPolicyStep
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('RESEL_DEVICE_COLLECT', '1' if device_collect else '0')
    monkeypatch.delenv('RESEL_GRAPH_ROLLOUT', raising=False)
    if graph_update is None:
        monkeypatch.delenv('RESEL_GRAPH_UPDATE', raising=False)
    else:
        monkeypatch.setenv('RESEL_GRAPH_UPDATE', graph_update)
    alg = alg_init(make_parameter(rnn, env=env, cuda_inference=True, **over))
    assert alg.discrete_env and alg.policy.categorical
    logged, add = [], alg.logger.add_tabular_data

    def record(tb_prefix=None, **kw):
        if tb_prefix == 'Train':
            logged.append((kw['EpRet'], kw['EpLength']))
        return add(tb_prefix=tb_prefix, **kw)

    replays, replay = [], GraphedPolicyStep.replay_device
    monkeypatch.setattr(alg.logger, 'add_tabular_data', record)
    monkeypatch.setattr(GraphedPolicyStep, 'replay_device', lambda self: (replays.append(self), replay(self))[1])
    alg.train()
    monkeypatch.setattr(GraphedPolicyStep, 'replay_device', replay)
    torch.cuda.synchronize()
    ring, e = alg.replay_buffer, alg.env
    dev = alg.sample_device
    out = dict(
        ring=_bits(ring.memory_buffer).copy(),
        tables=(list(ring.trajectory_start), list(ring.trajectory_length), ring.ptr, ring.transition_count, len(ring.memory)),
        pending=[_bits(ring.transition_to_array(tr)).tolist() for tr in ring.memory],            # the open episode, as the ring would store it
        logged=[(np.float64(r).view(np.int64).item(), n) for r, n in logged], log_types=sorted({(type(r), type(n)) for r, n in logged}, key=str),
        mirrors=[(a.dtype, a.shape, _bits(a.astype(a.dtype)).tolist()) for a in (alg.state_np, alg.last_state_np, alg.last_action_np, alg.reward_np)],
        env=(e.x, e.y, e.goal_y, e.oracle_visited, e.time_step, type(e.oracle_visited), e._rs.get_state()[1].tolist(), e._rs.get_state()[2]),
        hidden=[t.detach().cpu().numpy().view(np.int32).tolist() for t in alg.graph_step._state_tensors()],
        positions=[(ip.seqlen_offset, ip.device_offset.tolist()) for ip in alg.graph_step._counters()],        # cgpt: one KV cache per layer
        generators=(random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2], torch.get_rng_state().tolist(),
                    torch.cuda.get_rng_state(dev).tolist()),
        counts=(alg.sample_num, alg.grad_num),
        policy=_flat(alg.policy.store).cpu().numpy().view(np.int32), values=[_flat(v.store).cpu().numpy().view(np.int32) for v in alg.values],
        targets=[_flat(v.store).cpu().numpy().view(np.int32) for v in alg.target_values], alpha=alg.log_sac_alpha.detach().cpu().numpy().view(np.int32),
    )
    return alg, out, replays


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (what, k)
        elif isinstance(a[k], list) and a[k] and isinstance(a[k][0], np.ndarray):
            assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _differ(a, b):
    try:
        _assert_same(a, b, '')
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('rfh', [False, True], ids=['rnd-first-hidden', 'zero-first-hidden'])
@pytest.mark.parametrize('rnn', ['gru', 'smamba_s16_c4_b1'])
@pytest.mark.parametrize('env', ['Mem-T-passive-5-v0', 'Mem-T-active-3-v0'])
def test_collector_equals_the_host_loop_with_frozen_parameters(ops, env, rnn, rfh, tmp_path, monkeypatch):
    T, episodes = 6, 3                                          # both environments: six steps an episode
    over = dict(random_num=12, start_train_num=10 ** 9, total_iteration=1, step_per_iteration=episodes * T, test_nprocess=0, test_nrollout=0,
                randomize_first_hidden=rfh)
    host, want, host_replays = _run(monkeypatch, tmp_path, False, rnn, env, **over)
    assert host.collector is None and host.graph_step._graph is not None and not host_replays    # (the host step replays inside `__call__`)
    alg, got, replays = _run(monkeypatch, tmp_path, True, rnn, env, **over)
    c = alg.collector
    assert c is not None and alg.graph_step._graph is None      # one graph only: the B = 1 host step was never captured
    _assert_same(got, want, (env, rnn, rfh))
    assert len(want['logged']) == episodes and [n for _, n in want['logged']] == [T] * episodes
    assert want['tables'][1] == [T] * (2 + episodes) and want['counts'] == (12 + episodes * T, 0)
    # one replay per step and nothing else of the step object; one synchronise per finished episode, one init launch per episode begun
    assert c.replays == episodes * T == len(replays) and all(s is c.step for s in replays)
    assert c.episode_syncs == episodes and c.init_launches == episodes + 1


def test_cgpt_collector_equals_the_host_loop_and_stops_where_it_stops(ops, tmp_path, monkeypatch):
    """A KV cache: the host mirrors of its position follow the replays (40 steps end 4 tokens into an episode), and a cache shorter than
    an episode raises what the host step raises, at the same step."""
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    env = 'Mem-T-passive-5-v0'
    over = dict(random_num=12, start_train_num=10 ** 9, total_iteration=1, step_per_iteration=40, test_nprocess=0, test_nrollout=0)
    _, want, _ = _run(monkeypatch, tmp_path, False, 'cgpt_h1_l2_p0_ml32', env, **over)
    alg, got, _ = _run(monkeypatch, tmp_path, True, 'cgpt_h1_l2_p0_ml32', env, **over)
    _assert_same(got, want, 'cgpt')
    assert alg.collector.replays == 40 and want['positions'] and all(p == (4, [4]) for p in want['positions'])
    stopped = []
    for switch in ('0', '1'):
        monkeypatch.setenv('RESEL_DEVICE_COLLECT', switch)
        short = alg_init(make_parameter('cgpt_h1_l2_p0_ml4', env=env, cuda_inference=True, **over))
        with pytest.raises(RuntimeError, match=r'KV cache is full \(4 tokens, max_seqlen 4\)'):
            short.train()
        assert (short.collector is not None) == (switch == '1')
        stopped.append((short.sample_num, len(short.replay_buffer), short.env.time_step, short.env.x, short.env.y))
    assert stopped[0] == stopped[1] and stopped[0][0] == 12 + 4 and stopped[0][2] == 4


TRAIN = dict(random_num=24, update_interval=3, total_iteration=2, step_per_iteration=20, test_nprocess=1, test_nrollout=2, sac_batch_size=24)


def test_train_without_updates_equals_the_host_loop(ops, tmp_path, monkeypatch):
    """Two iterations of 20 steps on six-step episodes: the evaluation of the second iteration falls inside an episode."""
    over = dict(TRAIN, start_train_num=10 ** 9)
    host, want, _ = _run(monkeypatch, tmp_path, False, 'gru', 'Mem-T-passive-5-v0', **over)
    alg, got, replays = _run(monkeypatch, tmp_path, True, 'gru', 'Mem-T-passive-5-v0', **over)
    assert host.collector is None and alg.collector is not None and host.evaluator is not None and alg.evaluator is not None
    _assert_same(got, want, 'no updates')
    assert want['counts'] == (24 + 40, 0) and want['env'][4] == 40 % 6 and len(want['logged']) == 40 // 6
    c = alg.collector
    assert c.replays == 40 and c.episode_syncs == 6 and c.init_launches == 7
    assert sum(s is c.step for s in replays) == 40              # the rest are the evaluator's


@pytest.mark.parametrize('interval', [3, 5], ids=['updates-inside-episodes', 'updates-on-last-steps'])
@pytest.mark.parametrize('graph_update', [None, '0'], ids=['graphed-updates', 'eager-updates'])
def test_train_with_updates_equals_the_host_loop(ops, graph_update, interval, tmp_path, monkeypatch):
    """Updates from step 24 on, every `interval` steps: 3 puts them inside episodes, 5 also on an episode's last step (step 35), where the
    update must find the episode in the ring.  The host loop runs twice as a control; the device path must equal it when the control agrees."""
    over = dict(TRAIN, start_train_num=24, update_interval=interval)
    env = 'Mem-T-passive-5-v0'
    _, first, _ = _run(monkeypatch, tmp_path, False, 'gru', env, graph_update, **over)
    _, second, _ = _run(monkeypatch, tmp_path, False, 'gru', env, graph_update, **over)
    assert first['counts'][1] == len([s for s in range(24, 64) if s % interval == 0])
    if _differ(first, second):
        pytest.skip(HOST_RUNS_DIFFER)
    alg, got, _ = _run(monkeypatch, tmp_path, True, 'gru', env, graph_update, **over)
    assert alg.collector is not None and alg.collector.replays == 40
    _assert_same(got, first, ('updates', graph_update, interval))


# ------------------------------------------------------------------------------------------------ 4. fall-backs
@pytest.mark.parametrize('env,switch', [('Mem-T-passive-5-cont-act-v0', '1'), ('synthetic-o2-d4-T6', '1'), ('Mem-T-passive-5-v0', '0')])
def test_fallbacks_take_the_host_loop_and_say_why_once(ops, env, switch, tmp_path, monkeypatch):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.utility import device_collect
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('RESEL_DEVICE_COLLECT', switch)

    def never(self, alg):
        raise AssertionError('the collector must not be built')

    monkeypatch.setattr(device_collect.DeviceCollector, '__init__', never)
    alg = alg_init(make_parameter('gru', env=env, cuda_inference=True, random_num=12, start_train_num=10 ** 9, total_iteration=1,
                                  step_per_iteration=8, test_nprocess=0, test_nrollout=0))
    assert alg.discrete_env == ('cont-act' not in env)
    said, call = [], type(alg.logger).__call__
    monkeypatch.setattr(type(alg.logger), '__call__', lambda self, *a, **k: (said.append(' '.join(map(str, a))), call(self, *a, **k))[1])
    alg.train()
    alg.train()
    why = [s for s in said if 'collected through the host loop' in s]
    assert len(why) == 1 and alg.collector is None and alg.graph_step._graph is not None
    assert ('RESEL_DEVICE_COLLECT=0' in why[0]) == (switch == '0') and ('no device step' in why[0]) == (switch == '1')
    assert alg.sample_num == 2 * (12 + 8) and len(alg.replay_buffer) >= 4
