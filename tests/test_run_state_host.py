"""Run states (algorithm/run_state.py, `SAC.save_state` / `load_state`, RESEL_CHECKPOINT_DIR) on the host: the ring's round trip, the
directory protocol, the fingerprint, the environment objects, and whole `train()` runs on the CPU oracle - uninterrupted without and
with checkpoints, and resumed from the middle - which must end in the same state bit for bit.  `snapshot` (everything two trainers
must agree on, as integer views) is shared with tests/test_run_state_gpu.py."""
import os
import pickle
import random
import shutil

import numpy as np
import pytest
import torch

from offpolicy_rnn.algorithm import run_state
from offpolicy_rnn.buffers.transition_buffer.nested_replay_memory import NestedMemoryArray
from offpolicy_rnn.buffers.transition_buffer.replay_memory import MemoryArray, Transition
from offpolicy_rnn.env_utils.make_env import make_env


def bits(a):
    """Integer view of an array / tensor / scalar: -0.0 and NaN payloads count."""
    if torch.is_tensor(a):
        a = a.detach().cpu()
        if a.dtype == torch.bfloat16:
            return a.contiguous().view(torch.int16).numpy()
        a = a.numpy()
    a = np.ascontiguousarray(a)
    if a.dtype.kind == 'f':
        return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return a


def plain(obj, depth=0):
    """Any host object as nested tuples of comparable things: arrays as (dtype, shape, bits), random streams as their state."""
    assert depth < 8
    if isinstance(obj, np.random.RandomState):
        s = obj.get_state()
        return ('RandomState', s[1].tolist(), s[2], s[3], np.float64(s[4]).view(np.int64).item())
    if isinstance(obj, np.ndarray):
        return ('ndarray', str(obj.dtype), obj.shape, bits(obj).tolist())
    if isinstance(obj, (float, np.floating)):
        return (type(obj).__name__, np.float64(obj).view(np.int64).item())
    if isinstance(obj, (bool, int, str, type(None), np.integer, np.bool_, range)):
        return (type(obj).__name__, obj)
    if isinstance(obj, (list, tuple)):
        return (type(obj).__name__, tuple(plain(v, depth + 1) for v in obj))
    if isinstance(obj, dict):
        return ('dict', tuple((k, plain(v, depth + 1)) for k, v in sorted(obj.items())))
    return (type(obj).__name__, tuple((k, plain(v, depth + 1)) for k, v in sorted(vars(obj).items())))


def hidden_snapshot(hidden):
    """Per layer: tensors by bits; a KV cache by its position and the entries up to it (what lies behind is never read)."""
    out = []
    for h in ([] if hidden is None else hidden._data):
        if torch.is_tensor(h):
            out.append(bits(h).reshape(-1).tolist())
        elif isinstance(h, tuple):
            out.append([bits(t).reshape(-1).tolist() for t in h])
        else:
            pos = int(h.seqlen_offset)
            dev = None if h.device_offset is None else h.device_offset.tolist()
            out.append((pos, dev, sorted((k, bits(v[:, :pos]).reshape(-1).tolist()) for k, v in h.key_value_memory_dict.items())))
    return out


def snapshot(alg):
    """Everything a trainer that continues a run must share with the one that was never stopped."""
    dev = alg.sample_device
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    ring = alg.replay_buffer
    hi = run_state.occupied_rows(ring)
    ev = alg.evaluator
    subset = getattr(alg, '_subset_rng', None)
    alpha_state = alg.optimizer_alpha.state_dict()['state']
    return dict(
        ring=bits(ring.memory_buffer[:hi]).copy(), ring_shape=ring.memory_buffer.shape,
        tables=(list(ring.trajectory_start), list(ring.trajectory_length), ring.ptr, ring.transition_count, len(ring.memory)),
        layout=(ring.width, sorted(ring.name2range.items())),
        pending=[bits(ring.transition_to_array(tr)).tolist() for tr in ring.memory], pending_types=[plain(tuple(tr)) for tr in ring.memory],
        mirrors=[plain(a) for a in (alg.state_np, alg.last_state_np, alg.last_action_np, alg.reward_np)],
        env=plain(alg.env), episode=(plain(alg.ep_ret), alg.ep_len),
        hidden=hidden_snapshot(alg.graph_step._hidden if alg.graph_step is not None else alg.sample_hidden),
        generators=(random.getstate(), plain(np.random.get_state()), torch.get_rng_state().tolist(),
                    torch.cuda.get_rng_state(dev).tolist() if dev.type == 'cuda' else None),
        subset_rng=None if subset is None else plain(subset),
        counts=(alg.sample_num, alg.grad_num, alg.iteration),
        networks={name: bits(net.store.flat) for name, net in alg._state_networks().items()},
        alpha=bits(alg.log_sac_alpha), alpha_optimizer=sorted((k, sorted((n, bits(torch.as_tensor(v)).tolist()) for n, v in st.items())) for k, st in alpha_state.items()),
        moments={name: (bits(opt.m), bits(opt.v), opt.step_count) for name, opt in alg._state_optimizers().items()},
        q_guard=bits(alg.Q_guard.state).tolist(),
        evaluator=None if ev is None else (plain(ev.rs), list(ev.env_seeds), [plain(e) for e in ev.envs]),
    )


def assert_same(a, b, what=''):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and np.array_equal(x, y), (what, k)
        elif isinstance(x, dict):
            assert x.keys() == y.keys(), (what, k)
            for n in x:
                xs, ys = (x[n], y[n]) if isinstance(x[n], tuple) else ((x[n],), (y[n],))
                assert len(xs) == len(ys) and all(np.array_equal(p, q) for p, q in zip(xs, ys)), (what, k, n)
        else:
            assert x == y, (what, k)


def differ(a, b):
    try:
        assert_same(a, b)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------ the ring
def _transition(rs, t, n, done):
    return Transition(state=rs.randn(1, 3), last_state=rs.randn(1, 3), last_action=rs.randn(1, 2), action=rs.randn(1, 2).astype(np.float32),
                      next_state=rs.randn(1, 3), reward=float(rs.randn()), logp=None, mask=1, done=done, timeout=t + 1 >= n, start=t == 0,
                      reward_input=rs.randn(1, 1))


def _filled_ring(cls=MemoryArray, capacity=40, lengths=(9, 7, 11, 8, 10, 6, 9), partial=4, **kw):
    ring = cls(capacity, 12, **kw)
    rs = np.random.RandomState(3)
    for n in lengths:
        for t in range(n):
            ring.mem_push(_transition(rs, t, n, t == n - 1))
    for t in range(partial):
        ring.mem_push(_transition(rs, t, 12, False))
    return ring


def _ring_view(ring):
    hi = run_state.occupied_rows(ring)
    live = np.concatenate([np.arange(s, s + n) for s, n in zip(ring.trajectory_start, ring.trajectory_length)])
    return dict(rows=bits(ring.memory_buffer[:hi]).copy(), live=bits(ring.memory_buffer[live]).copy(), shape=ring.memory_buffer.shape,
                tables=(list(ring.trajectory_start), list(ring.trajectory_length), ring.ptr, ring.transition_count),
                layout=(ring.width, sorted(ring.name2range.items())), pending=[plain(tuple(tr)) for tr in ring.memory],
                types=(type(ring.ptr), type(ring.transition_count), {type(v) for v in ring.trajectory_start + ring.trajectory_length}))


@pytest.mark.parametrize('cls', [MemoryArray, NestedMemoryArray])
def test_ring_round_trip_after_eviction_and_wrap(cls, tmp_path):
    ring = _filled_ring(cls)
    # 60 transitions into 40: trajectories were evicted, `ptr` went back to row 0 once, and rows behind the furthest table entry are stale
    assert ring.transition_count <= 40 < 60 and len(ring) < 7 and 0 < ring.ptr < max(ring.trajectory_start) and len(ring.memory) == 4
    ring._dev_state = {'buf': object()}                          # what a device mirror leaves on the object: must not travel, must not survive
    path = str(tmp_path / 'ring.npz')
    run_state.save_ring(ring, path)
    want = _ring_view(ring)
    fresh = cls(40, 12)
    fresh._dev_state = {'buf': object()}
    fresh._dirty = [(0, 5)]
    run_state.load_ring(fresh, run_state.read_ring(path), pickle.loads(pickle.dumps(ring.memory)))
    got = _ring_view(fresh)
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]) if isinstance(want[k], np.ndarray) else got[k] == want[k], k
    assert '_dev_state' not in fresh.__dict__ and fresh._dirty == []          # the device mirror is rebuilt from the loaded block
    # the loaded ring goes on like the original: the same eviction, the same rows
    rs_a, rs_b = np.random.RandomState(5), np.random.RandomState(5)
    for r, rs in ((ring, rs_a), (fresh, rs_b)):
        for t in range(4, 12):
            r.mem_push(_transition(rs, t, 12, t == 11))
    a, b = _ring_view(ring), _ring_view(fresh)
    assert a['tables'] == b['tables'] and np.array_equal(a['live'], b['live']) and not ring.memory and not fresh.memory


def test_ring_file_scales_with_occupancy_not_capacity(tmp_path):
    sizes = {}
    for capacity, lengths in ((4000, (10,) * 3), (4000, (10,) * 30), (400000, (10,) * 30)):
        ring = _filled_ring(capacity=capacity, lengths=lengths, partial=0)
        assert ring.memory_buffer.shape[0] == capacity + 12
        path = str(tmp_path / f'ring-{capacity}-{len(lengths)}.npz')
        run_state.save_ring(ring, path)
        sizes[capacity, len(lengths)] = os.path.getsize(path)
        assert run_state.read_ring(path)['rows'].shape == (10 * len(lengths), ring.width)
    row_bytes = 4 * 19                                          # 3 + 3 + 2 + 2 + 3 + 1 + 0 + 1 + 1 + 1 + 1 + 1 columns of fp32
    assert sizes[4000, 30] - sizes[4000, 3] == 270 * row_bytes + 27 * 16      # 27 more trajectories of 10 rows: their bytes, two int64 table entries each
    assert sizes[400000, 30] == sizes[4000, 30] < 300 * row_bytes + 4096      # a hundred times the capacity: the same file


def test_empty_ring_round_trip(tmp_path):
    ring = MemoryArray(40, 12)
    path = str(tmp_path / 'ring.npz')
    run_state.save_ring(ring, path)
    fresh = _filled_ring()
    run_state.load_ring(fresh, run_state.read_ring(path))
    assert fresh.memory_buffer is None and fresh.name2range == {} and len(fresh) == 0 and fresh.ptr == 0 and fresh.memory == []


# ------------------------------------------------------------------------------------------------ the directory protocol
def _write(directory, iterations, fingerprint=None, mark=0):
    ring = _filled_ring(lengths=(5,), partial=0)
    return run_state.write_checkpoint(str(directory), iterations, lambda path: run_state.write_state(
        path, dict(iteration=iterations, fingerprint=fingerprint or {}), ring, dict(mark=mark), dict(t=torch.arange(3))))


def test_directory_protocol(tmp_path):
    d = tmp_path / 'ckpt'
    assert run_state.newest_state(str(d)) is None and run_state.complete_states(str(d)) == []          # no directory at all
    d.mkdir()
    (d / 'state-000009').mkdir()                                # a state that was never finished: payload, no manifest
    (d / 'state-000009' / run_state.HOST).write_bytes(b'partial')
    (d / 'tmp-12345').mkdir()                                   # a writer that died before its rename
    (d / 'notes.txt').write_text('not ours')
    assert run_state.newest_state(str(d)) is None               # ignored on resume
    _write(d, 2, mark=2)
    assert sorted(os.listdir(d)) == ['notes.txt', 'state-000002']             # ... and cleaned by the next successful write
    assert sorted(os.listdir(d / 'state-000002')) == sorted([run_state.MANIFEST, run_state.RING, run_state.HOST, run_state.TENSORS])
    _write(d, 4, mark=4)
    _write(d, 6, mark=6)
    _write(d, 12, mark=12)
    assert sorted(os.listdir(d)) == ['notes.txt', 'state-000006', 'state-000012']                      # only two are kept
    assert run_state.newest_state(str(d)) == (12, str(d / 'state-000012'))                             # the newest complete state wins
    os.remove(d / 'state-000012' / run_state.MANIFEST)
    assert run_state.newest_state(str(d)) == (6, str(d / 'state-000006'))
    manifest, ring_st, host, tensors = run_state.read_state(str(d / 'state-000006'))
    assert manifest['iteration'] == 6 and manifest['format_version'] == run_state.FORMAT_VERSION and host == dict(mark=6)
    assert tensors['t'].tolist() == [0, 1, 2] and ring_st['rows'].shape == (5, 19)
    with pytest.raises(FileNotFoundError, match='no complete run state'):
        run_state.read_state(str(d / 'state-000012'))
    _write(d, 6, mark=66)                                       # the same name again: replaced whole, the broken one is gone
    assert sorted(os.listdir(d)) == ['notes.txt', 'state-000006'] and run_state.read_state(str(d / 'state-000006'))[2] == dict(mark=66)
    (d / 'state-000020').mkdir()
    (d / 'state-000020' / run_state.MANIFEST).write_text('{"format_version": 999}')                    # another format: not a state of this one
    assert run_state.newest_state(str(d)) == (6, str(d / 'state-000006'))


@pytest.mark.parametrize('raw,want', [(None, 25), ('1', 1), ('40', 40), ('0', None), ('-3', None), ('2.5', None), ('often', None), ('', None)])
def test_checkpoint_every_switch(raw, want, monkeypatch):
    if raw is None:
        monkeypatch.delenv('RESEL_CHECKPOINT_EVERY', raising=False)
    else:
        monkeypatch.setenv('RESEL_CHECKPOINT_EVERY', raw)
    if want is None:
        with pytest.raises(ValueError, match='RESEL_CHECKPOINT_EVERY'):
            run_state.checkpoint_every_from_env()
    else:
        assert run_state.checkpoint_every_from_env() == want


def test_fingerprint_names_the_field():
    saved = dict(env_name='Wind-v0', seed=1, policy_embedding_layer_type=['fc', 'gru', 'fc'], ring_width=17, ring_name2range={'state': (0, 2)})
    run_state.check_fingerprint(saved, dict(saved))
    run_state.check_fingerprint(saved, dict(saved, ring_width=None, ring_name2range=None))             # a fresh ring has no layout to compare
    for field, other in (('env_name', 'Mem-T-passive-5-v0'), ('seed', 2), ('policy_embedding_layer_type', ['fc', 'gilr', 'fc']), ('ring_width', 18),
                         ('ring_name2range', {'state': (0, 3)})):
        with pytest.raises(run_state.RunStateMismatch, match=field) as e:
            run_state.check_fingerprint(saved, dict(saved, **{field: other}))
        assert e.value.field == field
    with pytest.raises(run_state.RunStateMismatch, match='act_dim'):
        run_state.check_fingerprint(saved, dict(saved, act_dim=3))                                     # a field the state does not hold at all


# ------------------------------------------------------------------------------------------------ environment objects
def _roll(env, actions, reset_arg):
    out = [plain(env.step(a)) for a in actions]
    out.append(plain(env.reset(*reset_arg)))
    out.append(plain(env.action_space.sample()))
    out.append(plain(env))
    return out


@pytest.mark.parametrize('name', ['Mem-T-active-3-v0', 'Wind-v0', 'synthetic-o5-a3-T12'])
def test_environment_objects_round_trip(name):
    env = make_env(name, 11)['train_env']
    env.seed(16)
    env.action_space.seed(17)
    rs = np.random.RandomState(2)
    if name.startswith('Mem-T'):
        for _ in range(4):                                       # goal draws from the private stream
            env.reset()
        assert env.goal_y in (-1, 1)
        env.step(2)                                              # onto the oracle: the goal side has been shown
        env.step(0)
        assert env.oracle_visited and env.time_step == 2
        actions, reset_arg = [int(rs.randint(4)) for _ in range(10)], ()
    elif name == 'Wind-v0':
        env.reset(7)                                             # a task that is not the first
        for _ in range(5):
            env.step(rs.uniform(-1, 1, 2))
        assert env.step_count == 5 and env._wind.tolist() == env.winds[7] and env.winds[7] != env.winds[0]
        actions, reset_arg = [rs.uniform(-1.5, 1.5, 2) for _ in range(10)], (3,)
    else:
        env.reset()
        for _ in range(5):
            env.step(env.action_space.sample())
        actions, reset_arg = [rs.uniform(-1, 1, 3) for _ in range(10)], ()
    twin = pickle.loads(pickle.dumps(env, protocol=4))
    assert twin is not env and plain(twin) == plain(env)
    assert _roll(twin, actions, reset_arg) == _roll(env, actions, reset_arg)


# ------------------------------------------------------------------------------------------------ whole runs on the CPU oracle
RUN = dict(total_iteration=4, step_per_iteration=20, random_num=24, start_train_num=24, update_interval=3, sac_batch_size=24, test_nprocess=0)
CASES = {'gru-tmaze': dict(rnn='gru', env='Mem-T-passive-5-v0'), 'gru-wind': dict(rnn='gru', env='Wind-v0'),
         'gru-td3-synthetic': dict(rnn='gru', env='synthetic-o5-a3-T12', algo='td3')}


def _train(monkeypatch, ckpt_dir, case, every=2, **over):
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    if ckpt_dir is None:
        monkeypatch.delenv('RESEL_CHECKPOINT_DIR', raising=False)
    else:
        monkeypatch.setenv('RESEL_CHECKPOINT_DIR', str(ckpt_dir))
    monkeypatch.setenv('RESEL_CHECKPOINT_EVERY', str(every))
    alg = alg_init(make_parameter(**dict(RUN, **CASES[case], **over)))
    said, call = [], type(alg.logger).__call__
    monkeypatch.setattr(type(alg.logger), '__call__', lambda self, *a, **k: (said.append(' '.join(map(str, a))), call(self, *a, **k))[1])
    alg.train()
    monkeypatch.setattr(type(alg.logger), '__call__', call)
    return alg, snapshot(alg), said


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize('case', list(CASES))
def test_a_resumed_run_is_the_uninterrupted_run(case, oracle_ops, tmp_path, monkeypatch):
    """(a) no checkpoint directory, (b) a state every 2 iterations, (c) a fresh trainer that finds only `state-000002`: three equal ends."""
    monkeypatch.setenv('RESEL_LOG_DIR', str(tmp_path / 'logs-a'))
    monkeypatch.chdir(tmp_path)
    plain_alg, want, said = _train(monkeypatch, None, case)
    warm = 75 if case == 'gru-wind' else 24                      # the warm-up ends with an episode: Wind's have 75 steps
    assert want['counts'] == (warm + 80, len([s for s in range(warm, warm + 80) if s % 3 == 0]), 4)
    assert not any('run state' in s for s in said)
    assert all(f.startswith('logs-a' + os.sep) for f in _files(tmp_path)), _files(tmp_path)            # (a) wrote its log folder and nothing else
    assert not any('state-' in f or 'tmp-' in f for f in _files(tmp_path))
    assert want['tables'][4] > 0 or case != 'gru-tmaze'         # six-step episodes: 80 steps end inside one
    b_dir = tmp_path / 'ckpt-b'
    _, with_states, said = _train(monkeypatch, b_dir, case)
    assert_same(with_states, want, 'writing states perturbs nothing')
    assert sorted(os.listdir(b_dir)) == ['state-000002', 'state-000004'] and sum('no run state in' in s for s in said) == 1
    c_dir = tmp_path / 'ckpt-c'
    c_dir.mkdir()
    shutil.copytree(b_dir / 'state-000002', c_dir / 'state-000002')
    resumed, got, said = _train(monkeypatch, c_dir, case)
    assert sum('resumed the run state' in s for s in said) == 1 and 'state-000002' in [s for s in said if 'resumed' in s][0]
    assert_same(got, want, 'resumed from iteration 2')
    assert sorted(os.listdir(c_dir)) == ['state-000002', 'state-000004']
    # the state the resumed run wrote at the end is the state the uninterrupted run wrote there
    mb, rb, hb, tb = run_state.read_state(str(b_dir / 'state-000004'))
    mc, rc, hc, tc = run_state.read_state(str(c_dir / 'state-000004'))
    assert mb == mc and all(np.array_equal(rb[k], rc[k]) for k in rb) and torch.equal(tb['stores']['policy'], tc['stores']['policy'])
    # a run that is complete resumes to nothing: no step, no update
    again, end, _ = _train(monkeypatch, c_dir, case)
    assert_same(end, want, 'resumed at the end')


def test_states_follow_the_cadence_and_hold_the_open_episode(oracle_ops, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    d = tmp_path / 'ckpt'
    alg, _, _ = _train(monkeypatch, d, 'gru-tmaze', every=2, total_iteration=5)
    assert sorted(os.listdir(d)) == ['state-000002', 'state-000004'] and alg.iteration == 5
    manifest, ring_st, host, tensors = run_state.read_state(str(d / 'state-000002'))
    assert manifest['iteration'] == 2 and manifest['sample_num'] == 24 + 40 == host['sample_num']
    assert host['ep_len'] == 40 % 6 == len(host['pending'])      # six-step episodes: the state was taken four steps into one
    assert ring_st['rows'].shape[0] == sum(ring_st['trajectory_length']) < alg.replay_buffer.memory_buffer.shape[0]
    assert set(tensors['stores']) == {'policy', 'value0', 'target_value0', 'target_policy'} and set(tensors['moments']) == {'policy', 'value0'}
    monkeypatch.setenv('RESEL_CHECKPOINT_EVERY', 'weekly')
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    bad = alg_init(make_parameter(**dict(RUN, **CASES['gru-tmaze'])))
    with pytest.raises(ValueError, match='RESEL_CHECKPOINT_EVERY'):
        bad.train()
    assert bad.sample_num == 0                                  # refused before anything ran


def test_a_mismatch_names_the_field_and_leaves_the_trainer_alone(oracle_ops, tmp_path, monkeypatch):
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    short = dict(RUN, total_iteration=1)
    writer, _, _ = _train(monkeypatch, None, 'gru-tmaze', total_iteration=1)
    path = writer.save_state(str(tmp_path / 'one' / 'state'))
    assert os.path.isdir(path) and not [n for n in os.listdir(tmp_path / 'one') if n.startswith('tmp-')]
    for field, over in (('policy_embedding_layer_type', dict(rnn='gilr')), ('env_name', dict(env='Mem-T-passive-7-v0')), ('seed', dict(seed=5)),
                        ('alg_name', dict(alg_name='sac_rnn_full_horizon_redQ')), ('policy_embedding_hidden_size', dict(D=16))):
        other = alg_init(make_parameter(**dict(short, **dict(CASES['gru-tmaze'], **over))))
        before = snapshot_of_fresh(other)
        with pytest.raises(run_state.RunStateMismatch, match=field) as e:
            other.load_state(path)
        assert e.value.field == field
        assert_same(snapshot_of_fresh(other), before, field)
    # a trainer that has trained and holds a ring of its own is untouched as well
    other, before, _ = _train(monkeypatch, None, 'gru-tmaze', total_iteration=1, seed=5)
    with pytest.raises(run_state.RunStateMismatch, match='seed'):
        other.load_state(path)
    assert_same(snapshot(other), before, 'trained trainer')
    same = alg_init(make_parameter(**dict(short, **CASES['gru-tmaze'])))
    same.load_state(path)
    assert_same(snapshot(same), snapshot(writer), 'round trip')


def snapshot_of_fresh(alg):
    """`snapshot` of a trainer whose ring has no block yet."""
    ring = alg.replay_buffer
    assert ring.memory_buffer is None
    ring.memory_buffer, ring.width = np.zeros((0, 0), dtype=np.float32), 0
    try:
        return snapshot(alg)
    finally:
        ring.memory_buffer = None
        del ring.width


def test_more_than_one_rank_is_refused(oracle_ops, tmp_path, monkeypatch):
    import torch.distributed as dist
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    alg = alg_init(make_parameter(**dict(RUN, **CASES['gru-tmaze'])))
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    for call in (lambda: alg.save_state(str(tmp_path / 's')), lambda: alg.load_state(str(tmp_path / 's'))):
        with pytest.raises(NotImplementedError, match='process group of 2 ranks'):
            call()
    monkeypatch.setenv('RESEL_CHECKPOINT_DIR', str(tmp_path / 'ckpt'))
    with pytest.raises(NotImplementedError, match='single process'):
        alg.train()
    assert alg.sample_num == 0 and not os.path.exists(tmp_path / 's') and not os.path.exists(tmp_path / 'ckpt')
