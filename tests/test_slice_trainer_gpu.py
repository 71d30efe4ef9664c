"""The slice trainer `sac_rnn_slice` on cuda:0: the slice gather against its host spelling, three updates of every recording of the
reference, the families without a recording against the same trainer on the CPU path, replayed against eagerly launched updates,
`train()` on a synthetic environment and on a T-Maze, and a run state.  Host side: tests/test_slice_trainer_host.py."""
import os

import numpy as np
import pytest
import torch

from test_mlp_redq_host import feed_draws, val, wrapped_ring
from test_slice_trainer_host import RECS, check_against_recording, fill_slice_ring, golden_trainer, host_window, slice_parameter

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')


@pytest.fixture(scope='module')
def ops():
    from offpolicy_rnn.hip import ops
    return ops


DEV = torch.device('cuda', 0)


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int32 if a.dtype.itemsize == 4 else np.int64).copy()


# ------------------------------------------------------------------------------------------------ 1. the gather
@pytest.mark.parametrize('L,n', [(2, 13), (4, 37), (7, 37), (7, 13), (12, 13)])
def test_gather_slices_is_bit_equal_to_the_host_window(ops, L, n):
    """The wrapped, twice-evicted 27-column ring: 27 (L + 1) floats per slice are no multiple of the 256 threads of a block, and at
    L = 12 (351 floats) a slice takes two blocks; batches 13 and 37; three passes, each selected by argument and by the device pass
    word; `c_timeout = -1` leaves `done` as stored; some drawn row did time out and some slice is padded."""
    from offpolicy_rnn.algorithm.sac_rnn_slice import host_slice_batch, pre_step_pairs
    ring = wrapped_ring()
    R = ring.name2range
    c_done, c_timeout = R['done'][0], R['timeout'][0]
    passes = 3
    np.random.seed(5)
    plan = ring.plan_slices(n, L, passes)
    np.random.seed(5)
    want = [ring.sample_fix_length_sub_trajs(n, L) for _ in range(passes)]
    mirror = ring._mirror(DEV)
    plan_dev = torch.from_numpy(plan).to(DEV)
    pairs = pre_step_pairs(R, False)
    pairs_dev = torch.from_numpy(pairs).to(DEV)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    fixed = padded = 0
    for p in range(passes):
        window = host_window(ring, plan[p], L)
        stored = np.concatenate([f for f in want[p] if f is not None], axis=-1)
        fix = stored.copy()
        fix[..., c_done][stored[..., c_timeout] > 0] = 0
        assert np.array_equal(window[:, 1:], fix)                  # the host window's batch IS `sample_fix_length_sub_trajs` + the done fix
        fixed += int((fix != stored).sum())
        padded += int((want[p].mask == 0).sum())
        word.fill_(p)
        for got in (ops.gather_slices(mirror, plan_dev, L, pairs_dev, None, p, c_done, c_timeout),
                    ops.gather_slices(mirror, plan_dev, L, pairs_dev, word, 0, c_done, c_timeout)):
            assert got.shape == (n, L + 1, 27)
            assert np.array_equal(_bits(got), window.view(np.int32)), p
        raw = ops.gather_slices(mirror, plan_dev, L, pairs_dev, None, p, c_done, -1)
        assert np.array_equal(_bits(raw), host_slice_batch(ring, plan[p], L, pairs, c_done, -1).view(np.int32)), p
        assert np.array_equal(_bits(raw[:, 1:]), stored.view(np.int32)), p
    assert fixed > 0 and padded > 0


def test_gather_slices_edge_entries(ops):
    """A trajectory shorter than L, the last transition of a trajectory (n = 1), every kind of bad plan entry and an out-of-table pass
    word (zero slices, their neighbours intact), an out-of-range pass argument (an error)."""
    from offpolicy_rnn.algorithm.sac_rnn_slice import pre_step_pairs
    ring = wrapped_ring()
    R = ring.name2range
    c_done, c_timeout = R['done'][0], R['timeout'][0]
    L = 7
    starts, lens = np.asarray(ring.trajectory_start), np.asarray(ring.trajectory_length)
    short = int(np.flatnonzero(lens < L)[0])
    long_ = int(np.flatnonzero(lens >= L)[0])
    cap = len(ring.memory_buffer)
    good = [(starts[short], lens[short]),                          # a whole trajectory shorter than L
            (starts[long_] + lens[long_] - 1, 1),                  # the last transition of a trajectory
            (starts[long_], L), (starts[long_] + 2, min(L, lens[long_] - 2))]
    bad = [(-1, 3), (starts[long_], 0), (starts[long_], -2), (starts[long_], L + 1), (cap - 2, 3), (cap, 1)]
    order = [good[0], bad[0], good[1], bad[1], bad[2], good[2], bad[3], bad[4], good[3], bad[5]]
    plan = np.asarray(order, dtype=np.int32).reshape(1, len(order), 2)
    is_good = [e in good for e in order]
    mirror = ring._mirror(DEV)
    pairs_dev = torch.from_numpy(pre_step_pairs(R, False)).to(DEV)
    got = ops.gather_slices(mirror, torch.from_numpy(plan).to(DEV), L, pairs_dev, None, 0, c_done, c_timeout).cpu().numpy()
    want = host_window(ring, plan[0][is_good], L)
    k = 0
    for i, ok in enumerate(is_good):
        if ok:
            assert np.array_equal(got[i].view(np.int32), want[k].view(np.int32)), i
            assert got[i, 1].any() and not got[i, 1 + plan[0, i, 1]:].any()
            k += 1
        else:
            assert not got[i].any(), i
    word = torch.full((1,), 1, dtype=torch.int32, device=DEV)      # a pass word outside the table: zero slices, nothing read
    assert not ops.gather_slices(mirror, torch.from_numpy(plan).to(DEV), L, pairs_dev, word, 0, c_done, c_timeout).cpu().numpy().any()
    word.fill_(-1)
    assert not ops.gather_slices(mirror, torch.from_numpy(plan).to(DEV), L, pairs_dev, word, 0, c_done, c_timeout).cpu().numpy().any()
    with pytest.raises(RuntimeError):
        ops.gather_slices(mirror, torch.from_numpy(plan).to(DEV), L, pairs_dev, None, 1, c_done, c_timeout)


# ------------------------------------------------------------------------------------------------ 2. against the reference
@pytest.mark.parametrize('rec', RECS)
def test_three_eager_updates_equal_the_reference_recording(ops, monkeypatch, rec):
    """Initial networks and ring of the recording, its Gaussian draws through utility/rng.py, three eager updates on cuda:0 (plan + gather,
    the HIP ops): logs within 2e-3 / 5e-4, every parameter element within 1e-3 / 2e-5 (tests/test_trainer_gpu.py,
    `test_mlp_redq_host.check_against_recording`)."""
    alg, g, m = golden_trainer(rec, cuda_inference=True)
    assert alg.device.type == 'cuda'
    fed = feed_draws(monkeypatch, g, rec, m['draws'])
    torch.manual_seed(200)
    np.random.seed(200)
    logs = [dict(alg.train_one_batch()) for _ in range(3)]
    assert fed['k'] == m['draws']
    for it, log in enumerate(logs):
        print(rec, it, {k: val(v) for k, v in log.items()})
    check_against_recording(alg, g, rec, logs, m, 2e-3, 5e-4, 1e-3, 2e-5)


# ------------------------------------------------------------------------------------------------ 3. families without a recording
def _unrecorded(rnn):
    from offpolicy_rnn import alg_init
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(slice_parameter(rnn, L=5, cuda_inference=True))
    fill_slice_ring(alg.replay_buffer)
    return alg


@pytest.mark.parametrize('rnn', ['gilr_lstm', 'conv1d_4', 'mamba_s8_c3'])
def test_two_updates_equal_the_cpu_path(ops, monkeypatch, rnn):
    """B = 8, L = 5, obs 5 / act 3, D = 32: two updates on cuda:0 against the same trainer on the CPU path (the host window, the CPU
    oracle's layers, the torch spelling of target and losses) from identical weights, ring and draws, at the bars of the recordings."""
    import oracle_backend
    from offpolicy_rnn.algorithm.sac import SAC
    from offpolicy_rnn.utility import rng
    block = torch.randn(4096, generator=torch.Generator().manual_seed(7))
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: block[:int(np.prod(shape))].view(tuple(shape)).to(dtype).to(device))
    gpu_alg = _unrecorded(rnn)
    assert gpu_alg.device.type == 'cuda'
    nets = lambda a: dict(a._state_networks())
    start = {k: {mod: {kk: t.detach().cpu().clone() for kk, t in d.items()} for mod, d in n.state_dict().items()} for k, n in nets(gpu_alg).items()}
    np.random.seed(11)
    logs_gpu = [dict(gpu_alg.train_one_batch()) for _ in range(2)]
    torch.cuda.synchronize()
    # the same trainer on the CPU: the op table of the oracle, the device pinned to the host
    oracle_backend.install(monkeypatch)
    monkeypatch.setattr(SAC, '_pick_device', staticmethod(lambda: torch.device('cpu')))
    cpu_alg = _unrecorded(rnn)
    assert cpu_alg.device.type == 'cpu'
    for k, n in nets(cpu_alg).items():
        n.load_state_dict(start[k])
    np.random.seed(11)
    logs_cpu = [dict(cpu_alg.train_one_batch()) for _ in range(2)]
    for it, (lg, lc) in enumerate(zip(logs_gpu, logs_cpu)):
        print(rnn, it, {k: (val(lg[k]), val(lc[k])) for k in lc})
        assert set(lg) == set(lc) and len(lc) == 8
        for k, v in lc.items():
            assert val(lg[k]) == pytest.approx(val(v), rel=2e-3, abs=5e-4), (it, k, val(lg[k]), val(v))
    moved = 0
    for k, n in nets(cpu_alg).items():
        sd_gpu = nets(gpu_alg)[k].state_dict()
        for mod, d in n.state_dict().items():
            for kk, t in d.items():
                np.testing.assert_allclose(sd_gpu[mod][kk].detach().cpu().numpy(), t.detach().numpy(), rtol=1e-3, atol=2e-5, err_msg=f'{k}|{mod}.{kk}')
                moved += int(not torch.equal(t.detach(), start[k][mod][kk]))
    assert moved > 0
    np.testing.assert_allclose(gpu_alg.log_sac_alpha.detach().cpu(), cpu_alg.log_sac_alpha.detach(), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 4. replayed against eager
def _state(alg):
    return [n.store.flat.detach().clone() for n in alg._state_networks().values()] + [alg.log_sac_alpha.detach().clone()]


def _fresh(rnn, n_actions, **over):
    from offpolicy_rnn import alg_init
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(slice_parameter(rnn, L=4, n_actions=n_actions, cuda_inference=True, sac_batch_size=13, **over))
    fill_slice_ring(alg.replay_buffer, n_actions)
    np.random.seed(11)
    return alg


@pytest.mark.parametrize('rnn,n_actions', [('gru', 0), ('smamba_s8_c3_b2_nln', 0), ('gru', 4)], ids=['gru', 'smamba', 'gru-discrete'])
def test_replayed_update_equals_the_eager_update(ops, monkeypatch, rnn, n_actions):
    """utd = 3, policy_utd = 1: same start, same numpy seed, the same Gaussian numbers for every draw (a fixed device block): three steps
    through `GraphedTransitionUpdate` with `warmup = 0` - one eager pass per launch sequence, two recordings (with and without the actor
    step), replays - against three `train_one_batch()`, at the bars of `test_mlp_redq_gpu.test_replayed_update_equals_the_eager_update`
    (parameters 2e-5 / 2e-7, logs 2e-5)."""
    from offpolicy_rnn.algorithm.graphed_transition_update import GraphedTransitionUpdate
    from offpolicy_rnn.utility import rng
    over = dict(utd=3, policy_utd=1)
    block = torch.randn(4096, generator=torch.Generator().manual_seed(7)).to(DEV)
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: block[:int(np.prod(shape))].view(tuple(shape)).to(dtype))
    eager = _fresh(rnn, n_actions, **over)
    start = _state(eager)
    logs_e = [dict(eager.train_one_batch()) for _ in range(3)]
    graphed = _fresh(rnn, n_actions, **over)
    assert GraphedTransitionUpdate.refusal(graphed) is None
    g = GraphedTransitionUpdate(graphed, warmup=0)
    try:
        logs_g = [dict(g.step()) for _ in range(3)]
        torch.cuda.synchronize()
        assert len(g.graphs) == 2 and g.eager_fallbacks == 2, (len(g.graphs), g.eager_fallbacks)      # one eager pass per launch sequence
        assert int(g.pass_word.item()) == 3 and g.recording.steps == 9
    finally:
        g.close()
    for a, b in zip(eager.optimizers_value + [eager.optimizer_policy], graphed.optimizers_value + [graphed.optimizer_policy]):
        assert a.step_count == b.step_count
    assert eager.optimizers_value[1].step_count == 9 and eager.optimizer_policy.step_count == 3
    names = list(eager._state_networks()) + ['log alpha']
    for nm, a, b in zip(names, _state(graphed), _state(eager)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=2e-7, err_msg=nm)
    moved = [not torch.equal(a, b) for a, b in zip(start, _state(eager))]
    assert all(moved[:-1]) and (moved[-1] or n_actions)          # every network moved, and the temperature
    for le, lg in zip(logs_e, logs_g):
        assert set(le) == set(lg) and len(le) == 8
        for k in le:
            assert abs(val(le[k]) - val(lg[k])) <= 2e-5 * max(1.0, abs(val(le[k]))), (k, le[k], lg[k])


# ------------------------------------------------------------------------------------------------ 5. train()
def _env_trainer(monkeypatch, tmp_path, env, graph_update, **over):
    from offpolicy_rnn import alg_init
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('RESEL_DEVICE_COLLECT', raising=False)
    monkeypatch.delenv('RESEL_GRAPH_ROLLOUT', raising=False)
    monkeypatch.delenv('RESEL_CHECKPOINT_DIR', raising=False)
    if graph_update is None:
        monkeypatch.delenv('RESEL_GRAPH_UPDATE', raising=False)
    else:
        monkeypatch.setenv('RESEL_GRAPH_UPDATE', graph_update)
    kw = dict(env=env, cuda_inference=True, total_iteration=3, step_per_iteration=100, random_num=60, start_train_num=60,
              update_interval=2, utd=2, policy_utd=1, sac_batch_size=16, test_nprocess=1, test_nrollout=2)
    return alg_init(slice_parameter('gru', L=4, **dict(kw, **over)))


@pytest.mark.parametrize('graph_update', [None, '0'], ids=['replayed', 'eager'])
@pytest.mark.parametrize('env', ['synthetic-o5-a3-T12', 'Mem-T-passive-10-v0'])
def test_train(ops, monkeypatch, tmp_path, env, graph_update):
    """3 iterations x 100 steps behind 60 random steps, an update (utd = 2) behind every second step: finite logs of the reference's
    eight keys, `grad_num` as the loop's rule gives it, an `EpRetTest` per iteration."""
    from offpolicy_rnn.algorithm.graphed_transition_update import GraphedTransitionUpdate
    alg = _env_trainer(monkeypatch, tmp_path, env, graph_update)
    logged, add = [], alg.logger.add_tabular_data
    drivers, close = [], GraphedTransitionUpdate.close

    def record(tb_prefix=None, **data):
        logged.append((tb_prefix, dict(data)))
        return add(tb_prefix=tb_prefix, **data)

    monkeypatch.setattr(alg.logger, 'add_tabular_data', record)
    monkeypatch.setattr(GraphedTransitionUpdate, 'close', lambda self: (drivers.append(self), close(self))[1])      # `train()` closes its driver
    alg.train()
    torch.cuda.synchronize()
    # `sample_num` counts from the warm-up's total (>= 60: whole episodes); an update wherever it is even
    first = alg.sample_num - 300
    n_updates = sum(1 for s in range(first, first + 300) if s % 2 == 0)
    assert first >= 60 and alg.grad_num == n_updates
    updates = [d for p, d in logged if p == 'train']
    keys = {'actor_loss', 'critic_loss', 'alpha_loss', 'log_alpha', 'log_prob', 'target_q_max', 'policy_l2_norm_square', 'q1_l2_norm_square'}
    assert len(updates) == n_updates and all(set(d) == keys for d in updates)
    assert all(np.isfinite(val(v)) for d in updates for v in d.values())
    tests = [d for p, d in logged if p == 'performance']
    assert len(tests) == 3 and all(len(d['EpRetTest']) == 2 and np.isfinite(d['EpRetTest']).all() for d in tests)
    assert all(o.step_count == 2 * n_updates for o in alg.optimizers_value) and alg.optimizer_policy.step_count == n_updates
    for name, net in alg._state_networks().items():
        assert torch.isfinite(net.store.flat).all(), name
    if graph_update is None:
        assert len(drivers) == 1 and len(drivers[0].graphs) == 2 and drivers[0].eager_fallbacks <= 4
    else:
        assert not drivers


# ------------------------------------------------------------------------------------------------ 6. run state
def _snapshot(alg):
    torch.cuda.synchronize()
    ring = alg.replay_buffer
    return dict(ring=_bits(ring.memory_buffer), tables=(list(ring.trajectory_start), list(ring.trajectory_length), ring.ptr, ring.transition_count),
                networks={k: _bits(n.store.flat) for k, n in alg._state_networks().items()}, alpha=_bits(alg.log_sac_alpha),
                moments={k: (_bits(o.m), _bits(o.v), o.step_count) for k, o in alg._state_optimizers().items()},
                numpy=[np.asarray(x).tolist() if isinstance(x, np.ndarray) else x for x in np.random.get_state()],
                torch_cpu=torch.get_rng_state().tolist(), torch_dev=torch.cuda.get_rng_state(alg.sample_device).tolist(),
                counts=(alg.sample_num, alg.grad_num, alg.iteration))


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            for n in a[k]:
                xs, ys = (a[k][n], b[k][n]) if isinstance(a[k][n], tuple) else ((a[k][n],), (b[k][n],))
                assert all(np.array_equal(x, y) for x, y in zip(xs, ys)), (what, k, n)
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k)


def test_run_state_continues_bit_for_bit(ops, monkeypatch, tmp_path):
    """RESEL_GRAPH_UPDATE=0 (every update the same sequence of eager launches): three iterations straight through, against a fresh trainer
    that finds only the state written behind iteration two and runs the third - the ring, the parameters of all five networks, the moments
    and the generators are equal bit for bit (the pattern of tests/test_mlp_redq_gpu.py)."""
    import shutil
    kw = dict(total_iteration=3, step_per_iteration=40, random_num=48, start_train_num=48, update_interval=1, utd=1)

    def run(ckpt_dir):
        alg = _env_trainer(monkeypatch, tmp_path, 'synthetic-o5-a3-T12', '0', **kw)
        if ckpt_dir is not None:
            monkeypatch.setenv('RESEL_CHECKPOINT_DIR', str(ckpt_dir))
            monkeypatch.setenv('RESEL_CHECKPOINT_EVERY', '2')
        alg.train()
        return alg, _snapshot(alg)

    _, straight = run(None)
    _, writing = run(tmp_path / 'b')
    assert sorted(os.listdir(tmp_path / 'b')) == ['state-000002']
    os.makedirs(tmp_path / 'c')
    shutil.copytree(tmp_path / 'b' / 'state-000002', tmp_path / 'c' / 'state-000002')
    resumed_alg, resumed = run(tmp_path / 'c')
    assert straight['counts'] == (48 + 120, 120, 3) and straight['moments']['value1'][2] == 120 and straight['moments']['policy'][2] == 120
    _same(writing, straight, 'a state written on the way')
    _same(resumed, straight, 'resumed behind iteration two')
    fp = resumed_alg.state_fingerprint()
    assert fp['alg_name'] == 'sac_rnn_slice' and fp['trainer'] == 'SACRNNSlice' and 'numel_target_value1' in fp
