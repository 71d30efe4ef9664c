"""The memoryless REDQ baseline `sac_mlp_redq_ensemble_q` on cuda:0: the transition gather and the guard-less target against their
host / fp64 spellings, three updates against the recording of the reference, replayed against eagerly launched updates, the REDQ subset
path, `train()` on Wind-v0 and a run state.  Host side: tests/test_mlp_redq_host.py."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from test_mlp_redq_host import check_against_recording, feed_draws, fill, golden_trainer, mlp_parameter, val, wrapped_ring

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


# ------------------------------------------------------------------------------------------------ 1. the gather
def test_gather_transitions_is_bit_equal_to_sample_transitions(ops):
    """The wrapped, twice-evicted 27-column ring; batch 37 (no multiple of the four rows of a block), three passes, each selected by
    argument and by the device pass word; `c_timeout = -1` leaves `done` as stored; rows outside the ring come back as zeros."""
    ring = wrapped_ring()
    n, passes = 37, 3
    np.random.seed(5)
    rows = ring.plan_transitions(n, passes)
    np.random.seed(5)
    want = [ring.sample_transitions(n) for _ in range(passes)]
    mirror = ring._mirror(DEV)
    rows_dev = torch.from_numpy(rows).to(DEV)
    R = ring.name2range
    c_done, c_timeout = R['done'][0], R['timeout'][0]
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    fixed = 0
    for p in range(passes):
        stored = np.concatenate([f for f in want[p] if f is not None], axis=1)
        fix = stored.copy()
        fix[stored[:, c_timeout] > 0, c_done] = 0
        fixed += int((fix != stored).sum())
        word.fill_(p)
        for got in (ops.gather_transitions(mirror, rows_dev, None, p, c_done, c_timeout),
                    ops.gather_transitions(mirror, rows_dev, word, 0, c_done, c_timeout)):
            assert got.shape == (n, 27)
            assert np.array_equal(got.cpu().numpy().view(np.int32), fix.view(np.int32)), p
        raw = ops.gather_transitions(mirror, rows_dev, None, p, c_done, -1)
        assert np.array_equal(raw.cpu().numpy().view(np.int32), stored.view(np.int32)), p
    assert fixed > 0                                             # some drawn transition did time out
    bad = rows_dev.clone()
    bad[1, 3], bad[1, 36] = -1, mirror.shape[0]
    got = ops.gather_transitions(mirror, bad, None, 1, c_done, c_timeout).cpu().numpy()
    assert not got[3].any() and not got[36].any() and got[4].any()
    word.fill_(passes)                                           # a pass word outside the table: zero rows, nothing read
    assert not ops.gather_transitions(mirror, rows_dev, word, 0, c_done, c_timeout).cpu().numpy().any()
    with pytest.raises(RuntimeError):
        ops.gather_transitions(mirror, rows_dev, None, passes, c_done, c_timeout)


# ------------------------------------------------------------------------------------------------ 2. the target
@pytest.mark.parametrize('with_logp', [True, False])
def test_redq_target_against_fp64(ops, with_logp):
    """E = 4, m = 2, M = 37, some done = 1 rows, against the fp64 torch spelling at the forward bar of the fused RL kernels."""
    from test_rl_tail_gpu import close_fwd, f32
    g = torch.Generator().manual_seed(3)
    E, m, M, gamma = 4, 2, 37, 0.99
    q = torch.randn(E, M, 1, generator=g) * 3
    logp = torch.randn(M, 1, generator=g) - 1
    reward, done = torch.randn(M, 1, generator=g), (torch.rand(M, 1, generator=g) < 0.3).float()
    assert 0 < done.sum() < M
    log_alpha = torch.tensor([-0.3])
    subset = torch.tensor([3, 1], dtype=torch.int32)
    stats = torch.zeros(1, device=DEV)
    got = ops.redq_target(q.to(DEV), subset.to(DEV), logp.to(DEV) if with_logp else None, log_alpha.to(DEV), reward.to(DEV), done.to(DEV),
                          gamma, stats)
    v = q.double()[subset.long()].min(dim=0).values
    if with_logp:
        v = v - log_alpha.double().exp() * logp.double()
    ref = reward.double() + (1 - done.double()) * f32(gamma) * v
    assert got.shape == reward.shape
    close_fwd(got, ref, name='target')
    close_fwd(stats, ref.abs().max().reshape(1), name='max |target|')


# ------------------------------------------------------------------------------------------------ 3. against the reference
META = json.load(open(os.path.join(GOLDEN, 'train_mlp_meta.json'))) if os.path.exists(os.path.join(GOLDEN, 'train_mlp_meta.json')) else {}


@pytest.mark.parametrize('rec', ['utd3', 'utd4'])
def test_three_eager_updates_equal_the_reference_recording(ops, monkeypatch, rec):
    """Initial networks and ring of the recording, its Gaussian draws through utility/rng.py, three eager updates on cuda:0 (plan + gather,
    the HIP ops): logs within 2e-3 / 5e-4 (`test_discrete_train_one_batch_gpu_vs_reference_logs`), parameters within 1e-3 / 2e-5,
    every element."""
    g = load_golden('train_mlp_redq.npz')
    alg = golden_trainer(rec, META, g)
    assert alg.device.type == 'cuda'
    fed = feed_draws(monkeypatch, g, rec, META[rec]['draws'])
    torch.manual_seed(200)
    np.random.seed(200)
    logs = [dict(alg.train_one_batch()) for _ in range(3)]
    assert fed['k'] == META[rec]['draws']
    for it, log in enumerate(logs):
        print(rec, it, {k: val(v) for k, v in log.items()})
    check_against_recording(alg, g, rec, logs, META[rec], 2e-3, 5e-4, 1e-3, 2e-5)


# ------------------------------------------------------------------------------------------------ 4. replayed against eager
def _state(alg):
    return [alg.policy.store.flat.detach().clone(), alg.values[0].store.flat.detach().clone(), alg.target_values[0].store.flat.detach().clone(),
            alg.log_sac_alpha.detach().clone()]


def _fresh(**over):
    from offpolicy_rnn import alg_init
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(mlp_parameter(cuda_inference=True, sac_batch_size=37, **over))
    fill(alg.replay_buffer)
    np.random.seed(11)
    return alg


@pytest.mark.parametrize('case', ['utd3', 'utd4-policy_utd2-clipped', 'utd3-encoders'])
def test_replayed_update_equals_the_eager_update(ops, monkeypatch, case):
    """Same start, same numpy seed, the same Gaussian numbers for every draw (a fixed device block: a recording has no host draw to
    feed): three steps through `GraphedTransitionUpdate` - an eager pass, a recording per launch sequence, replays - against three
    `train_one_batch()`, at the bars of `test_graphed_update_equals_the_eager_update` (parameters 2e-5 / 2e-7, logs 2e-5)."""
    from offpolicy_rnn.algorithm.graphed_transition_update import GraphedTransitionUpdate
    from offpolicy_rnn.utility import rng
    over = {'utd3': dict(utd=3, policy_utd=1), 'utd3-encoders': dict(utd=3, policy_utd=1, encoders=True),
            'utd4-policy_utd2-clipped': dict(utd=4, policy_utd=2, value_max_gradnorm=0.5, policy_max_gradnorm=0.05)}[case]
    block = torch.randn(4096, generator=torch.Generator().manual_seed(7)).to(DEV)
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: block[:int(np.prod(shape))].view(tuple(shape)).to(dtype))
    eager = _fresh(**over)
    start = _state(eager)
    logs_e = [dict(eager.train_one_batch()) for _ in range(3)]
    graphed = _fresh(**over)
    assert GraphedTransitionUpdate.refusal(graphed) is None
    g = GraphedTransitionUpdate(graphed, warmup=0)
    try:
        logs_g = [dict(g.step()) for _ in range(3)]
        torch.cuda.synchronize()
        passes = 3 * over['utd']
        assert len(g.graphs) == 2 and g.eager_fallbacks == 2, (len(g.graphs), g.eager_fallbacks)      # one eager pass per launch sequence
        assert int(g.pass_word.item()) == over['utd'] and g.recording.steps == passes
    finally:
        g.close()
    assert eager.optimizer_value.step_count == graphed.optimizer_value.step_count == 3 * over['utd']
    assert eager.optimizer_policy.step_count == graphed.optimizer_policy.step_count == 3 * over['policy_utd']
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), _state(graphed), _state(eager)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=2e-7, err_msg=nm)
    assert not any(torch.equal(a, b) for a, b in zip(start, _state(eager)))      # every network and the temperature moved
    for le, lg in zip(logs_e, logs_g):
        assert set(le) == set(lg) and len(le) == 10
        for k in le:
            assert abs(val(le[k]) - val(lg[k])) <= 2e-5 * max(1.0, abs(val(le[k]))), (k, le[k], lg[k])
    if 'clipped' in case:
        assert logs_e[-1]['q_grad_norm'] > 0.5 and logs_e[-1]['pi_grad_norm'] > 0.05     # both clips did bite


# ------------------------------------------------------------------------------------------------ 5. the REDQ subset
@pytest.mark.parametrize('encoders', [False, True])
def test_subset_path_equals_evaluate_all_then_select(ops, encoders):
    """`member_index` through the critic's embedding stack and head against all members evaluated and the drawn ones selected."""
    from offpolicy_rnn.algorithm.sac_mlp_redq_ensemble_q import _ensemble_subset
    alg = _fresh(encoders=encoders)
    tv = alg.target_values[0]
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    state, last_state, last_action, action, reward = r(37, 5), r(37, 5), r(37, 3), torch.tanh(r(37, 3)), r(37, 1)
    index = torch.tensor([2, 0], dtype=torch.int64, device=DEV)
    with torch.no_grad():
        full = tv.forward(state, last_state, last_action, action, None, reward)[0]
        with _ensemble_subset(tv, index):
            part = tv.forward(state, last_state, last_action, action, None, reward)[0]
    assert full.shape == (4, 37, 1) and part.shape == (2, 37, 1)
    assert all(l.member_index is None for net in (tv.embedding_network, tv.uni_network) for l in net.layer_list)
    np.testing.assert_allclose(part.cpu().numpy(), full[index].cpu().numpy(), rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------------ 6. train()
def _wind_trainer(monkeypatch, tmp_path, graph_update, **over):
    from offpolicy_rnn import alg_init
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('RESEL_DEVICE_COLLECT', '1')
    monkeypatch.delenv('RESEL_GRAPH_ROLLOUT', raising=False)
    monkeypatch.delenv('RESEL_CHECKPOINT_DIR', raising=False)
    if graph_update is None:
        monkeypatch.delenv('RESEL_GRAPH_UPDATE', raising=False)
    else:
        monkeypatch.setenv('RESEL_GRAPH_UPDATE', graph_update)
    kw = dict(env='Wind-v0', cuda_inference=True, total_iteration=3, step_per_iteration=150, random_num=150, start_train_num=150,
              update_interval=1, utd=2, policy_utd=1, sac_batch_size=32, test_nprocess=1, test_nrollout=2)
    return alg_init(mlp_parameter(**dict(kw, **over)))


@pytest.mark.parametrize('graph_update', [None, '0'], ids=['replayed', 'eager'])
def test_train_on_wind(ops, monkeypatch, tmp_path, graph_update):
    """3 iterations x 150 steps behind 150 random steps, utd = 2: finite logs, `grad_num` as the loop's rule gives it, an `EpRetTest` per
    iteration, training episodes collected on the device."""
    from offpolicy_rnn.algorithm.graphed_transition_update import GraphedTransitionUpdate
    alg = _wind_trainer(monkeypatch, tmp_path, graph_update)
    logged, add = [], alg.logger.add_tabular_data
    drivers, close = [], GraphedTransitionUpdate.close

    def record(tb_prefix=None, **data):
        logged.append((tb_prefix, dict(data)))
        return add(tb_prefix=tb_prefix, **data)

    monkeypatch.setattr(alg.logger, 'add_tabular_data', record)
    monkeypatch.setattr(GraphedTransitionUpdate, 'close', lambda self: (drivers.append(self), close(self))[1])      # `train()` closes its driver
    alg.train()
    torch.cuda.synchronize()
    assert alg.sample_num == 150 + 450 and alg.grad_num == 450       # an update behind every step from `start_train_num` on
    updates = [d for p, d in logged if p == 'train']
    assert len(updates) == 450 and len(updates[0]) == 10
    assert all(np.isfinite(val(v)) for d in updates for v in d.values())
    tests = [d for p, d in logged if p == 'performance']
    assert len(tests) == 3 and all(len(d['EpRetTest']) == 2 and np.isfinite(d['EpRetTest']).all() for d in tests)
    assert alg.collector is not None and alg.collector.replays == 450 and alg.collector.episode_syncs == 6
    assert len(alg.replay_buffer) == 2 + 6 and alg.optimizer_value.step_count == 900 and alg.optimizer_policy.step_count == 450
    for name, net in alg._state_networks().items():
        assert torch.isfinite(net.store.flat).all(), name
    if graph_update is None:
        assert len(drivers) == 1 and len(drivers[0].graphs) == 2 and drivers[0].eager_fallbacks <= 4
    else:
        assert not drivers


# ------------------------------------------------------------------------------------------------ 7. run state
def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.int32 if a.dtype.itemsize == 4 else np.int64).copy()


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
    that finds only the state written behind iteration two and runs the third - the ring, the parameters, the moments and the generators
    are equal bit for bit (the pattern of tests/test_run_state_gpu.py `_three_runs`)."""
    import shutil
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm import run_state
    from test_host_logic import make_parameter
    kw = dict(total_iteration=3, step_per_iteration=40, random_num=75, start_train_num=75, sac_batch_size=16)

    def run(ckpt_dir):
        alg = _wind_trainer(monkeypatch, tmp_path, '0', **kw)
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
    assert straight['counts'] == (75 + 120, 120, 3) and straight['moments']['value0'][2] == 240 and straight['moments']['policy'][2] == 120
    _same(writing, straight, 'a state written on the way')
    _same(resumed, straight, 'resumed behind iteration two')
    assert resumed_alg.collector is not None
    # the fingerprint tells this trainer from the others
    assert resumed_alg.state_fingerprint()['alg_name'] == 'sac_mlp_redq_ensemble_q' and resumed_alg.state_fingerprint()['trainer'] == 'SAC_MLP_REDQ_EnsembleQ'
    monkeypatch.delenv('RESEL_CHECKPOINT_DIR')
    other = alg_init(make_parameter('gilr', env='Wind-v0', cuda_inference=True))
    with pytest.raises(run_state.RunStateMismatch):
        other.load_state(str(tmp_path / 'b' / 'state-000002'))
