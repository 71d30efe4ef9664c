"""Run states on the device (algorithm/run_state.py, `SAC.save_state` / `load_state`, RESEL_CHECKPOINT_DIR at `train()`):
1. round trip - a fresh trainer that loads a state is the trainer that wrote it; 2. continuation - a run resumed from the middle ends
as the uninterrupted run, bit for bit wherever the update is a sequence of eager launches or there is none; 3. graphed updates - the
same training, counted; 4. writing states leaves the running trainer alone.  All comparisons are `snapshot`s (tests/test_run_state_host.py):
integer views of every buffer, every random stream, the environment, the open episode with its recurrent state, the evaluator."""
import os
import shutil

import numpy as np
import pytest
import torch

from test_run_state_host import assert_same, differ, snapshot

pytestmark = pytest.mark.gpu
CONTROLS_DIFFER = 'two uninterrupted runs do not agree bit for bit on this GPU'
TMAZE, WIND, SYNTHETIC = 'Mem-T-passive-5-v0', 'Wind-v0', 'synthetic-o5-a3-T12'
T = 6                                                           # steps of a Mem-T-passive-5 episode
TRAIN = dict(random_num=24, start_train_num=24, update_interval=3, step_per_iteration=20, sac_batch_size=24, test_nprocess=0, test_nrollout=0)
EVAL = dict(test_nprocess=1, test_nrollout=2)
NO_UPDATES = dict(start_train_num=10 ** 9)


@pytest.fixture(scope='module', autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')


def _trainer(monkeypatch, tmp_path, rnn, env, ckpt_dir=None, every=2, collect=True, graph_update=None, graph_rollout=None, algo='sac', **over):
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('RESEL_DEVICE_COLLECT', '1' if collect else '0')
    for name, value in (('RESEL_GRAPH_ROLLOUT', graph_rollout), ('RESEL_GRAPH_UPDATE', graph_update)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    if ckpt_dir is None:
        monkeypatch.delenv('RESEL_CHECKPOINT_DIR', raising=False)
    else:
        monkeypatch.setenv('RESEL_CHECKPOINT_DIR', str(ckpt_dir))
    monkeypatch.setenv('RESEL_CHECKPOINT_EVERY', str(every))
    return alg_init(make_parameter(rnn, env=env, algo=algo, cuda_inference=True, **dict(TRAIN, **over)))


def _run(monkeypatch, tmp_path, rnn, env, **kw):
    """One trainer, `train()` -> (trainer, its snapshot, the training episodes it logged as (return bits, length))."""
    alg = _trainer(monkeypatch, tmp_path, rnn, env, **kw)
    logged, add = [], alg.logger.add_tabular_data

    def record(tb_prefix=None, **data):
        if tb_prefix == 'Train':
            logged.append((np.float64(data['EpRet']).view(np.int64).item(), type(data['EpRet']), data['EpLength'], type(data['EpLength'])))
        return add(tb_prefix=tb_prefix, **data)

    monkeypatch.setattr(alg.logger, 'add_tabular_data', record)
    alg.train()
    return alg, snapshot(alg), logged


def _only_state(src_dir, dst_dir, name):
    """A checkpoint directory that holds the one state `name` of `src_dir` - what a run stopped right behind that write leaves."""
    os.makedirs(dst_dir)
    shutil.copytree(os.path.join(src_dir, name), os.path.join(dst_dir, name))
    return dst_dir


# ------------------------------------------------------------------------------------------------ 1. round trip
ROUND_TRIPS = {
    'gru-tmaze-device-collect': dict(rnn='gru', env=TMAZE),                                   # the state falls four steps into an episode
    'smamba-wind': dict(rnn='smamba_s16_c4_b1', env=WIND),
    'cgpt-tmaze-kv-cache': dict(rnn='cgpt_h1_l2_p0_ml32', env=TMAZE),                         # a KV cache mid-episode with its position
    'gilr-td3-synthetic-host-loop': dict(rnn='gilr', env=SYNTHETIC, algo='td3'),              # the host loop; `target_policy`
    'gru-tmaze-evaluator': dict(rnn='gru', env=TMAZE, **EVAL),
    'gru-tmaze-eager-rollout': dict(rnn='gru', env=TMAZE, graph_rollout='0'),                 # the recurrent state lives in `sample_hidden`
}


@pytest.mark.parametrize('case', list(ROUND_TRIPS))
def test_round_trip(case, tmp_path, monkeypatch):
    kw = dict(ROUND_TRIPS[case], total_iteration=2)
    eager_rollout = kw.get('graph_rollout') == '0'
    writer = _trainer(monkeypatch, tmp_path, **kw)
    writer.train()
    want = snapshot(writer)
    path = writer.save_state(str(tmp_path / 'states' / 'one'))
    assert_same(snapshot(writer), want, 'writing a state changes nothing')
    n = 40
    assert want['counts'][2] == 2 and want['counts'][0] == (75 if kw['env'] == WIND else 24) + n and want['counts'][1] > 0
    assert any(m.any() for m, _, _ in want['moments'].values()) and all(s > 0 for _, _, s in want['moments'].values())
    if kw['env'] == TMAZE:
        assert want['episode'][1] == n % T == want['tables'][4] and (writer.collector is not None) == (not eager_rollout)
    if 'cgpt' in kw['rnn']:
        caches = [h for h in want['hidden'] if isinstance(h, tuple)]
        assert caches and all(pos == n % T and dev == [n % T] and filled for pos, dev, filled in caches)          # four tokens into the episode
    if kw.get('algo') == 'td3':
        assert writer.collector is None and 'target_policy' in want['networks'] and want['episode'][1] == n % 12
    assert (want['evaluator'] is not None) == ('test_nprocess' in kw)
    assert (writer.graph_step is None) == eager_rollout
    reader = _trainer(monkeypatch, tmp_path, **kw)
    fresh = reader.policy.store.flat.clone()
    reader.load_state(path)
    assert_same(snapshot(reader), want, case)
    assert not torch.equal(reader.policy.store.flat, fresh)
    assert '_dev_state' not in reader.replay_buffer.__dict__ and reader.replay_buffer._dirty == []        # the mirror is built anew at the next sample


# ------------------------------------------------------------------------------------------------ 2. continuation
def _three_runs(monkeypatch, tmp_path, rnn, env, **kw):
    """(a) four iterations without a checkpoint directory, (b) the same with a state every two, (c) a fresh trainer that finds only
    `state-000002` -> (a, b, c) as `_run` returns them."""
    a = _run(monkeypatch, tmp_path, rnn, env, total_iteration=4, **kw)
    b = _run(monkeypatch, tmp_path, rnn, env, total_iteration=4, ckpt_dir=tmp_path / 'b', **kw)
    assert sorted(os.listdir(tmp_path / 'b')) == ['state-000002', 'state-000004']
    c = _run(monkeypatch, tmp_path, rnn, env, total_iteration=4, ckpt_dir=_only_state(tmp_path / 'b', tmp_path / 'c', 'state-000002'), **kw)
    assert sorted(os.listdir(tmp_path / 'c')) == ['state-000002', 'state-000004']
    assert 0 < len(c[2]) < len(a[2]) == len(b[2])              # (c) ran the second half only: it logged that half's episodes
    return a, b, c


@pytest.mark.parametrize('rnn,collect,steps', [('gru', True, 20), ('gru', True, 18), ('gru', False, 20), ('cgpt_h1_l2_p0_ml32', True, 20)],
                         ids=['device-collect', 'device-collect-state-behind-a-reset', 'host-loop', 'cgpt-device-collect'])
def test_continuation_without_updates(rnn, collect, steps, tmp_path, monkeypatch):
    """No update, so nothing may differ and nothing may skip.  20 steps an iteration put the state four steps into an episode: the resumed
    run finishes that episode through the host loop and the collector takes over behind its `env_reset()`; 18 put it behind a reset."""
    (_, want, logged), (_, with_states, _), (alg, got, tail) = _three_runs(
        monkeypatch, tmp_path, rnn, TMAZE, collect=collect, step_per_iteration=steps, **dict(EVAL, **NO_UPDATES))
    assert want['counts'] == (24 + 4 * steps, 0, 4) and len(logged) == 4 * steps // T and want['evaluator'] is not None
    assert_same(with_states, want, 'states written on the way')
    assert_same(got, want, 'resumed from iteration 2')
    assert tail == logged[-len(tail):] and len(tail) == 4 * steps // T - 2 * steps // T
    c = alg.collector
    assert (c is not None) == collect
    if collect:
        resumed_steps = 2 * steps
        host_steps = (T - 2 * steps % T) % T                    # the steps that finished the open episode
        assert host_steps == (2 if steps == 20 else 0)
        assert c.replays == resumed_steps - host_steps
        assert c.episode_syncs == (resumed_steps - host_steps) // T and c.init_launches == c.episode_syncs + 1
        assert (alg.graph_step._graph is not None) == (host_steps > 0)         # the B = 1 step is captured only to finish an open episode
    else:
        assert alg.graph_step._graph is not None


@pytest.mark.parametrize('interval', [3, 5], ids=['updates-inside-episodes', 'updates-on-last-steps'])
def test_continuation_with_eager_updates(interval, tmp_path, monkeypatch):
    """RESEL_GRAPH_UPDATE=0: every update is the same sequence of launches in both runs.  The uninterrupted run is done twice as a
    control (atomics may order differently from run to run); the resumed run must equal it whenever the control agrees with itself."""
    kw = dict(graph_update='0', update_interval=interval, **EVAL)
    _, control, _ = _run(monkeypatch, tmp_path, 'gru', TMAZE, total_iteration=4, **kw)
    (_, first, _), (_, with_states, _), (alg, got, _) = _three_runs(monkeypatch, tmp_path, 'gru', TMAZE, **kw)
    assert first['counts'] == (24 + 80, len([s for s in range(24, 104) if s % interval == 0]), 4)
    if differ(first, control):
        pytest.skip(CONTROLS_DIFFER)
    assert alg.collector is not None and alg.collector.replays == 38
    assert_same(with_states, first, ('eager updates, states written on the way', interval))
    assert_same(got, first, ('eager updates, resumed', interval))


def test_continuation_with_eager_updates_on_the_host_loop(tmp_path, monkeypatch):
    """TD3 on the synthetic environment: the host loop, target smoothing noise from the device generator, no temperature step."""
    kw = dict(graph_update='0', algo='td3')
    _, control, _ = _run(monkeypatch, tmp_path, 'gilr', SYNTHETIC, total_iteration=4, **kw)
    (_, first, _), (_, with_states, _), (alg, got, _) = _three_runs(monkeypatch, tmp_path, 'gilr', SYNTHETIC, **kw)
    if differ(first, control):
        pytest.skip(CONTROLS_DIFFER)
    assert alg.collector is None and first['counts'][1] > 0
    assert_same(with_states, first, 'td3 host loop, states written on the way')
    assert_same(got, first, 'td3 host loop, resumed')


# ------------------------------------------------------------------------------------------------ 3. graphed updates (the default)
def test_continuation_with_graphed_updates_continues_the_same_training(tmp_path, monkeypatch):
    """A replayed update draws its actor noise at graph-safe Philox offsets, and a resumed run records its graphs anew (eager warm-up
    passes first): the same training distribution, not the same bits.  What does not depend on parameters is equal."""
    (_, want, logged), _, (alg, got, tail) = _three_runs(monkeypatch, tmp_path, 'gru', TMAZE, **EVAL)
    assert got['counts'] == want['counts'] == (24 + 80, len([s for s in range(24, 104) if s % 3 == 0]), 4)
    assert got['tables'] == want['tables'] and got['episode'][1] == want['episode'][1] == 80 % T
    assert len(tail) == 80 // T - 40 // T and [e[2:] for e in tail] == [e[2:] for e in logged[-len(tail):]]
    assert {k: s for k, (_, _, s) in got['moments'].items()} == {k: s for k, (_, _, s) in want['moments'].items()}
    for name, net in alg._state_networks().items():
        assert torch.isfinite(net.store.flat).all(), name
    assert torch.isfinite(alg.log_sac_alpha).all() and torch.isfinite(alg.Q_guard.state).all()
    assert alg.collector is not None and alg.collector.replays == 38


# ------------------------------------------------------------------------------------------------ 4. writing a state perturbs nothing
def test_states_every_iteration_leave_the_run_as_it_is(tmp_path, monkeypatch):
    """Wind-v0, collected on the device, a state after every iteration - each one inside a 75-step episode (`sync_host()`, snapshot,
    pending transitions out of the ring again) - against the same run that writes nothing."""
    kw = dict(total_iteration=3, step_per_iteration=30, **dict(EVAL, **NO_UPDATES))
    plain_alg, want, logged = _run(monkeypatch, tmp_path, 'smamba_s16_c4_b1', WIND, **kw)
    alg, got, logged_b = _run(monkeypatch, tmp_path, 'smamba_s16_c4_b1', WIND, ckpt_dir=tmp_path / 'b', every=1, **kw)
    assert alg.collector is not None and alg.collector.replays == 90 and want['counts'] == (75 + 90, 0, 3)
    assert_same(got, want, 'a state per iteration')
    assert logged_b == logged and len(logged) == 1 and want['episode'][1] == 15
    assert sorted(os.listdir(tmp_path / 'b')) == ['state-000002', 'state-000003']
    assert not [f for f in os.listdir(tmp_path) if f.startswith('state-') or f.startswith('tmp-')]
