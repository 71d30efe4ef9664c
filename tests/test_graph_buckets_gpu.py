"""Update graphs for variable-length episodes (algorithm/graphed_update.py `buckets`, buffers/transition_buffer/shape_buckets.py) on
the GPU: the gather kernel's padding of a bucketed plan, replays of bucketed shapes against the eager update on the same shapes, the
padded update against the unpadded one, the 'auto' switch and the refusal for layers that need sequence tables.
Workload, helpers: tests/test_shape_buckets.py (24 trajectories of 3..40 steps, batches of 95 transitions).  Actor noise is off as in
tests/test_trainer_gpu.py `test_graphed_update_equals_the_eager_update` (a padded update draws noise for a larger tensor)."""
import numpy as np
import pytest
import torch

from test_host_logic import _push, _synth, make_parameter
from test_shape_buckets import fill_ragged, ragged_trainer


@pytest.fixture
def no_noise(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.utility import rng
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.zeros(tuple(shape), dtype=dtype, device=device))


def _trainer(rnn, algo='sac', per=1):
    torch.manual_seed(0)
    np.random.seed(0)
    alg = ragged_trainer(rnn, algo=algo, cuda_inference=True, policy_update_per=per)
    np.random.seed(11)
    return alg


def _state(alg):
    return [alg.policy.store.flat.detach().clone(), alg.values[0].store.flat.detach().clone(), alg.target_values[0].store.flat.detach().clone(),
            alg.log_sac_alpha.detach().clone()]


def _value(v):
    return v[0] if isinstance(v, tuple) else v


def _key_len(g, bucketed):
    """Entries of a graph key of the driver `g`, from the key function on the plan of its last pass."""
    from offpolicy_rnn.algorithm.graph_policy import exact_table_key, graph_key
    from offpolicy_rnn.buffers.transition_buffer.shape_buckets import pad_seq_tables
    pl, table = g._plan, ()
    if g.alg._needs_seq_table:
        built = g._build_seqs(pl)
        table = pad_seq_tables(built, pl['nrow'], pl['longest'])[1] if bucketed else exact_table_key(built)
    return len(graph_key(pl, table, bucketed, False))


def _compare(what, alg_a, alg_b, logs_a, logs_b, rtol, atol):
    """Parameters, target parameters, log alpha and every logged scalar; every figure is printed before anything is asserted."""
    worst = []
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), _state(alg_a), _state(alg_b)):
        a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
        excess = np.abs(a - b) - rtol * np.abs(b)
        print(f'MEASURED {what} {nm}: max |a - b| = {np.abs(a - b).max():.3e}, max (|a - b| - {rtol:g} |b|) = {excess.max():.3e} (atol {atol:g})')
        worst.append((nm, excess.max()))
    log_err = 0.0
    for la, lb in zip(logs_a, logs_b):
        assert set(la) == set(lb)
        for k in la:
            log_err = max(log_err, abs(_value(la[k]) - _value(lb[k])) / max(1.0, abs(_value(lb[k]))))
    print(f'MEASURED {what} logged scalars: max |a - b| / max(1, |b|) = {log_err:.3e} (bound {rtol:g})')
    for nm, e in worst:
        assert e <= atol, (what, nm, e)
    assert log_err <= rtol, (what, log_err)


# ---------------------------------------------------------------------------------------------------------------- 1. padded gather
@pytest.mark.gpu
@pytest.mark.parametrize('nest,hist', [(True, 1), (False, 1), (True, 5)])
def test_bucketed_gather_is_the_exact_batch_plus_padding(nest, hist):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.buffers.transition_buffer.nested_replay_memory import NestedMemoryArray
    buf = NestedMemoryArray(5000, 40, additional_history_len=hist)
    fill_ragged(buf)
    dev = torch.device('cuda')
    out = {}
    for buckets in (False, True):
        np.random.seed(1)                             # draws (2, 58), (5, 33), (3, 55): padded to (2, 64), (6, 48), (3, 64)
        pl = buf.plan_trajs_device(95, None, nest_stack_trajs=nest, buckets=buckets)
        seg = torch.from_numpy(pl['seg']).to(dev)
        out[buckets] = (pl, buf.gather_planned(dev, seg, pl['max_len'], pl['nrow'], pl['longest']).cpu().numpy())
    (ple, exact), (pl, padded) = out[False], out[True]
    r, t = pl['nrow_real'], pl['longest_real']
    assert exact.shape[:2] == (r, t) and padded.shape == (pl['nrow'], pl['longest'], exact.shape[2])
    assert padded.shape[1] > t and (nest or padded.shape[0] > r), 'nothing was padded'
    assert exact[..., buf.name2range['mask'][0]].sum() == ple['total_size']
    np.testing.assert_array_equal(padded[:r, :t], exact)
    W = exact.shape[2] - 3
    R = buf.name2range
    pad = np.ones(padded.shape[:2], dtype=bool)
    pad[:r, :t] = False
    for name, col, want in (('mask', R['mask'][0], 0), ('validity', W, 0), ('extended validity', W + 1, 0), ('done', R['done'][0], 0),
                            ('start', R['start'][0], 1), ('target start', W + 2, 1)):
        assert (padded[..., col][pad] == want).all(), name


# ------------------------------------------------------------------------------------- 2. replay == eager run on the same shapes
@pytest.mark.gpu
@pytest.mark.parametrize('rnn,algo,per', [('smamba_s8_c4_b1_nln', 'sac', 1), ('smamba_s8_c4_b1_nln', 'sac', 2), ('gilr', 'td3', 1),
                                          ('lru', 'sac', 1), ('gru', 'sac', 1)])
def test_bucketed_replays_equal_the_eager_updates_on_the_same_shapes(rnn, algo, per, no_noise):
    """24 (48 with policy_update_per = 2) updates of the ragged workload: an eager trainer that pads its batches into their buckets
    against `GraphedUpdate(buckets='on')`.  Bounds of tests/test_trainer_gpu.py `test_graphed_update_equals_the_eager_update` for more
    than 16 chained updates.  Exact keys would replay next to nothing here (20-22 shapes in 24 updates); bucketed, all but the warm-up
    and the first visit of each shape are replays."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    n_upd = 24 * per
    eager = _trainer(rnn, algo, per)
    eager.shape_buckets = True
    logs_e = []
    for _ in range(n_upd):
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    graphed = _trainer(rnn, algo, per)
    g = GraphedUpdate(graphed, warmup=1, buckets='on')
    assert g.max_graphs == 8 * per
    logs_g = []
    for _ in range(n_upd):
        logs_g.append(dict(g.step()))
        graphed.grad_num += 1
    torch.cuda.synchronize()
    print(f'MEASURED {rnn} {algo} per {per}: graphs {len(g.graphs)} {sorted(g.graphs)}, eager updates {g.eager_fallbacks} of {n_upd}')
    assert len(g.graphs) >= 1 and all(len(k) == _key_len(g, True) for k in g.graphs)
    assert g.eager_fallbacks <= (6 if per == 1 else 10)
    _compare(f'{rnn} {algo} per {per} replay vs eager', graphed, eager, logs_g, logs_e, rtol=2e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------- 3. padding is free
@pytest.mark.gpu
@pytest.mark.parametrize('rnn,algo', [('smamba_s8_c4_b1_nln', 'sac'), ('gilr', 'td3'), ('lru', 'sac'), ('gru', 'sac')])
def test_the_padded_update_equals_the_unpadded_one(rnn, algo, no_noise):
    """One eager update on the same draw, padded into its bucket and not.  Padding changes M of the token-major GEMMs and K of the
    weight-gradient GEMMs (another split-K choice, another summation order): last-bit differences, the bounds of
    `test_graphed_update_equals_the_eager_update` for a short chain."""
    algs, logs = [], []
    for buckets in (True, False):
        alg = _trainer(rnn, algo)
        alg.shape_buckets = buckets
        logs.append([dict(alg.train_one_batch())])
        algs.append((alg, alg.replay_buffer._last_batch_shape))
    (padded, shape_p), (exact, shape_e) = algs
    print(f'MEASURED {rnn} {algo}: batch {shape_e} padded to {shape_p}')
    assert shape_p[0] >= shape_e[0] and shape_p[1] > shape_e[1]
    for k in ('real_batch_size', 'real_batch_traj_num'):
        assert logs[0][0][k] == logs[1][0][k], k
    assert logs[1][0]['real_batch_traj_num'] == shape_e[0]
    _compare(f'{rnn} {algo} padded vs unpadded', padded, exact, logs[0], logs[1], rtol=2e-5, atol=2e-7)


# -------------------------------------------------------------------------------------------------------------- 4. auto mode
@pytest.mark.gpu
def test_auto_mode_switches_on_ragged_data(no_noise):
    """Two graphs cannot hold the exact shapes of the ragged workload: 'auto' counts a third distinct shape, drops what it has and
    buckets from that update on - its shape is visited once eagerly, recorded on its second visit and replayed from then on."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    alg = _trainer('smamba_s8_c4_b1_nln')
    g = GraphedUpdate(alg, warmup=1, max_graphs=2, buckets='auto')
    assert g.buckets == 'auto'
    replayed, switched_at = [], None
    for i in range(24):
        before = g.eager_fallbacks
        log = dict(g.step())
        alg.grad_num += 1
        replayed.append(g.eager_fallbacks == before)
        if switched_at is None and g.buckets == 'on':
            switched_at = i + 1
        assert np.isfinite(_value(log['critic_loss']))
    torch.cuda.synchronize()
    print(f'MEASURED auto: switched at update {switched_at}, replays {sum(replayed)} of 24, graphs {sorted(g.graphs)}')
    assert switched_at is not None and switched_at <= 8
    assert g.max_graphs == 2, 'a caller\'s max_graphs is kept'
    assert sum(replayed[11:24]) >= 10
    assert all(len(k) == _key_len(g, True) for k in g.graphs) and 1 <= len(g.graphs) <= 2


@pytest.mark.gpu
def test_auto_mode_never_switches_on_fixed_length_data(no_noise):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter('smamba_s8_c4_b1_nln', sac_batch_size=4 * 12 - 1, cuda_inference=True))
    rs = np.random.RandomState(3)
    for _ in range(8):
        o, a, r = _synth(rs, 12, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=False)
    np.random.seed(11)
    g = GraphedUpdate(alg, warmup=1, max_graphs=2, buckets='auto')
    for _ in range(6):
        g.step()
        alg.grad_num += 1
    torch.cuda.synchronize()
    assert g.buckets == 'auto' and len(g.graphs) == 1 and all(len(k) == _key_len(g, False) for k in g.graphs)      # an exact key
    assert g.eager_fallbacks <= 2                               # the warm-up update (and a first visit, had the shape changed)


# ---------------------------------------------------------------------------------------------------- 5. sequence-table refusal
@pytest.mark.gpu
def test_buckets_refuse_layers_that_need_sequence_tables():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    alg = alg_init(make_parameter('cgpt_h1_l2_p0.0_ml64_rms', algo='td3', sac_batch_size=4 * 12 - 1, cuda_inference=True))
    rs = np.random.RandomState(3)
    for _ in range(4):
        o, a, r = _synth(rs, 12, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=False)
    assert GraphedUpdate.refusal(alg) is None
    with pytest.raises(RuntimeError, match='sequence tables'):
        GraphedUpdate(alg, warmup=1, buckets='on')
    alg.shape_buckets = True                                                 # the eager path refuses as well
    with pytest.raises(RuntimeError, match='sequence tables'):
        alg.train_one_batch()
    alg.shape_buckets = False


@pytest.mark.gpu
def test_auto_mode_stays_exact_with_sequence_tables():
    """cgpt on ragged data with room for one graph: another trainer would switch at its second shape; this one keeps exact keys."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter('cgpt_h1_l2_p0.0_ml64_rms', algo='td3', sac_batch_size=23, cuda_inference=True))
    rs = np.random.RandomState(3)
    for n in (12, 9, 7, 12, 5, 12, 10, 8):
        o, a, r = _synth(rs, n, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=(n != 12))
    np.random.seed(11)
    g = GraphedUpdate(alg, warmup=1, buckets='auto', max_graphs=1)
    try:
        for _ in range(4):
            log = dict(g.step())
            alg.grad_num += 1
            assert np.isfinite(_value(log['critic_loss']))
        torch.cuda.synchronize()
        print(f'MEASURED cgpt auto: {len(g._seen)} keys seen, buckets {g.buckets}')
        assert g.buckets == 'auto' and len(g._seen) >= 2, 'the shapes did not vary: nothing would have switched'
        assert all(len(k) == _key_len(g, False) for k in g._seen)                # exact key + the sizes of the two sequence tables + actor flag
    finally:
        g.close()
