"""Shape buckets of the packed batch (buffers/transition_buffer/shape_buckets.py) on the host: the ladder arithmetic, the planner's
contract with `buckets=True` (same sampling decisions and numpy draws, padding that the gather kernel drops) and how few bucketed
shapes a ragged workload has where its exact shapes hardly recur - what lets `GraphedUpdate(buckets=...)` replay such updates."""
import numpy as np
import pytest

from test_host_logic import _push, _synth, make_parameter

RAGGED_ENV = 'synthetic-o5-a3-T40'
RAGGED_LENGTHS = np.random.RandomState(5).randint(3, 41, 24)       # early-terminating episodes of an environment with T = 40
FAMILIES = ('smamba_s8_c4_b1_nln', 'gilr', 'lru', 'gru')


def fill_ragged(buf, lengths=RAGGED_LENGTHS, obs=5, act=3, full=40):
    rs = np.random.RandomState(3)
    for n in lengths:
        o, a, r = _synth(rs, int(n), obs, act)
        _push(buf, o, a, r, early_done=(n != full))


def ragged_trainer(rnn, algo='sac', **over):
    """The trainer of the ragged workload: batches of 95 transitions drawn from 24 trajectories of 3..40 steps."""
    from offpolicy_rnn import alg_init
    alg = alg_init(make_parameter(rnn, algo=algo, sac_batch_size=95, env=RAGGED_ENV, **over))
    fill_ragged(alg.replay_buffer)
    return alg


def test_ladder():
    from offpolicy_rnn.buffers.transition_buffer.shape_buckets import ladder
    assert [ladder(x) for x in range(1, 18)] == [1, 2, 3, 4, 6, 6, 8, 8, 12, 12, 12, 12, 16, 16, 16, 16, 24]
    members = {1} | {2 ** k for k in range(1, 14)} | {3 * 2 ** k for k in range(0, 13)}
    for x in range(1, 5001):
        y = ladder(x)
        assert y >= x and ladder(y) == y and y in members, x
        assert y == min(m for m in members if m >= x), x
        if x > 1:
            assert y < 1.5 * x, x


def test_bucket_shape_respects_the_row_capacity():
    from offpolicy_rnn.buffers.transition_buffer.shape_buckets import bucket_shape, ladder
    for cap in (16, 47, 64, 1000, 1024):
        for longest in range(1, cap + 2):
            rows, row_len, nseg = bucket_shape(5, longest, 7, cap)
            assert longest <= row_len <= cap + 1 and (rows, nseg) == (6, 16)
            assert row_len == cap + 1 or (row_len == ladder(row_len) and row_len >= 32)
        assert bucket_shape(1, cap + 1, 1, cap)[1] == cap + 1          # a full row is never padded
    assert [bucket_shape(1, 1, n, 64)[2] for n in (1, 16, 17, 32, 33, 1000)] == [16, 16, 32, 32, 64, 1024]
    assert bucket_shape(2, 501, 3, 1024) == (2, 512, 16) and bucket_shape(4, 1001, 4, 1024) == (4, 1024, 16)


def test_the_module_needs_no_torch():
    import ast
    import offpolicy_rnn.buffers.transition_buffer.shape_buckets as sb
    tree = ast.parse(open(sb.__file__).read())
    names = {a.name.split('.')[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    names |= {(n.module or '').split('.')[0] for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert 'torch' not in names


@pytest.mark.parametrize('nest,hist', [(True, 1), (False, 1), (True, 5)])
def test_planner_with_buckets_draws_the_same_plan(nest, hist):
    from offpolicy_rnn.buffers.transition_buffer.nested_replay_memory import NestedMemoryArray
    from offpolicy_rnn.buffers.transition_buffer.shape_buckets import ladder
    buf = NestedMemoryArray(5000, 40, additional_history_len=hist)
    fill_ragged(buf)
    cap = buf.max_traj_step
    grown_rows = grown_len = 0
    for seed in range(12):
        np.random.seed(seed)
        exact = buf.plan_trajs_device(95, None, nest_stack_trajs=nest)
        st_exact = np.random.get_state()
        np.random.seed(seed)
        pl = buf.plan_trajs_device(95, None, nest_stack_trajs=nest, buckets=True)
        st = np.random.get_state()
        assert st[0] == st_exact[0] and (st[1] == st_exact[1]).all() and st[2:] == st_exact[2:]
        n_real = exact['seg'].shape[0]
        assert 'nrow_real' not in exact and pl['seg'].dtype == np.int32
        np.testing.assert_array_equal(pl['seg'][:n_real], exact['seg'])
        np.testing.assert_array_equal(pl['seg'][n_real:], np.tile(np.int32([-1, 0, 0, 0]), (pl['seg'].shape[0] - n_real, 1)))
        assert pl['total_size'] == exact['total_size']
        assert (pl['nrow_real'], pl['longest_real']) == (exact['nrow'], exact['longest'])
        # the shapes are on the ladder (the row length: or the longest row the planner can emit)
        assert pl['nrow'] == ladder(pl['nrow']) >= exact['nrow'] and pl['nrow'] < 1.5 * exact['nrow'] + 1
        assert pl['longest'] >= exact['longest'] and pl['longest'] >= exact['max_len']
        assert pl['longest'] == cap + 1 or (pl['longest'] == ladder(pl['longest']) and pl['longest'] >= 32)
        assert pl['max_len'] == pl['longest']
        nseg = pl['seg'].shape[0]
        assert nseg >= max(16, n_real) and nseg & (nseg - 1) == 0 and nseg < max(17, 2 * n_real)
        # one table row per batch row: the drawn ones unchanged, [1, 0, ...] (the leading dummy sequence alone) for an empty row
        assert pl['table'].shape == (pl['nrow'], exact['table'].shape[1])
        np.testing.assert_array_equal(pl['table'][:exact['nrow']], exact['table'])
        assert (pl['table'][exact['nrow']:, 0] == 1).all() and not pl['table'][exact['nrow']:, 1:].any()
        grown_rows += pl['nrow'] > exact['nrow']
        grown_len += pl['longest'] > exact['longest']
    assert grown_len and (nest or grown_rows), 'no plan was padded: the cases above checked nothing'


@pytest.mark.parametrize('rnn', FAMILIES)
def test_ragged_batches_have_few_bucketed_shapes(rnn, oracle_ops):
    """24 updates' worth of plans from the real planner (the REDQ subset draw of an update follows each plan on the same numpy
    stream): the exact graph keys hardly recur (20-22 distinct for the packed families, 10 for gru, whose rows are not packed), the
    bucketed ones are 1-4 shapes."""
    from offpolicy_rnn.algorithm.graph_policy import graph_key
    alg = ragged_trainer(rnn)
    par, buf = alg.parameter, alg.replay_buffer
    keys = {}
    for buckets in (False, True):
        np.random.seed(11)
        keys[buckets] = set()
        for _ in range(24):
            pl = buf.plan_trajs_device(par.sac_batch_size, None, random_trunc_traj=par.random_trunc_traj,
                                       nest_stack_trajs=alg.allow_nest_stack, buckets=buckets)
            keys[buckets].add(graph_key(pl, (), buckets, False))
            alg._select_target_ensemble(8)
    print(f'{rnn}: {len(keys[False])} exact keys, {len(keys[True])} bucketed keys in 24 plans: {sorted(keys[True])}')
    assert len(keys[True]) <= 5 and len(keys[False]) >= 10


def test_train_reads_the_bucket_mode_from_the_environment(monkeypatch):
    """`SAC.train()` builds `GraphedUpdate(self, buckets=GraphedUpdate.buckets_from_env())`."""
    import inspect
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    from offpolicy_rnn.algorithm.sac import SAC
    assert 'GraphedUpdate(self, buckets=GraphedUpdate.buckets_from_env())' in inspect.getsource(SAC.train)
    monkeypatch.delenv('RESEL_GRAPH_BUCKETS', raising=False)
    assert GraphedUpdate.buckets_from_env() == 'off'
    for value, mode in (('', 'off'), ('1', 'on'), ('0', 'off'), ('auto', 'auto')):
        monkeypatch.setenv('RESEL_GRAPH_BUCKETS', value)
        assert GraphedUpdate.buckets_from_env() == mode
    for value in ('on', 'off', 'AUTO', '2'):
        monkeypatch.setenv('RESEL_GRAPH_BUCKETS', value)
        with pytest.raises(ValueError, match='RESEL_GRAPH_BUCKETS'):
            GraphedUpdate.buckets_from_env()
    assert inspect.signature(GraphedUpdate.__init__).parameters['buckets'].default == 'off'
