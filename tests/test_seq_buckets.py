"""Buckets of the sequence tables of attention layers (buffers/transition_buffer/shape_buckets.py `pad_seq_tables`) on the host: what
the padding keeps and adds, how few bucketed graph keys a ragged cgpt workload has where its exact keys hardly recur, and the
`seq_buckets` switch of `GraphedUpdate` and of the trainer.  Workload and helpers: tests/test_shape_buckets.py."""
import numpy as np
import pytest

from test_shape_buckets import fill_ragged, ragged_trainer

CGPT = 'cgpt_h1_l2_p0.0_ml64_rms'


def _plans(hist, n_plans=12):
    """(exact tables, bucketed plan, its tables) of `n_plans` draws of the real planner."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    from offpolicy_rnn.buffers.transition_buffer.nested_replay_memory import NestedMemoryArray
    buf = NestedMemoryArray(5000, 40, additional_history_len=hist)
    fill_ragged(buf)
    out = []
    for seed in range(n_plans):
        np.random.seed(seed)
        pl = buf.plan_trajs_device(95, None, nest_stack_trajs=True, buckets=True)
        out.append((pl, GraphedUpdate._build_seqs(pl)))
    return out


@pytest.mark.parametrize('hist', [1, 5])
def test_padding_keeps_the_real_prefix_and_adds_empty_sequences(hist):
    from offpolicy_rnn.buffers.transition_buffer.shape_buckets import ladder, pad_seq_tables
    grown_tok = grown_seq = free = 0
    for pl, built in _plans(hist):
        rows, row_len = pl['nrow'], pl['longest']
        padded, key = pad_seq_tables(built, rows, row_len)
        tb, n_cu, nqb = key
        sb = n_cu - 1
        assert len(padded) == len(built) == 2
        n_max = max(b[0].size for b in built)
        s_max = max(b[1].size - 1 for b in built)
        cap = rows * row_len
        # one bucket for both tables
        assert n_max <= tb <= cap
        assert tb == ladder(tb) or tb == cap or tb == 256
        if tb not in (cap, 256):
            assert tb < 1.5 * n_max
            free += 1
        assert sb >= 16 and sb >= s_max and sb & (sb - 1) == 0 and sb < max(17, 2 * s_max)
        assert nqb == -(-row_len // 128)
        for (idx, cu, mx, table), (idx_p, cu_p, mx_p, table_p) in zip(built, padded):
            n, s = idx.size, cu.size - 1
            assert idx_p.dtype == np.int64 and cu_p.dtype == np.int32 and idx_p.shape == (tb,) and cu_p.shape == (sb + 1,)
            np.testing.assert_array_equal(idx_p[:n], idx)
            np.testing.assert_array_equal(cu_p[:s + 1], cu)
            assert (cu_p[s:] == cu[s]).all() and cu_p[sb] == n                 # empty sequences; the last entry is the real token count
            assert ((idx_p >= 0) & (idx_p < cap)).all()                        # the tail is never read, but it is in range
            assert (np.diff(idx_p[:n]) > 0).all()                              # what the unpack kernel's binary search relies on
            assert mx_p == 128 * nqb >= mx and mx_p >= row_len
            assert table_p is table
            grown_tok += tb > n
            grown_seq += sb > s
    assert grown_tok and grown_seq, 'nothing was padded: the cases above checked nothing'
    print(f'history {hist}: {free} plans with a token bucket between floor and cap')


def test_degenerate_tables():
    from offpolicy_rnn.buffers.transition_buffer.shape_buckets import pad_seq_tables
    from offpolicy_rnn.models.flash_attention.TransformerFlashAttention import PackedSeqs
    empty = PackedSeqs.build_host(np.zeros((2, 8), dtype=np.int32), 8)         # no sequence at all: cu = [0]
    one = PackedSeqs.build_host(np.array([[3, 0, 0, 0, 0, 0, 0, 0], [1, 2, 0, 0, 0, 0, 0, 0]], dtype=np.int32), 8)
    padded, key = pad_seq_tables([one, empty], 2, 8)
    assert key == (16, 17, 1)                                                  # the token bucket is capped by rows * row_len
    assert padded[0][1].tolist() == [0, 3, 4] + [6] * 14 and padded[1][1].tolist() == [0] * 17
    assert padded[0][0][:6].tolist() == [0, 1, 2, 8, 9, 10] and padded[0][2] == 128
    big = PackedSeqs.build_host(np.full((3, 1), 300, dtype=np.int32), 300)
    _, key = pad_seq_tables([big, big], 3, 300)
    assert key == (900, 17, 3)                                                 # ladder(900) = 1024 > 3 * 300
    full = PackedSeqs.build_host(np.full((40, 1), 20, dtype=np.int32), 20)
    _, key = pad_seq_tables([full, full], 48, 32)
    assert key == (1024, 65, 1)                                                # ladder(800) = 1024, 40 sequences -> 64


def test_the_module_still_needs_no_torch():
    import ast
    import offpolicy_rnn.buffers.transition_buffer.shape_buckets as sb
    tree = ast.parse(open(sb.__file__).read())
    names = {a.name.split('.')[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    names |= {(n.module or '').split('.')[0] for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert 'torch' not in names and hasattr(sb, 'pad_seq_tables')


def test_ragged_cgpt_batches_have_few_bucketed_keys(oracle_ops):
    """24 updates' worth of plans (the REDQ subset draw of an update follows each plan on the same numpy stream, as in
    tests/test_shape_buckets.py `test_ragged_batches_have_few_bucketed_shapes`): the exact cgpt graph key - batch shape plus the sizes
    of the two sequence tables - hardly recurs; the bucketed one has as few values as the other families' (cap 5)."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    from offpolicy_rnn.buffers.transition_buffer.shape_buckets import pad_seq_tables
    alg = ragged_trainer(CGPT, algo='td3')
    assert alg._needs_seq_table
    par, buf = alg.parameter, alg.replay_buffer
    keys, batch_keys, growth = {}, set(), 0.0
    for buckets in (False, True):
        np.random.seed(11)
        keys[buckets] = set()
        for _ in range(24):
            pl = buf.plan_trajs_device(par.sac_batch_size, None, random_trunc_traj=par.random_trunc_traj,
                                       nest_stack_trajs=alg.allow_nest_stack, buckets=buckets)
            n = pl['seg'].shape[0]
            built = GraphedUpdate._build_seqs(pl)
            if buckets:
                _, seq_key = pad_seq_tables(built, pl['nrow'], pl['longest'])
                keys[True].add((pl['nrow'], pl['longest'], n) + seq_key)
                batch_keys.add((pl['nrow'], pl['longest'], n))
                growth = max(growth, seq_key[0] / max(b[0].size for b in built))
            else:
                keys[False].add((pl['nrow'], pl['longest'], pl['max_len'], n) + tuple(x for b in built for x in (b[0].size, b[1].size, b[2])))
            alg._select_target_ensemble(8)
    print(f'cgpt: {len(keys[False])} exact keys, {len(keys[True])} bucketed keys ({len(batch_keys)} batch buckets) in 24 plans: '
          f'{sorted(keys[True])}; largest token growth {growth:.2f}x')
    assert len(keys[False]) >= 20
    assert len(keys[True]) <= 5
    assert all(len(k) == 6 for k in keys[True])                                # + the actor flag = the 7 entries of a graph key


def test_seq_buckets_switch_defaults_and_environment(monkeypatch, oracle_ops):
    import inspect
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    from offpolicy_rnn.algorithm.sac import SAC
    from offpolicy_rnn.models.flash_attention.TransformerFlashAttention import PackedSeqs
    sig = inspect.signature(GraphedUpdate.__init__).parameters
    assert sig['seq_buckets'].default is None and sig['buckets'].default == 'off'
    # the constructor reads the variable itself: train()'s call text is pinned (tests/test_shape_buckets.py) and passes no seq_buckets
    assert 'GraphedUpdate(self, buckets=GraphedUpdate.buckets_from_env())' in inspect.getsource(SAC.train)
    assert 'seq_buckets_from_env()' in inspect.getsource(GraphedUpdate.__init__)
    monkeypatch.delenv('RESEL_GRAPH_SEQ_BUCKETS', raising=False)
    assert GraphedUpdate.seq_buckets_from_env() is False
    for value, on in (('', False), ('0', False), ('1', True)):
        monkeypatch.setenv('RESEL_GRAPH_SEQ_BUCKETS', value)
        assert GraphedUpdate.seq_buckets_from_env() is on
    for value in ('on', 'auto', 'true', '2', ' 1'):
        monkeypatch.setenv('RESEL_GRAPH_SEQ_BUCKETS', value)
        with pytest.raises(ValueError, match='RESEL_GRAPH_SEQ_BUCKETS'):
            GraphedUpdate.seq_buckets_from_env()
    # trainer and table defaults: off
    alg = ragged_trainer(CGPT, algo='td3')
    assert alg.seq_buckets is False and alg.shape_buckets is False
    assert PackedSeqs.padded is False
    assert inspect.signature(PackedSeqs.from_static).parameters['padded'].default is False
    idx, cu, mx, tb = PackedSeqs.build_host(np.array([[2, 1]]), 4)
    assert PackedSeqs.from_static(idx, cu, mx, tb).padded is False and PackedSeqs.from_static(idx, cu, mx, tb, padded=True).padded is True
