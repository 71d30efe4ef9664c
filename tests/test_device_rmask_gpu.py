"""Randomised loss masks (`randomize_mask`, equalised form) on the device replay path and in update graphs: the gather kernel applies
the plan's selection bitmap (`resel_gather_trajs_sel`), so the device batch is BIT-EXACT the host batch from the same numpy stream,
updates built from it leave the same parameters, and `GraphedUpdate` replays such updates - and randomly truncated ones - like any
other.  Host half: tests/test_device_rmask.py.  Patterns: tests/test_device_replay_gpu.py, tests/test_graph_buckets_gpu.py."""
import numpy as np
import pytest
import torch

from test_graph_buckets_gpu import _compare, no_noise  # noqa: F401  (fixture)
from test_host_logic import _push, _synth, make_parameter
from test_shape_buckets import ragged_trainer

pytestmark = pytest.mark.gpu
LONG_ENV = 'synthetic-o5-a3-T45'                      # rows of 64 slots: one trajectory of 45 steps crosses a bitmap word


def _trainer(lengths, rnn='gru', seed=3, env=LONG_ENV, full=45, **over):
    from offpolicy_rnn import alg_init
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter(rnn, sac_batch_size=40, cuda_inference=True, env=env, **over))
    rs = np.random.RandomState(seed)
    for n in lengths:
        o, a, r = _synth(rs, n, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=(n != full))
    return alg


def _same_state(a, b):
    return a[0] == b[0] and (a[1] == b[1]).all() and a[2:] == b[2:]


# ------------------------------------------------------------------------------------------------------------ 1. bit-exact batch
@pytest.mark.parametrize('rnn', ['gru', 'smamba_s8_c4_b1_nln'])          # skip_step 2 and 6
@pytest.mark.parametrize('kw', [dict(nest_stack_trajs=True), dict(nest_stack_trajs=False), dict(nest_stack_trajs=True, random_trunc_traj=True)])
def test_device_batch_with_randomised_mask_is_bit_exact(rnn, kw):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    alg = _trainer((12, 5, 7, 12, 9, 3, 12, 6, 45), rnn)
    buf = alg.replay_buffer
    m0 = buf.name2range['mask'][0]
    buf.memory_buffer[[2, 60], m0] = 0                # two stored masks of 0: they stay 0 whatever the selection says
    buf._dirty = None                                 # the device mirror takes the whole ring again
    thinned = 0
    for k in (16, 1, 1000):
        for seed in (1, 2, 3):
            np.random.seed(seed)
            batch, size_h, valid, table_h = buf.sample_trajs(40, None, equalize_data_of_each_traj=True, randomize_mask=True,
                                                             valid_number_post_randomized=k, **kw)
            host = alg._upload_batch(batch, valid, table_h)['state']._base
            st_h = np.random.get_state()
            np.random.seed(seed)
            dev, size_d, table_d = buf.sample_trajs_device(alg.device, 40, None, randomize_mask=True, valid_number_post_randomized=k, **kw)
            torch.cuda.synchronize()
            assert _same_state(st_h, np.random.get_state()), 'the two paths consumed different numpy draws'
            assert host.shape == dev.shape and size_h == size_d and np.array_equal(table_h, table_d)
            assert torch.equal(host, dev), f'k {k} seed {seed}: {int((host != dev).sum())} differing entries'
            thinned += int(dev[..., m0].sum().item() < dev[..., -3].sum().item())      # loss mask thinner than validity
    assert thinned >= 6, 'the selection hardly cleared anything: the comparison checked nothing'


# ---------------------------------------------------------------------------------------------------------- 2. plan robustness
def test_dropped_entries_and_out_of_range_bitmaps_keep_their_masks():
    """A plan entry with row -1 never reads the selection; an entry whose bitmap would reach outside the words part (one word too far,
    or a negative offset) keeps all its masks: its slots equal the gather without a selection, nothing else differs."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    alg = _trainer((12, 5, 7, 12, 9, 3, 12, 6, 45))
    buf, dev = alg.replay_buffer, alg.device
    np.random.seed(2)
    pl = buf.plan_trajs_device(40, None, randomize_mask=True, valid_number_post_randomized=1)
    n = pl['seg'].shape[0]
    seg = np.concatenate((pl['seg'], np.int32([[-1, 0, 0, 0]])))
    good = np.concatenate((pl['sel'][:n], np.int32([1 << 30]), pl['sel'][n:]))         # the dropped entry's offset is never looked at
    last = int(np.argmax(pl['sel'][:n]))                                               # the entry whose words end the array
    first = int(np.argmin(pl['sel'][:n]))
    assert last != first
    bad = good.copy()
    bad[last] += 1                                                                     # one word past the end
    bad[first] = -1
    seg_dev = torch.from_numpy(seg).to(dev)

    def gather(sel):
        out = buf.gather_planned(dev, seg_dev, pl['max_len'], pl['nrow'], pl['longest'], sel_dev=None if sel is None else torch.from_numpy(sel).to(dev))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    plain, want, got = gather(None), gather(good), gather(bad)
    np.random.seed(2)
    ref = buf.sample_trajs_device(dev, 40, None, randomize_mask=True, valid_number_post_randomized=1)[0].cpu().numpy()
    np.testing.assert_array_equal(want, ref)                                           # the extra dropped entry changes nothing
    touched = np.zeros(plain.shape[:2], dtype=bool)
    for e in (first, last):
        r, pos, ln, _ = pl['seg'][e]
        touched[r, pos:pos + ln] = True
        assert (want[r, pos:pos + ln] != plain[r, pos:pos + ln]).any(), 'the selection cleared nothing in this entry'
    np.testing.assert_array_equal(got[touched], plain[touched])
    np.testing.assert_array_equal(got[~touched], want[~touched])


# ------------------------------------------------------------------------------------------------------- 3. update equivalence
def test_update_with_device_built_randomised_mask_equals_host_replay():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    out = []
    for device_replay in (False, True):
        alg = _trainer((12, 5, 7, 12, 9), 'gilr', env='synthetic-o5-a3-T12', full=12, randomize_mask=True, valid_number_post_randomized=16)
        alg.device_replay = device_replay
        torch.manual_seed(11); torch.cuda.manual_seed_all(11); np.random.seed(11)
        for _ in range(2):
            alg.train_one_batch()
            alg.grad_num += 1
        torch.cuda.synchronize()
        out.append((alg.policy.store.flat.clone(), alg.values[0].store.flat.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# -------------------------------------------------------------------------------------------------------------------- 4. graphs
def _fixed_trainer(rnn, **over):
    from offpolicy_rnn import alg_init
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter(rnn, sac_batch_size=4 * 12 - 1, cuda_inference=True, **over))
    rs = np.random.RandomState(3)
    for _ in range(8):
        o, a, r = _synth(rs, 12, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=False)
    np.random.seed(11)
    return alg


def _ragged(rnn, **over):
    torch.manual_seed(0)
    np.random.seed(0)
    alg = ragged_trainer(rnn, cuda_inference=True, **over)
    np.random.seed(11)
    return alg


def _run_pair(what, build, n_upd, buckets):
    """`n_upd` eager updates against `n_upd` `GraphedUpdate.step()` calls from the same seeds; the valid count of every stepped update
    (sum of the loss mask, the trainer's `_stats[1]`) against the plan: the selected positions, or every transition without a selection."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    eager = build()
    eager.shape_buckets = buckets == 'on'
    logs_e = []
    for _ in range(n_upd):
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    graphed = build()
    assert GraphedUpdate.refusal(graphed) is None
    g = GraphedUpdate(graphed, warmup=1, buckets=buckets)
    logs_g, thinned = [], 0
    for _ in range(n_upd):
        logs_g.append(dict(g.step()))
        graphed.grad_num += 1
        torch.cuda.synchronize()
        pl = g._plan
        want = pl['total_size']
        if 'sel' in pl:
            want = int(np.unpackbits(pl['sel'][pl['seg'].shape[0]:].view(np.uint8)).sum())     # bits behind a segment's last position are 0
            thinned += want < pl['total_size']
        assert float(graphed._stats[1]) == want, (float(graphed._stats[1]), want, pl['total_size'])
    print(f'MEASURED {what}: graphs {sorted(g.graphs)}, eager updates {g.eager_fallbacks} of {n_upd}, thinned updates {thinned}')
    assert g.eager_fallbacks < n_upd and len(g.graphs) >= 1, 'no update was a replay'
    if graphed.parameter.randomize_mask:
        assert thinned == n_upd
    _compare(what, graphed, eager, logs_g, logs_e, rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize('rnn', ['gilr', 'smamba_s8_c4_b1_nln'])
def test_graphed_updates_with_randomised_mask_equal_the_eager_updates(rnn, no_noise):
    _run_pair(f'{rnn} rmask replay vs eager', lambda: _fixed_trainer(rnn, randomize_mask=True, valid_number_post_randomized=16), 4, 'off')


@pytest.mark.parametrize('rnn', ['gilr', 'smamba_s8_c4_b1_nln'])
def test_graphed_updates_with_truncation_equal_the_eager_updates(rnn, no_noise):
    _run_pair(f'{rnn} trunc replay vs eager', lambda: _ragged(rnn, random_trunc_traj=True), 4, 'on')


# ------------------------------------------------------------------------------------------------------- 5. bucketed mask run
@pytest.mark.parametrize('rnn', ['gilr', 'smamba_s8_c4_b1_nln'])
def test_bucketed_replays_with_randomised_mask_equal_the_eager_updates(rnn, no_noise):
    _run_pair(f'{rnn} rmask bucketed replay vs eager', lambda: _ragged(rnn, randomize_mask=True, valid_number_post_randomized=16), 8, 'on')
