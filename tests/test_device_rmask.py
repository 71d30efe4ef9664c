"""Randomised loss masks on the device replay path, host half (buffers/transition_buffer/nested_replay_memory.py `plan_trajs_device(...,
randomize_mask=True)`): the plan's `sel` bitmap, decoded in pure numpy, is the mask `sample_trajs(..., equalize_data_of_each_traj=True)`
builds from the same seed - same numpy stream consumption, with truncation, packing, both skip lengths and the quirks of the host
expression (`k = 0` and `k >= n` keep every position); `shape_buckets.pad_plan` keeps it decodable."""
import numpy as np
import pytest

from test_host_logic import _push, _synth

LENGTHS = (12, 5, 7, 45, 9, 3, 12, 6, 33)             # 45 and 33 data positions: bitmaps that cross a 32-bit word boundary
BATCH = 100


def _buffer(hist):
    from offpolicy_rnn.buffers.transition_buffer.nested_replay_memory import NestedMemoryArray
    buf = NestedMemoryArray(1000, 64, additional_history_len=hist)
    rs = np.random.RandomState(7)
    for n in LENGTHS:
        o, a, r = _synth(rs, n, 4, 2)
        _push(buf, o, a, r, early_done=(n != 12))
    return buf


def decode(buf, pl, use_sel=True):
    """The mask column [rows, T', 1] a gather of this plan writes: stored masks placed by the plan, cleared where the bit is 0."""
    m0, skip = buf.name2range['mask'][0], buf._skip_step
    seg = pl['seg']
    nseg = seg.shape[0]
    out = np.zeros((pl['nrow'], pl['longest'], 1), dtype=np.float32)
    if use_sel:
        sel = pl['sel']
        assert sel.dtype == np.int32 and sel.ndim == 1
        off, words = sel[:nseg], sel[nseg:].view(np.uint32)
    for s, (r, pos, n, first) in enumerate(seg):
        if r < 0:
            continue
        stored = buf.memory_buffer[first:first + n - skip, m0]
        if use_sel:
            p = np.arange(n - skip)
            stored = stored * ((words[off[s] + (p >> 5)] >> (p & 31).astype(np.uint32)) & 1)
        out[r, pos + skip:pos + n, 0] = stored
    return out


def _same_state(a, b):
    return a[0] == b[0] and (a[1] == b[1]).all() and a[2:] == b[2:]


@pytest.mark.parametrize('trunc', [False, True])
@pytest.mark.parametrize('k', [9, 1, 0, 1000])
@pytest.mark.parametrize('nest', [True, False])
@pytest.mark.parametrize('hist', [1, 5])                                     # skip 2 and 6
def test_plan_selection_decodes_to_the_host_mask(hist, nest, k, trunc):
    from offpolicy_rnn.buffers.transition_buffer.shape_buckets import pad_plan
    buf = _buffer(hist)
    skip = buf._skip_step
    grown = 0
    for seed in (1, 2, 3):
        np.random.seed(seed)
        res, total, valid, table = buf.sample_trajs(BATCH, None, randomize_mask=True, valid_number_post_randomized=k,
                                                    equalize_data_of_each_traj=True, random_trunc_traj=trunc, nest_stack_trajs=nest)
        host_mask, st_host = res.mask.copy(), np.random.get_state()
        np.random.seed(seed)
        pl = buf.plan_trajs_device(BATCH, None, random_trunc_traj=trunc, nest_stack_trajs=nest, randomize_mask=True,
                                   valid_number_post_randomized=k)
        assert _same_state(st_host, np.random.get_state()), 'the two paths consumed different numpy draws'
        assert pl['total_size'] == total
        np.testing.assert_array_equal(pl['table'], table)
        assert host_mask.shape == (pl['nrow'], pl['longest'], 1)
        got = decode(buf, pl)
        np.testing.assert_array_equal(got, host_mask)
        np.testing.assert_array_equal(decode(buf, pl, use_sel=False), valid)          # validity: the stored masks, untouched
        # the sum: k positions of a trajectory of n where 0 < k < n, all n otherwise (`[:-0]` and `[:-k]` with k >= n are empty)
        lens = [int(n) for n in pl['seg'][:, 2]]
        ks = buf.get_equalized_valid_num_each_traj(lens, k)
        want = sum(kk if 0 < kk < n - skip else n - skip for kk, n in zip(ks, lens))
        assert host_mask.sum() == want == got.sum()
        if k == 9 and not trunc:
            assert want < total, 'nothing was thinned: the case checks nothing'
        if k in (0, 1000):
            assert want == total
        # bucketed: the offset header grows with the plan, the words follow - the same mask plus padding
        pb = pad_plan(pl, buf.max_traj_step)
        assert pb['sel'].size == pl['sel'].size + pb['seg'].shape[0] - pl['seg'].shape[0] and pb['sel'].dtype == np.int32
        padded = decode(buf, pb)
        assert padded.shape == (pb['nrow'], pb['longest'], 1)
        grown += pb['seg'].shape[0] > pl['seg'].shape[0]
        np.testing.assert_array_equal(padded[:pl['nrow'], :pl['longest']], host_mask)
        assert padded.sum() == host_mask.sum()
        np.random.seed(seed)
        direct = buf.plan_trajs_device(BATCH, None, random_trunc_traj=trunc, nest_stack_trajs=nest, buckets=True, randomize_mask=True,
                                       valid_number_post_randomized=k)
        np.testing.assert_array_equal(direct['sel'], pb['sel'])
        np.testing.assert_array_equal(direct['seg'], pb['seg'])
    assert grown, 'no offset header was padded: the bucketed decode checked nothing'


def test_zeroed_stored_masks_stay_zero():
    """A stored mask of 0 stays 0 whether or not its position is selected (the bitmap keeps or clears, it never sets)."""
    buf = _buffer(1)
    m0 = buf.name2range['mask'][0]
    buf.memory_buffer[[3, 40], m0] = 0
    np.random.seed(4)
    res, *_ = buf.sample_trajs(BATCH, None, randomize_mask=True, valid_number_post_randomized=9, equalize_data_of_each_traj=True)
    host_mask = res.mask.copy()
    np.random.seed(4)
    pl = buf.plan_trajs_device(BATCH, None, randomize_mask=True, valid_number_post_randomized=9)
    np.testing.assert_array_equal(decode(buf, pl), host_mask)


@pytest.mark.parametrize('nest', [True, False])
def test_plans_without_the_flag_are_unchanged(nest):
    from offpolicy_rnn.buffers.transition_buffer.shape_buckets import pad_plan
    buf = _buffer(1)
    np.random.seed(5)
    plain = buf.plan_trajs_device(BATCH, None, nest_stack_trajs=nest)
    st = np.random.get_state()
    np.random.seed(5)
    again = buf.plan_trajs_device(BATCH, None, nest_stack_trajs=nest, randomize_mask=False, valid_number_post_randomized=9)
    assert _same_state(st, np.random.get_state())
    assert set(plain) == set(again) == {'seg', 'max_len', 'nrow', 'longest', 'total_size', 'table'}
    np.random.seed(5)
    flagged = buf.plan_trajs_device(BATCH, None, nest_stack_trajs=nest, randomize_mask=True, valid_number_post_randomized=9)
    assert set(flagged) == set(plain) | {'sel'}
    pp, pf = pad_plan(plain, buf.max_traj_step), pad_plan(flagged, buf.max_traj_step)
    assert set(pp) == set(plain) | {'nrow_real', 'longest_real'} and set(pf) == set(pp) | {'sel'}
    n = plain['seg'].shape[0]
    np.testing.assert_array_equal(pp['seg'][:n], plain['seg'])
    np.testing.assert_array_equal(pp['seg'][n:], np.tile(np.int32([-1, 0, 0, 0]), (pp['seg'].shape[0] - n, 1)))
    for key in pp:                                    # the selection changes nothing else of a plan, padded or not
        np.testing.assert_array_equal(pp[key], pf[key], err_msg=key)
        if key in plain:
            np.testing.assert_array_equal(plain[key], flagged[key], err_msg=key)


def test_device_supported():
    buf = _buffer(1)
    assert buf.device_supported() and buf.device_supported(randomize_mask=False)
    assert buf.device_supported(randomize_mask=True) and buf.device_supported(randomize_mask=True, equalize_data_of_each_traj=True)
    assert not buf.device_supported(randomize_mask=True, equalize_data_of_each_traj=False)      # the whole-batch form stays host-only
    assert buf.device_supported(randomize_mask=False, equalize_data_of_each_traj=False)
