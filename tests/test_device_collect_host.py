"""`MemoryArray.push_rows` (the ring side of the on-device training rollout, utility/device_collect.py) against `mem_push`: the
same ring, row for row and table for table, through eviction and a wrapping `ptr`; the refusals; the ctypes form of the kernel's
layout struct and the entry's host-side validation.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from offpolicy_rnn.buffers.transition_buffer.replay_memory import MemoryArray, Transition, tuplenames

CAPACITY, TRAJ = 20, 6                                          # 20 rows hold three trajectories of 6: the fourth evicts and wraps


def _transition(rs, t, n):
    """One step of a T-Maze-shaped trajectory as `SAC._push` builds it (observations 2 wide, one-hot last action, index action)."""
    f32 = lambda *s: rs.randn(*s).astype(np.float32)
    one_hot = np.zeros((1, 4))
    one_hot[0, rs.randint(4)] = 1
    return Transition(state=f32(1, 2), last_state=f32(1, 2), last_action=one_hot, action=np.array([[rs.randint(4)]], dtype=np.int64),
                      next_state=f32(1, 2), reward=float(rs.randn()) * (1.0 / 3.0) if t % 2 else -0.0, logp=None, mask=1, done=t == n - 1,
                      timeout=t + 1 >= n, start=t == 0, reward_input=np.array([[rs.randn()]]))


def _tables(m):
    return dict(trajectory_start=list(m.trajectory_start), trajectory_length=list(m.trajectory_length), ptr=m.ptr,
                transition_count=m.transition_count, dirty=list(m._dirty), size=m.size, trajs=len(m), pending=len(m.memory))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_push_rows_equals_mem_push_through_eviction_and_wrap():
    rs = np.random.RandomState(0)
    one, bulk = MemoryArray(CAPACITY, TRAJ), MemoryArray(CAPACITY, TRAJ)
    lengths = [TRAJ, TRAJ, TRAJ, TRAJ, 4, TRAJ, 1, TRAJ, TRAJ, 5]
    seen_wrap = seen_evict = False
    for k, n in enumerate(lengths):
        traj = [_transition(rs, t, n) for t in range(n)]
        for tr in traj:
            one.mem_push(tr)
        if k == 0:                                             # the first trajectory fixes the column layout
            for tr in traj:
                bulk.mem_push(tr)
        else:
            before = (bulk.ptr, len(bulk))
            rows = np.concatenate([bulk.transition_to_array(tr) for tr in traj], axis=0)
            assert rows.dtype == np.float32 and rows.shape == (n, bulk.width)
            bulk.push_rows(rows)
            rows[:] = 7.0                                      # the ring took a copy
            seen_wrap |= bulk.ptr < before[0]
            seen_evict |= len(bulk) <= before[1]
        assert _tables(one) == _tables(bulk), k
        assert np.array_equal(_bits(one.memory_buffer), _bits(bulk.memory_buffer)), k       # every row of the ring, -0.0 included
        assert one.name2range == bulk.name2range and bulk.memory == []
    assert seen_wrap and seen_evict and one.transition_count <= CAPACITY
    assert (one.memory_buffer.view(np.int32) == np.float32(-0.0).view(np.int32)).any()  # a negative zero was stored and compared
    np.random.seed(3)
    a = one.sample_transitions(8)
    np.random.seed(3)
    b = bulk.sample_transitions(8)
    for name, x, y in zip(tuplenames, a, b):
        assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y)), name


def test_push_rows_refuses_a_pending_partial_trajectory_and_bad_rows():
    rs = np.random.RandomState(1)
    m = MemoryArray(CAPACITY, TRAJ)
    with pytest.raises(RuntimeError, match='no column layout'):
        m.push_rows(np.zeros((2, 17), dtype=np.float32))
    for t in range(TRAJ):
        m.mem_push(_transition(rs, t, TRAJ))
    rows = m.memory_buffer[:TRAJ].copy()
    m.mem_push(_transition(rs, 0, TRAJ))                        # an episode is under way on the host side
    before, ring = _tables(m), m.memory_buffer.copy()
    with pytest.raises(RuntimeError, match='unfinished trajectory'):
        m.push_rows(rows)
    assert _tables(m) == before and np.array_equal(m.memory_buffer, ring)
    m.memory = []
    for bad in (rows.astype(np.float64), rows[:, :-1], rows[0], rows[:0]):
        with pytest.raises(ValueError, match='push_rows'):
            m.push_rows(bad)
    assert _tables(m) == dict(before, pending=0) and np.array_equal(m.memory_buffer, ring)
    m.push_rows(rows)
    assert m.trajectory_start == [0, TRAJ] and m.trajectory_length == [TRAJ, TRAJ] and m._dirty == [(0, TRAJ), (TRAJ, TRAJ)]


def test_layout_struct_and_the_entry_s_refusals():
    """`resel_collect_layout_t` is twelve int32 in the ring's field order, and the entry refuses bad arguments before it touches a device."""
    from offpolicy_rnn.hip import _lib
    assert _lib.COLLECT_FIELDS == tuplenames
    assert ctypes.sizeof(_lib.CollectLayout) == 48 and [n for n, _ in _lib.CollectLayout._fields_] == list(tuplenames)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    fn = h.resel_tmaze_collect_step
    fn.restype, fn.argtypes = _lib.SIGNATURES['resel_tmaze_collect_step']
    cfg = _lib.TMazeCfg(3, 0, 4, 1.0, -1.0 / 3.0, 0.0)
    ring = MemoryArray(CAPACITY, TRAJ)
    ring.mem_push(_transition(np.random.RandomState(2), 0, 1))
    assert ring.width == 17

    def layout(**over):
        lay = _lib.CollectLayout()
        for name in tuplenames:
            a, b = ring.name2range[name]
            setattr(lay, name, a if b > a else -1)
        for k, v in over.items():
            setattr(lay, k, v)
        return lay

    assert layout().logp == -1 and layout().timeout == 16
    p = ctypes.c_void_p(4096)                                   # never dereferenced: every call below is refused on the host (or B == 0)
    base = dict(cfg=cfg, lay=layout(), init=0, action=p, ld_action=6, goal=p, env_state=p, ret_acc=p, traj=p, T_cap=4, ld_row=17,
                max_episode_steps=4, in_block=p, ld_in=9, A=4, B=0, stream=None)
    call = lambda **over: fn(*dict(base, **over).values())
    assert call() == 0                                          # B == 0: nothing launched
    for over in (dict(action=None), dict(goal=None), dict(env_state=None), dict(ret_acc=None), dict(traj=None), dict(in_block=None),
                 dict(A=3), dict(B=-1), dict(T_cap=0), dict(max_episode_steps=0), dict(ld_in=8), dict(ld_action=0), dict(ld_row=16),
                 dict(lay=layout(logp=5)), dict(lay=layout(last_action=14)), dict(lay=layout(timeout=17)),
                 dict(cfg=_lib.TMazeCfg(0, 0, 4, 1.0, 0.0, 0.0)), dict(cfg=_lib.TMazeCfg(3, 0, 4, 1.0, 0.5, 0.0))):
        assert call(**over) == -1, over
    assert call(lay=layout(timeout=-1), ld_row=16) == 0         # an absent field needs no column
