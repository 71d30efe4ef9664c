"""Host side of the selective scan's state sizes 1 to 256 (GPU side: tests/test_sscan_states_gpu.py).

1. `ops.sscan_state_plan`: the table of groups for native, padded and grouped sizes, the padded width and the real count per group, and
   what is refused.
2. The three "state groups" entries exist in the header, in the ctypes table and in the built library, under ABI 11.
3. Their argument checks return RESEL_EINVAL before the device is touched (pointers here are fake and never dereferenced)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESEL_EINVAL = -1
ENTRIES = ('resel_sscan_gate_fwd', 'resel_sscan_gate_bwd_workspace_bytes', 'resel_sscan_gate_bwd', 'resel_sscan_group_reduce')

PLANS = {
    4: [(0, 4, 4)], 16: [(0, 16, 16)], 64: [(0, 64, 64)],
    12: [(0, 12, 16)], 24: [(0, 24, 32)], 40: [(0, 40, 64)],
    65: [(0, 64, 64), (64, 1, 4)],
    72: [(0, 64, 64), (64, 8, 8)],
    96: [(0, 64, 64), (64, 32, 32)],
    100: [(0, 64, 64), (64, 36, 64)],
    128: [(0, 64, 64), (64, 64, 64)],
    200: [(0, 64, 64), (64, 64, 64), (128, 64, 64), (192, 8, 8)],
    256: [(0, 64, 64), (64, 64, 64), (128, 64, 64), (192, 64, 64)],
}
PADDED = {4: 4, 12: 16, 16: 16, 24: 32, 40: 64, 64: 64, 65: 68, 72: 72, 96: 96, 100: 128, 128: 128, 200: 200, 256: 256}


def test_plan_table():
    from offpolicy_rnn.hip import ops
    assert {N: ops.sscan_state_plan(N) for N in PLANS} == PLANS
    assert {N: ops.sscan_padded_states(ops.sscan_state_plan(N)) for N in PADDED} == PADDED


def test_every_size_is_covered_once_by_native_kernels_and_only_the_last_group_is_padded():
    from offpolicy_rnn.hip import ops
    for N in range(1, 257):
        plan = ops.sscan_state_plan(N)
        assert 1 <= len(plan) <= ops.SSCAN_MAX_GROUPS == 4
        assert [f for f, _, _ in plan] == [sum(s for _, s, _ in plan[:i]) for i in range(len(plan))] and sum(s for _, s, _ in plan) == N
        assert all(k in ops.SSCAN_NATIVE_STATES and 1 <= s <= k for _, s, k in plan)
        assert all(s == k == 64 for _, s, k in plan[:-1])
        f, s, k = plan[-1]
        assert k == min(w for w in ops.SSCAN_NATIVE_STATES if w >= s)                  # the smallest native size that holds the remainder
        assert ops.sscan_padded_states(plan) == f + k
        if N in ops.SSCAN_NATIVE_STATES:
            assert plan == [(0, N, N)]


@pytest.mark.parametrize('N', [0, -3, 257, 300])
def test_sizes_outside_1_to_256_are_refused_with_the_range_and_the_bound(N):
    from offpolicy_rnn.hip import ops
    with pytest.raises(ValueError, match=r'accepted are 1 to 256 .*256 is this build\'s bound: 4 groups'):
        ops.sscan_state_plan(N)


def test_entries_are_declared_bound_and_built():
    from offpolicy_rnn.hip import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'resel_hip.h')).read()
    for name in ENTRIES:
        assert f' {name}(' in header, name
        assert name in _lib.SIGNATURES, name
    assert '#define RESEL_SSCAN_MAX_GROUPS 4' in header and 'N in {4, 8, 16, 32, 64} (any other N: RESEL_EINVAL)' in header
    for slot, kid in (('sscan_gate_fwd_kernel', 16), ('sscan_gate_bwd_kernel', 17), ('sscan_group_reduce_kernel', 18)):
        assert ops.PROF_SLOTS[kid] == slot and f'RESEL_PROF_{slot[:-7].upper()} = {kid}' in header
    assert len(ops.PROF_SLOTS) == 19 and 'RESEL_PROF_NSLOTS = 19' in header
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(h, name) for name in ENTRIES)
    h.resel_abi_version.restype = ctypes.c_int
    assert h.resel_abi_version() == _lib.ABI_VERSION == 11


@pytest.fixture(scope='module')
def lib():
    from offpolicy_rnn.hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


FAKE = 4096                          # 16-byte aligned, never dereferenced: every call below returns before anything is enqueued
M, DI = 10, 8


def test_gate_fwd_argument_checks(lib):
    def call(parts=FAKE, stride_g=M * DI, G=2, u=FAKE, ld_u=DI, D=FAKE, z=FAKE, ld_z=DI, out=FAKE, ld_out=DI, rows=M, Di=DI, amax=None):
        return lib.resel_sscan_gate_fwd(parts, stride_g, G, u, ld_u, D, z, ld_z, out, ld_out, rows, Di, amax, 0, None)

    for kw in (dict(parts=None), dict(out=None), dict(u=None), dict(G=0), dict(G=5), dict(rows=0), dict(Di=6), dict(Di=0),
               dict(stride_g=M * DI - 4), dict(stride_g=M * DI + 2), dict(ld_u=4), dict(ld_z=6), dict(ld_out=4),
               dict(parts=FAKE + 4), dict(z=FAKE + 8), dict(out=FAKE + 4), dict(D=FAKE + 4), dict(amax=FAKE + 4)):
        assert call(**kw) == RESEL_EINVAL, kw


def test_gate_bwd_argument_checks(lib):
    def call(dout=FAKE, ld_dout=DI, parts=FAKE, stride_g=M * DI, G=2, u=FAKE, ld_u=DI, D=FAKE, z=FAKE, ld_z=DI, g=FAKE, ld_g=DI, dz=FAKE,
             ld_dz=DI, dD=FAKE, ws=FAKE, rows=M, Di=DI, amax=None):
        return lib.resel_sscan_gate_bwd(dout, ld_dout, parts, stride_g, G, u, ld_u, D, z, ld_z, g, ld_g, dz, ld_dz, dD, ws, rows, Di, amax, 0, None)

    for kw in (dict(dout=None), dict(parts=None), dict(u=None), dict(ws=None), dict(G=0), dict(G=5), dict(rows=0), dict(Di=6),
               dict(z=None), dict(dz=None), dict(g=None), dict(D=None), dict(dD=None),            # z / dz / g and D / dD come and go together
               dict(z=None, dz=None, g=None, D=None, dD=None),                                    # nothing to form
               dict(stride_g=M * DI - 4), dict(ld_dout=4), dict(ld_g=6), dict(ld_dz=4), dict(ld_z=4), dict(ld_u=4),
               dict(dout=FAKE + 4), dict(g=FAKE + 8), dict(ws=FAKE + 4), dict(amax=FAKE + 4)):
        assert call(**kw) == RESEL_EINVAL, kw
    assert lib.resel_sscan_gate_bwd_workspace_bytes(0, DI) == 0
    assert lib.resel_sscan_gate_bwd_workspace_bytes(129, DI) == 2 * 4 * DI * 4               # 128 rows per block, one partial row per wave


def test_group_reduce_argument_checks(lib):
    def call(du_p=FAKE, dd_p=FAKE, stride_g=M * DI, db_p=FAKE, G=2, g=FAKE, ld_g=DI, D=FAKE, du=FAKE, ld_du=DI, dd=FAKE, ld_dd=DI, dbias=FAKE,
             rows=M, Di=DI, amax=None):
        return lib.resel_sscan_group_reduce(du_p, dd_p, stride_g, db_p, G, g, ld_g, D, du, ld_du, dd, ld_dd, dbias, rows, Di, amax, 0, None)

    for kw in (dict(du_p=None), dict(dd_p=None), dict(du=None), dict(dd=None), dict(g=None), dict(db_p=None), dict(dbias=None),
               dict(G=0), dict(G=5), dict(rows=0), dict(Di=6), dict(stride_g=M * DI - 4), dict(ld_g=4), dict(ld_du=6), dict(ld_dd=4),
               dict(du_p=FAKE + 4), dict(dd=FAKE + 8), dict(dbias=FAKE + 4), dict(amax=FAKE + 4)):
        assert call(**kw) == RESEL_EINVAL, kw
