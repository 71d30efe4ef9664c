"""Multi-network GRU forward (`resel_gru_multi_*`): what can be checked without a GPU - the workspace size and the argument checks that
return before the device is touched.  The library loads on a CPU-only machine (`resel_abi_version()` is called that way too)."""
import ctypes
import os

import pytest

RESEL_EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    from offpolicy_rnn.hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('resel_gru_workspace_bytes', 'resel_gru_multi_workspace_bytes', 'resel_gru_multi_fwd', 'resel_gru_multi_form'):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


@pytest.mark.parametrize('B,L,H', [(64, 1027, 256), (8, 131, 256), (5, 33, 48), (6, 21, 192), (6, 17, 384), (4, 9, 512)])
def test_multi_workspace_holds_n_single_workspaces(lib, B, L, H):
    single = lib.resel_gru_workspace_bytes(B, L, H)
    for n in (1, 2, 3, 4):
        got = lib.resel_gru_multi_workspace_bytes(n, B, L, H)
        assert got >= n * single and got % 16 == 0, (n, got, single)


def test_multi_fwd_rejects_bad_arguments_before_touching_the_device(lib):
    """Nothing here is a device pointer: a call that got past the argument checks would fault, not return."""
    B, L, H = 4, 3, 32
    fake = 0x1000                                                  # 16-byte aligned, never dereferenced
    VP = ctypes.c_void_p

    def arrays(n, **override):
        a = {k: (VP * max(n, 1))(*[fake] * max(n, 1)) for k in ('gi', 'w_hh', 'b_hh', 'h0', 'h_all', 'gates')}
        a.update(override)
        return a

    def call(n, a, B=B, L=L, H=H, ws=fake):
        return lib.resel_gru_multi_fwd(n, a['gi'], a['w_hh'], a['b_hh'], a['h0'], a['h_all'], a['gates'], ws, B, L, H, None)

    assert call(0, arrays(1)) == RESEL_EINVAL                       # n_net out of range
    assert call(5, arrays(5)) == RESEL_EINVAL
    for key in ('gi', 'w_hh', 'b_hh', 'h_all'):                     # a NULL array
        assert call(2, arrays(2, **{key: None})) == RESEL_EINVAL, key
    for key in ('gi', 'w_hh', 'b_hh', 'h_all'):                     # a NULL required entry
        assert call(2, arrays(2, **{key: (VP * 2)(fake, None)})) == RESEL_EINVAL, key
    assert call(2, arrays(2), ws=None) == RESEL_EINVAL
    assert call(2, arrays(2), H=40) == RESEL_EINVAL                 # H not a multiple of 16
    assert call(2, arrays(2), H=528) == RESEL_EINVAL                # H > 512
    assert call(2, arrays(2), H=272) == RESEL_EINVAL                # no reduction split for this width (as resel_gru_seq_fwd)
    assert call(2, arrays(2), B=0) == RESEL_EINVAL
    assert call(2, arrays(2, h_all=(VP * 2)(fake, fake + 4))) == RESEL_EINVAL       # misaligned output
    assert lib.resel_gru_multi_form(0, B, H) == RESEL_EINVAL and lib.resel_gru_multi_form(5, B, H) == RESEL_EINVAL
    assert lib.resel_gru_multi_form(2, B, 40) == RESEL_EINVAL
