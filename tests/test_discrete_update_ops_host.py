"""The discrete-action update entries (`resel_categorical_fwd / _bwd`, `resel_discrete_value`, `resel_q_taken_loss_*`,
`resel_discrete_actor_loss_*`): the argument checks that return before the device is touched.  The library loads on a CPU-only machine;
nothing here is a device pointer, so a call that got past the checks with M > 0 would fault instead of returning."""
import ctypes
import os
import re

import pytest

RESEL_EINVAL = -1
FAKE = 0x1000                                                      # 16-byte aligned, never dereferenced
NAMES = ('resel_categorical_fwd', 'resel_categorical_bwd', 'resel_discrete_value', 'resel_q_taken_loss_fwd', 'resel_q_taken_loss_bwd',
         'resel_discrete_actor_loss_fwd', 'resel_discrete_actor_loss_bwd')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from offpolicy_rnn.hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


def max_actions():
    header = open(os.path.join(ROOT, 'include', 'resel_hip.h')).read()
    return int(re.search(r'#define\s+RESEL_CATEGORICAL_MAX_ACTIONS\s+(\d+)', header).group(1))


# name -> (pointer arguments in order, the ones that may be NULL, trailing non-shape arguments); shapes are (E, M, A) or (M, A)
ENTRIES = {
    'resel_categorical_fwd': (('logits', 'logp', 'probs', 'mode'), (), False),
    'resel_categorical_bwd': (('logits', 'dlogp', 'dprobs', 'dlogits'), ('dlogp', 'dprobs'), False),
    'resel_discrete_value': (('q', 'subset', 'logp', 'log_alpha', 'v'), ('subset',), True),
    'resel_q_taken_loss_fwd': (('q', 'action', 'y', 'mask', 'out2', 'workspace'), ('mask',), True),
    'resel_q_taken_loss_bwd': (('q', 'action', 'y', 'mask', 'g', 'dq'), ('mask',), True),
    'resel_discrete_actor_loss_fwd': (('logp', 'q', 'mask', 'log_alpha', 'out2', 'workspace'), ('mask',), True),
    'resel_discrete_actor_loss_bwd': (('logp', 'q', 'mask', 'log_alpha', 'g', 'dlogp', 'dq'), ('mask', 'dq'), True),
}


def call(lib, name, E=2, M=0, A=3, **null):
    """Every pointer FAKE unless named in `null`; M defaults to 0 so that a call that passes the checks launches nothing."""
    ptrs, _, has_e = ENTRIES[name]
    p = {k: (None if null.get(k) else FAKE) for k in ptrs}
    fn = getattr(lib, name)
    if name == 'resel_categorical_fwd':
        return fn(p['logits'], 0.01, p['logp'], p['probs'], p['mode'], M, A, None)
    if name == 'resel_categorical_bwd':
        return fn(p['logits'], 0.01, p['dlogp'], p['dprobs'], p['dlogits'], M, A, None)
    if name == 'resel_discrete_value':
        return fn(p['q'], p['subset'], 2, p['logp'], p['log_alpha'], p['v'], E, M, A, None)
    if name == 'resel_q_taken_loss_fwd':
        return fn(p['q'], p['action'], p['y'], p['mask'], p['out2'], p['workspace'], E, M, A, None)
    if name == 'resel_q_taken_loss_bwd':
        return fn(p['q'], p['action'], p['y'], p['mask'], p['g'], p['dq'], E, M, A, None)
    if name == 'resel_discrete_actor_loss_fwd':
        return fn(p['logp'], p['q'], p['mask'], p['log_alpha'], p['out2'], p['workspace'], E, M, A, 1, None)
    return fn(p['logp'], p['q'], p['mask'], p['log_alpha'], p['g'], p['dlogp'], p['dq'], E, M, A, 0, None)


@pytest.mark.parametrize('name', NAMES)
def test_empty_batch_launches_nothing(lib, name):
    assert call(lib, name, M=0) == 0
    assert call(lib, name, M=0, A=1) == 0 and call(lib, name, M=0, A=max_actions()) == 0
    for k in ENTRIES[name][1]:                                       # the optional pointers, one at a time
        assert call(lib, name, M=0, **{k: True}) == 0, k


@pytest.mark.parametrize('name', NAMES)
def test_null_required_pointer_is_rejected(lib, name):
    ptrs, optional, _ = ENTRIES[name]
    for k in ptrs:
        if k not in optional:
            assert call(lib, name, M=4, **{k: True}) == RESEL_EINVAL, k
            assert call(lib, name, M=0, **{k: True}) == RESEL_EINVAL, k


def test_head_backward_needs_one_incoming_gradient(lib):
    assert call(lib, 'resel_categorical_bwd', M=4, dlogp=True, dprobs=True) == RESEL_EINVAL
    assert call(lib, 'resel_categorical_bwd', M=0, dlogp=True, dprobs=True) == RESEL_EINVAL


@pytest.mark.parametrize('name', NAMES)
def test_bad_sizes_are_rejected(lib, name):
    assert call(lib, name, M=4, A=0) == RESEL_EINVAL
    assert call(lib, name, M=4, A=-1) == RESEL_EINVAL
    assert call(lib, name, M=4, A=max_actions() + 1) == RESEL_EINVAL
    assert call(lib, name, M=-1) == RESEL_EINVAL
    if ENTRIES[name][2]:
        assert call(lib, name, M=4, E=0) == RESEL_EINVAL
        assert call(lib, name, M=4, E=-2) == RESEL_EINVAL


def test_masked_loss_workspace_is_shared(lib):
    from offpolicy_rnn.hip import _lib
    fn = lib.resel_masked_loss_workspace_bytes
    fn.restype, fn.argtypes = _lib.SIGNATURES['resel_masked_loss_workspace_bytes']
    assert fn() >= 2 * 256 * 4                                       # two floats per block of the first stage
