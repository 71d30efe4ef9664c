"""The `ln+<act>` / `eln-<E>+<act>` norm blocks of the dense stacks (`resel_member_layernorm_*`, `ops.member_layer_norm`): what can be
checked without a GPU - the ABI additions, the argument checks that return before the device is touched, and the parameters an
RNNBase with such specs holds.  The kernels themselves: tests/test_norm_blocks_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

RESEL_EINVAL = -1
NAMES = ('resel_member_layernorm_fwd', 'resel_member_layernorm_bwd_workspace_bytes', 'resel_member_layernorm_bwd')


@pytest.fixture(scope='module')
def lib():
    from offpolicy_rnn.hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES + ('resel_abi_version',):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


def test_prototypes_agree_between_header_binding_and_library(lib):
    from ctypes import c_float, c_int, c_int64, c_size_t, c_uint, c_void_p
    from offpolicy_rnn.hip import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'resel_hip.h')).read(), flags=re.S)
    protos = dict(re.findall(r'\b(?:int|size_t)\s+(resel_member_layernorm[a-z0-9_]*)\s*\(([^;]*?)\)\s*;', header))
    assert set(protos) == set(NAMES)
    for name, params in protos.items():
        params = [p.strip() for p in params.split(',')]
        res, args = _lib.SIGNATURES[name]
        assert res is (c_size_t if name.endswith('_bytes') else c_int), name
        assert len(params) == len(args), (name, len(params), len(args))
        for ptxt, ctype in zip(params, args):
            want = (c_void_p if ('*' in ptxt or 'resel_stream_t' in ptxt) else c_int64 if ptxt.startswith('int64_t') else
                    c_float if ptxt.startswith('float') else c_uint if ptxt.startswith('unsigned') else c_int)
            assert ctype is want, (name, ptxt, ctype)
        assert hasattr(lib, name), name
    assert lib.resel_abi_version() == 11 == _lib.ABI_VERSION


def test_workspace_bytes(lib):
    ws = lib.resel_member_layernorm_bwd_workspace_bytes
    assert ws(1, 8, 256) == 2 * 1 * 2048 * 4                        # one block, a dw and a db partial of E C floats
    assert ws(5, 3, 8) == 2 * 2 * 24 * 4                            # tokens of up to 512 floats: four to a block
    assert ws(10 ** 6, 1, 256) == ws(8192, 1, 256) == 2 * 2048 * 256 * 4         # ... and the persistent grid stops at 2048 blocks
    assert ws(700, 8, 256) == 2 * 700 * 2048 * 4                    # wider tokens: one to a block
    assert ws(10 ** 6, 8, 256) == ws(66752, 8, 256) == 2 * 1024 * 2048 * 4       # ... up to 1024 blocks
    assert ws(4, 3, 6) == 0 and ws(4, 9, 256) == 0 and ws(0, 1, 8) == 0          # refused shapes


def test_entries_reject_bad_arguments_before_touching_the_device(lib):
    """Nothing here is a device pointer: a call that got past the argument checks would fault, not return."""
    fake = 0x1000                                                  # 16-byte aligned, never dereferenced
    M, E, C = 5, 3, 8

    def fwd(x=fake, w=fake, b=fake, y=fake, stats=fake, M=M, E=E, C=C, act=1, lx=(8, 24), ly=(8, 24), amax=None):
        return lib.resel_member_layernorm_fwd(x, lx[0], lx[1], w, b, y, ly[0], ly[1], stats, M, E, C, 1e-5, act, amax, 0, None)

    def bwd(dy=fake, x=fake, w=fake, b=fake, stats=fake, dx=fake, dw=fake, db=fake, ws=fake, M=M, E=E, C=C, act=1, lg=(8, 24), lx=(8, 24),
            ld=(40, 8), amax=None):
        return lib.resel_member_layernorm_bwd(dy, lg[0], lg[1], x, lx[0], lx[1], w, b, stats, dx, ld[0], ld[1], dw, db, ws, M, E, C, act,
                                              amax, 0, None)

    for key in ('x', 'w', 'y', 'stats'):                            # a NULL required operand (the bias may be NULL)
        assert fwd(**{key: None}) == RESEL_EINVAL, key
    for key in ('dy', 'x', 'w', 'stats', 'dx', 'dw', 'ws'):
        assert bwd(**{key: None}) == RESEL_EINVAL, key
    assert bwd(b=None) == RESEL_EINVAL                              # a bias gradient without a bias
    for call in (fwd, bwd):
        assert call(C=6) == RESEL_EINVAL                            # C % 4 != 0
        assert call(C=10) == RESEL_EINVAL
        assert call(E=8, C=260) == RESEL_EINVAL                     # E * C above the cap of 2048
        assert call(E=1, C=2052) == RESEL_EINVAL
        assert call(E=2049, C=4) == RESEL_EINVAL
        assert call(act=2) == RESEL_EINVAL and call(act=-1) == RESEL_EINVAL
        assert call(M=0) == RESEL_EINVAL and call(E=0) == RESEL_EINVAL and call(C=0) == RESEL_EINVAL
        assert call(x=fake + 4) == RESEL_EINVAL and call(w=fake + 8) == RESEL_EINVAL and call(b=fake + 4) == RESEL_EINVAL    # misaligned
        assert call(lx=(6, 24)) == RESEL_EINVAL and call(lx=(8, 22)) == RESEL_EINVAL and call(lx=(0, 24)) == RESEL_EINVAL    # strides
        assert call(lx=(1 << 30, 8)) == RESEL_EINVAL               # E * ld_e would not fit the kernel's 32-bit token offsets
        assert call(amax=fake + 4) == RESEL_EINVAL                  # magnitude handles are 8-byte words
    assert fwd(y=fake + 4) == RESEL_EINVAL and fwd(ly=(8, 2)) == RESEL_EINVAL
    assert bwd(dy=fake + 4) == RESEL_EINVAL and bwd(dx=fake + 4) == RESEL_EINVAL and bwd(ws=fake + 4) == RESEL_EINVAL
    assert bwd(lg=(3, 24)) == RESEL_EINVAL and bwd(ld=(40, 3)) == RESEL_EINVAL


@pytest.mark.parametrize('layer_type,activation,expect', [
    (['fc', 'fc', 'fc'], ['ln+elu', 'ln+elu', 'linear'], {'activation_list.0.0': (12,), 'activation_list.1.0': (20,)}),
    (['efc-3', 'efc-3', 'efc-3'], ['eln-3+elu', 'eln-3+tanh', 'linear'], {'activation_list.0.0': (3, 12), 'activation_list.1.0': (3, 20)}),
    (['fc', 'gru', 'fc'], ['ln+elu', 'ln+elu', 'linear'], {'activation_list.0.0': (12,), 'activation_list.1.0': (20,)})])
def test_rnn_base_builds_the_reference_parameters(layer_type, activation, expect):
    """Names and shapes of the norm parameters are the reference's (`activation_list.<i>.0.weight` / `.bias` of a torch LayerNorm, rnn_base.py:250-258)
    - what `oracle.network.init_rnn_base` restates - so reference checkpoints keep loading; ones / zeros at construction."""
    from offpolicy_rnn.models.rnn_base import RNNBase
    from oracle import network as NW
    net = RNNBase(7, 4, [12, 20], activation, layer_type)
    sd = net.state_dict()
    ref = NW.init_rnn_base(7, 4, [12, 20], activation, layer_type)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    for pre, shape in expect.items():
        assert tuple(sd[pre + '.weight'].shape) == shape == tuple(sd[pre + '.bias'].shape)
        assert torch.equal(sd[pre + '.weight'], torch.ones(shape)) and torch.equal(sd[pre + '.bias'], torch.zeros(shape))
    assert not [k for k in sd if k.startswith('activation_list.2')]
    assert isinstance(net.activation_list[0], torch.nn.ModuleList) and isinstance(net.activation_list[0][0], torch.nn.LayerNorm)
    net.load_state_dict({k: v.clone() for k, v in ref.items()})          # a reference-shaped checkpoint loads


def test_cpu_tensors_keep_the_torch_spelling(oracle_ops):
    """A CPU forward of such a stack (the dense layers on the oracle's op table) keeps the torch LayerNorm - `ops.member_layer_norm`, which
    has no CPU form, is never asked: the result is the oracle restatement of the reference's arithmetic."""
    from offpolicy_rnn.models.rnn_base import RNNBase
    from oracle import network as NW
    torch.manual_seed(0)
    lt, act = ['fc', 'fc', 'fc'], ['ln+elu', 'ln+tanh', 'linear']
    net = RNNBase(7, 4, [12, 20], act, lt)
    with torch.no_grad():
        for p in net.activation_list.parameters():
            p.add_(torch.randn_like(p) * 0.3)
    x = torch.randn(3, 9, 7)
    y, _, _ = net.meta_forward(x)
    ref = NW.rnn_base_forward({k: v for k, v in net.state_dict().items()}, dict(layer_type=lt, activation=act), x)
    torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-6)


def test_switch_is_read_per_call(monkeypatch):
    from offpolicy_rnn.hip import ops
    monkeypatch.delenv('RESEL_NORM_FUSED', raising=False)
    assert ops.norm_fused_on() == (ops.NORM_FUSED_DEFAULT != '0')
    monkeypatch.setenv('RESEL_NORM_FUSED', '0')
    assert not ops.norm_fused_on()
    monkeypatch.setenv('RESEL_NORM_FUSED', '1')
    assert ops.norm_fused_on()
    assert ops.member_layer_norm_ok(8, 256) and ops.member_layer_norm_ok(1, 12) and not ops.member_layer_norm_ok(8, 260)
    assert not ops.member_layer_norm_ok(1, 6)


def test_trainer_with_norm_specs_matches_the_oracle_trainer(oracle_ops, monkeypatch):
    """A gru SAC-REDQ trainer with `eln-4+elu` critic layers and `ln+elu` policy / encoder layers on the CPU (torch norms, the oracle's op
    table): construction, flat stores, optimizer regrouping, flat AdamW and the soft update against the oracle trainer over two updates.
    REDQ draws 2 of the 4 critics for the target: the norm couples the members, so all four are evaluated and the drawn ones picked."""
    import numpy as np
    from offpolicy_rnn import alg_init
    from oracle.trainer import OracleTrainer, default_parameter
    from test_host_logic import _push, _synth, make_parameter
    from test_oracle_golden import _push as opush
    over = dict(value_activations=['eln-4+elu', 'eln-4+elu', 'linear'], value_layer_type=['efc-4'] * 3,
                policy_activations=['ln+elu', 'ln+elu', 'linear'], value_embedding_activations=['ln+elu', 'ln+elu', 'linear'],
                policy_embedding_activations=['ln+elu', 'ln+elu', 'linear'], sac_batch_size=40)
    from offpolicy_rnn.utility import rng                      # both trainers draw the actor noise from the CPU generator, wherever the product runs
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.randn(tuple(shape), dtype=dtype).to(device))
    torch.manual_seed(11)
    alg = alg_init(make_parameter('gru', **over))
    assert alg.parameter.redq_m == 2 and alg.values[0].uni_network.members_coupled() and not alg.policy.uni_network.members_coupled()
    names = [k for k, _ in alg.values[0].uni_network.named_parameters()]
    assert 'activation_list.0.0.weight' in names and 'activation_list.1.0.bias' in names
    for net in (alg.policy, alg.values[0], alg.target_values[0]):          # the norm parameters live in the flat buffers
        flat = net.store.flat
        for p, o, n in net.store.slices:
            assert p.data_ptr() == flat.data_ptr() + 4 * o
    cpu = lambda sd: {m: {k: v.detach().cpu().clone() for k, v in d.items()} for m, d in sd.items()}
    par = default_parameter(rnn='gru', D=32, policy_embedding_dim=16, value_embedding_dim=16, policy_uni_model_input_mapping_dim=16,
                            value_uni_model_input_mapping_dim=16, max_buffer_transition_num=5000, **over)
    tr = OracleTrainer(par, 5, 3, 12, policy_state=cpu(alg.policy.state_dict()), value_state=cpu(alg.values[0].state_dict()))
    rs = np.random.RandomState(9)
    for n in [12, 5, 7, 12, 4, 9, 6]:
        o, a, r = _synth(rs, n, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=(n != 12))
        opush(tr.buffer, o, a, r, early_done=(n != 12))
    logs = []
    for runner in (alg, tr):
        torch.manual_seed(200)
        np.random.seed(200)
        out = []
        for _ in range(2):
            out.append(dict(runner.train_one_batch()))
            runner.grad_num += 1
        logs.append(out)
    val = lambda v: v[0] if isinstance(v, tuple) else v
    for it, (a, b) in enumerate(zip(*logs)):
        for k, v in b.items():
            assert val(a[k]) == pytest.approx(val(v), rel=2e-3, abs=2e-4), (it, k, val(a[k]), val(v))
    for net, ref in ((alg.policy, tr.policy), (alg.values[0], tr.value), (alg.target_values[0], tr.target_value)):
        sd = net.state_dict()
        for mod, d in ref.items():
            for k, v in d.items():
                np.testing.assert_allclose(sd[mod][k].detach().cpu(), v.detach(), rtol=1e-3, atol=2e-5, err_msg=f'{mod}.{k}')
    w = alg.values[0].state_dict()['universal_model']['activation_list.0.0.weight']
    assert tuple(w.shape) == (4, 32) and not torch.equal(w.cpu(), torch.ones(4, 32)), 'the norm weights take part in the update'
