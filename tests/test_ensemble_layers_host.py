"""Host side of the ensemble sequence layers `elru-<E>` / `econv1d[_<K>]-<E>` (models/lru/elru.py, models/conv1d/econv1d.py): the id
grammar, the shapes recorded from the reference (tests/golden/generate_ensemble_golden.py), where these layers may stand, and the C ABI of
their kernels.  No GPU."""
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, load_golden
from test_host_logic import make_parameter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = json.load(open(os.path.join(GOLDEN, 'train_ensemble_meta.json')))
NEW_ENTRIES = ('resel_linrec_complex_members_fwd', 'resel_linrec_complex_members_bwd_workspace_bytes', 'resel_linrec_complex_members_bwd',
               'resel_member_conv1d_fwd', 'resel_member_conv1d_bwd_workspace_bytes', 'resel_member_conv1d_bwd',
               'resel_member_add_layernorm_fwd')


def _trainer(name, **over):
    from offpolicy_rnn import alg_init
    m = META[name]
    kw = dict(D=m['D'], algo=m['algo'], sac_batch_size=m['sac_batch_size'], redq_m=m['redq_m'],
              value_embedding_layer_type=['efc-4', m['rnn'], 'efc-4'], value_layer_type=['efc-4'] * 3)
    kw.update(over)
    return alg_init(make_parameter('gilr', **kw))


# ------------------------------------------------------------------------------------------------ grammar
@pytest.mark.parametrize('lid,family,E,K', [('elru-1', 'elru', 1, 4), ('elru-8', 'elru', 8, 4), ('elru-12', 'elru', 12, 4),
                                            ('econv1d-4', 'econv1d', 4, 4), ('econv1d_1-3', 'econv1d', 3, 1), ('econv1d_32-2', 'econv1d', 2, 32),
                                            ('econv1d_3-10', 'econv1d', 10, 3)])
def test_accepted_ids(lid, family, E, K):
    from offpolicy_rnn.models.layer_kinds import kind_of, parse_e_seq_id
    from offpolicy_rnn.models.rnn_base import RNNBase
    kind = kind_of(lid)
    assert kind.name == family and kind.member_axis and kind.honours_start and not kind.deferred
    assert parse_e_seq_id(lid) == dict(family=family, num_ensemble=E, d_conv=K)
    net = RNNBase(8, 8, [], ['linear'], [lid])
    layer = net.layer_list[0]
    assert layer.num_ensemble == E and kind.context_len(layer) == (K if family == 'econv1d' else 0)
    assert net.rnn_hidden_state_input_size == [2 * E * 8 if family == 'elru' else E * (K - 1) * 8]
    assert tuple(net.make_init_state(3)[0].shape) == (1, 3, net.rnn_hidden_state_input_size[0])
    assert not kind.fuses_out_act(layer, torch.zeros(E, 2, 3, 8))


@pytest.mark.parametrize('lid', ['econv1d-4_4', 'egilr-2', 'egilr_lstm-2', 'elru', 'elru-', 'elru-0', 'elru_3-2', 'elru-4x', 'elru-+4', 'elru- 4',
                                 'elru-4_0', 'elru-٤', 'econv1d', 'econv1d-', 'econv1d-0', 'econv1d_0-2', 'econv1d_33-2', 'econv1d_3_3-2',
                                 'econv1d_-2', 'econv1d_3-2-2', 'econv1d_1_6-2', 'econv1dx-2', 'elrux-2'])
def test_rejected_ids_raise_not_implemented(lid):
    """`int('4_4')` is 44 and `int('٤')` is 4 in Python: the digits are matched, not converted."""
    from offpolicy_rnn.models.layer_kinds import kind_of, parse_e_seq_id
    from offpolicy_rnn.models.rnn_base import RNNBase
    with pytest.raises(NotImplementedError):
        parse_e_seq_id(lid)
    with pytest.raises(NotImplementedError):
        kind_of(lid)
    with pytest.raises(NotImplementedError):
        RNNBase(32, 32, [], ['linear'], [lid])


def test_egilr_names_the_reference_defect():
    from offpolicy_rnn.models.layer_kinds import kind_of
    for lid in ('egilr-4', 'egilr_lstm-4'):
        with pytest.raises(NotImplementedError, match=r'egilr\.py:72-76'):
            kind_of(lid)


def test_unequal_widths_are_refused_with_a_message():
    from offpolicy_rnn.models.rnn_base import RNNBase
    for lid in ('elru-2', 'econv1d-2'):
        with pytest.raises(AssertionError, match='input_dim == output_dim'):
            RNNBase(8, 16, [], ['linear'], [lid])


def test_a_network_with_these_layers_copies_and_pickles():
    import copy
    import pickle
    from offpolicy_rnn.models.rnn_base import RNNBase
    net = RNNBase(8, 8, [8, 8], ['elu', 'elu', 'linear'], ['efc-2', 'elru-2', 'econv1d_3-2'])
    for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        assert [k if k is None else k.name for k in twin.layer_kind] == [None, 'elru', 'econv1d'] and twin.layer_kind[1] is net.layer_kind[1]


# ------------------------------------------------------------------------------------------------ shapes recorded from the reference
@pytest.mark.parametrize('lid', ['elru-3', 'econv1d_3-3'])
def test_layer_state_dict_and_state_width_equal_the_reference(lid):
    from offpolicy_rnn.models.rnn_base import RNNBase
    g = load_golden('ensemble_layers.npz')
    ref = {k.split('|p|')[1]: tuple(g[k].shape) for k in g if k.startswith(f'{lid}|m|p|')}
    net = RNNBase(8, 8, [], ['linear'], [lid])
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == ref and list(net.state_dict()) == list(ref)
    assert tuple(g[f'{lid}|m|h0'].shape) == tuple(net.make_init_state(2)[0].shape) == (1, 2, 48)
    # (the convolution hands its window back as [B, 1, width], like `conv1d`: the same memory as [1, B, width])
    assert tuple(g[f'{lid}|m|h'].shape) == ((1, 2, 48) if lid.startswith('elru') else (2, 1, 48))
    net.load_state_dict({k: torch.from_numpy(g[f'{lid}|m|p|{k}']) for k in ref})
    # every parameter the reference differentiates is a parameter here (same names): nothing extra, nothing missing
    assert {n for n, _ in net.named_parameters()} == {k.split('|g|')[1] for k in g if k.startswith(f'{lid}|m|g|')}


def test_elru_initialisation_follows_the_reference_distributions():
    from offpolicy_rnn.models.rnn_base import RNNBase
    torch.manual_seed(0)
    layer = RNNBase(64, 64, [], ['linear'], ['elru-3']).layer_list[0]
    for proj in (layer.in_proj, layer.middle_proj):
        assert torch.count_nonzero(proj.bias) == 0
        bound = (6.0 / (64 + 64)) ** 0.5                           # Xavier-uniform per [i, j] slice
        assert proj.weight.abs().max() <= bound and proj.weight.abs().max() > 0.9 * bound
    nu, theta, gamma = torch.exp(layer.params_log.detach())
    mag = torch.exp(-nu)
    assert tuple(layer.params_log.shape) == (3, 3, 64) and (mag >= 0.9 - 1e-6).all() and (mag <= 0.999 + 1e-6).all()
    assert (theta >= 0).all() and (theta <= 6.2832).all()
    torch.testing.assert_close(gamma, torch.sqrt(1 - mag ** 2), rtol=1e-5, atol=1e-6)
    assert not torch.equal(layer.params_log[:, 0], layer.params_log[:, 1])        # drawn per member


@pytest.mark.parametrize('name', list(META))
def test_critic_state_dict_state_widths_and_parameter_count_equal_the_reference(name):
    m = META[name]
    alg = _trainer(name)
    v = alg.values[0]
    assert {mod: {k: list(t.shape) for k, t in d.items()} for mod, d in v.state_dict().items()} == m['value_shapes']
    assert [int(w) for w in v.embedding_network.rnn_hidden_state_input_size] == m['value_state_width']
    assert sum(p.numel() for p in v.parameters()) == m['value_nparam']
    assert alg._get_skip_len() == m['skip_len'] and bool(alg.allow_nest_stack) == m['nest']
    g = load_golden(f'train_{name}.npz')
    from conftest import nested
    v.load_state_dict(nested(g, 'value0|'))
    for p, o, n in v.store.slices:                                  # the flat store keeps the reference's keys and shapes, as views
        assert p.data_ptr() == v.store.flat.data_ptr() + 4 * o
    # sep_optim: the context encoder - the ensemble sequence layer's parameters among them - trains at the rnn learning rate
    a, b = v.store.module_range['embedding_model']
    seg = list(alg.optimizer_value.seg_end.tolist()).index(b)
    assert alg.optimizer_value.seg_lr[seg].item() == pytest.approx(alg.parameter.rnn_value_lr)
    ids = {id(p) for p in v.embedding_network.rnn_parameters()}
    assert ids >= {id(p) for p in v.embedding_network.layer_list[1].parameters()}


# ------------------------------------------------------------------------------------------------ host logic on the CPU op backend
def load_layer(lid, form, device='cpu'):
    """The recorded layer of ensemble_layers.npz -> (net, x leaf, carried-in state with start / mask, recorded arrays by short name)."""
    from offpolicy_rnn.models.rnn_base import RNNBase
    g = load_golden('ensemble_layers.npz')
    pre = f'{lid}|{form}|'
    rec = {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}
    net = RNNBase(8, 8, [], ['linear'], [lid])
    net.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith('p|')})
    net.to(device)
    hid = net.make_init_state(2, device)
    hid[0] = torch.from_numpy(rec['h0']).to(device)
    hid.set_rnn_start(torch.from_numpy(g['start']).to(device))
    hid.set_mask(torch.from_numpy(g['mask']).to(device))
    x = torch.from_numpy(rec['x']).to(device).requires_grad_(True)
    return net, x, hid, rec


def check_layer(net, x, hid, rec, out_tol, grad_tol):
    import numpy as np
    y, h, _ = net.meta_forward(x, hid)
    (y * torch.from_numpy(rec['w']).to(y.device)).sum().backward()
    np.testing.assert_allclose(y.detach().cpu(), rec['y'], rtol=out_tol[0], atol=out_tol[1], err_msg='y')
    np.testing.assert_allclose(h[0].detach().cpu().reshape(rec['h'].shape), rec['h'], rtol=out_tol[0], atol=out_tol[1], err_msg='state')
    np.testing.assert_allclose(x.grad.cpu(), rec['dx'], rtol=grad_tol[0], atol=grad_tol[1], err_msg='dx')
    for n, p in net.named_parameters():
        np.testing.assert_allclose(p.grad.cpu(), rec['g|' + n], rtol=grad_tol[0], atol=grad_tol[1], err_msg=n)


@pytest.mark.parametrize('form', ['m', 's'])
@pytest.mark.parametrize('lid', ['elru-3', 'econv1d_3-3'])
def test_layer_host_path_equals_the_reference(lid, form, oracle_ops, monkeypatch):
    """RESEL_MEMBER_SEQ=0 is E calls of the single-member ops: with the CPU stand-ins for those, the layers' own code (projections,
    state layout, masks, the feed-forward block) reproduces the reference's recording - member-major and shared input, live state."""
    monkeypatch.setenv('RESEL_MEMBER_SEQ', '0')
    check_layer(*load_layer(lid, form), out_tol=(1e-4, 2e-5), grad_tol=(2e-3, 3e-4))


@pytest.mark.parametrize('name', list(META))
def test_trainer_host_path_equals_the_reference_logs(name, oracle_ops, monkeypatch):
    """Three updates of the reference's recording on the CPU op backend (RESEL_MEMBER_SEQ=0): logs and every parameter."""
    import numpy as np
    from conftest import nested
    from test_host_logic import _push, _synth
    monkeypatch.setenv('RESEL_MEMBER_SEQ', '0')
    m = META[name]
    g = load_golden(f'train_{name}.npz')
    alg = _trainer(name)
    alg.policy.load_state_dict(nested(g, 'policy0|'))
    alg.values[0].load_state_dict(nested(g, 'value0|'))
    alg._value_update(tau=0.0)
    rs = np.random.RandomState(m['ring_seed'])
    for n in m['lens']:
        o, a, r = _synth(rs, n, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=(n != 12))
    torch.manual_seed(200)
    np.random.seed(200)
    for it in range(3):
        log = alg.train_one_batch()
        alg.grad_num += 1
        for k, v in m['logs'][it].items():
            got = log[k][0] if isinstance(log[k], tuple) else log[k]
            assert got == pytest.approx(v, rel=2e-3, abs=5e-4), (it, k, got, v)
    for pre, net in (('policy3|', alg.policy), ('value3|', alg.values[0]), ('target3|', alg.target_values[0])):
        sd = net.state_dict()
        for mod, d in nested(g, pre).items():
            for k, v in d.items():
                np.testing.assert_allclose(sd[mod][k].detach(), v, rtol=2e-3, atol=2e-5, err_msg=f'{pre}{mod}.{k}')
    np.testing.assert_allclose(alg.log_sac_alpha.detach(), g['log_alpha3'], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ where these layers may stand
def test_a_policy_stack_with_an_ensemble_sequence_layer_raises_value_error():
    from offpolicy_rnn import alg_init
    for lid in ('elru-4', 'econv1d-4'):
        with pytest.raises(ValueError, match='policy'):
            alg_init(make_parameter('gilr', D=16, policy_embedding_layer_type=['fc', lid, 'fc']))


def test_a_member_count_mismatch_raises_value_error_naming_both():
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.models.rnn_base import RNNBase
    with pytest.raises(ValueError, match=r"'elru-3'.*'efc-4'"):
        RNNBase(8, 8, [8, 8], ['elu', 'elu', 'linear'], ['efc-4', 'elru-3', 'efc-4'])
    with pytest.raises(ValueError, match=r"'econv1d_3-2'.*'efc-4'"):
        RNNBase(8, 8, [8], ['elu', 'linear'], ['econv1d_3-2', 'efc-4'])
    with pytest.raises(ValueError, match='efc-8'):                   # across the critic's two stacks: the head keeps efc-8
        alg_init(make_parameter('gilr', D=16, value_embedding_layer_type=['efc-4', 'elru-4', 'efc-4']))


def test_a_stack_with_an_ensemble_sequence_layer_couples_its_members():
    from offpolicy_rnn.models.rnn_base import RNNBase
    assert RNNBase(8, 8, [8, 8], ['elu', 'elu', 'linear'], ['efc-4', 'elru-4', 'efc-4']).members_coupled()
    assert RNNBase(8, 8, [], ['linear'], ['econv1d-4']).members_coupled()
    assert not RNNBase(8, 8, [8, 8], ['elu', 'elu', 'linear'], ['efc-4', 'efc-4', 'efc-4']).members_coupled()
    assert not RNNBase(8, 8, [8, 8], ['elu', 'elu', 'linear'], ['fc', 'lru', 'fc']).members_coupled()
    alg = _trainer('elru_sac')
    tv = alg.target_values[0]
    assert tv.embedding_network.members_coupled() and tv.embedding_network.emits_member_axis() and not tv.uni_network.emits_member_axis()
    # the routes that assume a 3-D embedding decline: no head row buffer, no action-only dX
    assert not tv._action_only_graph() and not alg.values[0]._action_only_graph()


def test_one_token_steps_raise():
    from offpolicy_rnn.models.rnn_base import RNNBase
    for lid in ('elru-2', 'econv1d-2'):
        net = RNNBase(8, 8, [], ['linear'], [lid])
        with torch.no_grad(), pytest.raises(NotImplementedError, match='never stepped'):
            net.meta_forward(torch.zeros(2, 3, 1, 8), net.make_init_state(3))


def test_the_memoryless_trainer_keeps_refusing_sequence_layers():
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.models.layer_kinds import is_rnn_layer, kind_of
    assert is_rnn_layer('elru-4') and kind_of('elru-4').member_axis          # a sequence layer like any other to that trainer's check
    with pytest.raises(AssertionError, match='sequence layers'):
        alg_init(make_parameter('fc', D=16, alg_name='sac_mlp_redq_ensemble_q', rnn_fix_length=0, redq_m=2, state_action_encoder=False,
                                value_embedding_layer_type=['efc-4', 'elru-4', 'efc-4'], value_layer_type=['efc-4'] * 3,
                                policy_embedding_layer_type=['fc'] * 3, policy_layer_type=['fc'] * 3))


# ------------------------------------------------------------------------------------------------ switch and ABI
def test_member_seq_switch_takes_0_and_1_only(monkeypatch):
    from offpolicy_rnn.hip import ops
    monkeypatch.delenv('RESEL_MEMBER_SEQ', raising=False)
    assert ops.member_seq_on() == (ops.MEMBER_SEQ_DEFAULT == '1')
    for v, want in (('0', False), ('1', True)):
        monkeypatch.setenv('RESEL_MEMBER_SEQ', v)                    # read per call
        assert ops.member_seq_on() is want
    for v in ('', '2', 'on', 'true', '01', ' 1'):
        monkeypatch.setenv('RESEL_MEMBER_SEQ', v)
        with pytest.raises(ValueError, match='RESEL_MEMBER_SEQ'):
            ops.member_seq_on()


def test_the_two_sides_of_the_abi_agree_for_the_new_entries():
    """Header prototype against ctypes signature, parameter by parameter (the rule of test_host_logic, restated for these entries so that
    a drift names them), and the built library exports them."""
    from ctypes import c_float, c_int, c_int64, c_size_t, c_void_p
    from offpolicy_rnn.hip import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'resel_hip.h')).read(), flags=re.S)
    protos = dict(re.findall(r'\b(?:int|size_t)\s+(resel_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', header))
    for name in NEW_ENTRIES:
        assert name in protos and name in _lib.SIGNATURES, name
        params = [p.strip() for p in protos[name].split(',') if p.strip()]
        res, args = _lib.SIGNATURES[name]
        assert res is (c_size_t if name.endswith('_bytes') else c_int) and len(params) == len(args), (name, len(params), len(args))
        for ptxt, ctype in zip(params, args):
            if '*' in ptxt or 'resel_stream_t' in ptxt:
                assert ctype is c_void_p, (name, ptxt)
            elif ptxt.startswith('int64_t'):
                assert ctype is c_int64, (name, ptxt)
            elif ptxt.startswith('float'):
                assert ctype is c_float, (name, ptxt)
            elif ptxt.startswith('unsigned'):
                assert ctype is ctypes.c_uint, (name, ptxt)
            else:
                assert ptxt.startswith('int ') and ctype is c_int, (name, ptxt)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(h, name), name
    # refused arguments come back as RESEL_EINVAL without a launch (no device needed): null operands, E * rows beyond the grid
    for name in ('resel_linrec_complex_members_fwd', 'resel_member_conv1d_fwd', 'resel_member_add_layernorm_fwd'):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    assert h.resel_linrec_complex_members_fwd(None, None, 8, None, None, None, None, None, None, None, None, 2, 2, 4, 8, None, 0, None) == -1
    assert h.resel_member_conv1d_fwd(None, 8, 0, None, None, None, None, 8, 2, 2, 4, 8, 3, None, 0, None) == -1
    assert h.resel_member_add_layernorm_fwd(None, None, None, 8, 8, None, None, None, 8, 8, None, 2, 2, 8, 1e-5, 0, None, 0, None) == -1
    ws = h.resel_linrec_complex_members_bwd_workspace_bytes
    ws.restype, ws.argtypes = _lib.SIGNATURES['resel_linrec_complex_members_bwd_workspace_bytes']
    one = h.resel_linrec_complex_bwd_workspace_bytes
    one.restype, one.argtypes = _lib.SIGNATURES['resel_linrec_complex_bwd_workspace_bytes']
    assert ws(3, 2, 65, 20) == one(6, 65, 20)
