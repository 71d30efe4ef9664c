"""relu, leaky_relu, tanh and sigmoid behind the `fc` / `efc-<E>` layers (activation codes 6 .. 9 of `resel_gemm_f32x` and
`resel_bias_act_*`): what can be checked without a GPU - the code table, the argument checks that return before the device is touched,
the CPU spelling of such a stack, and the guard for the inputs of the GPU update test.  The kernels: tests/test_dense_activations_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import update_parity as UP

RESEL_EINVAL = -1
NEW = {'relu': 6, 'leaky_relu': 7, 'tanh': 8, 'sigmoid': 9}
# the whole-update cases, shared with tests/test_dense_activations_gpu.py: gilr SAC-REDQ, D = 32, 8 rows x 64 steps
ROWS, STEPS, OBS, ACT, D = 8, 64, 17, 6, 32
INIT_SEED, DATA_SEED, UPDATE_SEED = 2, 0, 200        # weights, trajectories, the update's draws (seed 1 / 200 puts a relu pre-activation of the
                                                    # tanh-relu case within fp32 distance of zero: 7.0e-5 on the policy's last_act_encoder.weight)
UPDATE_CASES = {'relu': ('relu', 'relu'), 'tanh-relu': ('tanh', 'relu')}        # (embedding stacks, heads): all relu; the reference defaults' mix


def update_overrides(emb, head):
    """Parameter fields of an update case (oracle.trainer.default_parameter / offpolicy_rnn.Parameter names)."""
    over = dict(policy_embedding_dim=16, value_embedding_dim=16, policy_uni_model_input_mapping_dim=16, value_uni_model_input_mapping_dim=16)
    for w in ('value', 'policy'):
        over[f'{w}_embedding_activations'] = [emb, emb, 'linear']
        over[f'{w}_activations'] = [head, head, 'linear']
        over[f'{w}_embedding_hidden_size'] = [D, D]
        over[f'{w}_hidden_size'] = [D, D]
    return over


@pytest.fixture(scope='module')
def lib():
    from offpolicy_rnn.hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('resel_gemm_f32x', 'resel_bias_act_fwd', 'resel_bias_act_bwd', 'resel_abi_version'):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


def test_code_table(lib):
    from offpolicy_rnn.hip import _lib, ops
    for name, code in NEW.items():
        assert ops.ACT_IDS[name] == code == ops.GEMM_EPILOGUES[name], name
    assert {k: ops.ACT_IDS[k] for k in (None, 'linear', 'elu')} == {None: 0, 'linear': 0, 'elu': 1} and len(ops.ACT_IDS) == 7
    assert {k: ops.GEMM_EPILOGUES[k] for k in (None, 'linear', 'elu', ops.GEMM_ACCUMULATE, ops.GEMM_SOFTPLUS)} == \
        {None: 0, 'linear': 0, 'elu': 1, ops.GEMM_ACCUMULATE: 2, ops.GEMM_SOFTPLUS: 3} and len(ops.GEMM_EPILOGUES) == 9
    assert lib.resel_abi_version() == 11 == _lib.ABI_VERSION


def test_entries_reject_other_codes_before_touching_the_device(lib):
    """Nothing here is a device pointer: a call that got past the argument checks would fault, not return."""
    fake = 0x1000                                                  # 16-byte aligned, never dereferenced
    for act in (4, 5, 10, -1):
        assert lib.resel_gemm_f32x(fake, 32, 0, 1, fake, 32, 0, 1, fake, 0, act, fake, 8, 0, fake, 4, 8, 32, 1, 0, None, None, None, 0, None) == RESEL_EINVAL, act
    for act in (2, 3, 4, 5, 10, -1):
        assert lib.resel_bias_act_fwd(fake, fake, 4, 8, 4, act, None) == RESEL_EINVAL, act
        assert lib.resel_bias_act_bwd(fake, 8, fake, 8, fake, fake, fake, 4, 8, 4, act, None, 0, None) == RESEL_EINVAL, act
    for act in NEW.values():                                        # the new codes need the layer output and a destination, like ELU
        assert lib.resel_bias_act_bwd(fake, 8, None, 8, fake, fake, fake, 4, 8, 4, act, None, 0, None) == RESEL_EINVAL, act
        assert lib.resel_bias_act_bwd(fake, 8, fake, 8, None, fake, fake, 4, 8, 4, act, None, 0, None) == RESEL_EINVAL, act


def test_switch_is_read_per_call_and_refuses_other_values(monkeypatch):
    from offpolicy_rnn.hip import ops
    monkeypatch.delenv('RESEL_ACT_FUSED', raising=False)
    assert ops.act_fused_on()
    monkeypatch.setenv('RESEL_ACT_FUSED', '0')
    assert not ops.act_fused_on()
    monkeypatch.setenv('RESEL_ACT_FUSED', '1')
    assert ops.act_fused_on()
    for bad in ('2', '', 'on'):
        monkeypatch.setenv('RESEL_ACT_FUSED', bad)
        with pytest.raises(ValueError):
            ops.act_fused_on()
    monkeypatch.setenv('RESEL_ACT_FUSED', '0')
    x = torch.zeros(2, 4)
    assert ops.dense_act_name(torch.nn.ELU(), x) == 'elu'           # ELU: whatever the switch and the device say
    for mod in (torch.nn.ReLU(), torch.nn.LeakyReLU(), torch.nn.Tanh(), torch.nn.Sigmoid(), torch.nn.GELU(), torch.nn.LeakyReLU(0.2), torch.nn.ELU(0.5)):
        assert ops.dense_act_name(mod, x) is None
    monkeypatch.setenv('RESEL_ACT_FUSED', '1')
    for mod in (torch.nn.ReLU(), torch.nn.LeakyReLU(), torch.nn.Tanh(), torch.nn.Sigmoid()):
        assert ops.dense_act_name(mod, x) is None                   # a CPU pass keeps the module


@pytest.mark.parametrize('name', list(NEW))
def test_cpu_passes_keep_the_torch_spelling(name, oracle_ops, monkeypatch):
    """A CPU forward and backward of a dense stack with one of the four activations (the dense layers on the oracle's op table, which knows
    no activation name but 'elu'): the activation stays the torch module, bit for bit what RESEL_ACT_FUSED=0 computes, and the oracle's
    restatement of the reference; no new name reaches `ops`."""
    from offpolicy_rnn.models.rnn_base import RNNBase
    from oracle import network as NW
    ops = oracle_ops
    seen = []
    for fn_name, pos in (('linear_act', 3), ('gemm_f32', 5), ('bias_act_', 3), ('bias_act_bwd', 3)):
        def spy(*a, _f=getattr(ops, fn_name), _pos=pos, **kw):
            seen.append(kw.get('act', a[_pos] if len(a) > _pos else None))
            return _f(*a, **kw)
        monkeypatch.setattr(ops, fn_name, spy)
    lt, act = ['fc', 'efc-2', 'efc-2'], [name, name, 'linear']
    torch.manual_seed(0)
    net = RNNBase(7, 4, [12, 20], act, lt)
    x = torch.randn(3, 9, 7)
    w = torch.randn(2, 3, 9, 4)

    def run():
        xs = x.clone().requires_grad_(True)
        y, _, _ = net.meta_forward(xs)
        (y * w).sum().backward()
        out = [y.detach().clone(), xs.grad.clone()] + [p.grad.clone() for p in net.parameters()]
        net.zero_grad()
        return out

    monkeypatch.delenv('RESEL_ACT_FUSED', raising=False)
    on = run()
    monkeypatch.setenv('RESEL_ACT_FUSED', '0')
    off = run()
    assert len(seen) >= 6 and not [s for s in seen if s in NEW], seen
    assert all(torch.equal(a, b) for a, b in zip(on, off))
    ref = NW.rnn_base_forward({k: v.detach() for k, v in net.state_dict().items()}, dict(layer_type=lt, activation=act), x)
    torch.testing.assert_close(on[0], ref, rtol=1e-5, atol=1e-6)
    assert all(torch.isfinite(t).all() and t.abs().max() > 0 for t in on)


def _one_update(dtype, over, policy_state, value_state):
    from oracle.trainer import OracleTrainer, default_parameter
    par = default_parameter(rnn='gilr', D=D, algo='sac', sac_batch_size=ROWS * STEPS - 1, max_buffer_transition_num=4 * ROWS * STEPS, **over)
    tr = OracleTrainer(par, OBS, ACT, STEPS, policy_state=policy_state, value_state=value_state, dtype=dtype)
    tr.fill_synthetic(2 * ROWS, STEPS, seed=DATA_SEED)
    torch.manual_seed(UPDATE_SEED)
    np.random.seed(UPDATE_SEED)
    log = tr.train_one_batch()
    return dict(policy=UP.oracle_moments(tr.policy, tr.opt_policy), value=UP.oracle_moments(tr.value, tr.opt_value)), log


@pytest.mark.parametrize('case', list(UPDATE_CASES))
def test_update_inputs_have_no_kink_within_fp32_distance(case):
    """The guard for test_dense_activations_gpu.py's whole-update cases: at their shape and seeds an honest fp32 update (the oracle trainer
    in fp32) stays within a tenth of the bound against the fp64 one - no pre-activation sits so close to relu's kink that fp32 rounding
    flips its side, which would show as a gradient error of the size of a whole term, not of a rounding."""
    from oracle import network as NW
    from oracle.trainer import OracleTrainer, default_parameter
    over = update_overrides(*UPDATE_CASES[case])
    torch.manual_seed(INIT_SEED)
    shapes = OracleTrainer(default_parameter(rnn='gilr', D=D, algo='sac', **over), OBS, ACT, STEPS)
    ps, vs = NW.init_model(shapes.pcfg, 'policy'), NW.init_model(shapes.vcfg, 'value')
    m32, l32 = _one_update(torch.float32, over, ps, vs)
    m64, l64 = _one_update(torch.float64, over, ps, vs)
    rep = UP.compare_update(f'fp32 oracle gilr sac {case} {ROWS}x{STEPS} D={D}', m32, m64, [l32], [l64])
    assert not rep['failures'], rep['failures']                      # MAX_UNDER_FLOOR and LOG_TOL are compare_update's own
    for net, (worst, name) in rep['worst'].items():
        assert worst <= UP.MOMENT_BOUND / 10, (net, name, worst)
