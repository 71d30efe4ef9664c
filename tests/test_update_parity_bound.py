"""Is the bound of tests/update_parity.py fair?  One update of the fp32 oracle trainer and one of the fp64 oracle trainer on identical
weights, data and seeds at the published width (D = 256, efc-8 critic, REDQ m = 2, obs 17, act 6), 8 rows x 64 steps, through the same
comparison the GPU test (test_update_published_width_gpu.py) sends the product through: an honest fp32 implementation of the update
must stay well inside the bound (<= 1/10 of it), and the comparison must notice a tensor that is off by 1e-3 or missing.

Measured: gilr SAC worst tensor 8.0e-7 (policy) / 1.5e-6 (value) of the tensor's scale, lru TD3 4.8e-6 / 1.2e-6; bound 2e-4, so 2e-5 is
asserted.  gilr has two tensors under the floor in each network - the layer's `layer_norm.weight` / `.bias`, which its forward never
reads (no gradient at all) - lru none.  Worst logged scalar: 0.6 % of its tolerance."""
import copy

import numpy as np
import pytest
import torch

import update_parity as UP

ROWS, STEPS, OBS, ACT = 8, 64, 17, 6


def _one_update(rnn, algo, dtype, policy_state, value_state):
    from oracle.trainer import OracleTrainer, default_parameter
    par = default_parameter(rnn=rnn, algo=algo, sac_batch_size=ROWS * STEPS - 1, max_buffer_transition_num=4 * ROWS * STEPS)
    tr = OracleTrainer(par, OBS, ACT, STEPS, policy_state=policy_state, value_state=value_state, dtype=dtype)
    tr.fill_synthetic(2 * ROWS, STEPS, seed=0)
    torch.manual_seed(200)
    np.random.seed(200)
    log = tr.train_one_batch()
    assert all(t.dtype == dtype for net in (tr.policy, tr.value, tr.target_value) for t in _tensors(net)) and tr.log_alpha.dtype == dtype
    assert all(s['exp_avg'].dtype == dtype for opt in (tr.opt_policy, tr.opt_value) for s in opt.state.values())
    return dict(policy=UP.oracle_moments(tr.policy, tr.opt_policy), value=UP.oracle_moments(tr.value, tr.opt_value)), log


def _above_floor(ref):
    size = {k: t.abs().max().item() for k, t in ref.items()}
    return {k: v for k, v in size.items() if v >= UP.FLOOR * max(size.values())}


def _tensors(net):
    return [t for d in net.values() for t in d.values()]


@pytest.fixture(scope='module', params=[('gilr', 'sac'), ('lru', 'td3')], ids=lambda p: '-'.join(p))
def runs(request):
    from oracle import network as NW
    from oracle.trainer import OracleTrainer, default_parameter
    rnn, algo = request.param
    torch.manual_seed(1)
    shapes = OracleTrainer(default_parameter(rnn=rnn, algo=algo), OBS, ACT, STEPS)
    ps, vs = NW.init_model(shapes.pcfg, 'policy'), NW.init_model(shapes.vcfg, 'value')
    m32, l32 = _one_update(rnn, algo, torch.float32, ps, vs)
    m64, l64 = _one_update(rnn, algo, torch.float64, ps, vs)
    return f'fp32 oracle {rnn} {algo} {ROWS}x{STEPS}', m32, l32, m64, l64


def test_fp32_oracle_is_well_inside_the_bound(runs):
    label, m32, l32, m64, l64 = runs
    rep = UP.compare_update(label, m32, m64, [l32], [l64])
    assert not rep['failures'], rep['failures']
    for net, (worst, name) in rep['worst'].items():
        assert worst <= UP.MOMENT_BOUND / 10, (net, name, worst)


def test_a_tensor_off_by_1e_3_fails(runs):
    label, m32, l32, m64, l64 = runs
    for net in m32:
        above = _above_floor(m64[net])
        for name in (max(above, key=above.get), min(above, key=above.get)):       # the largest tensor and the smallest the floor does not cover
            bad = copy.copy(m32)
            bad[net] = dict(m32[net])
            bad[net][name] = m32[net][name] * (1 + 1e-3)
            rep = UP.compare_update(label + f' [{net} {name} x (1 + 1e-3)]', bad, m64, [l32], [l64])
            assert len(rep['failures']) == 1 and f'{net} {name}:' in rep['failures'][0], rep['failures']


def test_the_smallest_tensor_above_the_floor_zeroed_fails(runs):
    label, m32, l32, m64, l64 = runs
    for net in m32:
        above = _above_floor(m64[net])
        name = min(above, key=above.get)
        bad = copy.copy(m32)
        bad[net] = dict(m32[net])
        bad[net][name] = torch.zeros_like(m32[net][name])
        rep = UP.compare_update(label + f' [{net} {name} zeroed]', bad, m64, [l32], [l64])
        assert len(rep['failures']) == 1 and f'{net} {name}:' in rep['failures'][0], rep['failures']


def test_a_scalar_off_by_1e_3_fails(runs):
    label, m32, l32, m64, l64 = runs
    bad = dict(l32, critic_loss=l32['critic_loss'] * (1 + 1e-3))
    rep = UP.compare_update(label + ' [critic_loss x (1 + 1e-3)]', m32, m64, [bad], [l64])
    assert len(rep['failures']) == 1 and 'critic_loss' in rep['failures'][0], rep['failures']
