"""The memoryless REDQ baseline `sac_mlp_redq_ensemble_q` on the CPU (no GPU): public interface and constructor contract, the host half
of the transition gather, the pass schedule, and three updates against the recording of the reference (kernels replaced by the CPU oracle
through the `oracle_ops` fixture; the real HIP kernels are checked by tests/test_mlp_redq_gpu.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, nested

LENS = [12, 5, 7, 12, 4, 9, 6]


def mlp_parameter(E=4, D=32, env='synthetic-o5-a3-T12', encoders=False, **over):
    """The flag set of the fixtures (tests/golden/generate_mlp_golden.py): `efc-E` critic stacks, `fc` policy stacks."""
    from test_host_logic import make_parameter
    p = make_parameter('fc', D=D, env=env)
    p.alg_name = 'sac_mlp_redq_ensemble_q'
    p.value_embedding_layer_type, p.value_layer_type = [f'efc-{E}'] * 3, [f'efc-{E}'] * 3
    p.policy_embedding_layer_type, p.policy_layer_type = ['fc'] * 3, ['fc'] * 3
    p.state_action_encoder = encoders
    p.sac_batch_size, p.redq_m, p.utd, p.policy_utd, p.rnn_fix_length = 16, 2, 3, 1, 0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def fill(ring, lens=LENS, seed=9, obs=5, act=3, T=12):
    from test_host_logic import _push, _synth
    rs = np.random.RandomState(seed)
    for n in lens:
        o, a, r = _synth(rs, n, obs, act)
        _push(ring, o, a, r, early_done=(n != T))


def wrapped_ring(width_obs=5, width_act=3):
    """64 transitions of capacity, filled until `ptr` has wrapped and trajectories have been evicted at least twice; 27 columns."""
    from offpolicy_rnn.buffers.transition_buffer.replay_memory import MemoryArray
    ring = MemoryArray(64, 12)
    lens = [12, 5, 7, 12, 4, 9, 6, 11, 12, 3, 8, 12, 7, 5, 10, 12, 6]
    from test_host_logic import _push, _synth
    rs = np.random.RandomState(21)
    wraps = evictions = 0
    for n in lens:
        before, had = ring.ptr, len(ring)
        o, a, r = _synth(rs, n, width_obs, width_act)
        _push(ring, o, a, r, early_done=(n != 12))
        wraps += ring.ptr < before
        evictions += len(ring) <= had
    assert wraps >= 1 and evictions >= 2 and ring.width == 27, (wraps, evictions, ring.width)
    return ring


def val(v):
    return v[0] if isinstance(v, tuple) else v


def golden_trainer(rec, meta, g):
    """A trainer in the state the recording `rec` started from: the recorded initial networks, the ring rebuilt from its stream."""
    from offpolicy_rnn import alg_init
    m = meta[rec]
    alg = alg_init(mlp_parameter(utd=m['utd'], policy_utd=m['policy_utd'], value_max_gradnorm=m['value_max_gradnorm'],
                                 policy_max_gradnorm=m['policy_max_gradnorm'], sac_batch_size=m['sac_batch_size'], redq_m=m['redq_m']))
    alg.policy.load_state_dict(nested(g, 'policy0|'))
    alg.values[0].load_state_dict(nested(g, 'value0|'))
    alg._value_update(tau=0.0)
    fill(alg.replay_buffer, m['lens'], seed=m['ring_seed'])
    return alg


def feed_draws(monkeypatch, g, rec, n):
    """The recorded Gaussian draws, in call order, through utility/rng.py."""
    from offpolicy_rnn.utility import rng
    draws = [g[f'{rec}|noise{k}'] for k in range(n)]
    state = dict(k=0)

    def randn(shape, device, dtype=torch.float32):
        z = torch.from_numpy(draws[state['k']]).to(dtype)
        state['k'] += 1
        assert tuple(z.shape) == tuple(shape), (z.shape, shape)
        return z.to(device)

    monkeypatch.setattr(rng, 'randn', randn)
    return state


def check_against_recording(alg, g, rec, logs, meta, log_rel, log_abs, rtol, atol):
    """Logs and EVERY element of the final parameters against the recording."""
    for it, (log, ref) in enumerate(zip(logs, meta['logs'])):
        assert set(ref) == set(log), set(ref) ^ set(log)
        for k, v in ref.items():
            assert val(log[k]) == pytest.approx(v, rel=log_rel, abs=log_abs), (it, k, val(log[k]), v)
    for name, net in (('policy', alg.policy), ('value', alg.values[0]), ('target', alg.target_values[0])):
        sd = net.state_dict()
        for mod, d in nested(g, f'{rec}|{name}3|').items():
            for k, v in d.items():
                np.testing.assert_allclose(sd[mod][k].detach().cpu(), v, rtol=rtol, atol=atol, err_msg=f'{rec}|{name}3|{mod}.{k}')
    np.testing.assert_allclose(alg.log_sac_alpha.detach().cpu(), g[f'{rec}|log_alpha3'], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ interface and contract
def test_alg_init_returns_the_trainer_and_still_refuses_sac_mlp(oracle_ops):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm.sac_mlp_redq_ensemble_q import SAC_MLP_REDQ_EnsembleQ
    from offpolicy_rnn.buffers.transition_buffer.replay_memory import MemoryArray
    from offpolicy_rnn.utility.alg_init import _OUT_OF_SCOPE
    alg = alg_init(mlp_parameter())
    assert type(alg) is SAC_MLP_REDQ_EnsembleQ and type(alg.replay_buffer) is MemoryArray
    layers = [l for v in (alg.values[0], alg.target_values[0]) for net in (v.embedding_network, v.uni_network) for l in net.layer_list]
    assert len(layers) == 12 and all(l.desire_ndim == 3 for l in layers)
    assert not hasattr(alg, 'Q_guard') and not hasattr(alg, 'target_policy')
    assert 'sac_mlp_redq_ensemble_q' not in _OUT_OF_SCOPE and len(_OUT_OF_SCOPE) == 4
    for name in _OUT_OF_SCOPE:
        with pytest.raises(NotImplementedError, match='sac_mlp_redq_ensemble_q'):
            alg_init(mlp_parameter(alg_name=name))


@pytest.mark.parametrize('stack', ['policy_embedding_layer_type', 'policy_layer_type', 'value_embedding_layer_type', 'value_layer_type'])
def test_a_sequence_layer_in_any_stack_is_refused(oracle_ops, stack):
    from offpolicy_rnn import alg_init
    p = mlp_parameter()
    kept = list(getattr(p, stack))
    setattr(p, stack, [kept[0], 'gru', kept[2]])
    with pytest.raises(AssertionError):
        alg_init(p)


def test_contract_violations_raise(oracle_ops):
    from offpolicy_rnn import alg_init
    with pytest.raises(NotImplementedError, match='continuous actions only'):
        alg_init(mlp_parameter(env='synthetic-o5-d4-T12'))
    with pytest.raises(AssertionError, match='value_net_num'):
        alg_init(mlp_parameter(value_net_num=2))
    with pytest.raises(AssertionError, match='rnn_fix_length'):
        alg_init(mlp_parameter(rnn_fix_length=4))
    with pytest.raises(AssertionError, match='ensemble'):
        alg_init(mlp_parameter(value_embedding_layer_type=['fc'] * 3))


def test_save_and_load_round_trip(oracle_ops, tmp_path):
    """`save()` writes the reference's per-module files for the policy, the critic and its target; `load()` puts them back in place."""
    from offpolicy_rnn import alg_init
    alg = alg_init(mlp_parameter())
    with torch.no_grad():
        alg.log_sac_alpha.fill_(-0.25)
    before = [net.store.flat.clone() for net in alg._state_networks().values()]
    alg.save(str(tmp_path))
    names = os.listdir(tmp_path)
    assert 'ContextualSACValue-0-target-embedding_model.pt' in names and 'ContextualSACPolicy-0-universal_model.pt' in names
    with torch.no_grad():
        for net in alg._state_networks().values():
            net.store.flat.add_(1.0)
        alg.log_sac_alpha.zero_()
    alg.load(str(tmp_path))
    for net, kept in zip(alg._state_networks().values(), before):
        for _, o, n in net.store.slices:                         # (the alignment gaps between tensors belong to nobody)
            assert torch.equal(net.store.flat[o:o + n], kept[o:o + n])
    assert alg.log_sac_alpha.item() == -0.25 and sorted(alg._state_networks()) == ['policy', 'target_value0', 'value0']


# ------------------------------------------------------------------------------------------------ host half of the gather
@pytest.mark.parametrize('n,passes', [(37, 3), (1, 1), (64, 2)])
def test_plan_transitions_draws_and_maps_like_sample_transitions(n, passes):
    """Same numpy stream as `passes` calls of `sample_transitions(n)`, and rows that index the ring rows those calls copy."""
    ring = wrapped_ring()
    np.random.seed(5)
    rows = ring.plan_transitions(n, passes)
    after_plan = np.random.get_state()
    assert rows.dtype == np.int32 and rows.shape == (passes, n) and rows.min() >= 0 and rows.max() < len(ring.memory_buffer)
    np.random.seed(5)
    for p in range(passes):
        tr = ring.sample_transitions(n)
        got = ring.array_to_transition(ring.memory_buffer[rows[p]])
        for name, a, b in zip(tr._fields, tr, got):
            assert (a is None) == (b is None), name
            if a is not None:
                np.testing.assert_array_equal(a, b, err_msg=f'pass {p} {name}')
    after_sample = np.random.get_state()
    assert after_plan[2] == after_sample[2] and np.array_equal(after_plan[1], after_sample[1])


def test_the_ring_mirror_lives_on_the_base_class():
    from offpolicy_rnn.buffers.transition_buffer.nested_replay_memory import NestedMemoryArray
    from offpolicy_rnn.buffers.transition_buffer.replay_memory import MemoryArray
    assert '_mirror' in vars(MemoryArray) and '_mirror' not in vars(NestedMemoryArray)
    ring = wrapped_ring()
    mirror = ring._mirror(torch.device('cpu'))
    assert torch.equal(mirror, torch.from_numpy(ring.memory_buffer)) and ring._dirty == []


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize('utd,policy_utd', [(1, 1), (3, 1), (4, 2), (20, 1), (20, 20)])
def test_pass_schedule_equals_the_reference_rule(oracle_ops, utd, policy_utd):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm.graphed_transition_update import GraphedTransitionUpdate
    alg = alg_init(mlp_parameter(utd=utd, policy_utd=policy_utd))
    want, cnt = [], 0
    for utd_idx in range(utd):                                   # the reference loop's rule, spelled out
        due = (utd_idx + 1) / utd * policy_utd > cnt
        want.append(due)
        cnt += due
    assert GraphedTransitionUpdate.pass_schedule(alg) == want and sum(want) == policy_utd
    assert GraphedTransitionUpdate.refusal(alg) == 'needs a GPU'


# ------------------------------------------------------------------------------------------------ three updates against the reference
META = json.load(open(os.path.join(GOLDEN, 'train_mlp_meta.json'))) if os.path.exists(os.path.join(GOLDEN, 'train_mlp_meta.json')) else {}


@pytest.mark.parametrize('rec', ['utd3', 'utd4'])
def test_three_updates_equal_the_reference_recording(oracle_ops, monkeypatch, rec):
    """The eager CPU pass (`sample_transitions`, the oracle's ops) against the reference's own three `train_one_batch()` calls: logs at
    the bound of `test_discrete_train_one_batch_equals_reference_logs`' GPU twin (2e-3 / 5e-4), parameters at 1e-3 / 2e-5."""
    g = load_golden('train_mlp_redq.npz')
    alg = golden_trainer(rec, META, g)
    fed = feed_draws(monkeypatch, g, rec, META[rec]['draws'])
    torch.manual_seed(200)
    np.random.seed(200)
    logs = [dict(alg.train_one_batch()) for _ in range(3)]
    assert fed['k'] == META[rec]['draws']
    assert all(isinstance(v, float) for log in logs for v in log.values())
    check_against_recording(alg, g, rec, logs, META[rec], 2e-3, 5e-4, 1e-3, 2e-5)
