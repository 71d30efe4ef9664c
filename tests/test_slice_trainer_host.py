"""The slice trainer `sac_rnn_slice` on the CPU (no GPU): the host form of the slice batch against the recorded batches of the reference,
the plan that the device gather consumes, the constructor contract and `alg_init`, the pass schedule, and three updates of every
recording of the reference (kernels replaced by the CPU oracle through the `oracle_ops` fixture; the real HIP kernels are checked by
tests/test_slice_trainer_gpu.py).  Fixtures: tests/golden/generate_slice_golden.py."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, nested
from test_mlp_redq_host import LENS, feed_draws, fill, val, wrapped_ring

META = json.load(open(os.path.join(GOLDEN, 'train_slice_meta.json')))
RECS = list(META['recordings'])
FIELDS = ('state', 'last_state', 'last_action', 'action', 'next_state', 'reward', 'mask', 'start', 'done', 'reward_input', 'timeout')


def slice_parameter(rnn='gru', L=4, n_actions=0, D=32, env=None, **over):
    """The flag set of the fixtures: two separate `fc` critics, no input encoders, batches of 8 slices."""
    from test_host_logic import make_parameter
    p = make_parameter(rnn, D=D, env=env or (f'synthetic-o5-d{n_actions}-T12' if n_actions else 'synthetic-o5-a3-T12'))
    p.alg_name = 'sac_rnn_slice'
    p.value_layer_type = ['fc'] * 3
    p.state_action_encoder = False
    p.value_net_num, p.sac_batch_size, p.rnn_slice_length, p.utd, p.policy_utd, p.sac_alpha = 2, 8, L, 2, 1, 0.2
    for k, v in over.items():
        setattr(p, k, v)
    return p


def fill_slice_ring(ring, n_actions=0, lens=LENS, seed=None):
    seed = META['ring_seed'] if seed is None else seed
    if not n_actions:
        return fill(ring, lens, seed=seed)
    from offpolicy_rnn.buffers.transition_buffer.replay_memory import Transition
    from test_oracle_golden import push_discrete
    rs = np.random.RandomState(seed)
    for n in lens:
        push_discrete(ring, Transition, rs, n, 5, n_actions, 12)


def golden_trainer(rec, **over):
    """-> (a trainer in the state the recording `rec` started from, the recording's arrays, its meta entry)."""
    from offpolicy_rnn import alg_init
    m = META['recordings'][rec]
    g = load_golden(f'train_slice_{rec}.npz')
    alg = alg_init(slice_parameter(m['rnn'], m['rnn_slice_length'], m['n_actions'], utd=m['utd'], policy_utd=m['policy_utd'],
                                   sac_batch_size=m['sac_batch_size'], value_net_num=m['value_net_num'], sac_alpha=m['sac_alpha'], **over))
    alg.policy.load_state_dict(nested(g, f'{rec}|policy0|'))
    for i, v in enumerate(alg.values):
        v.load_state_dict(nested(g, f'{rec}|value0_{i}|'))
    alg._value_update(tau=0.0)
    fill_slice_ring(alg.replay_buffer, m['n_actions'], m['lens'])
    return alg, g, m


def check_against_recording(alg, g, rec, logs, m, log_rel, log_abs, rtol, atol):
    """Logs and EVERY element of the final parameters - the policy, both critics, both targets - against the recording."""
    for it, (log, ref) in enumerate(zip(logs, m['logs'])):
        assert set(ref) == set(log), set(ref) ^ set(log)
        for k, v in ref.items():
            assert val(log[k]) == pytest.approx(v, rel=log_rel, abs=log_abs), (it, k, val(log[k]), v)
    nets = [('policy3', alg.policy)]
    for i, (v, t) in enumerate(zip(alg.values, alg.target_values)):
        nets += [(f'value3_{i}', v), (f'target3_{i}', t)]
    for name, net in nets:
        sd = net.state_dict()
        ref = nested(g, f'{rec}|{name}|')
        assert ref
        for mod, d in ref.items():
            for k, v in d.items():
                np.testing.assert_allclose(sd[mod][k].detach().cpu(), v, rtol=rtol, atol=atol, err_msg=f'{rec}|{name}|{mod}.{k}')
    np.testing.assert_allclose(alg.log_sac_alpha.detach().cpu(), g[f'{rec}|log_alpha3'], rtol=1e-5, atol=1e-6)


def host_window(ring, plan, L, discrete=False):
    """What the device gather writes for one pass of a plan: [batch, L + 1, W] with the pre-step row in slot 0."""
    from offpolicy_rnn.algorithm.sac_rnn_slice import host_slice_batch, pre_step_pairs
    R = ring.name2range
    return host_slice_batch(ring, plan, L, pre_step_pairs(R, discrete), R['done'][0], R['timeout'][0])


# ------------------------------------------------------------------------------------------------ the slice batch
def _new_ring():
    from offpolicy_rnn.buffers.transition_buffer.replay_memory import MemoryArray
    ring = MemoryArray(5000, 12)
    fill_slice_ring(ring)
    return ring


@pytest.mark.parametrize('L', [4, 5])
def test_sample_fix_length_sub_trajs_equals_the_recorded_batch(L):
    """Bit for bit, compared as fp32 (the ring stores fp32, the reference float64); full and tail-padded slices are both in it."""
    g = load_golden('train_slice.npz')
    ring = _new_ring()
    np.random.seed(5)
    batch = ring.sample_fix_length_sub_trajs(8, L)
    assert batch.logp is None
    for name in FIELDS:
        want = g[f'batch_L{L}|{name}'].astype(np.float32)
        got = getattr(batch, name)
        assert got.shape == want.shape == (8, L, want.shape[-1]) and got.dtype == np.float32
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), name
    assert batch.mask.sum() == META['batches'][f'L{L}']['mask_sum'] and 0 < batch.mask.sum() < batch.mask.size


def _check_plan(ring, n, L, passes):
    np.random.seed(5)
    plan = ring.plan_slices(n, L, passes)
    after_plan = np.random.get_state()
    assert plan.dtype == np.int32 and plan.shape == (passes, n, 2)
    assert plan[..., 0].min() >= 0 and plan[..., 1].min() >= 1 and plan[..., 1].max() <= L
    assert (plan[..., 0] + plan[..., 1]).max() <= len(ring.memory_buffer)
    np.random.seed(5)
    padded = 0
    for p in range(passes):
        batch = ring.sample_fix_length_sub_trajs(n, L)
        at = np.arange(L)[None, :]
        valid = at < plan[p, :, 1:2]
        rebuilt = np.where(valid[..., None], ring.memory_buffer[np.where(valid, plan[p, :, 0:1] + at, 0)], 0)      # from `memory_buffer` alone
        got = ring.array_to_transition(rebuilt)
        for name, a, b in zip(batch._fields, batch, got):
            assert (a is None) == (b is None), name
            if a is not None:
                np.testing.assert_array_equal(a, b, err_msg=f'pass {p} {name}')
        assert np.array_equal(batch.mask[..., 0] > 0, valid)      # the mask is exactly the plan's valid count
        padded += int((~valid).sum())
    after_sample = np.random.get_state()
    assert after_plan[2] == after_sample[2] and np.array_equal(after_plan[1], after_sample[1])
    return plan, padded


@pytest.mark.parametrize('n,L,passes', [(8, 4, 1), (37, 7, 3), (13, 2, 2)])
def test_plan_slices_draws_and_maps_like_sample_fix_length_sub_trajs(n, L, passes):
    _, padded = _check_plan(_new_ring(), n, L, passes)
    assert padded > 0


@pytest.mark.parametrize('n,L,passes', [(37, 7, 3), (64, 4, 1)])
def test_plan_slices_on_the_wrapped_ring(n, L, passes):
    """`ptr` wrapped, trajectories evicted: the row behind a trajectory belongs to another one (or to an evicted one), so a tail read from
    the ring would not be zero - the slices still are."""
    ring = wrapped_ring()
    plan, padded = _check_plan(ring, n, L, passes)
    assert padded > 0
    short = plan[plan[..., 1] < L]
    assert any(ring.memory_buffer[r + k].any() for r, k in short if r + k < len(ring.memory_buffer))


def test_the_host_window_holds_the_batch_and_the_pre_step_row():
    ring = wrapped_ring()
    R = ring.name2range
    np.random.seed(5)
    plan = ring.plan_slices(13, 4, 1)[0]
    np.random.seed(5)
    batch = ring.sample_fix_length_sub_trajs(13, 4)
    w = host_window(ring, plan, 4)
    stored = np.concatenate([f for f in batch if f is not None], axis=-1)
    fix = stored.copy()
    fix[..., R['done'][0]][stored[..., R['timeout'][0]] > 0] = 0
    assert np.array_equal(w[:, 1:], fix) and (fix != stored).any()
    first = ring.array_to_transition(ring.memory_buffer[plan[:, 0]])
    pre = ring.array_to_transition(w[:, 0])
    for dst, src in (('next_state', 'state'), ('state', 'last_state'), ('action', 'last_action'), ('reward', 'reward_input')):
        assert np.array_equal(getattr(pre, dst), getattr(first, src)), dst
    for name in ('last_state', 'last_action', 'mask', 'start', 'done', 'reward_input', 'timeout'):
        assert not getattr(pre, name).any(), name


# ------------------------------------------------------------------------------------------------ interface and contract
def test_alg_init_returns_the_trainer_and_refuses_a_zero_slice_length(oracle_ops):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm.sac_rnn_slice import SACRNNSlice
    from offpolicy_rnn.buffers.transition_buffer.replay_memory import MemoryArray
    from offpolicy_rnn.utility.alg_init import _OUT_OF_SCOPE
    alg = alg_init(slice_parameter())
    assert type(alg) is SACRNNSlice and type(alg.replay_buffer) is MemoryArray and alg.slice_length == 4
    assert len(alg.values) == len(alg.target_values) == len(alg.optimizers_value) == 2
    assert not hasattr(alg, 'Q_guard') and not hasattr(alg, 'target_policy')
    assert sorted(alg._state_networks()) == ['policy', 'target_value0', 'target_value1', 'value0', 'value1']
    assert _OUT_OF_SCOPE == ('sac_no_train', 'sac_mlp', 'sac_mlp_redq', 'sac_rnn_slice')
    with pytest.raises(NotImplementedError, match='sac_mlp_redq_ensemble_q'):
        alg_init(slice_parameter(rnn_slice_length=0))
    assert type(alg_init(slice_parameter(n_actions=4))) is SACRNNSlice


def test_contract_violations_raise(oracle_ops):
    from offpolicy_rnn import alg_init
    with pytest.raises(ValueError, match='one token'):
        alg_init(slice_parameter(rnn_slice_length=1))
    for stack, ids in (('value_layer_type', ['efc-4'] * 3), ('value_embedding_layer_type', ['fc', 'elru-4', 'fc']),
                       ('policy_embedding_layer_type', ['fc', 'econv1d_4-2', 'fc']), ('policy_layer_type', ['fc', 'eln-4', 'fc'])):
        with pytest.raises(ValueError, match='member axis'):
            alg_init(slice_parameter(**{stack: ids}))
    for stack in ('value_embedding_layer_type', 'policy_embedding_layer_type'):
        with pytest.raises(NotImplementedError, match='sequence table'):
            alg_init(slice_parameter(**{stack: ['fc', 'cgpt_h1_l1_p0_ml32', 'fc']}))


def test_a_process_group_is_refused(oracle_ops, monkeypatch):
    import torch.distributed as dist
    from offpolicy_rnn import alg_init
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match='process group'):
        alg_init(slice_parameter())


def test_save_and_load_round_trip(oracle_ops, tmp_path):
    from offpolicy_rnn import alg_init
    alg = alg_init(slice_parameter())
    with torch.no_grad():
        alg.log_sac_alpha.fill_(-0.25)
    before = [net.store.flat.clone() for net in alg._state_networks().values()]
    alg.save(str(tmp_path))
    names = os.listdir(tmp_path)
    assert 'ContextualSACValue-1-target-embedding_model.pt' in names and 'ContextualSACPolicy-0-universal_model.pt' in names
    with torch.no_grad():
        for net in alg._state_networks().values():
            net.store.flat.add_(1.0)
        alg.log_sac_alpha.zero_()
    alg.load(str(tmp_path))
    for net, kept in zip(alg._state_networks().values(), before):
        for _, o, n in net.store.slices:
            assert torch.equal(net.store.flat[o:o + n], kept[o:o + n])
    assert alg.log_sac_alpha.item() == -0.25


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize('utd,policy_utd', [(1, 1), (2, 1), (3, 2), (20, 1), (20, 20)])
def test_pass_schedule_equals_the_reference_rule(oracle_ops, utd, policy_utd):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm.graphed_transition_update import GraphedTransitionUpdate
    alg = alg_init(slice_parameter(utd=utd, policy_utd=policy_utd))
    want, cnt = [], 0
    for utd_idx in range(utd):                                   # the reference loop's rule, spelled out
        due = (utd_idx + 1) / utd * policy_utd > cnt
        want.append(due)
        cnt += due
    assert GraphedTransitionUpdate.pass_schedule(alg) == want and sum(want) == policy_utd
    assert GraphedTransitionUpdate.refusal(alg) == 'needs a GPU' and alg.update_driver() is GraphedTransitionUpdate
    assert alg.graph_plan_words() == 16 and alg.graph_subset_size() == 0 and len(alg.graph_optimizers()[0]) == 2


# ------------------------------------------------------------------------------------------------ three updates against the reference
@pytest.mark.parametrize('rec', RECS)
def test_three_updates_equal_the_reference_recording(oracle_ops, monkeypatch, rec):
    """The eager CPU pass (the host window, the oracle's ops, the torch spelling of target and losses) against the reference's own three
    `train_one_batch()` calls: logs at 2e-3 / 5e-4, every parameter element at 1e-3 / 2e-5 (the bars of tests/test_trainer_gpu.py and of
    `test_mlp_redq_host.check_against_recording`).  No ring stream meets the residue rule for these recordings
    (train_slice_meta.json `residue_rule_met`, `residue_elements`; the generator's docstring says why); every element is held all the same."""
    alg, g, m = golden_trainer(rec)
    fed = feed_draws(monkeypatch, g, rec, m['draws'])
    torch.manual_seed(200)
    np.random.seed(200)
    logs = [dict(alg.train_one_batch()) for _ in range(3)]
    assert fed['k'] == m['draws']
    assert all(isinstance(v, float) for log in logs for v in log.values())
    check_against_recording(alg, g, rec, logs, m, 2e-3, 5e-4, 1e-3, 2e-5)
