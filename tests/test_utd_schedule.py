"""The captured update at update-to-data ratios above one (algorithm/graphed_update.py): its unit is the PASS - one iteration of the
`utd` loop - and `GraphedUpdate.step()` walks the schedule of the coming step.  Host side only: the schedule helper against the
reference's loop, the number of launch sequences derived from it, the one seam between trainer and driver, and the log with a fixed slot
per key.  CPU trainers as in tests/test_host_logic.py `test_actor_due_has_one_spelling`."""
import pytest
import torch

from test_host_logic import make_parameter

# (utd, policy_utd, policy_update_per, grad_num)
CASES = [(1, 1, 1, 0), (1, 1, 2, 0), (1, 1, 2, 1), (2, 1, 1, 0), (2, 2, 2, 1), (4, 2, 1, 0), (3, 0, 1, 0), (4, 4, 1, 0)]


def reference_flags(utd, policy_utd, per, grad_num):
    """The reference's loop: it counts the actor steps of the update, `(utd_idx + 1) / utd * policy_utd > count`, behind
    `grad_num % policy_update_per == 0`."""
    count, flags = 0, []
    for utd_idx in range(utd):
        due = grad_num % per == 0 and (utd_idx + 1) / utd * policy_utd > count
        flags.append(bool(due))
        count += bool(due)
    return flags


@pytest.fixture
def cpu_alg(oracle_ops):
    from offpolicy_rnn import alg_init
    return alg_init(make_parameter('gru'))


@pytest.mark.parametrize('utd,policy_utd,per,grad_num', CASES)
def test_pass_schedule_walks_the_reference_loop(cpu_alg, utd, policy_utd, per, grad_num):
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    alg, par = cpu_alg, cpu_alg.parameter
    par.utd, par.policy_utd, par.policy_update_per, alg.grad_num = utd, policy_utd, per, grad_num
    flags = GraphedUpdate.pass_schedule(alg)
    assert flags == reference_flags(utd, policy_utd, per, grad_num)
    assert len(flags) == utd and all(type(f) is bool for f in flags)
    assert alg.grad_num == grad_num


@pytest.mark.parametrize('utd,policy_utd,per,grad_num', CASES)
def test_two_launch_sequences_exactly_when_two_passes_can_differ(cpu_alg, utd, policy_utd, per, grad_num):
    """Over a whole run `grad_num` takes every residue of `policy_update_per`: the flags a run can show are those of one period."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    alg, par = cpu_alg, cpu_alg.parameter
    par.utd, par.policy_utd, par.policy_update_per, alg.grad_num = utd, policy_utd, per, grad_num
    run = {f for g in range(per) for f in reference_flags(utd, policy_utd, per, g)}
    assert GraphedUpdate.launch_sequences(alg) == (2 if run == {True, False} else 1)
    assert alg.grad_num == grad_num                               # walked, then put back
    # the published flag sets: utd = 1 with policy_update_per = 2 alternates, REDQ's utd = 20 with policy_utd = 1 mixes within a step
    assert GraphedUpdate.launch_sequences(alg) == {(1, 1, 1): 1, (1, 1, 2): 2, (2, 1, 1): 2, (2, 2, 2): 2, (4, 2, 1): 2, (3, 0, 1): 1,
                                                   (4, 4, 1): 1}[(utd, policy_utd, per)]


def test_no_refusal_left_for_utd_and_one_seam_to_the_trainer():
    """`refusal()` names no update-to-data ratio any more; the driver holds no copy of the phase sequence - it hands the trainer the
    position of the pass (`pass_position`) and the trainer's `_train_one_batch` runs `_one_pass` once for it."""
    import inspect
    from offpolicy_rnn.algorithm import graphed_update
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    from offpolicy_rnn.algorithm.sac_full_length_rnn_ensembleQ import SACFullLengthRNNEnsembleQ as T
    assert 'utd' not in inspect.getsource(GraphedUpdate.refusal)
    src = inspect.getsource(graphed_update)
    for phase in ('_hidden_states(', '_critic_step(', '_actor_step(', '_value_update(', '_one_pass('):
        assert phase not in src, phase
    assert 'self._graph.pass_position()' in inspect.getsource(T._train_one_batch)
    assert list(inspect.signature(T._one_pass).parameters) == ['self', 'utd_idx', 'actor_steps', 'scal', 'host']
    for cls in T.__subclasses__():                                # the subclasses override phases, not the loop
        assert '_one_pass' not in vars(cls) and '_train_one_batch' not in vars(cls)


def test_eager_loop_is_the_sum_of_its_passes(cpu_alg, monkeypatch):
    """`_train_one_batch` keeps the loop: `utd` calls of `_one_pass` with the running count of actor steps, one `_log` with the last
    pass's batch; while a driver is attached, one call at the position it hands over."""
    alg, par = cpu_alg, cpu_alg.parameter
    par.utd, par.policy_utd, par.policy_update_per, alg.grad_num = 4, 2, 1, 0
    calls, logged = [], []

    def one_pass(utd_idx, actor_steps, scal, host):
        calls.append((utd_idx, actor_steps))
        due = bool(alg._actor_due(utd_idx, actor_steps))
        scal['critic_loss'] = torch.tensor(float(utd_idx))
        if due:
            scal['actor_loss'] = torch.tensor(10.0 + utd_idx)
        return due, 100 + utd_idx, 7 + utd_idx
    monkeypatch.setattr(alg, '_one_pass', one_pass)
    monkeypatch.setattr(alg, '_log', lambda scal, host, batch_size, real_rows: logged.append((dict(scal), batch_size, real_rows)))
    alg._train_one_batch()
    assert calls == [(0, 0), (1, 1), (2, 1), (3, 2)]
    assert len(logged) == 1 and logged[0][1:] == (103, 10)
    assert float(logged[0][0]['critic_loss']) == 3.0 and float(logged[0][0]['actor_loss']) == 12.0

    class Driver:
        def pass_position(self):
            return 2, 1
    del calls[:], logged[:]
    alg._graph = Driver()
    try:
        alg._train_one_batch()
    finally:
        alg._graph = None
    assert calls == [(2, 1)] and logged[0][1:] == (102, 9)


def test_deferred_log_reads_named_slots():
    """The step's log names some slots of a buffer that holds one slot per key: values by slot, `actor_loss` still a 1-tuple, host
    entries on top, and a key that is not named does not appear although its slot holds an (older) value."""
    from offpolicy_rnn.utility.deferred_log import DeferredLog
    buf = torch.tensor([0.5, 7.0, 8.0, 9.0, 1.5])                  # slots: critic_loss, log_prob, actor_loss, alpha_loss, log_alpha
    log = DeferredLog(['critic_loss', 'log_alpha'], buf, None, dict(real_batch_size=47), index=[0, 4])
    assert dict(log) == dict(critic_loss=0.5, log_alpha=1.5, real_batch_size=47)
    log = DeferredLog(['critic_loss', 'actor_loss', 'log_alpha'], buf, None, {}, index=[0, 2, 4])
    assert log['actor_loss'] == (8.0,) and 'log_prob' not in log
    assert dict(DeferredLog(['a', 'b'], torch.tensor([1.0, 2.0]), None)) == dict(a=1.0, b=2.0)      # without an index: in key order
