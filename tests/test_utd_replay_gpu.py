"""`GraphedUpdate.step()` at update-to-data ratios above one: a step is `utd` passes, each replayed from the graph of its own launch
sequence (algorithm/graphed_update.py).  One trainer is stepped by the eager `train_one_batch()`, a twin by
`GraphedUpdate(alg, warmup=1).step()`.  Fixtures, seeds and tolerances of tests/test_trainer_gpu.py
`test_graphed_update_equals_the_eager_update` (fp32 families rtol 2e-5, atol 2e-7; cgpt, whose attention runs in bf16, 5e-3, 3e-4), of
its dropout twin, of tests/test_device_rmask_gpu.py, tests/test_data_parallel_gpu.py (rtol 2e-4, atol 2e-6) and
tests/test_discrete_update_gpu.py.  The smallest shapes at which the captured update is exercised: eight trajectories of 12 steps (or
ragged), observation width 5, action width 3, batches of 47 transitions."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
ACTOR_KEYS = {'log_prob', 'actor_loss', 'alpha_loss', 'policy_l2_norm_square', 'policy_grad_norm'}
RAGGED = (12, 9, 7, 12, 5, 12, 10, 8)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')


def _quiet(patcher):
    """Actor noise off: the captured generator draws from graph-safe offsets, so noise cannot agree draw for draw."""
    from offpolicy_rnn.utility import rng
    patcher.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.zeros(tuple(shape), dtype=dtype, device=device))
    patcher.setattr(rng, 'randn_like', lambda t: torch.zeros_like(t))


def _val(v):
    return v[0] if isinstance(v, tuple) else v


def _state(alg):
    return [alg.policy.store.flat.detach().clone(), alg.values[0].store.flat.detach().clone(), alg.target_values[0].store.flat.detach().clone(),
            alg.log_sac_alpha.detach().clone()]


def _small(rnn, algo, utd, policy_utd, per, ragged=False, **extra):
    from test_host_logic import _push, _synth, make_parameter
    from offpolicy_rnn import alg_init
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter(rnn, algo=algo, sac_batch_size=4 * 12 - 1, cuda_inference=True, utd=utd, policy_utd=policy_utd,
                                  policy_update_per=per, **extra))
    rs = np.random.RandomState(3)
    for i in range(8):
        n = RAGGED[i] if ragged else 12
        o, a, r = _synth(rs, n, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=(n != 12))
    np.random.seed(11)
    return alg


def _step_both(build, steps, warmup=1, max_graphs=None):
    """`steps` eager updates of one trainer, `steps` `step()` calls of its twin -> both trainers, the driver, the logs, the actor flags of
    every step and the numpy stream's state behind each run."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    eager = build()
    logs_e = []
    for _ in range(steps):
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    torch.cuda.synchronize()
    np_e = np.random.get_state()
    graphed = build()
    assert GraphedUpdate.refusal(graphed) is None
    st0 = np.random.get_state()[1].copy()
    g = GraphedUpdate(graphed, warmup=warmup, max_graphs=max_graphs)
    assert (np.random.get_state()[1] == st0).all()              # the constructor consumes no draw
    logs_g, flags = [], []
    for _ in range(steps):
        flags.append(GraphedUpdate.pass_schedule(graphed))
        logs_g.append(dict(g.step()))
        graphed.grad_num += 1
    torch.cuda.synchronize()
    np_g = np.random.get_state()
    return eager, graphed, g, logs_e, logs_g, flags, (np_e, np_g)


def _same_stream(np_e, np_g):
    """Plan and subset were drawn in the eager loop's order, pass by pass: the two runs leave numpy's stream in the same state."""
    assert np_e[0] == np_g[0] and (np_e[1] == np_g[1]).all() and np_e[2:] == np_g[2:]


def _compare(eager, graphed, logs_e, logs_g, flags, rtol, atol, log_rtol):
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), _state(graphed), _state(eager)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=rtol, atol=atol, err_msg=nm)
    assert len(logs_e) == len(logs_g) == len(flags)
    for le, lg, fl in zip(logs_e, logs_g, flags):
        assert set(le) == set(lg), (sorted(le), sorted(lg))
        if not any(fl):                                         # a step none of whose passes ran the actor step carries no actor key
            assert not ACTOR_KEYS & set(lg), sorted(lg)
        else:
            assert isinstance(lg['actor_loss'], tuple) and len(lg['actor_loss']) == 1
        for k in le:
            ve, vg = _val(le[k]), _val(lg[k])
            print(f'{k}: eager {ve!r} stepped {vg!r}')
            assert abs(ve - vg) <= log_rtol * max(1.0, abs(ve)), (k, ve, vg)


CASES = [('gilr', 'sac', 2, 1, 1, 4, False), ('smamba_s8_c4_b1_nln', 'sac', 2, 2, 2, 4, False), ('gru', 'sac', 4, 2, 1, 3, False),
         ('lru', 'td3', 2, 1, 1, 4, False), ('cgpt_h1_l2_p0.0_ml64_rms', 'td3', 2, 1, 1, 4, False),
         ('smamba_s8_c4_b1_nln', 'sac', 2, 1, 1, 8, True)]


@pytest.mark.parametrize('rnn,algo,utd,policy_utd,per,steps,ragged', CASES)
def test_stepped_passes_equal_the_eager_update(rnn, algo, utd, policy_utd, per, steps, ragged, monkeypatch):
    _need_gpu()
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    _quiet(monkeypatch)
    if rnn == 'gru':
        monkeypatch.setenv('RESEL_GRU_BATCH', '1')              # the lockstep recurrences
    assert utd * steps <= 16
    eager, graphed, g, logs_e, logs_g, flags, streams = _step_both(
        lambda: _small(rnn, algo, utd, policy_utd, per, ragged), steps, max_graphs=2 if ragged else None)
    try:
        passes = utd * steps
        sequences = GraphedUpdate.launch_sequences(graphed)
        print(f'graphs {sorted(g.graphs)}, eager passes {g.eager_fallbacks} of {passes}, launch sequences {sequences}')
        assert g._steps == passes
        if rnn == 'gru':
            assert graphed.gru_batch
        if ragged:
            assert len(g.graphs) <= 2 and passes - g.eager_fallbacks >= 1, 'no pass was replayed'
        else:                                                   # one recording per launch sequence; a shape is recorded on its second visit
            assert sequences == 2 and g._sequences == 2
            assert sorted(k[-1] for k in g.graphs) == [False, True]
            assert g.eager_fallbacks <= 1 + sequences
        rtol, atol = (5e-3, 3e-4) if rnn.startswith('cgpt') else (2e-5, 2e-7)
        _compare(eager, graphed, logs_e, logs_g, flags, rtol, atol, max(rtol, 100 * atol if rnn.startswith('cgpt') else 0))
        _same_stream(*streams)
    finally:
        g.close()


def test_dropout_masks_move_on_with_every_pass(monkeypatch):
    """cgpt with dropout 0.1, td3, utd = 2: the same object stepped through replays (warmup 1) and through its eager path (the warm-up
    never ends) agrees step by step, to the bounds of tests/test_trainer_gpu.py
    `test_graphed_update_with_dropout_replays_what_its_eager_path_runs`; no mask is drawn twice (the critic losses of consecutive
    steps differ) and the device word the masks are keyed on has advanced once per pass either way."""
    _need_gpu()
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    _quiet(monkeypatch)
    runs = []
    for warmup in (1, 10 ** 6):
        alg = _small('cgpt_h1_l2_p0.1_ml64_rms', 'td3', 2, 1, 1)
        g = GraphedUpdate(alg, warmup=warmup)
        logs, words = [], []
        try:
            for _ in range(3):
                logs.append(dict(g.step()))
                alg.grad_num += 1
                words.append(int(g._drop_base.item()))
            torch.cuda.synchronize()
        finally:
            runs.append((logs, alg.policy.store.flat.detach().clone(), alg.values[0].store.flat.detach().clone(), len(g.graphs),
                         g.eager_fallbacks, words))
            g.close()
    (lg, pg, vg, ng, eg, wg), (le, pe, ve, ne, ee, we) = runs
    assert ng == 2 and eg <= 3 and ne == 0 and ee == 6
    assert wg == we == [2 * (i + 1) * GraphedUpdate.DROP_STRIDE for i in range(3)]
    np.testing.assert_allclose(pg.cpu().numpy(), pe.cpu().numpy(), rtol=5e-3, atol=1e-4)
    np.testing.assert_allclose(vg.cpu().numpy(), ve.cpu().numpy(), rtol=5e-3, atol=1e-4)
    for a, b in zip(lg, le):
        assert set(a) == set(b)
        for k in a:
            assert abs(_val(a[k]) - _val(b[k])) <= 1e-2 * max(1.0, abs(_val(b[k]))), (k, a[k], b[k])
    assert len({round(_val(l['critic_loss']), 7) for l in lg}) == len(lg)


def test_randomised_masks_at_utd_two(monkeypatch):
    """gru, sac, utd = 2 with `randomize_mask`: 16 loss positions of the 47 drawn - every pass is thinned; its selection words travel
    in the pass's own staging slot.  rtol 2e-5, atol 1e-6 as tests/test_device_rmask_gpu.py `_run_pair`."""
    _need_gpu()
    _quiet(monkeypatch)
    eager, graphed, g, logs_e, logs_g, flags, streams = _step_both(
        lambda: _small('gru', 'sac', 2, 1, 1, randomize_mask=True, valid_number_post_randomized=16), 4)
    try:
        pl = g._plan
        assert 'sel' in pl and float(graphed._stats[1]) < pl['total_size'], 'the selection thinned nothing'
        assert len(g.graphs) == 2 and g.eager_fallbacks <= 3
        _compare(eager, graphed, logs_e, logs_g, flags, 2e-5, 1e-6, 2e-5)
        _same_stream(*streams)
    finally:
        g.close()


def test_discrete_actions_at_utd_two(monkeypatch):
    """The graphed trainer of tests/test_discrete_update_gpu.py (fused head, target and losses) with utd = 2, policy_utd = 1."""
    _need_gpu()
    from test_discrete_rollout_gpu import _update_alg
    monkeypatch.setenv('RESEL_DISCRETE_FUSED', '1')

    def build():
        alg = _update_alg('gru')
        alg.parameter.utd, alg.parameter.policy_utd = 2, 1
        return alg
    eager, graphed, g, logs_e, logs_g, flags, streams = _step_both(build, 3)
    try:
        assert flags == [[True, False]] * 3                     # the actor keys of every log come from the FIRST pass of its step
        assert len(g.graphs) == 2 and g.eager_fallbacks == 2
        _compare(eager, graphed, logs_e, logs_g, flags, 2e-5, 2e-7, 2e-5)
        _same_stream(*streams)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------ data parallel
LENS = (12, 5, 7, 12, 9)                              # tests/test_data_parallel_gpu.py: five trajectories, split over two ranks
SPLIT = ((0, 2, 4), (1, 3))


class _Patch:                                         # worker processes patch for good; the pytest process passes monkeypatch
    def setattr(self, obj, name, val):
        setattr(obj, name, val)


def _dp_build(rnn, keep, batch, patcher=None):
    sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'recurrent-offpolicy-rl_amd')]
    from test_host_logic import _push, _synth, make_parameter
    from offpolicy_rnn import alg_init
    _quiet(patcher or _Patch())
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter(rnn, sac_batch_size=batch, cuda_inference=True, utd=2, policy_utd=1))
    rs = np.random.RandomState(3)
    for i, n in enumerate(LENS):
        o, a, r = _synth(rs, n, 5, 3)
        if keep is None or i in keep:
            _push(alg.replay_buffer, o, a, r, early_done=(n != 12))
    torch.manual_seed(11)
    torch.cuda.manual_seed_all(11)
    np.random.seed(11)
    alg._subset_rng = np.random.RandomState(int(alg.parameter.seed) + 7919)     # the stream data-parallel ranks share
    return alg


def _dp_result(alg):
    return dict(policy=alg.policy.store.flat[:alg.policy.store.numel].detach().cpu(),
                value=alg.values[0].store.flat[:alg.values[0].store.numel].detach().cpu(),
                alpha=alg.log_sac_alpha.detach().cpu(), guard=alg.Q_guard.state.detach().cpu())


def _dp_worker(rank, world, port, rnn, out_dir, steps):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    alg = _dp_build(rnn, SPLIT[rank], sum(LENS[i] for i in SPLIT[rank]))
    alg._subset_rng = None                            # product default under world > 1: the shared stream
    alg.grad_sync.__init__()
    assert alg.grad_sync.world == world and alg.device.type == 'cuda' and alg.grad_sync.backend == 'gloo'
    assert GraphedUpdate.refusal(alg) is None, GraphedUpdate.refusal(alg)
    gu = GraphedUpdate(alg, warmup=1)
    for _ in range(steps):
        gu.step()
        alg.grad_num += 1
    torch.cuda.synchronize()
    res = _dp_result(alg)
    res['segments'] = {bool(k[-1]): len(v['segs']) for k, v in gu.graphs.items()}
    res['eager'] = gu.eager_fallbacks
    res['calls'] = dict(alg.grad_sync.calls)
    gu.close()
    torch.save(res, os.path.join(out_dir, f'rank{rank}.pt'))
    dist.destroy_process_group()


def test_two_ranks_step_passes_cut_at_their_exchanges(tmp_path, monkeypatch):
    """Two `gloo` ranks on one GPU with disjoint rows, gilr, utd = 2, policy_utd = 1, two steps through `GraphedUpdate`: passes 0 and 1
    run eagerly (warm-up, first visit), passes 2 and 3 are recorded and replayed - cut at their gradient exchanges, three segments with
    the actor step, two without.  The ranks agree bit for bit and match the single-process eager utd = 2 run over the union batch."""
    _need_gpu()
    from test_data_parallel import _free_port
    rnn, steps = 'gilr', 2
    mp.spawn(_dp_worker, args=(2, _free_port(), rnn, str(tmp_path), steps), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f'rank{i}.pt')) for i in range(2))
    for k in ('policy', 'value', 'alpha', 'guard'):
        assert torch.equal(r0[k], r1[k]), f'{k} diverged across ranks'
    assert r0['segments'] == r1['segments'] == {True: 3, False: 2}
    assert r0['eager'] == 2
    # per step: two critic steps + one actor step = 3 flat-gradient all-reduces
    assert r0['calls']['all_reduce_sum'] == 3 * steps and r0['calls']['all_reduce_max'] == 0, r0['calls']
    one = _dp_build(rnn, None, sum(LENS), patcher=monkeypatch)
    for _ in range(steps):
        one.train_one_batch()
        one.grad_num += 1
    torch.cuda.synchronize()
    ref = _dp_result(one)
    for k in ('policy', 'value', 'alpha', 'guard'):
        np.testing.assert_allclose(r0[k].numpy(), ref[k].numpy(), rtol=2e-4, atol=2e-6, err_msg=k)
