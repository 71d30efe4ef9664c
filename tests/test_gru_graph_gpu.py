"""The gru trainer with its concurrent recurrences in one launch (RESEL_GRU_BATCH=1, the default) or one after another
(RESEL_GRU_BATCH=0, the serial form): either way the update is a launch sequence on the current stream and `GraphedUpdate` replays it.  Pattern, helpers and tolerances of tests/test_trainer_gpu.py `test_graphed_update_equals_the_eager_update`
(fp32 families: rtol 2e-5, atol 2e-7, 1e-6 past 16 chained updates) and of tests/test_data_parallel_gpu.py (rtol 5e-4, atol 5e-6).
No gru trainer creates a stream of its own: `test_no_gru_form_is_refused_or_creates_a_stream` counts them."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')


def _quiet(monkeypatch):
    from offpolicy_rnn.utility import rng
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.zeros(tuple(shape), dtype=dtype, device=device))


def _small(algo='sac', per=1, ragged=False, seed=0, **extra):
    from test_host_logic import _push, _synth, make_parameter
    from offpolicy_rnn import alg_init
    torch.manual_seed(seed)
    np.random.seed(seed)
    alg = alg_init(make_parameter('gru', algo=algo, sac_batch_size=4 * 12 - 1, cuda_inference=True, policy_update_per=per, **extra))
    rs = np.random.RandomState(3)
    for i in range(8):
        n = (12, 9, 7, 12, 5, 12, 10, 8)[i] if ragged else 12
        o, a, r = _synth(rs, n, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=(n != 12))
    np.random.seed(11)
    return alg


def _state(alg):
    return [alg.policy.store.flat.detach().clone(), alg.values[0].store.flat.detach().clone(), alg.target_values[0].store.flat.detach().clone(),
            alg.log_sac_alpha.detach().clone()]


def _val(v):
    return v[0] if isinstance(v, tuple) else v


def _count_new_streams(monkeypatch):
    """Replace `torch.cuda.Stream` by a subclass that counts the streams CREATED through it (a wrapper object around an existing
    stream - what `torch.cuda.current_stream()` returns - passes stream_id / stream_ptr and is not one)."""
    made = []

    class CountingStream(torch.cuda.Stream):
        def __new__(cls, *args, **kwargs):
            if 'stream_id' not in kwargs and 'stream_ptr' not in kwargs:
                made.append((args, kwargs))
            return super().__new__(cls, *args, **kwargs)
    monkeypatch.setattr(torch.cuda, 'Stream', CountingStream)
    return made


@pytest.mark.parametrize('algo', ['sac', 'td3'])
def test_no_gru_form_is_refused_or_creates_a_stream(algo, monkeypatch):
    """Both forms of the gru trainer are linear launch sequences on the current stream: `GraphedUpdate` refuses neither, and building
    the trainer and running two eager updates creates no `torch.cuda.Stream` (what keeps a fork / join out of every capture)."""
    _need_gpu()
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    made = _count_new_streams(monkeypatch)
    probe = torch.cuda.Stream()                                     # the counter sees a stream that IS created ...
    assert len(made) == 1 and isinstance(torch.cuda.current_stream(), torch.cuda.Stream) and len(made) == 1     # ... and only those
    del made[:], probe
    for batched in (True, False):
        monkeypatch.setenv('RESEL_GRU_BATCH', '1' if batched else '0')
        alg = _small(algo)
        assert alg.gru_batch == batched and not alg.share_policy_pass
        assert GraphedUpdate.refusal(alg) is None
        for _ in range(2):
            log = dict(alg.train_one_batch())
            alg.grad_num += 1
            assert all(np.isfinite(_val(v)) for v in log.values())
        torch.cuda.synchronize()
        assert made == [], (batched, made)


@pytest.mark.parametrize('algo,per,n_upd', [('td3', 1, 4), ('sac', 2, 4), ('sac', 2, 8), ('td3', 1, 8)])
def test_batched_update_equals_the_serial_form_bit_for_bit(algo, per, n_upd, monkeypatch):
    """Batched eager update (embedding towers in lockstep, `ops.gru_seq_multi`; a prefetched embedding is placed by `cat_into`, the
    critic's differentiated pass included) against the serial form (RESEL_GRU_BATCH=0: one recurrence after another, the last
    fc of the tower writing into the head's row buffer): logs and flat parameters - forward values AND gradients - bit for bit."""
    _need_gpu()
    runs = []
    for batched in (True, False):
        monkeypatch.setenv('RESEL_GRU_BATCH', '1' if batched else '0')
        alg = _small(algo, per, seed=5)
        assert alg.gru_batch == batched
        torch.manual_seed(200)
        np.random.seed(200)
        logs = []
        for _ in range(n_upd):
            logs.append(dict(alg.train_one_batch()))
            alg.grad_num += 1
        torch.cuda.synchronize()
        runs.append((logs, _state(alg)))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert set(a) == set(b)
        for k in b:
            assert _val(a[k]) == _val(b[k]), (k, _val(a[k]), _val(b[k]))
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), runs[0][1], runs[1][1]):
        assert torch.equal(a, b), (nm, (a - b).abs().max().item())


def _graphed_against_eager(algo, per, clip, ragged, batched, monkeypatch):
    """Graphed against eager, batched form, the tolerances of the fp32 families.  (The eager step takes the AdamW bias corrections the
    captured step reads from device words, `ops.adamw_bias_corrections`: with the fp32 `1 - powf(beta, t)` the eager entry point used
    before, the (td3, per 2) row missed rtol 2e-5 in one of 23 544 policy parameters by a factor 1.3 after 8 updates - a deterministic
    actor's near-zero gradients turn a last bit of the step size into a different normalised step.  With the shared spelling the TD3
    rows are bit-equal; SAC keeps the capturable torch AdamW of the entropy coefficient as its one difference.)"""
    _need_gpu()
    from test_host_logic import _push, _synth
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    _quiet(monkeypatch)
    monkeypatch.setenv('RESEL_GRU_BATCH', '1' if batched else '0')
    extra = dict(value_max_gradnorm=0.05, policy_max_gradnorm=0.01) if clip else {}

    n_upd = (16 if ragged else 4) * per
    rs_new = np.random.RandomState(99)
    fresh = [_synth(rs_new, n, 5, 3) for n in (12, 6)]

    def push_fresh(alg):
        for (o, a, r), n in zip(fresh, (12, 6)):
            _push(alg.replay_buffer, o, a, r, early_done=(n != 12))

    eager = _small(algo, per, ragged, **extra)
    logs_e = []
    for i in range(n_upd):
        if i == n_upd - 2:
            push_fresh(eager)
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    graphed = _small(algo, per, ragged, **extra)
    assert eager.gru_batch == batched and graphed.gru_batch == batched
    assert GraphedUpdate.refusal(graphed) is None
    g = GraphedUpdate(graphed, warmup=1, max_graphs=2 if ragged else 4)
    logs_g = []
    for i in range(n_upd):
        if i == n_upd - 2:
            push_fresh(graphed)
        logs_g.append(dict(g.step()))
        graphed.grad_num += 1
    torch.cuda.synchronize()
    print(f'graphs recorded {len(g.graphs)}, eager updates {g.eager_fallbacks} of {n_upd}')
    assert len(g.graphs) >= 1 and g.eager_fallbacks >= 1
    assert ragged or (g.graph is not None and g.eager_fallbacks <= 3 * per)
    if per == 2 and not ragged:
        assert {k[-1] for k in g.graphs} == {True, False}, 'one recording with and one without the actor step'
    rtol, atol = 2e-5, (2e-7 if n_upd <= 16 else 1e-6)
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), _state(graphed), _state(eager)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=rtol, atol=atol, err_msg=nm)
    for le, lg in zip(logs_e, logs_g):
        assert set(le) == set(lg)
        for k in le:
            ve, vg = _val(le[k]), _val(lg[k])
            assert abs(ve - vg) <= rtol * max(1.0, abs(ve)), (k, ve, vg)
    g.close()


@pytest.mark.parametrize('algo,per,clip,ragged', [('sac', 1, False, False), ('td3', 2, False, False), ('sac', 1, True, False), ('sac', 1, False, True)])
def test_graphed_gru_update_equals_the_eager_update(algo, per, clip, ragged, monkeypatch):
    _graphed_against_eager(algo, per, clip, ragged, True, monkeypatch)


def test_graphed_serial_gru_update_equals_the_eager_update(monkeypatch):
    """The serial form (RESEL_GRU_BATCH=0) through `GraphedUpdate`: same tolerances as the batched rows."""
    _graphed_against_eager('sac', 2, False, False, False, monkeypatch)


@pytest.mark.parametrize('per', [1, 2])
def test_two_ranks_graphed_gru_update_reproduces_the_union_batch_update(tmp_path, per, monkeypatch):
    """Two ranks share cuda:0 and exchange through gloo; each drives its (batched) gru updates through the cut graphs."""
    _need_gpu()
    import torch.multiprocessing as mp
    from test_data_parallel import _free_port
    from test_data_parallel_gpu import LENS, _build, _run, _worker
    monkeypatch.setenv('RESEL_GRU_BATCH', '1')                      # inherited by the spawned ranks
    steps = 5 if per == 1 else 8
    mp.spawn(_worker, args=(2, _free_port(), 'gru', str(tmp_path), True, 'gloo', True, steps, per), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f'rank{i}.pt')) for i in range(2))
    for k in ('policy', 'value', 'alpha', 'guard'):
        assert torch.equal(r0[k], r1[k]), f'{k} diverged across ranks'
    one = _build('gru', batch=sum(LENS), quiet=True, patcher=monkeypatch)
    one.parameter.policy_update_per = per
    ref = _run(one, steps)
    for k in ('policy', 'value', 'alpha', 'guard'):
        np.testing.assert_allclose(r0[k].numpy(), ref[k].numpy(), rtol=5e-4, atol=5e-6, err_msg=k)


@pytest.mark.parametrize('rows,horizon', [(64, 1024), (8, 128)])
def test_batched_gru_update_at_size_runs_eagerly_and_replayed(rows, horizon, monkeypatch):
    """The bench's trainer: one eager batched update and the replayed ones behind it are finite and move the parameters; the replayed
    trainer agrees with an eager one built from the same seeds."""
    _need_gpu()
    from bench import build_trainer
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    _quiet(monkeypatch)
    monkeypatch.setenv('RESEL_GRU_BATCH', '1')
    n_upd = 5

    def build():
        torch.manual_seed(0)
        np.random.seed(0)
        alg = build_trainer('gru', rows, horizon)
        assert alg.gru_batch and GraphedUpdate.refusal(alg) is None
        np.random.seed(11)
        return alg

    eager = build()
    before = _state(eager)
    for _ in range(n_upd):
        log = dict(eager.train_one_batch())
        eager.grad_num += 1
        assert all(np.isfinite(_val(v)) for v in log.values())
    graphed = build()
    g = GraphedUpdate(graphed, warmup=1)
    for _ in range(n_upd):
        log = dict(g.step())
        graphed.grad_num += 1
        assert all(np.isfinite(_val(v)) for v in log.values())
    torch.cuda.synchronize()
    print(f'graphs recorded {len(g.graphs)}, eager updates {g.eager_fallbacks} of {n_upd}')
    assert len(g.graphs) >= 1 and g.eager_fallbacks < n_upd
    for nm, a, b, c in zip(('policy', 'value', 'target value', 'log alpha'), _state(graphed), _state(eager), before):
        assert torch.isfinite(a).all() and not torch.equal(a, c), nm
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=2e-7, err_msg=nm)
    g.close()


def test_a_batched_gru_update_issues_no_library_gemm(monkeypatch):
    _need_gpu()
    from test_no_library_gemm_gpu import _library_gemms
    monkeypatch.setenv('RESEL_GRU_BATCH', '1')
    alg = _small('sac', ragged=True)
    assert alg.gru_batch
    alg.train_one_batch()
    alg.grad_num += 1

    def update():
        log = dict(alg.train_one_batch())
        assert all(np.isfinite(_val(v)) for v in log.values())
    assert _library_gemms(update) == []
