"""Whole updates at the published width against an fp64 oracle, and their replayed form against the eager one.

The published architecture (D = 256, efc-8 critic, REDQ m = 2, obs 17, act 6: what bench.py trains) at 64 rows x 128 steps - rows of
130 slots (146 with smamba's conv window), >= 8320 tokens per pass: the smallest count at which the 256-wide outputs, the 128-wide
ones (embedding, input mapping) and the efc-8 batch all reach 2^20 elements and get producer-published magnitude handles, as they do
at 64 x 1024; every fused-epilogue shape rule holds.  Every switch is at its default: GEMM product mode 2, fused critic epilogues
(`gemm_f32_dact`, `gemm_f32_head`), the shared policy pass, the action-only dX, RESEL_GRU_BATCH.

Leg A: one eager `train_one_batch` of the product against `OracleTrainer(dtype=torch.float64)` on the product's initial weights, the
same trajectories, seeds and noise draws, through tests/update_parity.py (bounds and their reasons there): the gradient of every
parameter tensor of actor and critic through AdamW's first moment, the logged scalars of the first update and of a second one (which
consumes the stepped parameters, the soft-updated target, the guard state and the Adam state).  The GEMM census asserts that the fast
paths under test actually ran.
Leg B: four updates through `GraphedUpdate` (one eager, one recorded, two replayed - the form `train()` uses) against four eager ones,
held to the tolerances of tests/test_trainer_gpu.py::test_graphed_update_equals_the_eager_update for the fp32 families.

Measured figures.  The reference's own noise through the same comparison (fp32 oracle vs fp64 oracle, CPU): worst tensor policy / value
3.8e-7 / 5.0e-7 for smamba SAC at 64 x 128 (7 / 8 tensors under the floor: A_log, dt_proj.weight, dt_proj.bias of both blocks and one / two
x_proj.weight), 8.0e-7 / 1.5e-6 for gilr SAC and 4.8e-6 / 1.2e-6 for lru TD3 at 8 x 64; logged scalars at most 0.6 % of their tolerance.
The product's host path on the CPU op backend (tests/oracle_backend.py) against the fp64 oracle at 4 x 24, D = 256: worst tensor 1.1e-6 /
1.5e-6 (smamba), 1.1e-6 / 1.3e-6 (gilr), 9.8e-6 / 1.7e-6 (lru), 8.9e-7 / 8.4e-7 (gru).  The fp64 oracle takes 59 s for the two smamba
updates at 64 x 128 on 8 threads and about 45 GB of host memory (its selective-scan restatement keeps every step's state for autograd);
the other three families take a few seconds.  The figures of the HIP kernels on an MI355X are the MEASURED lines this module prints;
none had been recorded when this docstring was written.
"""
import collections
import time

import numpy as np
import pytest
import torch

import update_parity as UP

pytestmark = pytest.mark.gpu

ROWS, STEPS, OBS, ACT = 64, 128, 17, 6
CONFIGS = [('smamba_s32_c16_b2_nln', 'sac'), ('gilr', 'sac'), ('lru', 'td3'), ('gru', 'sac')]
IDS = ['-'.join(c) for c in CONFIGS]


@pytest.fixture
def cpu_noise(monkeypatch):
    """The product's Gaussian draws come from the CPU generator, like the oracle's (the autouse fixture of test_trainer_gpu.py)."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.utility import rng
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.randn(tuple(shape), dtype=dtype).to(device))


@pytest.fixture
def no_noise(monkeypatch):
    """Actor noise off: a captured generator draws from graph-safe Philox offsets, an eager one does not."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.utility import rng
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.zeros(tuple(shape), dtype=dtype, device=device))


def _census(monkeypatch):
    """Record every GEMM the host path issues (entry, product mode, handles passed) and every magnitude pre-pass."""
    from offpolicy_rnn.hip import ops
    gemms, prepasses = [], []
    run, prepass = ops._gemm_run, ops._prepass

    def gemm_run(fn, name, A, B, args, M, N, K, batch, split, ha, hb, out, *rest, **kw):
        gemms.append((name, split, ha is not None and hb is not None))
        return run(fn, name, A, B, args, M, N, K, batch, split, ha, hb, out, *rest, **kw)

    def counted_prepass(x):
        prepasses.append(tuple(x.shape))
        return prepass(x)
    monkeypatch.setattr(ops, '_gemm_run', gemm_run)
    monkeypatch.setattr(ops, '_prepass', counted_prepass)
    return gemms, prepasses


@pytest.mark.parametrize('rnn,algo', CONFIGS, ids=IDS)
def test_eager_update_against_the_fp64_oracle(rnn, algo, cpu_noise, monkeypatch):
    from bench import build_trainer
    from offpolicy_rnn.hip import ops
    from oracle.trainer import OracleTrainer, default_parameter
    assert ops.gemm_split() == 2
    torch.manual_seed(0)
    np.random.seed(0)
    alg = build_trainer(rnn, ROWS, STEPS, seed=0, algo=algo)
    assert alg.device.type == 'cuda'
    cpu_sd = lambda m: {k: {n: t.detach().cpu().clone() for n, t in d.items()} for k, d in m.state_dict().items()}
    par = default_parameter(rnn=rnn, algo=algo, sac_batch_size=ROWS * STEPS - 1, max_buffer_transition_num=4 * ROWS * STEPS)
    tr = OracleTrainer(par, OBS, ACT, STEPS, policy_state=cpu_sd(alg.policy), value_state=cpu_sd(alg.values[0]), dtype=torch.float64)
    tr.fill_synthetic(2 * ROWS, STEPS, seed=0)

    # the product: two eager updates, the first moments taken between them
    gemms, prepasses = _census(monkeypatch)
    torch.manual_seed(200)
    np.random.seed(200)
    got_logs = [dict(alg.train_one_batch())]
    alg.grad_num += 1
    got = dict(policy=UP.product_moments(alg.policy.store, alg.optimizer_policy),
               value=UP.product_moments(alg.values[0].store, alg.optimizer_value))
    got_logs.append(dict(alg.train_one_batch()))
    torch.cuda.synchronize()

    # the oracle: the same two updates in fp64 on the host
    torch.manual_seed(200)
    np.random.seed(200)
    t0 = time.time()
    ref_logs = [tr.train_one_batch()]
    tr.grad_num += 1
    ref = dict(policy=UP.oracle_moments(tr.policy, tr.opt_policy), value=UP.oracle_moments(tr.value, tr.opt_value))
    ref_logs.append(tr.train_one_batch())
    oracle_s = time.time() - t0
    assert all(t.dtype == torch.float64 for net in ref.values() for t in net.values())

    census = collections.Counter(gemms)
    mode2 = sum(n for (name, split, handles), n in census.items() if split == 2 and handles)
    print(f'MEASURED {rnn} {algo} {ROWS}x{STEPS} GEMM census of two updates (entry, product mode, handles passed): '
          + ', '.join(f'{k}: {n}' for k, n in sorted(census.items())) + f'; mode-2 products {mode2}, pre-passes {len(prepasses)}')
    print(f'MEASURED {rnn} {algo} {ROWS}x{STEPS} fp64 oracle: {oracle_s:.1f} s for two updates on {torch.get_num_threads()} threads')
    rep = UP.compare_update(f'{rnn} {algo} {ROWS}x{STEPS}', got, ref, got_logs, ref_logs)

    assert mode2 >= 40, 'mode 2 did not run'
    assert sum(n for (name, _, _), n in census.items() if name == 'gemm_f32_dact') >= 1, 'the fused ELU-backward epilogue did not run'
    assert sum(n for (name, _, _), n in census.items() if name == 'gemm_f32_head') >= 1, 'the fused critic-head epilogue did not run'
    assert len(prepasses) < mode2, 'every handle came from a pre-pass: no producer or weight store published one'
    assert got_logs[0]['real_batch_size'] == ROWS * STEPS and got_logs[0]['real_batch_traj_num'] == ROWS
    assert not rep['failures'], rep['failures']


@pytest.mark.parametrize('rnn,algo', CONFIGS, ids=IDS)
def test_replayed_update_equals_the_eager_update(rnn, algo, no_noise):
    from bench import build_trainer
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    n_upd = 4

    def build():
        torch.manual_seed(0)
        np.random.seed(0)
        alg = build_trainer(rnn, ROWS, STEPS, seed=0, algo=algo)
        np.random.seed(11)
        return alg

    def state(alg):
        return [alg.policy.store.flat.detach().clone(), alg.values[0].store.flat.detach().clone(),
                alg.target_values[0].store.flat.detach().clone(), alg.log_sac_alpha.detach().clone()]

    eager = build()
    why = GraphedUpdate.refusal(eager)
    if why:
        pytest.skip(why)
    logs_e = []
    for _ in range(n_upd):
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    graphed = build()
    gu = GraphedUpdate(graphed, warmup=1)
    try:
        logs_g = []
        for _ in range(n_upd):
            logs_g.append(dict(gu.step()))
            graphed.grad_num += 1
        torch.cuda.synchronize()
        rtol, atol = 2e-5, 2e-7                                  # test_graphed_update_equals_the_eager_update, fp32 families, <= 16 updates
        names = ('policy', 'value', 'target value', 'log alpha')
        pairs = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(state(graphed), state(eager))]
        val = lambda v: v[0] if isinstance(v, tuple) else v
        log_err = max(abs(val(le[k]) - val(lg[k])) / max(1.0, abs(val(le[k]))) for le, lg in zip(logs_e, logs_g) for k in le)
        print(f'MEASURED {rnn} {algo} {ROWS}x{STEPS} replayed vs eager after {n_upd} updates: graphs {len(gu.graphs)}, eager updates {gu.eager_fallbacks}; '
              + ', '.join(f'{nm} max (|a - b| - {rtol:g} |b|) = {(np.abs(a - b) - rtol * np.abs(b)).max():.3e}' for nm, (a, b) in zip(names, pairs))
              + f' (atol {atol:g}); logged scalars max |a - b| / max(1, |b|) = {log_err:.3e} (bound {rtol:g})')
        assert len(gu.graphs) == 1
        for nm, (a, b) in zip(names, pairs):
            np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=nm)
        for le, lg in zip(logs_e, logs_g):
            assert set(le) == set(lg)
            for k in le:
                assert abs(val(le[k]) - val(lg[k])) <= rtol * max(1.0, abs(val(le[k]))), (k, le[k], lg[k])
    finally:
        gu.close()
