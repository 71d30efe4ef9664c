"""world_size-2 data parallelism on CPU (`gloo`): the flat-gradient all-reduce with the piggy-backed valid count, the shared
REDQ subset stream and the global Q-guard.

(a) ranks that hold DIFFERENT rows end every update with identical parameters;
(b) two ranks that hold the SAME rows reproduce the single-process update (sum of two equal gradients over twice the
    count = the single-process mean gradient), which pins the global `/ valid_num` normalisation;
(c) two ranks that hold DISJOINT trajectory sets and each train on all of theirs reproduce the single-process update over the
    UNION batch (actor noise switched off so that a trajectory sees the same draws wherever it is trained): this pins the
    semantics SURVEY.md 8(e) asks for - same critics in the REDQ minimum on every rank, Q-guard extrema of the global batch,
    global normalisation.
Kernels are the CPU oracle stand-ins (tests/oracle_backend.py); RCCL itself is exercised by the driver's multi-GPU bench."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))


class _Patch:
    def setattr(self, obj, name, val):
        setattr(obj, name, val)


LENS = (12, 5, 7, 12, 9)


def _build(seed_data, same_noise_seed, patcher=None, keep=None, batch=30, quiet=False, lens=LENS):
    """keep: indices of `lens` this process holds (None = all); quiet: actor noise off."""
    sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'recurrent-offpolicy-rl_amd')]
    import oracle_backend
    patcher = patcher or _Patch()
    oracle_backend.install(patcher)                  # worker processes patch for good; the pytest process uses monkeypatch
    from test_host_logic import _push, _synth, make_parameter
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.utility import rng
    if quiet:
        patcher.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.zeros(tuple(shape), dtype=dtype, device=device))
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter('gilr', sac_batch_size=batch))
    rs = np.random.RandomState(seed_data)
    for i, n in enumerate(lens):
        o, a, r = _synth(rs, n, 5, 3)
        if keep is None or i in keep:
            _push(alg.replay_buffer, o, a, r, early_done=(n != 12))
    torch.manual_seed(same_noise_seed)
    np.random.seed(same_noise_seed)
    alg._subset_rng = np.random.RandomState(int(alg.parameter.seed) + 7919)     # the stream the data-parallel ranks share
    return alg


SPLIT = ((0, 2, 4), (1, 3))                        # disjoint trajectory sets of the two ranks in mode 'union'
LENS_WIDE = (12, 5, 7, 12, 9, 4, 12, 6, 11, 3, 8)  # mode 'wide': dealt round-robin to 3, 4 or 8 ranks (at 8, five ranks hold ONE trajectory)
UPDATES_WIDE = 3                                   # the guard acts on the NEXT target: two updates would exercise one clamp only


def _worker(rank, world, port, mode, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    if mode == 'union':                            # every rank trains on ALL of its own trajectories (batch = its transition count)
        alg = _build(3, 11, keep=SPLIT[rank], batch=sum(LENS[i] for i in SPLIT[rank]), quiet=True)
        alg._subset_rng = None                     # product default under world > 1: the shared stream
    elif mode == 'wide':                           # 'union' over more ranks than two
        keep = tuple(range(rank, len(LENS_WIDE), world))
        alg = _build(3, 11, keep=keep, batch=sum(LENS_WIDE[i] for i in keep), quiet=True, lens=LENS_WIDE)
        alg._subset_rng = None
    else:
        same_data = mode == 'same'
        alg = _build(seed_data=3 if same_data else 3 + rank, same_noise_seed=11 if same_data else 11 + rank)
        alg._subset_rng = None
    alg.grad_sync.__init__()
    assert alg.grad_sync.world == world
    for _ in range(UPDATES_WIDE if mode == 'wide' else 2):
        log = alg.train_one_batch()
        alg.grad_num += 1
    torch.save(dict(policy=alg.policy.store.flat.clone(), value=alg.values[0].store.flat.clone(), guard=alg.Q_guard.state.detach().clone(),
                    alpha=alg.log_sac_alpha.detach().clone(), critic_loss=log['critic_loss'], calls=dict(alg.grad_sync.calls)),
               os.path.join(out_dir, f'rank{rank}.pt'))
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize('mode,guard', [('different', 'bucket'), ('same', 'bucket'), ('union', 'bucket'), ('union', 'allreduce')])
def test_two_rank_update(tmp_path, mode, guard, monkeypatch):
    """guard = bucket (default): one collective per optimizer step, the ranks' Q-guard extrema ride in the critic's gradient bucket
    (4 floats per rank in a zero-filled tail); allreduce: two MAX all-reduces inside the target.  Either way the parameters AND the
    guard state equal the single-process update over the union batch."""
    monkeypatch.setenv('RESEL_DP_GUARD', guard)
    mp.spawn(_worker, args=(2, _free_port(), mode, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f'rank{i}.pt')) for i in range(2))
    assert r0['calls']['all_reduce_sum'] == 4 and r0['calls']['all_reduce_max'] == (0 if guard == 'bucket' else 4), r0['calls']
    for k in ('policy', 'value', 'alpha', 'guard'):
        assert torch.equal(r0[k], r1[k]), f'{k} diverged across ranks'
    if mode != 'different':
        sys.path[:0] = [HERE]
        if mode == 'same':                         # single process, same rows, same noise
            alg = _build(seed_data=3, same_noise_seed=11, patcher=monkeypatch)
        else:                                      # single process over the union of the two ranks' trajectories
            alg = _build(3, 11, patcher=monkeypatch, batch=sum(LENS), quiet=True)
        for _ in range(2):
            alg.train_one_batch()
            alg.grad_num += 1
        n = alg.policy.store.numel
        np.testing.assert_allclose(r0['policy'][:n], alg.policy.store.flat[:n], rtol=1e-5, atol=1e-7)
        n = alg.values[0].store.numel
        np.testing.assert_allclose(r0['value'][:n], alg.values[0].store.flat[:n], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(r0['alpha'], alg.log_sac_alpha.detach(), rtol=1e-6)
        np.testing.assert_allclose(r0['guard'], alg.Q_guard.state.detach(), rtol=1e-6)


@pytest.mark.parametrize('guard', ['bucket', 'allreduce'])
@pytest.mark.parametrize('world', [3, 4, 8])
def test_many_rank_union_update(tmp_path, world, guard, monkeypatch):
    """`test_two_rank_update`'s union mode at world sizes above 2: 11 trajectories dealt round-robin, three updates.  All ranks end
    bitwise equal and rank 0 equals the single process over the union batch - which exercises rows 1.. of the `4 + 4 * rank` guard
    slots in the critic's gradient bucket (bucket form) and the MAX all-reduces over more than two contributions."""
    monkeypatch.setenv('RESEL_DP_GUARD', guard)
    mp.spawn(_worker, args=(world, _free_port(), 'wide', str(tmp_path)), nprocs=world, join=True)
    ranks = [torch.load(os.path.join(tmp_path, f'rank{i}.pt')) for i in range(world)]
    r0 = ranks[0]
    assert r0['calls']['all_reduce_sum'] == 2 * UPDATES_WIDE, r0['calls']
    assert r0['calls']['all_reduce_max'] == (0 if guard == 'bucket' else 2 * UPDATES_WIDE), r0['calls']
    for i, r in enumerate(ranks[1:], 1):
        for k in ('policy', 'value', 'alpha', 'guard'):
            assert torch.equal(r0[k], r[k]), f'{k} of rank {i} diverged from rank 0'
    sys.path[:0] = [HERE]
    alg = _build(3, 11, patcher=monkeypatch, batch=sum(LENS_WIDE), quiet=True, lens=LENS_WIDE)
    for _ in range(UPDATES_WIDE):
        alg.train_one_batch()
        alg.grad_num += 1
    n = alg.policy.store.numel
    np.testing.assert_allclose(r0['policy'][:n], alg.policy.store.flat[:n], rtol=1e-5, atol=1e-7)
    n = alg.values[0].store.numel
    np.testing.assert_allclose(r0['value'][:n], alg.values[0].store.flat[:n], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(r0['alpha'], alg.log_sac_alpha.detach(), rtol=1e-6)
    np.testing.assert_allclose(r0['guard'], alg.Q_guard.state.detach(), rtol=1e-6)


@pytest.mark.parametrize('sac', [True, False])
@pytest.mark.parametrize('world', [2, 8])
def test_oracle_standins_agree_across_virtual_ranks(world, sac):
    """The CPU stand-ins of the target (tests/oracle_backend.py) obey the equivalence the GPU tests hold the kernels to with their
    help: `world` virtual ranks over unequal contiguous shards of one batch - local form + slot block + `guard_apply_slots`, and
    the `reduce_max` form - reproduce the single-process stand-in over the union: targets and guard at rtol 1e-6, guards bitwise
    equal across ranks, counts and maxima add / max up exactly.  Three updates, later batches wider so that the guard clamps."""
    sys.path[:0] = [HERE]
    import oracle_backend as OB
    g = torch.Generator().manual_seed(world + 2 * sac)
    M, E, m, gamma = 300, 8, 2, 0.99
    edges = [0, 1] + [1 + (M - 1) * (i * (i + 3)) // (world * (world + 3) - 4) for i in range(2, world)] + [M] if world > 2 else [0, 1, M]
    assert edges == sorted(set(edges)) and len(edges) == world + 1
    reward, done = torch.randn(M, generator=g), (torch.rand(M, generator=g) < 0.05).float()
    mask = (torch.rand(M, generator=g) < 0.8).float()
    la = torch.tensor([-0.3])
    new_guard = lambda: torch.tensor([1000000.0, -1000000.0, 0.0, 0.999])
    g_one, g_bkt, g_max = new_guard(), [new_guard() for _ in range(world)], [new_guard() for _ in range(world)]
    clamped = []
    for it, width in enumerate((1.0, 3.0, 4.0)):
        q = torch.randn(E, M, generator=g) * 3.0 * width
        nl = torch.randn(M, generator=g) * width if sac else None
        subset = torch.randperm(E, generator=g)[:m].int()
        v = q[subset.long()].min(dim=0).values - (la.exp() * nl if sac else 0.0)
        if it:
            clamped.append(((v < g_one[0]) | (v > g_one[1])).float().mean().item())
        s_one = torch.zeros(2)
        y_one = OB.sac_target(q, subset, nl, la, reward, done, mask, gamma, g_one, s_one)
        cut = lambda t, a, b: None if t is None else t[..., a:b]
        parts = [(q[:, a:b], subset, cut(nl, a, b), la, cut(reward, a, b), cut(done, a, b), cut(mask, a, b), gamma) for a, b in zip(edges[:-1], edges[1:])]
        # local form: every rank fills its own row of a zero [world, 4] block; the SUM all-reduce delivers all rows everywhere
        exts, s_b = [torch.zeros(4) for _ in parts], [torch.zeros(2) for _ in parts]
        y_b = [OB.sac_target(*parts[r], g_bkt[r], s_b[r], local_ext=exts[r]) for r in range(world)]
        blocks = torch.zeros(world, world, 4)
        for r in range(world):
            blocks[r, r] = exts[r]
        slots = blocks.sum(dim=0).reshape(-1)
        for r in range(world):
            OB.guard_apply_slots(slots, world, g_bkt[r])

        # reduce_max form: the ranks run one after the other here, so the two exchanges are resolved in three passes over copies
        # of the guards - pass k knows the global maxima of the first k exchanges and records every rank's next contribution
        def run_pass(known):
            seen, ys, guards, sts = [[] for _ in parts], [], [gr.clone() for gr in g_max], [torch.zeros(2) for _ in parts]
            for r in range(world):
                def reduce_max(t, r=r):
                    seen[r].append(t.clone())
                    if len(seen[r]) <= len(known):
                        t.copy_(known[len(seen[r]) - 1])
                ys.append(OB.sac_target(*parts[r], guards[r], sts[r], reduce_max=reduce_max))
            return seen, ys, guards, sts
        first = torch.stack([s[0] for s in run_pass([])[0]]).max(dim=0).values
        second = torch.stack([s[1] for s in run_pass([first])[0]]).max(dim=0).values
        _, y_m, g_max, s_m = run_pass([first, second])
        for nm, ys, gs, sts in (('local + slots', y_b, g_bkt, s_b), ('reduce_max', y_m, g_max, s_m)):
            np.testing.assert_allclose(torch.cat(ys), y_one, rtol=1e-6, atol=0, err_msg=f'{nm}: targets, update {it}')
            np.testing.assert_allclose(gs[0], g_one, rtol=1e-6, err_msg=f'{nm}: guard, update {it}')
            assert all(torch.equal(x, gs[0]) for x in gs), f'{nm}: guards differ across ranks'
            assert sum(s[1].item() for s in sts) == s_one[1].item() and max(s[0].item() for s in sts) == s_one[0].item()
    assert all(0.01 <= c <= 0.5 for c in clamped), clamped


# ---- the launcher: `python bench.py --gpus N` starts its own ranks; the torchrun form keeps working (no GPU needed: --spawn-dry-run) ----

ROOT = os.path.dirname(HERE)


def _bench(args, env=None, launcher=()):
    import json
    import subprocess
    cmd = [sys.executable, *launcher, os.path.join(ROOT, 'bench.py'), *args]
    e = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT')}
    e.update(env or {})
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=e)
    js = [l for l in r.stdout.splitlines() if l.startswith('{')]
    return r, (json.loads(js[-1]) if js else None)


def test_bench_starts_its_own_ranks_and_splits_a_global_batch():
    r, line = _bench(['--gpus', '2', '--global-rows', '128', '--steps', '7', '--warmup', '2', '--spawn-dry-run'])
    assert r.returncode == 0, r.stderr[-2000:]
    assert line['n_gpus'] == 2 and line['rows_per_rank'] == 64 and line['global_rows'] == 128 and line['scaling'] == 'strong'
    assert line['local_rank_sum'] == 1 and line['rccl_ranks'] == 2 and line['collectives']['all_reduce_sum'] == 1
    assert line['steps'] == 7 and line['warmup'] == 2 and 'spawned its own ranks' in line['launcher']
    assert len([l for l in r.stdout.splitlines() if l.startswith('{')]) == 1          # ONE JSON line on stdout


def test_bench_weak_scaling_rows_per_rank_under_the_launcher():
    r, line = _bench(['--gpus', '4', '--spawn-dry-run'])
    assert r.returncode == 0, r.stderr[-2000:]
    assert line['n_gpus'] == 4 and line['rows_per_rank'] == 64 and line['global_rows'] == 256 and line['scaling'] == 'weak'
    assert line['local_rank_sum'] == 0 + 1 + 2 + 3


def test_bench_exits_non_zero_when_a_rank_fails():
    import time
    t0 = time.time()
    r, line = _bench(['--gpus', '2', '--spawn-dry-run'], env={'RESEL_BENCH_DRY_FAIL_RANK': '1'})
    assert r.returncode != 0 and line is None and 'rank 1 failed' in r.stderr
    assert time.time() - t0 < 120                    # the surviving rank (blocked in the rendezvous) was taken down, not waited for
    r, line = _bench(['--gpus', '3', '--global-rows', '128', '--spawn-dry-run'])
    assert r.returncode != 0 and line is None and 'does not split' in r.stderr


def test_bench_under_torchrun_keeps_working():
    r, line = _bench(['--gpus', '2', '--global-rows', '32', '--spawn-dry-run'],
                     launcher=('-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                               '--master-port', str(_free_port())))
    assert r.returncode == 0, r.stderr[-2000:]
    assert line['n_gpus'] == 2 and line['rows_per_rank'] == 16 and 'launcher' not in line


def test_one_rank_group_issues_and_counts_collectives(monkeypatch):
    """RESEL_DP_FORCE_COLLECTIVES=1: init_from_env creates a ONE-rank group and GradSync issues (and counts) every collective in it."""
    from offpolicy_rnn.parallel.data_parallel import GradSync, init_from_env
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT'):
        monkeypatch.delenv(k, raising=False)
    assert not GradSync().active
    monkeypatch.setenv('RESEL_DP_FORCE_COLLECTIVES', '1')
    assert init_from_env(backend='gloo') == (0, 1, 0) and dist.is_initialized()
    try:
        gs = GradSync()
        assert gs.active and gs.world == 1 and gs.backend == 'gloo'
        t = torch.arange(6.0)
        gs.all_reduce_async_(t)
        gs.wait()
        gs.all_reduce_max_(t[:2])
        gs.broadcast_(t)
        assert torch.equal(t, torch.arange(6.0))
        assert gs.calls == dict(all_reduce_sum=1, all_reduce_max=1, broadcast=1) and gs.bytes['all_reduce_sum'] == 24
        gs.reset_counters()
        assert sum(gs.calls.values()) == 0
    finally:
        dist.destroy_process_group()
