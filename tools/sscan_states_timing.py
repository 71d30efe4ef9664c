"""Times the selective scan and one whole update per d_state at the README shape: 64 rows of 1043 steps, d_inner 512.

    python tools/sscan_states_timing.py [--sizes 24,32,48,64,100,128,256] [--runs 10] [--warmup 3] [--no-update]

Scan: the calls of `MambaInnerFn` (code 6, z and D given, B / C as column blocks of x_dbl, checkpoints, magnitude handles) through
`ops._plan_fwd` / `_plan_bwd`, i.e. padded sizes on their native kernel and grouped sizes as their groups plus the gate, gate-backward and
reduce passes.  Forward and backward are stream-event intervals around the whole call (all groups and passes, launch gaps included), one
sample per run; printed: the median with the minimum and maximum, then the per-dispatch kernel times of the last run from the library's
profiling events (`ops.profile_enable`).  Update: `train_one_batch()` of the README trainer with `smamba_s<N>_c16_b2_nln` (bench.py's
`build_trainer(rnn, 64, 1043)`), launched eagerly, wall time between synchronisations, median of --update-runs after two warm-up updates.
One process, one device; for run-to-run spread start the tool again.  On a tree without the state plan (a parent commit) only native
sizes run: pass --sizes 32,64."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
import torch                                                   # noqa: E402
from offpolicy_rnn.hip import ops                              # noqa: E402

ROWS, STEPS, DI, R = 64, 1043, 512, 16


def med(xs):
    return f'{statistics.median(xs):8.1f} us [{min(xs):8.1f} .. {max(xs):8.1f}]'


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3, out


def scan_calls(N):
    """-> (forward(), backward(saved)) closures over one set of operands in the mixer's layout."""
    dev = torch.device('cuda')
    gen = torch.Generator(device='cuda').manual_seed(N)
    M = ROWS * STEPS
    planned = hasattr(ops, 'sscan_state_plan')
    plan = ops.sscan_state_plan(N) if planned else [(0, N, N)]
    Np = plan[-1][0] + plan[-1][2]
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
    xz, dout = rnd(M, 2 * DI), rnd(M, DI)
    x_dbl = rnd(M, R + 2 * Np)
    if Np != N:                                                # what x_proj's zero-padded weight rows give
        x_dbl[:, R + N:R + Np] = 0
        x_dbl[:, R + Np + N:] = 0
    dt = torch.nn.functional.softplus(0.5 * rnd(M, DI) + (0.5 * rnd(DI) - 2))
    A_log = torch.log(torch.arange(1, N + 1, dtype=torch.float32, device=dev)).repeat(DI, 1).contiguous()
    D = torch.ones(DI, device=dev)
    start = torch.zeros(ROWS, STEPS, device=dev)
    start[:, 0] = 1
    startf = start.reshape(-1).contiguous()
    u, z, Bm, Cm = xz[:, :DI], xz[:, DI:], x_dbl[:, R:R + Np], x_dbl[:, R + Np:]
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    y, dxz, dx_dbl, du, ddt, dD, dbias = new(M, DI), new(M, 2 * DI), new(M, R + 2 * Np), new(M, DI), new(M, DI), new(DI), new(DI)
    _, p_y, e_y = ops._slot_args(True, dev)
    _, p_dxz, e_b = ops._slot_args(True, dev)
    _, p_ddt, _ = ops._slot_args(True, dev)
    if planned:
        A_g = ops._group_A(A_log, plan)

        def forward():
            return ops._plan_fwd(plan, A_g, ROWS, STEPS, u, dt, z, Bm, Cm, D, None, startf, y, True, False, 6, p_y, e_y)

        def backward(saved):
            cks, parts, _ = saved
            ops._plan_bwd(plan, A_g, ROWS, STEPS, u, dt, z, Bm, Cm, D, None, startf, dout, cks, parts, du, ddt, dxz[:, DI:], dx_dbl[:, R:R + Np],
                          dx_dbl[:, R + Np:], dD, dbias, 6, p_dxz, p_ddt, e_b)
    else:
        dA = new(DI, N)

        def forward():
            ck = ops._ws(ops.lib().resel_selective_scan_ckpt_bytes(ROWS, STEPS, DI, N), dev)
            ops._sscan_fwd(ROWS, STEPS, u, dt, z, A_log, Bm, Cm, D, None, startf, y, ck, None, 6, p_y, e_y)
            return ck

        def backward(ck):
            ops._sscan_bwd(ROWS, STEPS, u, dt, z, A_log, Bm, Cm, D, None, startf, dout, ck, du, ddt, dxz[:, DI:], dx_dbl[:, R:R + N], dx_dbl[:, R + N:],
                           dA, dD, dbias, 6, p_dxz, p_ddt, e_b)
    return plan, forward, backward


def time_scan(N, runs, warmup):
    plan, forward, backward = scan_calls(N)
    fwd, bwd = [], []
    for run in range(warmup + runs):
        t1, saved = event_us(forward)
        t2, _ = event_us(lambda: backward(saved))
        if run >= warmup:
            fwd.append(t1)
            bwd.append(t2)
    ops.profile_enable(True)
    ops.profile_collect()
    backward(forward())
    torch.cuda.synchronize()
    prof = ops.profile_collect()
    ops.profile_enable(False)
    print(f'd_state {N}: kernels at {[k for _, _, k in plan]}, {ROWS} x {STEPS} x {DI}, median of {runs} runs [min .. max]:')
    print(f'  scan forward  {med(fwd)}')
    print(f'  scan backward {med(bwd)}')
    print('  per dispatch: ' + ', '.join(f'{name[:-7]} {n} x {us:.1f} us' for name, (n, us) in prof.items()))
    sys.stdout.flush()


def time_update(N, runs):
    import bench
    alg = bench.build_trainer(f'smamba_s{N}_c16_b2_nln', ROWS, STEPS)
    ms = []
    for run in range(2 + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        alg.train_one_batch()
        torch.cuda.synchronize()
        if run >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
        alg.grad_num += 1
    print(f'd_state {N}: one eager update of smamba_s{N}_c16_b2_nln at {ROWS} x {STEPS}: median {statistics.median(ms):7.1f} ms '
          f'[{min(ms):7.1f} .. {max(ms):7.1f}] over {runs}')
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='24,32,48,64,100,128,256')
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--update-runs', type=int, default=5)
    ap.add_argument('--no-update', action='store_true')
    args = ap.parse_args()
    sizes = [int(v) for v in args.sizes.split(',')]
    for N in sizes:
        time_scan(N, args.runs, args.warmup)
        torch.cuda.empty_cache()
    if not args.no_update:
        for N in sizes:
            time_update(N, args.update_runs)
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
