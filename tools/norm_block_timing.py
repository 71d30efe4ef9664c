"""Time one update of the README trainer's shape with normalised dense stacks, and the two norm kernels against the memory roof.

    python tools/norm_block_timing.py [--rows 64] [--horizon 1024] [--replays 12] [--kernels] [--tree DIR] [--label TEXT]

The trainer is bench.py's (`smamba_s32_c16_b2_nln`, D = 256, `efc-8` critic) with `eln-8+elu` on the critic's two hidden layers and `ln+elu` on
the policy's, `redq_m` = 8 (a coupled norm evaluates every critic anyway; the parent commit cannot take a subset through an `eln` layer at
all).  The update is stepped through `GraphedUpdate` until a step is replayed whole; then `--replays` replays are timed one by one (host
clock, a device synchronise on either side) and their median is the figure.  One process = one leg:

    the new path                     python tools/norm_block_timing.py
    switched off                     RESEL_NORM_FUSED=0 python tools/norm_block_timing.py
    another checkout (the parent)    python tools/norm_block_timing.py --tree DIR     (DIR/bench.py, DIR/recurrent-offpolicy-rl_amd, built)

Run the legs in alternation, more than once (profiles/r26_norm_blocks.md).  `--kernels` adds the forward and backward kernels on their
own at the update's shapes - the critic's [8, rows x horizon, 256] in both layouts and the policy's [rows x horizon, 256] - under
device events, median of 20 calls behind 5, against bytes moved / 8 TB/s: the forward reads x and writes y, the backward reads dy and x
and writes dx (weights, statistics and the gradient partials are below 1 % of that).  Prints one JSON line.  No GPU: an error."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=64)
ap.add_argument('--horizon', type=int, default=1024)
ap.add_argument('--replays', type=int, default=12)
ap.add_argument('--kernels', action='store_true')
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--label', default='')
args = ap.parse_args()
assert args.replays >= 10, 'the figure is a median of at least 10 replays'
ROOT = os.path.abspath(args.tree)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]

import numpy as np
import torch
if not torch.cuda.is_available():
    sys.exit('norm_block_timing: needs a GPU')
import bench
from offpolicy_rnn import alg_init
from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
from offpolicy_rnn.hip import ops

HBM = 8.0e12                                            # bytes / s


def time_update():
    torch.manual_seed(1234)
    np.random.seed(1234)
    par = bench.make_parameter('smamba_s32_c16_b2_nln', args.rows, args.horizon)
    par.value_activations = ['eln-8+elu', 'eln-8+elu', 'linear']
    par.policy_activations = ['ln+elu', 'ln+elu', 'linear']
    par.redq_m = 8
    alg = alg_init(par)
    alg.defer_log = True
    bench.fill_synthetic(alg, 2 * args.rows, args.horizon, 0)
    why = GraphedUpdate.refusal(alg)
    if why is not None:
        sys.exit(f'norm_block_timing: GraphedUpdate refuses the trainer: {why}')
    gu = GraphedUpdate(alg, warmup=1)

    def step():
        torch.cuda.synchronize()
        t = time.perf_counter()
        gu.step()
        torch.cuda.synchronize()
        alg.grad_num += 1
        return 1e3 * (time.perf_counter() - t)

    warm = 0
    while True:                                         # until a step is replayed whole
        before = gu.eager_fallbacks
        step()
        warm += 1
        if gu.eager_fallbacks == before:
            break
        if warm >= 12:
            sys.exit(f'norm_block_timing: still {gu.eager_fallbacks} eager passes after {warm} warm-up steps')
    step()
    before = gu.eager_fallbacks
    ms = [step() for _ in range(args.replays)]
    eager = gu.eager_fallbacks - before
    gu.close()
    return dict(ms_per_update=[round(v, 3) for v in ms], ms_per_update_median=round(statistics.median(ms), 3), ms_per_update_min=round(min(ms), 3),
                warm_steps=warm, eager_passes_in_timed_steps=eager)


def _events(fn, n=20, warm=5):
    for _ in range(warm):
        fn()
    us = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        us.append(1e3 * a.elapsed_time(b))
    return statistics.median(us)


def time_kernels():
    M, C = args.rows * args.horizon, 256
    out = []
    g = torch.Generator(device='cuda').manual_seed(0)
    for name, E, layout in (('critic eln-8, token-major [M, 8 x 256]', 8, 'token'), ('critic eln-8, member-major [8, M, 256]', 8, 'member'),
                            ('policy ln [M, 256]', 1, 'member')):
        def operand():
            if layout == 'token':
                return torch.randn(M, E, C, device='cuda', generator=g).transpose(0, 1)
            return torch.randn((E, M, C) if E > 1 else (M, C), device='cuda', generator=g)
        x, dy = operand().requires_grad_(True), operand()
        w = (1.0 + 0.1 * torch.randn((E, C) if E > 1 else (C,), device='cuda', generator=g)).requires_grad_(True)
        b = (0.1 * torch.randn((E, C) if E > 1 else (C,), device='cuda', generator=g)).requires_grad_(True)
        nbytes = 4 * M * E * C
        with torch.no_grad():
            fwd = _events(lambda: ops.member_layer_norm(x, w, b, 1e-5, 'elu'))
        y = ops.member_layer_norm(x, w, b, 1e-5, 'elu')
        bwd = _events(lambda: torch.autograd.grad(y, (x, w, b), dy, retain_graph=True))
        out.append(dict(shape=name, tensor_mb=round(nbytes / 1e6, 1),
                        fwd_us=round(fwd, 1), fwd_roof_us=round(2e6 * nbytes / HBM, 1), fwd_of_roof=round(2e6 * nbytes / HBM / fwd, 3),
                        bwd_us=round(bwd, 1), bwd_roof_us=round(3e6 * nbytes / HBM, 1), bwd_of_roof=round(3e6 * nbytes / HBM / bwd, 3)))
    return out


has_kernels = hasattr(ops, 'member_layer_norm')
fused = has_kernels and ops.norm_fused_on()
out = dict(label=args.label, tree=os.path.basename(ROOT), rows=args.rows, horizon=args.horizon,
           norm_path='hip' if fused else 'torch', RESEL_NORM_FUSED=os.environ.get('RESEL_NORM_FUSED'))
out.update(time_update())
if args.kernels:
    if not has_kernels:
        sys.exit('norm_block_timing: --kernels needs a checkout that has the norm kernels')
    out['kernels'] = time_kernels()                     # (the backward figure includes the two column-sum launches of dw / db)
print(json.dumps(out), flush=True)
