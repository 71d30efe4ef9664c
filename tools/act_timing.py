"""Time one update of the README trainer's shape with relu (or tanh, ...) on every dense layer: the activations in the GEMM epilogues
against the torch modules.

    python tools/act_timing.py [--act relu] [--rows 64] [--horizon 1024] [--replays 12] [--tree DIR] [--label TEXT]

The trainer is bench.py's (`smamba_s32_c16_b2_nln`, D = 256, `efc-8` critic, 64 x 1024) with `--act` in place of every `elu` of the
embedding stacks and the heads of both networks.  The update is stepped through `GraphedUpdate` until a step is replayed whole; then
`--replays` replays are timed one by one (host clock, a device synchronise on either side) and their median is the figure.  One process
= one leg:

    fused (the default)              python tools/act_timing.py --act relu
    the torch modules                RESEL_ACT_FUSED=0 python tools/act_timing.py --act relu
    another checkout (the parent)    python tools/act_timing.py --act relu --tree DIR     (DIR/bench.py, DIR/recurrent-offpolicy-rl_amd, built)

Run the legs in alternation, at least three times each, on one box (profiles/r30_dense_activations.md: boxes differ by ~8 %).  Prints one
JSON line.  No GPU: an error."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--act', default='relu', choices=['relu', 'leaky_relu', 'tanh', 'sigmoid', 'elu'])
ap.add_argument('--rows', type=int, default=64)
ap.add_argument('--horizon', type=int, default=1024)
ap.add_argument('--replays', type=int, default=12)
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--label', default='')
args = ap.parse_args()
assert args.replays >= 10, 'the figure is a median of at least 10 replays'
ROOT = os.path.abspath(args.tree)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]

import numpy as np
import torch
if not torch.cuda.is_available():
    sys.exit('act_timing: needs a GPU')
import bench
from offpolicy_rnn import alg_init
from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
from offpolicy_rnn.hip import ops


def time_update():
    torch.manual_seed(1234)
    np.random.seed(1234)
    par = bench.make_parameter('smamba_s32_c16_b2_nln', args.rows, args.horizon)
    for w in ('value', 'policy'):
        setattr(par, f'{w}_embedding_activations', [args.act, args.act, 'linear'])
        setattr(par, f'{w}_activations', [args.act, args.act, 'linear'])
    alg = alg_init(par)
    alg.defer_log = True
    bench.fill_synthetic(alg, 2 * args.rows, args.horizon, 0)
    why = GraphedUpdate.refusal(alg)
    if why is not None:
        sys.exit(f'act_timing: GraphedUpdate refuses the trainer: {why}')
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
            sys.exit(f'act_timing: still {gu.eager_fallbacks} eager passes after {warm} warm-up steps')
    step()
    before = gu.eager_fallbacks
    ms = [step() for _ in range(args.replays)]
    eager = gu.eager_fallbacks - before
    gu.close()
    return dict(ms_per_update=[round(v, 3) for v in ms], ms_per_update_median=round(statistics.median(ms), 3), ms_per_update_min=round(min(ms), 3),
                warm_steps=warm, eager_passes_in_timed_steps=eager)


has_codes = 'relu' in ops.ACT_IDS                       # (a checkout from before the codes: the torch modules, whatever the switch says)
fused = args.act == 'elu' or (has_codes and ops.act_fused_on())
out = dict(label=args.label, tree=os.path.basename(ROOT), act=args.act, rows=args.rows, horizon=args.horizon,
           act_path='hip' if fused else 'torch', RESEL_ACT_FUSED=os.environ.get('RESEL_ACT_FUSED'))
out.update(time_update())
print(json.dumps(out), flush=True)
