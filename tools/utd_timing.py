"""Time one `train_one_batch()` at an update-to-data ratio above one in its two launch forms: `GraphedUpdate.step()` - `utd` passes, each
replayed from the graph of its own launch sequence - against the eager `train_one_batch()`.  One trainer on a synthetic fixed-length
ring (bench.py's), both forms in the same process, in alternating windows.

    python tools/utd_timing.py --rnn gru --algo sac --rows 8 --horizon 128 --utd 4 [--policy-utd 1] [--policy-update-per 1]
                               [--n 20] [--repeats 3] [--root TREE]

A window is `--n` steps under a host clock and ends in a device synchronise; the logs are deferred (`defer_log`, as bench.py), so
neither form waits for the step it has just launched.  Before the first window every launch sequence the windows use is warmed: steps
are taken until a whole period of `policy_update_per` steps has run without an eager pass.  `--root TREE` measures another checkout of
this project (its own package and library) from this one script - run the two builds in alternation, one process each
(profiles/r17_utd_replay.md).  Where `GraphedUpdate.refusal` refuses the trainer (a checkout from before utd replay, at utd > 1) only
the eager form is timed.  Prints one JSON line: per form the ms per step and per pass of every window and their median, the graphs
held and the passes launched eagerly inside the replayed windows.  No GPU: an error."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--rnn', default='gru')
ap.add_argument('--algo', default='sac')
ap.add_argument('--rows', type=int, default=8)
ap.add_argument('--horizon', type=int, default=128)
ap.add_argument('--utd', type=int, default=2)
ap.add_argument('--policy-utd', type=int, default=1)
ap.add_argument('--policy-update-per', type=int, default=1)
ap.add_argument('--n', type=int, default=20)
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]

import numpy as np
import torch
if not torch.cuda.is_available():
    sys.exit('utd_timing: needs a GPU')
import bench
from offpolicy_rnn import alg_init
from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate

torch.manual_seed(1234)
np.random.seed(1234)
par = bench.make_parameter(args.rnn, args.rows, args.horizon, algo=args.algo)
par.utd, par.policy_utd, par.policy_update_per = args.utd, args.policy_utd, args.policy_update_per
alg = alg_init(par)
alg.defer_log = True
bench.fill_synthetic(alg, 2 * args.rows, args.horizon, 0)
why = GraphedUpdate.refusal(alg)
gu = GraphedUpdate(alg, warmup=1) if why is None else None


def window(form, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        form()
        alg.grad_num += 1
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / n


period = max(1, args.policy_update_per)
warm_steps = 0
window(alg.train_one_batch, 2 * period)                 # allocator, lazily initialised kernels, both schedules of the eager form
if gu is not None:
    while warm_steps < 8 * period + 8:
        before = gu.eager_fallbacks
        window(gu.step, period)
        warm_steps += period
        if gu.eager_fallbacks == before:                # a whole period replayed: every launch sequence the windows use is recorded
            break
    else:
        sys.exit(f'utd_timing: still {gu.eager_fallbacks} eager passes after {warm_steps} warm-up steps')

n = period * max(1, args.n // period)                   # whole periods: every window holds the same mix of passes
ms = dict(eager=[], replayed=[])
eager_in_windows = 0
for _ in range(args.repeats):                           # alternating: a drift of the box's clocks lands on both forms
    if gu is not None:
        before = gu.eager_fallbacks
        ms['replayed'].append(window(gu.step, n))
        eager_in_windows += gu.eager_fallbacks - before
    ms['eager'].append(window(alg.train_one_batch, n))

out = dict(root=os.path.basename(ROOT), rnn=args.rnn, algo=args.algo, rows=args.rows, horizon=args.horizon, utd=args.utd,
           policy_utd=args.policy_utd, policy_update_per=args.policy_update_per, steps_per_window=n, windows=args.repeats,
           refusal=why, graphs=None if gu is None else len(gu.graphs), warm_steps=warm_steps,
           eager_passes_in_replayed_windows=None if gu is None else eager_in_windows)
for form, v in ms.items():
    out[form] = None if not v else dict(ms_per_step=[round(x, 4) for x in v], ms_per_step_median=round(statistics.median(v), 4),
                                        ms_per_pass_median=round(statistics.median(v) / args.utd, 4),
                                        ms_per_pass_min=round(min(v) / args.utd, 4), ms_per_pass_max=round(max(v) / args.utd, 4))
if gu is not None:
    gu.close()
print(json.dumps(out))
