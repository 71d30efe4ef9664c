"""Time updates with randomised loss masks (`randomize_mask`, valid_number_post_randomized = 256) the way `SAC.train()` launches them:
a hipGraph replay per update where `GraphedUpdate.refusal` allows it (RESEL_GRAPH_BUCKETS as `train()` reads it), eagerly otherwise;
the log is read after every update as `train()`'s logger does, so every sample is device-synchronised.

    python tools/rmask_timing.py --rnn gru --rows 8 --horizon 128 [--rmask 0|1] [--n 20] [--root TREE]

`--root TREE` measures another checkout of this project (its own package and library) from this one script: run the two builds in
alternation, one process each (profiles/r10_rmask.md).  Prints one JSON line: median / min / max ms per update over `--n` updates
behind the warm-up (until a graph replays, then 3 more), the launch form, and the host time of `GraphedUpdate._prepare` (sampling
plan, selection bitmap, pinned staging) where a graph drives the update."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--rnn', default='gru')
ap.add_argument('--rows', type=int, default=8)
ap.add_argument('--horizon', type=int, default=128)
ap.add_argument('--rmask', type=int, default=1)
ap.add_argument('--n', type=int, default=20)
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]

import numpy as np
import torch
import bench
from offpolicy_rnn import alg_init
from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate

torch.manual_seed(1234)
np.random.seed(1234)
par = bench.make_parameter(args.rnn, args.rows, args.horizon)
par.randomize_mask, par.valid_number_post_randomized = bool(args.rmask), 256
alg = alg_init(par)
bench.fill_synthetic(alg, 2 * args.rows, args.horizon, 0)

why = GraphedUpdate.refusal(alg)
update, gu, prep = alg.train_one_batch, None, []
if why is None:
    gu = GraphedUpdate(alg, buckets=GraphedUpdate.buckets_from_env())
    update = gu.step
    inner = gu._prepare

    def timed_prepare():
        t = time.perf_counter()
        key = inner()
        prep.append(1e3 * (time.perf_counter() - t))
        return key
    gu._prepare = timed_prepare


def one():
    torch.cuda.synchronize()
    t = time.perf_counter()
    log = update()
    float(log['critic_loss'])                         # the logger's read: waits for the update
    torch.cuda.synchronize()
    alg.grad_num += 1
    return 1e3 * (time.perf_counter() - t)


warm = 0
while gu is not None and not gu.graphs and warm < 8:  # eager warm-up updates, the shape's first visit, the recording
    one()
    warm += 1
for _ in range(3):
    one()
del prep[:]
ms = [one() for _ in range(args.n)]
masked = float(alg._stats[1])
if gu is not None:
    gu.close()
print(json.dumps(dict(root=os.path.basename(ROOT), rnn=args.rnn, rows=args.rows, horizon=args.horizon, randomize_mask=bool(args.rmask),
                      launch='graph replay' if gu is not None else f'eager ({why})', replayed=None if gu is None else args.n + 3 + warm - gu.eager_fallbacks,
                      device_batch=bool(alg.device_replay and alg.replay_buffer.device_supported(randomize_mask=par.randomize_mask)),
                      loss_positions=masked, median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                      prepare_median_ms=round(statistics.median(prep), 4) if prep else None, n=args.n)))
