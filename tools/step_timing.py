"""Wall time of the B = 1 rollout step (`SAC.sample_action`: what `train()` runs once per environment step) at the published width
(D = 256) on a synthetic environment - `-a<n>-` continuous, `-d<n>-` discrete actions.  The launch form is the trainer's own: a
hipGraph replay, or the eager `policy.forward` with RESEL_GRAPH_ROLLOUT=0.

    python tools/step_timing.py [--rnn smamba_s32_c16_b2_nln] [--env synthetic-o17-d6-T1000] [--steps 2000] [--n 5]

Prints one JSON line per layer id: microseconds per step, median / min / max over `--n` loops of `--steps` steps behind one warm-up
loop (which captures the graph).  The inputs change every step (the sampled action and a fresh observation are fed back)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]

ap = argparse.ArgumentParser()
ap.add_argument('--rnn', nargs='+', default=['smamba_s32_c16_b2_nln'])
ap.add_argument('--env', default='synthetic-o17-d6-T1000')
ap.add_argument('--steps', type=int, default=2000)
ap.add_argument('--n', type=int, default=5)
args = ap.parse_args()

import numpy as np
import torch
import bench
from offpolicy_rnn import alg_init

for rnn in args.rnn:
    torch.manual_seed(1234)
    np.random.seed(1234)
    par = bench.make_parameter(rnn, 2, 1000, algo='sac')
    par.env_name = args.env
    alg = alg_init(par)
    alg.env_reset()

    def loop():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.steps):
            act = alg.sample_action()
            next_state, reward, done, _ = alg.env.step(int(act[0, 0]) if alg.discrete_env else act[0])
            alg.env_step(next_state, act, reward, done)
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t) / args.steps

    loop()
    us = [loop() for _ in range(args.n)]
    print(json.dumps(dict(rnn=rnn, env=args.env, launch='graph replay' if alg.graph_step is not None else 'eager', steps=args.steps, n=args.n,
                          us_per_step=dict(median=round(statistics.median(us), 1), min=round(min(us), 1), max=round(max(us), 1)))), flush=True)
