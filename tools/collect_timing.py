"""Wall time of `train()` on a discrete T-Maze: the training rollout inside the policy step's graph (utility/device_collect.py
`DeviceCollector`, the default follows profiles/r20_device_collect.md) against the host loop (`RESEL_DEVICE_COLLECT=0`).  One process
= one leg; the host clock runs around `alg.train()` with a device synchronise on either side, so the warm-up, the graph captures
and - in the training workload - the evaluations and updates are inside the figure on every leg alike.

    python tools/collect_timing.py --workload collect [--rnn smamba_s32_c16_b2_nln] [--D 256] [--steps 20020]
        collection only: `Mem-T-passive-1000-v0` (1001 steps an episode), one random warm-up episode, no update (`start_train_num`
        beyond the run), no evaluation, `--steps` environment steps in one iteration
    python tools/collect_timing.py --workload train [--iterations 40]
        the short training run of profiles/r19_device_env.md, shortened: `Mem-T-passive-10-v0`, gru, D = 32, `sac_batch_size` 1100, one update
        per 11 steps behind 1100 random steps, 10 evaluation episodes at the start of each iteration of 1100 steps
    python tools/collect_timing.py --workload collect --env Wind-v0 --rnn smamba_b1_c8_s64_ff --steps 20000
        collection only on another environment make_env.py builds without gym (`Wind-v0`, `synthetic-o2-a2-T75`): one random warm-up
        episode, no update, no evaluation
    --tree DIR   time the sources of another checkout (DIR/bench.py, DIR/recurrent-offpolicy-rl_amd), e.g. the parent commit's

Prints one JSON line: seconds, environment steps of the loop, microseconds per step, updates, and which path collected."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--workload', choices=['collect', 'train'], default='collect')
ap.add_argument('--rnn', default=None)
ap.add_argument('--D', type=int, default=None)
ap.add_argument('--steps', type=int, default=20020)
ap.add_argument('--iterations', type=int, default=40)
ap.add_argument('--env', default=None, help='collect workload: the environment (default Mem-T-passive-1000-v0)')
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--label', default='')
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]

import torch
import bench
from offpolicy_rnn import alg_init
from offpolicy_rnn.env_utils.make_env import make_env

if args.workload == 'collect':
    rnn = args.rnn or 'smamba_s32_c16_b2_nln'
    D = args.D or (32 if rnn == 'gru' else 256)
    env_name = args.env or 'Mem-T-passive-1000-v0'
    T = make_env(env_name, 0)['max_trajectory_len']
    par = bench.make_parameter(rnn, 2, T, D=D)
    par.env_name = env_name
    par.random_num, par.start_train_num, par.update_interval = T, 10 ** 9, 1
    par.total_iteration, par.step_per_iteration = 1, args.steps
    par.test_nprocess = par.test_nrollout = 0
    par.max_buffer_transition_num = 200000
else:
    rnn, D = args.rnn or 'gru', args.D or 32
    par = bench.make_parameter(rnn, 100, 11, D=D)
    par.env_name = 'Mem-T-passive-10-v0'
    par.sac_batch_size, par.max_buffer_transition_num = 1100, 1000000
    par.random_num, par.start_train_num, par.update_interval = 1100, 1100, 11
    par.total_iteration, par.step_per_iteration = args.iterations, 1100
    par.test_nprocess, par.test_nrollout = 5, 2
alg = alg_init(par)
alg.logger.quiet = True
torch.cuda.synchronize()
t0 = time.perf_counter()
alg.train()
torch.cuda.synchronize()
seconds = time.perf_counter() - t0
steps = par.total_iteration * par.step_per_iteration
collector = getattr(alg, 'collector', None)
print(json.dumps(dict(label=args.label, workload=args.workload, rnn=rnn, D=D, env=par.env_name, steps=steps, updates=alg.grad_num,
                      path='device' if collector is not None else 'host', seconds=round(seconds, 4), us_per_step=round(1e6 * seconds / steps, 1),
                      replays=getattr(collector, 'replays', None), episode_syncs=getattr(collector, 'episode_syncs', None),
                      episodes_in_ring=len(alg.replay_buffer), transitions_in_ring=alg.replay_buffer.size)), flush=True)
