"""Wall time of one policy evaluation (`SAC.evaluate`'s work): 10 episodes of 1000 synthetic steps at the published width (D = 256),
(a) 10 rows in ONE graphed step with per-row episode starts (utility/policy_eval.py `BatchedPolicyEval`), against
(b) the 10 episodes one after another through the B = 1 graphed step with `load_hidden(None)` between them - the only form there
    was before `row_reset`.
Both run the same host loop (`run_episodes`), the same environments and the policy in eval mode.  `--env synthetic-o17-d6-T1000` (any
name make_env.py builds without gym) replaces the benchmark's environment; a name with discrete actions (`-d<n>-`, `Mem-T-...-v0`) is a
discrete-action run: categorical policy, the evaluator's discrete form.  A discrete T-Maze (`Mem-T-passive-1000-v0`) is stepped inside
the graph of leg (a) unless RESEL_DEVICE_ENV=0 (utility/policy_eval.py `DeviceEnvEval`); `device_env` in the output says which it was.
`--env Wind-v0` is the meta-RL task (continuous actions, 75 steps, evaluation tasks of seed 0), stepped inside the graph the same way.

    python tools/eval_timing.py [--rnn smamba_s32_c16_b2_nln cgpt_h8_l6_p0.1_ml1024_rms] [--episodes 10] [--steps 1000] [--n 3]
                                [--env synthetic-o17-d6-T1000]

Prints one JSON line per layer id: median / min / max seconds per evaluation over `--n` evaluations behind one warm-up evaluation
(which captures the graph), and microseconds per graph replay."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]

ap = argparse.ArgumentParser()
ap.add_argument('--rnn', nargs='+', default=['smamba_s32_c16_b2_nln', 'cgpt_h8_l6_p0.1_ml1024_rms'])
ap.add_argument('--episodes', type=int, default=10)
ap.add_argument('--steps', type=int, default=1000)
ap.add_argument('--n', type=int, default=3)
ap.add_argument('--env', default=None, help='synthetic-o<obs>-[ad]<act>-T<len>, Mem-T-{passive,active}-<L>-v0 or Wind-v0: replaces the benchmark '
                                            'environment and --steps')
ap.add_argument('--skip-one-by-one', action='store_true', help='time leg (a) only')
args = ap.parse_args()

import numpy as np
import torch
import bench
from offpolicy_rnn import alg_init
from offpolicy_rnn.env_utils.make_env import make_env
from offpolicy_rnn.hip.graph_step import GraphedPolicyStep
from offpolicy_rnn.utility.policy_eval import BatchedPolicyEval, run_episodes


def timed(fn):
    out = []
    for i in range(args.n + 1):                              # the first one captures
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
        assert res['EpLenTest'] == [args.steps] * args.episodes, res['EpLenTest']
    return out[1:]


for rnn in args.rnn:
    torch.manual_seed(1234)
    np.random.seed(1234)
    discrete = args.env is not None and not make_env(args.env, 0)['act_continuous']
    par = bench.make_parameter(rnn, 2, args.steps, algo='td3' if rnn.startswith('cgpt') and not discrete else 'sac')
    if args.env is not None:
        par.env_name = args.env
        args.steps = make_env(args.env, 0)['max_trajectory_len']
    alg = alg_init(par)
    assert alg.discrete_env == discrete
    factory = lambda: make_env(par.env_name, 0)['eval_env']
    batched = BatchedPolicyEval(alg.policy, factory, alg.act_dim, args.episodes, alg.device, discrete=discrete,
                                eval_tasks=make_env(par.env_name, 0).get('eval_tasks'))
    t_rows = timed(lambda: batched.evaluate(args.episodes))

    single = GraphedPolicyStep(alg.policy, alg.device, batch_size=1)
    env = factory()
    env.seed(5)

    def one_by_one():
        def step(state, lst_state, lst_action, reward, reset):
            if reset[0]:
                single.load_hidden(None)
            return single(state, lst_state, lst_action, reward)[0]
        alg.policy.eval()
        try:
            return run_episodes(step, [env], args.episodes, alg.obs_dim, alg.act_dim, lambda e: e.reset(), discrete=discrete)[0]
        finally:
            alg.policy.train()
    t_one = [float('nan')] * args.n if args.skip_one_by_one else timed(one_by_one)
    med = statistics.median
    print(json.dumps(dict(
        rnn=rnn, env=par.env_name, episodes=args.episodes, steps=args.steps, n=args.n, device_env=batched.device_env is not None,
        rows_graph_all_s=[round(t, 4) for t in t_rows],
        rows_graph_s=dict(median=round(med(t_rows), 4), min=round(min(t_rows), 4), max=round(max(t_rows), 4)),
        one_by_one_s=dict(median=round(med(t_one), 4), min=round(min(t_one), 4), max=round(max(t_one), 4)),
        us_per_replay=dict(rows_graph=round(1e6 * med(t_rows) / args.steps, 1), one_by_one=round(1e6 * med(t_one) / (args.steps * args.episodes), 1)),
        ratio=round(med(t_one) / med(t_rows), 2))), flush=True)
