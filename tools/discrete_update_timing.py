"""Wall time of the replayed discrete-action update with the head, target value and losses in HIP (`RESEL_DISCRETE_FUSED=1`, the default)
against the torch spelling (`RESEL_DISCRETE_FUSED=0`, the launch sequence before the switch existed), on one box.

The trainer is the benchmark's at the published width (`smamba_s32_c16_b2_nln`, D = 256, 64 rows) on `synthetic-o17-d6-T1000` - the
environment `tools/eval_timing.py --env synthetic-o17-d6-T1000` builds: 6 discrete actions, 1000-step rows - with 128 synthetic
trajectories in its replay ring; every update is one `GraphedUpdate.step()`.

    python tools/discrete_update_timing.py [--repeats 3] [--steps 20] [--rnn ID] [--rows 64] [--child-timeout 240]

Every measurement is a fresh child process under its own `timeout`; the two settings alternate (1, 0, 1, 0, ...); after the first
non-zero exit nothing more is started.  Behind the timed children one more child per setting watches ONE eager update with the
profiler on the ATen dispatcher (calls per op name) and times the head's unused `torch.multinomial` draw on its own.
Prints one JSON line per child and a closing summary line: ms per update (median, min, max over the children of a setting), the
run-to-run spread of each setting, and the census."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
ENV = 'synthetic-o17-d6-T1000'

ap = argparse.ArgumentParser()
ap.add_argument('--rnn', default='smamba_s32_c16_b2_nln')
ap.add_argument('--rows', type=int, default=64)
ap.add_argument('--steps', type=int, default=20, help='timed updates per child')
ap.add_argument('--repeats', type=int, default=3, help='children per setting')
ap.add_argument('--child-timeout', type=int, default=240, help='seconds, per child')
ap.add_argument('--child', choices=['time', 'census'], default=None, help=argparse.SUPPRESS)
args = ap.parse_args()


def build():
    import numpy as np
    import torch
    import bench
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.env_utils.make_env import make_env
    torch.manual_seed(1234)
    np.random.seed(1234)
    T = make_env(ENV, 0)['max_trajectory_len']
    par = bench.make_parameter(args.rnn, args.rows, T)
    par.env_name = ENV
    alg = alg_init(par)
    assert alg.discrete_env
    obs_dim, n_act = alg.obs_dim, alg.act_dim
    rs = np.random.RandomState(0)
    for _ in range(2 * args.rows):                              # bench.fill_synthetic with action indices and one-hot last actions
        obs, rew = rs.randn(T + 1, obs_dim), rs.randn(T, 1)
        act = rs.randint(n_act, size=(T, 1)).astype(np.float64)
        onehot = np.eye(n_act)[act[:, 0].astype(int)]
        first, last = np.zeros((T, 1)), np.zeros((T, 1))
        first[0], last[-1] = 1, 1
        alg.replay_buffer.push_trajectory(dict(
            state=obs[:-1], last_state=np.vstack((np.zeros((1, obs_dim)), obs[:-2])), last_action=np.vstack((np.zeros((1, n_act)), onehot[:-1])),
            action=act, next_state=obs[1:], reward=rew, logp=None, mask=np.ones((T, 1)), start=first, done=last,
            reward_input=np.vstack((np.zeros((1, 1)), rew[:-1])), timeout=last))
    return alg, T


def child_time():
    import torch
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    alg, T = build()
    why = GraphedUpdate.refusal(alg)
    assert why is None, why
    gu = GraphedUpdate(alg, warmup=1)
    try:
        for _ in range(4):                                      # the eager warm-up update, the shape's first visit, the recording, one replay
            gu.step()
            alg.grad_num += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            gu.step()
            alg.grad_num += 1
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        graphs = len(gu.graphs)
    finally:
        gu.close()
    print(json.dumps(dict(kind='time', fused=os.environ.get('RESEL_DISCRETE_FUSED', '1'), ms_per_update=round(ms, 4), steps=args.steps,
                          graphs=graphs, rows=args.rows, T=T, rnn=args.rnn)), flush=True)


def child_census():
    import collections
    import torch
    from torch.profiler import profile, ProfilerActivity
    alg, T = build()
    alg.train_one_batch()
    alg.grad_num += 1
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        alg.train_one_batch()
        torch.cuda.synchronize()
    calls = collections.Counter(e.name for e in prof.events() if e.name.startswith('aten::'))
    # the head's draw on its own: [rows * T, A] probabilities, one sample per row, as process_model_out calls it (twice per update)
    probs = torch.full((args.rows * T, alg.act_dim), 1.0 / alg.act_dim, device=alg.device)
    for _ in range(3):
        torch.multinomial(probs, 1, True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        torch.multinomial(probs, 1, True)
    b.record()
    torch.cuda.synchronize()
    print(json.dumps(dict(kind='census', fused=os.environ.get('RESEL_DISCRETE_FUSED', '1'), aten_calls=sum(calls.values()), aten_distinct=len(calls),
                          multinomial_us_per_draw=round(1e3 * a.elapsed_time(b) / 20, 1), multinomial_calls=calls.get('aten::multinomial', 0),
                          calls=dict(sorted(calls.items())))), flush=True)


def spawn(kind, fused):
    cmd = ['timeout', '-k', '10', str(args.child_timeout), sys.executable, os.path.abspath(__file__), '--child', kind, '--rnn', args.rnn,
           '--rows', str(args.rows), '--steps', str(args.steps)]
    r = subprocess.run(cmd, env={**os.environ, 'RESEL_DISCRETE_FUSED': fused}, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:                                       # a fault, an abort or the time limit: nothing more is started
        sys.stderr.write(r.stderr[-4000:])
        print(json.dumps(dict(kind=kind, fused=fused, failed=r.returncode)), flush=True)
        sys.exit(r.returncode)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    times = {'1': [], '0': []}
    for _ in range(args.repeats):
        for fused in ('1', '0'):
            times[fused].append(spawn('time', fused)['ms_per_update'])
    census = {fused: spawn('census', fused) for fused in ('1', '0')}
    stat = lambda v: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), spread=round(max(v) - min(v), 4))
    gone = {k: n for k, n in census['0']['calls'].items() if k not in census['1']['calls']}
    print(json.dumps(dict(
        kind='summary', rnn=args.rnn, rows=args.rows, env=ENV, repeats=args.repeats, steps=args.steps,
        fused_ms=stat(times['1']), plain_ms=stat(times['0']),
        fused_minus_plain_ms=round(statistics.median(times['1']) - statistics.median(times['0']), 4),
        aten_calls=dict(fused=census['1']['aten_calls'], plain=census['0']['aten_calls']),
        aten_ops_only_in_plain=gone, multinomial_us_per_draw=census['1']['multinomial_us_per_draw'],
        multinomial_calls_per_update=census['1']['multinomial_calls'])), flush=True)


if __name__ == '__main__':
    if args.child == 'time':
        child_time()
    elif args.child == 'census':
        child_census()
    else:
        main()
