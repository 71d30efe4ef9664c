#!/usr/bin/env python3
"""Per-update time of critics with per-member context encoders (`elru-<E>` / `econv1d[_<K>]-<E>`) at the README shape.

    python tools/ensemble_encoder_timing.py [--rows 64] [--steps 1024] [--runs 3] [--updates 6] [--out FILE.json]

Shape: bench.py's trainer (64 rows x 1024 steps, D = 256, obs 17 / act 6, `efc-8` critic head, REDQ) with the critic's embedding stack
replaced by ['efc-8', 'elru-8', 'efc-8'] and ['efc-8', 'econv1d_4-8', 'efc-8']; the policy keeps ['fc', 'gilr', 'fc'].  Every combination
of id and RESEL_MEMBER_SEQ (1: member kernels, 0: E launches of the single-member entries plus the torch add + LayerNorm) is run
`--runs` times, each run in a child process of its own, the combinations interleaved; for context one more child times the
shared-encoder critic ['fc', 'lru', 'fc'].  A child warms up, then times `--updates` eager `train_one_batch()` calls and as many
replays of the recorded update (`GraphedUpdate`), each window between device synchronisations, and prints one JSON line.
Needs a GPU: a child that finds none fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {'elru-8': ['efc-8', 'elru-8', 'efc-8'], 'econv1d_4-8': ['efc-8', 'econv1d_4-8', 'efc-8'], 'lru (shared encoder)': ['fc', 'lru', 'fc']}


def child(args):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    import bench
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate

    def build():
        torch.manual_seed(0)
        np.random.seed(0)
        p = bench.make_parameter('gilr', args.rows, args.steps)
        p.value_embedding_layer_type = CASES[args.case]
        alg = alg_init(p)
        bench.fill_synthetic(alg, 2 * args.rows, args.steps, 0)
        return alg

    def timed(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.updates):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.updates * 1e3

    alg = build()
    for _ in range(3):
        alg.train_one_batch()
    eager_ms = timed(alg.train_one_batch)
    peak_gb = torch.cuda.max_memory_allocated() / 2 ** 30
    del alg
    torch.cuda.empty_cache()
    alg = build()
    gu = GraphedUpdate(alg, warmup=1)
    try:
        for _ in range(4):                    # one eager pass, the shape's second occurrence is recorded, then replays
            gu.step()
        replay_ms = timed(gu.step)
        graphs, fallbacks = len(gu.graphs), gu.eager_fallbacks
    finally:
        gu.close()
    print(json.dumps(dict(case=args.case, member_seq=os.environ.get('RESEL_MEMBER_SEQ', 'unset'), rows=args.rows, steps=args.steps,
                          updates=args.updates, eager_ms=round(eager_ms, 3), replay_ms=round(replay_ms, 3), graphs=graphs,
                          eager_fallbacks=fallbacks, peak_gb=round(peak_gb, 2))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=64)
    ap.add_argument('--steps', type=int, default=1024)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--updates', type=int, default=6)
    ap.add_argument('--out', default=None)
    ap.add_argument('--case', default=None, help=argparse.SUPPRESS)          # set for a child
    args = ap.parse_args()
    if args.case is not None:
        return child(args)
    plan = [(case, sw) for _ in range(args.runs) for case in ('elru-8', 'econv1d_4-8') for sw in ('1', '0')] + [('lru (shared encoder)', '1')]
    results = []
    for case, sw in plan:
        env = dict(os.environ, RESEL_MEMBER_SEQ=sw)
        cmd = [sys.executable, os.path.abspath(__file__), '--case', case, '--rows', str(args.rows), '--steps', str(args.steps), '--updates', str(args.updates)]
        run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:               # a failed child ends the measurement: nothing more is started behind it
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            raise SystemExit(f'child {case} RESEL_MEMBER_SEQ={sw} failed with {run.returncode}')
        line = [ln for ln in run.stdout.splitlines() if ln.startswith('{')][-1]
        results.append(json.loads(line))
        print(line, flush=True)
        if args.out:
            with open(args.out, 'w') as f:
                json.dump(results, f, indent=1)
    for case in ('elru-8', 'econv1d_4-8'):
        for key in ('eager_ms', 'replay_ms'):
            on = [r[key] for r in results if r['case'] == case and r['member_seq'] == '1']
            off = [r[key] for r in results if r['case'] == case and r['member_seq'] == '0']
            print(f'{case} {key}: RESEL_MEMBER_SEQ=1 {on}  =0 {off}  every =1 run beats the fastest =0 run: {max(on) < min(off)}')


if __name__ == '__main__':
    main()
