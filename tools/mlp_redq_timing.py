"""Time one `train_one_batch()` of the memoryless REDQ trainer (`sac_mlp_redq_ensemble_q`) at REDQ's usual shape in its two launch
forms: `GraphedTransitionUpdate.step()` - one H2D, `utd` graph replays, one D2H - against the eager `train_one_batch()` of this same
tree (plan + gather + the same kernels, launched one by one).  obs 17 / act 6 (bench.py's synthetic ring), D = 256, `efc-10` critic
stacks, `redq_m = 2`, `sac_batch_size = 256`, `policy_utd = 1`; `utd = 20` and `utd = 1`.

    python tools/mlp_redq_timing.py [--utd 20 1] [--runs 3] [--n 40] [--windows 3] [--leg-timeout 120]

Every run of every form is a LEG: a child process of its own (`--leg`), under its own time limit, that builds the trainer, warms the form
up (the replayed form until a whole step ran without an eager pass) and times `--windows` windows of `--n` steps under a host clock,
each ending in a device synchronise; logs are deferred, so neither form waits for the step it has just launched.  The legs of the two
forms alternate, so a drift of the box's clocks lands on both.  One more leg counts the kernels of a pass with the actor step (an
eagerly launched `utd = 1` step under torch's profiler; the two norms of the log, launched once per step, are in that count).
The parent prints every leg's JSON line as the leg ends and then one summary line: per utd and form the median ms per step of every run, their spread, and the kernel count.  A leg that
fails or runs out of time ends the measurement: nothing further is started.  No GPU: an error."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--utd', type=int, nargs='+', default=[20, 1])
ap.add_argument('--runs', type=int, default=3)
ap.add_argument('--n', type=int, default=40)
ap.add_argument('--windows', type=int, default=3)
ap.add_argument('--batch', type=int, default=256)
ap.add_argument('--ensemble', type=int, default=10)
ap.add_argument('--width', type=int, default=256)
ap.add_argument('--leg-timeout', type=float, default=120.0)
ap.add_argument('--leg', choices=['replayed', 'eager', 'kernels'], default=None)
args = ap.parse_args()


def parent():
    legs = [('kernels', 1)] + [(form, utd) for utd in args.utd for _ in range(args.runs) for form in ('replayed', 'eager')]
    results = []
    for form, utd in legs:
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', form, '--utd', str(utd), '--n', str(args.n), '--windows', str(args.windows),
               '--batch', str(args.batch), '--ensemble', str(args.ensemble), '--width', str(args.width)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f'mlp_redq_timing: the {form} leg at utd = {utd} ran out of its {args.leg_timeout:.0f} s; nothing further is started')
        if done.returncode != 0:
            sys.exit(f'mlp_redq_timing: the {form} leg at utd = {utd} ended with status {done.returncode}; nothing further is started\n{done.stderr[-2000:]}')
        results.append(json.loads(done.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)       # every leg as it ends; the summary is the last line
    out = dict(shape=dict(obs=17, act=6, width=args.width, ensemble=args.ensemble, redq_m=2, batch=args.batch, policy_utd=1),
               steps_per_window=args.n, windows=args.windows, kernels_per_pass=results[0]['kernels'], box=results[0]['box'])
    for utd in args.utd:
        for form in ('replayed', 'eager'):
            runs = [r for r in results if r['leg'] == form and r['utd'] == utd]
            med = [r['ms_per_step_median'] for r in runs]
            out[f'utd{utd}_{form}'] = dict(ms_per_step=med, min=min(med), max=max(med), median=round(statistics.median(med), 4),
                                           ms_per_pass_median=round(statistics.median(med) / utd, 4), windows=[r['ms_per_step'] for r in runs],
                                           graphs=runs[0].get('graphs'), eager_passes_in_windows=sum(r.get('eager_passes_in_windows', 0) for r in runs))
        out[f'utd{utd}_every_replayed_run_faster_than_the_fastest_eager'] = out[f'utd{utd}_replayed']['max'] < out[f'utd{utd}_eager']['min']
    print(json.dumps(out))


def leg():
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('mlp_redq_timing: needs a GPU')
    import bench
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm.graphed_transition_update import GraphedTransitionUpdate
    utd, E, T = args.utd[0], args.ensemble, 64
    torch.manual_seed(1234)
    np.random.seed(1234)
    par = bench.make_parameter('fc', 64, T, D=args.width)
    par.alg_name = 'sac_mlp_redq_ensemble_q'
    par.value_embedding_layer_type, par.value_layer_type = [f'efc-{E}'] * 3, [f'efc-{E}'] * 3
    par.policy_embedding_layer_type, par.policy_layer_type = ['fc'] * 3, ['fc'] * 3
    par.redq_m, par.sac_batch_size, par.utd, par.policy_utd, par.rnn_fix_length = 2, args.batch, utd, 1, 0
    alg = alg_init(par)
    alg.defer_log = True
    bench.fill_synthetic(alg, 128, T, 0)
    out = dict(leg=args.leg, utd=utd, box=torch.cuda.get_device_name(0))

    def window(form, n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            form()
            alg.grad_num += 1
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / n

    if args.leg == 'kernels':
        from torch.profiler import ProfilerActivity, profile
        window(alg.train_one_batch, 3)
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            window(alg.train_one_batch, 1)
        names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA') and not e.name.lower().startswith(('memcpy', 'memset'))]
        out.update(kernels=len(names), distinct=len(set(names)))
    elif args.leg == 'eager':
        window(alg.train_one_batch, 3)
        ms = [window(alg.train_one_batch, args.n) for _ in range(args.windows)]
        out.update(ms_per_step=[round(x, 4) for x in ms], ms_per_step_median=round(statistics.median(ms), 4))
    else:
        gu = GraphedTransitionUpdate(alg, warmup=1)
        for _ in range(16):
            before = gu.eager_fallbacks
            window(gu.step, 1)
            if gu.eager_fallbacks == before:            # a whole step replayed: both launch sequences are recorded
                break
        else:
            sys.exit(f'mlp_redq_timing: still {gu.eager_fallbacks} eager passes after 16 warm-up steps')
        before = gu.eager_fallbacks
        ms = [window(gu.step, args.n) for _ in range(args.windows)]
        out.update(ms_per_step=[round(x, 4) for x in ms], ms_per_step_median=round(statistics.median(ms), 4), graphs=len(gu.graphs),
                   eager_passes_in_windows=gu.eager_fallbacks - before)
        gu.close()
    print(json.dumps(out))


if __name__ == '__main__':
    if args.leg is None:
        parent()
    else:
        leg()
