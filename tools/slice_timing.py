"""Time one `train_one_batch()` of the slice trainer (`sac_rnn_slice`) in its two launch forms: `GraphedTransitionUpdate.step()` - one
H2D, `utd` graph replays, one D2H - against the eager `train_one_batch()` of this same tree (plan + gather + the same kernels, launched
one by one); and `ops.gather_slices` alone at the same shape.  obs 17 / act 6 (bench.py's synthetic ring, 28 columns), two `fc` critics,
`sac_batch_size = 256`, `rnn_slice_length = 64`, D = 256, `utd = 1`, `policy_utd = 1`; layers `gru` and `smamba_s32_c16_b2_nln`.

    python tools/slice_timing.py [--layers gru smamba_s32_c16_b2_nln] [--runs 3] [--n 30] [--windows 3] [--leg-timeout 150]

Every run of every form is a LEG: a child process of its own (`--leg`), under its own time limit, that builds the trainer, warms the form
up (the replayed form until a whole step ran without an eager pass) and times `--windows` windows of `--n` steps under a host clock,
each ending in a device synchronise; logs are deferred, so neither form waits for the step it has just launched.  The legs of the two
forms alternate, so a drift of the box's clocks lands on both.  The `gather` leg times 200 launches of `ops.gather_slices` between two
device events, three times, and reports the median with the bytes it moves (the ring rows it reads, the whole output it writes).
The parent prints every leg's JSON line as the leg ends and then one summary line.  A leg that fails or runs out of time ends the
measurement: nothing further is started.  No GPU: an error."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--layers', nargs='+', default=['gru', 'smamba_s32_c16_b2_nln'])
ap.add_argument('--runs', type=int, default=3)
ap.add_argument('--n', type=int, default=30)
ap.add_argument('--windows', type=int, default=3)
ap.add_argument('--batch', type=int, default=256)
ap.add_argument('--length', type=int, default=64)
ap.add_argument('--width', type=int, default=256)
ap.add_argument('--utd', type=int, default=1)
ap.add_argument('--leg-timeout', type=float, default=150.0)
ap.add_argument('--leg', choices=['replayed', 'eager', 'gather'], default=None)
args = ap.parse_args()


def parent():
    legs = [('gather', args.layers[0])] + [(form, lid) for lid in args.layers for _ in range(args.runs) for form in ('replayed', 'eager')]
    results = []
    for form, lid in legs:
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', form, '--layers', lid, '--n', str(args.n), '--windows', str(args.windows),
               '--batch', str(args.batch), '--length', str(args.length), '--width', str(args.width), '--utd', str(args.utd)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.leg_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f'slice_timing: the {form} leg of {lid} ran out of its {args.leg_timeout:.0f} s; nothing further is started')
        if done.returncode != 0:
            sys.exit(f'slice_timing: the {form} leg of {lid} ended with status {done.returncode}; nothing further is started\n{done.stderr[-2000:]}')
        results.append(json.loads(done.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)       # every leg as it ends; the summary is the last line
    out = dict(shape=dict(obs=17, act=6, width=args.width, critics=2, batch=args.batch, length=args.length, utd=args.utd, policy_utd=1),
               steps_per_window=args.n, windows=args.windows, gather=results[0], box=results[0]['box'])
    for lid in args.layers:
        for form in ('replayed', 'eager'):
            runs = [r for r in results if r['leg'] == form and r['layer'] == lid]
            med = [r['ms_per_step_median'] for r in runs]
            out[f'{lid}_{form}'] = dict(ms_per_step=med, min=min(med), max=max(med), median=round(statistics.median(med), 4),
                                        windows=[r['ms_per_step'] for r in runs], graphs=runs[0].get('graphs'),
                                        eager_passes_in_windows=sum(r.get('eager_passes_in_windows', 0) for r in runs))
        out[f'{lid}_every_replayed_run_faster_than_the_fastest_eager'] = out[f'{lid}_replayed']['max'] < out[f'{lid}_eager']['min']
    print(json.dumps(out))


def leg():
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('slice_timing: needs a GPU')
    import bench
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm.graphed_transition_update import GraphedTransitionUpdate
    from offpolicy_rnn.hip import ops
    lid, T = args.layers[0], 2 * args.length
    torch.manual_seed(1234)
    np.random.seed(1234)
    par = bench.make_parameter(lid, 64, T, D=args.width)
    par.alg_name = 'sac_rnn_slice'
    par.value_layer_type = ['fc'] * len(par.value_layer_type)
    par.value_net_num, par.sac_batch_size, par.rnn_slice_length, par.utd, par.policy_utd = 2, args.batch, args.length, args.utd, 1
    alg = alg_init(par)
    alg.defer_log = True
    bench.fill_synthetic(alg, 128, T, 0)
    out = dict(leg=args.leg, layer=lid, box=torch.cuda.get_device_name(0))

    def window(form, n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n):
            form()
            alg.grad_num += 1
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / n

    if args.leg == 'gather':
        ring, B, L = alg.replay_buffer, args.batch, args.length
        mirror = ring._mirror(alg.device)
        plan = ring.plan_slices(B, L, 1)
        plan_dev = torch.from_numpy(plan).to(alg.device)
        c_done, c_timeout = alg._ring_columns()
        pairs = alg._pre_pairs()[1]
        launch = lambda: ops.gather_slices(mirror, plan_dev, L, pairs, None, 0, c_done, c_timeout)
        for _ in range(20):
            launch()
        us = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(200):
                launch()
            b.record()
            torch.cuda.synchronize()
            us.append(1e3 * a.elapsed_time(b) / 200)
        W = ring.width
        moved = 4 * W * (int(plan[0, :, 1].sum()) + B + B * (L + 1))          # ring rows read (+ the first row again for slot 0), output written
        med = statistics.median(us)
        out.update(us_per_launch=[round(x, 3) for x in us], us_per_launch_median=round(med, 3), columns=W, bytes_moved=moved,
                   padded_share=round(1 - float(plan[0, :, 1].sum()) / (B * L), 4), tb_per_s=round(moved / med / 1e6, 4),
                   share_of_8_tb_per_s=round(moved / med / 1e6 / 8, 5))
    elif args.leg == 'eager':
        window(alg.train_one_batch, 3)
        ms = [window(alg.train_one_batch, args.n) for _ in range(args.windows)]
        out.update(ms_per_step=[round(x, 4) for x in ms], ms_per_step_median=round(statistics.median(ms), 4))
    else:
        gu = GraphedTransitionUpdate(alg, warmup=1)
        for _ in range(16):
            before = gu.eager_fallbacks
            window(gu.step, 1)
            if gu.eager_fallbacks == before:            # a whole step replayed: every launch sequence is recorded
                break
        else:
            sys.exit(f'slice_timing: still {gu.eager_fallbacks} eager passes after 16 warm-up steps')
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
