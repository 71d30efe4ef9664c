"""Times the GRU recurrence per hidden width and the gru trainer's update, ONE CHILD PROCESS PER RUN (a run is one sample: run-to-run
spread includes process start, allocator state and clock ramp).

    python tools/gru_width_timing.py [--widths 512,640,768,896,1024] [--padded 200:208,520:640] [--runs 3] [--rows 8] [--steps 256]
                                     [--updates 8x128,64x1024] [--no-update] [--out FILE]

Per width and driver form (persistent; one launch per step, forced with RESEL_GRU_PERSISTENT=0): `ops.gru_seq` forward and backward over
--rows rows of --steps steps, stream-event intervals around the whole call (layout launch, memset and, at a padded width, the pad passes
included), divided by the steps: us per step.  Median of 5 calls inside the child after 2 warm-up calls; the parent prints every run's
figure.  A padded width is timed beside its native neighbour, with the pad passes (`resel_gru_pad_*`, timed alone on the same operands)
as their share of the call.  Update: `bench.py --rnn gru --rows R --horizon T` as the child, its `ms_per_step` (the replayed update).
On a tree without `ops.gru_width_plan` (a parent commit) only the widths native there run: pass --widths 512 --padded ''.
Each child has a time limit; a child that fails ends the tool with its status."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_step(H, rows, steps, padded):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
    import torch
    from offpolicy_rnn.hip import ops
    dev = torch.device('cuda')
    g = torch.Generator(device='cuda').manual_seed(H)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    gi, w, b = r(rows, steps, 3 * H).requires_grad_(True), (r(3 * H, H) / H ** 0.5).requires_grad_(True), (r(3 * H) / H ** 0.5).requires_grad_(True)
    h0, dh = r(rows, H), r(rows, steps, H)

    def event_us(fn):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        return a.elapsed_time(e) * 1e3, out

    fwd, bwd, pad = [], [], []
    for run in range(7):
        t1, y = event_us(lambda: ops.gru_seq(gi, w, b, h0))
        t2, _ = event_us(lambda: torch.autograd.grad(y, (gi, w, b), dh))
        t3 = 0.0
        if padded:
            Hk = ops.gru_width_plan(H).Hk

            yk, gk = torch.zeros(rows, steps, Hk, device=dev), torch.zeros(rows, steps, 3 * Hk, device=dev)

            def passes():                                  # the seven passes of one padded call, the parameter gradients' slice as a second widening
                with torch.no_grad():
                    ops.gru_pad_params(None, None, w, b, Hk), ops.gru_pad_rows(gi, 3, H, Hk), ops.gru_pad_rows(h0, 1, H, Hk)
                    ops.gru_unpad_rows(yk, 1, H, Hk)
                    ops.gru_pad_rows(dh, 1, H, Hk), ops.gru_unpad_rows(gk, 3, H, Hk), ops.gru_pad_params(None, None, w, b, Hk)
            t3, _ = event_us(passes)
        if run >= 2:
            fwd.append(t1), bwd.append(t2), pad.append(t3)
    form = os.environ.get('RESEL_GRU_PERSISTENT', '1')
    print(json.dumps(dict(H=H, rows=rows, steps=steps, persistent_allowed=form != '0', fwd_us_per_step=statistics.median(fwd) / steps,
                          bwd_us_per_step=statistics.median(bwd) / steps, pad_passes_us=statistics.median(pad),
                          fwd_us=statistics.median(fwd), bwd_us=statistics.median(bwd))))


def run_child(argv, env=None, limit=600):
    out = subprocess.run(argv, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=limit)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
        raise SystemExit(f'child {argv} ended with status {out.returncode}')
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child-step', type=int, default=0)
    ap.add_argument('--child-padded', action='store_true')
    ap.add_argument('--widths', default='512,640,768,896,1024')
    ap.add_argument('--padded', default='200:208,520:640')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--rows', type=int, default=8)
    ap.add_argument('--steps', type=int, default=256)
    ap.add_argument('--updates', default='8x128,64x1024')
    ap.add_argument('--no-update', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.child_step:
        return child_step(args.child_step, args.rows, args.steps, args.child_padded)
    me = [sys.executable, os.path.abspath(__file__), '--rows', str(args.rows), '--steps', str(args.steps)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda rs, k: ' / '.join(f'{r[k]:.2f}' for r in rs)
    for H in [int(v) for v in args.widths.split(',') if v]:
        for form, env in (('persistent', {}), ('per-step', {'RESEL_GRU_PERSISTENT': '0'})):
            rs = [run_child(me + ['--child-step', str(H)], env) for _ in range(args.runs)]
            say(f'| {H} | {form} | {args.rows} x {args.steps} | {fmt(rs, "fwd_us_per_step")} | {fmt(rs, "bwd_us_per_step")} |')
    for pair in [p for p in args.padded.split(',') if p]:
        H, Hk = (int(v) for v in pair.split(':'))
        a = [run_child(me + ['--child-step', str(H), '--child-padded']) for _ in range(args.runs)]
        n = [run_child(me + ['--child-step', str(Hk)]) for _ in range(args.runs)]
        share = ' / '.join(f'{100 * r["pad_passes_us"] / (r["fwd_us"] + r["bwd_us"]):.1f}%' for r in a)
        say(f'| {H} on {Hk} | {fmt(a, "fwd_us_per_step")} | {fmt(a, "bwd_us_per_step")} | {fmt(n, "fwd_us_per_step")} | {fmt(n, "bwd_us_per_step")} | '
            f'{fmt(a, "pad_passes_us")} us = {share} |')
    if not args.no_update:
        for shape in [s for s in args.updates.split(',') if s]:
            rows, horizon = shape.split('x')
            bench = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--rnn', 'gru', '--rows', rows, '--horizon', horizon, '--steps', '10',
                     '--warmup', '3', '--no-cpu-baseline', '--no-suite', '--no-graph-leg', '--no-strict-leg', '--no-rccl-leg']
            rs = [run_child(bench, limit=900) for _ in range(args.runs)]
            say(f'| gru update {rows} x {horizon} | {fmt(rs, "ms_per_step")} ms |')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
