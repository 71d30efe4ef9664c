"""Wall time and bytes of one `save_state` / `load_state` (algorithm/run_state.py) of the README trainer - smamba_s32_c16_b2_nln, D = 256,
updates of 64 x 1024 - with the ring filled to --fill transitions, beside the duration of each 1000-step iteration (one update per
step) of the same run, so the share of a state in the default cadence of 25 iterations is visible (profiles/r23_resume.md).

    python tools/resume_cost.py --fill 100000
    python tools/resume_cost.py --fill 1000000 [--out DIR]     # DIR: where the states are written (default: a fresh temporary directory)

The host clock runs around each call with a device synchronise on either side; `save_state` ends with the files flushed to the disk.  Every call is
made twice (the first `save_state` also pays first-use costs).  Prints one JSON line."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
ap = argparse.ArgumentParser()
ap.add_argument('--fill', type=int, default=100000, help='transitions in the ring when the timed run starts')
ap.add_argument('--iterations', type=int, default=3)
ap.add_argument('--out', default=None)
args = ap.parse_args()
os.environ.pop('RESEL_CHECKPOINT_DIR', None)

import torch
import bench
from offpolicy_rnn import alg_init

T = 1024


def parameter():
    par = bench.make_parameter('smamba_s32_c16_b2_nln', 64, T, D=256)
    par.max_buffer_transition_num = 1000000
    par.total_iteration, par.step_per_iteration = args.iterations, 1000
    par.random_num, par.start_train_num, par.update_interval = T, 0, 1
    par.test_nprocess = par.test_nrollout = 0
    return par


alg = alg_init(parameter())
alg.logger.quiet = True
warmup = alg.warmup


def warm_and_fill():
    """The warm-up episode fixes the ring's column layout; synthetic trajectories fill the rest."""
    n = warmup()
    bench.fill_synthetic(alg, args.fill // T - len(alg.replay_buffer), T, 0)
    return n


stamps, dump = [], alg.logger.dump_tabular


def stamped():
    torch.cuda.synchronize()
    stamps.append(time.perf_counter())
    dump()


alg.warmup, alg.logger.dump_tabular = warm_and_fill, stamped
torch.cuda.synchronize()
t0 = time.perf_counter()
alg.train()
iterations = [b - a for a, b in zip(stamps[:-1], stamps[1:])]          # the first iteration (warm-up, fill, captures) is not one of them

out = args.out or tempfile.mkdtemp(prefix='resel_state_cost_')
saves, loads = [], []
for k in range(2):
    torch.cuda.synchronize()
    t = time.perf_counter()
    path = alg.save_state(os.path.join(out, f'state-{k}'))
    saves.append(time.perf_counter() - t)
files = {f: os.path.getsize(os.path.join(path, f)) for f in sorted(os.listdir(path))}
fresh = alg_init(parameter())
for k in range(2):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fresh.load_state(path)
    torch.cuda.synchronize()
    loads.append(time.perf_counter() - t)
assert fresh.replay_buffer.size == alg.replay_buffer.size and torch.equal(fresh.policy.store.flat, alg.policy.store.flat)
print(json.dumps(dict(fill=args.fill, transitions=alg.replay_buffer.size, trajectories=len(alg.replay_buffer), ring_width=alg.replay_buffer.width,
                      first_iteration_seconds=round(stamps[0] - t0, 3), iteration_seconds=[round(x, 3) for x in iterations], updates=alg.grad_num,
                      save_seconds=[round(x, 3) for x in saves], load_seconds=[round(x, 3) for x in loads], bytes=files,
                      total_bytes=sum(files.values()))), flush=True)
shutil.rmtree(out, ignore_errors=True)
