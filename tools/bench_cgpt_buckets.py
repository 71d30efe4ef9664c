"""ms per update of a RAGGED cgpt workload at a published-like size, for profiles/r09_cgpt_buckets.md:
cgpt_h8_l4_p0.0_ml1024 between fc layers of width 512, sac_batch_size 799, policy_update_per 2, 64 episodes of 20..1000 steps
(row capacity 1000).
python tools/bench_cgpt_buckets.py MODE [updates] [--root DIR]
  MODE  exact    every update through GraphedUpdate.step() with exact shape keys (what train() does by default: with ragged episodes a
                 key hardly ever recurs, so nearly every update is launched eagerly)
        eager    train_one_batch() directly
        buckets  GraphedUpdate(buckets='on', seq_buckets=True): RESEL_GRAPH_BUCKETS=1 RESEL_GRAPH_SEQ_BUCKETS=1
  --root DIR     import the project from another checkout (the parent commit, built there) instead of this one
Timed: wall clock around the updates after the first third (at least 100 when there are 300), ending in a device synchronise; logs are
read two updates late as a training loop would.  Prints one JSON line.  Compare modes by alternating runs in one job."""
import json
import os
import sys
import time

args = [a for a in sys.argv[1:] if not a.startswith('--')]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if '--root' in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index('--root') + 1])
    args.remove(sys.argv[sys.argv.index('--root') + 1])
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import bench  # noqa: E402

mode = args[0] if args else 'buckets'
n = int(args[1]) if len(args) > 1 else 300
assert mode in ('exact', 'eager', 'buckets'), mode
RNN, WIDTH, BATCH, T, N_TRAJ, LO, HI = 'cgpt_h8_l4_p0.0_ml1024', 512, 799, 1000, 64, 20, 1000


def build():
    from offpolicy_rnn import alg_init
    torch.manual_seed(0)
    np.random.seed(0)
    p = bench.make_parameter(RNN, 2, T, D=WIDTH, algo='sac')
    p.sac_batch_size, p.max_buffer_transition_num, p.policy_update_per = BATCH, N_TRAJ * T, 2
    alg = alg_init(p)
    rs = np.random.RandomState(0)
    for L in rs.randint(LO, HI + 1, N_TRAJ):
        obs, act, rew = rs.randn(L + 1, bench.OBS), np.tanh(rs.randn(L, bench.ACT)), rs.randn(L, 1)
        first, last = np.zeros((L, 1)), np.zeros((L, 1))
        first[0], last[-1] = 1, 1
        alg.replay_buffer.push_trajectory(dict(
            state=obs[:-1], last_state=np.vstack((np.zeros((1, bench.OBS)), obs[:-2])), last_action=np.vstack((np.zeros((1, bench.ACT)), act[:-1])),
            action=act, next_state=obs[1:], reward=rew, logp=None, mask=np.ones((L, 1)), start=first, done=last,
            reward_input=np.vstack((np.zeros((1, 1)), rew[:-1])), timeout=last * (L == T)))
    np.random.seed(11)
    return alg


assert torch.cuda.is_available(), 'a timing needs the GPU'
alg = build()
gu = None
if mode == 'eager':
    step = alg.train_one_batch
else:
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    gu = GraphedUpdate(alg, warmup=1, buckets='on', seq_buckets=True) if mode == 'buckets' else GraphedUpdate(alg, warmup=1)
    step = gu.step
alg.defer_log = True
warm = max(min(100, n // 3), 1)
pending, keys = [], set()
real = padded = slots = 0
worst = 0.0
eager0, t0 = 0, time.perf_counter()


def check(log):
    vals = {k: (v[0] if isinstance(v, tuple) else v) for k, v in dict(log).items()}
    assert all(np.isfinite(float(v)) for v in vals.values()), vals


for i in range(n):
    if i == warm:
        torch.cuda.synchronize()
        eager0, t0 = gu.eager_fallbacks if gu else 0, time.perf_counter()
    pending.append(step())
    alg.grad_num += 1
    if i >= warm and gu is not None:
        pl = gu._plan
        tokens = int(pl['table'].sum())                              # packed tokens of the batch (its one-slot shift has a few less)
        tb = gu.staging.seq_now[0][0]                                       # length of the token table the kernels ran on
        real, padded, slots = real + tokens, padded + tb, slots + pl['nrow'] * pl['longest']
        worst = max(worst, tb / tokens)
    if len(pending) > 2:
        check(pending.pop(0))
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) * 1e3 / (n - warm)
for log in pending:
    check(log)
out = dict(mode=mode, root=os.path.basename(ROOT), updates=n, timed=n - warm, ms_per_update=round(ms, 3))
if gu is not None:
    out.update(graphs=len(gu.graphs), eager_in_window=gu.eager_fallbacks - eager0, keys_seen=len(gu._seen),
               tokens_real=round(real / (n - warm), 1), tokens_run=round(padded / (n - warm), 1), batch_slots=round(slots / (n - warm), 1),
               token_growth_mean=round(padded / real, 3), token_growth_max=round(worst, 3))
    gu.close()
print(json.dumps(out))
