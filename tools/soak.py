"""Soak run: N consecutive updates of the bench configuration; prints the log scalars every 20 updates and checks they stay finite.
python tools/soak.py [rnn] [updates] [graph]     third argument 'graph': every update through GraphedUpdate.step() (replays)
SOAK_RAGGED=lo:hi   variable-length episodes: a trainer sized like the reference's published runs (sac_batch_size 1999, episodes of at
                    most 1000 steps: row capacity 1024) whose ring holds 400 early-terminating trajectories with lengths uniform in lo..hi
SOAK_BUCKETS=off|on|auto   shape buckets of the update graphs (eager updates: 'on' pads the batches the same way); default off
The last line reports graphs held, eager updates and wall ms per update after the warm-up (the first 100 updates, a third of a shorter run);
the time is that of a training loop only with SOAK_RAGGED (logs read two updates late) - other runs read every log at once."""
import sys, os, math, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
import numpy as np
import torch
import bench
from bench import build_trainer
rnn = sys.argv[1] if len(sys.argv) > 1 else 'smamba_s32_c16_b2_nln'
n = int(sys.argv[2]) if len(sys.argv) > 2 else 120
graph = len(sys.argv) > 3 and sys.argv[3] == 'graph'
buckets = os.environ.get('SOAK_BUCKETS', 'off')


def build_ragged(lo, hi, n_traj=400, T=1000, seed=0):
    from offpolicy_rnn import alg_init
    p = bench.make_parameter(rnn, 2, T)
    p.sac_batch_size, p.max_buffer_transition_num = 1999, n_traj * T
    alg = alg_init(p)
    rs = np.random.RandomState(seed)
    for L in rs.randint(lo, hi + 1, n_traj):
        obs, act, rew = rs.randn(L + 1, bench.OBS), np.tanh(rs.randn(L, bench.ACT)), rs.randn(L, 1)
        first, last = np.zeros((L, 1)), np.zeros((L, 1))
        first[0], last[-1] = 1, 1
        alg.replay_buffer.push_trajectory(dict(
            state=obs[:-1], last_state=np.vstack((np.zeros((1, bench.OBS)), obs[:-2])), last_action=np.vstack((np.zeros((1, bench.ACT)), act[:-1])),
            action=act, next_state=obs[1:], reward=rew, logp=None, mask=np.ones((L, 1)), start=first, done=last,
            reward_input=np.vstack((np.zeros((1, 1)), rew[:-1])), timeout=last * (L == T)))     # early termination: done without timeout
    return alg


if os.environ.get('SOAK_RAGGED'):
    alg = build_ragged(*[int(v) for v in os.environ['SOAK_RAGGED'].split(':')])
else:
    alg = build_trainer(rnn, 64, 1024)
# SOAK_PER=2: the reference's published cadence (the actor steps on every second update: two graphs alternate); SOAK_CLIP=1: gradient-norm clipping on
alg.parameter.policy_update_per = int(os.environ.get('SOAK_PER', '1'))
if os.environ.get('SOAK_CLIP') == '1':
    alg.parameter.value_max_gradnorm, alg.parameter.policy_max_gradnorm = 10.0, 1.0
step = alg.train_one_batch
gu = None
if graph:
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    gu = GraphedUpdate(alg, warmup=1, buckets=buckets)
    step = gu.step
else:
    alg.shape_buckets = buckets == 'on'
# SOAK_RAGGED runs are timed: as a training loop that logs now and then, a log is read two updates later, so that the host never waits for
# the update it has just launched.  Every other run reads each log at once, as this tool always did.
lag = 2 if os.environ.get('SOAK_RAGGED') else 0
alg.defer_log = lag > 0
warm = min(100, n // 3)
tokens = eager0 = 0
t0 = time.perf_counter()
pending = []


def check(i, log):
    vals = {k: (v[0] if isinstance(v, tuple) else v) for k, v in dict(log).items()}
    assert all(math.isfinite(float(v)) for v in vals.values()), (i, vals)
    if i % 20 == 0 or i == n - 1:
        print(i, {k: round(float(vals[k]), 4) for k in ('critic_loss', 'actor_loss', 'log_prob', 'log_alpha', 'target_q_max', 'clip_min', 'clip_max') if k in vals})


for i in range(n):
    if i == warm:
        torch.cuda.synchronize()
        eager0, t0 = gu.eager_fallbacks if gu else 0, time.perf_counter()
    pending.append((i, step()))
    alg.grad_num += 1
    if i >= warm:
        tokens += int(np.prod((gu._plan['nrow'], gu._plan['longest']) if gu else alg.replay_buffer._last_batch_shape))
    if len(pending) > lag:
        check(*pending.pop(0))
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) * 1e3 / max(n - warm, 1)
for item in pending:
    check(*item)
print('soak ok; device memory reserved %.1f GB, graphs %s, buckets %s; after the first %d updates: %.3f ms per update, eager updates %s of %d, '
      '%.0f batch tokens per update' % (torch.cuda.memory_reserved() / 2 ** 30, len(gu.graphs) if gu else '-', gu.buckets if gu else buckets,
                                        warm, ms, gu.eager_fallbacks - eager0 if gu else '-', n - warm, tokens / max(n - warm, 1)))
