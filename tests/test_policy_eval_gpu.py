"""Batched policy evaluation on the GPU: the per-row KV-cache decode and the in-graph state reset kernels, the graphed policy step
with per-row episode starts, the evaluator against the reference's sequential loop, and the hook in `train()`."""
import numpy as np
import pytest
import torch

from oracle import kernels as K

pytestmark = pytest.mark.gpu
HORIZONS = [3, 7, 5, 7, 2, 4]
STEP_IDS = [('gru', 'sac'), ('smamba_s8_c4_b2_nln', 'sac'), ('gilr', 'td3'), ('lru', 'sac'), ('gilr_lstm', 'sac'), ('conv1d_3', 'sac'),
            ('mamba_s8_c3', 'td3'), ('cgpt_h1_l2_p0_ml32', 'td3')]        # the list of test_graphed_policy_step_matches_eager


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def _step_tol(rnn):
    return 3e-2 if rnn.startswith('cgpt') else 1e-5           # test_graphed_policy_step_matches_eager's own


# ------------------------------------------------------------------------------------------------ 1. decode with one position per row
@pytest.mark.parametrize('B,H,hd,S,steps,starts', [(3, 4, 64, 40, 38, (0, 13, 30)), (2, 2, 32, 300, 290, (287, 0))])
def test_attn_decode_rows(ops, B, H, hd, S, steps, starts):
    """Row b starts a new episode (position 0) at step starts[b]; before that it decodes an earlier episode from step 0, so its slab
    holds stale keys beyond its position.  At the last step the rows stand at steps - 1 - starts[b]: (37, 24, 7) and (2, 289)."""
    g = torch.Generator().manual_seed(H * hd + B)
    qkv = torch.randn(steps + 1, B, 3, H, hd, generator=g).to(torch.bfloat16).cuda()
    slopes = K.alibi_slopes(H)
    sl, scale = slopes.cuda(), hd ** -0.5
    cache = torch.zeros(B, S, 2, H, hd, dtype=torch.bfloat16, device='cuda')
    pos = torch.zeros(B, dtype=torch.int32, device='cuda')
    singles = [(torch.zeros(1, S, 2, H, hd, dtype=torch.bfloat16, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'))
               for _ in range(B)]
    got, want = [], []
    for t in range(steps):
        for b, s0 in enumerate(starts):
            if t == s0:
                pos[b] = 0
        got.append(ops.attn_decode(qkv[t], cache, pos, sl, scale))
        pos += 1
        row = []
        for b, (c1, p1) in enumerate(singles):
            if t >= starts[b]:                                   # a B = 1 cache that holds this episode of the row only
                row.append(ops.attn_decode(qkv[t, b:b + 1], c1, p1, sl, scale)[0])
                p1 += 1
            else:
                row.append(got[-1][b])
        want.append(torch.stack(row))
    got, want = torch.stack(got), torch.stack(want)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))                 # bit for bit, every step of every row
    final = [steps - 1 - s0 for s0 in starts]
    assert pos.tolist() == [p + 1 for p in final]
    if S == 300:
        assert final[1] >= 257 and final[0] <= 3                 # past the 256-thread key stride next to a row that just started
    host = qkv.cpu()
    for b, s0 in enumerate(starts):
        for t in sorted({steps - 1, min(s0 + 257, steps - 1), s0}):
            p = t - s0
            ref = K.attn_decode_ref(host[t, b:b + 1, 0], host[s0:t + 1, b, 1].unsqueeze(0), host[s0:t + 1, b, 2].unsqueeze(0), p, slopes, scale)
            np.testing.assert_allclose(got[t, b:b + 1].float().cpu(), ref, rtol=2e-2, atol=2e-2, err_msg=f'row {b} step {t}')   # test_attn_decode_vs_oracle's
    # a row at position S: NaN in its own output, nothing written; the other rows go on as if alone
    bad = 0
    before = cache.clone()
    pos[bad] = S
    out = ops.attn_decode(qkv[steps], cache, pos, sl, scale)
    assert torch.isnan(out[bad].float()).all() and torch.equal(cache[bad], before[bad])
    for b, (c1, p1) in enumerate(singles):
        if b != bad:
            one = ops.attn_decode(qkv[steps, b:b + 1], c1, p1, sl, scale)[0]
            assert torch.isfinite(out[b].float()).all() and torch.equal(out[b].view(torch.int16), one.view(torch.int16))


# ------------------------------------------------------------------------------------------------ 2. state reset
def _reset_case():
    g = torch.Generator().manual_seed(4)
    a = torch.randn(5, 5, generator=g).cuda()
    b = torch.randn(1, 5, 96, generator=g).cuda()
    wide = torch.randn(5, 1037, generator=g).cuda()              # odd row stride: the rows of the view differ in alignment
    c = wide[:, 1:1028]                                            # width 1027, row stride 1037, base 4 bytes past a 16-byte boundary
    assert c.data_ptr() % 16 == 4 and c.stride(0) > c.shape[1]
    counters = [torch.arange(1, 6, dtype=torch.int32).cuda(), torch.full((5,), 9, dtype=torch.int32).cuda()]
    return [a, b, c], wide, counters


def test_step_state_reset(ops):
    tensors, wide, counters = _reset_case()
    keep = [t.clone() for t in tensors] + [wide.clone()] + [c.clone() for c in counters]
    flags = torch.tensor([1, 0, 0, 1, 0], dtype=torch.int32).cuda()
    ops.step_state_reset(torch.zeros_like(flags), tensors, counters)                    # all-zero flags change nothing
    for t, k in zip(tensors + [wide] + counters, keep):
        assert torch.equal(t, k)
    ops.step_state_reset(flags, tensors, counters)
    torch.cuda.synchronize()
    on = flags.bool()
    for t, k in zip(tensors, keep):
        t2, k2 = t.reshape(5, -1), k.reshape(5, -1)
        assert float(t2[on].abs().sum()) == 0.0
        assert torch.equal(t2[~on].view(torch.int32), k2[~on].view(torch.int32))
    expect = keep[3].clone()
    expect[on, 1:1028] = 0.0
    assert torch.equal(wide.view(torch.int32), expect.view(torch.int32))                # the gaps between the rows of the view too
    for c, k in zip(counters, keep[4:]):
        assert torch.equal(c, torch.where(on, torch.zeros_like(k), k))


def test_step_state_reset_more_tables_than_one_call_holds(ops):
    g = torch.Generator().manual_seed(5)
    tensors = [torch.randn(3, 1 + i, generator=g).cuda() for i in range(19)]              # widths 1..19: every head / body / tail split
    counters = [torch.full((3,), i + 1, dtype=torch.int32).cuda() for i in range(9)]
    keep = [t.clone() for t in tensors]
    ops.step_state_reset(torch.tensor([0, 7, 0], dtype=torch.int32).cuda(), tensors, counters)
    for t, k in zip(tensors, keep):
        assert float(t[1].abs().sum()) == 0.0 and torch.equal(t[0], k[0]) and torch.equal(t[2], k[2])
    for i, c in enumerate(counters):
        assert c.tolist() == [i + 1, 0, i + 1]


# ------------------------------------------------------------------------------------------------ 3. graphed step with per-row starts
@pytest.mark.parametrize('rnn,algo', STEP_IDS)
def test_graphed_step_row_reset(ops, rnn, algo):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.hip.graph_step import GraphedPolicyStep
    from test_host_logic import make_parameter
    alg = alg_init(make_parameter(rnn, algo=algo, cuda_inference=True))
    alg.policy.eval()
    B, n = 3, 6
    resets = {2: [1], 4: [0, 2]}
    rs = np.random.RandomState(2)
    o, a = alg.obs_dim, alg.act_dim
    obs, acts, rew = rs.randn(n + 1, B, o), np.tanh(rs.randn(n + 1, B, a)), rs.randn(n + 1, B, 1)
    batched = GraphedPolicyStep(alg.policy, alg.device, batch_size=B, row_reset=True)
    singles = [GraphedPolicyStep(alg.policy, alg.device, batch_size=1) for _ in range(B)]
    for s1 in singles:
        s1.load_hidden(None)
    tol = _step_tol(rnn)
    for t in range(n):
        flags = np.zeros(B, dtype=bool)
        flags[resets.get(t, [])] = True
        mean_b = batched(obs[t + 1], obs[t], acts[t], rew[t], reset=flags if t else None)[0]
        for r, s1 in enumerate(singles):
            if flags[r]:
                s1.load_hidden(None)
            mean_1 = s1(obs[t + 1, r:r + 1], obs[t, r:r + 1], acts[t, r:r + 1], rew[t, r:r + 1])[0]
            np.testing.assert_allclose(mean_b[r:r + 1], mean_1, rtol=tol, atol=tol, err_msg=f'{rnn} step {t} row {r}')
    if rnn.startswith('cgpt'):                                    # row 1 stands at 4, rows 0 and 2 at 2: row 1 fills its 32 positions first
        assert batched._row_pos.tolist() == [2, 4, 2]
        for t in range(28):
            batched(obs[0], obs[1], acts[0], rew[0])
        with pytest.raises(RuntimeError, match=r'KV cache is full \(row 1'):
            batched(obs[0], obs[1], acts[0], rew[0])
        batched.invalidate()                                      # a new capture warms up although row 1 has a full cache
        mean = batched(obs[0], obs[1], acts[0], rew[0], reset=[0, 1, 0])[0]              # the refused step launched nothing
        assert np.isfinite(mean).all() and batched._row_pos.tolist() == [31, 1, 31]


def test_graphed_step_without_row_reset_is_as_before(ops):
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.hip.graph_step import GraphedPolicyStep
    from test_host_logic import make_parameter
    alg = alg_init(make_parameter('cgpt_h1_l1_p0_ml32', cuda_inference=True))
    step = GraphedPolicyStep(alg.policy, alg.device, batch_size=2)
    z = np.zeros((2, alg.obs_dim)), np.zeros((2, alg.obs_dim)), np.zeros((2, alg.act_dim)), np.zeros((2, 1))
    with pytest.raises(ValueError, match='row_reset'):
        step(*z, reset=[1, 0])
    assert step._graph is None
    step(*z)
    assert step._counters() and all(ip.device_offset.numel() == 1 for ip in step._counters())        # one cgpt position for all rows
    assert step._in_host.shape == (2, 2 * alg.obs_dim + alg.act_dim + 1)


# ------------------------------------------------------------------------------------------------ 4. evaluator vs the sequential loop
class ScriptedEnv:
    """Seeded; the k-th reset over all environments that share `episodes` starts an episode of HORIZONS[k] steps; the next observation
    depends on the action; the reward is the mean of the action (1-Lipschitz in the largest action error)."""

    def __init__(self, episodes, obs_dim, act_dim):
        from offpolicy_rnn.env_utils.make_env import Box
        self.observation_space, self.action_space = Box(-np.inf, np.inf, (obs_dim,)), Box(-1.0, 1.0, (act_dim,))
        self.mix = np.random.RandomState(0).randn(obs_dim, act_dim) * 0.5
        self.episodes, self.rs, self.live = episodes, np.random.RandomState(0), False

    def seed(self, s):
        self.rs = np.random.RandomState(s)

    def reset(self):
        self.h, self.t, self.live = HORIZONS[self.episodes[0]], 0, True
        self.episodes[0] += 1
        self.x = self.rs.randn(self.observation_space.shape[0])
        return self.x.copy()

    def step(self, action):
        assert self.live, 'environment stepped between done and reset'
        action = np.asarray(action, dtype=np.float64)
        self.t += 1
        self.x = 0.6 * self.x + self.mix @ action + 0.1 * self.rs.randn(self.x.shape[0])
        self.live = self.t < self.h
        return self.x.copy(), float(action.mean()), not self.live, {}


def _sequential(policy, envs, rows_of_episode, act_dim, dev):
    """The reference's `policy_eval` loop (utility/sample_utility.py:50-100) at B = 1, eager, episode k on environment
    rows_of_episode[k]."""
    from offpolicy_rnn.utility.sample_utility import n2t_2dim, t2n, unorm_act
    rets, lens = [], []
    for r in rows_of_episode:
        env = envs[r]
        ep_ret, ep_len = 0, 0
        state_np = env.reset().reshape(1, -1)
        last_action_np, last_state_np, reward_np = np.zeros((1, act_dim)), np.zeros_like(state_np), np.zeros((1, 1))
        hidden, done = policy.make_init_state(1, device=dev), False
        while not done:
            with torch.no_grad():
                act_mean, _, _, _, hidden, _ = policy.forward(state=n2t_2dim(state_np, dev), lst_state=n2t_2dim(last_state_np, dev),
                                                              lst_action=n2t_2dim(last_action_np, dev), rnn_memory=hidden,
                                                              reward=n2t_2dim(reward_np, dev))
            act_mean = t2n(act_mean).reshape(1, -1)
            next_state, reward, done, _ = env.step(unorm_act(act_mean[0], env.action_space))
            last_state_np, state_np = state_np.copy(), next_state.reshape(1, -1).copy()
            reward_np[:] = reward
            last_action_np = act_mean.copy()
            ep_ret += reward
            ep_len += 1
        rets.append(ep_ret)
        lens.append(ep_len)
    return rets, lens


@pytest.mark.parametrize('rnn', ['gru', 'smamba_s8_c4_b1_nln', 'cgpt_h1_l1_p0.1_ml32'])
def test_evaluator_matches_the_sequential_loop(ops, rnn):
    import random
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.utility.policy_eval import BatchedPolicyEval
    from test_host_logic import make_parameter
    alg = alg_init(make_parameter(rnn, cuda_inference=True))
    alg.policy.train()
    o, a, dev = alg.obs_dim, alg.act_dim, alg.device
    episodes = [0]
    ev = BatchedPolicyEval(alg.policy, lambda: ScriptedEnv(episodes, o, a), a, 4, dev, seed=3)
    random.seed(1), np.random.seed(2), torch.manual_seed(3), torch.cuda.manual_seed(4)
    before = (random.getstate(), np.random.get_state(), torch.get_rng_state().clone(), torch.cuda.get_rng_state(dev).clone())
    out = ev.evaluate(6)
    assert random.getstate() == before[0] and all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), before[1]))
    assert torch.equal(torch.get_rng_state(), before[2]) and torch.equal(torch.cuda.get_rng_state(dev), before[3])
    from offpolicy_rnn.utility.policy_eval import _is_training
    assert _is_training(alg.policy)                               # the mode the policy had comes back
    assert ev.last_rows == [0, 1, 2, 3, 0, 0]
    # the reference's loop on identically seeded environments
    ref_episodes = [0]
    ref_envs = [ScriptedEnv(ref_episodes, o, a) for _ in range(4)]
    for env, s in zip(ref_envs, ev.env_seeds):
        env.seed(s + 5)
    alg.policy.eval()
    rets, lens = _sequential(alg.policy, ref_envs, ev.last_rows, a, dev)
    alg.policy.train()
    assert out['EpLenTest'] == lens == HORIZONS
    diffs = [abs(x - y) for x, y in zip(out['EpRetTest'], rets)]
    print(f'{rnn}: largest |EpRetTest - sequential| = {max(diffs):.3e} (bounds {[4 * h * _step_tol(rnn) for h in HORIZONS]})')
    for k, (d, h) in enumerate(zip(diffs, HORIZONS)):
        assert d <= 4 * h * _step_tol(rnn), (k, d)
    if 'p0.1' in rnn:                                             # dropout is off and no generator is consumed: the same numbers again
        episodes[0] = 0
        for env, s in zip(ev.envs, ev.env_seeds):
            env.seed(s + 5)
        again = ev.evaluate(6)
        assert again['EpRetTest'] == out['EpRetTest'] and again['EpLenTest'] == out['EpLenTest']


# ------------------------------------------------------------------------------------------------ 5. train()
def _flat(store):
    if hasattr(store, 'flat_views'):
        return torch.cat([v.detach().reshape(-1) for _, v in sorted(store.flat_views().items())]).clone()
    return store.flat.detach().clone()


@pytest.mark.parametrize('rnn', ['smamba_s8_c4_b1_nln', 'cgpt_h1_l1_p0_ml32'])
def test_train_logs_evaluations_and_is_not_perturbed(ops, rnn, tmp_path, monkeypatch):
    from offpolicy_rnn import alg_init
    from test_host_logic import _short_run_parameter
    monkeypatch.chdir(tmp_path)
    runs = []
    for over in (dict(test_nprocess=2, test_nrollout=2), dict(test_nprocess=2, test_nrollout=0)):
        alg = alg_init(_short_run_parameter(rnn, cuda_inference=True, **over))
        logged, add = [], alg.logger.add_tabular_data

        def record(tb_prefix=None, _logged=logged, _add=add, **kw):
            _logged.append((tb_prefix, {k: v for k, v in kw.items() if k.endswith('Test')}))
            return _add(tb_prefix=tb_prefix, **kw)

        monkeypatch.setattr(alg.logger, 'add_tabular_data', record)
        alg.train()
        runs.append((logged, _flat(alg.policy.store), _flat(alg.values[0].store), alg))
    perf = [kw for prefix, kw in runs[0][0] if prefix == 'performance']
    assert len(perf) == 2                                         # once per iteration
    for kw in perf:
        assert len(kw['EpRetTest']) == 4 and kw['EpLenTest'] == [12] * 4 and np.isfinite(kw['EpRetTest']).all()
    assert runs[0][3].evaluator is not None and runs[0][3].evaluator.rows == 4
    assert not any(kw for _, kw in runs[1][0]) and runs[1][3].evaluator is None
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])      # evaluation does not perturb training
