"""Discrete actions on the GPU above the head kernel: the graphed policy step of a categorical policy against the eager step, per-row
episode starts, the batched evaluator against the reference's sequential loop, the evaluation hook of `train()`, and the update graph.

A categorical policy at initialisation is close to uniform over its actions; the last layer of the head is scaled by HEAD_SCALE so
that the two largest probabilities stand apart.  Every comparison of action indices states the gap it relies on and asserts it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ENV = 'synthetic-o5-d4-T12'
NACT = 4
LAYERS = ['gru', 'smamba_s8_c4_b1_nln', 'cgpt_h1_l1_p0_ml32']
HORIZONS = [3, 7, 5, 7, 2, 4]                                   # tests/test_policy_eval_gpu.py
HEAD_SCALE = 40.0
MIN_GAP = 1e-3


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def _step_tol(rnn):
    return 3e-2 if rnn.startswith('cgpt') else 1e-5           # tests/test_rollout_gpu.py::test_graphed_policy_step_matches_eager's own


def _alg(rnn, **over):
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    alg = alg_init(make_parameter(rnn, env=ENV, cuda_inference=True, **over))
    assert alg.discrete_env and alg.act_dim == NACT
    with torch.no_grad():
        alg.policy.uni_network.layer_list[-1].weight.mul_(HEAD_SCALE)
    return alg


def _inputs(seed, n, B, o):
    rs = np.random.RandomState(seed)
    obs, rew = rs.randn(n + 1, B, o), rs.randn(n + 1, B, 1)
    onehot = np.eye(NACT)[rs.randint(0, NACT, size=(n + 1, B))]
    return obs, onehot, rew


def _top_two_gap(logp):
    top = torch.sort(logp.double().exp().reshape(-1, logp.shape[-1]), dim=-1, descending=True).values
    return (top[:, 0] - top[:, 1]).min().item() if top.shape[1] > 1 else 1.0


def _state_tensors(hidden):
    return [t for h in hidden._data for t in (h if isinstance(h, tuple) else (h,)) if torch.is_tensor(t)]


# ------------------------------------------------------------------------------------------------ 1. the trainer builds a graph
def test_trainer_builds_a_graphed_step(ops):
    alg = _alg('gru')
    assert alg.graph_step is not None and alg.graph_step.categorical
    assert alg.eval_refusal() is None
    alg.env_reset()
    a = alg.sample_action()
    assert a.shape == (1, 1) and a.dtype == np.int64 and 0 <= int(a[0, 0]) < NACT
    assert alg.graph_step._graph is not None and alg.graph_step._out_dev.shape == (1, 2 + NACT)


# ------------------------------------------------------------------------------------------------ 2. graphed against eager
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('rnn', LAYERS)
def test_graphed_step_matches_eager(ops, rnn, B):
    from offpolicy_rnn.hip.graph_step import GraphedPolicyStep
    alg = _alg(rnn)
    alg.policy.eval()
    dev, o, n = alg.device, alg.obs_dim, 10
    obs, onehot, rew = _inputs(7, n, B, o)
    t3 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev).unsqueeze(1)          # [B, 1, .]
    step = GraphedPolicyStep(alg.policy, dev, batch_size=B)
    hid = alg.policy.make_init_state(B, dev)
    step.load_hidden(alg.policy.make_init_state(B, dev))
    tol, gaps = _step_tol(rnn), []
    for t in range(n):
        with torch.no_grad():
            mode, _, sample, logp, hid, _ = alg.policy.forward(state=t3(obs[t + 1]), lst_state=t3(obs[t]), lst_action=t3(onehot[t]),
                                                               rnn_memory=hid, reward=t3(rew[t]))
        assert mode.dtype == torch.int64 and mode.shape == (B, 1, 1) and sample.shape == (B, 1, 1) and logp.shape == (B, 1, NACT)
        gmode, gsample, glogp = step(obs[t + 1], obs[t], onehot[t], rew[t])
        assert gmode.dtype == np.int64 and gmode.shape == (B, 1) and gsample.dtype == np.int64 and gsample.shape == (B, 1)
        assert glogp.dtype == np.float32 and glogp.shape == (B, NACT)
        np.testing.assert_allclose(glogp, logp.reshape(B, NACT).cpu().numpy(), rtol=tol, atol=tol, err_msg=f'{rnn} step {t}')
        for a, b in zip(_state_tensors(step._hidden), _state_tensors(hid)):
            np.testing.assert_allclose(a.reshape(-1).cpu().numpy(), b.reshape(-1).cpu().numpy(), rtol=tol, atol=tol, err_msg=f'{rnn} state, step {t}')
        gaps.append(_top_two_gap(logp))
        assert gaps[-1] >= MIN_GAP, f'{rnn} step {t}: eager top-two gap {gaps[-1]:.2e}: pick another seed'
        assert np.array_equal(gmode, mode.reshape(B, 1).cpu().numpy()), (rnn, t)
        assert gsample.min() >= 0 and gsample.max() < NACT
        assert abs(np.exp(glogp.astype(np.float64)).sum(axis=1) - 1).max() < 1e-5
    print(f'\n[{rnn} B={B}] smallest eager top-two gap over {n} steps: {min(gaps):.3e}')
    assert step._graph is not None and step._out_dev.shape == (B, 2 + NACT)
    assert step._in_host.shape == (B, 2 * o + NACT + 1)               # the input block of a continuous policy of the same widths


# ------------------------------------------------------------------------------------------------ 3. per-row episode starts
@pytest.mark.parametrize('rnn', LAYERS)
def test_graphed_step_row_reset(ops, rnn):
    """tests/test_policy_eval_gpu.py::test_graphed_step_row_reset for a categorical policy: row 1 starts an episode at step 4 and from
    then on gives the log-probabilities of a fresh B = 1 run; the rows beside it go on."""
    from offpolicy_rnn.hip.graph_step import GraphedPolicyStep
    alg = _alg(rnn)
    alg.policy.eval()
    B, n = 3, 8
    resets = {4: [1], 6: [0, 2]}
    obs, onehot, rew = _inputs(2, n, B, alg.obs_dim)
    batched = GraphedPolicyStep(alg.policy, alg.device, batch_size=B, row_reset=True)
    singles = [GraphedPolicyStep(alg.policy, alg.device, batch_size=1) for _ in range(B)]
    for s1 in singles:
        s1.load_hidden(None)
    tol = _step_tol(rnn)
    for t in range(n):
        flags = np.zeros(B, dtype=bool)
        flags[resets.get(t, [])] = True
        _, sample_b, logp_b = batched(obs[t + 1], obs[t], onehot[t], rew[t], reset=flags if t else None)
        assert sample_b.dtype == np.int64 and sample_b.min() >= 0 and sample_b.max() < NACT
        for r, s1 in enumerate(singles):
            if flags[r]:
                s1.load_hidden(None)
            logp_1 = s1(obs[t + 1, r:r + 1], obs[t, r:r + 1], onehot[t, r:r + 1], rew[t, r:r + 1])[2]
            np.testing.assert_allclose(logp_b[r:r + 1], logp_1, rtol=tol, atol=tol, err_msg=f'{rnn} step {t} row {r}')
    if rnn.startswith('cgpt'):
        assert batched._row_pos.tolist() == [2, 4, 2]


# ------------------------------------------------------------------------------------------------ 4. evaluator vs the sequential loop
class ScriptedDiscreteEnv:
    """Seeded; the k-th reset over all environments that share `episodes` starts an episode of HORIZONS[k] steps; the next observation
    and the reward depend on the action index."""

    def __init__(self, episodes, obs_dim):
        from offpolicy_rnn.env_utils.make_env import Box, Discrete
        self.observation_space, self.action_space = Box(-np.inf, np.inf, (obs_dim,)), Discrete(NACT)
        self.mix = np.random.RandomState(0).randn(obs_dim, NACT)
        self.episodes, self.rs, self.live = episodes, np.random.RandomState(0), False
        self.actions = []

    def seed(self, s):
        self.rs = np.random.RandomState(s)

    def reset(self):
        self.h, self.t, self.live = HORIZONS[self.episodes[0]], 0, True
        self.episodes[0] += 1
        self.x = self.rs.randn(self.observation_space.shape[0])
        return self.x.copy()

    def step(self, action):
        assert self.live, 'environment stepped between done and reset'
        assert type(action) is int and 0 <= action < NACT
        self.actions.append(action)
        self.t += 1
        self.x = 0.6 * self.x + self.mix[:, action] + 0.1 * self.rs.randn(self.x.shape[0])
        self.live = self.t < self.h
        return self.x.copy(), 0.3 * action - 0.1 * self.t + 0.01 * float(self.x[0]), not self.live, {}


def _sequential(policy, envs, rows_of_episode, dev):
    """The reference's `policy_eval` loop (utility/sample_utility.py:50-100) at B = 1, eager: int action, one-hot last action.
    -> (returns, lengths, smallest top-two probability gap over all steps)."""
    from offpolicy_rnn.utility.sample_utility import n2t_2dim, t2n, unorm_act
    rets, lens, gap = [], [], 1.0
    for r in rows_of_episode:
        env = envs[r]
        ep_ret, ep_len = 0, 0
        state_np = env.reset().reshape(1, -1)
        last_action_np, last_state_np, reward_np = np.zeros((1, NACT)), np.zeros_like(state_np), np.zeros((1, 1))
        hidden, done = policy.make_init_state(1, device=dev), False
        while not done:
            with torch.no_grad():
                act_mean, _, _, logp, hidden, _ = policy.forward(state=n2t_2dim(state_np, dev), lst_state=n2t_2dim(last_state_np, dev),
                                                                 lst_action=n2t_2dim(last_action_np, dev), rnn_memory=hidden,
                                                                 reward=n2t_2dim(reward_np, dev))
            gap = min(gap, _top_two_gap(logp))
            index = int(unorm_act(t2n(act_mean).reshape(-1)[0], env.action_space))
            next_state, reward, done, _ = env.step(index)
            last_state_np, state_np = state_np.copy(), next_state.reshape(1, -1).copy()
            reward_np[:] = reward
            last_action_np = np.zeros((1, NACT))
            last_action_np[..., index] = 1
            ep_ret += reward
            ep_len += 1
        rets.append(ep_ret)
        lens.append(ep_len)
    return rets, lens, gap


@pytest.mark.parametrize('rnn', ['gru', 'smamba_s8_c4_b1_nln'])
def test_evaluator_matches_the_sequential_loop(ops, rnn):
    """The fp32 layer families: four rows in one graph and one row eager agree to 1e-5 in every probability, so with a top-two gap of
    at least 1e-3 on every step of the sequential loop both pick the same actions, and equal actions give equal returns to the bit."""
    import random
    from offpolicy_rnn.utility.policy_eval import BatchedPolicyEval, _is_training
    alg = _alg(rnn)
    alg.policy.train()
    o, dev = alg.obs_dim, alg.device
    episodes = [0]
    ev = BatchedPolicyEval(alg.policy, lambda: ScriptedDiscreteEnv(episodes, o), NACT, 4, dev, seed=3, discrete=True)
    random.seed(1), np.random.seed(2), torch.manual_seed(3), torch.cuda.manual_seed(4)
    before = (random.getstate(), np.random.get_state(), torch.get_rng_state().clone(), torch.cuda.get_rng_state(dev).clone())
    out = ev.evaluate(6)
    assert random.getstate() == before[0] and all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), before[1]))
    assert torch.equal(torch.get_rng_state(), before[2]) and torch.equal(torch.cuda.get_rng_state(dev), before[3])
    assert _is_training(alg.policy)
    assert ev.last_rows == [0, 1, 2, 3, 0, 0]
    ref_episodes = [0]
    ref_envs = [ScriptedDiscreteEnv(ref_episodes, o) for _ in range(4)]
    for env, s in zip(ref_envs, ev.env_seeds):
        env.seed(s + 5)
    alg.policy.eval()
    rets, lens, gap = _sequential(alg.policy, ref_envs, ev.last_rows, dev)
    alg.policy.train()
    print(f'\n[{rnn}] smallest top-two gap of the sequential loop: {gap:.3e}')
    assert gap >= MIN_GAP, f'{rnn}: top-two gap {gap:.2e}: pick another seed or head scale'
    assert [e.actions for e in ev.envs] == [e.actions for e in ref_envs]
    assert len({a for e in ref_envs for a in e.actions}) > 1           # the policy does not sit on one action
    assert out['EpLenTest'] == lens == HORIZONS
    assert out['EpRetTest'] == rets                                   # the same rewards summed in the same order: equal to the last bit


# ------------------------------------------------------------------------------------------------ 5. train()
def _flat(store):
    if hasattr(store, 'flat_views'):
        return torch.cat([v.detach().reshape(-1) for _, v in sorted(store.flat_views().items())]).clone()
    return store.flat.detach().clone()


@pytest.mark.parametrize('rnn', ['gru', 'smamba_s8_c4_b1_nln'])
def test_train_logs_evaluations_and_is_not_perturbed(ops, rnn, tmp_path, monkeypatch):
    from offpolicy_rnn import alg_init
    from test_host_logic import _short_run_parameter
    monkeypatch.chdir(tmp_path)
    runs = []
    for over in (dict(test_nprocess=2, test_nrollout=2), dict(test_nprocess=2, test_nrollout=0)):
        alg = alg_init(_short_run_parameter(rnn, env=ENV, cuda_inference=True, **over))
        assert alg.discrete_env
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
    assert runs[0][3].evaluator is not None and runs[0][3].evaluator.rows == 4 and runs[0][3].evaluator.discrete
    assert not any(kw for _, kw in runs[1][0]) and runs[1][3].evaluator is None
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])      # evaluation does not perturb training
    for run in runs:                                              # the rollout steps were graph replays
        assert run[3].graph_step is not None and run[3].graph_step._graph is not None


# ------------------------------------------------------------------------------------------------ 6. the update graph
def _update_alg(rnn):
    """A discrete trainer with eight full-length trajectories in its replay ring (the draws of tests/test_oracle_golden.py
    `push_discrete`): every batch has the same shape, so the second update through `GraphedUpdate` is recorded and the third replayed."""
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.buffers.transition_buffer.replay_memory import Transition
    from test_host_logic import make_parameter
    from test_oracle_golden import push_discrete
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter(rnn, env=ENV, sac_batch_size=4 * 12 - 1, cuda_inference=True))
    assert alg.discrete_env
    rs = np.random.RandomState(3)
    for _ in range(8):
        push_discrete(alg.replay_buffer, Transition, rs, 12, alg.obs_dim, NACT, 12)
    torch.manual_seed(200)
    np.random.seed(200)
    return alg


@pytest.mark.parametrize('rnn', ['gru', 'gilr', 'smamba_s8_c4_b1_nln'])
def test_graphed_discrete_update_equals_the_eager_update(ops, rnn):
    """Three discrete updates through `GraphedUpdate.step` (one eager, one recorded, one replayed) against three eager ones from the same
    seeds: the losses take expectations over all actions, so the head's unused draws do not enter.  rtol 2e-5, atol 2e-7: the
    tolerances of tests/test_trainer_gpu.py::test_graphed_update_equals_the_eager_update."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate

    def state(alg):
        return [alg.policy.store.flat.detach().clone(), alg.values[0].store.flat.detach().clone(),
                alg.target_values[0].store.flat.detach().clone(), alg.log_sac_alpha.detach().clone()]

    val = lambda v: v[0] if isinstance(v, tuple) else v
    eager = _update_alg(rnn)
    logs_e = []
    for _ in range(3):
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    graphed = _update_alg(rnn)
    assert GraphedUpdate.refusal(graphed) is None
    g = GraphedUpdate(graphed, warmup=1)
    logs_g = []
    try:
        for _ in range(3):
            logs_g.append(dict(g.step()))
            graphed.grad_num += 1
        torch.cuda.synchronize()
        print(f'\n[{rnn}] graphs recorded {len(g.graphs)}, eager updates {g.eager_fallbacks} of 3')
        assert len(g.graphs) == 1 and g.eager_fallbacks == 1
    finally:
        g.close()
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), state(graphed), state(eager)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=2e-7, err_msg=nm)
    for le, lg in zip(logs_e, logs_g):
        assert set(le) == set(lg)
        for k in le:
            ve, vg = val(le[k]), val(lg[k])
            assert abs(ve - vg) <= 2e-5 * max(1.0, abs(ve)), (k, ve, vg)
