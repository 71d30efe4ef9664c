"""cgpt at head widths other than 32 and 64, through the model: embedding width 128 with 8 heads (hd = 16, runs zero-padded on the
32-wide kernels) and with 1 head (hd = 128, its own kernels).  The decoder layer forward / backward and one whole TD3 update against
the oracle (patterns and tolerances of tests/test_trainer_gpu.py `test_cgpt_layer_gpu_vs_oracle` / `test_cgpt_td3_update_gpu_vs_oracle`),
the graphed policy step against the eager one (tests/test_rollout_gpu.py `test_graphed_policy_step_matches_eager`, tests/test_policy_eval_gpu.py
`test_graphed_step_row_reset`).  Before these widths had kernels every test here stopped at the first forward with the attention
entry's invalid-argument return."""
import numpy as np
import pytest
import torch

from test_host_logic import _push, _synth, make_parameter

pytestmark = pytest.mark.gpu
D = 128
HEADS = [8, 1]                                              # hd = 16 and hd = 128


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')


@pytest.fixture
def cpu_noise(monkeypatch):
    """The update draws its actor noise on the host, as the oracle trainer does (not inside a stream capture: the step tests go without)."""
    from offpolicy_rnn.utility import rng
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.randn(tuple(shape), dtype=dtype).to(device))


@pytest.mark.parametrize('nhead', HEADS)
def test_decoder_layer_fwd_bwd_vs_oracle(nhead):
    """Two decoder blocks at D = 128, three rows of 70 tokens holding six sequences: output, dx and every parameter gradient."""
    from offpolicy_rnn.models.rnn_base import RNNBase
    from offpolicy_rnn.models.flash_attention.TransformerFlashAttention import PackedSeqs, TransformerDecoder
    from oracle import network as NW
    lid, B, L = f'cgpt_h{nhead}_l2_p0.0_ml256_rms', 3, 70
    torch.manual_seed(3)
    net = RNNBase(D, D, [], ['linear'], [lid])
    dec = [m for m in net.modules() if isinstance(m, TransformerDecoder)]
    assert len(dec) == 1 and dec[0].n_head == nhead and dec[0].decoder_layers[0].mha.head_dim == D // nhead
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x, w = torch.randn(B, L, D), torch.randn(B, L, D)
    table = np.zeros((B, L), dtype=np.int64)
    table[0, :3], table[1, :2], table[2, :1] = (1, 40, 29), (30, 40), (70,)
    xr = x.clone().requires_grad_(True)
    pr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = NW.rnn_base_forward(pr, dict(layer_type=[lid], activation=['linear']), xr, NW.Flags(seqlens=torch.from_numpy(table)))
    (ref * w).sum().backward()
    net.to('cuda')
    net.eval()
    xg = x.clone().cuda().requires_grad_(True)
    hid = net.make_init_state(B, torch.device('cuda'))
    hid.set_attention_concat_mask(PackedSeqs(table, L, torch.device('cuda')))
    y, _, _ = net.meta_forward(xg, hid)
    (y * w.cuda()).sum().backward()

    def rel(got, want, name, tol):
        e = (got.detach().cpu() - want.detach()).abs().max().item() / max(want.abs().max().item(), 1e-3)
        print(f'MEASURED cgpt h{nhead} D{D} layer {name}: max err / max|ref| = {e:.3e} (bound {tol:g})')
        assert e < tol, (name, e)
    rel(y, ref, 'y', 1e-2)
    rel(xg.grad, xr.grad, 'dx', 2e-2)
    for k, p in net.named_parameters():
        rel(p.grad, pr[k].grad, 'd ' + k, 2e-2)


@pytest.mark.parametrize('nhead', HEADS)
def test_td3_update_vs_oracle(nhead, cpu_noise):
    """One whole update on cuda:0 against the oracle trainer, logged scalars at the bf16 tolerance of the cgpt update test."""
    from offpolicy_rnn import alg_init
    from oracle.trainer import OracleTrainer, default_parameter
    from test_oracle_golden import _push as opush
    lid, lens = f'cgpt_h{nhead}_l2_p0.0_ml64_rms', [12, 5, 7, 12, 4, 9, 6]
    torch.manual_seed(5)
    alg = alg_init(make_parameter(lid, D=D, algo='td3', sac_batch_size=33))
    par = default_parameter(rnn=lid, D=D, algo='td3', sac_batch_size=33, policy_embedding_dim=16, value_embedding_dim=16,
                            policy_uni_model_input_mapping_dim=16, value_uni_model_input_mapping_dim=16, max_buffer_transition_num=5000)
    cpu_sd = lambda m: {k: {n: t.detach().cpu() for n, t in d.items()} for k, d in m.state_dict().items()}
    tr = OracleTrainer(par, 5, 3, 12, policy_state=cpu_sd(alg.policy), value_state=cpu_sd(alg.values[0]))
    rs = np.random.RandomState(9)
    for n in lens:
        o, a, r = _synth(rs, n, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=(n != 12))
        opush(tr.buffer, o, a, r, early_done=(n != 12))
    logs = []
    for runner in (alg, tr):
        torch.manual_seed(200)
        np.random.seed(200)
        logs.append(runner.train_one_batch())
    for k, v in logs[1].items():
        got = logs[0][k][0] if isinstance(logs[0][k], tuple) else logs[0][k]
        want = v[0] if isinstance(v, tuple) else v
        print(f'MEASURED cgpt h{nhead} D{D} td3 update {k}: {got:.6g} vs oracle {want:.6g}')
        assert got == pytest.approx(want, rel=5e-2, abs=5e-2), (k, got, want)


STEP_TOL = 3e-2                                             # the cgpt tolerance of test_graphed_policy_step_matches_eager


@pytest.mark.parametrize('nhead', HEADS)
def test_graphed_policy_step_matches_eager(nhead):
    """20 steps of the graphed policy step against the eager step; the KV cache is held at the kernel width."""
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.hip import ops
    from offpolicy_rnn.hip.graph_step import GraphedPolicyStep
    from offpolicy_rnn.utility.sample_utility import n2t_2dim
    rnn = f'cgpt_h{nhead}_l2_p0_ml32'
    alg = alg_init(make_parameter(rnn, D=D, algo='td3', cuda_inference=True))
    dev = alg.device
    assert dev.type == 'cuda' and alg.graph_step is not None
    rs = np.random.RandomState(3)
    o, a, n = alg.obs_dim, alg.act_dim, 20
    obs, acts, rew = rs.randn(n + 1, 1, o), np.tanh(rs.randn(n + 1, 1, a)), rs.randn(n + 1, 1, 1)
    step = GraphedPolicyStep(alg.policy, dev)
    hid = alg.policy.make_init_state(1, dev)
    step.load_hidden(hid)
    for t in range(n):
        with torch.no_grad():
            mean, _, _, _, hid, _ = alg.policy.forward(state=n2t_2dim(obs[t + 1], dev), lst_state=n2t_2dim(obs[t], dev),
                                                       lst_action=n2t_2dim(acts[t], dev), rnn_memory=hid, reward=n2t_2dim(rew[t], dev))
        gmean, gsample, glogp = step(obs[t + 1], obs[t], acts[t], rew[t])
        np.testing.assert_allclose(gmean, mean.reshape(1, -1).cpu().numpy(), rtol=STEP_TOL, atol=STEP_TOL, err_msg=f'{rnn} step {t}')
        assert np.isfinite(gsample).all() and np.isfinite(glogp).all()
    caches = [c for ip in step._counters() for c in ip.key_value_memory_dict.values()]
    assert caches and all(c.shape[-1] == ops.attn_head_pad(D // nhead) and c.shape[-2] == nhead for c in caches)


@pytest.mark.parametrize('nhead', HEADS)
def test_graphed_step_row_reset_two_rows_five_steps_apart(nhead):
    """row_reset=True: row 1 starts its episode 5 steps after row 0; each row equals a one-row step that was reset at the same step."""
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.hip.graph_step import GraphedPolicyStep
    rnn = f'cgpt_h{nhead}_l2_p0_ml32'
    alg = alg_init(make_parameter(rnn, D=D, algo='td3', cuda_inference=True))
    alg.policy.eval()
    B, n = 2, 20
    rs = np.random.RandomState(2)
    o, a = alg.obs_dim, alg.act_dim
    obs, acts, rew = rs.randn(n + 1, B, o), np.tanh(rs.randn(n + 1, B, a)), rs.randn(n + 1, B, 1)
    batched = GraphedPolicyStep(alg.policy, alg.device, batch_size=B, row_reset=True)
    singles = [GraphedPolicyStep(alg.policy, alg.device, batch_size=1) for _ in range(B)]
    for s1 in singles:
        s1.load_hidden(None)
    for t in range(n):
        flags = np.zeros(B, dtype=bool)
        flags[1] = t == 5
        mean_b = batched(obs[t + 1], obs[t], acts[t], rew[t], reset=flags if t else None)[0]
        for r, s1 in enumerate(singles):
            if flags[r]:
                s1.load_hidden(None)
            mean_1 = s1(obs[t + 1, r:r + 1], obs[t, r:r + 1], acts[t, r:r + 1], rew[t, r:r + 1])[0]
            np.testing.assert_allclose(mean_b[r:r + 1], mean_1, rtol=STEP_TOL, atol=STEP_TOL, err_msg=f'{rnn} step {t} row {r}')
    assert batched._row_pos.tolist() == [20, 15]
