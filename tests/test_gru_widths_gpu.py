"""GRU at every hidden width from 1 to 1024 (csrc/gru_seq.hip through ops.gru_seq / gru_seq_multi, the `gru` module, the trainers): the
native widths above 512 (640, 768, 896, 1024, persistent and one launch per step) and widths that run zero-padded per gate block on the
next native one.  tests/gru_widths.py has the case table, the draw and the bounds (derived on the CPU, asserted by
tests/test_gru_widths_host.py); models and metric are those of tests/recurrence_parity.py.

1. `ops.gru_seq` forward and backward against fp64 at the TRUE width, per (row, 64-step block) and per parameter-gradient element,
   with a live h0 and with none, two runs bit-equal.  2. the padding is exact: the bits of the native run on operands padded in torch.
3. `gru_seq_multi` = `gru_seq` of each job, bit for bit.  4. the module against torch.nn.GRU in fp64, true shapes in its state_dict,
single steps = the sequence.  5. the trainer: batched = serial bit for bit, graph replay = eager, model files and run states at the
true width.  6. native widths never reach the pad entries.

Every kernel comparison prints `GRUW-FIG <case> <output> <fraction of bound>` before anything is asserted (`pytest -s`); the fractions
measured on an MI355X are in profiles/r34_gru_widths.md."""
import os

import numpy as np
import pytest
import torch

import gru_widths as GW
import recurrence_parity as RP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))                 # the fp64 models run on the host
    yield o
    torch.set_num_threads(before)


def _d(t):
    return None if t is None else t.cuda()


def _leaf(t):
    return t.detach().clone().cuda().requires_grad_(True)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _gru(ops, gi, w_hh, b_hh, h0, dh):
    gi, w, b = _leaf(gi), _leaf(w_hh), _leaf(b_hh)
    h = ops.gru_seq(gi, w, b, _d(h0))
    dgi, dw, db = torch.autograd.grad(h, (gi, w, b), _d(dh))
    return dict(h=h.detach(), dgi=dgi, dw_hh=dw, db_hh=db)


def _run_case(ops, case):
    return _gru(ops, case['gi'], case['w_hh'], case['b_hh'], case['h0_t'], case['dh'])


# ------------------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize('name', GW.NAMES)
def test_gru_seq_at_the_true_width_holds_every_row_and_block_to_fp64(ops, name):
    case, ref = GW.case_and_ref(name)
    H = case['C']
    got, again = _run_case(ops, case), _run_case(ops, case)
    assert got['h'].shape == (case['B'], case['L'], H) and got['dgi'].shape == (case['B'], case['L'], 3 * H)
    assert got['dw_hh'].shape == (3 * H, H) and got['db_hh'].shape == (3 * H,)
    fr, (n, skipped) = GW.fractions(case, got, ref)
    plan = ops.gru_width_plan(H)
    for out, f in fr.items():
        print(f'GRUW-FIG {name} [Hk={plan.Hk} grid={(plan.Hk // 16) * ((case["B"] + 3) // 4)}] {out} {f:.4f} of {GW.bound(out):.0e}')
    over = {out: f for out, f in fr.items() if not f <= 1.0}
    assert not over, over
    assert skipped == 0 and RP.skip_cap_holds(case, n, skipped)
    assert _same(got, again), 'two runs differ'
    if case['h0_t'] is not None:                                # the twin without h0 is another answer in every row
        twin = GW.case_and_ref(name.replace('h0both', 'h0none'))[1]
        assert ((ref['h'] - twin['h']).abs().flatten(1).amax(dim=1) > 1e-2).all()


# ------------------------------------------------------------------------------------------------------ 2. the padding is exact
@pytest.mark.parametrize('H,Hk', [(200, 208), (1, 16), (520, 640)])
def test_padded_width_returns_the_bits_of_the_native_width_on_zero_padded_operands(ops, H, Hk):
    assert ops.gru_width_plan(H) == (Hk, False) and ops.gru_width_plan(Hk) == (Hk, True)
    case = GW.make_case(f'gruw-B3L5H{H}-h0both')
    got = _run_case(ops, case)
    h0k = torch.zeros(case['B'], Hk)
    h0k[:, :H] = case['h0_t']
    dhk = torch.zeros(case['B'], case['L'], Hk)
    dhk[..., :H] = case['dh']
    wide = _gru(ops, GW.pad_gates(case['gi'], H, Hk), GW.pad_gates(case['w_hh'], H, Hk, cols=True), GW.pad_gates(case['b_hh'], H, Hk), h0k, dhk)
    assert not wide['h'][..., H:].any(), 'a padded unit left zero'
    back = dict(h=wide['h'][..., :H], dgi=GW.unpad_gates(wide['dgi'], H, Hk), dw_hh=GW.unpad_gates(wide['dw_hh'], H, Hk, cols=True),
                db_hh=GW.unpad_gates(wide['db_hh'], H, Hk))
    for k in ('h', 'dgi', 'dw_hh', 'db_hh'):
        assert torch.equal(_bits(got[k]), _bits(back[k])), k
    pad_rows = torch.ones(3 * Hk, dtype=torch.bool)
    pad_rows.view(3, Hk)[:, :H] = False
    pad_rows = pad_rows.cuda()
    assert not wide['dgi'][..., pad_rows].any() and not wide['dw_hh'][pad_rows].any() and not wide['db_hh'][pad_rows].any()
    assert not wide['dw_hh'][:, H:].any()


# ------------------------------------------------------------------------------------------------------ 3. gru_seq_multi
@pytest.mark.parametrize('n,B,L,H', [(2, 5, 6, 40), (4, 5, 6, 40), (2, 3, 4, 1024), (4, 8, 3, 1024), (2, 3, 4, 1000)],
                         ids=['n2-H40', 'n4-H40', 'n2-H1024-persistent', 'n4-H1024-per-step', 'n2-H1000'])
def test_gru_seq_multi_equals_gru_seq_of_each_job(ops, n, B, L, H):
    """H = 40 runs on 48.  1024: 2 x 64 workgroups fit the persistent form, 4 x 128 do not (one workgroup per CU at this width)."""
    if H == 1024:
        assert ops.gru_multi_form(n, B, H) == (1 if n == 2 else 0)
    g = torch.Generator().manual_seed(77 + n)
    r = lambda *s: torch.randn(*s, generator=g)
    need = [True, False, True, False][:n]
    raw = [(r(B, L, 3 * H), r(3 * H, H) / H ** 0.5, r(3 * H) / H ** 0.5, r(B, H) if k % 2 == 0 else None, r(B, L, H)) for k in range(n)]

    def leaves(k):
        gi, w, b, h0, _ = raw[k]
        return (_leaf(gi), _leaf(w), _leaf(b), _d(h0)) if need[k] else (_d(gi), _d(w), _d(b), _d(h0))

    jobs = [leaves(k) for k in range(n)]
    ys = ops.gru_seq_multi([j + (need[k],) for k, j in enumerate(jobs)])
    for k in range(n):
        alone = leaves(k)
        y = ops.gru_seq(*alone)
        assert ys[k].shape == (B, L, H) and torch.equal(_bits(ys[k]), _bits(y)), k
        assert ys[k].requires_grad == need[k]
        if need[k]:
            g_multi = torch.autograd.grad(ys[k], jobs[k][:3], _d(raw[k][4]))
            g_alone = torch.autograd.grad(y, alone[:3], _d(raw[k][4]))
            for a, b in zip(g_multi, g_alone):
                assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), k


# ------------------------------------------------------------------------------------------------------ 4. the module
def close(got, ref, rtol=1e-4, atol_scale=2e-5, name=''):
    """tests/test_hip_ops.py `close`."""
    got, ref = got.detach().float().cpu(), ref.detach().float()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    assert err <= rtol * scale + atol_scale * scale, f'{name}: max err {err:.3e} vs scale {scale:.3e}'


def _module(n_in, H, seed):
    from offpolicy_rnn.models.rnn_base import RNNBase
    torch.manual_seed(seed)
    ref = torch.nn.GRU(n_in, H, batch_first=True)
    net = RNNBase(n_in, H, [], ['linear'], ['gru'])
    net.layer_list[0].load_state_dict(ref.state_dict())
    assert {k: tuple(v.shape) for k, v in net.layer_list[0].state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    return net.cuda(), ref.double()


def _steps_equal_the_sequence(net, x, y_seq, H):
    B, L = x.shape[:2]
    with torch.no_grad():
        hid = net.make_init_state(B, x.device)
        ys = []
        for t in range(L):
            y, hid, _ = net.meta_forward(x[:, t:t + 1].contiguous(), hid)
            assert tuple(hid[0].shape) == (1, B, H) and tuple(y.shape) == (B, 1, H)
            ys.append(y)
    np.testing.assert_allclose(torch.cat(ys, dim=1).cpu().numpy(), y_seq.detach().cpu().numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(hid[0][0].cpu().numpy(), y_seq[:, -1].detach().cpu().numpy(), rtol=1e-4, atol=2e-5)


def test_module_at_width_24_matches_torch_gru_in_fp64(ops):
    B, L, n_in, H = 5, 12, 32, 24
    net, ref = _module(n_in, H, 11)
    g = torch.Generator().manual_seed(12)
    x0, w = torch.randn(B, L, n_in, generator=g), torch.randn(B, L, H, generator=g)
    x = x0.cuda().requires_grad_(True)
    y, state, _ = net.meta_forward(x, net.make_init_state(B, x.device))
    assert tuple(y.shape) == (B, L, H) and tuple(state[0].shape) == (1, B, H)
    (y * w.cuda()).sum().backward()
    xr = x0.double().requires_grad_(True)
    yr, hr = ref(xr)
    (yr * w.double()).sum().backward()
    np.testing.assert_allclose(y.detach().cpu().numpy(), yr.detach().float().numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(state[0].detach().cpu().numpy(), hr.detach().float().numpy(), rtol=1e-4, atol=2e-5)
    close(x.grad, xr.grad, 2e-4, 5e-5, 'dx')
    params, ref_params = dict(net.layer_list[0].named_parameters()), dict(ref.named_parameters())
    assert set(params) == set(ref_params)
    for k, p in params.items():
        assert p.grad is not None and p.grad.shape == p.shape == ref_params[k].shape, k
        close(p.grad, ref_params[k].grad, 2e-4, 5e-5, k)
    _steps_equal_the_sequence(net, x.detach(), y, H)


def test_module_steps_at_width_520_equal_the_sequence(ops):
    B, L, n_in, H = 3, 12, 32, 520
    net, ref = _module(n_in, H, 13)
    x0 = torch.randn(B, L, n_in, generator=torch.Generator().manual_seed(14))
    with torch.no_grad():
        y, state, _ = net.meta_forward(x0.cuda(), net.make_init_state(B, 'cuda'))
        yr, _ = ref(x0.double())
    assert tuple(y.shape) == (B, L, H) and tuple(state[0].shape) == (1, B, H)
    np.testing.assert_allclose(y.cpu().numpy(), yr.float().numpy(), rtol=1e-4, atol=2e-5)
    _steps_equal_the_sequence(net, x0.cuda(), y, H)


def test_width_outside_the_range_raises_at_the_first_gpu_forward(ops):
    from offpolicy_rnn.models.gru import GRU
    layer = GRU(4, 1025).cuda()
    with pytest.raises(ValueError, match='1 to 1024'):
        layer(torch.zeros(2, 3, 4, device='cuda'))
    with pytest.raises(ValueError, match='1 to 1024'):
        ops.gru_seq(torch.zeros(2, 3, 3 * 1025, device='cuda'), torch.zeros(3 * 1025, 1025, device='cuda'), torch.zeros(3 * 1025, device='cuda'))


# ------------------------------------------------------------------------------------------------------ 5. the trainer
WIDE = dict(policy_embedding_hidden_size=[32, 24], value_embedding_hidden_size=[32, 40])


def _small(algo='sac', per=1, **extra):
    from test_gru_graph_gpu import _small as small
    alg = small(algo, per, **dict(WIDE, **extra))
    widths = lambda model: [layer.hidden_size for kind, layer in model.embedding_network.sequence_layers()]
    assert widths(alg.policy) == [24] and widths(alg.values[0]) == [40] and widths(alg.target_values[0]) == [40]
    return alg


def _updates(alg, n, step=None):
    logs = []
    for _ in range(n):
        logs.append(dict((step or alg.train_one_batch)()))
        alg.grad_num += 1
    torch.cuda.synchronize()
    return logs


def test_trainer_batched_update_equals_the_serial_form_bit_for_bit(ops, monkeypatch):
    from test_gru_graph_gpu import _state, _val
    runs = []
    for batched in (True, False):
        monkeypatch.setenv('RESEL_GRU_BATCH', '1' if batched else '0')
        alg = _small('sac', 2, seed=5)
        assert alg.gru_batch == batched
        torch.manual_seed(200)
        np.random.seed(200)
        runs.append((_updates(alg, 4), _state(alg)))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert set(a) == set(b)
        for k in b:
            assert _val(a[k]) == _val(b[k]), (k, _val(a[k]), _val(b[k]))
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), runs[0][1], runs[1][1]):
        assert torch.equal(a, b), (nm, (a - b).abs().max().item())


@pytest.mark.parametrize('batched', [True, False], ids=['batched', 'serial'])
def test_trainer_graph_replay_equals_the_eager_update(ops, batched, monkeypatch):
    """tests/test_gru_graph_gpu.py `_graphed_against_eager`, its tolerances (rtol 2e-5, atol 2e-7), at widths 24 and 40."""
    from test_gru_graph_gpu import _quiet, _state, _val
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    _quiet(monkeypatch)
    monkeypatch.setenv('RESEL_GRU_BATCH', '1' if batched else '0')
    n_upd = 4
    eager = _small('sac')
    logs_e = _updates(eager, n_upd)
    graphed = _small('sac')
    assert graphed.gru_batch == batched and GraphedUpdate.refusal(graphed) is None
    g = GraphedUpdate(graphed, warmup=1, max_graphs=4)
    logs_g = _updates(graphed, n_upd, g.step)
    assert g.graph is not None and len(g.graphs) >= 1 and 1 <= g.eager_fallbacks <= 3
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), _state(graphed), _state(eager)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=2e-7, err_msg=nm)
    for le, lg in zip(logs_e, logs_g):
        assert set(le) == set(lg)
        for k in le:
            ve, vg = _val(le[k]), _val(lg[k])
            assert abs(ve - vg) <= 2e-5 * max(1.0, abs(ve)), (k, ve, vg)
    g.close()


def test_trainer_model_files_round_trip_at_the_true_width(ops, tmp_path, monkeypatch):
    from test_gru_graph_gpu import _state
    writer = _small('sac', seed=3)
    _updates(writer, 2)
    want = lambda H: sorted([(3 * H, 32), (3 * H, H), (3 * H,), (3 * H,)])
    for model, H in ((writer.policy, 24), (writer.values[0], 40)):                # `state_dict()` is {module: {key: tensor}}
        shapes = [tuple(v.shape) for sd in model.state_dict().values() for k, v in sd.items() if k.endswith('_l0')]
        assert sorted(shapes) == want(H), shapes
    writer.save(str(tmp_path / 'model'))
    files = {f: torch.load(str(tmp_path / 'model' / f), map_location='cpu') for f in sorted(os.listdir(tmp_path / 'model')) if f != 'log_sac_alpha.pt'}
    shapes = [tuple(v.shape) for sd in files.values() for k, v in sd.items() if k.endswith('_l0')]      # policy, value, target value
    assert sorted(shapes) == sorted(want(24) + 2 * want(40)), shapes
    reader = _small('sac', seed=4)
    assert not torch.equal(reader.policy.store.flat, writer.policy.store.flat)
    reader.load(str(tmp_path / 'model'))
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), _state(reader), _state(writer)):
        assert torch.equal(a, b), nm


def test_trainer_run_state_round_trip_continues_bit_for_bit(ops, tmp_path, monkeypatch):
    """RESEL_GRAPH_UPDATE=0: two iterations of `train()` on the T-Maze (the open episode's recurrent state is [1, 1, 24]), a state, three
    more eager updates; a fresh trainer that loads the state is the writer (tests/test_run_state_host.py `snapshot`) and its three
    updates end in the writer's bits."""
    from test_gru_graph_gpu import _state
    from test_run_state_gpu import TMAZE, _trainer
    from test_run_state_host import assert_same, snapshot
    kw = dict(rnn='gru', env=TMAZE, graph_update='0', total_iteration=2, **WIDE)
    writer = _trainer(monkeypatch, tmp_path, **kw)
    writer.train()
    want = snapshot(writer)
    path = writer.save_state(str(tmp_path / 'states' / 'one'))
    hidden = writer.graph_step._hidden if writer.graph_step is not None else writer.sample_hidden
    assert [tuple(h.shape) for h in hidden._data if torch.is_tensor(h)][:1] == [(1, 1, 24)]
    assert want['counts'][1] > 0, 'no update ran'
    _updates(writer, 3)
    end = _state(writer)
    reader = _trainer(monkeypatch, tmp_path, **kw)
    reader.load_state(path)
    assert_same(snapshot(reader), want, 'gru 24 / 40 run state')
    _updates(reader, 3)
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), _state(reader), end):
        assert torch.equal(a, b), (nm, (a - b).abs().max().item())


# ------------------------------------------------------------------------------------------------------ 6. native widths
@pytest.mark.parametrize('H', [32, 512])
def test_native_widths_never_reach_the_pad_entries(ops, H, monkeypatch):
    from offpolicy_rnn.models.rnn_base import RNNBase
    real, calls = ops.lib(), []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if 'pad' not in name:
                return fn

            def counted(*a):
                calls.append(name)
                return fn(*a)
            return counted

    monkeypatch.setattr(ops, 'lib', lambda: Counting())
    torch.manual_seed(H)
    net = RNNBase(32, H, [], ['linear'], ['gru']).cuda()
    x = torch.randn(3, 5, 32, device='cuda', requires_grad=True)
    y, state, _ = net.meta_forward(x, net.make_init_state(3, x.device))
    y.sum().backward()
    gi = torch.randn(3, 5, 3 * H, device='cuda')
    w, b = torch.randn(3 * H, H, device='cuda') / H ** 0.5, torch.zeros(3 * H, device='cuda')
    ops.gru_seq(gi, w, b)
    ops.gru_seq_multi([(gi, w, b, None, False), (gi, w, b, None, False)])
    torch.cuda.synchronize()
    assert calls == []
    net24 = RNNBase(32, H - 8, [], ['linear'], ['gru']).cuda()               # the counter sees a padded width
    y, _, _ = net24.meta_forward(x, net24.make_init_state(3, x.device))
    y.sum().backward()
    torch.cuda.synchronize()
    assert sorted(calls) == ['resel_gru_pad_params', 'resel_gru_pad_rows', 'resel_gru_pad_rows', 'resel_gru_unpad_params', 'resel_gru_unpad_rows'], calls
