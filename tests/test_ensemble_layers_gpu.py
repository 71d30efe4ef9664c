"""The ensemble sequence layers `elru-<E>` / `econv1d[_<K>]-<E>` on the GPU: their three member kernels against fp64 models written here,
the layers against the reference's recordings (tests/golden/ensemble_layers.npz), the trainers against its three recorded runs, and
update graphs / persistence.  Shapes are the smallest at which each kernel can still go wrong (rows that map to members other than by
identity, 64-step blocks crossed, partly filled channel blocks, every tap padding, the 2048-float token limit).

Bars, none of them set here: the complex scan those of tests/recurrence_parity.py (per row and 64-step block, per-member parameter
gradients against the sum of the magnitudes they are formed from); the convolution those of tests/test_mixer_kernels_gpu.py
(`close_fwd`, `close(2e-4, 5e-5)`); the add + LayerNorm rtol 1e-4 / atol 2e-5 (tests/test_norm_blocks_gpu.py); layers 1e-4 / 2e-5
forward and 2e-3 / 3e-4 gradients (tests/test_sscan_states_gpu.py); trainers 2e-3 / 2e-5 parameters and 2e-3 / 5e-4 logs
(tests/test_trainer_gpu.py); replayed against eager 2e-5 / 2e-7 (tests/test_update_published_width_gpu.py).
Every comparison of a kernel prints `ENS-FIG ...` with its error as a fraction of the bound before anything is asserted (`pytest -s`)."""
import json
import os

import numpy as np
import pytest
import torch

import recurrence_parity as RP
from conftest import GOLDEN, load_golden, nested
from test_ensemble_layers_host import check_layer, load_layer
from test_host_logic import _push, _synth, make_parameter
from test_mixer_kernels_gpu import _fraction, close, close_fwd

pytestmark = pytest.mark.gpu
META = json.load(open(os.path.join(GOLDEN, 'train_ensemble_meta.json')))


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _leaf(t):
    return t.detach().clone().cuda().requires_grad_(True)


# ------------------------------------------------------------------------------------------------ member complex scan
def _scan_cases(E, B, L, C, with_h0, seed):
    """One lru case of tests/recurrence_parity.py per member (its own operands, lambda, gamma, carried-in state and upstream gradient)
    around ONE start table: row 0 carries its state in, row 1 starts with a reset, one start inside each row, random ones at 3 %."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    start = RP.make_start(B, L, g, 0.03)
    if L > 2:
        start[0, L // 2] = 1
        start[1, (2 * L) // 3] = 1
    cases = []
    for e in range(E):
        mag, th = 0.9 + 0.099 * torch.rand(C, generator=g), 6.28 * torch.rand(C, generator=g)
        cases.append(dict(name=f'member{e}-E{E}B{B}L{L}C{C}', kind='lru', B=B, L=L, C=C, start=start, vr=r(B, L, C), vi=r(B, L, C),
                          lam_re=mag * torch.cos(th), lam_im=mag * torch.sin(th), gamma=torch.sqrt(1 - mag ** 2), dhr=r(B, L, C), dhi=r(B, L, C),
                          h0r=2 * r(B, C) if with_h0 else None, h0i=2 * r(B, C) if with_h0 else None, skip=r(B, L, C), dskip=r(B, L, C)))
    return cases


def _run_member_scan(ops, cases):
    st = lambda k: torch.stack([c[k] for c in cases])
    u = _leaf(torch.stack((st('vr'), st('vi'), st('skip'))))                                   # [3, E, B, L, C]
    lam3 = _leaf(torch.stack((st('lam_re'), st('lam_im'), st('gamma'))))                       # [3, E, C]
    h0r, h0i = (None, None) if cases[0]['h0r'] is None else (st('h0r').cuda(), st('h0i').cuda())
    h2, u2 = ops.complex_scan_ensemble(u, lam3, cases[0]['start'].cuda(), h0r, h0i)
    du, dlam3 = torch.autograd.grad((h2, u2), (u, lam3), (torch.stack((st('dhr'), st('dhi'))).cuda(), st('dskip').cuda()))
    return dict(h2=h2.detach(), u2=u2.detach(), du=du, dlam3=dlam3, u=u.detach())


@pytest.mark.parametrize('with_h0', [True, False], ids=['h0', 'h0-None'])
@pytest.mark.parametrize('C', [4, 20, 68])
@pytest.mark.parametrize('L', [1, 65, 130])
def test_member_scan_holds_every_member_row_and_block_to_fp64(ops, L, C, with_h0):
    E, B = 3, 2                                                      # rows 0 .. 5 -> members 0, 0, 1, 1, 2, 2: not the identity
    cases = _scan_cases(E, B, L, C, with_h0, seed=3500 + 10 * L + C)
    out, again = _run_member_scan(ops, cases), _run_member_scan(ops, cases)
    over = {}
    for e, case in enumerate(cases):
        ref = RP.reference(case)
        got = dict(hr=out['h2'][0, e], hi=out['h2'][1, e], dvr=out['du'][0, e], dvi=out['du'][1, e],
                   dlam_re=out['dlam3'][0, e], dlam_im=out['dlam3'][1, e], dgamma=out['dlam3'][2, e])
        fr, _ = RP.fractions(case, got, ref)
        for k, f in fr.items():
            print(f'ENS-FIG scan E{E}B{B}L{L}C{C} h0={with_h0} member {e} {k} {f:.4f} of {RP.bound("lru", k):.0e}')
        over.update({(e, k): f for k, f in fr.items() if not f <= 1.0})
    assert torch.equal(out['u2'], out['u'][2]) and torch.equal(out['du'][2], torch.stack([c['dskip'] for c in cases]).cuda()), 'the pass-through member'
    assert not over, over
    assert all(torch.equal(_bits(out[k]), _bits(again[k])) for k in ('h2', 'du', 'dlam3')), 'two runs differ'


@pytest.mark.parametrize('L,C', [(65, 20), (130, 68), (1, 4)])
def test_member_scan_with_one_member_is_the_single_member_entry(ops, L, C):
    (case,) = _scan_cases(1, 4, L, C, True, seed=3600 + L)
    out = _run_member_scan(ops, [case])
    ls = [_leaf(case[k]) for k in ('vr', 'vi', 'lam_re', 'lam_im', 'gamma')]
    hr, hi = ops.complex_scan(*ls, case['start'].cuda(), case['h0r'].cuda(), case['h0i'].cuda())
    gs = torch.autograd.grad((hr, hi), ls, (case['dhr'].cuda(), case['dhi'].cuda()))
    pairs = [(out['h2'][0, 0], hr), (out['h2'][1, 0], hi), (out['du'][0, 0], gs[0]), (out['du'][1, 0], gs[1]),
             (out['dlam3'][0, 0], gs[2]), (out['dlam3'][1, 0], gs[3]), (out['dlam3'][2, 0], gs[4])]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in pairs)


# ------------------------------------------------------------------------------------------------ member convolution
def _conv_model(x, w, b, mask):
    """fp64: y[e, r, t, d] = b[e, d] + sum_k w[e, d, k] (mask x)[e, r, t - (K - 1) + k, d], zeros in front of the row; x shared or per member."""
    E, D, K = w.shape
    xm = x * mask[..., None]
    if xm.dim() == 3:
        xm = xm.unsqueeze(0).expand(E, *xm.shape)
    xp = torch.cat((xm.new_zeros(E, xm.shape[1], K - 1, D), xm), dim=2)
    win = xp.unfold(2, K, 1)                                         # [E, B, L, D, K]
    return (win * w[:, None, None]).sum(-1) + b[:, None, None]


@pytest.mark.parametrize('shared', [False, True], ids=['member-major', 'shared'])
@pytest.mark.parametrize('K', [1, 3, 8, 16, 17])
@pytest.mark.parametrize('D', [8, 36])
@pytest.mark.parametrize('L', [5, 70])
def test_member_conv_against_fp64(ops, L, D, K, shared):
    E, B = 3, 2
    g = torch.Generator().manual_seed(4000 + 100 * L + 10 * D + K + int(shared))
    r = lambda *s: torch.randn(*s, generator=g)
    x, w, b, dy = r(*((B, L, D) if shared else (E, B, L, D))), r(E, D, K) / max(1.0, K ** 0.5), r(E, D), r(E, B, L, D)
    mask = torch.ones(B, L)
    mask[0, L // 2] = 0                                              # a zero in mid-row
    mask[1, L - 1] = 0
    ins64 = [t.double().requires_grad_(True) for t in (x, w, b)]
    ref = _conv_model(ins64[0], ins64[1], ins64[2], mask.double())
    ref_g = torch.autograd.grad(ref, ins64, dy.double())
    ins = [_leaf(t) for t in (x, w, b)]
    runs = []
    for _ in range(2):
        y = ops.member_conv1d(ins[0], ins[1], ins[2], mask.cuda())
        runs.append((y.detach(),) + torch.autograd.grad(y, ins, dy.cuda()))
    tag = f'conv E{E}B{B}L{L}D{D}K{K} {"shared" if shared else "member-major"}'
    print(f'ENS-FIG {tag} y {_fraction(runs[0][0], ref.detach(), 1e-4, 2e-5, fwd=True):.4f}')
    for nm, got, want in zip(('dx', 'dw', 'db'), runs[0][1:], ref_g):
        print(f'ENS-FIG {tag} {nm} {_fraction(got, want, 2e-4, 5e-5):.4f}')
    assert tuple(runs[0][1].shape) == tuple(x.shape)                 # shared: ONE gradient, the sum over the members
    close_fwd(runs[0][0], ref.detach(), name=f'{tag} y')
    for nm, got, want in zip(('dx', 'dw', 'db'), runs[0][1:], ref_g):
        close(got, want, rtol=2e-4, atol_scale=5e-5, name=f'{tag} {nm}')
    assert all(torch.equal(_bits(a), _bits(c)) for a, c in zip(*runs)), 'two runs differ'


@pytest.mark.parametrize('L,K', [(70, 3), (5, 8), (70, 17)])
def test_member_conv_with_one_member_is_causal_conv1d_fn(ops, L, K):
    B, D = 4, 36
    g = torch.Generator().manual_seed(4100 + L + K)
    x, w, b, dy = (torch.randn(*s, generator=g) for s in ((B, L, D), (D, K), (D,), (B, L, D)))
    mask = (torch.rand(B, L, generator=g) > 0.1).float()
    one = [_leaf(t) for t in (x, w, b)]
    y1 = ops.causal_conv1d_fn(one[0], one[1], one[2], mask.cuda(), False)
    g1 = torch.autograd.grad(y1, one, dy.cuda())
    mem = [_leaf(x[None]), _leaf(w[None]), _leaf(b[None])]
    y2 = ops.member_conv1d(mem[0], mem[1], mem[2], mask.cuda())
    g2 = torch.autograd.grad(y2, mem, dy[None].cuda())
    assert torch.equal(_bits(y1), _bits(y2[0])) and all(torch.equal(_bits(a), _bits(c[0])) for a, c in zip(g1, g2))


# ------------------------------------------------------------------------------------------------ add + joint member LayerNorm
def _add_norm_model(a, r, w, b, elu):
    """fp64: one LayerNorm over all E x C features of a token of a + r (member-major [E, M, C]), then the optional ELU."""
    s = (a + r).transpose(0, 1)                                      # [M, E, C]
    mean, var = s.mean(dim=(1, 2), keepdim=True), s.var(dim=(1, 2), unbiased=False, keepdim=True)
    y = ((s - mean) / torch.sqrt(var + 1e-5) * w + b).transpose(0, 1)
    return torch.nn.functional.elu(y) if elu else y


@pytest.mark.parametrize('elu', [False, True], ids=['plain', 'elu'])
@pytest.mark.parametrize('M', [5, 130])
@pytest.mark.parametrize('E,C', [(1, 8), (3, 20), (8, 256)])
def test_member_add_layer_norm_against_fp64(ops, E, C, M, elu):
    g = torch.Generator().manual_seed(4200 + E * C + M)
    r_ = lambda *s: torch.randn(*s, generator=g)
    a, r, w, b, dy = r_(E, M, C), 2 * r_(E, M, C) + 0.5, 1 + 0.2 * r_(E, C), 0.3 * r_(E, C), r_(E, M, C)
    ins64 = [t.double().requires_grad_(True) for t in (a, r, w, b)]
    ref = _add_norm_model(*ins64, elu)
    ref_g = torch.autograd.grad(ref, ins64, dy.double())
    ins = [_leaf(t) for t in (a, r, w, b)]
    y = ops.member_add_layer_norm(ins[0], ins[1], ins[2], ins[3], 1e-5, 'elu' if elu else None)
    gs = torch.autograd.grad(y, ins, dy.cuda())
    names = ('y', 'da', 'dr', 'dw', 'db')
    for nm, got, want in zip(names, (y,) + gs, (ref,) + ref_g):
        err = (got.detach().cpu().double() - want.detach()).abs()
        print(f'ENS-FIG addnorm E{E}C{C}M{M} elu={elu} {nm} {(err / (2e-5 + 1e-4 * want.detach().abs())).max().item():.4f}')
    for nm, got, want in zip(names, (y,) + gs, (ref,) + ref_g):
        np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().numpy(), rtol=1e-4, atol=2e-5, err_msg=nm)
    # the magnitude bound published for the GEMM behind it holds
    h = ops.amax_of(y)
    assert h is None or ops.amax_value(h) >= y.abs().max().item()
    # the same numbers as the norm without a residual on the sum formed beforehand, bit for bit: that entry did not change
    two = [_leaf(t) for t in (a, r, w, b)]
    y2 = ops.member_layer_norm(two[0] + two[1], two[2], two[3], 1e-5, 'elu' if elu else None)
    g2 = torch.autograd.grad(y2, two, dy.cuda())
    assert torch.equal(_bits(y), _bits(y2)) and all(torch.equal(_bits(p), _bits(q)) for p, q in zip(gs, g2))


def test_a_token_the_norm_kernels_refuse_keeps_the_torch_spelling_and_says_so_once(ops, monkeypatch, capsys):
    """(E, C) = (10, 256) is 2560 floats, above the 2048 the kernels take."""
    from offpolicy_rnn.models.gilr.gilr import EnsemblePositionWiseFeedForward
    assert not ops.member_layer_norm_ok(10, 256) and ops.member_layer_norm_ok(8, 256)
    torch.manual_seed(0)
    ff = EnsemblePositionWiseFeedForward(256, 10, 0.0).cuda()
    x = torch.randn(10, 2, 5, 256, device='cuda')
    monkeypatch.setenv('RESEL_MEMBER_SEQ', '1')
    capsys.readouterr()
    y1, y1b = ff(x), ff(x)
    said = capsys.readouterr().out
    monkeypatch.setenv('RESEL_MEMBER_SEQ', '0')
    y0 = ff(x)
    assert said.count('WARNING') == 1 and '10 x 256' in said and capsys.readouterr().out == ''
    assert torch.equal(y1, y0) and torch.equal(y1, y1b)
    want = _add_norm_model(ff.w_2(torch.nn.functional.gelu(ff.w_1(x))).double().cpu().reshape(10, 10, 256), x.double().cpu().reshape(10, 10, 256),
                           ff.layer_norm.weight.double().cpu(), ff.layer_norm.bias.double().cpu(), False)
    np.testing.assert_allclose(y1.detach().cpu().numpy().reshape(10, 10, 256), want.detach().numpy(), rtol=1e-4, atol=2e-5)


# ------------------------------------------------------------------------------------------------ layers against the reference
@pytest.mark.parametrize('switch', ['1', '0'])
@pytest.mark.parametrize('form', ['m', 's'])
@pytest.mark.parametrize('lid', ['elru-3', 'econv1d_3-3'])
def test_layer_equals_the_reference(ops, lid, form, switch, monkeypatch):
    """Member-major and shared input, a live carried-in state, a start flag inside a row, a masked token; both forms of the switch."""
    monkeypatch.setenv('RESEL_MEMBER_SEQ', switch)
    check_layer(*load_layer(lid, form, 'cuda'), out_tol=(1e-4, 2e-5), grad_tol=(2e-3, 3e-4))


# ------------------------------------------------------------------------------------------------ trainers
@pytest.fixture
def cpu_noise(monkeypatch):
    """The product's Gaussian draws come from the CPU generator, like the reference's (the autouse fixture of test_trainer_gpu.py)."""
    from offpolicy_rnn.utility import rng
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.randn(tuple(shape), dtype=dtype).to(device))


def _fixture_trainer(name):
    from offpolicy_rnn import alg_init
    m = META[name]
    g = load_golden(f'train_{name}.npz')
    alg = alg_init(make_parameter('gilr', D=m['D'], algo=m['algo'], sac_batch_size=m['sac_batch_size'], redq_m=m['redq_m'],
                                  value_embedding_layer_type=['efc-4', m['rnn'], 'efc-4'], value_layer_type=['efc-4'] * 3))
    assert alg.device.type == 'cuda'
    alg.policy.load_state_dict(nested(g, 'policy0|'))
    alg.values[0].load_state_dict(nested(g, 'value0|'))
    alg._value_update(tau=0.0)
    rs = np.random.RandomState(m['ring_seed'])
    for n in m['lens']:
        o, a, r = _synth(rs, n, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=(n != 12))
    return alg, g, m


@pytest.mark.parametrize('switch', ['1', '0'])
@pytest.mark.parametrize('name', list(META))
def test_three_updates_equal_the_reference(ops, name, switch, cpu_noise, monkeypatch):
    """Every logged scalar of three updates and every element of every parameter behind them; none is excluded."""
    monkeypatch.setenv('RESEL_MEMBER_SEQ', switch)
    alg, g, m = _fixture_trainer(name)
    assert alg._get_skip_len() == m['skip_len'] and bool(alg.allow_nest_stack) == m['nest']
    torch.manual_seed(200)
    np.random.seed(200)
    for it in range(3):
        log = alg.train_one_batch()
        alg.grad_num += 1
        for k, v in m['logs'][it].items():
            got = log[k][0] if isinstance(log[k], tuple) else log[k]
            print(f'ENS-FIG train {name} switch {switch} update {it} {k} got {got:.7g} want {v:.7g}')
            assert got == pytest.approx(v, rel=2e-3, abs=5e-4), (it, k, got, v)
    for pre, net in (('policy3|', alg.policy), ('value3|', alg.values[0]), ('target3|', alg.target_values[0])):
        sd = net.state_dict()
        for mod, d in nested(g, pre).items():
            for k, v in d.items():
                np.testing.assert_allclose(sd[mod][k].detach().cpu(), v, rtol=2e-3, atol=2e-5, err_msg=f'{pre}{mod}.{k}')
    np.testing.assert_allclose(alg.log_sac_alpha.detach().cpu(), g['log_alpha3'], rtol=2e-3, atol=2e-5)


# ------------------------------------------------------------------------------------------------ graphs and persistence
ROWS, STEPS = 4, 16


def _small_trainer(seed=0, lid='elru-4'):
    from offpolicy_rnn import alg_init
    torch.manual_seed(seed)
    np.random.seed(seed)
    alg = alg_init(make_parameter('gilr', D=32, env=f'synthetic-o5-a3-T{STEPS}', sac_batch_size=ROWS * STEPS - 1, redq_m=2, cuda_inference=True,
                                  value_embedding_layer_type=['efc-4', lid, 'efc-4'], value_layer_type=['efc-4'] * 3,
                                  max_buffer_transition_num=4 * ROWS * STEPS))
    rs = np.random.RandomState(seed)
    for _ in range(2 * ROWS):
        o, a, r = _synth(rs, STEPS, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=False)
    np.random.seed(11)
    return alg


def _state(alg):
    return [alg.policy.store.flat.detach().clone(), alg.values[0].store.flat.detach().clone(),
            alg.target_values[0].store.flat.detach().clone(), alg.log_sac_alpha.detach().clone()]


def test_replayed_update_equals_the_eager_update(ops, monkeypatch):
    """elru-4 at 4 rows x 16 steps: one eager, one recorded and two replayed updates against four eager ones."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    from offpolicy_rnn.utility import rng
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.zeros(tuple(shape), dtype=dtype, device=device))
    n_upd = 4
    eager = _small_trainer()
    assert GraphedUpdate.refusal(eager) is None
    logs_e = []
    for _ in range(n_upd):
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    graphed = _small_trainer()
    gu = GraphedUpdate(graphed, warmup=1)
    try:
        logs_g = []
        for _ in range(n_upd):
            logs_g.append(dict(gu.step()))
            graphed.grad_num += 1
        torch.cuda.synchronize()
        assert len(gu.graphs) == 1
        for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), _state(graphed), _state(eager)):
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=2e-7, err_msg=nm)
        val = lambda v: v[0] if isinstance(v, tuple) else v
        for le, lg in zip(logs_e, logs_g):
            assert set(le) == set(lg)
            for k in le:
                assert abs(val(le[k]) - val(lg[k])) <= 2e-5 * max(1.0, abs(val(le[k]))), (k, le[k], lg[k])
    finally:
        gu.close()


@pytest.mark.parametrize('lid', ['elru-4', 'econv1d_3-4'])
def test_save_then_load_round_trips_bit_for_bit(ops, lid, tmp_path):
    alg = _small_trainer(lid=lid)
    alg.train_one_batch()
    want = _state(alg)
    alg.save(str(tmp_path))
    files = set(os.listdir(tmp_path))
    assert {'ContextualSACValue-0-embedding_model.pt', 'ContextualSACValue-0-target-embedding_model.pt'} <= files
    sd = torch.load(tmp_path / 'ContextualSACValue-0-embedding_model.pt', map_location='cpu')
    assert any(k.startswith('layer_list.1.') for k in sd)
    other = _small_trainer(seed=3, lid=lid)
    assert not torch.equal(other.values[0].store.flat, want[1])
    other.load(str(tmp_path))
    for a, b in zip(_state(other), want):
        assert torch.equal(a, b)


def test_a_loaded_run_state_continues_the_eager_run_bit_for_bit(ops, tmp_path):
    a = _small_trainer()
    for _ in range(2):
        a.train_one_batch()
        a.grad_num += 1
    path = a.save_state(str(tmp_path / 'state'))
    logs = []
    for _ in range(2):
        logs.append(a.train_one_batch()['critic_loss'])
        a.grad_num += 1
    b = _small_trainer(seed=5)
    b.load_state(path)                                               # (the random streams are the process's: restored here, behind a's updates)
    for _ in range(2):
        logs.append(b.train_one_batch()['critic_loss'])
        b.grad_num += 1
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert logs[:2] == logs[2:]
