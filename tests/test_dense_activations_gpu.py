"""relu, leaky_relu, tanh and sigmoid behind the `fc` / `efc-<E>` layers in HIP: activation codes 6 .. 9 of `resel_bias_act_fwd` / `_bwd`
and of every plain epilogue of `resel_gemm_f32x`, the autograd nodes that carry them, the routing of `RNNBase._dense_step` under
RESEL_ACT_FUSED and whole updates against the fp64 oracle trainer.

Every reference is fp64 on the CPU, computed from the inputs and never from a kernel.  `close` / `close_fwd` and their bounds are
restated from tests/test_hip_ops.py; the GEMM bar (rtol 1e-5, atol_scale 1e-6) is `test_gemm_f32_vs_fp64_product`'s, the autograd-node
bar (rtol 2e-4, atol_scale 5e-5) `test_ensemble_mlp_fused_tail_vs_torch`'s.  The GEMM shapes are one per epilogue site, derived from
`gemm_route` (csrc/gemm_f32.hip) and `make_plan` (csrc/gemm_splitk.h) as they stand: re-derive them if the routing changes.

The kernels' tanh is (1 - e) / (1 + e) with e = exp2(-2 log2(e) |v|) on v_exp_f32 / v_rcp_f32 (1 ulp each): an absolute error of about
2e-7, against |tanh| <= 1 well inside the 1.1e-5 of the GEMM bar; below |v| = 0.02 the series v - v^3 / 3 keeps the relative error
(next term 2.2e-8).  sigmoid is 1 / (1 + exp(-v)) on the same two instructions."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import update_parity as UP
from test_dense_activations_host import (ACT, D, DATA_SEED, INIT_SEED, OBS, ROWS, STEPS, UPDATE_CASES, UPDATE_SEED, update_overrides)

pytestmark = pytest.mark.gpu

ACTS = ['relu', 'leaky_relu', 'tanh', 'sigmoid']
TORCH64 = {'relu': F.relu, 'leaky_relu': lambda v: F.leaky_relu(v, 0.01), 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}
TORCH32 = {'relu': F.relu, 'leaky_relu': F.leaky_relu}            # the two whose fp32 result is one correctly rounded operation: torch's bits


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


@pytest.fixture(autouse=True)
def switch_unset(monkeypatch):
    monkeypatch.delenv('RESEL_ACT_FUSED', raising=False)


def close(got, ref, rtol=1e-4, atol_scale=2e-5, name=''):
    got = got.detach().float().cpu()
    ref = ref.detach().float()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    assert err <= rtol * scale + atol_scale * scale, f'{name}: max err {err:.3e} vs scale {scale:.3e}'


def close_fwd(got, ref, rtol=1e-4, floor=1e-5, name=''):
    close(got, ref, rtol=rtol, name=name)
    got = got.detach().float().cpu()
    ref = ref.detach().float()
    bound = rtol * ref.abs() + floor * max(ref.abs().max().item(), 1e-6)
    worst = ((got - ref).abs() / bound).max().item()
    assert worst <= 1.0, f'{name}: worst element at {worst:.2f}x its element-wise bound (rtol {rtol}, floor {floor})'


def rnd(*shape, g=None, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------ 1. bias_act_ / bias_act_bwd
def _bias_act_ref(y, bias, go, nseg, act):
    C = y.shape[1]
    yr, br = y.double().requires_grad_(True), bias.double().requires_grad_(True)
    ref = TORCH64[act](yr.view(nseg, -1, C) + br.view(nseg, 1, C)).reshape(-1, C)
    ref.backward(go.double())
    return ref.detach(), yr.grad, br.grad


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('rows,C,nseg', [(7, 8, 1), (6 * 37, 12, 6), (2 * 513, 260, 2), (300, 64, 1)])
def test_bias_act_fwd_bwd(ops, rows, C, nseg, act):
    g = torch.Generator().manual_seed(5)
    y, bias, go = rnd(rows, C, g=g, scale=2.0), rnd(nseg, C, g=g), rnd(rows, C, g=g)
    ref, gy_ref, db_ref = _bias_act_ref(y, bias, go, nseg, act)
    a = ops.bias_act_(y.cuda(), bias.cuda(), rows // nseg, act)
    close_fwd(a, ref, name='act(y + b)')
    if act in TORCH32:
        want = TORCH32[act]((y.cuda().view(nseg, -1, C) + bias.cuda().view(nseg, 1, C))).reshape(rows, C)
        assert torch.equal(a, want), 'not torch\'s fp32 bits'
    gy, db = ops.bias_act_bwd(go.cuda(), a, rows // nseg, act, True)
    close(gy, gy_ref, name='gy')
    close(db, db_ref, rtol=2e-4, atol_scale=5e-5, name='dbias')


@pytest.mark.parametrize('act', ACTS)
def test_bias_act_bwd_reads_column_blocks_in_place(ops, act):
    """g and a as column blocks of wider tensors (row stride > C), as the halves of a `cat` backward and a row buffer hand them over."""
    rows, C, nseg = 2 * 130, 24, 2
    g = torch.Generator().manual_seed(6)
    y, bias, go = rnd(rows, C, g=g, scale=2.0), rnd(nseg, C, g=g), rnd(rows, C, g=g)
    ref, gy_ref, db_ref = _bias_act_ref(y, bias, go, nseg, act)
    a = ops.bias_act_(y.cuda(), bias.cuda(), rows // nseg, act)
    wide_g = torch.full((rows, C + 16), float('nan'), device='cuda')
    wide_a = torch.full((rows, 8 + C + 4), float('nan'), device='cuda')
    wide_g[:, 16:] = go.cuda()
    wide_a[:, 8:8 + C] = a
    gv, av = wide_g[:, 16:], wide_a[:, 8:8 + C]
    # what `ops.bias_act_bwd` hands on as it is: unit column stride, rows of whole float4s on 16-byte boundaries
    assert gv.stride(0) == C + 16 and av.stride(0) == C + 12 and gv.data_ptr() % 16 == 0 and av.data_ptr() % 16 == 0
    gy, db = ops.bias_act_bwd(gv, av, rows // nseg, act, True)
    close(gy, gy_ref, name='gy')
    close(db, db_ref, rtol=2e-4, atol_scale=5e-5, name='dbias')
    gy2, db2 = ops.bias_act_bwd(go.cuda(), a, rows // nseg, act, True)
    assert torch.equal(gy, gy2) and torch.equal(db, db2), 'the dense form of the same call differs'


@pytest.mark.parametrize('act', ACTS)
def test_bias_act_edge_values(ops, act):
    """+-200, +-0, 1e-30 and friends: finite outputs, tanh(+-0) = +-0, saturation exact to 1 ulp of +-1 / 0 / 1."""
    vals = torch.tensor([200.0, -200.0, 0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0, 104.0, -104.0, 20.0, -20.0, 0.02, -0.02, 0.019, 1.0], dtype=torch.float32)
    y = vals.repeat(4, 1).contiguous()                               # [4, 16]
    a = ops.bias_act_(y.cuda(), None, 4, act).cpu()
    assert torch.isfinite(a).all()
    assert torch.equal(a[0], a[3])
    a, ulp1 = a[0], 2.0 ** -24                                       # spacing of the floats just below 1
    close_fwd(a, TORCH64[act](vals.double()), name='edge values')
    if act == 'tanh':
        assert a[0].item() == 1.0 and a[1].item() == -1.0 and a[6].item() == 1.0 and a[7].item() == -1.0
        assert a[2].item() == 0.0 and a[3].item() == 0.0 and not torch.signbit(a[2]) and torch.signbit(a[3])
        assert a[4].item() == pytest.approx(1e-30, rel=1e-6) and a[5].item() == pytest.approx(-1e-30, rel=1e-6)
        assert abs(a[10].item() - 1.0) <= ulp1 and abs(a[11].item() + 1.0) <= ulp1
    if act == 'sigmoid':
        assert a[0].item() == 1.0 and a[1].item() == 0.0 and a[2].item() == 0.5 and a[3].item() == 0.5
        assert abs(a[6].item() - 1.0) <= ulp1 and 0.0 <= a[7].item() <= 2e-38 and 0.0 <= a[9].item() <= 1e-44
        assert abs(a[10].item() - 1.0) <= ulp1
    if act == 'relu':
        assert a[1].item() == 0.0 and a[2].item() == 0.0 and a[3].item() == 0.0 and a[0].item() == 200.0
    if act == 'leaky_relu':
        assert a[1].item() == np.float32(-200.0) * np.float32(0.01) and a[0].item() == 200.0 and a[2].item() == 0.0
    g = torch.ones(4, 16)
    gy, _ = ops.bias_act_bwd(g.cuda(), a.repeat(4, 1).contiguous().cuda(), 4, act, False)
    assert torch.isfinite(gy).all()
    slope = {'relu': lambda o: (o > 0).double(), 'leaky_relu': lambda o: torch.where(o > 0, 1.0, 0.01).double(),
             'tanh': lambda o: 1 - o.double() ** 2, 'sigmoid': lambda o: o.double() * (1 - o.double())}[act](a)
    close(gy[0], slope, name='act\'(a)')


# ------------------------------------------------------------------------------------------ 2. GEMM epilogues
T_, F_ = True, False
GEMM_CASES = [
    # site,                                                    M,   N,   K,   akc, bkc, bias, batch, split (None: the wrapper's choice; 2: mode 2 with both handles given)
    ('rows form',                                              1,   256, 384, T_, T_, T_, 1, None),
    ('rows form, batch, ragged N',                             3,   130, 260, T_, T_, F_, 2, None),
    ('generic tiles, tiny and odd',                            5,   7,   3,   T_, T_, T_, 3, None),
    ('generic tiles, transposed A',                            300, 5,   33,  F_, T_, T_, 2, None),
    ('first edition, no K split, fp32 instruction',            100, 132, 72,  T_, T_, T_, 1, 0),
    ('first edition, no K split, bf16 planes',                 100, 132, 72,  T_, T_, T_, 1, 6),
    ('first edition, whole tiles, fp32 instruction',           128, 256, 96,  T_, T_, T_, 1, 0),
    ('first edition, whole tiles, bf16 planes',                128, 256, 96,  T_, T_, T_, 1, 6),
    ('first edition, fix-up',                                  300, 256, 384, T_, T_, T_, 1, 0),
    ('second edition, whole tile + both edges, 3 K steps',     300, 200, 96,  T_, T_, T_, 1, 6),
    ('third edition, whole tile + both edges, mode 2',         300, 200, 96,  T_, T_, T_, 1, 2),
    ('second edition, K tail, mode 2',                         300, 200, 72,  T_, T_, T_, 1, 2),
    ('K-split fix-up of the 256 x 128 editions, bf16 planes',  300, 256, 384, T_, T_, T_, 1, 6),
    ('K-split fix-up of the 256 x 128 editions, mode 2',       300, 256, 384, T_, T_, T_, 1, 2),
    ('per-member',                                             260, 256, 256, T_, F_, T_, 8, None),
]


@pytest.fixture(scope='module')
def gemm_inputs():
    """Operands and the fp64 product + bias of every GEMM case, computed once and shared by the four activations; never written to."""
    out = {}
    for site, M, N, K, akc, bkc, bias, batch, split in GEMM_CASES:
        g = torch.Generator().manual_seed(M + N + K)
        sh = (batch,) if batch > 1 else ()
        A = torch.randn(*sh, *((M, K) if akc else (K, M)), generator=g)
        B = torch.randn(*sh, *((N, K) if bkc else (K, N)), generator=g) / K ** 0.5
        b = torch.randn(*sh, N, generator=g) if bias else None
        Ad = A.double() if akc else A.double().transpose(-1, -2)
        Bd = B.double().transpose(-1, -2) if bkc else B.double()
        pre = Ad @ Bd
        if bias:
            pre = pre + b.double().unsqueeze(-2)
        out[site] = (A, B, b, pre)
    return out


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('case', GEMM_CASES, ids=[c[0].replace(' ', '_') for c in GEMM_CASES])
def test_gemm_epilogue_vs_fp64(ops, gemm_inputs, case, act):
    site, M, N, K, akc, bkc, bias, batch, split = case
    A, B, b, pre = gemm_inputs[site]
    Ad, Bd, bd = A.cuda(), B.cuda(), None if b is None else b.cuda()
    kw = dict(split=split)
    if split == 2:
        kw.update(amax_a=ops.amax(Ad), amax_b=ops.amax(Bd))

    def run(a):
        ops.LAST_SPLIT[0] = None
        o = ops.gemm_f32(Ad, Bd, akc, bkc, bd, a, **kw)
        if split is not None:
            assert ops.LAST_SPLIT[0] == split, f'the product ran in mode {ops.LAST_SPLIT[0]}'
        return o
    out = run(act)
    close(out, TORCH64[act](pre).float(), rtol=1e-5, atol_scale=1e-6, name=f'{site} {act}')
    assert torch.equal(out, run(act)), 'a second call differs'
    if act in TORCH32:
        assert torch.equal(out, TORCH32[act](run(None))), 'not torch\'s activation of the same call with act=None, bit for bit'


# ------------------------------------------------------------------------------------------ 3. magnitude
@pytest.mark.parametrize('act', ACTS)
def test_linear_act_publishes_the_magnitude_of_the_activated_values(ops, act):
    assert ops.amax_tracking()
    g = torch.Generator().manual_seed(9)
    x, W, b = rnd(4096, 128, g=g).cuda(), rnd(256, 128, g=g, scale=128 ** -0.5).cuda(), rnd(256, g=g).cuda()
    y = ops.linear_act(x, W, b, act)
    assert y.numel() == 1 << 20
    h = ops.amax_of(y)
    assert h is not None, 'the output carries no magnitude handle: the next product would run mode 6 or pay a pre-pass'
    assert ops.amax_value(h) == y.abs().max().item()
    if act == 'relu':                                               # (|pre-activation| is larger on the negative side for some seed: not the stored values')
        assert ops.amax_value(h) == y.max().item()


# ------------------------------------------------------------------------------------------ 4. autograd nodes
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('lead,n_in,n_out', [((5, 40), 17, 128), ((3, 700), 17, 6)])
def test_linear_act_odd_widths_vs_fp64(ops, lead, n_in, n_out, act):
    """Odd input width (17 -> 20 zero-padded columns: exact zeros in every dot product) and odd output width (6 -> 8: the padded output
    columns hold act(0 + 0) - 0.5 for sigmoid - and are sliced away; their gradient columns are dropped)."""
    g = torch.Generator().manual_seed(n_out)
    x, W, b = rnd(*lead, n_in, g=g), rnd(n_out, n_in, g=g, scale=n_in ** -0.5), rnd(n_out, g=g, scale=0.3)
    w = rnd(*lead, n_out, g=g)
    xr, Wr, br = (t.double().requires_grad_(True) for t in (x, W, b))
    ref = TORCH64[act](F.linear(xr, Wr, br))
    (ref * w.double()).sum().backward()
    xs, Ws, bs = (t.cuda().requires_grad_(True) for t in (x, W, b))
    y = ops.linear_act(xs, Ws, bs, act)
    assert y.shape == (*lead, n_out)
    (y * w.cuda()).sum().backward()
    for nm, a, r in (('y', y, ref), ('dx', xs.grad, xr.grad), ('dW', Ws.grad, Wr.grad), ('db', bs.grad, br.grad)):
        assert a.shape == r.shape, nm
        close(a, r, rtol=2e-4, atol_scale=5e-5, name=nm)
    if n_out % 4:
        npad = n_out + (-n_out) % 4
        assert y.stride(-2) == npad, 'the output is expected to be the leading columns of the padded GEMM output'
        rows = y.numel() // n_out
        whole = torch.as_strided(y.detach(), (rows, npad), (npad, 1), y.storage_offset())
        pad_value = TORCH64[act](torch.zeros((), dtype=torch.float64)).item()
        assert (whole[:, n_out:] == pad_value).all(), 'padded output columns hold act(0 + 0)'


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('R,T,n_in,H', [(3, 50, 24, 32), (3, 1500, 128, 128)])
def test_ensemble_layers_vs_fp64(ops, R, T, n_in, H, act):
    """Shared-input layer -> per-member layer -> per-member output layer, the activation fused into the first two: output, dX, dW, db
    against fp64 torch autograd; `grad_part` gives the same action-block gradient as the full dX."""
    from offpolicy_rnn.models.ensemble_linear_model import EnsembleLinear
    torch.manual_seed(3)
    E = 4
    l1, l2, l3 = EnsembleLinear(n_in, H, E), EnsembleLinear(H, H, E, desire_ndim=4), EnsembleLinear(H, 1, E, desire_ndim=4)
    for l in (l1, l2, l3):
        torch.nn.init.normal_(l.bias, std=0.3)
    x = torch.randn(R, T, n_in)
    w = torch.randn(E, R, T, 1)
    xr = x.double().requires_grad_(True)
    pr = [[p.detach().double().requires_grad_(True) for p in (l.weight, l.bias)] for l in (l1, l2, l3)]
    h = xr
    for i, (Wt, bt) in enumerate(pr):
        h = torch.einsum('...ti,eio->e...to', h, Wt) if i == 0 else torch.einsum('e...ti,eio->e...to', h, Wt)
        h = h + bt.view(E, 1, 1, -1)
        if i < 2:
            h = TORCH64[act](h)
    (h * w.double()).sum().backward()
    expect = [h.detach(), xr.grad] + [p.grad for pair in pr for p in pair]
    for l in (l1, l2, l3):
        l.cuda()
    flops0 = ops.GEMM_FLOPS[0]
    xs = x.cuda().requires_grad_(True)
    q = l3(l2(l1(xs, act=act), act=act))
    (q * w.cuda()).sum().backward()
    got = [q, xs.grad] + [p.grad for l in (l1, l2, l3) for p in (l.weight, l.bias)]
    for i, (a, b) in enumerate(zip(got, expect)):
        close(a, b, rtol=2e-4, atol_scale=5e-5, name=f'tensor {i}')
    assert ops.GEMM_FLOPS[0] > flops0
    col0 = n_in - 8                                                  # the action block: the last 8 input columns
    full = [xs.grad[..., col0:].clone()] + [p.grad.clone() for l in (l1, l2, l3) for p in (l.weight, l.bias)]
    for l in (l1, l2, l3):
        l.zero_grad()
    xs2 = x.cuda()
    xp = xs2[..., col0:].clone().requires_grad_(True)
    q2 = l3(l2(l1(xs2, act=act, grad_part=(xp, col0)), act=act))
    (q2 * w.cuda()).sum().backward()
    assert torch.equal(q2, q)
    close(xp.grad, expect[1][..., col0:], rtol=2e-4, atol_scale=5e-5, name='action block of dX')
    close(xp.grad, full[0].cpu(), rtol=2e-5, atol_scale=2e-5, name='action block vs the full dX')
    for a, b in zip([p.grad for l in (l1, l2, l3) for p in (l.weight, l.bias)], full[1:]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ 5. routing
def _count_modules(monkeypatch, *classes):
    calls = collections.Counter()
    for cls in classes:
        def fwd(self, x, _f=cls.forward, _n=cls.__name__):
            calls[_n] += 1
            return _f(self, x)
        monkeypatch.setattr(cls, 'forward', fwd)
    return calls


def _dense_pass(ops, monkeypatch, activation, switch, slope=None):
    """One forward and backward of RNNBase(['fc', 'efc-4', 'efc-4']) -> (names `ops.bias_act_bwd` was called with, module forward counts,
    output, dX).  slope: replaces every LeakyReLU module by one with that slope (the spec string builds torch's default)."""
    from offpolicy_rnn.models.rnn_base import RNNBase
    if switch is None:
        monkeypatch.delenv('RESEL_ACT_FUSED', raising=False)
    else:
        monkeypatch.setenv('RESEL_ACT_FUSED', switch)
    names = []
    real = ops.bias_act_bwd

    def spy(g2, a2, rows_per_seg, act, need_dbias):
        names.append(act)
        return real(g2, a2, rows_per_seg, act, need_dbias)
    monkeypatch.setattr(ops, 'bias_act_bwd', spy)
    calls = _count_modules(monkeypatch, torch.nn.ReLU, torch.nn.Tanh, torch.nn.LeakyReLU, torch.nn.GELU)
    torch.manual_seed(0)
    net = RNNBase(16, 4, [32, 32], activation, ['fc', 'efc-4', 'efc-4'])
    for i, a in enumerate(net.activation_list):
        if slope is not None and isinstance(a, torch.nn.LeakyReLU):
            net.activation_list[i] = torch.nn.LeakyReLU(slope)
    net.cuda()
    x = torch.randn(3, 40, 16, device='cuda', requires_grad=True)
    y, _, _ = net.meta_forward(x)
    y.sum().backward()
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    return names, calls, y.detach(), x.grad


@pytest.mark.parametrize('name,module', [('relu', 'ReLU'), ('tanh', 'Tanh')])
def test_dense_step_routes_by_the_switch(ops, monkeypatch, name, module):
    act = [name, name, 'linear']
    names, calls, y_on, dx_on = _dense_pass(ops, monkeypatch, act, None)
    assert names.count(name) == 2 and calls[module] == 0, (names, calls)
    names, calls, y_off, dx_off = _dense_pass(ops, monkeypatch, act, '0')
    assert name not in names and calls[module] == 2, (names, calls)
    close(y_on, y_off.cpu(), rtol=1e-5, atol_scale=1e-6, name='fused vs torch spelling: y')
    close(dx_on, dx_off.cpu(), rtol=2e-4, atol_scale=5e-5, name='fused vs torch spelling: dx')
    names, calls, _, _ = _dense_pass(ops, monkeypatch, act, '1')
    assert names.count(name) == 2 and calls[module] == 0
    with pytest.raises(ValueError):
        _dense_pass(ops, monkeypatch, act, '2')


@pytest.mark.parametrize('switch', [None, '0'])
def test_other_activations_keep_their_module(ops, monkeypatch, switch):
    names, calls, _, _ = _dense_pass(ops, monkeypatch, ['gelu', 'gelu', 'linear'], switch)
    assert calls['GELU'] == 2 and not [n for n in names if n is not None], (names, calls)
    names, calls, _, _ = _dense_pass(ops, monkeypatch, ['leaky_relu', 'leaky_relu', 'linear'], switch, slope=0.2)     # no code for another slope
    assert calls['LeakyReLU'] == 2 and 'leaky_relu' not in names, (names, calls)


def _update_parameter(case):
    import bench
    par = bench.make_parameter('gilr', ROWS, STEPS, D=D)
    for k, v in update_overrides(*UPDATE_CASES[case]).items():
        setattr(par, k, v)
    return par


def _build_trainer(case):
    import bench
    from offpolicy_rnn import alg_init
    torch.manual_seed(INIT_SEED)
    np.random.seed(INIT_SEED)
    alg = alg_init(_update_parameter(case))
    bench.fill_synthetic(alg, 2 * ROWS, STEPS, DATA_SEED)
    return alg


def test_action_only_graph_follows_the_switch(ops, monkeypatch):
    alg = _build_trainer('relu')
    critic = alg.values[0]
    assert isinstance(critic.uni_network.activation_list[0], torch.nn.ReLU)
    frozen = [critic.state_input_encoder.weight, critic.action_input_encoder.weight, critic.uni_network.layer_list[0].weight]
    was = [p.requires_grad for p in frozen]
    for p in frozen:
        p.requires_grad_(False)
    try:
        monkeypatch.delenv('RESEL_ACT_FUSED', raising=False)
        assert critic._action_only_graph()
        monkeypatch.setenv('RESEL_ACT_FUSED', '0')
        assert not critic._action_only_graph()
        monkeypatch.setenv('RESEL_ACT_FUSED', '1')
        assert critic._action_only_graph()
    finally:
        for p, r in zip(frozen, was):
            p.requires_grad_(r)


# ------------------------------------------------------------------------------------------ 6. whole update
@pytest.fixture
def cpu_noise(monkeypatch):
    """The product's Gaussian draws come from the CPU generator, like the oracle's."""
    from offpolicy_rnn.utility import rng
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.randn(tuple(shape), dtype=dtype).to(device))


@pytest.fixture
def no_noise(monkeypatch):
    """Actor noise off: a captured generator draws from graph-safe Philox offsets, an eager one does not."""
    from offpolicy_rnn.utility import rng
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.zeros(tuple(shape), dtype=dtype, device=device))


@pytest.mark.parametrize('case', list(UPDATE_CASES))
def test_eager_update_against_the_fp64_oracle(ops, case, cpu_noise, monkeypatch):
    """gilr SAC-REDQ, D = 32, 8 rows x 64 steps: two eager updates of the product against `OracleTrainer(dtype=torch.float64)` on the
    product's initial weights, the same trajectories, seeds and noise draws, through tests/update_parity.py with its own bounds.  The
    fp32 oracle on the same weights goes through the same comparison first: the inputs' own guard (test_dense_activations_host.py)."""
    from oracle.trainer import OracleTrainer, default_parameter
    alg = _build_trainer(case)
    assert alg.device.type == 'cuda'
    emb, head = UPDATE_CASES[case]
    cpu_sd = lambda m: {k: {n: t.detach().cpu().clone() for n, t in d.items()} for k, d in m.state_dict().items()}
    ps, vs = cpu_sd(alg.policy), cpu_sd(alg.values[0])

    def oracle(dtype, n_updates):
        par = default_parameter(rnn='gilr', D=D, algo='sac', sac_batch_size=ROWS * STEPS - 1, max_buffer_transition_num=4 * ROWS * STEPS,
                                **update_overrides(emb, head))
        tr = OracleTrainer(par, OBS, ACT, STEPS, policy_state=ps, value_state=vs, dtype=dtype)
        tr.fill_synthetic(2 * ROWS, STEPS, seed=DATA_SEED)
        torch.manual_seed(UPDATE_SEED)
        np.random.seed(UPDATE_SEED)
        logs = [tr.train_one_batch()]
        tr.grad_num += 1
        moments = dict(policy=UP.oracle_moments(tr.policy, tr.opt_policy), value=UP.oracle_moments(tr.value, tr.opt_value))
        for _ in range(n_updates - 1):
            logs.append(tr.train_one_batch())
        return moments, logs

    fused = []
    real = ops.bias_act_bwd

    def spy(g2, a2, rows_per_seg, act, need_dbias):
        fused.append(act)
        return real(g2, a2, rows_per_seg, act, need_dbias)
    monkeypatch.setattr(ops, 'bias_act_bwd', spy)
    torch.manual_seed(UPDATE_SEED)
    np.random.seed(UPDATE_SEED)
    got_logs = [dict(alg.train_one_batch())]
    alg.grad_num += 1
    got = dict(policy=UP.product_moments(alg.policy.store, alg.optimizer_policy), value=UP.product_moments(alg.values[0].store, alg.optimizer_value))
    got_logs.append(dict(alg.train_one_batch()))
    torch.cuda.synchronize()
    assert head in fused and emb in fused, f'the fused activations did not run: {collections.Counter(fused)}'

    ref, ref_logs = oracle(torch.float64, 2)
    m32, l32 = oracle(torch.float32, 1)
    guard = UP.compare_update(f'fp32 oracle gilr sac {case} {ROWS}x{STEPS} D={D} (the inputs\' guard)', m32, ref, l32, ref_logs[:1])
    assert not guard['failures'] and all(w <= UP.MOMENT_BOUND / 10 for w, _ in guard['worst'].values()), \
        f'these inputs put a pre-activation within fp32 distance of a kink: choose another seed ({guard["worst"]}, {guard["failures"]})'
    rep = UP.compare_update(f'gilr sac {case} {ROWS}x{STEPS} D={D}', got, ref, got_logs, ref_logs)
    assert got_logs[0]['real_batch_size'] == ROWS * STEPS and got_logs[0]['real_batch_traj_num'] == ROWS
    assert not rep['failures'], rep['failures']


@pytest.mark.parametrize('case', list(UPDATE_CASES))
def test_replayed_update_equals_the_eager_update(ops, case, no_noise):
    """The same update captured by `GraphedUpdate`: once a step is replayed whole, further steps launch nothing eagerly, and every step's
    logged scalars match the eager trainer's to LOG_TOL[0]."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    n_upd = 4

    def build():
        alg = _build_trainer(case)
        np.random.seed(11)
        return alg
    eager = build()
    assert GraphedUpdate.refusal(eager) is None, GraphedUpdate.refusal(eager)
    logs_e = []
    for _ in range(n_upd):
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    graphed = build()
    gu = GraphedUpdate(graphed, warmup=1)
    try:
        logs_g, fallbacks = [], []
        for _ in range(n_upd):
            before = gu.eager_fallbacks
            logs_g.append(dict(gu.step()))
            graphed.grad_num += 1
            fallbacks.append(gu.eager_fallbacks - before)
        torch.cuda.synchronize()
        print(f'MEASURED gilr sac {case} eager passes per step through GraphedUpdate: {fallbacks}, graphs {len(gu.graphs)}')
        assert len(gu.graphs) == 1 and fallbacks[-2:] == [0, 0], fallbacks
        rel, ab = UP.LOG_TOL[0]
        val = lambda v: v[0] if isinstance(v, tuple) else v
        for le, lg in zip(logs_e, logs_g):
            assert set(le) == set(lg)
            for k in le:
                assert float(val(lg[k])) == pytest.approx(float(val(le[k])), rel=rel, abs=ab), (k, le[k], lg[k])
    finally:
        gu.close()
