"""The selective scan at every d_state from 1 to 256 (`ops.sscan_state_plan`): sizes up to 64 zero-padded onto the next native kernel,
larger ones as groups of 64 plus a remainder joined by the gate / reduce kernels of csrc/sscan_gate.hip.  GPU box only.

1. Padding is exact: N = 12, 24, 40 through both nodes are `torch.equal` to the native kernel on hand-padded operands.
2. Against fp64 (`oracle.kernels.selective_scan_ref` on fp64 leaves; inputs, regimes and bars of tests/test_mixer_kernels_gpu.py): the
   mixer's form (code 6, column-block operands, in-place column-block outputs, handles) and `ops.selective_scan_tm` with and without
   z / D / delta_bias and with the last state.  For N > 64 a sum has up to N / 64 times as many terms, so every bar is that file's times
   ceil(N / 64) and no more.  Every error is printed as a fraction of its bound (`SSCAN-FIG`; profiles/r33_sscan_states.md keeps them).
3. Layers `smamba_s24 / s128`, `mamba_s24 / s96`: forward, dx and parameter gradients against the CPU oracle backend at the bars of
   tests/test_layers_gpu.py; the one-token step carried over a row against the whole-row forward at the bar of tests/test_rollout_gpu.py.
4. Trainers `smamba_s24_*` (padded) and `smamba_s96_*` (grouped): eager update finite, `GraphedUpdate` records and replays it and agrees
   with eager at the bar of tests/test_trainer_gpu.py::test_graphed_update_equals_the_eager_update; clean under RESEL_AMAX_VERIFY.
5. Native sizes launch what they launched; N = 300 is refused at the first forward.
Before the plan existed every case here except the native half of 5 stopped with `selective_scan_fwd failed`."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import kernels as K
from test_mixer_kernels_gpu import R, _fraction, close, held_handle, is_sentinel, scan_inputs, scan_reference_of, sentinel_fill

pytestmark = pytest.mark.gpu
B, L, DI = 2, 100, 128                                # two channel tiles; rows cross the 8-step checkpoint, the 16-step sub-chunk, the 32-step chunk


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def groups_of(N):
    return -(-N // 64)


def held_fwd(case, name, got, ref, k=1):
    """`close_fwd` of tests/test_mixer_kernels_gpu.py with every term of the bound times k = ceil(N / 64)."""
    print(f'SSCAN-FIG {case} {name} {_fraction(got, ref, 1e-4, 2e-5, fwd=True) / k:.4f}')
    close(got, ref, rtol=1e-4 * k, atol_scale=2e-5 * k, name=f'{case} {name}')
    got, ref = got.detach().float().cpu(), ref.detach().float()
    bound = k * (1e-4 * ref.abs() + 1e-5 * max(ref.abs().max().item(), 1e-6))
    worst = ((got - ref).abs() / bound).max().item()
    assert worst <= 1.0, f'{case} {name}: worst element at {worst:.2f}x its element-wise bound'


def held_grad(case, name, got, ref, k=1):
    print(f'SSCAN-FIG {case} {name} {_fraction(got, ref, 2e-4, 5e-5) / k:.4f}')
    close(got, ref, rtol=2e-4 * k, atol_scale=5e-5 * k, name=f'{case} {name}')


def pad_cols(t, Np):
    out = torch.zeros(*t.shape[:-1], Np, dtype=t.dtype, device=t.device)
    out[..., :t.shape[-1]] = t
    return out


# ------------------------------------------------------------------------------------------------ 1. padding is exact
def _tm_inputs(N, seed=0):
    g = torch.Generator().manual_seed(100 + N + seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    start = (torch.rand(B, L, generator=g) < 0.03).float()
    start[:, 0] = 1
    start[0, 32] = start[0, 63] = 1
    return dict(u=rnd(B, L, DI), delta=0.5 * rnd(B, L, DI), A=-torch.exp(0.3 * rnd(DI, N)), Bm=rnd(B, L, N), Cm=rnd(B, L, N), D=rnd(DI), z=rnd(B, L, DI),
                bias=0.1 * rnd(DI), start=start, dout=rnd(B, L, DI))


def _run_tm(ops, c, opts=('z', 'D', 'bias')):
    leaves = {k: c[k].cuda().requires_grad_(True) for k in ('u', 'delta', 'A', 'Bm', 'Cm', 'D', 'z', 'bias')}
    pick = lambda name: leaves[name] if name in opts else None
    out, last = ops.selective_scan_tm(leaves['u'], leaves['delta'], leaves['A'], leaves['Bm'], leaves['Cm'], pick('D'), pick('z'), pick('bias'),
                                      c['start'].cuda(), True, True)
    (out * c['dout'].cuda()).sum().backward()
    return out, last, {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize('N', [12, 24, 40])
def test_padding_is_exact_through_selective_scan_tm(ops, N):
    """Same kernel, same numbers: the bar is zero."""
    Np = ops.sscan_padded_states(ops.sscan_state_plan(N))
    assert Np in ops.SSCAN_NATIVE_STATES and Np > N
    c = _tm_inputs(N)
    hand = dict(c, A=pad_cols(c['A'], Np), Bm=pad_cols(c['Bm'], Np), Cm=pad_cols(c['Cm'], Np))
    out, last, g = _run_tm(ops, c)
    out_h, last_h, g_h = _run_tm(ops, hand)
    assert out.shape == (B, L, DI) and last.shape == (B, DI, N) and g['A'].shape == (DI, N) and g['Bm'].shape == (B, L, N)
    assert torch.equal(out, out_h) and torch.equal(last, last_h[..., :N])
    assert not last_h[..., N:].any(), 'a padded state left 0'
    for name in ('u', 'delta', 'z', 'D', 'bias'):
        assert torch.equal(g[name], g_h[name]), name
    for name in ('A', 'Bm', 'Cm'):
        assert torch.equal(g[name], g_h[name][..., :N]), name
        assert torch.isfinite(g_h[name]).all()


def _mixer_inputs(N, Dm=32, Rk=8, Kw=4, seed=0):
    g = torch.Generator().manual_seed(200 + N + seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    start = (torch.rand(B, L, generator=g) < 0.03).float()
    start[:, 0] = 1
    start[0, 32] = 1
    return dict(x=rnd(B, L, Dm), in_w=rnd(2 * DI, Dm) / math.sqrt(Dm), conv_w=0.3 * rnd(DI, 1, Kw), conv_b=0.1 * rnd(DI),
                xproj_w=rnd(Rk + 2 * N, DI) / math.sqrt(DI), dt_w=rnd(DI, Rk) / math.sqrt(Rk), dt_b=0.5 * rnd(DI) - 2,
                A_log=torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(DI, 1), D=torch.ones(DI) + 0.1 * rnd(DI),
                out_w=rnd(Dm, DI) / math.sqrt(DI), mask=(torch.rand(B, L, generator=g) > 0.1).float(), start=start, dout=rnd(B, L, Dm))


MIXER_LEAVES = ('x', 'in_w', 'conv_w', 'conv_b', 'xproj_w', 'dt_w', 'dt_b', 'A_log', 'D', 'out_w')


def _run_mixer(ops, c):
    lv = {k: c[k].cuda().requires_grad_(True) for k in MIXER_LEAVES}
    out = ops.mamba_inner_fn(*[lv[k] for k in MIXER_LEAVES], c['mask'].cuda(), c['start'].cuda())
    (out * c['dout'].cuda()).sum().backward()
    return out, {k: v.grad for k, v in lv.items()}


@pytest.mark.parametrize('N', [12, 24, 40])
def test_padding_is_exact_through_the_fused_node(ops, N):
    """`mamba_inner_fn` at N against itself at the native size with x_proj's weight and A_log padded by hand (zero rows / columns)."""
    Np, Rk = ops.sscan_padded_states(ops.sscan_state_plan(N)), 8
    c = _mixer_inputs(N, Rk=Rk)
    xw = torch.zeros(Rk + 2 * Np, DI)
    xw[:Rk + N], xw[Rk + Np:Rk + Np + N] = c['xproj_w'][:Rk + N], c['xproj_w'][Rk + N:]
    hand = dict(c, xproj_w=xw, A_log=pad_cols(c['A_log'], Np))
    out, g = _run_mixer(ops, c)
    out_h, g_h = _run_mixer(ops, hand)
    assert torch.equal(out, out_h)
    for name in MIXER_LEAVES:
        if name == 'xproj_w':
            assert g[name].shape == (Rk + 2 * N, DI)
            assert torch.equal(g[name][:Rk + N], g_h[name][:Rk + N]) and torch.equal(g[name][Rk + N:], g_h[name][Rk + Np:Rk + Np + N])
            assert torch.isfinite(g_h[name]).all(), 'the gradient rows of padded states (dropped by the plan) are finite'
        elif name == 'A_log':
            assert g[name].shape == (DI, N) and torch.equal(g[name], g_h[name][:, :N]) and torch.isfinite(g_h[name]).all()
        else:
            assert torch.equal(g[name], g_h[name]), name


# ------------------------------------------------------------------------------------------------ 2. against fp64
@functools.lru_cache(maxsize=None)
def scan_case(Bsz, Ln, N, regime):
    c = scan_inputs(Bsz, Ln, DI, N, regime)
    return c, scan_reference_of(c, Bsz, Ln, DI, N)


def run_plan_scan(ops, c, Bsz, Ln, N, segs, monkeypatch, backward=True):
    """The scan calls of `MambaInnerFn` for any N: x_dbl / dx_dbl are `sscan_padded_states` wide (x_proj's padded weight gives zero columns)."""
    monkeypatch.setattr(ops, 'SSCAN_TIME_SEGMENTS', segs)
    dev = torch.device('cuda', torch.cuda.current_device())
    M = Bsz * Ln
    plan = ops.sscan_state_plan(N)
    Np = ops.sscan_padded_states(plan)
    x_dbl = torch.zeros(M, R + 2 * Np)
    x_dbl[:, :R + N], x_dbl[:, R + Np:R + Np + N] = c['x_dbl'][:, :R + N], c['x_dbl'][:, R + N:]
    xz, x_dbl, dt, A_log, D, dout = (t.to(dev) for t in (c['xz'], x_dbl, c['dt'], c['A_log'], c['D'], c['dout']))
    startf = c['start'].to(dev).reshape(-1).contiguous()
    u, z, Bm, Cm = xz[:, :DI], xz[:, DI:], x_dbl[:, R:R + Np], x_dbl[:, R + Np:]
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    A_g = ops._group_A(A_log, plan)
    r = dict(y=new(M, DI), plan=plan, Np=Np)
    r['h_y'], p_y, e_y = ops._slot_args(True, dev)
    cks, parts, lasts = ops._plan_fwd(plan, A_g, Bsz, Ln, u, dt, z, Bm, Cm, D, None, startf, r['y'], True, True, 6, p_y, e_y)
    r['last'] = ops._join_states([t.view(Bsz * DI, -1) for t in lasts], plan, N).view(Bsz, DI, N)
    if not backward:
        return r
    r['dxz'], r['dx_dbl'] = sentinel_fill(new(M, 2 * DI)), sentinel_fill(new(M, R + 2 * Np))
    r.update(du=new(M, DI), ddt=new(M, DI), dD=new(DI), dbias=new(DI))
    r['h_dxz'], p_dxz, e_b = ops._slot_args(True, dev)
    r['h_ddt'], p_ddt, _ = ops._slot_args(True, dev)
    dA_g = ops._plan_bwd(plan, A_g, Bsz, Ln, u, dt, z, Bm, Cm, D, None, startf, dout, cks, parts, r['du'], r['ddt'], r['dxz'][:, DI:],
                         r['dx_dbl'][:, R:R + Np], r['dx_dbl'][:, R + Np:], r['dD'], r['dbias'], 6, p_dxz, p_ddt, e_b)
    r['dA'] = ops._join_states(dA_g, plan, N)
    return r


def check_plan_scan(ops, case, r, ref, N):
    k, Np = groups_of(N), r['Np']
    held_fwd(case, 'out', r['y'], ref['out'], k)
    held_fwd(case, 'last_state', r['last'], ref['last'], k)
    dz = r['dxz'][:, DI:].clone()
    for name, got in (('du', r['du']), ('ddelta', r['ddt']), ('dz', dz), ('dB', r['dx_dbl'][:, R:R + N]), ('dC', r['dx_dbl'][:, R + Np:R + Np + N]),
                      ('dA_log', r['dA']), ('dD', r['dD']), ('dbias', r['dbias'])):
        held_grad(case, name, got, ref['dA' if name == 'dA_log' else name], k)
    assert is_sentinel(r['dxz'][:, :DI]) and is_sentinel(r['dx_dbl'][:, :R]), f'{case}: the scan backward wrote outside its column blocks'
    assert torch.isfinite(r['dx_dbl'][:, R:]).all(), f'{case}: the dB / dC columns of padded states are finite'
    # the handles the out_proj, dt_proj and in_proj products scale with hold the maxima of the FINAL tensors, to the bit
    held_handle(ops, case, 'y', r['h_y'], r['y'])
    held_handle(ops, case, 'ddt', r['h_ddt'], r['ddt'])
    held_handle(ops, case, 'dxz(scan)', r['h_dxz'], dz)


@pytest.mark.parametrize('regime', ['init', 'slow'])
@pytest.mark.parametrize('N', [24, 72, 96, 100, 128, 256])
def test_plan_scan_code6_vs_fp64_oracle(ops, monkeypatch, N, regime):
    case = f'plan[{B}x{L}x{DI}x{N} {regime}]'
    c, ref = scan_case(B, L, N, regime)
    r = run_plan_scan(ops, c, B, L, N, 0, monkeypatch)
    assert [kn for _, _, kn in r['plan']] == {24: [32], 72: [64, 8], 96: [64, 32], 100: [64, 64], 128: [64, 64], 256: [64] * 4}[N]
    check_plan_scan(ops, case, r, ref, N)


@pytest.mark.parametrize('N', [24, 100])
def test_plan_scan_three_time_segments_vs_fp64_oracle_and_one_pass(ops, monkeypatch, N):
    """time_segments = 3 at L = 200 (segments of 96, the last one ragged): every group carries its own segment states."""
    Ln, regime = 200, 'slow'
    case = f'plan[{B}x{Ln}x{DI}x{N} segs=3 {regime}]'
    c, ref = scan_case(B, Ln, N, regime)
    assert ref['last'].abs().max().item() > 1.0, 'the carried state is load-bearing'
    r = run_plan_scan(ops, c, B, Ln, N, 3, monkeypatch)
    check_plan_scan(ops, case, r, ref, N)
    one = run_plan_scan(ops, c, B, Ln, N, 1, monkeypatch, backward=False)
    k = groups_of(N)
    print(f'SSCAN-FIG {case} segmented-vs-one-pass {_fraction(r["y"], one["y"].cpu(), 1e-5, 1e-6) / k:.4f}')
    close(r['y'], one['y'].cpu(), rtol=1e-5 * k, atol_scale=1e-6 * k, name=f'{case} segmented vs one pass')


OPTIONS = [('z', 'D', 'bias'), (), ('z',), ('D', 'bias')]


@functools.lru_cache(maxsize=None)
def tm_reference(N, opts):
    c = _tm_inputs(N, seed=1)
    lv = {k: c[k].double().requires_grad_(True) for k in ('u', 'delta', 'A', 'Bm', 'Cm', 'D', 'z', 'bias')}
    pick = lambda name: lv[name] if name in opts else None
    out, last = K.selective_scan_ref(lv['u'], lv['delta'], lv['A'], lv['Bm'], lv['Cm'], pick('D'), pick('z'), pick('bias'), c['start'].double(), True)
    (out * c['dout'].double()).sum().backward()
    return c, out.detach(), last.detach(), {k: v.grad for k, v in lv.items()}


@pytest.mark.parametrize('opts', OPTIONS, ids=lambda o: '+'.join(o) or 'bare')
@pytest.mark.parametrize('N', [24, 72, 96, 100, 128, 256])
def test_selective_scan_tm_options_vs_fp64_oracle(ops, N, opts):
    """`SelectiveScanFn` (the `mamba_*` family's node; softplus and delta_bias inside the scan): with and without z, D and delta_bias, with
    the last state.  An absent operand gets no gradient."""
    case = f'scan_tm[{B}x{L}x{DI}x{N} {"+".join(opts) or "bare"}]'
    k = groups_of(N)
    c, out_ref, last_ref, g_ref = tm_reference(N, opts)
    out, last, g = _run_tm(ops, c, opts)
    held_fwd(case, 'out', out, out_ref, k)
    held_fwd(case, 'last_state', last, last_ref, k)
    for name in ('u', 'delta', 'A', 'Bm', 'Cm', 'D', 'z', 'bias'):
        if name in opts or name in ('u', 'delta', 'A', 'Bm', 'Cm'):
            held_grad(case, 'd' + name, g[name], g_ref[name], k)
        else:
            assert g[name] is None and g_ref[name] is None, name


# ------------------------------------------------------------------------------------------------ 3. layers
LAYER_IDS = ['smamba_s24_c4_b1', 'smamba_s128_c4_b1_nln', 'mamba_s24_c3', 'mamba_s96_c3']


def _layer_net(lid):
    from offpolicy_rnn.models.rnn_base import RNNBase
    torch.manual_seed(11)
    net = RNNBase(32, 32, [], ['linear'], [lid])
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():                                  # zero-initialised biases would hide bias handling
        for n_, p_ in net.named_parameters():
            if 'bias' in n_ and p_.abs().sum() == 0:
                p_.copy_(torch.randn(p_.shape, generator=g) * 0.1)
    return net, g


@pytest.mark.parametrize('lid', LAYER_IDS)
def test_layer_fwd_bwd_vs_cpu_oracle_backend(ops, lid):
    """D = 32, B = 2, T = 40 with mid-row resets and masked slots: y, dx and every parameter gradient at the bars
    tests/test_layers_gpu.py::test_layer_fwd_bwd_vs_reference_recording holds the native ids to."""
    import oracle_backend
    net, g = _layer_net(lid)
    Bsz, T = 2, 40
    x, w = torch.randn(Bsz, T, 32, generator=g), torch.randn(Bsz, T, 32, generator=g)
    start = torch.zeros(Bsz, T, 1)
    start[:, 0], start[0, 17], start[1, 33] = 1, 1, 1
    mask = torch.ones(Bsz, T, 1)
    mask[1, 30:33] = 0

    def run(dev):
        net.zero_grad()
        xs = x.clone().to(dev).requires_grad_(True)
        hid = net.make_init_state(Bsz, torch.device(dev))
        hid.set_rnn_start(start.to(dev))
        hid.set_mask(mask.to(dev))
        y = net.meta_forward(xs, hid)[0]
        (y * w.to(dev)).sum().backward()
        return y.detach().cpu(), xs.grad.cpu(), {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None}

    with pytest.MonkeyPatch.context() as mp:
        oracle_backend.install(mp)
        y_ref, dx_ref, g_ref = run('cpu')
    net.cuda()
    y, dx, grads = run('cuda')
    np.testing.assert_allclose(y, y_ref, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(dx, dx_ref, rtol=1e-3, atol=1e-4)
    assert set(grads) == set(g_ref) and any('A_log' in k_ for k_ in grads)
    for name, v in g_ref.items():
        np.testing.assert_allclose(grads[name], v, rtol=2e-3, atol=3e-4, err_msg=name)


@pytest.mark.parametrize('lid', LAYER_IDS)
def test_layer_steps_carried_over_a_row_match_the_whole_row_forward(ops, lid):
    """The one-token rollout step (any N, untouched here) against the training forward of the same row, at the bar of
    tests/test_rollout_gpu.py::test_layer_steps_match_reference_recording."""
    net, g = _layer_net(lid)
    net.cuda()
    Bsz, T = 2, 40
    x = torch.randn(Bsz, T, 32, generator=g).cuda()
    with torch.no_grad():
        whole = net.meta_forward(x, net.make_init_state(Bsz, x.device))[0]
        hid, ys = net.make_init_state(Bsz, x.device), []
        for t in range(T):
            y, hid, _ = net.meta_forward(x[:, t:t + 1], hid)
            ys.append(y)
    np.testing.assert_allclose(torch.cat(ys, dim=1).cpu(), whole.cpu(), rtol=1e-4, atol=2e-5)


# ------------------------------------------------------------------------------------------------ 4. trainers
def _trainer(rnn):
    from test_host_logic import _push, _synth, make_parameter
    from offpolicy_rnn import alg_init
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter(rnn, algo='sac', sac_batch_size=4 * 12 - 1, cuda_inference=True))
    rs = np.random.RandomState(3)
    for _ in range(8):
        o, a, r = _synth(rs, 12, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=False)
    np.random.seed(11)
    return alg


@pytest.mark.parametrize('rnn', ['smamba_s24_c4_b1_nln', 'smamba_s96_c4_b1_nln'])
def test_trainer_updates_eagerly_replays_from_a_graph_and_is_clean_in_verify_mode(ops, monkeypatch, rnn):
    """The small shape and the bar (parameters and logged scalars to 2e-5) of
    tests/test_trainer_gpu.py::test_graphed_update_equals_the_eager_update: four eager updates against warm-up + recording + replays."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    from offpolicy_rnn.utility import rng
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.zeros(tuple(shape), dtype=dtype, device=device))
    state = lambda alg: [alg.policy.store.flat.detach().clone(), alg.values[0].store.flat.detach().clone(),
                         alg.target_values[0].store.flat.detach().clone(), alg.log_sac_alpha.detach().clone()]
    value = lambda v: v[0] if isinstance(v, tuple) else v
    n_upd = 4
    eager, logs_e = _trainer(rnn), []
    for _ in range(n_upd):
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    assert 'critic_loss' in logs_e[0] and all(math.isfinite(value(v)) for lg in logs_e for v in lg.values() if isinstance(value(v), float))
    graphed, logs_g = _trainer(rnn), []
    assert GraphedUpdate.refusal(graphed) is None
    gu = GraphedUpdate(graphed, warmup=1)
    try:
        for _ in range(n_upd):
            logs_g.append(dict(gu.step()))
            graphed.grad_num += 1
        torch.cuda.synchronize()
        assert gu.graph is not None and 1 <= gu.eager_fallbacks <= 3, 'the update was recorded and replayed'
    finally:
        gu.close()
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), state(graphed), state(eager)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=2e-7, err_msg=nm)
    for le, lg in zip(logs_e, logs_g):
        assert set(le) == set(lg)
        for key in le:
            assert abs(value(le[key]) - value(lg[key])) <= 2e-5 * max(1.0, abs(value(le[key]))), (key, le[key], lg[key])
    monkeypatch.setattr(ops, 'AMAX_VERIFY', True)
    checked = _trainer(rnn)
    log = checked.train_one_batch()                         # raises AmaxBoundError itself at the end of the update
    ops.amax_verify_raise(checked.device)
    assert all(math.isfinite(value(v)) for v in dict(log).values() if isinstance(value(v), float))


# ------------------------------------------------------------------------------------------------ 5. native sizes, refusals
def test_native_size_launches_what_it_launched_and_a_grouped_size_adds_the_gate_kernels(ops):
    def launches(N):
        c = _tm_inputs(N)
        ops.profile_collect()
        ops.profile_enable(True)
        try:
            _run_tm(ops, c)
            torch.cuda.synchronize()
            return {k_: n for k_, (n, _) in ops.profile_collect().items()}
        finally:
            ops.profile_enable(False)

    assert launches(32) == {'sscan_fwd_kernel': 1, 'sscan_bwd_kernel': 1}
    assert launches(24) == {'sscan_fwd_kernel': 1, 'sscan_bwd_kernel': 1}                      # padded: the native scan and nothing else
    assert launches(128) == {'sscan_fwd_kernel': 2, 'sscan_bwd_kernel': 2, 'sscan_gate_fwd_kernel': 1, 'sscan_gate_bwd_kernel': 1,
                             'sscan_group_reduce_kernel': 1}


def test_d_state_300_is_refused_at_the_first_forward(ops):
    from offpolicy_rnn.models.rnn_base import RNNBase
    c = _tm_inputs(300)
    with pytest.raises(ValueError, match='accepted are 1 to 256'):
        _run_tm(ops, c)
    with pytest.raises(ValueError, match='accepted are 1 to 256'):
        _run_mixer(ops, _mixer_inputs(300))
    net = RNNBase(32, 32, [], ['linear'], ['smamba_s300_c4_b1_nln']).cuda()                   # constructs: the grammar takes any size
    with pytest.raises(ValueError, match='256 is this build\'s bound: 4 groups'):
        net.meta_forward(torch.randn(2, 40, 32, device='cuda'), net.make_init_state(2, torch.device('cuda')))
