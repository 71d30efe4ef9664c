"""Products with one side at most 48 wide on the streaming fp32-MFMA kernels (csrc/skinny_gemm.hip: `resel_narrow_k`,
`resel_narrow_n_pair`) against fp64 products, and the Mamba mixer with and without them (`RESEL_NARROW`).  GPU box only.

Tolerances are derived, not measured.  u = 2^-24.
  product      a length-n fp32 dot product has the forward bound n u sum |a_i b_i|; a factor 4 covers the order in which the matrix
               instruction and the fixed-order partial sums add:   |err| <= 4 n u (|A| |B|), elementwise, n = K, Wd or M.
  bias         one more rounding of (product + bias): u |product + bias| <= u (|A| |B| + |bias|); 2 u is allowed so that second-order terms
               and the rounding of the stored fp32 result are inside.
  activation   softplus and ELU have slope <= 1, so the error in front of them passes at most unchanged; the function itself gets
               8 u |out| more.
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def within(got, ref64, bound64, name):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), f'{name}: non-finite'
    ratio = ((got - ref64).abs() / bound64.clamp_min(1e-300)).max().item()
    print(f'{name}: worst element at {ratio:.3f} of its bound')
    assert ratio <= 1.0, f'{name}: worst element at {ratio:.3f}x its bound'


ACTS = {None: lambda t: t, 'softplus': torch.nn.functional.softplus, 'elu': torch.nn.functional.elu}


@pytest.mark.parametrize('K', [4, 16, 20, 40, 48])
@pytest.mark.parametrize('N', [32, 96, 512])
def test_narrow_k_vs_fp64(ops, K, N):
    """M = 1 (one row), 37 (fewer rows than a wave's tile), 600 (ragged last block); A = columns [off, off + K) of an [M, 80] matrix;
    C = columns [4, 4 + N) of an [M, N + 12] buffer whose other columns must stay as they were; with and without bias; each activation;
    the published magnitude is max |C| exactly."""
    g = torch.Generator().manual_seed(100 * K + N)
    for M in (1, 37, 600):
        full = torch.randn(M, 80, generator=g)
        w = torch.randn(N, K, generator=g) * K ** -0.5
        b = torch.randn(N, generator=g)
        full_d, w_d, b_d = full.cuda(), w.cuda(), b.cuda()
        for off, use_bias, act in itertools.product((0, 16), (False, True), (None, 'softplus', 'elu')):
            a64 = full[:, off:off + K].double()
            mag = a64.abs() @ w.double().abs().t()
            pre = a64 @ w.double().t()
            bound = 4 * K * U * mag
            if use_bias:
                pre = pre + b.double()
                bound = bound + 2 * U * (mag + b.double().abs())
            ref = ACTS[act](pre)
            if act is not None:
                bound = bound + 8 * U * ref.abs()
            buf = torch.full((M, N + 12), 7.5, device='cuda')
            slot = ops._slot_args(True, buf.device)
            out = ops.narrow_k(full_d[:, off:off + K], w_d, b_d if use_bias else None, act, out=buf[:, 4:4 + N], amax_out=slot)
            assert out.data_ptr() == buf[:, 4:4 + N].data_ptr()
            name = f'narrow_k M={M} K={K} N={N} off={off} bias={use_bias} act={act}'
            within(out, ref, bound, name)
            assert (buf[:, :4] == 7.5).all() and (buf[:, 4 + N:] == 7.5).all(), f'{name}: wrote outside its column block'
            assert ops.amax_value(slot[0]) == out.abs().max().item(), f'{name}: published magnitude'
            assert ops.amax_of(out) is slot[0]


@pytest.mark.parametrize('M', [37, 600, 4100])
@pytest.mark.parametrize('Wd', [128, 512])
@pytest.mark.parametrize('Nn', [4, 16, 40])
def test_narrow_n_pair_vs_fp64(ops, M, Wd, Nn):
    """dX = G W into columns [8, 8 + Nn) of an [M, 80] buffer and dW = G^T X with X a column block of an [M, 80] matrix: each output alone
    and both together, every run repeated and bitwise equal.  M = 4100 spans several reduction slices."""
    g = torch.Generator().manual_seed(M + Wd + Nn)
    G = torch.randn(M, Wd, generator=g)
    W = torch.randn(Wd, Nn, generator=g) * Wd ** -0.5
    xfull = torch.randn(M, 80, generator=g)
    X = xfull[:, 16:16 + Nn]
    G64 = G.double()
    ref_dx, bound_dx = G64 @ W.double(), 4 * Wd * U * (G64.abs() @ W.double().abs())
    ref_dw, bound_dw = G64.t() @ X.double(), 4 * M * U * (G64.abs().t() @ X.double().abs())
    G_d, W_d, X_d = G.cuda(), W.cuda(), xfull.cuda()[:, 16:16 + Nn]
    for want_dx, want_dw in ((True, False), (False, True), (True, True)):
        runs = []
        for _ in range(2):
            buf = torch.full((M, 80), -3.25, device='cuda')
            dx, dw = ops.narrow_n_pair(G_d, W_d if want_dx else None, X_d if want_dw else None, dx_out=buf[:, 8:8 + Nn] if want_dx else None)
            runs.append((buf, dw))
            name = f'narrow_n_pair M={M} Wd={Wd} Nn={Nn} dx={want_dx} dw={want_dw}'
            if want_dx:
                assert dx.data_ptr() == buf[:, 8:8 + Nn].data_ptr()
                within(dx, ref_dx, bound_dx, name + ' dX')
                assert (buf[:, :8] == -3.25).all() and (buf[:, 8 + Nn:] == -3.25).all(), f'{name}: wrote outside its column block'
            else:
                assert dx is None and (buf == -3.25).all()
            if want_dw:
                within(dw, ref_dw, bound_dw, name + ' dW')
            else:
                assert dw is None
        assert torch.equal(runs[0][0], runs[1][0]) and (not want_dw or torch.equal(runs[0][1], runs[1][1])), 'not bitwise reproducible'


def _mixer_case():
    g = torch.Generator().manual_seed(21)
    B, L, Dm, N, Kw = 2, 75, 256, 32, 16                      # the flagship widths: Di = 512, R = 16
    Di, R = 2 * Dm, Dm // 16
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    x = r(B, L, Dm)
    ps = dict(in_w=r(2 * Di, Dm, scale=Dm ** -0.5), conv_w=r(Di, 1, Kw, scale=0.3), conv_b=r(Di, scale=0.1),
              xproj_w=r(R + 2 * N, Di, scale=Di ** -0.5), dt_w=r(Di, R, scale=R ** -0.5), dt_b=r(Di, scale=0.5) - 2,
              A_log=torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(Di, 1), D=torch.ones(Di) + r(Di, scale=0.1),
              out_w=r(Dm, Di, scale=Di ** -0.5))
    start = torch.zeros(B, L)
    start[:, 0] = 1
    start[0, 20] = start[0, 51] = 1                           # two trajectory starts inside a row
    start[1, 33] = start[1, 60] = 1
    mask = torch.ones(B, L, 1)
    mask[0, 68:] = 0                                          # masked tails
    mask[1, 71:] = 0
    return x, ps, start, mask, r(B, L, Dm)


def _run_mixer(ops, case, grad=True):
    x, ps, start, mask, w = case
    xs = x.cuda().requires_grad_(True)
    pp = {k: v.cuda().requires_grad_(True) for k, v in ps.items()}
    args = (xs, pp['in_w'], pp['conv_w'], pp['conv_b'], pp['xproj_w'], pp['dt_w'], pp['dt_b'], pp['A_log'], pp['D'], pp['out_w'], mask.cuda(), start.cuda())
    if not grad:
        with torch.no_grad():
            return ops.mamba_inner_fn(*args), None
    out = ops.mamba_inner_fn(*args)
    (out * w.cuda()).sum().backward()
    return out.detach(), dict(x=xs.grad, **{k: v.grad for k, v in pp.items()})


def test_mixer_narrow_route_vs_gemm_route(ops, monkeypatch):
    """`mamba_inner_fn` at the flagship widths, B = 2, L = 75, with `RESEL_NARROW` = 1 against 0: the output and every gradient.
    Bound: each route is held to the suite's fp32 bar against the oracle (tests/test_hip_ops.py `close`: norm-wise (1e-4 + 2e-5) max |ref| for
    the output and dx, (2e-4 + 5e-5) max |ref| for parameter gradients, as `test_mamba_inner_fused_vs_oracle_chain` asks); two routes that
    both meet it differ by at most the sum of the two bounds."""
    case = _mixer_case()
    calls = {'narrow_k': 0, 'narrow_n_pair': 0}
    for name in calls:
        def spy(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    monkeypatch.setenv('RESEL_NARROW', '0')
    out0, g0 = _run_mixer(ops, case)
    assert calls == {'narrow_k': 0, 'narrow_n_pair': 0}
    monkeypatch.setenv('RESEL_NARROW', '1')
    out1, g1 = _run_mixer(ops, case)
    assert calls == {'narrow_k': 1, 'narrow_n_pair': 1}, calls

    def agree(a, b, tol, name):
        scale = max(b.abs().max().item(), 1e-6)
        err = (a - b).abs().max().item()
        print(f'{name}: max difference {err:.3e} of {2 * tol * scale:.3e} allowed')
        assert torch.isfinite(a).all() and err <= 2 * tol * scale, f'{name}: routes differ by {err:.3e}, scale {scale:.3e}'

    agree(out1, out0, 1e-4 + 2e-5, 'out')
    agree(g1['x'], g0['x'], 1e-4 + 2e-5, 'dx')
    for k in case[1]:
        agree(g1[k], g0[k], 2e-4 + 5e-5, 'd' + k)


@pytest.mark.parametrize('narrow', ['1', '0'])
def test_mixer_no_grad_requests_no_checkpoints(ops, monkeypatch, narrow):
    """Under torch.no_grad() the mixer hands the scan no checkpoint buffer (parameters that require grad do not make it one), and its
    output is bitwise the grad-mode output."""
    monkeypatch.setenv('RESEL_NARROW', narrow)
    case = _mixer_case()
    seen = []

    def spy(*a, _f=ops._sscan_fwd, **kw):
        seen.append(a[12])                                    # the `ck` argument
        return _f(*a, **kw)
    monkeypatch.setattr(ops, '_sscan_fwd', spy)
    out_g, _ = _run_mixer(ops, case)
    out_n, _ = _run_mixer(ops, case, grad=False)
    assert len(seen) == 2 and seen[0] is not None and seen[1] is None
    assert torch.equal(out_g, out_n)


def test_selective_scan_no_grad_requests_no_checkpoints(ops, monkeypatch):
    g = torch.Generator().manual_seed(3)
    B, L, Di, N = 2, 70, 64, 32
    r = lambda *s: torch.randn(*s, generator=g)
    u, delta, Bm, Cm = r(B, L, Di).cuda(), (r(B, L, Di) * 0.5).cuda(), r(B, L, N).cuda(), r(B, L, N).cuda()
    A = (-torch.exp(r(Di, N) * 0.3)).cuda().requires_grad_(True)
    seen = []

    def spy(*a, _f=ops._sscan_fwd, **kw):
        seen.append(a[12])
        return _f(*a, **kw)
    monkeypatch.setattr(ops, '_sscan_fwd', spy)
    out_g = ops.selective_scan_tm(u, delta, A, Bm, Cm)
    with torch.no_grad():
        out_n = ops.selective_scan_tm(u, delta, A, Bm, Cm)
    assert len(seen) == 2 and seen[0] is not None and seen[1] is None
    assert torch.equal(out_g.detach(), out_n)
