"""The selective scan and the causal conv in the form the fused Mamba mixer calls them, against the fp64 CPU oracle.  GPU box only.

`ops.MambaInnerFn` drives `ops._sscan_fwd` / `_sscan_bwd` / `_conv_fwd` / `_conv_bwd` with `delta_softplus` code 6 (the kernels form
A = -exp(A_log) themselves and return dL/dA_log; delta arrives finished, without a bias, and ddelta is still taken back through the
softplus), with operands that are column blocks of wider matrices (xz [M, 2Di], x_dbl [M, R+2N]), with outputs written in place into
column blocks of dxz and dx_dbl, with a two-gradient conv backward (dy + dy2, summed on load) and with magnitude handles published
for xc, y, ddt and dxz (one handle, two publishers, one epoch).  The tests here call the same helpers with the same layout and
codes and NO GEMM in the way, so kernel error is not folded into GEMM error.

Reference: `oracle/kernels.py` on fp64 leaves (the fp32 inputs taken up exactly).  Tolerances are tests/test_hip_ops.py's: forward
outputs and the last state `close_fwd` (1e-4 element-wise with a 1e-5 floor on max|ref|), every gradient
`close(rtol=2e-4, atol_scale=5e-5)`; segmented against one-pass output `close(rtol=1e-5, atol_scale=1e-6)`.  Every comparison prints
its error as a fraction of its bound (`MIXER-FIG` lines under `pytest -s`; profiles/r26_mixer_kernel_tests.md keeps the measured ones).
"""
import functools
import math

import pytest
import torch

from oracle import kernels as K

pytestmark = pytest.mark.gpu

R = 8                                                 # dt_rank columns in front of B | C in x_dbl
SENTINEL = 0x7fc0beef                                 # a quiet NaN with a payload: no kernel output compares equal to it by accident


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def close(got, ref, rtol=1e-4, atol_scale=2e-5, name=''):
    got = got.detach().float().cpu()
    ref = ref.detach().float()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    assert err <= rtol * scale + atol_scale * scale, f'{name}: max err {err:.3e} vs scale {scale:.3e}'


def close_fwd(got, ref, rtol=1e-4, floor=1e-5, name=''):
    """Forward outputs: north_star's rtol read ELEMENT-WISE - |got - ref| <= rtol * |ref| + floor * max|ref| for every element
    (the floor keeps elements that vanish by cancellation from being held to their own size) - on top of the norm-wise bound."""
    close(got, ref, rtol=rtol, name=name)
    got = got.detach().float().cpu()
    ref = ref.detach().float()
    bound = rtol * ref.abs() + floor * max(ref.abs().max().item(), 1e-6)
    worst = ((got - ref).abs() / bound).max().item()
    assert worst <= 1.0, f'{name}: worst element at {worst:.2f}x its element-wise bound (rtol {rtol}, floor {floor})'


def _fraction(got, ref, rtol, atol_scale, fwd=False):
    """The error of `got` as a fraction of the bound `close` / `close_fwd` holds it to (measurement only: the assertions are theirs)."""
    got, ref = got.detach().float().cpu(), ref.detach().float()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs()
    frac = err.max().item() / ((rtol + atol_scale) * scale)
    if fwd:
        frac = max(frac, (err / (1e-4 * ref.abs() + 1e-5 * scale)).max().item())
    return frac


def held_fwd(case, name, got, ref):
    print(f'MIXER-FIG {case} {name} {_fraction(got, ref, 1e-4, 2e-5, fwd=True):.4f}')
    close_fwd(got, ref, name=f'{case} {name}')


def held_grad(case, name, got, ref):
    print(f'MIXER-FIG {case} {name} {_fraction(got, ref, 2e-4, 5e-5):.4f}')
    close(got, ref, rtol=2e-4, atol_scale=5e-5, name=f'{case} {name}')


def held_handle(ops, case, name, handle, *tensors):
    """A kernel publishes the maximum of what it stores: the handle equals max |.| over the tensors it covers, to the bit."""
    top = max(t.abs().max().item() for t in tensors)
    val = ops.amax_value(handle)
    print(f'MIXER-AMAX {case} {name} handle {val:.9g} max {top:.9g}')
    assert val == top, f'{case} {name}: handle {val!r} != max |.| {top!r}'


def sentinel_fill(t):
    t.view(torch.int32).fill_(SENTINEL)
    return t


def is_sentinel(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ inputs
def make_start(B, L, g):
    """Flag 1 at step 0, random resets at 3 %, and in row 0 resets either side of the 32-step chunk / checkpoint edges and of the 96-step
    segment edge, plus the last token."""
    s = (torch.rand(B, L, generator=g) < 0.03).float()
    s[:, 0] = 1
    for t in (31, 32, 63, 64, 95, 96, L - 1):
        if t < L:
            s[0, t] = 1
    return s


SLOW_U = 8.0                                          # see scan_inputs


def scan_inputs(B, L, Di, N, regime):
    """fp32 operands of one mixer scan call.  regime 'init': the mixer test's initialisation, A_log = log(1..N),
    dt = softplus(0.5 randn + dt_b), dt_b ~ N(-2, 0.5).  'slow': `_slow_decay_case`'s range, A in [-1, -0.01] and dt in [1e-3, 0.1], both
    log-uniform - a state survives hundreds of steps, so carries across chunks, checkpoints and segments count at full weight.  There u
    is SLOW_U randn: the 3 % resets cut a row into runs of ~33 steps, over which a state element grows to about
    rms(dt) sqrt(33) = 0.033 * 5.7 = 0.19 per unit of u (`_slow_decay_case` has unbroken rows of 300 to 1043 steps and needs no factor);
    8 puts a typical element near 1.5 and the largest final state above 1, which the cases assert.  The scan is linear in u: the factor
    changes no relative error."""
    g = torch.Generator().manual_seed(1000 * L + 10 * N + B + (7 if regime == 'slow' else 0))
    M = B * L
    rnd = lambda *s: torch.randn(*s, generator=g)
    xz, x_dbl, dout = rnd(M, 2 * Di), rnd(M, R + 2 * N), rnd(M, Di)
    if regime == 'slow':
        xz[:, :Di] *= SLOW_U
    if regime == 'init':
        A_log = torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(Di, 1)
        dt = torch.nn.functional.softplus(0.5 * rnd(M, Di) + (0.5 * rnd(Di) - 2))
    else:
        A_log = torch.rand(Di, N, generator=g) * math.log(100.0) + math.log(0.01)
        dt = torch.exp(torch.rand(M, Di, generator=g) * math.log(100.0) + math.log(1e-3))
    D = torch.ones(Di) + 0.1 * rnd(Di)
    return dict(xz=xz, x_dbl=x_dbl, dt=dt, A_log=A_log, D=D, dout=dout, start=make_start(B, L, g))


def scan_reference_of(c, B, L, Di, N):
    """fp64 oracle of code 6: out, last state and the gradients in the kernels' terms (ddelta through the softplus, dbias its column sum,
    dA with respect to A_log)."""
    lv = {k: c[k].double().requires_grad_(True) for k in ('xz', 'x_dbl', 'dt', 'A_log', 'D')}
    v3 = lambda t: t.view(B, L, -1)
    out, last = K.selective_scan_ref(v3(lv['xz'][:, :Di]), v3(lv['dt']), -torch.exp(lv['A_log']), v3(lv['x_dbl'][:, R:R + N]),
                                     v3(lv['x_dbl'][:, R + N:]), lv['D'], v3(lv['xz'][:, Di:]), None, c['start'].double(),
                                     delta_softplus=False)
    (out * v3(c['dout'].double())).sum().backward()
    dt = lv['dt'].detach()
    ddelta = lv['dt'].grad * (1 - torch.exp(-dt))
    gxz, gdbl = lv['xz'].grad, lv['x_dbl'].grad
    return dict(out=out.detach().reshape(B * L, Di), last=last.detach(), du=gxz[:, :Di], dz=gxz[:, Di:], dB=gdbl[:, R:R + N], dC=gdbl[:, R + N:],
                ddelta=ddelta, dbias=ddelta.sum(0), dA=lv['A_log'].grad, dD=lv['D'].grad)


@functools.lru_cache(maxsize=None)
def scan_case(B, L, Di, N, regime):
    """Inputs and fp64 reference of one (shape, regime): computed once, shared by every segment count, never modified."""
    c = scan_inputs(B, L, Di, N, regime)
    return c, scan_reference_of(c, B, L, Di, N)


def carried_state(c, ref, B, L, Di, N):
    """The state the slow-decay cases assert to be above 1, as test_selective_scan_slow_decay_vs_oracle does: the final one.  In a one-row
    case the row ENDS with a reset (the forced one at L - 1) and its final state is one step's input: there the state is read at the end
    of the row's longest run without a reset."""
    if B > 1:
        return ref['last']
    edges = [t for t in range(L) if c['start'][0, t]] + [L]
    end = max(zip(edges[:-1], edges[1:]), key=lambda e: e[1] - e[0])[1]
    head = {k: v[..., :end] if k == 'start' else v[:end] if k in ('xz', 'x_dbl', 'dt', 'dout') else v for k, v in c.items()}
    return scan_reference_of(head, 1, end, Di, N)['last']


def run_mixer_scan(ops, c, B, L, Di, N, segs, monkeypatch, backward=True):
    """The scan calls of `MambaInnerFn.forward` / `.backward`: code 6, column-block operands, in-place column-block outputs, handles."""
    monkeypatch.setattr(ops, 'SSCAN_TIME_SEGMENTS', segs)
    dev = torch.device('cuda', torch.cuda.current_device())
    M = B * L
    xz, x_dbl, dt, A_log, D, dout = (c[k].to(dev) for k in ('xz', 'x_dbl', 'dt', 'A_log', 'D', 'dout'))
    startf = c['start'].to(dev).reshape(-1).contiguous()
    u, z, Bm, Cm = xz[:, :Di], xz[:, Di:], x_dbl[:, R:R + N], x_dbl[:, R + N:]
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    ck = ops._ws(ops.lib().resel_selective_scan_ckpt_bytes(B, L, Di, N), dev)
    r = dict(xz=xz, y=new(M, Di), last=new(B, Di, N))
    r['h_y'], p_y, e_y = ops._slot_args(True, dev)
    ops._sscan_fwd(B, L, u, dt, z, A_log, Bm, Cm, D, None, startf, r['y'], ck, r['last'], 6, p_y, e_y)
    if not backward:
        return r
    r['dxz'], r['dx_dbl'] = sentinel_fill(new(M, 2 * Di)), sentinel_fill(new(M, R + 2 * N))
    r.update(du=new(M, Di), ddt=new(M, Di), dA=new(Di, N), dD=new(Di), dbias=new(Di))
    r['h_dxz'], r['p_dxz'], r['e_b'] = ops._slot_args(True, dev)          # ONE handle for dxz and ONE epoch for the whole backward
    r['h_ddt'], p_ddt, _ = ops._slot_args(True, dev)
    ops._sscan_bwd(B, L, u, dt, z, A_log, Bm, Cm, D, None, startf, dout, ck, r['du'], r['ddt'], r['dxz'][:, Di:], r['dx_dbl'][:, R:R + N],
                   r['dx_dbl'][:, R + N:], r['dA'], r['dD'], r['dbias'], 6, r['p_dxz'], p_ddt, r['e_b'])
    return r


def run_mixer_conv_bwd(ops, r, B, L, Di, Kw, gx_scale=1.0, seed=0):
    """The conv backward of `MambaInnerFn.backward` on the buffers of `run_mixer_scan`: x half of xz, dy = the scan's du, dy2 = a second
    dense gradient, dx into dxz[:, :Di], published into dxz's handle under the scan backward's epoch."""
    g = torch.Generator().manual_seed(seed + L + Kw)
    dev = r['xz'].device
    w = (0.3 * torch.randn(Di, Kw, generator=g)).to(dev)
    b = (0.2 * torch.randn(Di, generator=g)).to(dev)
    maskf = (torch.rand(B * L, generator=g) > 0.1).float().to(dev)
    gx = (gx_scale * torch.randn(B * L, Di, generator=g)).to(dev)
    dw, db = torch.empty(Di, Kw, device=dev), torch.empty(Di, device=dev)
    ops._conv_bwd(B, L, r['xz'][:, :Di], w, b, maskf, r['du'], gx, r['dxz'][:, :Di], dw, db, 1, r['p_dxz'], r['e_b'])


SCAN_ROWS = [  # B, L, Di, N, SSCAN_TIME_SEGMENTS values, regimes
    (3, 130, 72, 8, (1, 2, 0), ('init', 'slow')),       # partial channel tile (Di % 64 != 0), B padded to 8, launch<2, 4>
    (2, 300, 72, 64, (1, 3, 0), ('init', 'slow')),      # launch<8, 8>, three segments of 128
    (2, 175, 128, 32, (1, 0), ('init', 'slow')),        # launch<8, 4>
    (2, 200, 64, 16, (3,), ('init', 'slow')),           # launch<4, 4>, three segments of 96, the last one ragged
    (1, 97, 8, 4, (1,), ('init', 'slow')),              # launch<1, 4>, one tile of 8 channels
    (2, 1043, 64, 32, (1, 11), ('slow',)),              # the headline's row length
    (96, 41, 512, 32, (0,), ('init', 'slow')),          # sscan_fwd2_kernel<8, 4, 16, 0, 3> (bp * nd = 768)
]
SCAN_CASES = [(B, L, Di, N, s, rg) for B, L, Di, N, segs, rgs in SCAN_ROWS for rg in rgs for s in segs]


@pytest.mark.parametrize('B,L,Di,N,segs,regime', SCAN_CASES)
def test_mixer_scan_code6_vs_fp64_oracle(ops, monkeypatch, B, L, Di, N, segs, regime):
    """Code 6 as the mixer calls it: forward output, last state, du, ddelta, dz, dB, dC, dA_log, dD and dbias against the fp64 oracle; the
    column blocks of dxz / dx_dbl the scan does not own stay untouched, and the conv backward leaves the scan's dz untouched; the handles
    of y, ddt and dxz hold the maxima of what was stored.  Slow-decay cases: the carried state is load-bearing (see `carried` below)."""
    case = f'scan[{B}x{L}x{Di}x{N} segs={segs} {regime}]'
    c, ref = scan_case(B, L, Di, N, regime)
    if regime == 'slow':
        carried = carried_state(c, ref, B, L, Di, N)
        assert carried.abs().max().item() > 1.0, f'{case}: carried state {carried.abs().max().item():.3f}'
    r = run_mixer_scan(ops, c, B, L, Di, N, segs, monkeypatch)
    held_fwd(case, 'out', r['y'], ref['out'])
    held_fwd(case, 'last_state', r['last'], ref['last'])
    dz = r['dxz'][:, Di:].clone()
    for name, got in (('du', r['du']), ('ddelta', r['ddt']), ('dz', dz), ('dB', r['dx_dbl'][:, R:R + N]), ('dC', r['dx_dbl'][:, R + N:]),
                      ('dA_log', r['dA']), ('dD', r['dD']), ('dbias', r['dbias'])):
        held_grad(case, name, got, ref['dA' if name == 'dA_log' else name])
    # in-place column blocks: the scan backward owns dxz[:, Di:] and dx_dbl[:, R:], nothing else
    assert is_sentinel(r['dxz'][:, :Di]) and is_sentinel(r['dx_dbl'][:, :R]), f'{case}: the scan backward wrote outside its column blocks'
    held_handle(ops, case, 'y', r['h_y'], r['y'])
    held_handle(ops, case, 'ddt', r['h_ddt'], r['ddt'])
    held_handle(ops, case, 'dxz(scan)', r['h_dxz'], dz)
    run_mixer_conv_bwd(ops, r, B, L, Di, 4)
    assert torch.equal(r['dxz'][:, Di:].view(torch.int32), dz.view(torch.int32)), f'{case}: the conv backward touched the z half of dxz'
    assert not (r['dxz'][:, :Di].view(torch.int32) == SENTINEL).any(), f'{case}: the conv backward left part of the x half unwritten'
    held_handle(ops, case, 'dxz(both)', r['h_dxz'], r['dxz'])
    if segs != 1:
        one = run_mixer_scan(ops, c, B, L, Di, N, 1, monkeypatch, backward=False)
        print(f'MIXER-FIG {case} segmented-vs-one-pass {_fraction(r["y"], one["y"].cpu(), 1e-5, 1e-6):.4f}')
        close(r['y'], one['y'].cpu(), rtol=1e-5, atol_scale=1e-6, name=f'{case} segmented vs one pass')


@pytest.mark.parametrize('big', ['conv', 'scan'])
def test_mixer_dxz_handle_has_two_publishers(ops, monkeypatch, big):
    """dxz has ONE handle that the scan backward (z half) and the conv backward (x half) publish into under one epoch: with either half
    100 times larger than the other the handle holds the larger one - neither publisher can hide behind the other.  The conv's dy (the
    scan's du) is zeroed here, so dy2 alone sizes the x half (the conv backward is linear in dy + dy2: one unpublished run calibrates it)."""
    B, L, Di, N, Kw = 2, 130, 72, 8, 16
    case = f'dxz-handle[{big} half large]'
    c = scan_case(B, L, Di, N, 'init')[0]
    r = run_mixer_scan(ops, c, B, L, Di, N, 1, monkeypatch)
    dz = r['dxz'][:, Di:]
    dz_top = dz.abs().max().item()
    held_handle(ops, case, 'dxz(scan)', r['h_dxz'], dz)
    r['du'].zero_()
    cal = dict(xz=r['xz'], du=r['du'], dxz=torch.empty_like(r['dxz']), p_dxz=None, e_b=0)
    run_mixer_conv_bwd(ops, cal, B, L, Di, Kw, gx_scale=1.0)
    want = 100.0 if big == 'conv' else 0.01
    run_mixer_conv_bwd(ops, r, B, L, Di, Kw, gx_scale=want * dz_top / cal['dxz'][:, :Di].abs().max().item())
    dx_top = r['dxz'][:, :Di].abs().max().item()
    print(f'MIXER-AMAX {case} max|dz| {dz_top:.6g} max|dx| {dx_top:.6g}')
    assert 0.9 * want <= dx_top / dz_top <= 1.1 * want, f'{case}: max|dx| / max|dz| = {dx_top / dz_top}'
    held_handle(ops, case, 'dxz(both)', r['h_dxz'], r['dxz'])


# ------------------------------------------------------------------------------------------------ conv, mixer form
def pad_taps(Kw):
    return 4 if Kw <= 4 else 8 if Kw <= 8 else 16 if Kw <= 16 else 32


def bwd_chunk(L, KT):
    """`bwd_chunk` of csrc/causal_conv1d.hip: the chunk of 64 / 80 / 96 steps that walks the fewest steps over a row (ties: the shorter);
    0: the non-windowed kernel (more than 16 padded taps, or L < 64)."""
    if KT > 16 or L < 64:
        return 0
    best, best_steps = 0, 0
    for tt in range(64, min(96, L) + 1, 16):
        steps = -(-L // tt) * (tt + 2 * KT)
        if not best or steps < best_steps:
            best, best_steps = tt, steps
    return best


CONV_CASES = ([(2, L, 72, Kw, tt, nch) for L, tt, nch in ((70, 64, 2), (130, 80, 2), (175, 96, 2), (37, 0, 0)) for Kw in (4, 8, 16)]
              + [(2, 200, 72, 20, 0, 0),                                   # conv_bwd_kernel<32> with dy2
                 (1, 1043, 72, 16, 96, 11),                                # the headline's chunking: <16, true, 96>, eleven chunks
                 (2, 130, 520, 16, 80, 2)])                                # two 256-channel grid columns


@functools.lru_cache(maxsize=None)
def conv_case(B, L, Di, Kw):
    g = torch.Generator().manual_seed(100 * L + Kw)
    M = B * L
    rnd = lambda *s: torch.randn(*s, generator=g)
    c = dict(xz=rnd(M, 2 * Di), w=0.3 * rnd(Di, Kw), b=0.2 * rnd(Di), mask=(torch.rand(B, L, generator=g) > 0.1).float(),
             dy=rnd(M, Di), dy2=rnd(M, Di), dz=rnd(M, Di))
    xz, w, b = (c[k].double().requires_grad_(True) for k in ('xz', 'w', 'b'))
    y = K.causal_conv1d_silu_ref(xz[:, :Di].view(B, L, Di), w, b, c['mask'].double())
    (y * (c['dy'].double() + c['dy2'].double()).view(B, L, Di)).sum().backward()
    assert not xz.grad[:, Di:].any()
    return c, dict(y=y.detach().reshape(M, Di), dx=xz.grad[:, :Di], dw=w.grad, db=b.grad)


@pytest.mark.parametrize('B,L,Di,Kw,chunk,nchunk', CONV_CASES)
def test_mixer_conv_two_gradients_vs_fp64_oracle(ops, B, L, Di, Kw, chunk, nchunk):
    """The conv as the mixer calls it: x = xz[:, :Di] (token stride 2Di), bias, mask, SiLU; the backward gets dy and dy2 (summed on load)
    and writes dx into dxz[:, :Di].  y, dx, dw and db against the fp64 oracle; xc's and dxz's handles hold the stored maxima."""
    assert bwd_chunk(L, pad_taps(Kw)) == chunk and (not chunk or -(-L // chunk) == nchunk), \
        f'the chunk rule of causal_conv1d.hip now gives {bwd_chunk(L, pad_taps(Kw))} at L={L}, KT={pad_taps(Kw)}: this case no longer ' \
        f'reaches the instantiation its row of CONV_CASES names'
    case = f'conv[{B}x{L}x{Di} Kw={Kw} chunk={chunk}]'
    c, ref = conv_case(B, L, Di, Kw)
    dev = torch.device('cuda', torch.cuda.current_device())
    M = B * L
    xz, w, b, dy, dy2 = (c[k].to(dev) for k in ('xz', 'w', 'b', 'dy', 'dy2'))
    maskf = c['mask'].to(dev).reshape(-1).contiguous()
    xc = sentinel_fill(torch.empty(M, Di, device=dev))
    h_xc, p_xc, e_xc = ops._slot_args(True, dev)
    ops._conv_fwd(B, L, xz[:, :Di], w, b, maskf, xc, 1, p_xc, e_xc)
    held_fwd(case, 'y', xc, ref['y'])
    held_handle(ops, case, 'xc', h_xc, xc)
    dxz = sentinel_fill(torch.empty(M, 2 * Di, device=dev))
    dxz[:, Di:] = c['dz'].to(dev)                                         # what the scan backward left in the z half
    dw, db = sentinel_fill(torch.empty(Di, Kw, device=dev)), sentinel_fill(torch.empty(Di, device=dev))
    h_dxz, p_dxz, e_b = ops._slot_args(True, dev)
    ops._conv_bwd(B, L, xz[:, :Di], w, b, maskf, dy, dy2, dxz[:, :Di], dw, db, 1, p_dxz, e_b)
    held_grad(case, 'dx', dxz[:, :Di], ref['dx'])
    held_grad(case, 'dw', dw, ref['dw'])
    held_grad(case, 'db', db, ref['db'])
    assert torch.equal(dxz[:, Di:].cpu().view(torch.int32), c['dz'].view(torch.int32)), f'{case}: the conv backward touched the z half of dxz'
    held_handle(ops, case, 'dxz(conv)', h_dxz, dxz[:, :Di])


@pytest.mark.parametrize('B,L,Di,Kw', [(2, 70, 72, 4), (2, 37, 72, 16)])
@pytest.mark.parametrize('opts', ['no_mask_no_act', 'no_bias', 'plain'])
def test_causal_conv1d_fn_options_vs_fp64_oracle(ops, B, L, Di, Kw, opts):
    """`ops.causal_conv1d_fn` without a mask and without the activation (models/conv1d/conv1d.py's call), without a bias, and with none
    of the three: forward and backward against the fp64 oracle."""
    with_mask, with_bias, act = {'no_mask_no_act': (False, True, False), 'no_bias': (True, False, True), 'plain': (False, False, False)}[opts]
    case = f'conv_fn[{B}x{L}x{Di} Kw={Kw} {opts}]'
    g = torch.Generator().manual_seed(L + Kw)
    rnd = lambda *s: torch.randn(*s, generator=g)
    xz, w, b, dy = rnd(B, L, 2 * Di), 0.3 * rnd(Di, 1, Kw), 0.2 * rnd(Di), rnd(B, L, Di)
    mask = (torch.rand(B, L, generator=g) > 0.1).float()

    def run(dev, dtype, fn):
        ts = [t.to(dev, dtype).requires_grad_(True) for t in (xz, w, b)]
        y = fn(ts[0][..., :Di], ts[1], ts[2] if with_bias else None, mask.to(dev, dtype) if with_mask else None)
        (y * dy.to(dev, dtype)).sum().backward()
        return y, [t.grad for t in ts[:2 + with_bias]]

    y_ref, g_ref = run('cpu', torch.float64, lambda x, w_, b_, m: K.causal_conv1d_silu_ref(x, w_[:, 0], b_, m, act))
    y_gpu, g_gpu = run('cuda', torch.float32, lambda x, w_, b_, m: ops.causal_conv1d_fn(x, w_, b_, m, act))
    held_fwd(case, 'y', y_gpu, y_ref)
    for name, a, b_ in zip(('dx', 'dw', 'db'), g_gpu, g_ref):
        held_grad(case, name, a, b_)


@pytest.mark.parametrize('with_start', [True, False])
def test_selective_scan_tm_code0_bare_vs_fp64_oracle(ops, with_start):
    """`ops.selective_scan_tm(delta_softplus=False)` - code 0, the backward without its softplus branch - with D, z and delta_bias all
    None, with and without start flags: forward, last state and every gradient against the fp64 oracle."""
    B, L, Di, N = 2, 130, 72, 16
    case = f'scan_tm[code 0 bare start={with_start}]'
    c = scan_inputs(B, L, Di, N, 'init')
    A = -torch.exp(c['A_log'] + 0.3 * torch.randn(Di, N, generator=torch.Generator().manual_seed(3)))
    v3 = lambda t: t.view(B, L, -1)

    def run(dev, dtype, fn):
        xz, x_dbl, dt, A_ = (t.to(dev, dtype).requires_grad_(True) for t in (c['xz'], c['x_dbl'], c['dt'], A))
        start = c['start'].to(dev, dtype) if with_start else None
        out, last = fn(v3(xz[:, :Di]), v3(dt), A_, v3(x_dbl[:, R:R + N]), v3(x_dbl[:, R + N:]), start)
        (out * v3(c['dout'].to(dev, dtype))).sum().backward()
        return out, last, (xz.grad[:, :Di], dt.grad, x_dbl.grad[:, R:R + N], x_dbl.grad[:, R + N:], A_.grad)

    o_ref, l_ref, g_ref = run('cpu', torch.float64, lambda u, d, A_, Bm, Cm, s: K.selective_scan_ref(u, d, A_, Bm, Cm, None, None, None, s, False))
    o_gpu, l_gpu, g_gpu = run('cuda', torch.float32, lambda u, d, A_, Bm, Cm, s: ops.selective_scan_tm(u, d, A_, Bm, Cm, None, None, None, s, False, True))
    held_fwd(case, 'out', o_gpu, o_ref)
    held_fwd(case, 'last_state', l_gpu, l_ref)
    for name, a, b in zip(('du', 'ddelta', 'dB', 'dC', 'dA'), g_gpu, g_ref):
        held_grad(case, name, a, b)
