"""N independent GRU recurrences in one launch (`resel_gru_multi_fwd`, `ops.gru_seq_multi`) against the single-network entry points.

The multi kernels run the SAME step body as `resel_gru_seq_fwd`'s (csrc/gru_seq.hip: `gru_fwd_persistent_body` / `gru_fwd_step_body`), and
the persistent and the per-step form reduce in the same split and order, so every comparison between them here is `torch.equal`:
tolerance zero.  Each case prints the form (1 persistent, 0 per step) both calls took."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RG = 4                                                              # batch rows per workgroup (csrc/gru_seq.hip)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def _granules(B, H):
    return ((B + RG - 1) // RG) * 2 * RG * H


def _single_form(B, H):
    """The rule of `resel_gru_seq_fwd` (include/resel_hip.h): persistent while the grid has at most 256 workgroups."""
    return int(os.environ.get('RESEL_GRU_PERSISTENT', '1') != '0' and (H // 16) * ((B + RG - 1) // RG) <= 256)


def _inputs(n, B, L, H, seed, h0_mask, dev='cuda'):
    g = torch.Generator().manual_seed(seed)
    nets = []
    for k in range(n):
        gi = torch.randn(B, L, 3 * H, generator=g)
        w = torch.randn(3 * H, H, generator=g) / math.sqrt(H)
        b = torch.randn(3 * H, generator=g) * 0.1
        h0 = torch.randn(B, H, generator=g) * 0.5 if h0_mask[k] else None
        nets.append(tuple(None if t is None else t.to(dev) for t in (gi, w, b, h0)))
    return nets


def _run_single(o, net, B, L, H, want_gates):
    from offpolicy_rnn.hip._lib import check, lib
    gi, w, b, h0 = net
    h_all = torch.full((B, L, H), float('nan'), device='cuda')
    gates = torch.full((B, L, 4 * H), float('nan'), device='cuda') if want_gates else None
    ws = torch.empty(lib().resel_gru_workspace_bytes(B, L, H), dtype=torch.uint8, device='cuda')
    check(lib().resel_gru_seq_fwd(o._p(gi), o._p(w), o._p(b), o._p(h0), o._p(h_all), o._p(gates), o._p(ws), B, L, H, o._stream()), 'gru_seq_fwd')
    torch.cuda.synchronize()
    off = (3 * H * H + 2 * B * H) * 4 + _granules(B, H) * 8
    err = int(ws[off:off + 4].view(torch.int32).item()) if _single_form(B, H) else 0
    return h_all, gates, err


def _run_multi(o, nets, B, L, H, gates_mask):
    from offpolicy_rnn.hip._lib import check, lib
    n = len(nets)
    outs = [torch.full((B, L, H), float('nan'), device='cuda') for _ in nets]
    gates = [torch.full((B, L, 4 * H), float('nan'), device='cuda') if m else None for m in gates_mask]
    ws = torch.empty(lib().resel_gru_multi_workspace_bytes(n, B, L, H), dtype=torch.uint8, device='cuda')
    VP = ctypes.c_void_p * n
    arr = lambda ts: VP(*[None if t is None else t.data_ptr() for t in ts])
    check(lib().resel_gru_multi_fwd(n, arr([t[0] for t in nets]), arr([t[1] for t in nets]), arr([t[2] for t in nets]), arr([t[3] for t in nets]),
                                    arr(outs), arr(gates), o._p(ws), B, L, H, o._stream()), 'gru_multi_fwd')
    torch.cuda.synchronize()
    sync = _granules(B, H) * 8 + 64                                 # per network: granules, then the 64-byte block of its error word
    errs = []
    for k in range(n):
        off = n * 3 * H * H * 4 + k * sync + _granules(B, H) * 8
        errs.append(int(ws[off:off + 4].view(torch.int32).item()))
    return outs, gates, errs


def _compare(o, n, B, L, H, seed=0):
    """Multi against one single call per network: h_all and the requested gates bit for bit, error words zero, no NaN.  The gates /
    h0 patterns mix NULL and non-NULL entries inside one call (all four combinations appear at n = 4)."""
    gates_mask = [(True, False, True, False)[k] for k in range(n)]
    h0_mask = [(False, False, True, True)[k] for k in range(n)]
    nets = _inputs(n, B, L, H, seed + 17 * n + H, h0_mask)
    form_m, form_s = o.gru_multi_form(n, B, H), _single_form(B, H)
    print(f'n {n} B {B} L {L} H {H}: multi form {form_m}, single form {form_s}')
    outs, gates, errs = _run_multi(o, nets, B, L, H, gates_mask)
    assert errs == [0] * n, f'error words {errs}'
    for k, net in enumerate(nets):
        h_ref, g_ref, err = _run_single(o, net, B, L, H, gates_mask[k])
        assert err == 0
        assert torch.isfinite(outs[k]).all() and torch.isfinite(h_ref).all(), k
        assert torch.equal(outs[k], h_ref), (k, (outs[k] - h_ref).abs().max().item())
        if gates_mask[k]:
            assert torch.isfinite(gates[k]).all() and torch.equal(gates[k], g_ref), k
    return form_m, form_s


# (64, 1027, 256): the bench's pass; (8, 131, 256): BASELINE configs[0]'s; (5, 33, 48): rows past B, KC = 4; (6, 21, 192): KC = 12;
# (6, 17, 384), (4, 9, 512): the wide instantiations (KC = 24 / 32)
SHAPES = [(64, 1027, 256), (8, 131, 256), (5, 33, 48), (6, 21, 192), (6, 17, 384), (4, 9, 512)]


@pytest.mark.parametrize('B,L,H', SHAPES)
@pytest.mark.parametrize('n', [1, 2, 3, 4])
def test_multi_fwd_equals_one_single_call_per_network(ops, n, B, L, H):
    _compare(ops, n, B, L, H)


def test_multi_fwd_past_the_residency_bound_takes_the_per_step_form(ops):
    """4 x 32 x 16 = 2 048 workgroups at H = 512 (2 per CU admitted): not co-resident, so the launch-per-step form with the network in
    grid.z runs; the single call (512 workgroups > 256) is per-step too."""
    form_m, form_s = _compare(ops, 4, 64, 12, 512)
    assert form_m == 0 and form_s == 0


def test_multi_fwd_with_the_persistent_form_switched_off():
    """RESEL_GRU_PERSISTENT is read once per process: a child process runs one small shape with it set to 0."""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    env = dict(os.environ, RESEL_GRU_PERSISTENT='0')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'child'], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and 'multi form 0, single form 0' in r.stdout and 'child ok' in r.stdout


def close_fwd(got, ref, rtol=1e-4, floor=1e-5, name=''):
    """The bar `test_gru_seq_fwd_bwd_vs_aten` holds this layer's forward to (tests/test_hip_ops.py `close` + `close_fwd`, restated):
    norm-wise max |got - ref| <= (rtol + 2e-5) max |ref|, and element-wise |got - ref| <= rtol |ref| + floor max |ref|."""
    got = got.detach().float().cpu()
    ref = ref.detach().float()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    assert err <= rtol * scale + 2e-5 * scale, f'{name}: max err {err:.3e} vs scale {scale:.3e}'
    bound = rtol * ref.abs() + floor * scale
    worst = ((got - ref).abs() / bound).max().item()
    print(f'{name}: max err {err:.3e} (scale {scale:.3e}), worst element at {worst:.3f}x its bound')
    assert worst <= 1.0, f'{name}: worst element at {worst:.2f}x its element-wise bound (rtol {rtol}, floor {floor})'


def test_multi_fwd_three_weight_sets_vs_aten(ops):
    """Three networks with different weights in one launch, each against torch.nn.GRU on the CPU."""
    B, L, H = 6, 75, 64
    g = torch.Generator().manual_seed(4)
    jobs, refs = [], []
    for k in range(3):
        gru = torch.nn.GRU(H, H, batch_first=True)
        with torch.no_grad():
            for p in gru.parameters():
                p.copy_(torch.randn(*p.shape, generator=g) * (k + 1) / (2 * math.sqrt(H)))
        x = torch.randn(B, L, H, generator=g)
        h0 = torch.randn(1, B, H, generator=g) * 0.3 if k == 1 else None
        with torch.no_grad():
            refs.append(gru(x, h0)[0])
            gi = torch.nn.functional.linear(x, gru.weight_ih_l0, gru.bias_ih_l0)
        jobs.append((gi.cuda(), gru.weight_hh_l0.detach().cuda(), gru.bias_hh_l0.detach().cuda(), None if h0 is None else h0[0].cuda(), False))
    print(f'multi form {ops.gru_multi_form(3, B, H)}')
    for k, (y, ref) in enumerate(zip(ops.gru_seq_multi(jobs), refs)):
        close_fwd(y, ref, name=f'h_all of network {k}')


@pytest.mark.parametrize('flags', [(True, False, False), (True, False)])
def test_gru_seq_multi_autograd_equals_gru_seq_on_the_differentiated_job(ops, flags):
    B, L, H = 8, 41, 64
    nets = _inputs(len(flags), B, L, H, 23, [False] * len(flags))
    dy = torch.randn(B, L, H, generator=torch.Generator().manual_seed(2)).cuda()
    leaves = [[t.clone().requires_grad_(True) for t in net[:3]] for net in nets]          # every job's tensors ask for gradients
    ys = ops.gru_seq_multi([(gi, w, b, None, f) for (gi, w, b), f in zip(leaves, flags)])
    for y, f in zip(ys, flags):
        assert y.requires_grad == f
    sum((y * dy).sum() for y, f in zip(ys, flags) if f).backward()
    alone = [t.clone().requires_grad_(True) for t in nets[0][:3]]
    y_ref = ops.gru_seq(*alone)
    (y_ref * dy).sum().backward()
    assert torch.equal(ys[0], y_ref)
    for name, a, b in zip(('gi', 'w_hh', 'b_hh'), leaves[0], alone):
        assert a.grad is not None and torch.equal(a.grad, b.grad), name
    for k in range(1, len(flags)):
        with torch.no_grad():
            assert torch.equal(ys[k], ops.gru_seq(*nets[k][:3]))
        assert all(t.grad is None for t in leaves[k]), f'job {k} is a constant of the launch'


if __name__ == '__main__' and sys.argv[1:] == ['child']:
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'recurrent-offpolicy-rl_amd')]
    from offpolicy_rnn.hip import ops as _ops
    for _n in (1, 3):
        _compare(_ops, _n, 5, 33, 48)
    print('child ok')
