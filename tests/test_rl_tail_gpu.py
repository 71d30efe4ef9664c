"""The SAC / TD3 tail (tanh-Gaussian head, REDQ target + Q guard, masked losses, soft update, flat AdamW, sum of squares:
csrc/rl_fused.hip, csrc/losses.hip) at the row counts a real update has.  GPU box only.

Every reduction of these files launches at most 256 blocks of 256 threads and walks the rest in a grid-stride loop, so the row
counts below sit on both sides of 256 (one block) and of 65 536 (one trip of the loop), at the benchmark's own M = 64 x 1043 and
at the 512-trajectory global batch on one GPU.

References are fp64 restatements of the arithmetic include/resel_hip.h documents, evaluated on the SAME fp32 inputs.  Scalars
that cross the C ABI as `float` (gamma, tau, lr, weight decay, betas, eps) enter the reference as their fp32-rounded values: that
rounding is the ABI, not a kernel error.  No expected value comes from the kernel or from an fp32 copy of it.

Every test prints the worst `error / bound` it saw (pytest -s) so that the room each bound leaves can be read off a log.

That these tests can fail was checked with four one-line mutations of the kernels, each built into a library of its own and
loaded through RESEL_HIP_LIBRARY (red here / in the four single-case tests of tests/test_hip_ops.py):
  target_y_kernel stride `gridDim.x * 256 + 1`        every target test with M > 65 536 (22 cases) / none
  guard_apply_slots_kernel sums the ranks' rows        test_sac_target_virtual_ranks at every world > 1 (8 cases) / none
  adamw_flat_kernel segment search `i > seg_end`       test_adamw_flat_both_entry_points with 2 or 40 segments (24) / test_flat_optimizer_tail
  actor_loss_bwd_kernel `v <= r`                       test_actor_loss_min_ties (3 cases) / none"""
import math

import numpy as np
import pytest
import torch

from oracle import kernels as K

pytestmark = pytest.mark.gpu

ROWS = [1, 255, 256, 257, 32048, 65536, 65537, 66752, 534016]      # 32 048 = 16 x 2003, 66 752 = 64 x 1043, 534 016 = 512 x 1043
U24, U22 = 2.0 ** -24, 2.0 ** -22


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def f32(x):
    """The value a C `float` parameter receives."""
    return float(np.float32(x))


def close(got, ref, rtol=1e-4, atol_scale=2e-5, name=''):
    """tests/test_hip_ops.py `close` (norm-wise) in fp64; returns error / bound."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    assert err <= (rtol + atol_scale) * scale, f'{name}: max err {err:.3e} vs scale {scale:.3e}'
    return err / ((rtol + atol_scale) * scale)


def close_fwd(got, ref, rtol=1e-4, floor=1e-5, name=''):
    """tests/test_hip_ops.py `close_fwd` (element-wise |got - ref| <= rtol |ref| + floor max|ref|, on top of `close`) in fp64."""
    close(got, ref, rtol=rtol, name=name)
    got, ref = got.detach().double().cpu(), ref.detach().double()
    bound = rtol * ref.abs() + floor * max(ref.abs().max().item(), 1e-6)
    worst = ((got - ref).abs() / bound).max().item()
    assert worst <= 1.0, f'{name}: worst element at {worst:.2f}x its element-wise bound (rtol {rtol}, floor {floor})'
    return worst


def within(got, ref, bound, name):
    """Element-wise |got - ref| <= bound (fp64 tensors of one shape); returns the worst error / bound."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    err = (got - ref).abs()
    bad = err > bound
    if bad.any():
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f'{name}: {int(bad.sum())} of {bad.numel()} elements over their bound, first at flat index {i}: got '
                             f'{got.reshape(-1)[i].item():.9e} ref {ref.reshape(-1)[i].item():.9e} bound {bound.reshape(-1)[i].item():.3e}')
    return (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


# ------------------------------------------------------------------------------------------------ A1: tanh-Gaussian head
LS_LO, LS_HI = np.float32(-20.0), np.float32(2.0)
LS_SPECIAL = [float(LS_LO), float(LS_HI), float(np.nextafter(LS_LO, np.float32(-np.inf))), float(np.nextafter(LS_HI, np.float32(np.inf))),
              -25.0, 3.5]                     # at the bounds (gradient passes), one ulp outside and well outside (it does not)
PLANT_EVERY = 97


def head_inputs(M, A, seed):
    """out2 [M, 2A] = (log-std | mean), noise [M, A].  Row r with r % 97 == 0 carries LS_SPECIAL[(r // 97) % 6] as the log-std of
    action r % A; its noise is 0.25 so that a standard deviation of e^2 and more leaves the pre-activation moderate."""
    g = torch.Generator().manual_seed(seed)
    out2 = torch.randn(M, 2 * A, generator=g)
    out2[:, :A] = out2[:, :A] * 0.8 - 1.5
    noise = torch.randn(M, A, generator=g)
    rows = torch.arange(0, M, PLANT_EVERY)
    cols = rows % A
    out2[rows, cols] = torch.tensor([LS_SPECIAL[(int(r) // PLANT_EVERY) % 6] for r in rows])
    noise[rows, cols] = 0.25
    return out2, noise, rows, cols


def head_ref(out2, noise, ds, dl):
    A = noise.shape[-1]
    o = out2.double().requires_grad_(True)
    mean, samp, logp = K.tanh_gaussian_ref(o[..., A:], o[..., :A], noise.double())
    loss = o.sum() * 0
    if ds is not None:
        loss = loss + (samp * ds.double()).sum()
    if dl is not None:
        loss = loss + (logp.reshape(-1) * dl.double()).sum()
    loss.backward()
    return mean.detach(), samp.detach(), logp.detach().reshape(-1), o.grad


def head_bwd_raw(ops, out2c, noisec, ds, dl):
    """resel_tanh_gaussian_bwd through ctypes: the autograd wrapper always hands both upstream gradients over (zeros for an unused
    output), so the NULL branches of the kernel are only reachable here."""
    M, A = noisec.shape
    d2 = torch.full_like(out2c, float('nan'))
    ops.check(ops.lib().resel_tanh_gaussian_bwd(ops._p(out2c), ops._p(noisec), ops._p(ds), ops._p(dl), ops._p(d2), M, A, ops._stream()),
              'tanh_gaussian_bwd')
    return d2


@pytest.mark.parametrize('A', [1, 3, 6, 17])
@pytest.mark.parametrize('M', ROWS[:-1])
def test_tanh_gaussian_rows(ops, M, A):
    """Forward outputs element-wise at the file's fp32 bar (1e-4, floor 1e-5 of the largest), d_out2 norm-wise at 2.5e-4, against
    fp64 autograd of oracle.kernels.tanh_gaussian_ref; backward with both upstream gradients, with d_sample only and with d_logp
    only.  The planted log-stds check torch.clamp's gradient convention: 1 at -20 and at 2, 0 one ulp outside."""
    out2, noise, rows, cols = head_inputs(M, A, 1000 * A + M % 997)
    g = torch.Generator().manual_seed(M + A)
    ds, dl = torch.randn(M, A, generator=g), torch.randn(M, generator=g)
    mean_r, samp_r, logp_r, d2_r = head_ref(out2, noise, ds, dl)
    oc, nc = out2.cuda().requires_grad_(True), noise.cuda()
    mean, samp, logp = ops.tanh_gaussian(oc, nc)
    assert mean.shape == (M, A) and samp.shape == (M, A) and logp.shape == (M, 1)
    ((samp * ds.cuda()).sum() + (logp.reshape(-1) * dl.cuda()).sum()).backward()
    ratios = dict(mean=close_fwd(mean, mean_r, name='mean'), sample=close_fwd(samp, samp_r, name='sample'),
                  logp=close_fwd(logp.reshape(-1), logp_r, name='logp'),
                  d_out2=close(oc.grad, d2_r, rtol=2e-4, atol_scale=5e-5, name='d_out2'))
    od = oc.detach()
    for nm, a, b in (('d_sample only', ds, None), ('d_logp only', None, dl)):
        ref = head_ref(out2, noise, a, b)[3]
        got = head_bwd_raw(ops, od, nc, None if a is None else a.cuda(), None if b is None else b.cuda())
        ratios['d_out2, ' + nm] = close(got, ref, rtol=2e-4, atol_scale=5e-5, name='d_out2, ' + nm)
    # the clamp's gradient convention, read off the reference and then demanded of the kernel exactly where it is a plain zero
    gl = oc.grad.cpu()[rows, cols]
    outside = torch.tensor([(int(r) // PLANT_EVERY) % 6 >= 2 for r in rows])
    assert (d2_r[rows, cols][outside] == 0).all() and (d2_r[rows, cols][~outside] != 0).all()
    assert (gl[outside] == 0).all() and (gl[~outside] != 0).all()
    print(f'\n[tanh_gaussian M={M} A={A}] error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))


def test_tanh_gaussian_saturated(ops):
    """Pre-activations of magnitude 9, 20 and 60 (softplus branch max(-2 pre, 0), tanh saturated) in a case of their own: their
    log-probabilities of ~2 |pre| would inflate the floor of the ordinary cases."""
    A = 3
    pre = torch.tensor([9.0, -9.0, 20.0, -20.0, 60.0, -60.0, 0.3, -0.3])
    M = pre.numel() * 2
    out2 = torch.zeros(M, 2 * A)
    out2[:, :A] = -20.0                                   # sd = e^-20: pre = mean to fp32
    out2[:, A:] = pre.repeat(2).reshape(M, 1).expand(M, A)
    out2[M // 2:, :A] = 0.0                               # second half: sd = 1 and the noise moves pre by up to ~2
    g = torch.Generator().manual_seed(7)
    noise = torch.randn(M, A, generator=g)
    ds, dl = torch.randn(M, A, generator=g), torch.randn(M, generator=g)
    mean_r, samp_r, logp_r, d2_r = head_ref(out2, noise, ds, dl)
    oc = out2.cuda().requires_grad_(True)
    mean, samp, logp = ops.tanh_gaussian(oc, noise.cuda())
    ((samp * ds.cuda()).sum() + (logp.reshape(-1) * dl.cuda()).sum()).backward()
    r = (close_fwd(mean, mean_r, name='mean'), close_fwd(samp, samp_r, name='sample'), close_fwd(logp.reshape(-1), logp_r, name='logp'),
         close(oc.grad, d2_r, rtol=2e-4, atol_scale=5e-5, name='d_out2'))
    assert logp_r.abs().max() > 300
    print('\n[tanh_gaussian saturated] error / bound: mean %.3f, sample %.3f, logp %.3f, d_out2 %.3f' % r)


# ------------------------------------------------------------------------------------------------ A2: target + guard, one process
class GuardRef:
    """Plain-Python fp64 state machine of the reference's QValueGuard (utility/q_value_guard.py:22-38): clamp() initialises from
    its argument on the first call, update() takes the running min / max and, below decay 1, moves both towards the batch's."""

    def __init__(self, decay):
        self.min, self.max, self.fresh, self.decay = 1000000.0, -1000000.0, True, decay

    def clamp(self, value):
        if self.fresh:
            self.min, self.max, self.fresh = value.min().item(), value.max().item(), False
        return value.clamp(min=self.min, max=self.max)

    def update(self, value):
        vmin, vmax = value.min().item(), value.max().item()
        self.min, self.max = min(self.min, vmin), max(self.max, vmax)
        if self.decay < 1:
            self.min = self.decay * self.min + (1 - self.decay) * vmin
            self.max = self.decay * self.max + (1 - self.decay) * vmax


GAMMA = 0.99
WIDE = (None, 4.0, 5.0)             # from the second batch on, a fifth of the columns is drawn this much wider: the guard has to clamp


def target_batches(M, E, m, sac, mask_kind, seed, calls=3):
    """`calls` consecutive batches for one guard: fp32 CPU tensors q [E, M], subset int32 [m], next_logp [M] / None, log_alpha [1] /
    None, reward, done, mask [M] / None.  The first batch is N(0, 3); in the later ones a column is WIDE[call] x that with
    probability 0.2 and half of it otherwise (column 0 is always wide), so that whatever M and m make of the first batch's range,
    a share of the later columns well inside (1 %, 50 %) falls outside it."""
    g = torch.Generator().manual_seed(seed)
    reward = torch.randn(M, generator=g)
    done = (torch.rand(M, generator=g) < 0.05).float()
    mask = dict(given=(torch.rand(M, generator=g) < 0.8).float(), none=None, zero=torch.zeros(M))[mask_kind]
    out = []
    for it in range(calls):
        wide = WIDE[min(it, len(WIDE) - 1)]
        width = torch.ones(M)
        if wide is not None:
            width = torch.where(torch.rand(M, generator=g) < 0.2, torch.tensor(wide), torch.tensor(0.5))
            width[0] = wide
        q = torch.randn(E, M, generator=g) * (3.0 * width)
        subset = torch.randperm(E, generator=g)[:m].int()
        nl = torch.randn(M, generator=g) * width if sac else None
        la = torch.tensor([-0.3]) if sac else None
        out.append(dict(q=q, subset=subset, next_logp=nl, log_alpha=la, reward=reward, done=done, mask=mask))
    return out


def target_ref(b, guard):
    """One call of the reference (sac_full_length_rnn_redq.py:28-33, td3_full_length_rnn_redq.py:29-35) in fp64 on `guard`
    (a GuardRef).  Returns (y, share of elements the clamp moved)."""
    v = b['q'].double()[b['subset'].long()].min(dim=0).values
    if b['next_logp'] is not None:
        v = v - math.exp(float(b['log_alpha'][0])) * b['next_logp'].double()
    c = guard.clamp(v)
    y = b['reward'].double() + (1 - b['done'].double()) * f32(GAMMA) * c
    mask = torch.ones_like(y) if b['mask'] is None else b['mask'].double()
    guard.update(y * mask)
    return y, (c != v).double().mean().item()


def dev(b):
    return {k: (None if t is None else t.cuda()) for k, t in b.items()}


def run_target(ops, d, guard, stats, **kw):
    return ops.sac_target(d['q'], d['subset'], d['next_logp'], d['log_alpha'], d['reward'], d['done'], d['mask'], GAMMA, guard, stats, **kw)


def fresh_guard(decay):
    return torch.tensor([1000000.0, -1000000.0, 0.0, decay], dtype=torch.float32).cuda()


def _target_cases():
    cases = []
    for M in (66752, 257):           # every value of every axis at the benchmark's row count and at one small one
        cases += [(M, 8, 2, True, 'given', 0.999), (M, 10, 10, False, 'none', 1.0), (M, 1, 1, True, 'zero', 0.9), (M, 2, 1, False, 'given', 0.9),
                  (M, 2, 2, True, 'none', 1.0), (M, 10, 2, False, 'zero', 0.999), (M, 8, 8, True, 'given', 1.0), (M, 8, 1, False, 'none', 0.999)]
    for M in ROWS:                   # every row count in both forms
        if M not in (66752, 257):
            cases += [(M, 8, 2, True, 'given', 0.999), (M, 10, 1, False, 'none', 0.9)]
    cases += [(534016, 2, 2, True, 'zero', 1.0)]
    return cases


@pytest.mark.parametrize('M,E,m,sac,mask_kind,decay', _target_cases())
def test_sac_target_and_guard_rows(ops, M, E, m, sac, mask_kind, decay):
    """Three consecutive `ops.sac_target` calls on one guard that starts uninitialised, against the fp64 state machine: target
    element-wise (1e-4, floor 1e-5), guard {min, max} and max |y| at rel 1e-5, the mask count exactly.  The clamp must be at work:
    in the reference it moves between 1 % and 50 % of the second batch (a single row is moved or not: there the call is only
    required to clamp)."""
    batches = target_batches(M, E, m, sac, mask_kind, seed=M + 31 * E + 7 * m)
    ref_guard = GuardRef(f32(decay))
    guard, stats = fresh_guard(decay), torch.full((2,), float('nan')).cuda()
    worst = dict(target=0.0, guard=0.0, max_abs=0.0)
    shares = []
    for it, b in enumerate(batches):
        y, share = target_ref(b, ref_guard)
        shares.append(share)
        got = run_target(ops, dev(b), guard, stats)
        assert got.shape == (M,)
        worst['target'] = max(worst['target'], close_fwd(got, y, name=f'target[{it}]'))
        gd, st = guard.cpu().double(), stats.cpu().double()
        for nm, a, r in (('min', gd[0].item(), ref_guard.min), ('max', gd[1].item(), ref_guard.max)):
            assert a == pytest.approx(r, rel=1e-5, abs=1e-5), f'guard {nm} after call {it}: {a!r} vs {r!r}'
            worst['guard'] = max(worst['guard'], abs(a - r) / (1e-5 * abs(r) + 1e-5))
        assert gd[2].item() == 1.0 and gd[3].item() == f32(decay)
        assert st[0].item() == pytest.approx(y.abs().max().item(), rel=1e-5)
        worst['max_abs'] = max(worst['max_abs'], rel(st[0].item(), y.abs().max().item()) / 1e-5)
        assert st[1].item() == (M if b['mask'] is None else b['mask'].sum().item())
    assert shares[0] == 0.0                                    # the first interval is the batch's own range
    if M == 1:
        assert shares[1] == 1.0
    else:
        assert 0.01 <= shares[1] <= 0.5, shares
    print(f'\n[sac_target M={M} E={E} m={m} {"SAC" if sac else "TD3"} mask={mask_kind} decay={decay}] clamped share per call '
          + ' '.join(f'{s:.4f}' for s in shares) + ' | error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('sac', [True, False])
@pytest.mark.parametrize('m', [1, 2])
def test_sac_target_hands_nan_on(ops, m, sac):
    """A NaN next-Q in a SELECTED member reaches the target (q.min(dim=0) and clamp of the reference both propagate it; fminf /
    fmaxf alone would turn it into the guard's bound): exactly the planted columns are NaN, every other element is bitwise what
    the finite batch gives (same guard going in, so the clamp is the same), and a NaN in a member outside the subset changes
    nothing at all.  The guard skips NaN rows (include/resel_hip.h): afterwards it is what the finite rows alone produce.
    (Before target_v_kernel carried the NaN, these targets came out finite - at the guard's upper bound with m = 1.)"""
    M, E, decay = 66752, 8, 0.999
    b = target_batches(M, E, m, sac, 'given', seed=90 + m, calls=1)[0]
    g = torch.Generator().manual_seed(5)
    cols = torch.unique(torch.cat((torch.tensor([0, 255, 256, 65535, 65536, 66751]), torch.randint(0, M, (40,), generator=g))))
    b['mask'][cols[:3]] = 0.0                                  # a masked-out row is NaN all the same (0 * NaN)
    b['done'][cols[3:6]] = 1.0                                 # and so is a terminal one
    start = torch.tensor([-4.0, 3.0, 1.0, decay])              # an initialised guard that clamps a good part of the batch
    inside, outside = int(b['subset'][-1]), int([e for e in range(E) if e not in b['subset'].tolist()][0])

    def run(member):
        bb = dict(b, q=b['q'].clone())
        if member is not None:
            bb['q'][member, cols] = float('nan')
        guard, stats = start.clone().cuda(), torch.zeros(2).cuda()
        return run_target(ops, dev(bb), guard, stats).cpu(), guard.cpu(), stats.cpu()

    t0, g0, s0 = run(None)
    t1, g1, s1 = run(inside)
    t2, g2, s2 = run(outside)
    if sac:                                                    # a NaN log-probability takes the same way out
        bb = dict(b, next_logp=b['next_logp'].clone())
        bb['next_logp'][cols] = float('nan')
        t3 = run_target(ops, dev(bb), start.clone().cuda(), torch.zeros(2).cuda()).cpu()
        assert torch.equal(torch.isnan(t3), torch.isnan(t1)) and torch.equal(t3[~torch.isnan(t3)], t1[~torch.isnan(t1)])
    assert torch.isfinite(t0).all()
    assert torch.equal(t2, t0) and torch.equal(g2, g0) and torch.equal(s2, s0)
    nan = torch.zeros(M, dtype=torch.bool)
    nan[cols] = True
    assert torch.equal(torch.isnan(t1), nan), f'{int(torch.isnan(t1).sum())} NaN targets for {cols.numel()} planted columns'
    assert torch.equal(t1[~nan], t0[~nan])
    # fp64 reference over the finite rows, from the same guard
    keep = ~nan
    ref_guard = GuardRef(f32(decay))
    ref_guard.min, ref_guard.max, ref_guard.fresh = -4.0, 3.0, False
    sub = {k: (t[..., keep] if k in ('q', 'next_logp', 'reward', 'done', 'mask') and t is not None else t) for k, t in b.items()}
    y, share = target_ref(sub, ref_guard)
    assert 0.01 <= share <= 0.5
    close_fwd(t1[keep], y, name='finite targets')
    assert g1[0].item() == pytest.approx(ref_guard.min, rel=1e-5) and g1[1].item() == pytest.approx(ref_guard.max, rel=1e-5)
    assert s1[0].item() == pytest.approx(y.abs().max().item(), rel=1e-5) and s1[1].item() == b['mask'].sum().item()


# ------------------------------------------------------------------------------------------------ A3: data-parallel forms
def shard_bounds(M, world):
    """`world` contiguous, unequal shards of M rows; the first holds ONE row (world > 1), the others grow with the rank."""
    if world == 1:
        return [(0, M)]
    w = np.arange(1, world, dtype=np.float64) + 0.37
    sizes = np.maximum(1, np.floor((M - 1) * w / w.sum())).astype(np.int64)
    sizes[-1] += (M - 1) - sizes.sum()
    edges = np.concatenate(([0, 1], 1 + np.cumsum(sizes)))
    assert edges[-1] == M and (np.diff(edges) > 0).all() and len(set(np.diff(edges).tolist())) > 1
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def shard(d, a, b):
    out = dict(d)
    for k in ('next_logp', 'reward', 'done', 'mask'):
        out[k] = None if d[k] is None else d[k][a:b].contiguous()
    out['q'] = d['q'][:, a:b].contiguous()
    return out


def phase_call(ops, phase, d, guard, target, stats, ext, ws):
    E, M = d['q'].shape
    p = ops._p
    ops.check(ops.lib().resel_sac_target_phase(phase, p(d['q']), p(d['subset']), int(d['subset'].numel()), p(d['next_logp']), p(d['log_alpha']),
                                               p(d['reward']), p(d['done']), p(d['mask']), GAMMA, p(guard), p(target), p(stats), p(ext), p(ws),
                                               E, M, ops._stream()), f'sac_target_phase {phase}')


@pytest.mark.parametrize('M', [66752, 300])
@pytest.mark.parametrize('world', [1, 2, 3, 4, 8])
def test_sac_target_virtual_ranks(ops, world, M):
    """Both data-parallel forms of the target on `world` virtual ranks (contiguous unequal shards of one union batch, one guard
    per rank, three updates) reproduce single-process `ops.sac_target` over the union:
      bucket form   - resel_sac_target_local per rank, the [world, 4] slot block as the trainer's SUM all-reduce delivers it (every
                      rank fills its own row of a zero block), resel_guard_apply_slots on every rank;
      all-reduce form - resel_sac_target_phase in lock-step with the element-wise MAX of the two 2-float extrema blocks in between.
    Targets at rtol 1e-6 (same kernel, same inputs: only a clamped element may differ, by the guard's last bit), every rank's
    guard at rel 1e-6 of the single-process one and bitwise equal across ranks, mask counts and max |y| add / max up exactly.
    The fp64 state machine is the outside reference for the union; `ops.guard_apply_slots` is also held to the CPU stand-in the
    host-logic tests trust (tests/oracle_backend.py)."""
    import oracle_backend
    sac, E, m, decay = world % 2 == 1, 8, 2, 0.999
    batches = target_batches(M, E, m, sac, 'given', seed=17 * world + M)
    bounds = shard_bounds(M, world)
    ref_guard = GuardRef(f32(decay))
    g_one, s_one = fresh_guard(decay), torch.zeros(2).cuda()
    g_bkt, g_ar = [fresh_guard(decay) for _ in bounds], [fresh_guard(decay) for _ in bounds]
    ws = [torch.empty(max(int(ops.lib().resel_sac_target_workspace_bytes(b - a)), 16), dtype=torch.uint8).cuda() for a, b in bounds]
    shares, worst = [], 0.0
    for it, b in enumerate(batches):
        y, share = target_ref(b, ref_guard)
        shares.append(share)
        d = dev(b)
        t_one = run_target(ops, d, g_one, s_one)
        worst = max(worst, close_fwd(t_one, y, name=f'union target[{it}]'))
        assert g_one[0].item() == pytest.approx(ref_guard.min, rel=1e-5) and g_one[1].item() == pytest.approx(ref_guard.max, rel=1e-5)
        parts = [shard(d, a, e) for a, e in bounds]
        # ---- bucket form
        exts = [torch.zeros(4).cuda() for _ in bounds]
        stats = [torch.zeros(2).cuda() for _ in bounds]
        t_b = [run_target(ops, parts[r], g_bkt[r], stats[r], local_ext=exts[r]) for r in range(world)]
        blocks = torch.zeros(world, world, 4).cuda()
        for r in range(world):
            blocks[r, r] = exts[r]
        slots = blocks.sum(dim=0).reshape(-1).contiguous()
        before = g_bkt[0].cpu().clone()
        for r in range(world):
            ops.guard_apply_slots(slots, world, g_bkt[r])
        standin = before.clone()
        oracle_backend.guard_apply_slots(slots.cpu(), world, standin)
        np.testing.assert_allclose(g_bkt[0].cpu().numpy(), standin.numpy(), rtol=1e-6, err_msg='guard_apply_slots vs its CPU stand-in')
        # ---- all-reduce form
        ext2 = [torch.zeros(4).cuda() for _ in bounds]
        stats2 = [torch.zeros(2).cuda() for _ in bounds]
        t_a = [torch.empty(e - a).cuda() for a, e in bounds]
        for phase in range(3):
            for r in range(world):
                phase_call(ops, phase, parts[r], g_ar[r], t_a[r], stats2[r], ext2[r], ws[r])
            if phase < 2:
                mx = torch.stack([x[2 * phase:2 * phase + 2] for x in ext2]).max(dim=0).values
                for x in ext2:
                    x[2 * phase:2 * phase + 2] = mx
        # ---- both against the single process
        for nm, ts, gs, sts in (('bucket', t_b, g_bkt, stats), ('all-reduce', t_a, g_ar, stats2)):
            np.testing.assert_allclose(torch.cat(ts).cpu().numpy(), t_one.cpu().numpy(), rtol=1e-6, atol=0, err_msg=f'{nm} targets, update {it}')
            for r in range(world):
                assert torch.equal(gs[r], gs[0]), f'{nm}: guard of rank {r} differs from rank 0 after update {it}'
            np.testing.assert_allclose(gs[0].cpu().numpy(), g_one.cpu().numpy(), rtol=1e-6, err_msg=f'{nm} guard, update {it}')
            assert sum(s[1].item() for s in sts) == s_one[1].item()
            assert max(s[0].item() for s in sts) == s_one[0].item()
    assert shares[0] == 0.0 and 0.01 <= shares[1] <= 0.5 and shares[2] > 0, shares
    print(f'\n[virtual ranks world={world} M={M} {"SAC" if sac else "TD3"}] shards {[e - a for a, e in bounds]} clamped share per update '
          + ' '.join(f'{s:.4f}' for s in shares) + f' | union target error / bound {worst:.3f}')


# ------------------------------------------------------------------------------------------------ A4: masked losses
LOSS_SHAPES = [(8, 66752), (10, 65537), (2, 65536), (8, 534016), (1, 1), (3, 257)]


def loss_inputs(E, M, seed, with_mask):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(E, M, generator=g) * 2.0
    y = torch.randn(M, generator=g)
    logp = torch.randn(M, generator=g) * 1.5
    mask = (torch.rand(M, generator=g) > 0.3).float() if with_mask else None
    if with_mask and M == 1:
        mask[:] = 1.0
    return q, y, logp, mask


def sum_bound(E, S):
    """|fp32 two-stage sum - exact| <= (E + 32) 2^-24 S, S the sum of magnitudes before any cancellation.  Per element E + 3
    roundings (E fused steps of the member loop, the mask product, alpha logp - r, its fused add); at most 9 serial adds per
    thread (534 016 rows = 9 trips of the grid-stride loop), 8 tree levels per 256-thread block, 9 in the finishing block over
    256 partials: E + 3 + 9 + 8 + 9 = E + 29 <= E + 32."""
    return (E + 32) * U24 * S


@pytest.mark.parametrize('with_mask', [True, False])
@pytest.mark.parametrize('E,M', LOSS_SHAPES)
def test_masked_losses_rows(ops, E, M, with_mask):
    """`ops.masked_q_loss` / `ops.masked_actor_loss` (SAC form and TD3 form with logp=None; mean and min reduction; upstream
    gradient != 1) against fp64: sums within `sum_bound`, gradients element-wise at 1e-6 of their largest."""
    q, y, logp, mask = loss_inputs(E, M, 11 * E + M % 1009, with_mask)
    la = torch.tensor([-0.7])
    alpha = math.exp(float(la[0]))
    qd, yd, lpd = q.double(), y.double(), logp.double()
    mk = torch.ones(M, dtype=torch.float64) if mask is None else mask.double()
    cm = None if mask is None else mask.cuda()
    ratios = {}
    # critic
    sq = ((qd - yd) ** 2).sum(0)
    qc = q.cuda().requires_grad_(True)
    got = ops.masked_q_loss(qc, y.cuda(), cm)
    (got * 1.5).backward()
    ref, S = (sq * mk).sum().item(), (sq * mk).sum().item()
    assert abs(got.item() - ref) <= sum_bound(E, S), f'critic sum {got.item()!r} vs {ref!r}, bound {sum_bound(E, S):.3e}'
    ratios['critic'] = abs(got.item() - ref) / max(sum_bound(E, S), 1e-300)
    ratios['critic dq'] = close(qc.grad, 2 * 1.5 * mk * (qd - yd), rtol=1e-6, atol_scale=1e-7, name='dq (critic)')
    # actor
    for use_logp in (True, False):
        for reduce_min in (False, True):
            red = qd.min(dim=0).values if reduce_min else qd.mean(dim=0)
            a = alpha if use_logp else 0.0
            ref = (mk * (a * lpd - red)).sum().item()
            S = (mk * (a * lpd.abs() + (red.abs() if reduce_min else qd.abs().mean(dim=0)))).sum().item()
            qc = q.cuda().requires_grad_(True)
            lc = logp.cuda().requires_grad_(True) if use_logp else None
            got, lps = ops.masked_actor_loss(lc, qc, cm, la.cuda(), use_logp, reduce_min)
            (got * 0.75).backward()
            nm = f'actor {"SAC" if use_logp else "TD3"} {"min" if reduce_min else "mean"}'
            assert abs(got.item() - ref) <= sum_bound(E, S), f'{nm}: sum {got.item()!r} vs {ref!r}, bound {sum_bound(E, S):.3e}'
            ratios[nm] = abs(got.item() - ref) / max(sum_bound(E, S), 1e-300)
            if use_logp:
                ref2, S2 = (mk * lpd).sum().item(), (mk * lpd.abs()).sum().item()
                assert abs(lps.item() - ref2) <= sum_bound(E, S2), f'{nm}: sum mask logp {lps.item()!r} vs {ref2!r}'
                ratios[nm + ' logp sum'] = abs(lps.item() - ref2) / max(sum_bound(E, S2), 1e-300)
                close(lc.grad, 0.75 * a * mk, rtol=1e-6, atol_scale=1e-7, name=nm + ' dlogp')
            if reduce_min:
                dq = torch.zeros(E, M, dtype=torch.float64)
                dq[torch.from_numpy(np.argmin(q.numpy(), axis=0)), torch.arange(M)] = -0.75 * mk
            else:
                dq = (-0.75 * mk / E).expand(E, M)
            ratios[nm + ' dq'] = close(qc.grad, dq, rtol=1e-6, atol_scale=1e-7, name=nm + ' dq')
    print(f'\n[masked losses E={E} M={M} mask={"given" if with_mask else "None"}] error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))


@pytest.mark.parametrize('E,M', [(8, 66752), (3, 257), (2, 65537)])
def test_actor_loss_min_ties(ops, E, M):
    """Several members exactly equal at the minimum in a third of the columns: the FIRST minimal member gets -g mask, every other
    member exactly 0 (include/resel_hip.h; expected from numpy.argmin, which documents first-occurrence), and each column of dq
    sums to -g mask exactly."""
    q, y, logp, mask = loss_inputs(E, M, 3 * E + M, True)
    qn = q.numpy()
    tied = np.arange(M) % 3 == 0
    am = np.argmin(qn, axis=0)
    for shift in (3, 5):                                       # copy the minimum into up to two other members, below and above it
        other = (am + shift) % E
        qn[other[tied], np.nonzero(tied)[0]] = qn[am[tied], np.nonzero(tied)[0]]
    n_tied = ((qn == qn.min(axis=0, keepdims=True)).sum(axis=0) > 1).sum()
    assert n_tied >= M / 4
    first = np.argmin(qn, axis=0)
    assert (first[tied] != am[tied]).any() or E == 1           # the first minimal member is not always the one the value came from
    g = 0.75
    qc, lc = torch.from_numpy(qn).cuda().requires_grad_(True), logp.cuda().requires_grad_(True)
    got, _ = ops.masked_actor_loss(lc, qc, mask.cuda(), torch.tensor([-0.7]).cuda(), True, True)
    (got * g).backward()
    dq = torch.zeros(E, M)
    dq[torch.from_numpy(first), torch.arange(M)] = -g * mask
    assert torch.equal(qc.grad.cpu(), dq), f'{int((qc.grad.cpu() != dq).sum())} elements of dq differ from first-minimum-takes-all'
    assert torch.equal(qc.grad.cpu().sum(dim=0), -g * mask)
    print(f'\n[actor min ties E={E} M={M}] {int(n_tied)} tied columns')


# ------------------------------------------------------------------------------------------------ A5: optimizer tail
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
ADAM_N = [1, 255, 257, 10007, 5000001]


def segment_table(n, nseg, seed):
    """(ends int64 [k], lr fp32 [k], wd fp32 [k]) with k = min(nseg, n) segments.  The 40-segment table has ends on a multiple of
    the 256-thread block, one below and one above it (which makes two segments of length 1), the rest drawn at random; learning
    rates and weight decays are distinct per segment, some of them zero."""
    rs = np.random.RandomState(seed)
    k = min(nseg, n)
    if k == 1:
        ends = [n]
    elif k == 2:
        ends = [int(rs.randint(1, n)), n]
    else:
        blk = 256 * max(1, (n // 256) // 2)
        ends = {e for e in (blk - 1, blk, blk + 1) if 0 < e < n}
        while len(ends) < k - 1:
            ends.add(int(rs.randint(1, n)))
        ends = sorted(ends) + [n]
    lr = 10.0 ** rs.uniform(-4, -2, size=k)
    wd = rs.uniform(0.001, 0.1, size=k)
    lr[3::5] = 0.0
    wd[1::4] = 0.0
    if k <= 2:
        lr, wd = np.array([1e-2, 3e-3][:k]), np.array([0.0, 0.01][:k])
    return torch.tensor(ends, dtype=torch.int64), torch.tensor(lr, dtype=torch.float32), torch.tensor(wd, dtype=torch.float32)


def adam_ref_step(p0, g, m0, v0, step, ends, lr, wd, gs):
    """oracle.kernels.adamw_ref in fp64, segment by segment, from the fp32 state (p0, m0, v0); every float of the C ABI enters as
    its fp32 value.  Returns p, m, v, the scaled gradient and d p / d m = (lr / bc1) / denom per element."""
    gd = g.double() * (1.0 if gs is None else float(gs))
    b1, b2 = f32(BETA1), f32(BETA2)
    outs = [torch.empty_like(gd) for _ in range(4)]
    a = 0
    for e, l, w in zip(ends.tolist(), lr.tolist(), wd.tolist()):
        r = K.adamw_ref(p0[a:e].double(), gd[a:e], m0[a:e].double(), v0[a:e].double(), step, l, b1, b2, f32(EPS), w)
        for o, x in zip(outs, r):
            o[a:e] = x
        outs[3][a:e] = (l / (1 - b1 ** step)) / (r[2].sqrt() / math.sqrt(1 - b2 ** step) + f32(EPS))
        a = e
    return outs[0], outs[1], outs[2], gd, outs[3]


def _adam_cases():
    return [(n, k, gs) for n in ADAM_N for k in (1, 2, 40) if k == 1 or n >= 255 for gs in ('none', 'count', 'clip')]


@pytest.mark.parametrize('n,nseg,gs_kind', _adam_cases())
def test_adamw_flat_both_entry_points(ops, n, nseg, gs_kind):
    """`ops.adamw_flat_` (bias corrections taken on the host) and `ops.adamw_flat_dev_` (read from device memory, computed the way
    FlatAdamW.prepare_step does) against fp64 AdamW per segment: steps 1, 2, 3 chained from zero moments, then one step at
    t = 100 000 from non-zero moments.  Every step starts both entry points and the reference from the same fp32 state (the host
    form's), so each bound is that of ONE step:
      m   1e-6 (|beta1 m_old| + |(1 - beta1) g|)          v   rel 1e-6
      p   |p - p_ref| <= 1e-4 |step_ref| + 2^-22 |p_ref| + (lr / bc1) / denom * 2^-22 (|beta1 m_old| + |(1 - beta1) g|),
          step_ref = p_ref - p_old: the fp32 bar on the STEP; 2^-22 |p| for the three roundings p itself takes (1 - lr wd, the
          product, the subtraction); the third term is what the roundings of the first moment cost p when its two addends
          cancel.  fp32 forms m = beta1 m_old + (1 - beta1) (g * scale) with at most four roundings (g * scale, the two
          products, the sum), each 2^-24 of an addend or of the smaller sum: |dm| <= 3 x 2^-24 (|a| + |b|) <= 2^-22 (|a| + |b|),
          and p moves by (lr / bc1) / denom per unit of m.  Where the addends do not cancel this adds 0.24 % to the first term;
          where they do, no fp32 AdamW can do better.  Measured with the first two terms alone (n = 5 000 001, 40 segments,
          1 / 66 752 scale, t = 100 000): ONE element of 5 000 001 at 1.51x - beta1 m_old = -0.119744, (1 - beta1) g = +0.119740,
          m = -4.6e-6, so one rounding of an addend is 3e-3 of m and of the step; the ratio to those two terms is still printed.
      the two entry points among themselves: 2e-5 |step_ref| + 2^-22 |p_ref| (the same m in both, so no third term)."""
    ends, lr, wd = segment_table(n, nseg, seed=n % 1000 + nseg)
    g = torch.Generator().manual_seed(n % 1013 + 3 * nseg)
    p = torch.randn(n, generator=g)
    grad_unit = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 3 - 2)
    gs = None
    if gs_kind != 'none':                                       # 1 / valid count of the benchmark's update, as a device scalar
        gs = torch.tensor([1.0]) / torch.tensor([66752.0])
        if gs_kind == 'clip':
            gs = gs * torch.tensor([0.37])                      # times a clip coefficient < 1
        grad_unit = grad_unit * 66752.0
    gsc = None if gs is None else gs.cuda()
    dv = lambda *ts: [t.cuda() for t in ts]
    cends, clr, cwd = dv(ends, lr, wd)
    state = dv(p, torch.zeros(n), torch.zeros(n))
    b1, b2 = f32(BETA1), f32(BETA2)
    worst = {'m': 0.0, 'v': 0.0, 'p': 0.0, 'p / first two terms': 0.0, 'agree': 0.0}
    plan = [(1, None), (2, None), (3, None), (100000, (torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.05 + 1e-4))]
    for step, moments in plan:
        if moments is not None:
            state[1], state[2] = dv(*moments)
        grad = grad_unit * (1.0 + 0.25 * (step % 7))
        cg = grad.cuda()
        p0, m0, v0 = (t.cpu() for t in state)
        host = [t.clone() for t in state]
        devs = [t.clone() for t in state]
        ops.adamw_flat_(host[0], cg, host[1], host[2], cends, clr, cwd, step, BETA1, BETA2, EPS, gsc)
        t = float(step)
        bc = torch.tensor([1.0 - BETA1 ** t, (1.0 - BETA2 ** t) ** 0.5], dtype=torch.float32).cuda()      # FlatAdamW.prepare_step
        ops.adamw_flat_dev_(devs[0], cg, devs[1], devs[2], cends, clr, cwd, bc, BETA1, BETA2, EPS, gsc)
        pr, mr, vr, gd, dp_dm = adam_ref_step(p0, grad, m0, v0, step, ends, lr, wd, None if gs is None else gs.item())
        addends = (b1 * m0.double()).abs() + ((1 - b1) * gd).abs()
        m_bound = 1e-6 * addends
        p_bound = lambda rt: rt * (pr - p0.double()).abs() + U22 * pr.abs()
        p_full = p_bound(1e-4) + dp_dm * U22 * addends
        for nm, st in (('host', host), ('dev', devs)):
            worst['m'] = max(worst['m'], within(st[1], mr, m_bound, f'm ({nm}, step {step})'))
            worst['v'] = max(worst['v'], within(st[2], vr, 1e-6 * vr.abs(), f'v ({nm}, step {step})'))
            worst['p'] = max(worst['p'], within(st[0], pr, p_full, f'p ({nm}, step {step})'))
            worst['p / first two terms'] = max(worst['p / first two terms'], ((st[0].double().cpu() - pr).abs() / p_bound(1e-4).clamp_min(1e-300)).max().item())
        worst['agree'] = max(worst['agree'], within(host[0], devs[0].double().cpu(), p_bound(2e-5), f'p host vs dev, step {step}'))
        state = host
    print(f'\n[adamw n={n} segments={ends.numel()} grad_scale={gs_kind}] error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('n', [1, 255, 65537, 5000001])
def test_sumsq_rows(ops, n):
    """Sum of squares of inputs spanning four decades against the fp64 sum at (ceil(n / 65 536) + 32) 2^-24 relative: all terms
    positive; per element the square and ceil(n / 65 536) serial adds at most, then 8 + 8 tree levels."""
    g = torch.Generator().manual_seed(n % 911)
    x = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 4 - 2)
    ref = (x.double() ** 2).sum().item()
    got = ops.sumsq(x.cuda()).item()
    bound = (math.ceil(n / 65536) + 32) * U24 * ref
    assert abs(got - ref) <= bound, f'sumsq {got!r} vs {ref!r}: off by {abs(got - ref) / ref:.3e} relative, bound {bound / ref:.3e}'
    print(f'\n[sumsq n={n}] error / bound: {abs(got - ref) / bound:.3f}')


@pytest.mark.parametrize('tau', [0.995, 0.0, 1.0])
@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 1023, 10007, 5000001])
def test_soft_update_rows(ops, n, tau):
    """target <- tau target + (1 - tau) online against fp64 (tau as its fp32 value, 1 - tau is then exact) at
    2^-22 (|tau t| + |(1 - tau) s|); the tail of a longer backing buffer stays untouched."""
    g = torch.Generator().manual_seed(n % 907)
    pad = 7
    tgt, src = torch.randn(n + pad, generator=g), torch.randn(n + pad, generator=g)
    ct, cs = tgt.cuda(), src.cuda()
    ops.soft_update_(ct[:n], cs[:n], tau)
    tf = f32(tau)
    a, b = tf * tgt[:n].double(), (1 - tf) * src[:n].double()
    r = within(ct[:n], a + b, U22 * (a.abs() + b.abs()), f'soft_update n={n} tau={tau}')
    assert torch.equal(ct[n:].cpu(), tgt[n:]) and torch.equal(cs.cpu(), src)
    if tau == 0.0:
        assert torch.equal(ct[:n].cpu(), src[:n])
    if tau == 1.0:
        assert torch.equal(ct[:n].cpu(), tgt[:n])
    print(f'\n[soft_update n={n} tau={tau}] error / bound: {r:.3f}')


def test_soft_update_refuses_a_misaligned_view(ops):
    """The kernel moves float4: a view that does not start on 16 bytes is an error (RESEL_EINVAL), not a slower path."""
    flat, src = torch.arange(64.0).cuda(), torch.ones(64).cuda()
    for t, s in ((flat[1:], src[1:]), (flat[1:], src[:63]), (flat[:63], src[1:])):
        with pytest.raises(RuntimeError, match='soft_update'):
            ops.soft_update_(t, s, 0.5)
    assert torch.equal(flat.cpu(), torch.arange(64.0))
