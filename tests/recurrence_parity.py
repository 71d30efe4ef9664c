"""What holds the linear recurrences (csrc/linrec_scan.hip: gilr, gilr_lstm's second stage, lru) and the GRU (csrc/gru_seq.hip) to
fp64 per (row, 64-step time block) instead of per tensor, with carried-in states that are alive.  Shared by
tests/test_recurrence_fp64_gpu.py (the kernels, on the GPU) and tests/test_recurrence_parity_host.py (the models, the fp32 emulation
and its mutants, on the CPU).

`real_scan` / `complex_scan` / `gru_scan`
    forward AND backward of one recurrence written out step by step, in the recursions the kernels use (linrec_scan.hip:96, :219;
    gru_seq.hip:360-372).  One body serves two readers:
      * `reference(case)`: float64, one segment, exact tanh / sigmoid - the model the GPU results are compared with.  The host test
        checks it against autograd through `oracle.kernels.linrec_real_ref / linrec_complex_ref / gru_seq_ref`.
      * `emulate(case, mutant=None)`: float32 in the kernels' arithmetic - two passes over `NST = 1024 / CL` time segments of
        ceil(L / NST) steps, carries composed in the kernel's order (linrec_scan.hip:80, :132, :196, :256), the explicit FMAs of the real
        scan as exact product + one rounding, tanh as (1 - e) / (1 + e) with e = exp(-2|x|) and sigmoid as 1 / (1 + exp(-x)), each
        division a reciprocal and a product, per-segment partial sums of the lru parameter gradients.  It is what a correct fp32
        kernel may return (the compiler's own contractions and the 1-ulp hardware exp / rcp are not reproduced: the factor 8 below).
        `mutant=` breaks it the way a wrong kernel would, see MUTANTS.
    Both return the parameter-gradient sums together with S = sum |term| of each sum: `S_dlam_re`, `S_dlam_im`, `S_dgamma` per channel
    over (b, t); `S_db_hh` per gate unit; `S_dw_hh` = |dgh|^T |h_prev| per element.
`sliced_fraction`  worst max|got - ref| / (tol * max|ref|) over (row b, 64-step time block) slices.  A slice whose reference is exactly
    0 cannot be scaled: it is skipped, counted, and `got` has to be exactly 0 there (inf otherwise).  At most SKIP_CAP of a case's slices
    may be skipped; the one structural exception is `expected_zero_slices`.
`sum_fraction`     worst |got - ref| / (tol * S) per element of a parameter gradient.
`CASES`            the table both test files run; `ROUTE` names the kernel instantiation a case reaches.

Bounds.  Ceilings are the project's fp32 bars (tests/test_hip_ops.py): 1e-4 forward, 2.5e-4 = close(2e-4, 5e-5) for gradients, applied
per slice, and 2.5e-4 * S for sums.  The working bound of an output is 8 x the worst fraction the fp32 emulation reaches over the
whole table (EMULATION_WORST, measured on the CPU; asserted by the host test), rounded up to one significant digit, never above the
ceiling.  The 8 covers v_exp_f32 / v_rcp_f32 at 1 ulp where libm is near half an ulp, and FMA contraction.  It measures the
reference's own error, not the kernels'."""
import functools
import math

import torch

from oracle import kernels as K

FWD_CEIL, GRAD_CEIL, SUM_CEIL = 1e-4, 2.5e-4, 2.5e-4
BLOCK = 64
SKIP_CAP = 0.02
MODEL_SHARE, MUTANT_FACTOR = 0.5, 3.0

FWD_OUTPUTS = ('h', 'hr', 'hi')
SUM_OUTPUTS = ('dlam_re', 'dlam_im', 'dgamma', 'dw_hh', 'db_hh')
OUTPUTS = {'gilr': ('h', 'dv', 'df'), 'gilr_noact': ('h', 'dv', 'df'),
           'lru': ('hr', 'hi', 'dvr', 'dvi', 'dlam_re', 'dlam_im', 'dgamma'),
           'gru': ('h', 'dgi', 'dw_hh', 'db_hh')}

# worst fraction-of-1 error (the `tol = 1` reading of the metrics above) of `emulate` against `reference` over all cases of a kind,
# measured on the CPU (profiles/r28_recurrence_fp64_tests.md has every case); tests/test_recurrence_parity_host.py asserts that no
# case exceeds its entry.
EMULATION_WORST = {
    'gilr': {'h': 8.31e-7, 'dv': 6.42e-7, 'df': 8.65e-7},
    'gilr_noact': {'h': 4.42e-7, 'dv': 2.06e-7, 'df': 2.56e-7},
    'lru': {'hr': 8.64e-7, 'hi': 8.52e-7, 'dvr': 8.00e-7, 'dvi': 9.05e-7, 'dlam_re': 8.28e-7, 'dlam_im': 7.06e-7, 'dgamma': 1.90e-7},
    'gru': {'h': 4.07e-7, 'dgi': 6.06e-7, 'dw_hh': 1.26e-6, 'db_hh': 3.91e-7},
}


def ceiling(out):
    return FWD_CEIL if out in FWD_OUTPUTS else (SUM_CEIL if out in SUM_OUTPUTS else GRAD_CEIL)


def round_up_1sig(x):
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x))
    m = math.ceil(x / 10 ** e - 1e-9)
    return float(f'{m}e{e}')


def working_bound(kind, out):
    """8 x the emulation's worst, rounded up to one significant digit, capped by the project's ceiling."""
    return min(ceiling(out), round_up_1sig(8.0 * EMULATION_WORST[kind][out]))


# outputs whose working bound a correct kernel exceeds on the MI355X while under the ceiling: (kind, output) -> (bound <= ceiling, reason
# read in the code).  Empty: the measured run stays at 0.15 of every working bound (profiles/r28_recurrence_fp64_tests.md).
RAISED = {}


def bound(kind, out):
    return RAISED[(kind, out)][0] if (kind, out) in RAISED else working_bound(kind, out)


# --------------------------------------------------------------------------------------------------------------- case table
def pick_cl(B, C):
    """csrc/linrec_scan.hip `pick_cl`: channels per wave; NST = 1024 / CL time segments."""
    if ((C + 63) // 64) * B >= 256:
        return 64
    if ((C + 31) // 32) * B >= 256:
        return 32
    return 16


# route, B, C, L, decay, reset probability.  The smallest shapes that reach each instantiation with a partly filled last channel block
# (C = 40 = 2.5 x 16, 120 = 3.75 x 32, 250 = 3.9 x 64); L = 1, 2: fewer steps than segments; 63 / 64 / 65: one step per segment with the last
# segment empty / full / two steps per segment with half of the segments empty; 130: three steps, 20 empty segments.
_SHAPES = [
    ('cl16', 2, 40, 1, 'fast', 0.03), ('cl16', 2, 40, 2, 'fast', 0.03), ('cl16', 2, 40, 63, 'slow', 0.03),
    ('cl16', 2, 40, 64, 'fast', 0.03), ('cl16', 2, 40, 65, 'slow', 0.03), ('cl16', 2, 40, 130, 'slow', 0.03),
    ('cl32', 64, 120, 33, 'fast', 0.03), ('cl32', 64, 120, 45, 'slow', 0.03),
    ('cl64', 64, 250, 17, 'fast', 0.03), ('cl64', 64, 250, 40, 'slow', 0.03),
    ('long', 1, 48, 2003, 'slow', 0.0), ('longr', 1, 48, 2003, 'slow', 0.03),
]
_H0_CYCLE = ('both', 'r', 'i')
CASES = {}
for _i, (_route, _B, _C, _L, _decay, _p) in enumerate(_SHAPES):
    for _j, _kind in enumerate(('gilr', 'gilr_noact', 'lru')):
        CASES[f'{_kind}-{_route}-L{_L}'] = dict(kind=_kind, B=_B, C=_C, L=_L, decay=_decay, p_reset=_p, seed=2802 + 10 * _i + _j,
                                                h0=_H0_CYCLE[_i % 3] if _kind == 'lru' else 'both')
# continuation (one per layer kind): 150 steps = 64 segments of 3, split at 71 = no multiple of 3
for _j, _kind in enumerate(('gilr', 'lru')):
    CASES[f'{_kind}-cont-L150'] = dict(kind=_kind, B=2, C=40, L=150, decay='slow', p_reset=0.03, seed=2990 + _j, h0='both')
CONT_SPLIT = 71
# GRU: (3, 5, 32), (5, 4, 80) persistent form with a ragged 4-row group; (88, 3, 192), (344, 3, 48) one launch per step
for _i, (_B, _L, _H) in enumerate([(3, 5, 32), (5, 4, 80), (88, 3, 192), (344, 3, 48)]):
    for _h0 in ('both', 'none'):
        CASES[f'gru-B{_B}L{_L}H{_H}-h0{_h0}'] = dict(kind='gru', B=_B, C=_H, L=_L, seed=2950 + _i, h0=_h0)

LINREC_CASES = [n for n, c in CASES.items() if c['kind'] != 'gru']
GRU_CASES = [n for n, c in CASES.items() if c['kind'] == 'gru']


def cases_of(kind):
    return [n for n, c in CASES.items() if c['kind'] == kind]


def route(name):
    c = CASES[name]
    if c['kind'] == 'gru':
        grid = (c['C'] // 16) * ((c['B'] + 3) // 4)
        return f'gru {"persistent" if grid <= 256 else "per-step"} ({grid} workgroups, KC={gru_kc(c["C"])})'
    cl = pick_cl(c['B'], c['C'])
    return f'CL={cl} NST={1024 // cl} seg={-(-c["L"] // (1024 // cl))}'


def gru_kc(H):
    """Reduction elements per thread: H / KQ with KQ <= 16 pieces (tests/test_hip_ops.py `test_gru_seq_fwd_bwd_vs_aten`)."""
    return {32: 4, 48: 4, 64: 4, 80: 8, 192: 12, 256: 16, 384: 24, 512: 32}[H]


def make_start(B, L, g, p):
    """start[:, 0] = 0 on even rows (the carried-in state is alive) and 1 on odd rows; other resets with probability p."""
    s = (torch.rand(B, L, generator=g) < p).float() if p > 0 else torch.zeros(B, L)
    s[:, 0] = (torch.arange(B) % 2).float()
    return s


@functools.lru_cache(maxsize=None)
def make_case(name):
    """fp32 tensors of a case, drawn from its seed.  gilr: v, f pre-activation (f = randn + 3 'slow' / randn 'fast'); gilr_noact:
    v = sigmoid(.) tanh(.), f = sigmoid(.) as gilr_lstm's second stage passes them; lru: |lambda| in [0.9, 0.999], gamma = sqrt(1 -
    |lambda|^2); h0 at scale 2 (GRU: 1); upstream gradients randn."""
    c = dict(CASES[name])
    c['name'] = name
    B, L, C, kind = c['B'], c['L'], c['C'], c['kind']
    g = torch.Generator().manual_seed(c['seed'])
    r = lambda *s: torch.randn(*s, generator=g)
    if kind == 'gru':
        H = C
        c.update(gi=r(B, L, 3 * H), w_hh=r(3 * H, H) / math.sqrt(H), b_hh=r(3 * H) / math.sqrt(H), dh=r(B, L, H))
        h0 = r(B, H)
        c['h0_t'] = h0 if c['h0'] == 'both' else None
        return c
    c['start'] = make_start(B, L, g, c['p_reset'])
    shift = 3.0 if c['decay'] == 'slow' else 0.0
    if kind == 'gilr':
        c.update(v=r(B, L, C), f=r(B, L, C) + shift, h0_t=2 * r(B, C), dh=r(B, L, C))
    elif kind == 'gilr_noact':
        c.update(v=torch.sigmoid(r(B, L, C)) * torch.tanh(r(B, L, C)), f=torch.sigmoid(r(B, L, C) + shift), h0_t=2 * r(B, C), dh=r(B, L, C))
    else:
        mag, th = 0.9 + 0.099 * torch.rand(C, generator=g), 6.28 * torch.rand(C, generator=g)
        c.update(vr=r(B, L, C), vi=r(B, L, C), lam_re=mag * torch.cos(th), lam_im=mag * torch.sin(th), gamma=torch.sqrt(1 - mag ** 2),
                 dhr=r(B, L, C), dhi=r(B, L, C))
        h0r, h0i = 2 * r(B, C), 2 * r(B, C)
        c['h0r'] = h0r if c['h0'] in ('both', 'r') else None
        c['h0i'] = h0i if c['h0'] in ('both', 'i') else None
    return c


def old_style_case(kind, B=2, L=33, C=64):
    """Inputs drawn exactly as tests/test_hip_ops.py `test_gilr_scan_fwd_bwd` (fuse = True) / `test_lru_scan_fwd_bwd` draw them:
    start[:, 0] = 1 on every row; gilr with a random h0 that the reset gate multiplies by 0, lru without h0."""
    rnd = lambda *s: torch.randn(*s, generator=g)
    if kind == 'gilr':
        g = torch.Generator().manual_seed(L + C)
        v, f = rnd(B, L, C), rnd(B, L, C)
        start = (torch.rand(B, L, generator=g) < 0.03).float()
        start[:, 0] = 1
        h0 = rnd(B, C)
        return dict(name=f'old-gilr-{B}x{L}x{C}', kind='gilr', B=B, L=L, C=C, v=v, f=f, start=start, h0_t=h0, dh=rnd(B, L, C))
    g = torch.Generator().manual_seed(L + C + 1)
    vr, vi = rnd(B, L, C), rnd(B, L, C)
    mag, th = 0.9 + 0.099 * torch.rand(C, generator=g), 6.28 * torch.rand(C, generator=g)
    start = (torch.rand(B, L, generator=g) < 0.03).float()
    start[:, 0] = 1
    return dict(name=f'old-lru-{B}x{L}x{C}', kind='lru', B=B, L=L, C=C, vr=vr, vi=vi, lam_re=mag * torch.cos(th), lam_im=mag * torch.sin(th),
                gamma=torch.sqrt(1 - mag ** 2), start=start, h0r=None, h0i=None, dhr=rnd(B, L, C), dhi=rnd(B, L, C))


def time_slice(case, a, b, **h0):
    """The steps a .. b of a linrec case as a case of its own, with the given carried-in state (h0_t= / h0r=, h0i=)."""
    c = dict(case)
    for k in ('v', 'f', 'dh', 'vr', 'vi', 'dhr', 'dhi', 'start'):
        if k in c:
            c[k] = c[k][:, a:b].contiguous()
    c['L'] = b - a
    c['name'] = f'{case["name"]}[{a}:{b}]'
    c.update(h0)
    return c


# ------------------------------------------------------------------------------------------------------- shared arithmetic
MUTANTS = ('h0_fwd_zero',           # the forward's incoming state starts from 0 instead of h0
           'h0_bwd_zero',           # the backward reads 0 for h_{-1} at t = 0; the forward is right
           'carry_nearest',         # the forward composes only the nearest earlier segment's map (onto h0)
           'bwd_carry_dropped',     # the backward's g does not cross a segment boundary
           'start0_ignored')        # start[:, 0] is read as 0


def _fma(a, b, c):
    """fp32: the exact product plus one rounding (through fp64; the second rounding to fp32 differs from a true FMA only on ties)."""
    if a.dtype == torch.float32:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


def _tanh(x, kernel):
    if not kernel:
        return torch.tanh(x)
    e = torch.exp(-2.0 * x.abs())
    return torch.copysign((1.0 - e) * (1.0 / (1.0 + e)), x)


def _sigmoid(x, kernel):
    return 1.0 / (1.0 + torch.exp(-x)) if kernel else torch.sigmoid(x)


def _seg(x, nst, ln):
    """[B, L, ...] -> [B, nst, ln, ...], zero-padded in time."""
    B, L = x.shape[:2]
    pad = nst * ln - L
    if pad:
        x = torch.cat((x, x.new_zeros((B, pad) + tuple(x.shape[2:]))), dim=1)
    return x.reshape((B, nst, ln) + tuple(x.shape[2:]))


def _unseg(steps, L):
    """list over ln of [B, nst, C] -> [B, L, C]."""
    x = torch.stack(steps, dim=2)
    return x.reshape(x.shape[0], -1, x.shape[-1])[:, :L]


def _valid(L, nst, ln):
    return (torch.arange(nst * ln) < L).reshape(1, nst, ln, 1)


def _keep(case, dtype, mutant):
    keep = 1.0 - case['start'].to(dtype)
    if mutant == 'start0_ignored':
        keep = keep.clone()
        keep[:, 0] = 1.0
    return keep[:, :, None]                                                  # [B, L, 1]


def _carry_fwd(compose, x0, n, mutant):
    """Incoming state of each of n segments: x_w = map_{w-1}( ... map_0(x0)); `carry_nearest`: x_w = map_{w-1}(x0)."""
    xs = [x0]
    for w in range(n - 1):
        xs.append(compose(w, x0 if mutant == 'carry_nearest' else xs[-1]))
    return xs


# ----------------------------------------------------------------------------------------------------------- real recurrence
def real_scan(case, dtype=torch.float64, nst=1, kernel=False, mutant=None, **_):
    """-> dict(h, dv, df [B, L, C]) in `dtype`.  fuse_act = (case kind is 'gilr')."""
    act = case['kind'] == 'gilr'
    B, L, C = case['v'].shape
    ln = -(-L // nst)
    vraw, fraw, dh = case['v'].to(dtype), case['f'].to(dtype), case['dh'].to(dtype)
    keep = _keep(case, dtype, mutant)
    h0 = case['h0_t'].to(dtype) if case.get('h0_t') is not None else torch.zeros(B, C, dtype=dtype)
    vv = _tanh(vraw, kernel) if act else vraw
    sg = _sigmoid(fraw, kernel) if act else fraw
    fe = sg * keep
    ok = _valid(L, nst, ln)
    V, F = _seg(vv, nst, ln), _seg(fe, nst, ln)
    step = lambda i, x: torch.where(ok[:, :, i], _fma(F[:, :, i], x - V[:, :, i], V[:, :, i]), x)
    # ---- forward: pass 1 (segment -> affine map), carries, pass 2
    zero = torch.zeros(B, nst, C, dtype=dtype)
    a, hl = torch.ones(B, nst, C, dtype=dtype), zero
    if nst > 1:
        for i in range(ln):
            hl = step(i, hl)
            a = torch.where(ok[:, :, i], a * F[:, :, i], a)
    hin0 = torch.zeros_like(h0) if mutant == 'h0_fwd_zero' else h0
    hc = torch.stack(_carry_fwd(lambda w, x: _fma(a[:, w], x, hl[:, w]), hin0, nst, mutant), dim=1)
    hs = []
    for i in range(ln):
        hc = step(i, hc)
        hs.append(hc)
    h = _unseg(hs, L)
    # ---- backward: g_t = dh_t + f_{t+1} g_{t+1}
    fnext = torch.cat((fe[:, 1:], torch.zeros(B, 1, C, dtype=dtype)), dim=1)
    hzero = torch.zeros_like(h0) if mutant == 'h0_bwd_zero' else h0
    hprev = torch.cat((hzero[:, None], h[:, :-1]), dim=1)
    FN, DH = _seg(fnext, nst, ln), _seg(dh, nst, ln)
    a, gl = torch.ones(B, nst, C, dtype=dtype), zero
    if nst > 1:
        for i in reversed(range(ln)):
            gl = torch.where(ok[:, :, i], _fma(FN[:, :, i], gl, DH[:, :, i]), gl)
            a = torch.where(ok[:, :, i], a * FN[:, :, i], a)
    gins = [torch.zeros(B, C, dtype=dtype)]                                  # of the last segment
    for w in range(nst - 1, 0, -1):
        gins.append(torch.zeros(B, C, dtype=dtype) if mutant == 'bwd_carry_dropped' else _fma(a[:, w], gins[-1], gl[:, w]))
    g = torch.stack(gins[::-1], dim=1)
    gs = [None] * ln
    for i in reversed(range(ln)):
        g = torch.where(ok[:, :, i], _fma(FN[:, :, i], g, DH[:, :, i]), g)
        gs[i] = g
    g = _unseg(gs, L)
    gv = g * (1.0 - fe)
    gf = g * (hprev - vv) * keep
    if act:
        gv = gv * (1.0 - vv * vv)
        gf = gf * (sg * (1.0 - sg))
    return dict(h=h, dv=gv, df=gf)


# -------------------------------------------------------------------------------------------------------- complex recurrence
def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def complex_scan(case, dtype=torch.float64, nst=1, kernel=False, mutant=None, gamma=True):
    """-> dict(hr, hi, dvr, dvi [B, L, C]; dlam_re, dlam_im, dgamma [C] and their S_*) in `dtype` (S in float64).  gamma=False is the
    `gamma=None` call: gm = 1, no dgamma."""
    B, L, C = case['vr'].shape
    ln = -(-L // nst)
    vr, vi, dhr, dhi = (case[k].to(dtype) for k in ('vr', 'vi', 'dhr', 'dhi'))
    lr, li = case['lam_re'].to(dtype), case['lam_im'].to(dtype)
    gm = case['gamma'].to(dtype) if gamma else torch.ones(C, dtype=dtype)
    keep = _keep(case, dtype, mutant)
    z = torch.zeros(B, C, dtype=dtype)
    h0r = case['h0r'].to(dtype) if case.get('h0r') is not None else z
    h0i = case['h0i'].to(dtype) if case.get('h0i') is not None else z
    ok = _valid(L, nst, ln)
    FR, FI = _seg(lr * keep, nst, ln), _seg(li * keep, nst, ln)
    XR, XI = _seg(gm * vr, nst, ln), _seg(gm * vi, nst, ln)
    zero, one = torch.zeros(B, nst, C, dtype=dtype), torch.ones(B, nst, C, dtype=dtype)

    def fstep(i, cr, ci):
        nr = cr * FR[:, :, i] - ci * FI[:, :, i] + XR[:, :, i]
        ni = cr * FI[:, :, i] + ci * FR[:, :, i] + XI[:, :, i]
        return torch.where(ok[:, :, i], nr, cr), torch.where(ok[:, :, i], ni, ci)

    ar, ai, cr, ci = one, zero, zero, zero
    if nst > 1:
        for i in range(ln):
            cr, ci = fstep(i, cr, ci)
            pr, pi = _cmul(ar, ai, FR[:, :, i], FI[:, :, i])
            ar, ai = torch.where(ok[:, :, i], pr, ar), torch.where(ok[:, :, i], pi, ai)
    x0 = (z, z) if mutant == 'h0_fwd_zero' else (h0r, h0i)

    def compose(a_r, a_i, c_r, c_i):
        return lambda w, x: (a_r[:, w] * x[0] - a_i[:, w] * x[1] + c_r[:, w], a_r[:, w] * x[1] + a_i[:, w] * x[0] + c_i[:, w])

    xs = _carry_fwd(compose(ar, ai, cr, ci), x0, nst, mutant)
    cr, ci = torch.stack([x[0] for x in xs], dim=1), torch.stack([x[1] for x in xs], dim=1)
    hrs, his = [], []
    for i in range(ln):
        cr, ci = fstep(i, cr, ci)
        hrs.append(cr)
        his.append(ci)
    hr, hi = _unseg(hrs, L), _unseg(his, L)
    # ---- backward: g_t = dh_t + conj(f_{t+1}) g_{t+1}
    kn = torch.cat((keep[:, 1:], torch.zeros(B, 1, 1, dtype=dtype)), dim=1)
    GR, GI = _seg(lr * kn, nst, ln), _seg(-li * kn, nst, ln)
    DR, DI = _seg(dhr, nst, ln), _seg(dhi, nst, ln)

    def bstep(i, gr, gi):
        nr = gr * GR[:, :, i] - gi * GI[:, :, i] + DR[:, :, i]
        ni = gr * GI[:, :, i] + gi * GR[:, :, i] + DI[:, :, i]
        return torch.where(ok[:, :, i], nr, gr), torch.where(ok[:, :, i], ni, gi)

    ar, ai, gr, gi = one, zero, zero, zero
    if nst > 1:
        for i in reversed(range(ln)):
            gr, gi = bstep(i, gr, gi)
            pr, pi = _cmul(ar, ai, GR[:, :, i], GI[:, :, i])
            ar, ai = torch.where(ok[:, :, i], pr, ar), torch.where(ok[:, :, i], pi, ai)
    comp = compose(ar, ai, gr, gi)
    gins = [(z, z)]
    for w in range(nst - 1, 0, -1):
        gins.append((z, z) if mutant == 'bwd_carry_dropped' else comp(w, gins[-1]))
    gr, gi = torch.stack([x[0] for x in gins[::-1]], dim=1), torch.stack([x[1] for x in gins[::-1]], dim=1)
    p0 = (z, z) if mutant == 'h0_bwd_zero' else (h0r, h0i)
    PR, PI = _seg(torch.cat((p0[0][:, None], hr[:, :-1]), dim=1), nst, ln), _seg(torch.cat((p0[1][:, None], hi[:, :-1]), dim=1), nst, ln)
    KT, VR, VI = _seg(keep.expand(B, L, 1).contiguous(), nst, ln), _seg(vr, nst, ln), _seg(vi, nst, ln)
    dlr, dli, dgm = zero, zero, zero                                         # per-(row, segment) partials, accumulated in time order
    S = [torch.zeros(B, nst, C, dtype=torch.float64) for _ in range(3)]
    grs, gis = [None] * ln, [None] * ln
    for i in reversed(range(ln)):
        gr, gi = bstep(i, gr, gi)
        grs[i], gis[i] = gr, gi
        m = ok[:, :, i].to(dtype)
        terms = (KT[:, :, i] * (gr * PR[:, :, i] + gi * PI[:, :, i]) * m, KT[:, :, i] * (gi * PR[:, :, i] - gr * PI[:, :, i]) * m,
                 (gr * VR[:, :, i] + gi * VI[:, :, i]) * m)
        dlr, dli, dgm = dlr + terms[0], dli + terms[1], dgm + terms[2]
        for s, t in zip(S, terms):
            s += t.double().abs()
    g_r, g_i = _unseg(grs, L), _unseg(gis, L)
    res = dict(hr=hr, hi=hi, dvr=gm * g_r, dvi=gm * g_i, dlam_re=dlr.sum(dim=(0, 1)), dlam_im=dli.sum(dim=(0, 1)),
               S_dlam_re=S[0].sum(dim=(0, 1)), S_dlam_im=S[1].sum(dim=(0, 1)))
    if gamma:
        res.update(dgamma=dgm.sum(dim=(0, 1)), S_dgamma=S[2].sum(dim=(0, 1)))
    return res


# ------------------------------------------------------------------------------------------------------------------------ GRU
def gru_scan(case, dtype=torch.float64, kernel=False, mutant=None, **_):
    """-> dict(h [B, L, H], dgi [B, L, 3H], dw_hh [3H, H], db_hh [3H], S_dw_hh, S_db_hh) with gru_seq.hip's step arithmetic
    (forward :139-152, backward :360-372) and `GruSeqFn.backward`'s parameter sums."""
    gi, w, b, dh_all = (case[k].to(dtype) for k in ('gi', 'w_hh', 'b_hh', 'dh'))
    B, L, H3 = gi.shape
    H = H3 // 3
    h0 = case['h0_t'].to(dtype) if case.get('h0_t') is not None else torch.zeros(B, H, dtype=dtype)
    h = torch.zeros_like(h0) if mutant == 'h0_fwd_zero' else h0
    hs, gates = [], []
    for t in range(L):
        a = h @ w.t()
        rg = _sigmoid(gi[:, t, :H] + a[:, :H] + b[:H], kernel)
        zg = _sigmoid(gi[:, t, H:2 * H] + a[:, H:2 * H] + b[H:2 * H], kernel)
        hn = a[:, 2 * H:] + b[2 * H:]
        ng = _tanh(gi[:, t, 2 * H:] + rg * hn, kernel)
        h = (1.0 - zg) * ng + zg * h
        hs.append(h)
        gates.append((rg, zg, ng, hn))
    h_all = torch.stack(hs, dim=1)
    hp0 = torch.zeros_like(h0) if mutant == 'h0_bwd_zero' else h0
    h_prev = torch.cat((hp0[:, None], h_all[:, :-1]), dim=1)
    carry = torch.zeros(B, H, dtype=dtype)
    dgi, dgh = [None] * L, [None] * L
    for t in reversed(range(L)):
        rg, zg, ng, hn = gates[t]
        dh = dh_all[:, t] + carry
        dn = dh * (1.0 - zg)
        dz_ = dh * (h_prev[:, t] - ng) * zg * (1.0 - zg)
        dn_ = dn * (1.0 - ng * ng)
        dr_ = dn_ * hn * rg * (1.0 - rg)
        dhn = dn_ * rg
        dgi[t] = torch.cat((dr_, dz_, dn_), dim=1)
        dgh[t] = torch.cat((dr_, dz_, dhn), dim=1)
        carry = dh * zg + dgh[t] @ w
    dgi, dgh = torch.stack(dgi, dim=1), torch.stack(dgh, dim=1)
    g2, p2 = dgh.reshape(-1, 3 * H), h_prev.reshape(-1, H)
    return dict(h=h_all, dgi=dgi, dw_hh=g2.t() @ p2, db_hh=g2.sum(dim=0),
                S_dw_hh=g2.double().abs().t() @ p2.double().abs(), S_db_hh=g2.double().abs().sum(dim=0))


_SCAN = {'gilr': real_scan, 'gilr_noact': real_scan, 'lru': complex_scan, 'gru': gru_scan}


def reference(case, **kw):
    """The fp64 model of a case (kw: gamma=False for the `gamma=None` call of lru)."""
    return _SCAN[case['kind']](case, **kw)


def emulate(case, mutant=None, **kw):
    """The fp32 emulation of the kernels' arithmetic on a case."""
    if case['kind'] == 'gru':
        return gru_scan(case, dtype=torch.float32, kernel=True, mutant=mutant)
    return _SCAN[case['kind']](case, dtype=torch.float32, nst=1024 // pick_cl(case['B'], case['C']), kernel=True, mutant=mutant, **kw)


@functools.lru_cache(maxsize=None)
def case_and_ref(name, gamma=True):
    case = make_case(name)
    return case, (reference(case, gamma=gamma) if case['kind'] == 'lru' else reference(case))


# --------------------------------------------------------------------------------------------------------------------- metric
def sliced_fraction(got, ref, tol, block=BLOCK):
    """got, ref [B, L, C] -> (worst over (row, time block) slices of max|got - ref| / (tol * max|ref|), slices, skipped slices).
    A slice whose reference is exactly 0 is skipped - and has to be exactly 0 in `got`.  inf where got is not finite."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    B, L, C = ref.shape
    nb = -(-L // block)
    if tuple(got.shape) != tuple(ref.shape) or not torch.isfinite(got).all():
        return float('inf'), B * nb, 0
    pad = nb * block - L
    blocks = lambda x: torch.cat((x, x.new_zeros(B, pad, C)), dim=1).reshape(B, nb, block * C).amax(dim=-1)
    err, mag = blocks((got - ref).abs()), blocks(ref.abs())
    dead = mag == 0
    if (err[dead] != 0).any():
        return float('inf'), B * nb, int(dead.sum())
    live = ~dead
    worst = float((err[live] / (tol * mag[live])).max()) if live.any() else 0.0
    return worst, B * nb, int(dead.sum())


def sum_fraction(got, ref, S, tol):
    """Parameter gradients: (worst |got - ref| / (tol * S) per element, elements, elements with S = 0)."""
    got, ref, S = got.detach().double().cpu(), ref.detach().double().cpu(), S.detach().double().cpu()
    if tuple(got.shape) != tuple(ref.shape) or not torch.isfinite(got).all():
        return float('inf'), ref.numel(), 0
    err = (got - ref).abs()
    dead = S == 0
    if (err[dead] != 0).any():
        return float('inf'), ref.numel(), int(dead.sum())
    live = ~dead
    return (float((err[live] / (tol * S[live])).max()) if live.any() else 0.0), ref.numel(), int(dead.sum())


def whole_fraction(got, ref, tol):
    """The metric of tests/test_hip_ops.py `close`: max|got - ref| / (tol * max|ref|) over the whole tensor."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (tol * ref.abs().max()))


def expected_zero_slices(case):
    """Slices that are zero by construction: with L = 1 the whole df slice of a row with start[b, 0] = 1 is g (h_prev - v) * 0."""
    if case['kind'] in ('gilr', 'gilr_noact') and case['L'] == 1:
        return int(case['start'][:, 0].sum())
    return 0


def fractions(case, got, ref, tol=None, outputs=None):
    """{output: fraction of its bound}, (slices, skipped) of a result dict against a reference dict.  tol=None: the bound the GPU test
    asserts; a number: that tolerance for every output (tol = 1 gives raw relative errors)."""
    kind = case['kind']
    fr, n, skipped = {}, 0, 0
    for out in outputs or OUTPUTS[kind]:
        if out not in ref:
            continue
        t = bound(kind, out) if tol is None else tol
        if out in SUM_OUTPUTS:
            f, a, b = sum_fraction(got[out], ref[out], ref['S_' + out], t)
        else:
            f, a, b = sliced_fraction(got[out], ref[out], t)
        fr[out] = f
        n, skipped = n + a, skipped + b
    return fr, (n, skipped)


def skip_cap_holds(case, n, skipped):
    return skipped <= max(int(SKIP_CAP * n), expected_zero_slices(case))
