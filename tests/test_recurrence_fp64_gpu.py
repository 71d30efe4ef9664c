"""The linear recurrences (csrc/linrec_scan.hip through ops.gilr_scan, gilr_scan_members, complex_scan, complex_scan_members) and the GRU
(csrc/gru_seq.hip through ops.gru_seq) against fp64, every (row, 64-step time block) slice held to its OWN scale and every parameter
gradient to the sum of the magnitudes it is formed from, with carried-in states that are alive: start[:, 0] = 0 on even rows, h0 at
scale 2.  tests/recurrence_parity.py has the models, the metric, the bounds and the case table - every kernel instantiation (CL = 16 / 32
/ 64 channels per wave) with a partly filled last channel block, fewer steps than time segments, empty segments, a 2003-step carry;
tests/test_recurrence_parity_host.py shows on the CPU that a correct fp32 scan uses at most half of each bound and that five wrong
kernels exceed them by orders of magnitude.

Beyond the bounds: rows whose start[b, 0] = 1 return the bits of the h0 = None run (fma(0, h0 - v, v) = v) while the other rows differ,
two runs of a call agree bit for bit, the strided forms leave the columns they do not own untouched, and a sequence split between two
calls - the state handed over as the non-contiguous view the layers return - matches the model of the unsplit sequence.

Every comparison prints `REC-FIG <case> <entry>:<output> <fraction of bound>` before anything is asserted (`pytest -s`); the fractions
measured on an MI355X are in profiles/r28_recurrence_fp64_tests.md."""
import pytest
import torch

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


def _figures(case, entry, got, ref):
    """Print every fraction of `got` against `ref`; -> the outputs over their bound (asserted empty by the caller, last)."""
    fr, _ = RP.fractions(case, got, ref)
    for out, f in fr.items():
        print(f'REC-FIG {case["name"]} [{RP.route(case["name"]) if case["name"] in RP.CASES else "-"}] {entry}:{out} {f:.4f} of {RP.bound(case["kind"], out):.0e}')
    return {out: f for out, f in fr.items() if not f <= 1.0}


def _state_rows(case, with_h0, without, key):
    """Rows with start[b, 0] = 1: the bits of the run without h0.  Rows with start[b, 0] = 0: they differ."""
    reset = case['start'][:, 0] == 1
    a, b = _bits(with_h0[key]).cpu(), _bits(without[key]).cpu()
    assert torch.equal(a[reset], b[reset]), f'{case["name"]} {key}: a row that starts with a reset depends on h0'
    assert (a[~reset] != b[~reset]).flatten(1).any(dim=1).all(), f'{case["name"]} {key}: a row that carries its state in does not see h0'


def _members(*blocks):
    """[B, L, C] blocks -> (the [E, B, L, C] strided view of one [B L, E C] matrix, as a shared-input EnsembleLinear leaves it)."""
    B, L, C = blocks[0].shape
    y2 = torch.cat([b.reshape(B * L, C) for b in blocks], dim=1).cuda()
    E = len(blocks)
    u = y2.as_strided((E, B, L, C), (C, L * E * C, E * C, 1))          # = y2.view(B L, E, C).transpose(0, 1).reshape(E, B, L, C), also at L = 1
    return u.requires_grad_(True)


# ------------------------------------------------------------------------------------------------------------------- real (gilr)
def _gilr(ops, case, h0):
    fuse = case['kind'] == 'gilr'
    v, f = _leaf(case['v']), _leaf(case['f'])
    h = ops.gilr_scan(v, f, _d(case['start']), _d(h0), fuse)
    dv, df = torch.autograd.grad(h, (v, f), _d(case['dh']))
    return dict(h=h.detach(), dv=dv, df=df)


@pytest.mark.parametrize('name', RP.cases_of('gilr') + RP.cases_of('gilr_noact'))
def test_gilr_scan_holds_every_row_and_block_to_fp64(ops, name):
    """fuse_act = True as gilr's first stage, False as gilr_lstm's second stage: post-activation operands and a live m0."""
    case, ref = RP.case_and_ref(name)
    got, again, none = _gilr(ops, case, case['h0_t']), _gilr(ops, case, case['h0_t']), _gilr(ops, case, None)
    over = _figures(case, 'gilr_scan', got, ref)
    assert not over, over
    assert _same(got, again), 'two runs differ'
    _state_rows(case, got, none, 'h')


@pytest.mark.parametrize('name', RP.cases_of('gilr'))
def test_gilr_scan_members_reads_the_shared_matrix_in_place(ops, name):
    case, ref = RP.case_and_ref(name)
    u = _members(case['v'], case['f'])
    h = ops.gilr_scan_members(u, _d(case['start']), _d(case['h0_t']), True)
    (du,) = torch.autograd.grad(h, u, _d(case['dh']))
    got = dict(h=h.detach(), dv=du[0], df=du[1])
    over = _figures(case, 'gilr_scan_members', got, ref)
    assert not over, over
    assert du.stride() == u.stride()
    assert _same(got, _gilr(ops, case, case['h0_t'])), 'the in-place form and the dense form differ'


# ------------------------------------------------------------------------------------------------------------------ complex (lru)
_LRU_OUT = ('hr', 'hi', 'dvr', 'dvi', 'dlam_re', 'dlam_im', 'dgamma')


def _lru(ops, case, gamma, h0r, h0i):
    ls = [_leaf(case[k]) for k in ('vr', 'vi', 'lam_re', 'lam_im')] + ([_leaf(case['gamma'])] if gamma else [])
    hr, hi = ops.complex_scan(ls[0], ls[1], ls[2], ls[3], ls[4] if gamma else None, _d(case['start']), _d(h0r), _d(h0i))
    gs = torch.autograd.grad((hr, hi), ls, (_d(case['dhr']), _d(case['dhi'])))
    return dict(zip(_LRU_OUT[2:], gs), hr=hr.detach(), hi=hi.detach())


@pytest.mark.parametrize('gamma', [True, False], ids=['gamma', 'gamma-None'])
@pytest.mark.parametrize('name', RP.cases_of('lru'))
def test_complex_scan_holds_every_row_and_block_to_fp64(ops, name, gamma):
    """The case table cycles h0 through (h0r and h0i), h0r only, h0i only; gamma = None is the gm = 1 path without a dgamma sum."""
    case, ref = RP.case_and_ref(name, gamma)
    run = lambda r, i: _lru(ops, case, gamma, r, i)
    got, again, none = run(case['h0r'], case['h0i']), run(case['h0r'], case['h0i']), run(None, None)
    over = _figures(case, f'complex_scan({"gamma" if gamma else "gamma=None"},h0={case["h0"]})', got, ref)
    assert not over, over
    assert ('dgamma' in got) == gamma
    assert _same(got, again), 'two runs differ'
    _state_rows(case, got, none, 'hr')
    _state_rows(case, got, none, 'hi')


@pytest.mark.parametrize('E', [2, 3])
@pytest.mark.parametrize('name', RP.cases_of('lru'))
def test_complex_scan_members_reads_the_shared_matrix_in_place(ops, name, E):
    case, ref = RP.case_and_ref(name)
    g = torch.Generator().manual_seed(case['seed'] + 5)
    skip_in, dskip = torch.randn(case['B'], case['L'], case['C'], generator=g), torch.randn(case['B'], case['L'], case['C'], generator=g).cuda()
    u = _members(case['vr'], case['vi'], *([skip_in] if E == 3 else []))
    lam3 = _leaf(torch.stack((case['lam_re'], case['lam_im'], case['gamma'])))
    h2, u2 = ops.complex_scan_members(u, lam3, _d(case['start']), _d(case['h0r']), _d(case['h0i']))
    dh2 = torch.stack((_d(case['dhr']), _d(case['dhi'])))
    du, dlam3 = torch.autograd.grad((h2,) + ((u2,) if E == 3 else ()), (u, lam3), (dh2,) + ((dskip,) if E == 3 else ()))
    got = dict(hr=h2[0].detach(), hi=h2[1].detach(), dvr=du[0], dvi=du[1], dlam_re=dlam3[0], dlam_im=dlam3[1], dgamma=dlam3[2])
    over = _figures(case, f'complex_scan_members(E={E})', got, ref)
    assert not over, over
    assert du.stride() == u.stride() and (u2 is None) == (E == 2)
    if E == 3:
        assert torch.equal(u2, u.detach()[2]) and torch.equal(du[2], dskip), 'the pass-through member'
    dense = _lru(ops, case, True, case['h0r'], case['h0i'])
    assert all(torch.equal(_bits(got[k]), _bits(dense[k])) for k in ('hr', 'hi', 'dvr', 'dvi')), 'the in-place form and the dense form differ'


# --------------------------------------------------------------------------------------------------------------------------- GRU
def _gru(ops, case):
    gi, w, b = _leaf(case['gi']), _leaf(case['w_hh']), _leaf(case['b_hh'])
    h = ops.gru_seq(gi, w, b, _d(case['h0_t']))
    dgi, dw, db = torch.autograd.grad(h, (gi, w, b), _d(case['dh']))
    return dict(h=h.detach(), dgi=dgi, dw_hh=dw, db_hh=db)


@pytest.mark.parametrize('name', RP.GRU_CASES)
def test_gru_seq_forward_and_backward_with_a_carried_in_state_to_fp64(ops, name):
    case, ref = RP.case_and_ref(name)
    got, again = _gru(ops, case), _gru(ops, case)
    over = _figures(case, 'gru_seq', got, ref)
    assert not over, over
    assert _same(got, again), 'two runs differ'
    if case['h0_t'] is not None:                                # the twin without h0 is another answer in every row
        twin = RP.case_and_ref(name.replace('h0both', 'h0none'))[1]
        assert ((ref['h'] - twin['h']).abs().flatten(1).amax(dim=1) > 1e-2).all()


# ------------------------------------------------------------------------------------------- columns the strided forms do not own
@pytest.mark.parametrize('name', ['gilr-cl16-L65', 'gilr-cl64-L17', 'lru-cl16-L65', 'lru-cl32-L33'])
def test_strided_gradients_leave_the_neighbouring_columns_alone(ops, name):
    """Operands and gradients as column blocks 0 and 2 of [B L, 3 C] matrices (ld = 3 C > C) whose middle block is NaN: the lanes
    c >= C of the partly filled last channel block would land there."""
    case, _ = RP.case_and_ref(name)
    B, L, C = case['B'], case['L'], case['C']
    nan = lambda: torch.full((B * L, 3 * C), float('nan'), device='cuda')
    blocks = lambda m: (m.view(B, L, 3 * C)[:, :, :C], m.view(B, L, 3 * C)[:, :, 2 * C:])
    X, G = nan(), nan()
    a, b = blocks(X)
    da, db = blocks(G)
    start = ops._flags(_d(case['start']), B, L)
    if case['kind'] == 'gilr':
        a.copy_(_d(case['v'])), b.copy_(_d(case['f']))
        h0 = ops._h0(_d(case['h0_t']), B, C)
        h = ops._real_fwd(a, b, 3 * C, start, h0, True)
        ops._real_bwd(a, b, 3 * C, start, h0, h, _d(case['dh']).contiguous(), da, db, 3 * C, True)
        dense = _gilr(ops, case, case['h0_t'])
        want = (dense['h'], dense['dv'], dense['df'])
        have = (h, da, db)
    else:
        a.copy_(_d(case['vr'])), b.copy_(_d(case['vi']))
        lr, li, gm, start, h0r, h0i = ops._complex_args(_d(case['lam_re']), _d(case['lam_im']), _d(case['gamma']), _d(case['start']),
                                                        _d(case['h0r']), _d(case['h0i']), B, L, C)
        h2, _ = ops._complex_fwd(a, b, 3 * C, lr, li, gm, start, h0r, h0i)
        dlam = torch.full((3, C), float('nan'), device='cuda')
        dh2 = torch.stack((_d(case['dhr']), _d(case['dhi']))).contiguous()
        ops._complex_bwd(a, b, 3 * C, lr, li, gm, start, h0r, h0i, h2, dh2, da, db, 3 * C, dlam[0], dlam[1], dlam[2])
        dense = _lru(ops, case, True, case['h0r'], case['h0i'])
        want = (dense['hr'], dense['hi'], dense['dvr'], dense['dvi'], dense['dlam_re'], dense['dlam_im'], dense['dgamma'])
        have = (h2[0], h2[1], da, db, dlam[0], dlam[1], dlam[2])
    torch.cuda.synchronize()
    assert torch.isnan(G[:, C:2 * C]).all() and torch.isnan(X[:, C:2 * C]).all(), 'a column outside the owned blocks was written'
    for i, (x, y) in enumerate(zip(have, want)):
        assert torch.equal(_bits(x), _bits(y)), f'output {i}: the strided form differs from the dense form'


# ------------------------------------------------------------------------------------------------------------------ continuation
def test_gilr_continues_a_split_sequence_from_the_state_the_layer_returns(ops):
    """GILRLayer's protocol: hidden = h[:, -1:, :].transpose(0, 1), the next call's h0 = hidden[0] (a non-contiguous [B, C] view),
    detached as the trainer detaches carried states.  150 steps run as 64 segments of 3; 71 is no segment edge."""
    case, whole = RP.case_and_ref('gilr-cont-L150')
    s, L = RP.CONT_SPLIT, case['L']
    first = RP.time_slice(case, 0, s)
    second = RP.time_slice(case, s, L, h0_t=whole['h'][:, s - 1])
    refs = (RP.reference(first), RP.reference(second))
    over, hidden = {}, case['h0_t'].cuda()[None]
    for part, ref, (a, b) in zip((first, second), refs, ((0, s), (s, L))):
        u = _members(part['v'], part['f'])
        h0 = hidden[0].detach()
        h = ops.gilr_scan_members(u, _d(part['start']), h0, True)
        (du,) = torch.autograd.grad(h, u, _d(part['dh']))
        assert a == 0 or not h0.is_contiguous()
        hidden = h.detach()[:, -1:, :].transpose(0, 1)
        got = dict(h=h.detach(), dv=du[0], df=du[1])
        over.update({f'{a}:{b} {k}': f for k, f in _figures(part, f'continuation[{a}:{b}]', got, dict(ref, h=whole['h'][:, a:b])).items()})
    assert not over, over


def test_lru_continues_a_split_sequence_from_the_state_the_layer_returns(ops):
    """LRULayer's protocol: hidden = cat(hr[:, -1:], hi[:, -1:], -1).transpose(0, 1); h0r, h0i = hidden[0].chunk(2, -1)."""
    case, whole = RP.case_and_ref('lru-cont-L150')
    s, L = RP.CONT_SPLIT, case['L']
    first = RP.time_slice(case, 0, s)
    second = RP.time_slice(case, s, L, h0r=whole['hr'][:, s - 1], h0i=whole['hi'][:, s - 1])
    refs = (RP.reference(first), RP.reference(second))
    over, hidden = {}, torch.cat((case['h0r'], case['h0i']), dim=-1).cuda()[None]
    for part, ref, (a, b) in zip((first, second), refs, ((0, s), (s, L))):
        u = _members(part['vr'], part['vi'])
        lam3 = _leaf(torch.stack((part['lam_re'], part['lam_im'], part['gamma'])))
        h0r, h0i = hidden[0].detach().chunk(2, dim=-1)
        h2, _ = ops.complex_scan_members(u, lam3, _d(part['start']), h0r, h0i)
        du, dlam3 = torch.autograd.grad(h2, (u, lam3), torch.stack((_d(part['dhr']), _d(part['dhi']))))
        hidden = torch.cat((h2.detach()[0][:, -1:, :], h2.detach()[1][:, -1:, :]), dim=-1).transpose(0, 1)
        assert not h0r.is_contiguous()
        got = dict(hr=h2[0].detach(), hi=h2[1].detach(), dvr=du[0], dvi=du[1], dlam_re=dlam3[0], dlam_im=dlam3[1], dgamma=dlam3[2])
        ref = dict(ref, hr=whole['hr'][:, a:b], hi=whole['hi'][:, a:b])
        over.update({f'{a}:{b} {k}': f for k, f in _figures(part, f'continuation[{a}:{b}]', got, ref).items()})
    assert not over, over
