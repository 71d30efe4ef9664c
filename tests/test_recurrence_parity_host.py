"""Host side of the per-(row, 64-step block) comparison of the recurrences (tests/recurrence_parity.py; the GPU side is
tests/test_recurrence_fp64_gpu.py).

1. The fp64 models agree with autograd through `oracle.kernels.linrec_real_ref / linrec_complex_ref / gru_seq_ref` on every case.
2. The fp32 emulation of the kernels' arithmetic stays at <= 0.5 of every bound the GPU test holds the kernels to, in the same metric
   on the same data, and its worst figures are the ones `EMULATION_WORST` records (the working bounds are 8 x those).
3. Each mutant of the emulation exceeds the bound of a named output at least threefold on a named case (MUTANT_TABLE).
4. The h0 mutants are invisible - bit for bit - on inputs drawn as tests/test_hip_ops.py `test_gilr_scan_fwd_bwd` draws them
   (start[:, 0] = 1 on every row), and the start[:, 0] mutant on inputs drawn as `test_lru_scan_fwd_bwd` draws them (no h0): the hole
   those tests leave.  (With the gilr draw a kernel that ignores start[:, 0] lets the random h0 in and is seen.)
5. The metric: skip cap, no all-zero reference, one wrong element of a quiet slice.
Every figure is printed as `REC-FIG` before it is asserted (profiles/r28_recurrence_fp64_tests.md keeps them)."""
import pytest
import torch

import recurrence_parity as RP
from oracle import kernels as K


@pytest.fixture(scope='module', autouse=True)
def sixteen_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))
    yield
    torch.set_num_threads(before)


def _variants(name):
    return (True, False) if RP.CASES[name]['kind'] == 'lru' else (True,)


def _leaf(t):
    return None if t is None else t.double().requires_grad_(True)


def _autograd(case, gamma=True):
    """The outputs of a case through the oracle functions on fp64 leaves."""
    kind = case['kind']
    if kind in ('gilr', 'gilr_noact'):
        v, f = _leaf(case['v']), _leaf(case['f'])
        h, _ = K.linrec_real_ref(v, f, case['start'].double(), case['h0_t'].double(), kind == 'gilr')
        dv, df = torch.autograd.grad(h, (v, f), case['dh'].double())
        return dict(h=h.detach(), dv=dv, df=df)
    if kind == 'lru':
        ls = [_leaf(case[k]) for k in ('vr', 'vi', 'lam_re', 'lam_im')] + ([_leaf(case['gamma'])] if gamma else [])
        h0r, h0i = (None if case[k] is None else case[k].double() for k in ('h0r', 'h0i'))
        hr, hi = K.linrec_complex_ref(ls[0], ls[1], ls[2], ls[3], case['start'].double(), h0r, h0i, ls[4] if gamma else None)
        gs = torch.autograd.grad((hr * case['dhr'].double()).sum() + (hi * case['dhi'].double()).sum(), ls)
        return dict(zip(('dvr', 'dvi', 'dlam_re', 'dlam_im', 'dgamma'), gs), hr=hr.detach(), hi=hi.detach())
    gi, w, b = _leaf(case['gi']), _leaf(case['w_hh']), _leaf(case['b_hh'])
    h = K.gru_seq_ref(gi, w, b, None if case['h0_t'] is None else case['h0_t'].double())
    dgi, dw, db = torch.autograd.grad(h, (gi, w, b), case['dh'].double())
    return dict(h=h.detach(), dgi=dgi, dw_hh=dw, db_hh=db)


@pytest.mark.parametrize('name', list(RP.CASES))
def test_fp64_models_agree_with_autograd_through_the_oracle(name):
    for gamma in _variants(name):
        case, ref = RP.case_and_ref(name, gamma)
        auto = _autograd(case, gamma)
        assert set(auto) == {k for k in ref if not k.startswith('S_')}
        for out, a in auto.items():
            if out in RP.SUM_OUTPUTS:                                   # a sum in another order: held to its own S
                S = ref['S_' + out]
                assert ((ref[out] - a).abs() <= 1e-12 * S).all(), (name, out)
                assert (S >= ref[out].abs() * (1 - 1e-12)).all() and (S > 0).all(), (name, out)
            else:
                assert (ref[out] - a).abs().max() <= 1e-12 * a.abs().max(), (name, out)


@pytest.mark.parametrize('name', list(RP.CASES))
def test_emulation_uses_at_most_half_of_every_bound_and_skips_almost_nothing(name):
    for gamma in _variants(name):
        case, ref = RP.case_and_ref(name, gamma)
        emu = RP.emulate(case, gamma=gamma)
        fr, (n, skipped) = RP.fractions(case, emu, ref)
        raw, _ = RP.fractions(case, emu, ref, tol=1.0)
        tag = '' if gamma else '(gamma=None)'
        for out in fr:
            print(f'REC-FIG {name}{tag} [{RP.route(name)}] emulation:{out} {fr[out]:.4f} of {RP.bound(case["kind"], out):.0e} (raw {raw[out]:.2e})')
        print(f'REC-FIG {name}{tag} skipped {skipped} of {n}')
        assert all(f <= RP.MODEL_SHARE for f in fr.values()), fr
        assert all(raw[out] <= RP.EMULATION_WORST[case['kind']][out] * 1.25 for out in raw), raw
        assert RP.skip_cap_holds(case, n, skipped), (n, skipped)
        assert all(float(ref[out].abs().max()) > 0 for out in fr), 'an all-zero reference'


def test_recorded_emulation_maxima_are_the_measured_ones_and_no_bound_exceeds_its_ceiling():
    worst = {}
    for name in RP.CASES:
        for gamma in _variants(name):
            case, ref = RP.case_and_ref(name, gamma)
            raw, _ = RP.fractions(case, RP.emulate(case, gamma=gamma), ref, tol=1.0)
            for out, f in raw.items():
                key = (case['kind'], out)
                worst[key] = max(worst.get(key, 0.0), f)
    for (kind, out), f in worst.items():
        rec = RP.EMULATION_WORST[kind][out]
        print(f'REC-FIG worst {kind}:{out} measured {f:.3e} recorded {rec:.3e} working bound {RP.working_bound(kind, out):.0e} '
              f'bound {RP.bound(kind, out):.0e} ceiling {RP.ceiling(out):.1e}')
        assert 0.8 * rec <= f <= 1.25 * rec, (kind, out, f, rec)
        assert RP.working_bound(kind, out) <= RP.bound(kind, out) <= RP.ceiling(out)
    assert RP.round_up_1sig(8 * 8.31e-7) == 7e-6 and RP.round_up_1sig(2e-5) == 2e-5 and RP.round_up_1sig(1.01e-6) == 2e-6


# mutant -> [(case, outputs that must exceed their bound threefold)]
MUTANT_TABLE = {
    'h0_fwd_zero': [('gilr-cl16-L65', ('h',)), ('gilr_noact-cl64-L17', ('h',)), ('lru-cl32-L45', ('hr', 'hi')), ('gru-B5L4H80-h0both', ('h',))],
    'h0_bwd_zero': [('gilr-cl16-L1', ('df',)), ('gilr-cl16-L2', ('df',)), ('gilr_noact-cl64-L40', ('df',)),
                    ('lru-cl16-L1', ('dlam_re', 'dlam_im')), ('lru-cl16-L2', ('dlam_re', 'dlam_im')), ('gru-B88L3H192-h0both', ('dgi', 'dw_hh'))],
    'carry_nearest': [('gilr-long-L2003', ('h',)), ('gilr_noact-cl32-L45', ('h',)), ('lru-long-L2003', ('hr', 'hi')), ('lru-cl64-L40', ('hr',))],
    'bwd_carry_dropped': [('gilr-cl32-L45', ('dv', 'df')), ('gilr-longr-L2003', ('dv',)), ('lru-cl64-L40', ('dvr', 'dvi', 'dgamma')),
                          ('lru-cl16-L130', ('dvr', 'dlam_re'))],
    'start0_ignored': [('gilr-cl16-L130', ('h', 'dv')), ('gilr_noact-cl16-L2', ('h',)), ('lru-cl16-L2', ('hr', 'hi')), ('lru-cl64-L17', ('hr', 'dlam_im'))],
}


@pytest.mark.parametrize('mutant', list(MUTANT_TABLE))
def test_each_mutant_exceeds_a_named_bound_threefold(mutant):
    for name, outs in MUTANT_TABLE[mutant]:
        case, ref = RP.case_and_ref(name)
        bad = RP.emulate(case, mutant=mutant)
        fr, _ = RP.fractions(case, bad, ref)
        for out in outs:
            ceil_fr = fr[out] * RP.bound(case['kind'], out) / RP.ceiling(out)
            print(f'REC-FIG {name} mutant:{mutant}:{out} {fr[out]:.1f} (of the ceiling: {ceil_fr:.1f})')
            assert fr[out] >= RP.MUTANT_FACTOR and ceil_fr >= RP.MUTANT_FACTOR, (name, out, fr[out], ceil_fr)
        if mutant == 'h0_bwd_zero' and case['kind'] != 'lru':                 # it is the first step that is wrong, and only that one
            out = 'df' if case['kind'] != 'gru' else 'dgi'
            first, _, _ = RP.sliced_fraction(bad[out][:, :1], ref[out][:, :1], RP.bound(case['kind'], out))
            good = RP.emulate(case)
            assert first >= RP.MUTANT_FACTOR and torch.equal(bad[out][:, 1:], good[out][:, 1:]) and torch.equal(bad['h'], good['h'])
        if mutant == 'carry_nearest' and name.endswith('long-L2003'):         # what one scale per tensor makes of it
            out = outs[0]
            whole = RP.whole_fraction(bad[out], ref[out], 1e-4)
            print(f'REC-FIG {name} mutant:{mutant}:{out} whole-tensor(1e-4) {whole:.1f} sliced(1e-4) {fr[out] * RP.bound(case["kind"], out) / 1e-4:.1f}')


@pytest.mark.parametrize('B,L,C', [(2, 33, 64), (2, 7, 32)])
def test_the_older_draws_cannot_see_a_dead_initial_state(B, L, C):
    old = RP.old_style_case('gilr', B, L, C)
    good = RP.emulate(old)
    for mutant in ('h0_fwd_zero', 'h0_bwd_zero'):
        bad = RP.emulate(old, mutant=mutant)
        assert all(torch.equal(bad[k], good[k]) for k in good), mutant
    fr, _ = RP.fractions(old, RP.emulate(old, mutant='start0_ignored'), RP.reference(old))
    print(f'REC-FIG {old["name"]} mutant:start0_ignored:h {fr["h"]:.1f} (seen: the random h0 gets in)')
    old = RP.old_style_case('lru', B, L, C)
    good = RP.emulate(old)
    for mutant in ('h0_fwd_zero', 'h0_bwd_zero', 'start0_ignored'):
        bad = RP.emulate(old, mutant=mutant)
        assert all(torch.equal(bad[k], good[k]) for k in good), mutant
    # the same mutants on the same shape with the new draw
    new = dict(old, start=RP.make_start(B, L, torch.Generator().manual_seed(1), 0.03),
               h0r=2 * torch.randn(B, C, generator=torch.Generator().manual_seed(2)), h0i=None)
    ref = RP.reference(new)
    for mutant in ('h0_fwd_zero', 'h0_bwd_zero', 'start0_ignored'):
        fr, _ = RP.fractions(new, RP.emulate(new, mutant=mutant), ref)
        assert max(fr.values()) >= RP.MUTANT_FACTOR, (mutant, fr)


def test_metric_slices_rows_and_blocks_skips_exact_zeros_and_sees_a_quiet_slice():
    ref = torch.ones(2, 130, 4, dtype=torch.float64)
    ref[0, :64] *= 100.0
    got = ref.clone()
    got[1, 129, 2] += 0.5
    f, n, skipped = RP.sliced_fraction(got, ref, 1e-2)
    assert (n, skipped) == (6, 0) and f == pytest.approx(50.0) and RP.whole_fraction(got, ref, 1e-2) == pytest.approx(0.5)
    ref[1, 64:128] = 0.0
    got = ref.clone()
    assert RP.sliced_fraction(got, ref, 1e-2) == (0.0, 6, 1)
    got[1, 70, 0] = 1e-30                                       # a skipped slice has to be exactly zero
    assert RP.sliced_fraction(got, ref, 1e-2)[0] == float('inf')
    got[1, 70, 0] = float('nan')
    assert RP.sliced_fraction(got, ref, 1e-2)[0] == float('inf')
    S = torch.tensor([10.0, 0.0, 2.0])
    assert RP.sum_fraction(torch.tensor([1.0, 0.0, 1.001], dtype=torch.float64), torch.tensor([1.0, 0.0, 1.0]), S, 1e-3) == (pytest.approx(0.5), 3, 1)
    # the structural exception of the skip cap: L = 1 and start[b, 0] = 1 make the whole df slice of that row zero
    case = RP.make_case('gilr-cl16-L1')
    assert RP.expected_zero_slices(case) == 1 and RP.skip_cap_holds(case, 6, 1) and not RP.skip_cap_holds(case, 6, 2)
    assert not RP.skip_cap_holds(RP.make_case('gilr-cl16-L65'), 12, 1) and RP.skip_cap_holds(RP.make_case('gilr-cl64-L40'), 192, 3)


def test_case_table_reaches_every_instantiation_with_a_partly_filled_channel_block():
    routes = {}
    for name in RP.LINREC_CASES:
        c = RP.CASES[name]
        cl = RP.pick_cl(c['B'], c['C'])
        routes.setdefault(cl, set()).add(c['L'])
        assert c['C'] % cl != 0 or c['L'] == 2003, name                  # the long-carry cases: C = 48, three full blocks
        start = RP.make_case(name)['start']
        assert start[0::2, 0].sum() == 0 and (start[1::2, 0] == 1).all()
    assert routes == {16: {1, 2, 63, 64, 65, 130, 150, 2003}, 32: {33, 45}, 64: {17, 40}}
    assert RP.make_case('gilr-long-L2003')['start'].sum() == 0 and RP.make_case('gilr-longr-L2003')['start'].sum() > 20
    for name in RP.GRU_CASES:
        c = RP.CASES[name]
        persistent = (c['C'] // 16) * ((c['B'] + 3) // 4) <= 256
        assert persistent == (c['L'] > 3) and (c['B'] % 4 != 0 or not persistent)
    assert 150 // 64 + 1 == 3 and RP.CONT_SPLIT % 3 != 0
