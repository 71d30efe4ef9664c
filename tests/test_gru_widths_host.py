"""GRU hidden widths, what can be checked without a GPU: the one width table (`ops.gru_width_plan`) against the set of widths the C
entries accept, the argument checks of the pad entries (which return before the device is touched), and the bounds the GPU test
(tests/test_gru_widths_gpu.py) asserts - derived on the CPU from the fp32 emulation of tests/recurrence_parity.py."""
import ctypes
import os

import pytest
import torch

import gru_widths as GW
import recurrence_parity as RP

RESEL_EINVAL = -1
PAD_ENTRIES = ('resel_gru_pad_params', 'resel_gru_unpad_params', 'resel_gru_pad_rows', 'resel_gru_unpad_rows')


@pytest.fixture(scope='module')
def ops():
    from offpolicy_rnn.hip import ops as o
    return o


@pytest.fixture(scope='module')
def lib():
    from offpolicy_rnn.hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('resel_gru_workspace_bytes', 'resel_gru_multi_workspace_bytes', 'resel_gru_multi_form', 'resel_gru_seq_fwd', 'resel_gru_seq_bwd') + PAD_ENTRIES:
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


def test_native_set_and_bound(ops):
    assert ops.GRU_MAX_HIDDEN == 1024
    assert ops.GRU_NATIVE_WIDTHS == tuple(range(16, 257, 16)) + (288, 320, 336, 352, 384, 416, 448, 480, 512, 640, 768, 896, 1024)
    assert list(ops.GRU_NATIVE_WIDTHS) == sorted(set(ops.GRU_NATIVE_WIDTHS))


def test_every_width_has_the_smallest_native_width_above_it(ops, lib):
    native = ops.GRU_NATIVE_WIDTHS
    for H in range(1, 1025):
        plan = ops.gru_width_plan(H)
        assert plan.Hk >= H and plan.Hk in native, (H, plan)
        assert plan.Hk == min(w for w in native if w >= H), (H, plan)
        assert plan.native == (H in native) == (plan.Hk == H), (H, plan)
        assert lib.resel_gru_multi_form(1, 4, plan.Hk) != RESEL_EINVAL, (H, plan)


def test_the_c_entries_accept_the_native_set_and_nothing_else(ops, lib):
    """The accepted set is a list: a width is taken by `resel_gru_multi_form` (the same `gru_ok` as every entry) exactly when the table
    calls it native - 40, 200 = 40 x 5, 272, 528, 576 and 1040 stay refused."""
    for H in range(-2, 1100):
        ok = lib.resel_gru_multi_form(1, 4, H) != RESEL_EINVAL
        assert ok == (H in ops.GRU_NATIVE_WIDTHS), H
    for H in (640, 768, 896, 1024):                     # the workspace holds the W copy, the carry and the granules of the new widths
        assert lib.resel_gru_workspace_bytes(3, 5, H) >= 3 * H * H * 4 + 2 * 3 * H * 4 + 8 * H * 8 + 64
        assert lib.resel_gru_multi_workspace_bytes(4, 3, 5, H) >= 4 * lib.resel_gru_workspace_bytes(3, 5, H)


@pytest.mark.parametrize('H', [0, -3, 1025])
def test_widths_outside_the_range_raise(ops, H):
    with pytest.raises(ValueError, match='1 to 1024') as e:
        ops.gru_width_plan(H)
    assert '512, 640, 768, 896, 1024' in str(e.value) and 'multiples of 16 up to 256' in str(e.value)


def test_module_keeps_true_shapes_at_any_width():
    """nn.GRU's parameter shapes whatever the kernel width (the flat store, state_dict and checkpoints see these)."""
    from offpolicy_rnn.models.gru import GRU
    for H in (1, 24, 200, 520, 1000):
        m = GRU(7, H)
        ref = torch.nn.GRU(7, H, batch_first=True)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}


def test_pad_entries_reject_bad_arguments_before_touching_the_device(lib):
    """Nothing here is a device pointer: a call that got past the argument checks would fault, not return."""
    fake = 0x1000
    H, Hk, n_in = 24, 32, 8

    def params(fn, src=(fake,) * 4, dst=(fake,) * 4, n_in=n_in, H=H, Hk=Hk):
        return fn(*src, *dst, n_in, H, Hk, None)

    def rows(fn, src=fake, dst=fake, n=6, G=3, H=H, Hk=Hk):
        return fn(src, dst, n, G, H, Hk, None)

    for fn in (lib.resel_gru_pad_params, lib.resel_gru_unpad_params):
        for k in range(4):                                                  # a NULL source / destination
            holed = tuple(None if i == k else fake for i in range(4))
            assert params(fn, src=holed) == RESEL_EINVAL, k
            assert params(fn, dst=holed) == RESEL_EINVAL, k
        assert params(fn, src=(None, None, fake, None), dst=(None, None, fake, fake)) == RESEL_EINVAL      # recurrent pair without b_hh
        assert params(fn, src=(fake, fake, fake + 2, fake)) == RESEL_EINVAL                                # misaligned
        assert params(fn, dst=(fake, fake, fake, fake + 1)) == RESEL_EINVAL
        assert params(fn, n_in=0) == RESEL_EINVAL
        for h, hk in ((0, 32), (-1, 32), (32, 32), (33, 32), (24, 40), (24, 528), (24, 1040), (24, 0)):
            assert params(fn, H=h, Hk=hk) == RESEL_EINVAL, (h, hk)
    for fn in (lib.resel_gru_pad_rows, lib.resel_gru_unpad_rows):
        assert rows(fn, src=None) == RESEL_EINVAL and rows(fn, dst=None) == RESEL_EINVAL
        assert rows(fn, src=fake + 2) == RESEL_EINVAL and rows(fn, dst=fake + 3) == RESEL_EINVAL
        assert rows(fn, n=0) == RESEL_EINVAL and rows(fn, n=-4) == RESEL_EINVAL
        assert rows(fn, G=0) == RESEL_EINVAL and rows(fn, G=5) == RESEL_EINVAL
        assert rows(fn, n=1 << 31) == RESEL_EINVAL and rows(fn, n=(1 << 31) // (3 * Hk)) == RESEL_EINVAL     # 2^31 elements and more
        for h, hk in ((0, 32), (32, 32), (40, 32), (24, 40), (24, 272), (24, 2048)):
            assert rows(fn, H=h, Hk=hk) == RESEL_EINVAL, (h, hk)


def test_recurrence_entries_reject_what_they_refused_before(lib):
    fake = 0x1000
    for H in (40, 200, 272, 528, 576, 1040):
        assert lib.resel_gru_seq_fwd(fake, fake, fake, None, fake, None, fake, 4, 3, H, None) == RESEL_EINVAL, H
        assert lib.resel_gru_seq_bwd(fake, None, fake, fake, fake, fake, fake, fake, 4, 3, H, None) == RESEL_EINVAL, H


def test_case_table_reaches_both_drivers_at_every_new_native_width(ops):
    grids = {}
    for name, c in GW.CASES.items():
        Hk = ops.gru_width_plan(c['C']).Hk
        grids.setdefault(Hk, set()).add((Hk // 16) * ((c['B'] + 3) // 4) <= 256)
    for Hk in GW.NEW_NATIVE:
        assert grids[Hk] == {True, False}, Hk
    assert [GW.per_step_rows(H) for H in GW.NEW_NATIVE] == [25, 21, 17, 17]
    for H in GW.NEW_NATIVE:
        B = GW.per_step_rows(H)
        assert (H // 16) * ((B + 3) // 4) > 256 >= (H // 16) * ((B + 2) // 4)
    assert {c['C'] for c in GW.CASES.values()} == set(GW.WIDTHS)


def test_working_bounds_are_eight_times_the_emulation_worst_and_under_the_ceilings():
    """Every case of the table: the fp32 emulation of the kernels' arithmetic stays within the recorded worst of each output (so within
    1/8 of its working bound), no slice is skipped, and the bounds are the recorded figures."""
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))
    try:
        for name in GW.NAMES:
            case, ref = GW.case_and_ref(name)
            fr, (n, skipped) = RP.fractions(case, RP.emulate(case), ref, tol=1.0)
            print(f'GRUW-EMU {name} ' + ' '.join(f'{o}:{f:.2e}' for o, f in fr.items()))
            assert skipped == 0 and RP.skip_cap_holds(case, n, skipped), name
            for out, f in fr.items():
                assert f <= GW.EMULATION_WORST[out], (name, out, f)
    finally:
        torch.set_num_threads(before)
    assert {o: GW.working_bound(o) for o in RP.OUTPUTS['gru']} == {'h': 5e-6, 'dgi': 8e-6, 'dw_hh': 7e-5, 'db_hh': 1e-5}
    for out in RP.OUTPUTS['gru']:
        assert GW.working_bound(out) <= RP.ceiling(out) and GW.bound(out) <= RP.ceiling(out)
        assert GW.working_bound(out) >= 8.0 * GW.EMULATION_WORST[out]


def test_pad_gates_is_per_gate_block():
    H, Hk = 3, 5
    w = torch.arange(3 * H * H, dtype=torch.float32).reshape(3 * H, H) + 1
    p = GW.pad_gates(w, H, Hk, cols=True)
    for g in range(3):
        assert torch.equal(p[g * Hk:g * Hk + H, :H], w[g * H:(g + 1) * H]) and not p[g * Hk + H:(g + 1) * Hk].any() and not p[:, H:].any()
    assert torch.equal(GW.unpad_gates(p, H, Hk, cols=True), w)
    b = torch.arange(2 * 3 * H, dtype=torch.float32).reshape(2, 3 * H) + 1
    q = GW.pad_gates(b, H, Hk)
    assert q.shape == (2, 3 * Hk) and torch.equal(q[:, Hk:Hk + H], b[:, H:2 * H]) and torch.equal(GW.unpad_gates(q, H, Hk), b)
