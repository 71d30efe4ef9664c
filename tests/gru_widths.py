"""The case table, the draw and the bounds of the GRU width tests (tests/test_gru_widths_host.py on the CPU, tests/test_gru_widths_gpu.py
on the GPU): `ops.gru_seq` at hidden widths that are not native to csrc/gru_seq.hip (zero-padded onto the next native one) and at the
native widths above 512, held to fp64 with the models and the metric of tests/recurrence_parity.py.

Cases are drawn exactly as `recurrence_parity.make_case` draws its gru branch (that table and its `route` / `gru_kc` only know the
older widths, so the dicts are built here).  Bounds are derived as that module derives its own: 8 x the worst fraction the fp32
emulation (`RP.emulate`) reaches against the fp64 model (`RP.reference`) over THIS table, measured on the CPU, rounded up to one
significant digit, never above the project's ceilings.  The host test asserts the recorded worsts."""
import functools
import math

import torch

import recurrence_parity as RP

# widths at (B, L) = (3, 5): the persistent form with a ragged 4-row group.  1, 8, 24: onto 16 / 16 / 32; 200 onto 208; 264 onto 288;
# 500 onto 512; 520 onto 640; 1000 onto 1024; 640 / 768 / 896 / 1024: the native widths above 512.
WIDTHS = (1, 8, 24, 200, 264, 500, 520, 640, 768, 896, 1000, 1024)
NEW_NATIVE = (640, 768, 896, 1024)


def per_step_rows(Hk):
    """The smallest B whose (Hk / 16) x ceil(B / 4) workgroups exceed the 256 the persistent form takes."""
    groups = 256 // (Hk // 16) + 1
    return 4 * (groups - 1) + 1


_SHAPES = [(3, 5, H) for H in WIDTHS] + [(3, 70, 200)]                           # 70 steps: across a 64-step block
_SHAPES += [(per_step_rows(H), 3, H) for H in NEW_NATIVE]                        # one launch per step: 25, 21, 17, 17 rows
_SHAPES += [(28, 3, 640), (20, 3, 1024)]                                         # the same grids with a full last row group
CASES = {}
for _i, (_B, _L, _H) in enumerate(_SHAPES):
    for _h0 in ('both', 'none'):
        CASES[f'gruw-B{_B}L{_L}H{_H}-h0{_h0}'] = dict(kind='gru', B=_B, C=_H, L=_L, seed=3400 + _i, h0=_h0)
NAMES = list(CASES)

# worst fraction-of-1 error of `RP.emulate` against `RP.reference` over the table above, measured on the CPU
# (profiles/r34_gru_widths.md has every case); tests/test_gru_widths_host.py asserts that no case exceeds its entry.
EMULATION_WORST = {'h': 5.36e-7, 'dgi': 9.81e-7, 'dw_hh': 8.26e-6, 'db_hh': 1.17e-6}
# -> working bounds 5e-6, 8e-6, 7e-5, 1e-5 (ceilings 1e-4, 2.5e-4, 2.5e-4, 2.5e-4)

# outputs whose working bound a correct kernel exceeds on the MI355X while under the ceiling: output -> (bound <= ceiling, reason read
# in the code).
RAISED = {}


def working_bound(out):
    return min(RP.ceiling(out), RP.round_up_1sig(8.0 * EMULATION_WORST[out]))


def bound(out):
    return RAISED[out][0] if out in RAISED else working_bound(out)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """fp32 tensors of a case: the draw of `recurrence_parity.make_case` for kind 'gru', in its order."""
    c = dict(CASES[name])
    c['name'] = name
    B, L, H = c['B'], c['L'], c['C']
    g = torch.Generator().manual_seed(c['seed'])
    r = lambda *s: torch.randn(*s, generator=g)
    c.update(gi=r(B, L, 3 * H), w_hh=r(3 * H, H) / math.sqrt(H), b_hh=r(3 * H) / math.sqrt(H), dh=r(B, L, H))
    h0 = r(B, H)
    c['h0_t'] = h0 if c['h0'] == 'both' else None
    return c


@functools.lru_cache(maxsize=None)
def case_and_ref(name):
    case = make_case(name)
    return case, RP.reference(case)


def fractions(case, got, ref):
    """{output: fraction of its bound here}, (slices, skipped): `RP.fractions` with this table's bound per output."""
    fr, n, skipped = {}, 0, 0
    for out in RP.OUTPUTS['gru']:
        f, (a, b) = RP.fractions(case, got, ref, tol=bound(out), outputs=(out,))
        fr.update(f)
        n, skipped = n + a, skipped + b
    return fr, (n, skipped)


def pad_gates(t, H, Hk, cols=False):
    """Zero-pad a [.., 3H] (or, cols: [3H, H]) operand per gate block to 3Hk (and Hk columns): row g * Hk + j <- row g * H + j."""
    if cols:
        out = t.new_zeros(3, Hk, Hk)
        out[:, :H, :H] = t.reshape(3, H, H)
        return out.reshape(3 * Hk, Hk)
    out = t.new_zeros(t.shape[:-1] + (3, Hk))
    out[..., :H] = t.reshape(t.shape[:-1] + (3, H))
    return out.reshape(t.shape[:-1] + (3 * Hk,))


def unpad_gates(t, H, Hk, cols=False):
    if cols:
        return t.reshape(3, Hk, Hk)[:, :H, :H].reshape(3 * H, H).contiguous()
    return t.reshape(t.shape[:-1] + (3, Hk))[..., :H].reshape(t.shape[:-1] + (3 * H,)).contiguous()
