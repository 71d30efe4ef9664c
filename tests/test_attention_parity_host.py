"""Host side of the per-(head, block) attention comparison (tests/attention_parity.py; the GPU side is tests/test_attention_fp64_gpu.py).

1. The rounding model - fp64 with the bf16 rounding points of csrc/attention.hip - stays at <= 0.5 of every bound the GPU test holds
   the kernels to, in the same metric and on the same data: the GPU test has no slack it does not need and does not ask what bf16
   cannot give.
2. A kernel that loses ONE 32-key score tile for the late queries of the longest sequence (`drop_key_tile = (32, 384)`) exceeds the
   sliced bounds of `out` and `dq` at least threefold, while it passes the whole-tensor bounds of the older attention tests (printed,
   not asserted).  At 385 tokens the mutant touches a single query row, and how far its dq sticks out depends on the data (1.7 .. 6.6
   times the bound over eleven seeds): the seed of `ragged64` is one at which that one row is seen clearly.
Every figure is printed as `ATTN-FIG` before it is asserted (profiles/r27_attention_fp64_tests.md keeps them)."""
import functools

import pytest
import torch

import attention_parity as AP

MODEL_SHARE = 0.5
MUTANT_FACTOR = 3.0


@pytest.fixture(scope='module', autouse=True)
def sixteen_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))
    yield
    torch.set_num_threads(before)


@functools.lru_cache(maxsize=None)
def _case_and_ref(name):
    case = AP.make_case(name)
    return case, AP.model_of(case)


@pytest.mark.parametrize('name', AP.HOST_CASES)
def test_rounding_model_uses_at_most_half_of_every_bound(name):
    case, ref = _case_and_ref(name)
    model = AP.model_of(case, rounding=True)
    fr = AP.fractions(case, model, ref)
    for nm, f in fr.items():
        print(f'ATTN-FIG {name} model:{nm} {f:.4f}')
    assert all(f <= MODEL_SHARE for f in fr.values()), fr
    assert fr['out'] > 0.05 and min(fr[nm] for nm in ('dq', 'dk', 'dv')) > 0.05, f'the model rounds nothing: {fr}'


def test_peaked_gradients_are_held_at_the_finest_granularity_the_rounding_model_allows():
    """The one `peaked` figure the host computes: which of (head, block) / (head) / (operand) the GPU test may ask of dq, dk, dv."""
    case, ref = _case_and_ref('peaked')
    model = AP.model_of(case, rounding=True)
    holds = {}
    for gran in AP.GRANULARITIES:
        fr = {nm: AP.sliced_fraction(model[nm], ref[nm], case['pos'], AP.GRAD_TOL, gran) for nm in ('dq', 'dk', 'dv')}
        for nm, f in fr.items():
            print(f'ATTN-FIG peaked model:{nm}@{gran} {f:.4f}')
        holds[gran] = max(fr.values()) <= MODEL_SHARE
    assert [g for g in AP.GRANULARITIES if holds[g]][0] == AP.PEAKED_GRAD_GRANULARITY, holds
    fr = AP.fractions(case, model, ref)
    print(f'ATTN-FIG peaked model:out {fr["out"]:.4f}')
    assert fr['out'] <= MODEL_SHARE and fr['lse2'] <= MODEL_SHARE


@pytest.mark.parametrize('name', ['ragged32', 'ragged64'])
def test_a_lost_score_tile_exceeds_the_sliced_bounds_threefold(name):
    case, ref = _case_and_ref(name)
    mutant = AP.model_of(case, drop_key_tile=(32, 384))
    fr = AP.fractions(case, mutant, ref)
    for nm, f in fr.items():
        print(f'ATTN-FIG {name} mutant:{nm} {f:.4f}')
    cat = lambda r: torch.stack([r[nm] for nm in ('dq', 'dk', 'dv')])
    print(f'ATTN-FIG {name} mutant:out(whole-tensor,1e-2) {AP.whole_fraction(mutant["out"], ref["out"], 1e-2):.4f}')
    print(f'ATTN-FIG {name} mutant:dqkv(whole-tensor,2e-2) {AP.whole_fraction(cat(mutant), cat(ref), 2e-2):.4f}')
    assert fr['out'] >= MUTANT_FACTOR and fr['dq'] >= MUTANT_FACTOR, fr
    assert fr['lse2'] >= MUTANT_FACTOR, fr


def test_slices_follow_position_in_sequence_and_short_tails_join_the_block_before():
    pos = torch.cat([torch.arange(n) for n in (641, 1, 127, 160, 159, 129)])
    blk = AP.block_ids(pos)
    ends = torch.cumsum(torch.tensor([641, 1, 127, 160, 159, 129]), 0) - 1
    assert blk[ends].tolist() == [4, 0, 0, 1, 0, 0]           # 641: the one-token sixth block joins the fifth; 160 = 128 + 32 keeps its tail
    assert blk[:641].tolist() == [min(i // 128, 4) for i in range(641)]
    # one wrong element of a small slice: invisible at the scale of the tensor, seen at the scale of its slice
    ref = torch.ones(641, 2, 4, dtype=torch.float64)
    ref[:128] *= 100.0
    got = ref.clone()
    got[600, 1, 2] += 0.5
    assert AP.whole_fraction(got, ref, 1e-2) == pytest.approx(0.5) and AP.sliced_fraction(got, ref, torch.arange(641), 1e-2) == pytest.approx(50.0)
    assert AP.sliced_fraction(got, ref, torch.arange(641), 1e-2, 'head') == pytest.approx(0.5)
    got[5, 0, 0] = float('nan')
    assert AP.sliced_fraction(got, ref, torch.arange(641), 1e-2) == float('inf')
