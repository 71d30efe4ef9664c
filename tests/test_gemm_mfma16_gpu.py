"""The third GEMM edition's consumers form their products with v_mfma_f32_16x16x32_f16 (8 x 4 accumulators of 16 x 16 per wave): where an
accumulator element lands, and what it holds.

Placement: with integer-valued A (|a| <= 1024: exact in the first fp16 plane under any power-of-two scale) and B a 0 / 1 selection
matrix every output is ONE exact product, so C must equal the selected columns of A bit for bit - a wrong lane-to-element map in the K
loop, an epilogue's scatter, the slab or the fix-up is an exact mismatch, not a tolerance.  Values: the smallest shapes the edition takes
(M > 128, K a multiple of 32) against fp64 under the bound the plain mode-2 product is already held to (`test_gemm_fused_gpu.py`: RTOL +
ATOL_SCALE of the reference's largest magnitude), through every epilogue; row dots and column sums against the kernel's own output
inside the rigorous bound of an fp32 sum in any order.  Every call is made twice and must be bit-equal."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL_SCALE = 1e-5, 1e-6                                  # of max |reference|: the bound of test_gemm_fused_gpu.py's plain product
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]       # (A [M, K] else [K, M], B [N, K] else [K, N])
EPILOGUES = ['none', 'bias', 'elu', 'softplus', 'accumulate']


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


@pytest.fixture(autouse=True)
def mode2(ops, monkeypatch):
    monkeypatch.setattr(ops, 'GEMM_SPLIT', 2)


def held(case, got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    print(f'MFMA16-FIG {case} {err / ((RTOL + ATOL_SCALE) * scale):.4f}')
    assert torch.isfinite(got).all(), f'{case}: non-finite output'
    assert err <= (RTOL + ATOL_SCALE) * scale, f'{case}: max err {err:.3e} vs scale {scale:.3e}'


def laid_out(A, B, akc, bkc):
    """A [.., M, K], B [.., K, N] -> the operands in the layout the call names, on the GPU."""
    return (A if akc else A.transpose(-1, -2)).contiguous().cuda(), (B.transpose(-1, -2) if bkc else B).contiguous().cuda()


def product(ops, A, B, akc, bkc, bias=None, act=None, out=None):
    """Mode 2 with both handles given (no fall-back to another mode), twice, bit-equal -> the output."""
    ha, hb = ops.amax(A), ops.amax(B)
    res = []
    for _ in range(2):
        ops.LAST_SPLIT[0] = None
        o = None if out is None else out.clone()
        res.append(ops.gemm_f32(A, B, akc, bkc, bias, act, out=o, split=2, amax_a=ha, amax_b=hb))
        assert ops.LAST_SPLIT[0] == 2, 'the product did not run in mode 2'
    assert torch.equal(res[0], res[1]), 'two runs differ'
    return res[0]


# ------------------------------------------------------------------------------------------------ placement
# (batch, M, N, K): whole tiles, an edge in M, an edge in N, batch 3, and a K-sliced plan (few tiles, long K: slab + fix-up)
PLACEMENT = [(1, 256, 128, 32), (1, 512, 256, 64), (1, 300, 128, 64), (1, 256, 136, 96), (3, 260, 132, 32), (1, 256, 128, 4096)]


@functools.lru_cache(maxsize=None)
def placement_case(batch, M, N, K):
    g = torch.Generator().manual_seed(M + 3 * N + 5 * K + batch)
    A = torch.randint(-1024, 1025, (batch, M, K), generator=g).float()
    sel = torch.randint(0, K, (batch, N), generator=g)                  # column n of C selects column sel[n] of A
    B = torch.zeros(batch, K, N)
    B.scatter_(1, sel.unsqueeze(1), 1.0)
    return A, B, torch.gather(A, 2, sel.unsqueeze(1).expand(batch, M, N))


@pytest.mark.parametrize('akc,bkc', LAYOUTS)
@pytest.mark.parametrize('batch,M,N,K', PLACEMENT)
def test_placement_is_exact(ops, batch, M, N, K, akc, bkc):
    A, B, want = placement_case(batch, M, N, K)
    if batch == 1:
        A, B, want = A[0], B[0], want[0]
    Ad, Bd = laid_out(A, B, akc, bkc)
    got = product(ops, Ad, Bd, akc, bkc).cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} misplaced or inexact elements, the first at {bad[0].tolist()}: {got[tuple(bad[0])].item()} for {want[tuple(bad[0])].item()}'


@pytest.mark.parametrize('b_kcontig', [True, False])
@pytest.mark.parametrize('M', [256, 300])
def test_placement_head_and_dact_are_exact(ops, M, b_kcontig):
    """The fused exits at E = 2: with zero bias and non-negative integers ELU is the identity, and with Y > 0 the dact factor is 1."""
    A, B, want = placement_case(2, M, 128, 64)
    A, want = A.abs(), want.abs()
    Ad, Bd = laid_out(A, B, True, b_kcontig)
    ha, hb = ops.amax(Ad), ops.amax(Bd)
    zero, w3 = torch.zeros(2, 128, device='cuda'), torch.ones(2, 128, device='cuda')
    for _ in range(2):
        a, q = ops.gemm_f32_head(Ad, Bd, b_kcontig, zero, w3, None, amax_a=ha, amax_b=hb)
        assert torch.equal(a.cpu(), want)
        assert torch.equal(q.cpu(), want.sum(-1))                       # integers below 2^24: every order of the sum is exact
        out, dbias = ops.gemm_f32_dact(Ad, Bd, b_kcontig, torch.ones(2, M, 128, device='cuda'), torch.empty(2, M, 128, device='cuda'), True, amax_a=ha, amax_b=hb)
        assert torch.equal(out.cpu(), want)
        assert torch.equal(dbias.cpu(), want.sum(-2))


# ------------------------------------------------------------------------------------------------ values against fp64
SHAPES = [(M, N, K) for M in (129, 256, 300, 513) for N in (128, 136, 256) for K in (32, 64, 96)]


@functools.lru_cache(maxsize=None)
def value_case(M, N, K):
    g = torch.Generator().manual_seed(7919 * M + 101 * N + K)
    M4 = (M + 3) // 4 * 4                                               # [K, M] operands need whole float4 rows: those layouts run M rounded up
    A, B = torch.randn(M4, K, generator=g), torch.randn(K, N, generator=g) / K ** 0.5
    return A, B, torch.randn(N, generator=g), torch.randn(M4, N, generator=g), A.double() @ B.double()


@pytest.mark.parametrize('M,N,K', SHAPES)
def test_epilogues_vs_fp64(ops, M, N, K):
    A, B, bias, C0, ref = value_case(M, N, K)
    for n, epi in enumerate(EPILOGUES):
        akc, bkc = LAYOUTS[(n + M + N // 8 + K // 32) % 4]               # every epilogue meets every layout over the shapes
        rows = M if akc else A.shape[0]
        Ad, Bd = laid_out(A[:rows], B, akc, bkc)
        r, b, act, out = ref[:rows], None, None, None
        if epi != 'none' and epi != 'accumulate':
            b, r = bias.cuda(), r + bias.double()
        if epi == 'elu':
            act, r = 'elu', torch.nn.functional.elu(r)
        if epi == 'softplus':
            act, r = ops.GEMM_SOFTPLUS, torch.nn.functional.softplus(r)
        if epi == 'accumulate':
            act, out, r = ops.GEMM_ACCUMULATE, C0[:rows].cuda(), r + C0[:rows].double()
        held(f'({rows},{N},{K}){"mk" if akc else "km"}-{"nk" if bkc else "kn"} {epi}', product(ops, Ad, Bd, akc, bkc, b, act, out), r)


def sum_excess(got, terms, dim, extra=None):
    """|got - sum(terms)| as a fraction of the rigorous bound of an fp32 sum of n terms in any order, 1.01 n 2^-23 sum |terms|."""
    t = terms.double()
    n = t.shape[dim] + (0 if extra is None else 1)
    exact, mass = t.sum(dim), t.abs().sum(dim)
    if extra is not None:
        exact, mass = exact + extra.double(), mass + extra.double().abs()
    return ((got.double() - exact).abs() / (1.01 * n * 2.0 ** -23 * mass).clamp_min(1e-300)).max().item()


@pytest.mark.parametrize('b_kcontig', [True, False])
@pytest.mark.parametrize('M', [256, 300])                              # one whole and one ragged row tile
def test_head_and_dact_vs_fp64(ops, M, b_kcontig):
    E, N, K = 2, 128, 64
    g = torch.Generator().manual_seed(M + b_kcontig)
    rnd = lambda *s: torch.randn(*s, generator=g)
    A, B, bias, w3, b3 = rnd(E, M, K), rnd(E, K, N) / K ** 0.5, rnd(E, N), rnd(E, N), rnd(E)
    Y = torch.nn.functional.elu(rnd(E, M, N))
    prod = A.double() @ B.double()
    Ad, Bd = laid_out(A, B, True, b_kcontig)
    ha, hb = ops.amax(Ad), ops.amax(Bd)
    heads = [ops.gemm_f32_head(Ad, Bd, b_kcontig, bias.cuda(), w3.cuda(), b3.cuda(), amax_a=ha, amax_b=hb) for _ in range(2)]
    assert torch.equal(heads[0][0], heads[1][0]) and torch.equal(heads[0][1], heads[1][1])
    a, q = (t.cpu() for t in heads[0])
    held(f'head({M}) a', a, torch.nn.functional.elu(prod + bias.double().unsqueeze(-2)))
    frac = sum_excess(q, a * w3.unsqueeze(-2), -1, b3.unsqueeze(-1))
    assert torch.isfinite(q).all() and frac <= 1.0, f'head({M}): a row dot at {frac:.3g} x the fp32 summation bound over the kernel\'s own a'
    Yd = Y.cuda()
    dacts = [ops.gemm_f32_dact(Ad, Bd, b_kcontig, Yd, torch.empty(E, M, N, device='cuda'), True, amax_a=ha, amax_b=hb) for _ in range(2)]
    assert torch.equal(dacts[0][0], dacts[1][0]) and torch.equal(dacts[0][1], dacts[1][1])
    out, dbias = (t.cpu() for t in dacts[0])
    held(f'dact({M}) out', out, prod * torch.where(Y > 0, torch.ones_like(Y), Y + 1).double())
    frac = sum_excess(dbias, out, -2)
    assert torch.isfinite(dbias).all() and frac <= 1.0, f'dact({M}): a column sum at {frac:.3g} x the fp32 summation bound over the kernel\'s own out'


# ------------------------------------------------------------------------------------------------ published magnitude
@pytest.mark.parametrize('M,N,act', [(4096, 256, None), (4100, 264, 'elu')])           # 2^20 elements and more: the output gets a magnitude slot
def test_published_magnitude_bounds_the_output(ops, M, N, act):
    g = torch.Generator().manual_seed(M)
    A, B, bias = torch.randn(M, 64, generator=g).cuda(), torch.randn(N, 64, generator=g).cuda(), torch.randn(N, generator=g).cuda()
    out = product(ops, A, B, True, True, bias, act)
    h = ops.amax_of(out)
    assert h is not None, 'no magnitude handle on the output'
    val, top = ops.amax_value(h), out.abs().max().item()
    assert top <= val <= top * (1 + 2.0 ** -20), f'handle {val!r} against max |out| {top!r}'
