"""`ops.categorical_step` (resel_categorical_step): the categorical head of one policy step against the four steps of
`ContextualSACDiscretePolicy.process_model_out` in float64 on the same fp32 logits - log-probabilities, mode, inverse-CDF sample - and
its behaviour on a row that holds a NaN.

Error bound of the log-probabilities (derived, not measured): the three sums of A terms contribute at most (A - 1) 2^-24 each, about a
dozen single roundings (a 2-ulp expf and logf among them) one 2^-24 each, so |p - p64| <= (3 (A - 1) + 12) 2^-24 p64 and
|logp - logp64| <= (3 (A - 1) + 12) 2^-24 + 4 2^-24 |logp64|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 2), (3, 4), (64, 63), (5, 64), (257, 65), (2, 130)]
STRIDED = (2, 130)                                       # logp as columns of a wider block
FLOOR = 0.01
EPS = 2.0 ** -24


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def ref64(logits):
    """process_model_out's four steps in float64 -> (p, log p, cdf)."""
    s = torch.softmax(logits.double(), dim=-1)
    t = s + FLOOR
    p = t / t.sum(dim=-1, keepdim=True)
    p = p / p.sum(dim=-1, keepdim=True)
    return p, torch.log(p), torch.cumsum(p, dim=-1)


_CASES = {}


def case(M, A):
    """Logits uniform in [-2, 2] (fp32, on the host) and their float64 reference: computed once per shape, never changed."""
    if (M, A) not in _CASES:
        g = torch.Generator().manual_seed(1000 * M + A)
        x = torch.rand(M, A, generator=g) * 4 - 2
        _CASES[(M, A)] = (x,) + ref64(x)
    return _CASES[(M, A)]


def run(ops, x, u=None, strided=False):
    x = x.cuda()
    M, A = x.shape
    u = torch.full((M,), 0.5, device='cuda') if u is None else u.float().cuda()
    out = None
    if strided:
        out = torch.full((M, 2 + A), 7.0, device='cuda')
    mode, sample, logp = ops.categorical_step(x, u, FLOOR, out=out)
    if strided:
        assert logp.stride(0) == 2 + A and logp.data_ptr() == out.data_ptr() + 8
    torch.cuda.synchronize()
    return mode.cpu(), sample.cpu(), logp.cpu()


def check_logp(logp, p64, logp64, A, what):
    rel = (3 * (A - 1) + 12) * EPS
    bound = rel + 4 * EPS * logp64.abs()
    ratio = ((logp.double() - logp64).abs() / bound).max().item()
    ratio_p = ((logp.double().exp() - p64).abs() / (bound * p64)).max().item()
    print(f'\n[categorical_step {what}] largest |logp - logp64| / bound = {ratio:.3f}, |exp(logp) - p64| / (bound p64) = {ratio_p:.3f}')
    assert torch.isfinite(logp).all()
    assert ratio <= 1.0, (what, ratio)


# ------------------------------------------------------------------------------------------------ 1. arithmetic
@pytest.mark.parametrize('M,A', SHAPES)
def test_logp_against_fp64(ops, M, A):
    x, p64, logp64, _ = case(M, A)
    mode, sample, logp = run(ops, x, strided=(M, A) == STRIDED)
    assert logp.shape == (M, A) and mode.shape == (M,) and sample.shape == (M,)
    check_logp(logp, p64, logp64, A, f'M={M} A={A}')
    for idx in (mode, sample):
        assert idx.dtype == torch.float32 and torch.equal(idx, idx.round()) and idx.min() >= 0 and idx.max() <= A - 1


def test_logp_saturated_softmax(ops):
    """Entries of +-1e4: the softmax is an indicator of the +1e4 entries (a row without one: of all its entries), the floor does the rest."""
    M, A = 6, 70
    g = torch.Generator().manual_seed(5)
    x = torch.where(torch.rand(M, A, generator=g) < 0.3, 1e4, -1e4).float()
    x[0] = -1e4                                                     # no +1e4 in the row: uniform
    x[1, 1:] = -1e4
    x[1, 0] = 1e4                                                   # a single winner
    p64, logp64, _ = ref64(x)
    mode, sample, logp = run(ops, x)
    check_logp(logp, p64, logp64, A, 'saturated')
    assert mode[0] == 0 and mode[1] == 0


# ------------------------------------------------------------------------------------------------ 2. mode
@pytest.mark.parametrize('M,A', SHAPES)
def test_mode_finds_a_planted_winner(ops, M, A):
    x = case(M, A)[0].clone()
    win = torch.from_numpy(np.random.RandomState(M + A).randint(0, A, size=M))
    x[torch.arange(M), win] += 4.5                                  # leads every other logit by at least 0.5
    mode, _, _ = run(ops, x, strided=(M, A) == STRIDED)
    assert torch.equal(mode.long(), win)


@pytest.mark.parametrize('A', [1, 5, 64, 65, 130])
def test_mode_of_equal_logits_is_zero(ops, A):
    mode, _, logp = run(ops, torch.full((3, A), 0.37))
    assert torch.equal(mode, torch.zeros(3))
    assert torch.equal(logp, logp[:, :1].expand(3, A))


@pytest.mark.parametrize('A,i,j', [(5, 1, 3), (65, 0, 64), (130, 63, 64), (130, 10, 100), (130, 70, 129), (64, 62, 63)])
def test_mode_of_two_equal_maxima_is_the_lower_index(ops, A, i, j):
    x = case(4, A)[0].clone()
    x[:, i] = 3.0
    x[:, j] = 3.0
    mode, _, logp = run(ops, x)
    assert torch.equal(logp[:, i], logp[:, j])                      # the same arithmetic in two lanes: exactly equal
    assert torch.equal(mode, torch.full((4,), float(i)))


# ------------------------------------------------------------------------------------------------ 3. sample, deterministic
@pytest.mark.parametrize('M,A', SHAPES)
def test_sample_at_every_interval_midpoint(ops, M, A):
    """u at the float64 midpoint of [cdf_{k-1}, cdf_k) for every (row, k).  An interval is at least FLOOR / (1 + FLOOR A) wide, the
    midpoint so at least 3.8e-4 (A = 130) from both ends: three orders of magnitude above the bound of test 1."""
    x, p64, _, cdf = case(M, A)
    assert p64.min().item() >= FLOOR / (1 + FLOOR * A) * (1 - 1e-12)
    lo = torch.cat((torch.zeros(M, 1, dtype=torch.float64), cdf[:, :-1]), dim=1)
    u = ((lo + cdf) / 2).reshape(-1)                                # [M * A]: row m, interval k
    rows = x.repeat_interleave(A, dim=0)                            # [M * A, A]
    _, sample, _ = run(ops, rows, u, strided=(M, A) == STRIDED)
    want = torch.arange(A).repeat(M)
    assert torch.equal(sample.long(), want), (sample.long() != want).nonzero()[:5]


@pytest.mark.parametrize('M,A', SHAPES)
def test_sample_at_the_ends_of_the_unit_interval(ops, M, A):
    x = case(M, A)[0]
    _, sample, _ = run(ops, x, torch.zeros(M))
    assert torch.equal(sample, torch.zeros(M))
    _, sample, _ = run(ops, x, torch.full((M,), 1.0 - 2.0 ** -24))
    assert sample.min() >= 0 and sample.max() <= A - 1 and torch.equal(sample, sample.round())
    # cdf_{A-2} = 1 - p_{A-1} <= 1 - FLOOR / (1 + FLOOR A) lies far below this u, so it is the last interval or the clamp: A - 1 both
    assert torch.equal(sample, torch.full((M,), float(A - 1)))


# ------------------------------------------------------------------------------------------------ 4. sample, statistical
def test_sample_frequencies(ops):
    M, A = 65536, 5
    x = torch.tensor([[0.3, -1.2, 1.9, 0.0, -0.4]])
    p = ref64(x)[0][0]
    g = torch.Generator(device='cuda').manual_seed(12)
    u = torch.rand(M, device='cuda', generator=g)
    _, sample, _ = run(ops, x.expand(M, A).contiguous(), u)
    counts = torch.bincount(sample.long(), minlength=A).double()
    assert counts.sum() == M and counts.numel() == A
    sigma = torch.sqrt(M * p * (1 - p))
    z = (counts - M * p).abs() / sigma
    print(f'\n[categorical_step frequencies] counts {counts.tolist()}, expected {[round(v, 1) for v in (M * p).tolist()]}, largest deviation {z.max():.2f} sigma')
    assert (z <= 5.0).all(), z


# ------------------------------------------------------------------------------------------------ 5. a NaN row
@pytest.mark.parametrize('A', [7, 130])
def test_nan_row_stays_in_its_row(ops, A):
    x = case(4, A)[0].clone()
    u = torch.tensor([0.1, 0.6, 0.3, 0.9])
    bad = 2
    x[bad, A // 2] = float('nan')
    mode, sample, logp = run(ops, x, u)
    assert torch.isnan(logp[bad]).all()
    assert 0 <= mode[bad] <= A - 1 and 0 <= sample[bad] <= A - 1
    keep = [r for r in range(4) if r != bad]
    mode3, sample3, logp3 = run(ops, x[keep], u[keep])
    assert torch.equal(logp[keep].view(torch.int32), logp3.view(torch.int32))
    assert torch.equal(mode[keep], mode3) and torch.equal(sample[keep], sample3)
    torch.cuda.synchronize()                                        # no device assert anywhere: returns normally
