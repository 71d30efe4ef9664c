"""The kernels of the discrete-action update behind `ops.categorical_head`, `ops.discrete_value`, `ops.masked_q_taken_loss` and
`ops.masked_discrete_actor_loss`, against float64 autograd on the CPU of the torch spelling of each formula (the code these ops replace:
`ContextualSACDiscretePolicy.process_model_out`, `_target_Q_discrete`, the discrete branches of `_critic_step` / `_actor_step`).

Head forward: the derived bound of tests/test_categorical_step_gpu.py.  Everything else has no derived bound; the yardstick is the
replaced fp32 torch spelling run on the GPU on the same inputs:  max|kernel - ref64| <= 2 max|torch32 - ref64| + 16 2^-24 max|ref64|
(two correct fp32 evaluations in different summation orders differ by that much).  All three quantities are printed per case.

Inputs come from seeded host generators; every fp64 reference is computed once per case and never changed."""
import pytest
import torch

from test_categorical_step_gpu import EPS, FLOOR, case, ref64

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 2), (3, 4), (257, 6), (64, 63), (5, 64), (257, 65), (2, 130)]      # partial last wave, packed rows, one wave per row, chunked
ENSEMBLES = [1, 2, 8]
SUBSETS = [None, [5, 1]]                                  # of E = 8
LOG_ALPHA = -1.2
G_UP = 0.7                                                # incoming gradient of the loss sums


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


def within(what, kernel, ref, torch32):
    """max|kernel - ref64| <= 2 max|torch32 - ref64| + 16 eps max|ref64|, printed."""
    ref = ref.double()
    ek = (kernel.detach().double().cpu() - ref).abs().max().item() if ref.numel() else 0.0
    et = (torch32.detach().double().cpu() - ref).abs().max().item() if ref.numel() else 0.0
    scale = ref.abs().max().item() if ref.numel() else 0.0
    print(f'\n[{what}] max|kernel - ref64| = {ek:.3e}   max|torch32 - ref64| = {et:.3e}   max|ref64| = {scale:.3e}')
    assert torch.isfinite(kernel).all(), what
    assert ek <= 2 * et + 16 * EPS * scale, (what, ek, et, scale)


# ------------------------------------------------------------------------------------------------ torch spellings (any dtype / device)
def head_spelling(x):
    p = torch.softmax(x, dim=-1) + FLOOR
    p = p / p.sum(dim=-1, keepdim=True)
    p = p / p.sum(dim=-1, keepdim=True)
    return torch.log(p), p


def value_spelling(q, subset, logp, log_alpha):
    if subset is not None:
        q = q[torch.as_tensor(subset, device=q.device)]
    return ((q.min(dim=0).values - log_alpha.exp() * logp) * logp.exp()).sum(dim=-1, keepdim=True)


def q_taken_spelling(q, action, y, mask):
    qt = q.gather(-1, action.long().unsqueeze(0).expand(q.shape[0], -1, -1))
    return ((qt - y.unsqueeze(0)).pow(2).sum(dim=0) * mask).sum()


def actor_spelling(logp, q, mask, log_alpha, reduce_min):
    qr = q.min(dim=0).values if reduce_min else q.mean(dim=0)
    objective = ((log_alpha.exp().detach() * logp - qr) * logp.exp()).sum(dim=-1, keepdim=True)
    return (objective * mask).sum(), ((logp * logp.exp()).sum(dim=-1, keepdim=True) * mask).sum()


# ------------------------------------------------------------------------------------------------ inputs, once per case
_BATCH = {}


def batch(E, M, A):
    """fp32 host tensors: logp [M, A] (the head spelling of the logits of `case`), q [E, M, A], action / y / mask [M, 1] (about 30 % of the
    mask is 0), cotangents for the head."""
    if (E, M, A) not in _BATCH:
        g = torch.Generator().manual_seed(7000 + 100 * M + 10 * A + E)
        x = case(M, A)[0]
        _BATCH[(E, M, A)] = dict(
            x=x, logp=head_spelling(x)[0], q=torch.randn(E, M, A, generator=g) * 2,
            action=torch.randint(0, A, (M, 1), generator=g).float(), y=torch.randn(M, 1, generator=g),
            mask=(torch.rand(M, 1, generator=g) >= 0.3).float(), dlogp=torch.randn(M, A, generator=g), dprobs=torch.randn(M, A, generator=g))
    return _BATCH[(E, M, A)]


def leaf(t, dtype, device):
    return t.to(dtype=dtype, device=device).clone().requires_grad_(True)


LA = torch.tensor([LOG_ALPHA])


# ------------------------------------------------------------------------------------------------ 1. head, forward
@pytest.mark.parametrize('M,A', SHAPES)
def test_head_forward_against_fp64(ops, M, A):
    x, p64, logp64, _ = case(M, A)
    mode, logp, probs = ops.categorical_head(x.cuda(), FLOOR)
    assert mode.shape == (M,) and mode.dtype == torch.float32 and logp.shape == (M, A) and probs.shape == (M, A)
    mode, logp, probs = mode.cpu(), logp.cpu(), probs.cpu()
    rel = (3 * (A - 1) + 12) * EPS
    bound = rel + 4 * EPS * logp64.abs()
    r_lp = ((logp.double() - logp64).abs() / bound).max().item()
    r_p = ((probs.double() - p64).abs() / (rel * p64)).max().item()
    print(f'\n[categorical_head M={M} A={A}] largest |logp - logp64| / bound = {r_lp:.3f}, |p - p64| / bound = {r_p:.3f}')
    assert torch.isfinite(logp).all() and torch.isfinite(probs).all()
    assert r_lp <= 1.0 and r_p <= 1.0, (r_lp, r_p)
    top = torch.sort(p64, dim=-1, descending=True).values
    clear = (top[:, 0] - top[:, 1] > rel * top[:, 0]) if A > 1 else torch.ones(M, dtype=torch.bool)
    assert torch.equal(mode.long()[clear], p64.argmax(dim=-1)[clear])
    assert torch.equal(mode, mode.round()) and mode.min() >= 0 and mode.max() <= A - 1


@pytest.mark.parametrize('M,A', SHAPES)
def test_head_forward_is_the_step_kernel_bit_for_bit(ops, M, A):
    """One device function does the row arithmetic of both kernels; a narrower lane group only drops additions of zero."""
    x = case(M, A)[0].cuda()
    mode, logp, probs = ops.categorical_head(x, FLOOR)
    smode, _, slogp = ops.categorical_step(x, torch.full((M,), 0.5, device='cuda'), FLOOR)
    assert torch.equal(logp.view(torch.int32), slogp.view(torch.int32)) and torch.equal(mode, smode)


def test_head_takes_any_leading_shape(ops):
    x = case(6, 5)[0].cuda()
    mode, logp, probs = ops.categorical_head(x.reshape(2, 3, 5), FLOOR)
    m2, l2, p2 = ops.categorical_head(x, FLOOR)
    assert mode.shape == (2, 3) and logp.shape == (2, 3, 5) and probs.shape == (2, 3, 5)
    assert torch.equal(logp.reshape(6, 5), l2) and torch.equal(probs.reshape(6, 5), p2) and torch.equal(mode.reshape(6), m2)
    assert not mode.requires_grad


@pytest.mark.parametrize('A', [7, 130])
def test_head_nan_row_stays_in_its_row(ops, A):
    x = case(4, A)[0].clone()
    clean = [t.cpu() for t in ops.categorical_head(x.cuda(), FLOOR)]
    bad = 2
    x[bad, A // 2] = float('nan')
    mode, logp, probs = [t.cpu() for t in ops.categorical_head(x.cuda(), FLOOR)]
    assert torch.isnan(logp[bad]).all() and torch.isnan(probs[bad]).all() and mode[bad] == 0
    keep = [r for r in range(4) if r != bad]
    assert torch.equal(logp[keep].view(torch.int32), clean[1][keep].view(torch.int32))
    assert torch.equal(probs[keep].view(torch.int32), clean[2][keep].view(torch.int32)) and torch.equal(mode[keep], clean[0][keep])


# ------------------------------------------------------------------------------------------------ 2. head, backward
@pytest.mark.parametrize('which', ['logp', 'probs', 'both'])
@pytest.mark.parametrize('M,A', SHAPES)
def test_head_backward(ops, M, A, which):
    b = batch(1, M, A)

    def grad(dtype, device, head):
        x = leaf(b['x'], dtype, device)
        logp, probs = head(x)
        loss = 0
        if which in ('logp', 'both'):
            loss = loss + (logp * b['dlogp'].to(dtype=dtype, device=device)).sum()
        if which in ('probs', 'both'):
            loss = loss + (probs * b['dprobs'].to(dtype=dtype, device=device)).sum()
        loss.backward()
        return x.grad

    ref = grad(torch.float64, 'cpu', head_spelling)
    t32 = grad(torch.float32, 'cuda', head_spelling)
    got = grad(torch.float32, 'cuda', lambda x: ops.categorical_head(x, FLOOR)[1:])
    within(f'head bwd {which} M={M} A={A}', got, ref, t32)
    if A == 1:
        assert torch.equal(got.cpu(), torch.zeros(M, 1))            # exactly 0


# ------------------------------------------------------------------------------------------------ 3. all-action value
@pytest.mark.parametrize('E,subset', [(1, None), (2, None), (8, None), (8, [5, 1])])
@pytest.mark.parametrize('M,A', SHAPES)
def test_discrete_value(ops, M, A, E, subset):
    b = batch(E, M, A)
    ref = value_spelling(b['q'].double(), subset, b['logp'].double(), LA.double())
    t32 = value_spelling(b['q'].cuda(), subset, b['logp'].cuda(), LA.cuda())
    sub = None if subset is None else torch.tensor(subset, dtype=torch.int32, device='cuda')
    got = ops.discrete_value(b['q'].cuda(), sub, b['logp'].cuda(), LA.cuda())
    assert got.shape == (M, 1) and not got.requires_grad
    within(f'value M={M} A={A} E={E} subset={subset}', got, ref, t32)


# ------------------------------------------------------------------------------------------------ 4. critic loss on the taken action
def q_taken(b, dtype, device, fn, mask=None, action=None):
    q = leaf(b['q'], dtype, device)
    to = lambda t: t.to(dtype=dtype, device=device)
    loss = fn(q, to(b['action'] if action is None else action), to(b['y']), to(b['mask'] if mask is None else mask))
    (loss * G_UP).backward()
    return loss.detach(), q.grad


@pytest.mark.parametrize('E', ENSEMBLES)
@pytest.mark.parametrize('M,A', SHAPES)
def test_q_taken_loss(ops, M, A, E):
    b = batch(E, M, A)
    ref = q_taken(b, torch.float64, 'cpu', q_taken_spelling)
    t32 = q_taken(b, torch.float32, 'cuda', q_taken_spelling)
    got = q_taken(b, torch.float32, 'cuda', ops.masked_q_taken_loss)
    within(f'q_taken sum M={M} A={A} E={E}', got[0], ref[0], t32[0])
    within(f'q_taken dq M={M} A={A} E={E}', got[1], ref[1], t32[1])
    dq = got[1].cpu()
    assert dq.shape == (E, M, A)
    hit = torch.zeros(M, A, dtype=torch.bool).scatter_(1, b['action'].long(), True) & (b['mask'] != 0)
    assert torch.equal(dq[:, ~hit], torch.zeros_like(dq[:, ~hit]))    # exactly 0 off the taken action and on masked rows
    again = q_taken(b, torch.float32, 'cuda', ops.masked_q_taken_loss)
    assert torch.equal(again[0].view(torch.int32), got[0].view(torch.int32)) and torch.equal(again[1], got[1])


def test_q_taken_masked_row_with_an_index_out_of_range(ops):
    """A padded row (mask 0) whose index is A + 3: the read is clamped, every result is bit-identical to the same call with index 0."""
    E, M, A = 8, 257, 6
    b = batch(E, M, A)
    row = 200
    mask = b['mask'].clone()
    mask[row] = 0
    bad, zero = b['action'].clone(), b['action'].clone()
    bad[row], zero[row] = A + 3, 0
    l1, d1 = q_taken(b, torch.float32, 'cuda', ops.masked_q_taken_loss, mask=mask, action=bad)
    l0, d0 = q_taken(b, torch.float32, 'cuda', ops.masked_q_taken_loss, mask=mask, action=zero)
    assert torch.equal(l1.view(torch.int32), l0.view(torch.int32)) and torch.equal(d1.view(torch.int32), d0.view(torch.int32))
    assert torch.equal(d1[:, row].cpu(), torch.zeros(E, A))
    # the rows at the very end of the batch too: one past them is the end of the buffer
    bad[M - 1], zero[M - 1], mask[M - 1] = A + 3, 0, 0
    l1, d1 = q_taken(b, torch.float32, 'cuda', ops.masked_q_taken_loss, mask=mask, action=bad)
    l0, d0 = q_taken(b, torch.float32, 'cuda', ops.masked_q_taken_loss, mask=mask, action=zero)
    assert torch.equal(l1.view(torch.int32), l0.view(torch.int32)) and torch.equal(d1.view(torch.int32), d0.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 5. actor loss over all actions
def actor(b, dtype, device, fn, reduce_min, mask=None, q=None, q_grad=True):
    logp = leaf(b['logp'], dtype, device)
    qq = (b['q'] if q is None else q).to(dtype=dtype, device=device).clone().requires_grad_(q_grad)
    to = lambda t: t.to(dtype=dtype, device=device)
    loss, stat = fn(logp, qq, to(b['mask'] if mask is None else mask), to(LA), reduce_min)
    (loss * G_UP).backward()
    return loss.detach(), stat.detach(), logp.grad, qq.grad


@pytest.mark.parametrize('reduce_min', [True, False])
@pytest.mark.parametrize('E', ENSEMBLES)
@pytest.mark.parametrize('M,A', SHAPES)
def test_discrete_actor_loss(ops, M, A, E, reduce_min):
    b = batch(E, M, A)
    ref = actor(b, torch.float64, 'cpu', actor_spelling, reduce_min)
    t32 = actor(b, torch.float32, 'cuda', actor_spelling, reduce_min)
    got = actor(b, torch.float32, 'cuda', ops.masked_discrete_actor_loss, reduce_min)
    tag = f'M={M} A={A} E={E} {"min" if reduce_min else "mean"}'
    for nm, g, r, t in zip(('actor sum', 'actor sum p logp', 'actor dlogp', 'actor dq'), got, ref, t32):
        within(f'{nm} {tag}', g, r, t)
    assert not got[1].requires_grad and got[3].shape == (E, M, A)
    again = actor(b, torch.float32, 'cuda', ops.masked_discrete_actor_loss, reduce_min)
    for a, g in zip(again, got):                                      # fixed-order sums: bitwise reproducible
        assert torch.equal(a.view(torch.int32), g.view(torch.int32))
    frozen = actor(b, torch.float32, 'cuda', ops.masked_discrete_actor_loss, reduce_min, q_grad=False)      # the trainer's call: no dq
    assert frozen[3] is None and torch.equal(frozen[2], got[2]) and torch.equal(frozen[0], got[0])


def test_actor_min_gives_the_gradient_to_the_first_of_two_equal_minima(ops):
    E, M, A = 4, 3, 4
    b = batch(E, M, A)
    q = b['q'].clone()
    q[1], q[3] = -50.0, -50.0                                        # members 1 and 3 tie for the minimum everywhere
    mask = torch.ones(M, 1)
    _, _, _, dq = actor(b, torch.float32, 'cuda', ops.masked_discrete_actor_loss, True, mask=mask, q=q)
    dq = dq.cpu()
    want = -G_UP * b['logp'].exp()
    assert torch.allclose(dq[1], want, rtol=1e-6, atol=0) and (dq[1] != 0).all()
    assert torch.equal(dq[[0, 2, 3]], torch.zeros(3, M, A))


# ------------------------------------------------------------------------------------------------ 6. an all-zero mask
@pytest.mark.parametrize('M,A', [(3, 4), (257, 6), (2, 130)])
def test_all_zero_mask_gives_exact_zeros(ops, M, A):
    E = 8
    b = batch(E, M, A)
    mask = torch.zeros(M, 1)
    loss, dq = q_taken(b, torch.float32, 'cuda', ops.masked_q_taken_loss, mask=mask)
    assert loss.item() == 0.0 and torch.equal(dq.cpu(), torch.zeros(E, M, A))
    for reduce_min in (True, False):
        loss, stat, dlogp, dq = actor(b, torch.float32, 'cuda', ops.masked_discrete_actor_loss, reduce_min, mask=mask)
        assert loss.item() == 0.0 and stat.item() == 0.0
        assert torch.equal(dlogp.cpu(), torch.zeros(M, A)) and torch.equal(dq.cpu(), torch.zeros(E, M, A))
