"""The two fused-epilogue GEMMs of the efc-E critic head, `ops.gemm_f32_head` (`gemm_ws_kernel<.., 5>` + `head_fold_kernel`) and
`ops.gemm_f32_dact` (`gemm_ws_kernel<.., 4>` over the whole 256-row tiles, the plain product + `dact_tail_kernel` over the rows behind
them, `launch_colsum`), each called ON ITS OWN against an fp64 reference, and the plain product pinned to mode 2 at ragged shapes.
GPU box only; the case tables and references import without one (tests/test_gemm_fused_host.py reads them).

Operands: fp32 `randn` from a seeded CPU generator, taken up exactly into fp64; A unit scale, B / sqrt(K), biases, w3 and b3 unit scale.
Bounds: the project's own for a product against fp64 (`test_gemm_f32_vs_fp64_product`): `close(rtol=1e-5, atol_scale=1e-6)`, norm-wise,
for a, q, out and dbias.  Two checks carry no measured number: the column sums against the kernel's OWN out and the row dots against
the kernel's OWN a, each inside the rigorous bound of an fp32 sum in any order (`held_colsum`, `held_rowdot`).  Every call is made
twice and must be bit-equal (no atomics on these paths).  Every comparison prints its error as a fraction of its bound (`FUSED-FIG`
lines under `pytest -s`; profiles/r27_fused_epilogue_tests.md keeps the measured ones)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0beef                                 # a quiet NaN with a payload: no kernel output compares equal to it by accident
RTOL, ATOL_SCALE = 1e-5, 1e-6

# (batch, M, N, K): what each is the smallest instance of is said in profiles/r27_fused_epilogue_tests.md
HEAD_CASES = [(1, 129, 4, 32), (2, 256, 128, 32), (2, 255, 128, 64), (3, 257, 128, 96), (2, 384, 160, 128), (2, 300, 144, 64),
              (2, 260, 68, 32), (1, 512, 36, 256), (2, 400, 252, 160), (8, 1044, 256, 256), (1, 1024, 512, 1024)]
HEAD_NODE_CASES = [(2, 384, 160, 128), (8, 1044, 256, 256)]
DACT_CASES = [(1, 256, 128, 32), (2, 257, 128, 64), (2, 264, 256, 96), (1, 265, 128, 32), (3, 384, 128, 160), (2, 385, 256, 128),
              (1, 511, 128, 256), (2, 768, 384, 32), (8, 1044, 256, 256), (1, 512, 128, 1024)]
DACT_DENSE_CASES = [(2, 257, 128, 64), (2, 768, 384, 32)]
DACT_NODBIAS_CASES = [(2, 257, 128, 64), (2, 385, 256, 128), (2, 768, 384, 32)]
BIG = (8, 1044, 256, 256)                             # configs[1]'s widths: the one case whose output is large enough for a magnitude slot

# plain product in mode 2: (M, N, K); K a multiple of 32 -> third edition (whole K steps), else second edition (K tail)
MODE2_SHAPES = [(129, 132, 32), (257, 260, 64), (300, 4, 96), (513, 36, 256), (129, 132, 36), (257, 260, 100), (300, 256, 44), (513, 384, 200)]
# (a_kcontig, b_kcontig, bias + ELU, batch): the four layouts, options paired instead of the full product
MODE2_OPTIONS = [(True, True, False, 1), (True, False, True, 3), (False, True, True, 1), (False, False, False, 3), (True, True, True, 3)]


def mode2_cases():
    """MODE2_SHAPES x MODE2_OPTIONS; where A is [K, M] its rows must be whole float4s for the matrix-core editions: M rounded up to 4."""
    return [((M + 3) // 4 * 4 if not akc else M, N, K, akc, bkc, be, batch) for (M, N, K) in MODE2_SHAPES for (akc, bkc, be, batch) in MODE2_OPTIONS]


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


@pytest.fixture(autouse=True)
def mode2(ops, monkeypatch):
    """Product mode 2 in force (the default of the trainers): outputs of 2^20 elements and more then get a magnitude slot."""
    monkeypatch.setattr(ops, 'GEMM_SPLIT', 2)


def close(got, ref, rtol=1e-4, atol_scale=2e-5, name=''):
    got = got.detach().float().cpu()
    ref = ref.detach().float()
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got - ref).abs().max().item()
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    assert err <= rtol * scale + atol_scale * scale, f'{name}: max err {err:.3e} vs scale {scale:.3e}'


def _fraction(got, ref, rtol, atol_scale):
    """The error of `got` as a fraction of the bound `close` holds it to (measurement only: the assertion is `close`'s)."""
    got, ref = got.detach().float().cpu(), ref.detach().float()
    scale = max(ref.abs().max().item(), 1e-6)
    return (got - ref).abs().max().item() / ((rtol + atol_scale) * scale)


def held(case, name, got, ref):
    print(f'FUSED-FIG {case} {name} {_fraction(got, ref, RTOL, ATOL_SCALE):.4f}')
    close(got, ref, rtol=RTOL, atol_scale=ATOL_SCALE, name=f'{case} {name}')


def colsum_excess(dbias, out):
    """max over columns of |dbias - sum_m out (fp64)| / (1.01 M 2^-24 sum_m |out|): the rigorous bound of an fp32 sum of M terms in any
    order (each of the M - 1 additions rounds once, relative 2^-24, a partial sum of at most sum |out|; second-order terms under the 1.01).
    dbias [batch, N] and out [batch, M, N] on the CPU."""
    M = out.shape[-2]
    o = out.double()
    err = (dbias.double() - o.sum(-2)).abs()
    bound = 1.01 * M * 2.0 ** -24 * o.abs().sum(-2)
    return (err / bound.clamp_min(1e-300)).max().item()


def rowdot_excess(q, a, w3, b3):
    """max over rows of |q - t| / (1.01 (N + 1) 2^-23 (sum_n |a w3| + |b3|)), t = sum_n a w3 + b3 in fp64 over the fp32 a: one rounding
    per product and one per addition.  q [batch, M], a [batch, M, N], w3 [batch, N], b3 [batch] or None, on the CPU."""
    N = a.shape[-1]
    terms = a.double() * w3.double().unsqueeze(-2)
    b = torch.zeros(a.shape[0], dtype=torch.float64) if b3 is None else b3.double()
    err = (q.double() - (terms.sum(-1) + b.unsqueeze(-1))).abs()
    bound = 1.01 * (N + 1) * 2.0 ** -23 * (terms.abs().sum(-1) + b.abs().unsqueeze(-1))
    return (err / bound.clamp_min(1e-300)).max().item()


def held_colsum(case, dbias, out):
    frac = colsum_excess(dbias.cpu(), out.cpu())
    print(f'FUSED-FIG {case} colsum-own {frac:.4f}')
    assert torch.isfinite(dbias).all() and frac <= 1.0, f'{case}: a column sum at {frac:.3g} x the fp32 summation bound over the kernel\'s own out'


def held_rowdot(case, q, a, w3, b3):
    frac = rowdot_excess(q.cpu(), a.cpu(), w3, b3)
    print(f'FUSED-FIG {case} rowdot-own {frac:.4f}')
    assert torch.isfinite(q).all() and frac <= 1.0, f'{case}: a row dot at {frac:.3g} x the fp32 bound over the kernel\'s own a'


def held_handle(ops, case, name, t):
    """A kernel publishes the maximum of what it stores: the handle of t equals max |t|, to the bit."""
    h = ops.amax_of(t)
    assert h is not None, f'{case} {name}: no magnitude handle on an output of {t.numel()} elements'
    top, val = t.abs().max().item(), ops.amax_value(h)
    print(f'FUSED-AMAX {case} {name} handle {val:.9g} max {top:.9g}')
    assert val == top, f'{case} {name}: handle {val!r} != max |.| {top!r}'


def sentinel_fill(t):
    t.view(torch.int32).fill_(SENTINEL)
    return t


def is_sentinel(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


@pytest.fixture
def poisoned_ws(ops, monkeypatch):
    """Every workspace of the calls under test arrives full of the NaN sentinel: a partial row the kernel should have written and did not
    then reaches q / dbias as NaN.  Before the call a buffer of the workspace's size is filled and freed (`poison`), so that the caching
    allocator hands the block to the call; `ops._ws` is wrapped to say whether it did (FUSED-WS lines) and to fill the block where it
    did not.  -> poison(nbytes)."""
    state = {'ptr': None}
    plain = ops._ws

    def poison(nbytes):
        buf = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device='cuda')
        sentinel_fill(buf[:buf.numel() // 4 * 4])
        state['ptr'] = buf.data_ptr()

    def ws(nbytes, device):
        buf = plain(nbytes, device)
        same = buf.data_ptr() == state['ptr']
        print(f'FUSED-WS {buf.numel()} bytes: the allocator {"returned" if same else "did NOT return"} the poisoned block')
        if not same:
            sentinel_fill(buf[:buf.numel() // 4 * 4])
        return buf

    monkeypatch.setattr(ops, '_ws', ws)
    return poison


# ------------------------------------------------------------------------------------------------ inputs and references
def head_reference(A, B, bias, w3, b3, dtype=torch.float64):
    """a = elu(A B + bias), q = a . w3 + b3 in `dtype`.  A [batch, M, K], B [batch, K, N], bias / w3 [batch, N], b3 [batch] or None."""
    A, B, bias, w3 = (t.to(dtype) for t in (A, B, bias, w3))
    a = torch.nn.functional.elu(torch.matmul(A, B) + bias.unsqueeze(-2))
    q = (a * w3.unsqueeze(-2)).sum(-1)
    return a, (q if b3 is None else q + b3.to(dtype).unsqueeze(-1))


def dact_reference(A, B, Y, dtype=torch.float64):
    """out = (A B) * elu'(Y) with elu' from the ELU OUTPUT (y > 0 ? 1 : y + 1), dbias = column sums of out, in `dtype`.
    A [batch, M, K], B [batch, K, N], Y [batch, M, N]."""
    A, B, Y = (t.to(dtype) for t in (A, B, Y))
    out = torch.matmul(A, B) * torch.where(Y > 0, torch.ones_like(Y), Y + 1)
    return out, out.sum(-2)


def _generator(kind, batch, M, N, K):
    return torch.Generator().manual_seed(kind + 1000003 * batch + 7919 * M + 101 * N + K)


def head_inputs(batch, M, N, K):
    g = _generator(5, batch, M, N, K)
    rnd = lambda *s: torch.randn(*s, generator=g)
    return dict(A=rnd(batch, M, K), B=rnd(batch, K, N) / K ** 0.5, bias=rnd(batch, N), w3=rnd(batch, N), b3=rnd(batch))


def make_y(batch, M, N, g):
    """An ELU output, as in production, with row 0 exactly -1 (factor 0) and row 1 exactly 0 (the y > 0 comparison's edge)."""
    Y = torch.nn.functional.elu(torch.randn(batch, M, N, generator=g))
    Y[..., 0, :] = -1.0
    Y[..., 1, :] = 0.0
    return Y


def dact_inputs(batch, M, N, K):
    g = _generator(4, batch, M, N, K)
    rnd = lambda *s: torch.randn(*s, generator=g)
    return dict(A=rnd(batch, M, K), B=rnd(batch, K, N) / K ** 0.5, Y=make_y(batch, M, N, g))


@functools.lru_cache(maxsize=None)
def head_case(batch, M, N, K):
    """Inputs and fp64 reference of one shape: computed once, shared by both layouts and every variant, never modified."""
    c = head_inputs(batch, M, N, K)
    return c, head_reference(c['A'], c['B'], c['bias'], c['w3'], c['b3'])


@functools.lru_cache(maxsize=None)
def dact_case(batch, M, N, K):
    c = dact_inputs(batch, M, N, K)
    return c, dact_reference(c['A'], c['B'], c['Y'])


def weight(B, b_kcontig):
    """The [batch, K, N] weight in the layout the call names: as it is, or [batch, N, K]."""
    return (B.transpose(-1, -2).contiguous() if b_kcontig else B).cuda()


def token_major(t, pad=0, lead=0):
    """t [E, M, C] as the [E, M, C] view of a token-major [M, lead + E C + pad] buffer on the GPU (row stride lead + E C + pad, member
    stride C), the buffer sentinel-filled first.  -> (view, buffer)."""
    E, M, C = t.shape
    buf = sentinel_fill(torch.empty(M, lead + E * C + pad, dtype=torch.float32, device='cuda'))
    view = buf[:, lead:lead + E * C].unflatten(1, (E, C)).permute(1, 0, 2)
    view.copy_(t)
    return view, buf


# ------------------------------------------------------------------------------------------------ head
def run_head(ops, poison, c, b_kcontig, node=False, b3=True, loose=False):
    batch, M, K = c['A'].shape
    N = c['B'].shape[-1]
    A = token_major(c['A'])[0] if node else c['A'].cuda()
    Bw = weight(c['B'], b_kcontig)
    if node:
        bias = sentinel_fill(torch.empty(batch, N + 4, dtype=torch.float32, device='cuda'))[:, :N]
        bias.copy_(c['bias'])
    else:
        bias = c['bias'].cuda()
    w3 = c['w3'].cuda()
    b3v = None if b3 is None else (c['b3'] if b3 is True else b3).cuda()
    ha, hb = (ops.amax(3 * A.contiguous()), ops.amax(3 * Bw)) if loose else (ops.amax(A), ops.amax(Bw))
    poison(ops.lib().resel_gemm_f32_fused_workspace_bytes(M, N, K, batch, 5))
    a, q = ops.gemm_f32_head(A, Bw, b_kcontig, bias, w3, b3v, amax_a=ha, amax_b=hb)
    poison(ops.lib().resel_gemm_f32_fused_workspace_bytes(M, N, K, batch, 5))
    a2, q2 = ops.gemm_f32_head(A, Bw, b_kcontig, bias, w3, b3v, amax_a=ha, amax_b=hb)
    assert a.shape == (batch, M, N) and q.shape == (batch, M)
    assert torch.equal(a, a2) and torch.equal(q, q2), 'a second call differs (there are no atomics on this path)'
    return a, q


def check_head(case, c, ref, a, q, b3=True):
    held(case, 'a', a, ref[0])
    held(case, 'q', q, ref[1])
    held_rowdot(case, q, a, c['w3'], None if b3 is None else c['b3'])


@pytest.mark.parametrize('b_kcontig', [False, True])
@pytest.mark.parametrize('batch,M,N,K', HEAD_CASES)
def test_head_vs_fp64(ops, poisoned_ws, batch, M, N, K, b_kcontig):
    """`ops.gemm_f32_head` on dense operands in the node's weight layout (B [batch, K, N]) and the other one: a and q against fp64, q
    against the kernel's own a, a poisoned workspace, two calls bit-equal; at configs[1]'s widths the handle of a is max |a| to the bit."""
    case = f'head({batch},{M},{N},{K}){"nk" if b_kcontig else "kn"}'
    c, ref = head_case(batch, M, N, K)
    a, q = run_head(ops, poisoned_ws, c, b_kcontig)
    check_head(case, c, ref, a, q)
    if (batch, M, N, K) == BIG:
        held_handle(ops, case, 'a', a)


@pytest.mark.parametrize('batch,M,N,K', HEAD_NODE_CASES)
def test_head_node_layout_vs_fp64(ops, poisoned_ws, batch, M, N, K):
    """A as the [E, M, K] view of a token-major [M, E K] buffer (lda = E K, batch stride K) and the bias as a view with row stride N + 4:
    what `_CriticMLP` hands the entry."""
    case = f'head({batch},{M},{N},{K})node'
    c, ref = head_case(batch, M, N, K)
    a, q = run_head(ops, poisoned_ws, c, False, node=True)
    check_head(case, c, ref, a, q)


def test_head_loose_handles_vs_fp64(ops, poisoned_ws):
    """Handles that are bounds about three times above the maxima, as a store-wide weight handle is: same bound."""
    shape = (2, 384, 160, 128)
    c, ref = head_case(*shape)
    a, q = run_head(ops, poisoned_ws, c, False, loose=True)
    check_head('head(2,384,160,128)loose', c, ref, a, q)


@pytest.mark.parametrize('batch,M,N,K', [(2, 384, 160, 128), (1, 129, 4, 32)])
def test_head_without_b3_equals_zero_b3(ops, poisoned_ws, batch, M, N, K):
    """`b3 = None` gives q bit-equal to the `b3 = zeros` run, and both are the reference without the output bias."""
    case = f'head({batch},{M},{N},{K})no-b3'
    c, _ = head_case(batch, M, N, K)
    a0, q0 = run_head(ops, poisoned_ws, c, False, b3=None)
    a1, q1 = run_head(ops, poisoned_ws, c, False, b3=torch.zeros(batch))
    assert torch.equal(q0, q1) and torch.equal(a0, a1)
    ref = head_reference(c['A'], c['B'], c['bias'], c['w3'], None)
    check_head(case, c, ref, a0, q0, b3=None)


# ------------------------------------------------------------------------------------------------ dact
def run_dact(ops, poison, c, b_kcontig, node=True, need_dbias=True, a_scale=None):
    """-> (out, dbias, A as the call saw it on the CPU).  node: Y and out as [E, M, N] views of token-major buffers, out's buffer 8 columns
    wider than the kernel owns (4 in front, 4 behind), which must still hold the sentinel afterwards."""
    batch, M, K = c['A'].shape
    N = c['B'].shape[-1]
    A = c['A'] if a_scale is None else c['A'] * a_scale
    Ad, Bw = A.cuda(), weight(c['B'], b_kcontig)
    Y = token_major(c['Y'])[0] if node else c['Y'].cuda()
    ha, hb = ops.amax(Ad), ops.amax(Bw)
    res = []
    for _ in range(2):
        if node:
            out, buf = token_major(torch.zeros(batch, M, N), pad=4, lead=4)
            sentinel_fill(buf)
        else:
            out, buf = sentinel_fill(torch.empty(batch, M, N, dtype=torch.float32, device='cuda')), None
        poison(ops.lib().resel_gemm_f32_fused_workspace_bytes(M, N, K, batch, 4))
        o, dbias = ops.gemm_f32_dact(Ad, Bw, b_kcontig, Y, out, need_dbias=need_dbias, amax_a=ha, amax_b=hb)
        assert o is out and (dbias is None) == (not need_dbias)
        if node:
            assert out.stride(-2) % 4 == 0 and out.data_ptr() % 16 == 0
            assert is_sentinel(buf[:, :4]) and is_sentinel(buf[:, 4 + batch * N:]), 'the kernel wrote outside the columns it owns'
        res.append((out, dbias))
    (o1, d1), (o2, d2) = res
    assert torch.equal(o1, o2) and (d1 is None or torch.equal(d1, d2)), 'a second call differs (there are no atomics on this path)'
    return o1, d1, A


def check_dact(case, ref, out, dbias):
    held(case, 'out', out, ref[0])
    if dbias is not None:
        held(case, 'dbias', dbias, ref[1])
        held_colsum(case, dbias, out)


@pytest.mark.parametrize('b_kcontig', [True, False])
@pytest.mark.parametrize('batch,M,N,K', DACT_CASES)
def test_dact_vs_fp64(ops, poisoned_ws, batch, M, N, K, b_kcontig):
    """`ops.gemm_f32_dact` in the node's layout (Y and out column blocks of token-major buffers), the weight [batch, N, K] as in the node
    and the other way: out and dbias against fp64, dbias against the kernel's own out, the columns around out untouched, two calls
    bit-equal; at configs[1]'s widths the handle of out (two publishers: body and tail) is max |out| to the bit."""
    case = f'dact({batch},{M},{N},{K}){"nk" if b_kcontig else "kn"}'
    c, ref = dact_case(batch, M, N, K)
    out, dbias, _ = run_dact(ops, poisoned_ws, c, b_kcontig)
    check_dact(case, ref, out, dbias)
    assert (out[:, 0] == 0).all(), 'Y = -1 exactly: factor 0'
    if (batch, M, N, K) == BIG:
        held_handle(ops, case, 'out', out)


@pytest.mark.parametrize('batch,M,N,K', DACT_DENSE_CASES)
def test_dact_dense_operands_vs_fp64(ops, poisoned_ws, batch, M, N, K):
    case = f'dact({batch},{M},{N},{K})dense'
    c, ref = dact_case(batch, M, N, K)
    out, dbias, _ = run_dact(ops, poisoned_ws, c, True, node=False)
    check_dact(case, ref, out, dbias)


@pytest.mark.parametrize('batch,M,N,K', DACT_NODBIAS_CASES)
def test_dact_without_dbias_is_bit_equal(ops, poisoned_ws, batch, M, N, K):
    """`need_dbias=False`: None for dbias and out bit-equal to the run that sums the columns."""
    c, ref = dact_case(batch, M, N, K)
    out, dbias, _ = run_dact(ops, poisoned_ws, c, True)
    out0, none, _ = run_dact(ops, poisoned_ws, c, True, need_dbias=False)
    assert none is None and dbias is not None and torch.equal(out, out0)
    held(f'dact({batch},{M},{N},{K})no-dbias', 'out', out0, ref[0])


@pytest.mark.parametrize('which', ['tail', 'body'])
def test_dact_handle_has_two_publishers(ops, poisoned_ws, which):
    """The whole-tile body and `dact_tail_kernel` publish into one slot: with the tail rows of A (M = 1044: rows 1024 ..) or its first 256
    rows a hundred times larger, the handle is max |out| to the bit both times - and that maximum lies where the scaling put it."""
    batch, M, N, K = BIG
    c, _ = dact_case(*BIG)
    scale = torch.ones(1, M, 1)
    scale[:, (slice(1024, None) if which == 'tail' else slice(0, 256))] = 100.0
    out, dbias, A = run_dact(ops, poisoned_ws, c, True, a_scale=scale)
    case = f'dact(8,1044,256,256)x100-{which}'
    check_dact(case, dact_reference(A, c['B'], c['Y']), out, dbias)
    held_handle(ops, case, 'out', out)
    top_tail, top_body = out[:, 1024:].abs().max().item(), out[:, :1024].abs().max().item()
    assert (top_tail > 10 * top_body) if which == 'tail' else (top_body > 10 * top_tail)


# ------------------------------------------------------------------------------------------------ plain product, mode 2
@pytest.mark.parametrize('M,N,K,akc,bkc,bias_elu,batch', mode2_cases())
def test_gemm_f32_mode2_ragged_shapes_vs_fp64(ops, M, N, K, akc, bkc, bias_elu, batch):
    """`ops.gemm_f32(..., split=2)` with both handles given (the wrapper cannot fall back to mode 6) at ragged M / N and small K in the four
    layouts: K a multiple of 32 runs the third edition (`gemm_ws_kernel<.., 0>`), a K tail the second (`gemm_bf3_kernel<.., 2>`).
    Reference and bound of `test_gemm_f32_vs_fp64_product`."""
    case = f'mode2({M},{N},{K}){"mk" if akc else "km"}-{"nk" if bkc else "kn"}{"+bias+elu" if bias_elu else ""}x{batch}'
    g = torch.Generator().manual_seed(M + N + K + 2 * akc + bkc + batch)
    sh = (batch,) if batch > 1 else ()
    A = torch.randn(*sh, *((M, K) if akc else (K, M)), generator=g)
    B = torch.randn(*sh, *((N, K) if bkc else (K, N)), generator=g) / K ** 0.5
    b = torch.randn(*sh, N, generator=g) if bias_elu else None
    ref = (A.double() if akc else A.double().transpose(-1, -2)) @ (B.double().transpose(-1, -2) if bkc else B.double())
    if bias_elu:
        ref = torch.nn.functional.elu(ref + b.double().unsqueeze(-2))
    Ad, Bd, bd = A.cuda(), B.cuda(), None if b is None else b.cuda()
    ha, hb = ops.amax(Ad), ops.amax(Bd)
    outs = []
    for _ in range(2):
        ops.LAST_SPLIT[0] = None
        outs.append(ops.gemm_f32(Ad, Bd, akc, bkc, bd, 'elu' if bias_elu else None, split=2, amax_a=ha, amax_b=hb))
        assert ops.LAST_SPLIT[0] == 2, 'the product did not run in mode 2'
    held(case, 'out', outs[0], ref.float())
    assert torch.equal(outs[0], outs[1])                # bitwise reproducible (no atomics)
