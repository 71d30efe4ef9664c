"""The cgpt attention core and the decode step at head widths beyond 32 and 64, against the fp64 model of tests/attention_parity.py in
its metric and at its bounds (OUT_TOL 1e-2 / GRAD_TOL 2e-2 per (head, 128-token block), lse2 at 1e-4 |ref| + 1e-4, decode 1e-2 per
(position, head)): hd = 128 on its own kernels, hd = 16 / 96 / 8 zero-padded to 32 / 128 / 32 (`resel_head_pad`, scale of the TRUE width).
tests/test_attention_head_dims_host.py shows on the CPU that a correct bf16 pipeline uses at most half of each bound on these cases and
that a kernel which loses one score tile exceeds them.  Every comparison prints `ATTN-FIG <case> <name> <fraction of bound>` before it
asserts (`pytest -s`); profiles/r31_attention_head_dims.md keeps the fractions measured on an MI355X.  No bound was fitted to them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attention_head_dims as HD
import attention_parity as AP
from oracle import kernels as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))                 # the fp64 model runs on the host
    yield o
    torch.set_num_threads(before)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _nan_like(shape, dtype, dev='cuda'):
    return torch.full(shape, float('nan'), dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def _pad(ops, x, hdp):
    """[T, n, H, hd] -> [T, n, H, hdp] through `resel_head_pad` into a NaN-filled buffer."""
    from offpolicy_rnn.hip._lib import check, lib
    T, n, H, hd = x.shape
    out = _nan_like((T, n, H, hdp), torch.bfloat16)
    check(lib().resel_head_pad(_ptr(x), _ptr(out), T, n, H, hd, hdp, ops._stream()), 'head_pad')
    return out


def _unpad(ops, x, hd):
    from offpolicy_rnn.hip._lib import check, lib
    T, n, H, hdp = x.shape
    out = _nan_like((T, n, H, hd), torch.bfloat16)
    check(lib().resel_head_unpad(_ptr(x), _ptr(out), T, n, H, hd, hdp, ops._stream()), 'head_unpad')
    return out


@functools.lru_cache(maxsize=None)
def _case_and_ref(name):
    case = HD.make_case(name)
    return case, AP.model_of(case)


def _run_core(ops, case, cu=None, T=None, padded=False, max_seqlen=None):
    """Forward and backward through the C entries at the kernel width into NaN-filled buffers -> (out [T, H, hd] bf16, lse [H, T] fp32,
    dqkv [T, 3, H, hd] bf16) on the device, at the TRUE width.  `cu`, `T`, `padded`: a padded problem over the same tokens."""
    from offpolicy_rnn.hip._lib import check, lib
    dev = torch.device('cuda')
    n, _, H, hd = case['qkv'].shape
    T = n if T is None else T
    qkv, dout = torch.zeros(T, 3, H, hd, dtype=torch.bfloat16), torch.zeros(T, 1, H, hd, dtype=torch.bfloat16)
    qkv[:n], dout[:n, 0] = case['qkv'], case['dout']
    qkv, dout = qkv.to(dev), dout.to(dev)
    cu = (case['cu'] if cu is None else cu).to(dev)
    slopes = case['slopes'].to(dev)
    hdp = ops.attn_head_pad(hd)
    if hdp != hd:
        qkv, dout = _pad(ops, qkv, hdp), _pad(ops, dout, hdp)
        assert (_bits(qkv[..., hd:]) == 0).all() and (_bits(dout[..., hd:]) == 0).all(), 'pad tail is not +0'
    S, max_seqlen = cu.numel() - 1, max(case['lens']) if max_seqlen is None else max_seqlen
    out, lse, dqkv = _nan_like((T, 1, H, hdp), torch.bfloat16), _nan_like((H, T), torch.float32), _nan_like((T, 3, H, hdp), torch.bfloat16)
    ws_f = ops._ws(lib().resel_attn_varlen_fwd_workspace_bytes(S, max_seqlen), dev)
    ws_b = ops._ws(lib().resel_attn_varlen_bwd_workspace_bytes(T, S, H, hdp, max_seqlen), dev)
    args = (T, S, H, hdp, max_seqlen, float(case['scale']), float(case['p_drop']), AP.SEED, AP.OFFSET, ops._stream())
    fwd, bwd = (lib().resel_attn_varlen_fwd_padded, lib().resel_attn_varlen_bwd_padded) if padded else (lib().resel_attn_varlen_fwd, lib().resel_attn_varlen_bwd)
    check(fwd(_ptr(qkv), _ptr(cu), _ptr(slopes), _ptr(out), _ptr(lse), _ptr(ws_f), *args), 'attn fwd')
    check(bwd(_ptr(qkv), _ptr(cu), _ptr(slopes), _ptr(out), _ptr(lse), _ptr(dout), _ptr(dqkv), _ptr(ws_b), *args), 'attn bwd')
    torch.cuda.synchronize()
    if hdp != hd:
        assert (_bits(out[:n, ..., hd:]) == 0).all() and (_bits(dqkv[:n, ..., hd:]) == 0).all(), 'zero columns in, zero columns out'
        out, dqkv = _unpad(ops, out, hd), _unpad(ops, dqkv, hd)
    return out[:, 0], lse, dqkv


# ------------------------------------------------------------------------------------------------------------- training core
@pytest.mark.parametrize('name', list(HD.CASES))
def test_attention_core_holds_every_head_and_block_to_fp64(ops, name):
    case, ref = _case_and_ref(name)
    out, lse, dqkv = _run_core(ops, case)
    got = dict(out=out, lse2=lse, dq=dqkv[:, 0], dk=dqkv[:, 1], dv=dqkv[:, 2])
    fr = AP.fractions(case, got, ref)
    for nm, f in fr.items():
        print(f'ATTN-FIG {name} {nm} {f:.4f}')
    assert all(f <= 1.0 for f in fr.values()), fr            # a non-finite result gives inf

    # the autograd wrapper chooses the kernel width, pads and unpads by itself and runs the same kernels on the same operands
    dev = out.device
    x = case['qkv'].to(dev).requires_grad_(True)
    o2 = ops.attn_varlen(x, case['cu'].to(dev), max(case['lens']), case['slopes'].to(dev), case['scale'], case['p_drop'], AP.SEED, AP.OFFSET)
    o2.backward(case['dout'].to(dev))
    assert o2.shape == out.shape and x.grad.shape == dqkv.shape
    assert torch.equal(_bits(o2.detach()), _bits(out)), 'ops.attn_varlen: out differs from the C entry'
    assert torch.equal(_bits(x.grad), _bits(dqkv)), 'ops.attn_varlen: dqkv differs from the C entry'
    if name == 'ragged16':                                   # the default scale is that of the width the caller passes
        o3 = ops.attn_varlen(case['qkv'].to(dev), case['cu'].to(dev), max(case['lens']), case['slopes'].to(dev))
        assert torch.equal(_bits(o3), _bits(out))


def test_padded_table_form_at_hd_128(ops):
    """`_padded` entries at hd = 128: T above cu[-1], one empty sequence in the table, a grid sized by a bucket's max_seqlen.  The real
    rows hold the bounds (and are the unpadded entries' bits), the token tail comes back as +0."""
    case, ref = _case_and_ref('drop128')
    n, lens = case['qkv'].shape[0], case['lens']
    cu_np = np.concatenate(([0], np.cumsum([lens[0], 0, lens[1]])))
    cu = torch.tensor(np.concatenate((cu_np, np.full(9 - cu_np.size, n))), dtype=torch.int32)       # 8 sequences: one empty inside, 5 behind
    plain = _run_core(ops, case)
    got = _run_core(ops, case, cu=cu, T=n + 70, padded=True, max_seqlen=512)
    out, lse, dqkv = got
    fr = AP.fractions(case, dict(out=out[:n], lse2=lse[:, :n], dq=dqkv[:n, 0], dk=dqkv[:n, 1], dv=dqkv[:n, 2]), ref)
    for nm, f in fr.items():
        print(f'ATTN-FIG drop128-padded {nm} {f:.4f}')
    assert all(f <= 1.0 for f in fr.values()), fr
    for nm, g, r, tok_dim in zip(('out', 'lse', 'dqkv'), got, plain, (0, 1, 0)):
        assert torch.equal(_bits(g.narrow(tok_dim, 0, n)), _bits(r)), nm
        assert (_bits(g.narrow(tok_dim, n, 70)) == 0).all(), nm           # +0.0, not the NaN the buffer held
    # and through the wrapper
    dev = out.device
    x = torch.zeros(n + 70, 3, case['H'], case['hd'], dtype=torch.bfloat16)
    x[:n] = case['qkv']
    x = x.to(dev).requires_grad_(True)
    dout = torch.zeros(n + 70, case['H'], case['hd'], dtype=torch.bfloat16)
    dout[:n] = case['dout']
    o2 = ops.attn_varlen(x, cu.to(dev), 512, case['slopes'].to(dev), case['scale'], case['p_drop'], AP.SEED, AP.OFFSET, padded=True)
    o2.backward(dout.to(dev))
    assert torch.equal(_bits(o2.detach()), _bits(out)) and torch.equal(_bits(x.grad), _bits(dqkv))


# -------------------------------------------------------------------------------------------------------------------- decode
S_CACHE, N_STEPS = 160, 136                                 # the steps cross position 128 (a second pass of the 256 threads over the keys: none;
ROWS_POS = (0, 37, 130)                                     # 128 is where a block of the training kernels ends)


@functools.lru_cache(maxsize=None)
def _decode_data(H, hd):
    """Three rows of S_CACHE tokens, qkv [3 * S, 3, H, hd] bf16 (0.8 randn), and the fp64 attention output of every token: the decode
    step at position p of a row is the last-query row of causal attention over its first p + 1 tokens."""
    g = torch.Generator().manual_seed(7100 + H * hd)
    qkv = (0.8 * torch.randn(3 * S_CACHE, 3, H, hd, generator=g)).to(torch.bfloat16)
    cu = torch.tensor([0, S_CACHE, 2 * S_CACHE, 3 * S_CACHE], dtype=torch.int32)
    ref = AP.attn_model(qkv, torch.zeros(3 * S_CACHE, H, hd, dtype=torch.bfloat16), cu, K.alibi_slopes(H), hd ** -0.5)['out']
    return qkv.view(3, S_CACHE, 3, H, hd), ref.view(3, S_CACHE, H, hd)


@pytest.mark.parametrize('hd', [128, 16])
def test_decode_steps_and_rows_hold_every_position_and_head_to_fp64(ops, hd):
    H = 2
    qkv, ref = _decode_data(H, hd)
    hdp = ops.attn_head_pad(hd)
    sl, scale = K.alibi_slopes(H).cuda(), hd ** -0.5
    x = qkv.cuda()
    outs = {}
    for source in ('host', 'device'):                       # B = 1, stepped from an empty cache
        cache = torch.zeros(1, S_CACHE, 2, H, hdp, dtype=torch.bfloat16, device='cuda')
        where = torch.zeros(1, dtype=torch.int32, device='cuda')
        got = []
        for pos in range(N_STEPS):
            got.append(ops.attn_decode(x[0:1, pos].contiguous(), cache, pos if source == 'host' else where, sl, scale)[0])
            where += 1
        outs[source] = torch.stack(got)                     # [P, H, hd]
        f = AP.decode_fraction(outs[source], ref[0, :N_STEPS])
        print(f'ATTN-FIG decode-{H}x{hd} steps=0..{N_STEPS - 1}({source}) {f:.4f}')
        assert outs[source].shape == (N_STEPS, H, hd) and f <= 1.0, (source, f)
        # the cache holds the fed k, v in its first hd columns, zeros behind, and nothing beyond the last step
        assert torch.equal(_bits(cache[0, :N_STEPS, ..., :hd]), _bits(x[0, :N_STEPS, 1:]))
        assert (_bits(cache[0, :N_STEPS, ..., hd:]) == 0).all() and (_bits(cache[0, N_STEPS:]) == 0).all()
    assert torch.equal(_bits(outs['host']), _bits(outs['device'])), 'host position and device counter disagree'

    # one call, three rows at three positions; what lies beyond a row's position, and the row not in use, is NaN
    B = len(ROWS_POS)
    cache = _nan_like((B + 1, S_CACHE, 2, H, hdp), torch.bfloat16)
    for b, p in enumerate(ROWS_POS):
        cache[b, :p] = 0
        cache[b, :p, ..., :hd] = x[b, :p, 1:]
    before = cache.clone()
    pos_rows = torch.tensor(ROWS_POS, dtype=torch.int32, device='cuda')
    step = torch.stack([x[b, p] for b, p in enumerate(ROWS_POS)]).contiguous()                      # [B, 3, H, hd]
    out = ops.attn_decode(step, cache, pos_rows, sl, scale)
    want = torch.stack([ref[b, p] for b, p in enumerate(ROWS_POS)])
    f = AP.decode_fraction(out, want)
    print(f'ATTN-FIG decode-{H}x{hd} rows={",".join(map(str, ROWS_POS))} {f:.4f}')
    assert out.shape == (B, H, hd) and f <= 1.0
    for b, p in enumerate(ROWS_POS):
        before[b, p] = 0
        before[b, p, ..., :hd] = x[b, p, 1:]
    assert torch.equal(_bits(cache), _bits(before)), 'the cache differs from (before the call + the appended k, v)'


# ------------------------------------------------------------------------------------------------------------ padding kernels
@pytest.mark.parametrize('T', [1, 1027])
@pytest.mark.parametrize('hd', [8, 24, 120])
def test_head_pad_then_unpad_is_the_identity_and_the_tail_is_zero(ops, hd, T):
    hdp = ops.attn_head_pad(hd)
    g = torch.Generator().manual_seed(hd * 10000 + T)
    for n, H in ((3, 3), (1, 2)):                            # qkv / dqkv and dout / out
        x = torch.randn(T, n, H, hd, generator=g).to(torch.bfloat16).cuda()
        wide = _pad(ops, x, hdp)
        assert torch.equal(_bits(wide[..., :hd]), _bits(x)) and (_bits(wide[..., hd:]) == 0).all()
        assert torch.equal(_bits(_unpad(ops, wide, hd)), _bits(x))
        assert torch.equal(_bits(ops._head_unpad(ops._head_pad(x, hdp), hd)), _bits(x))


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('hd', [12, 136, 256])
def test_other_head_widths_raise_a_value_error_that_names_the_accepted_set(ops, hd):
    H, T = 2, 40
    qkv = torch.zeros(T, 3, H, hd, dtype=torch.bfloat16, device='cuda')
    cu = torch.tensor([0, T], dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='multiples of 8 from 8 to 128') as e:
        ops.attn_varlen(qkv, cu, T)
    assert '136 to 256' in str(e.value)
    cache = torch.zeros(1, 8, 2, H, hd, dtype=torch.bfloat16, device='cuda')
    with pytest.raises(ValueError, match='multiples of 8 from 8 to 128'):
        ops.attn_decode(qkv[:1].contiguous(), cache, 0, None, 1.0)
