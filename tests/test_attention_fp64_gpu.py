"""The cgpt attention core (csrc/attention.hip: forward, dQ, dK/dV) and the KV-cache decode step (csrc/rollout_step.hip) against fp64,
each (head, 128-token block of position in sequence) slice held to its OWN scale - tests/attention_parity.py has the model, the
metric, the bounds and the case table; tests/test_attention_parity_host.py shows on the CPU that a correct bf16 pipeline uses at most
half of each bound and that a kernel which loses one 32-key score tile for the late queries exceeds them several times over (while it
passes the whole-tensor bounds of tests/test_hip_ops.py).  New here besides the metric: `lse` against a reference, dq / dk / dv each
on its own, a non-default `scale`, `slopes = None` at 513 tokens, decode at block edges deep in the cache without an absolute floor.

Every comparison prints `ATTN-FIG <case> <name> <fraction of bound>` before it asserts (`pytest -s`); the fractions measured on an
MI355X are in profiles/r27_attention_fp64_tests.md.  No bound here was fitted to them."""
import ctypes
import functools

import pytest
import torch

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


def _nan_like(shape, dtype, dev):
    return torch.full(shape, float('nan'), dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case_and_ref(name):
    case = AP.make_case(name)
    return case, AP.model_of(case)


def _run_core(ops, case):
    """Forward and backward through the C entries into NaN-filled buffers (as `_attn_run` of tests/test_seq_buckets_gpu.py, with the
    case's scale) -> (out [T, H, hd] bf16, lse [H, T] fp32, dqkv [T, 3, H, hd] bf16) on the device."""
    from offpolicy_rnn.hip._lib import check, lib
    dev = torch.device('cuda')
    qkv, dout, cu = case['qkv'].to(dev), case['dout'].to(dev), case['cu'].to(dev)
    slopes = None if case['slopes'] is None else case['slopes'].to(dev)
    T, _, H, hd = qkv.shape
    S, max_seqlen = cu.numel() - 1, max(case['lens'])
    out, lse, dqkv = _nan_like((T, H, hd), torch.bfloat16, dev), _nan_like((H, T), torch.float32, dev), _nan_like(tuple(qkv.shape), torch.bfloat16, dev)
    ws_f = ops._ws(lib().resel_attn_varlen_fwd_workspace_bytes(S, max_seqlen), dev)
    ws_b = ops._ws(lib().resel_attn_varlen_bwd_workspace_bytes(T, S, H, hd, max_seqlen), dev)
    args = (T, S, H, hd, max_seqlen, float(case['scale']), float(case['p_drop']), AP.SEED, AP.OFFSET, ops._stream())
    check(lib().resel_attn_varlen_fwd(_ptr(qkv), _ptr(cu), _ptr(slopes), _ptr(out), _ptr(lse), _ptr(ws_f), *args), 'attn fwd')
    check(lib().resel_attn_varlen_bwd(_ptr(qkv), _ptr(cu), _ptr(slopes), _ptr(out), _ptr(lse), _ptr(dout), _ptr(dqkv), _ptr(ws_b), *args), 'attn bwd')
    torch.cuda.synchronize()
    return out, lse, dqkv


# ------------------------------------------------------------------------------------------------------------- training core
@pytest.mark.parametrize('name', list(AP.CASES))
def test_attention_core_holds_every_head_and_block_to_fp64(ops, name):
    case, ref = _case_and_ref(name)
    out, lse, dqkv = _run_core(ops, case)
    got = dict(out=out, lse2=lse, dq=dqkv[:, 0], dk=dqkv[:, 1], dv=dqkv[:, 2])
    fr = AP.fractions(case, got, ref)
    for nm, f in fr.items():
        gran = f'@{AP.grad_granularity(name)}' if name == 'peaked' and nm in ('dq', 'dk', 'dv') else ''
        print(f'ATTN-FIG {name} {nm}{gran} {f:.4f}')
    if name == 'peaked':                                    # measured only: the granularities the assertion does not use
        for gran in AP.GRANULARITIES:
            for nm in ('dq', 'dk', 'dv'):
                print(f'ATTN-FIG {name} {nm}@{gran}(not-asserted) {AP.sliced_fraction(got[nm], ref[nm], case["pos"], AP.GRAD_TOL, gran):.4f}')
    assert all(f <= 1.0 for f in fr.values()), fr

    if name == 'ragged32':                                  # the autograd wrapper runs the same kernels on the same operands
        dev = out.device
        x = case['qkv'].to(dev).requires_grad_(True)
        slopes = case['slopes'].to(dev)
        o2 = ops.attn_varlen(x, case['cu'].to(dev), max(case['lens']), slopes, case['scale'])
        o2.backward(case['dout'].to(dev))
        assert torch.equal(_bits(o2.detach()), _bits(out)), 'ops.attn_varlen: out differs from the C entry'
        assert torch.equal(_bits(x.grad), _bits(dqkv)), 'ops.attn_varlen: dqkv differs from the C entry'


# -------------------------------------------------------------------------------------------------------------------- decode
S_CACHE = 704
DECODE_POS = (0, 31, 32, 127, 128, 129, 383, 640)
ROWS_POS = (640, 0, 129)                                    # one `decode_rows` call, three rows at three positions of DECODE_POS


@functools.lru_cache(maxsize=None)
def _decode_data(H, hd):
    """q [B, P, H, hd] (one query per row and tested position), kv [B, S, 2, H, hd]: 0.8 randn rounded to bf16."""
    g = torch.Generator().manual_seed(7000 + H * hd)
    B = 3
    q = (0.8 * torch.randn(B, S_CACHE, H, hd, generator=g)).to(torch.bfloat16)
    kv = (0.8 * torch.randn(B, S_CACHE, 2, H, hd, generator=g)).to(torch.bfloat16)
    return q, kv


def _decode_ref(q, kv, b, pos, slopes, scale):
    """fp64 `attn_decode_ref` of row b at position pos -> [H, hd]."""
    return K.attn_decode_ref(q[b:b + 1, pos].double(), kv[b:b + 1, :, 0].double(), kv[b:b + 1, :, 1].double(), pos, slopes, scale)[0]


def _cache_with(kv, positions, Bmax):
    """bf16 cache [Bmax, S, 2, H, hd] on the device: row b holds kv[b, :positions[b]], everything else NaN (a key read from beyond
    the row's position, or from a row not in use, poisons the output)."""
    cache = _nan_like((Bmax,) + tuple(kv.shape[1:]), torch.bfloat16, 'cuda')
    for b, p in enumerate(positions):
        cache[b, :p] = kv[b, :p].cuda()
    return cache


def _check_cache(cache, before, kv, positions, what):
    """Row b's slot `positions[b]` holds exactly the k, v that were fed; every other element has the bits it had before the call."""
    expect = before.clone()
    for b, p in enumerate(positions):
        expect[b, p] = kv[b, p].cuda()
    assert torch.equal(_bits(cache), _bits(expect)), f'{what}: the cache differs from (before the call + the appended k, v)'


@pytest.mark.parametrize('H,hd', [(8, 32), (4, 64)])
def test_decode_holds_every_position_and_head_to_fp64(ops, H, hd):
    q, kv = _decode_data(H, hd)
    slopes, scale = K.alibi_slopes(H), hd ** -0.5
    sl = slopes.cuda()
    B, case = 2, f'decode-{H}x{hd}'
    worst = []
    for pos in DECODE_POS:
        ref = torch.stack([_decode_ref(q, kv, b, pos, slopes, scale) for b in range(B)])                     # [B, H, hd]
        qkv = torch.stack((q[:B, pos], kv[:B, pos, 0], kv[:B, pos, 1]), dim=1).contiguous().cuda()            # [B, 3, H, hd]
        outs = []
        for source in ('host', 'device'):
            cache = _cache_with(kv, [pos] * B, B + 1)
            before = cache.clone()
            where = pos if source == 'host' else torch.full((1,), pos, dtype=torch.int32, device='cuda')
            outs.append(ops.attn_decode(qkv, cache, where, sl, scale))
            _check_cache(cache, before, kv, [pos] * B, f'{case} pos {pos} ({source} position)')
            f = AP.decode_fraction(outs[-1], ref)
            print(f'ATTN-FIG {case} pos={pos}({source}) {f:.4f}')
            worst.append((f, pos, source))
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), f'pos {pos}: host position and device counter disagree'
    assert max(worst)[0] <= 1.0, max(worst)

    # one call, three rows at three different positions
    from offpolicy_rnn.hip._lib import check, lib
    B = len(ROWS_POS)
    ref = torch.stack([_decode_ref(q, kv, b, p, slopes, scale) for b, p in enumerate(ROWS_POS)])
    qkv = torch.stack([torch.stack((q[b, p], kv[b, p, 0], kv[b, p, 1])) for b, p in enumerate(ROWS_POS)]).contiguous().cuda()
    cache = _cache_with(kv, ROWS_POS, B + 1)
    before = cache.clone()
    pos_rows = torch.tensor(ROWS_POS, dtype=torch.int32, device='cuda')
    out = _nan_like((B, H, hd), torch.bfloat16, 'cuda')
    check(lib().resel_attn_decode_rows(_ptr(qkv), 3 * H * hd, _ptr(cache), _ptr(pos_rows), _ptr(sl), _ptr(out), float(scale), B, H, hd,
                                       S_CACHE, ops._stream()), 'attn_decode_rows')
    torch.cuda.synchronize()
    _check_cache(cache, before, kv, ROWS_POS, f'{case} rows')
    f = AP.decode_fraction(out, ref)
    print(f'ATTN-FIG {case} rows={",".join(map(str, ROWS_POS))} {f:.4f}')
    assert f <= 1.0
    # and the wrapper's per-row form is that entry
    cache2 = _cache_with(kv, ROWS_POS, B + 1)
    assert torch.equal(_bits(ops.attn_decode(qkv, cache2, pos_rows, sl, scale)), _bits(out))
