"""Bucketed sequence tables of attention layers on the GPU (`seq_buckets`; buffers/transition_buffer/shape_buckets.py `pad_seq_tables`):
the pack / unpack kernels that take the real token count from device memory, the padded forms of the attention core against the
unpadded entries, one padded cgpt update against the unpadded one, replays of bucketed cgpt updates against the eager update on the
same shapes, how many updates of the ragged workload replay, and the 'auto' switch.
Workload and helpers: tests/test_shape_buckets.py, tests/test_graph_buckets_gpu.py (24 trajectories of 3..40 steps, batches of 95
transitions, actor noise off).  Bounds of the update tests: those of tests/test_trainer_gpu.py
`test_graphed_update_equals_the_eager_update` for cgpt (parameters rtol 5e-3 / atol 3e-4, logged scalars max(rtol, 100 atol) of
max(1, |value|)) - the attention runs in bf16, an operand that differs in its last fp32 bit can round to the next bf16 value."""
import ctypes

import numpy as np
import pytest
import torch

from test_graph_buckets_gpu import _key_len, _state, _trainer, _value, no_noise  # noqa: F401  (no_noise: fixture)
from test_host_logic import _push, _synth, make_parameter

CGPT = 'cgpt_h1_l2_p0.0_ml64_rms'
RTOL, ATOL = 5e-3, 3e-4


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda')


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------------- 1. pack / unpack
def _pack_case(C, T, n, dev, gen):
    M = T + 7
    idx = torch.sort(torch.randperm(M, generator=gen)[:T]).values.to(dev)      # strictly increasing rows of [0, M)
    n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
    src = torch.randn(M, C, generator=gen).to(dev)
    packed = torch.randn(T, C, generator=gen).to(dev)
    return M, idx, n_dev, src, packed


def _pack_ref(src, idx, n, T):
    ref = torch.zeros(T, src.shape[1], device=src.device)
    ref[:n] = src.index_select(0, idx[:n])
    return ref


def _unpack_ref(packed, idx, n, M):
    return torch.zeros(M, packed.shape[1], device=packed.device).index_copy(0, idx[:n], packed[:n])


CASES = [(T, n) for T in (1, 130) for n in sorted({0, 1, T - 1, T})]


@pytest.mark.gpu
@pytest.mark.parametrize('C', [4, 36, 256])
def test_pack_and_unpack_equal_index_select_and_index_copy(C):
    dev = _gpu()
    from offpolicy_rnn.hip import ops
    from offpolicy_rnn.hip._lib import check, lib
    gen = torch.Generator().manual_seed(C)
    for T, n in CASES:
        M, idx, n_dev, src, packed = _pack_case(C, T, n, dev, gen)
        out = torch.full((T, C), float('nan'), device=dev)
        check(lib().resel_pack_rows(_ptr(src), C, _ptr(idx), _ptr(n_dev), _ptr(out), C, T, C, ops._stream()), 'pack_rows')
        assert torch.equal(out, _pack_ref(src, idx, n, T)), (C, T, n)
        assert (out[n:] == 0).all() and torch.isfinite(out).all(), (C, T, n)
        dst = torch.full((M, C), float('nan'), device=dev)
        check(lib().resel_unpack_rows(_ptr(packed), C, _ptr(idx), _ptr(n_dev), _ptr(dst), C, M, T, C, ops._stream()), 'unpack_rows')
        assert torch.isfinite(dst).all(), (C, T, n)                              # every row was written
        assert torch.equal(dst, _unpack_ref(packed, idx, n, M)), (C, T, n)
        # rows inside wider buffers (leading dimension > C): the slack columns stay untouched
        wide_src = torch.randn(M, C + 8, device=dev)
        wide_out = torch.full((T, C + 4), float('nan'), device=dev)
        check(lib().resel_pack_rows(_ptr(wide_src), C + 8, _ptr(idx), _ptr(n_dev), _ptr(wide_out), C + 4, T, C, ops._stream()), 'pack_rows')
        assert torch.equal(wide_out[:, :C], _pack_ref(wide_src[:, :C], idx, n, T)) and torch.isnan(wide_out[:, C:]).all(), (C, T, n)
    # a count beyond the table is clamped to its length (never an access behind it)
    M, idx, n_dev, src, packed = _pack_case(C, 130, 130, dev, gen)
    big = torch.tensor([10 ** 6], dtype=torch.int32, device=dev)
    assert torch.equal(ops.pack_tokens(src, idx, big), _pack_ref(src, idx, 130, 130))
    assert torch.equal(ops.unpack_tokens(packed, idx, big, M), _unpack_ref(packed, idx, 130, M))


@pytest.mark.gpu
@pytest.mark.parametrize('C', [4, 36, 256])
def test_pack_and_unpack_are_each_other_s_gradient(C):
    dev = _gpu()
    from offpolicy_rnn.hip import ops
    gen = torch.Generator().manual_seed(100 + C)
    for T, n in CASES:
        M, idx, n_dev, src, packed = _pack_case(C, T, n, dev, gen)
        g_t, g_m = torch.randn(T, C, generator=gen).to(dev), torch.randn(M, C, generator=gen).to(dev)
        x = src.clone().requires_grad_(True)
        y = ops.pack_tokens(x, idx, n_dev)
        assert torch.equal(y, _pack_ref(src, idx, n, T))
        y.backward(g_t)
        assert torch.equal(x.grad, _unpack_ref(g_t, idx, n, M)), (C, T, n)     # a padded token sends no gradient anywhere
        p = packed.clone().requires_grad_(True)
        z = ops.unpack_tokens(p, idx, n_dev, M)
        assert torch.equal(z, _unpack_ref(packed, idx, n, M))
        z.backward(g_m)
        assert torch.equal(p.grad, _pack_ref(g_m, idx, n, T)) and (p.grad[n:] == 0).all(), (C, T, n)


# ------------------------------------------------------------------------------------------- 2. padded attention == unpadded
def _nan_like(shape, dtype, dev):
    return torch.full(shape, float('nan'), dtype=dtype, device=dev)


def _attn_run(lib_fwd, lib_bwd, qkv, dout, cu, slopes, max_seqlen, p_drop):
    """Forward and backward through the C entries into NaN-filled buffers; (out, lse, dqkv)."""
    from offpolicy_rnn.hip import ops
    from offpolicy_rnn.hip._lib import check, lib
    T, _, H, hd = qkv.shape
    S = cu.numel() - 1
    dev = qkv.device
    out, lse, dqkv = _nan_like((T, H, hd), torch.bfloat16, dev), _nan_like((H, T), torch.float32, dev), _nan_like(tuple(qkv.shape), torch.bfloat16, dev)
    ws_f = ops._ws(lib().resel_attn_varlen_fwd_workspace_bytes(S, max_seqlen), dev)
    ws_b = ops._ws(lib().resel_attn_varlen_bwd_workspace_bytes(T, S, H, hd, max_seqlen), dev)
    scale, seed, offset = hd ** -0.5, 1234, 8
    check(lib_fwd(_ptr(qkv), _ptr(cu), _ptr(slopes), _ptr(out), _ptr(lse), _ptr(ws_f), T, S, H, hd, max_seqlen, scale, p_drop, seed, offset,
                  ops._stream()), 'attn fwd')
    check(lib_bwd(_ptr(qkv), _ptr(cu), _ptr(slopes), _ptr(out), _ptr(lse), _ptr(dout), _ptr(dqkv), _ptr(ws_b), T, S, H, hd, max_seqlen, scale,
                  p_drop, seed, offset, ops._stream()), 'attn bwd')
    return out, lse, dqkv


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('p_drop', [0.0, 0.1])
def test_padded_attention_equals_the_unpadded_entries(hd, p_drop):
    dev = _gpu()
    from offpolicy_rnn.hip._lib import lib
    from offpolicy_rnn.models.flash_attention.TransformerFlashAttention import alibi_slopes
    H, lens = 2, [1, 130, 5, 257]
    n = sum(lens)
    gen = torch.Generator().manual_seed(hd)
    qkv = torch.randn(n + 200, 3, H, hd, generator=gen).to(dev).to(torch.bfloat16)
    dout = torch.randn(n + 200, H, hd, generator=gen).to(dev).to(torch.bfloat16)
    slopes = alibi_slopes(H).to(dev)
    cu = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int32, device=dev)
    ref = _attn_run(lib().resel_attn_varlen_fwd, lib().resel_attn_varlen_bwd, qkv[:n].contiguous(), dout[:n].contiguous(), cu, slopes, max(lens), p_drop)
    assert all(torch.isfinite(r.float()).all() for r in ref)
    for with_empty in (False, True):
        ls = lens[:2] + [0] + lens[2:] if with_empty else lens
        cu_np = np.concatenate(([0], np.cumsum(ls)))
        cu_p = torch.tensor(np.concatenate((cu_np, np.full(17 - cu_np.size, n))), dtype=torch.int32, device=dev)      # 16 sequences
        for pad in (0, 1, 200):
            T = n + pad
            got = _attn_run(lib().resel_attn_varlen_fwd_padded, lib().resel_attn_varlen_bwd_padded, qkv[:T].contiguous(), dout[:T].contiguous(),
                            cu_p, slopes, 512, p_drop)
            for nm, g, r, tok_dim in zip(('out', 'lse', 'dqkv'), got, ref, (0, 1, 0)):
                real, tail = g.narrow(tok_dim, 0, n), g.narrow(tok_dim, n, pad)
                assert torch.equal(_bits(real.contiguous()), _bits(r)), (nm, with_empty, pad)
                assert (_bits(tail.contiguous()) == 0).all(), (nm, with_empty, pad)    # +0.0, not the NaN the buffer held


# ---------------------------------------------------------------------------------------------------- update-level comparisons
def _compare(what, alg_a, alg_b, logs_a, logs_b):
    """Parameters as np.testing.assert_allclose(rtol, atol) would, logged scalars to max(rtol, 100 atol) of max(1, |value|) - the
    assertions of `test_graphed_update_equals_the_eager_update` for cgpt; every figure is printed before anything is asserted."""
    worst = []
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), _state(alg_a), _state(alg_b)):
        a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
        excess = (np.abs(a - b) - RTOL * np.abs(b)).max()
        print(f'MEASURED {what} {nm}: max |a - b| = {np.abs(a - b).max():.3e}, max (|a - b| - {RTOL:g} |b|) = {excess:.3e} (atol {ATOL:g})')
        worst.append((nm, excess))
    log_err = 0.0
    for la, lb in zip(logs_a, logs_b):
        assert set(la) == set(lb)
        for k in la:
            log_err = max(log_err, abs(_value(la[k]) - _value(lb[k])) / max(1.0, abs(_value(lb[k]))))
    bound = max(RTOL, 100 * ATOL)
    print(f'MEASURED {what} logged scalars: max |a - b| / max(1, |b|) = {log_err:.3e} (bound {bound:g})')
    for nm, e in worst:
        assert e <= ATOL, (what, nm, e)
    assert log_err <= bound, (what, log_err)


@pytest.mark.gpu
def test_the_padded_cgpt_update_equals_the_unpadded_one(no_noise):
    """One eager update on the same draw: batch and sequence tables padded into their buckets, and neither."""
    algs, logs = [], []
    for buckets in (True, False):
        alg = _trainer(CGPT, 'td3')
        alg.shape_buckets = alg.seq_buckets = buckets
        logs.append([dict(alg.train_one_batch())])
        algs.append((alg, alg.replay_buffer._last_batch_shape))
    (padded, shape_p), (exact, shape_e) = algs
    print(f'MEASURED cgpt td3: batch {shape_e} padded to {shape_p}')
    assert shape_p[0] >= shape_e[0] and shape_p[1] > shape_e[1]
    for k in ('real_batch_size', 'real_batch_traj_num'):
        assert logs[0][0][k] == logs[1][0][k], k
    _compare('cgpt td3 padded vs unpadded', padded, exact, logs[0], logs[1])


@pytest.mark.gpu
def test_bucketed_cgpt_replays_equal_the_eager_updates_on_the_same_shapes(no_noise):
    """8 updates of the ragged workload: an eager trainer that pads batch and sequence tables into their buckets against
    `GraphedUpdate(buckets='on', seq_buckets=True)` - the chain length the bounds were established for."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    eager = _trainer(CGPT, 'td3')
    eager.shape_buckets = eager.seq_buckets = True
    logs_e = []
    for _ in range(8):
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    graphed = _trainer(CGPT, 'td3')
    g = GraphedUpdate(graphed, warmup=1, buckets='on', seq_buckets=True)
    try:
        logs_g = []
        for _ in range(8):
            logs_g.append(dict(g.step()))
            graphed.grad_num += 1
        torch.cuda.synchronize()
        print(f'MEASURED cgpt td3: graphs {sorted(g.graphs)}, eager updates {g.eager_fallbacks} of 8')
        assert len(g.graphs) >= 1 and g.eager_fallbacks < 8, 'nothing was replayed'
        _compare('cgpt td3 replay vs eager', graphed, eager, logs_g, logs_e)
    finally:
        g.close()


@pytest.mark.gpu
def test_ragged_cgpt_updates_replay(no_noise, monkeypatch):
    """24 updates of the ragged workload: exact keys would replay next to nothing (24 distinct keys in 24 plans); bucketed, all but
    the warm-up and the first visit of each shape are replays."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    monkeypatch.delenv('RESEL_GRAPH_SEQ_BUCKETS', raising=False)
    alg = _trainer(CGPT, 'td3')
    with pytest.raises(RuntimeError, match='sequence tables'):                  # `seq_buckets` left at its default (the variable is unset)
        GraphedUpdate(alg, warmup=1, buckets='on')
    g = GraphedUpdate(alg, warmup=1, buckets='on', seq_buckets=True)
    try:
        for _ in range(24):
            log = dict(g.step())
            alg.grad_num += 1
            for k, v in log.items():
                if 'loss' in k:
                    assert np.isfinite(_value(v)), (k, v)
        torch.cuda.synchronize()
        print(f'MEASURED cgpt td3: graphs {len(g.graphs)} {sorted(g.graphs)}, eager updates {g.eager_fallbacks} of 24')
        assert len(g.graphs) >= 1 and all(len(k) == _key_len(g, True) for k in g.graphs)
        assert g.eager_fallbacks <= 6
    finally:
        g.close()


@pytest.mark.gpu
def test_auto_mode_switches_with_sequence_buckets(no_noise):
    """The eight-trajectory workload of tests/test_graph_buckets_gpu.py `test_auto_mode_stays_exact_with_sequence_tables`, room for one
    graph: with `seq_buckets` the second distinct shape switches 'auto' to 'on' and the keys become the bucketed ones."""
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter(CGPT, algo='td3', sac_batch_size=23, cuda_inference=True))
    rs = np.random.RandomState(3)
    for n in (12, 9, 7, 12, 5, 12, 10, 8):
        o, a, r = _synth(rs, n, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=(n != 12))
    np.random.seed(11)
    g = GraphedUpdate(alg, warmup=1, buckets='auto', max_graphs=1, seq_buckets=True)
    try:
        assert g.buckets == 'auto'
        switched_at = None
        for i in range(6):
            log = dict(g.step())
            alg.grad_num += 1
            assert np.isfinite(_value(log['critic_loss']))
            if switched_at is None and g.buckets == 'on':
                switched_at = i + 1
        torch.cuda.synchronize()
        print(f'MEASURED cgpt auto with seq_buckets: switched at update {switched_at}, keys {sorted(g._seen)}')
        assert switched_at is not None and switched_at <= 4
        assert g.max_graphs == 1 and all(len(k) == _key_len(g, True) for k in g._seen)
    finally:
        g.close()
