"""What tests/test_gemm_fused_gpu.py rests on, checked without a GPU: the library's shape rules accept every case of its tables, its
fp64 references are well conditioned for the bound they are held to, its Y generator keeps its promises, and the two derived
summation bounds hold for a plain fp32 sum (and do not hold for a sum with one term missing)."""
import ctypes
import os

import pytest
import torch

import test_gemm_fused_gpu as G

NAMES = ('resel_gemm_f32_fused_supported', 'resel_gemm_f32_fused_workspace_bytes')


@pytest.fixture(scope='module')
def lib():
    from offpolicy_rnn.hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('library not built (run __graft_entry__.build())')
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


def test_case_tables_are_what_the_issue_lists():
    assert len(G.HEAD_CASES) == 11 and len(G.DACT_CASES) == 10 and len(set(G.HEAD_CASES)) == 11 and len(set(G.DACT_CASES)) == 10
    for sub, table in ((G.HEAD_NODE_CASES, G.HEAD_CASES), (G.DACT_DENSE_CASES, G.DACT_CASES), (G.DACT_NODBIAS_CASES, G.DACT_CASES), ([G.BIG], G.HEAD_CASES),
                       ([G.BIG], G.DACT_CASES)):
        assert set(sub) <= set(table)
    assert G.BIG[0] * G.BIG[1] * G.BIG[2] >= 1 << 20                      # the magnitude-slot threshold of `_gemm_run`
    tails = sorted(M % 256 for _, M, _, _ in G.DACT_CASES)
    assert tails == [0, 0, 0, 1, 8, 9, 20, 128, 129, 255]                   # rows form 1 .. 8, first edition .. 128, mode 2 from 129
    cases = G.mode2_cases()
    assert len(cases) == 40 and len(set(cases)) == 40
    for M, N, K, akc, bkc, _, _ in cases:
        assert M > 128 and K >= 32                                          # mode 2 (`gemm_route`), not the fp32 instruction
        assert (K if akc else M) % 4 == 0 and (K if bkc else N) % 4 == 0    # readable by the matrix-core editions (`gemm_mfma_readable`)
    assert {(akc, bkc) for _, _, _, akc, bkc, _, _ in cases} == {(a, b) for a in (True, False) for b in (True, False)}
    assert sum(K % 32 == 0 for _, _, K, *_ in cases) == 20                  # third edition / second edition, half each


def test_library_takes_every_case(lib):
    """A later change of the shape rules cannot quietly empty the GPU test: every head case is a kind-5 shape, every dact case a kind-4
    shape, in the dense and in the token-major leading dimensions, and both need a workspace."""
    for kind, table in ((5, G.HEAD_CASES), (4, G.DACT_CASES)):
        for batch, M, N, K in table:
            for ld in (max(N, K), batch * max(N, K) + 8):
                assert lib.resel_gemm_f32_fused_supported(kind, M, N, K, ld, ld) == 1, (kind, batch, M, N, K, ld)
            assert lib.resel_gemm_f32_fused_workspace_bytes(M, N, K, batch, kind) > 0
    assert lib.resel_gemm_f32_fused_supported(4, 255, 128, 32, 128, 128) == 0 and lib.resel_gemm_f32_fused_supported(4, 256, 132, 32, 132, 132) == 0
    assert lib.resel_gemm_f32_fused_supported(5, 128, 128, 32, 128, 128) == 0 and lib.resel_gemm_f32_fused_supported(5, 129, 4, 36, 36, 36) == 0


@pytest.mark.parametrize('batch,M,N,K', G.HEAD_CASES)
def test_head_reference_is_well_conditioned(batch, M, N, K):
    """The same formulas in fp32 on the CPU meet the GPU test's bound against the fp64 reference, and the row-dot bound holds for an fp32
    sum of the reference's terms - and fails once a term is left out."""
    c, (a64, q64) = G.head_case(batch, M, N, K)
    a32, q32 = G.head_reference(c['A'], c['B'], c['bias'], c['w3'], c['b3'], dtype=torch.float32)
    assert a32.dtype == torch.float32 and a64.dtype == torch.float64
    G.close(a32, a64, rtol=G.RTOL, atol_scale=G.ATOL_SCALE, name='a')
    G.close(q32, q64, rtol=G.RTOL, atol_scale=G.ATOL_SCALE, name='q')
    a = a64.float()
    q = (a * c['w3'].unsqueeze(-2)).sum(-1) + c['b3'].unsqueeze(-1)
    assert q.dtype == torch.float32 and G.rowdot_excess(q, a, c['w3'], c['b3']) <= 1.0
    assert G.rowdot_excess((a * c['w3'].unsqueeze(-2)).sum(-1), a, c['w3'], None) <= 1.0
    short = (a[..., 1:] * c['w3'][:, 1:].unsqueeze(-2)).sum(-1) + c['b3'].unsqueeze(-1)
    assert G.rowdot_excess(short, a, c['w3'], c['b3']) > 1.0


@pytest.mark.parametrize('batch,M,N,K', G.DACT_CASES)
def test_dact_reference_is_well_conditioned(batch, M, N, K):
    c, (o64, d64) = G.dact_case(batch, M, N, K)
    o32, d32 = G.dact_reference(c['A'], c['B'], c['Y'], dtype=torch.float32)
    assert o32.dtype == torch.float32 and o64.dtype == torch.float64
    G.close(o32, o64, rtol=G.RTOL, atol_scale=G.ATOL_SCALE, name='out')
    G.close(d32, d64, rtol=G.RTOL, atol_scale=G.ATOL_SCALE, name='dbias')
    o = o64.float()
    assert G.colsum_excess(o.sum(-2), o) <= 1.0
    seq = torch.zeros(batch, N)
    for m in range(M):                                   # one running fp32 sum per column, row by row: the order least like torch's
        seq += o[:, m]
    assert G.colsum_excess(seq, o) <= 1.0
    assert G.colsum_excess(seq - o[:, M - 1], o) > 1.0   # the last row missing
    assert G.colsum_excess(seq + o[:, 2], o) > 1.0       # a row counted twice


@pytest.mark.parametrize('batch,M,N,K', G.DACT_CASES)
def test_y_generator_invariants(batch, M, N, K):
    """Y is an ELU output (> -1) with row 0 exactly -1 and row 1 exactly 0, and every 32 x 32 block (partial ones at the end of the rows
    included) holds both signs: each block's derivative factors mix 1 and y + 1."""
    Y = G.dact_case(batch, M, N, K)[0]['Y']
    assert Y.shape == (batch, M, N) and Y.dtype == torch.float32
    assert (Y[:, 0] == -1.0).all() and (Y[:, 1] == 0.0).all() and (Y[:, 2:] > -1.0).all()
    for m0 in range(0, M, 32):
        blk = Y[:, m0:m0 + 32].unflatten(-1, (N // 32, 32))                  # [batch, rows, blocks, 32]
        assert (blk > 0).any(-1).any(1).all() and (blk < 0).any(-1).any(1).all(), f'a 32 x 32 block of rows {m0} .. has one sign only'
