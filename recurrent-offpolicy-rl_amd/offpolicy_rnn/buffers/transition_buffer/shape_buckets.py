"""Shape buckets of the packed batch (new design; the reference trims every batch to the longest row it drew, nested_replay_memory.py).

A recorded update graph (algorithm/graphed_update.py) is valid for one batch shape, and with early-terminating episodes the exact
shape - rows, row length, plan segments - hardly ever recurs.  Rounding each of the three UP to a coarse ladder makes a handful of
shapes cover every batch.  The extra slots are what the sampler writes behind a short row anyway (`mask = 0, start = 1`), the extra
plan entries carry row -1 and are dropped by the gather kernel, the losses divide by the sum of the mask: the padded update computes
what the exact one does, at up to 1.5x the tokens in the worst case.

Attention layers (cgpt) also take two SEQUENCE tables per batch - the packed token indices and cu_seqlens of the batch and of its
one-slot shift - whose sizes vary with the draw even inside one batch bucket.  `pad_seq_tables` moves both into ONE more bucket
(token count up the ladder, number of sequences up to a power of two) that is a function of what the batch bucket already bounds,
so in practice the graph key gains no value of its own: the extra sequences are empty (cu_seqlens repeats its last value - which
is the real token count, readable by the kernels on the device), the extra token slots are never read.

Host arithmetic only: no torch in here (the planner runs while the previous update is still on the GPU)."""
import numpy as np

MIN_ROW_LEN = 32                                      # shorter rows are not worth a shape of their own
MIN_NSEG = 16
MIN_TOKENS = 256                                      # token tables shorter than this are not worth a shape of their own
MIN_SEQS = 16
ATTN_BLOCK = 128                                      # tokens per attention workgroup: the longest-sequence bound is a multiple of it

NO_SEQ_BUCKETS = 'shape buckets do not cover layers that need sequence tables (cgpt): the token and cu_seqlens tables vary with the batch ' \
                 'and are bucketed only with seq_buckets (RESEL_GRAPH_SEQ_BUCKETS=1)'


def ladder(x):
    """Smallest member of {2^k, 3 * 2^(k-1)} that is >= x: 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, ... (at most 1.5x growth)."""
    x = int(x)
    if x <= 1:
        return 1
    p = 1 << (x - 1).bit_length()                     # next power of two >= x
    t = 3 * p // 4
    return t if p >= 4 and t >= x else p


def bucket_shape(nrow, longest, nseg, row_cap):
    """(rows, row_len, nseg) of the bucket that holds a batch of `nrow` rows, longest row `longest` (the +1 slot included) and `nseg`
    plan segments.  `row_cap` is the buffer's `max_traj_step`: row_cap + 1 is the longest row the planner can emit, so a full row is
    never padded."""
    row_len = min(max(ladder(longest), MIN_ROW_LEN), int(row_cap) + 1)
    return ladder(nrow), row_len, max(MIN_NSEG, 1 << max(int(nseg) - 1, 0).bit_length())


def pad_plan(pl, row_cap):
    """The plan of `plan_trajs_device` moved into its bucket: same sampled trajectories at the same slots; `seg` padded with (-1, 0, 0, 0)
    (dropped by the gather kernel), `table` with a row [1, 0, ...] per empty row (the leading dummy sequence every row has);
    `nrow` / `longest` / `max_len` become the bucket's (`max_len` only sizes the gather grid), the drawn values stay in `nrow_real` /
    `longest_real`.  A plan with a selection of loss positions (`sel` = [one word offset per entry | bitmap words], offsets relative to
    the words part): the offset header is padded with zeros to the bucketed entry count, the words follow unchanged."""
    seg, table = pl['seg'], pl['table']
    rows, row_len, nseg = bucket_shape(pl['nrow'], pl['longest'], seg.shape[0], row_cap)
    # the gather kernel drops what does not fit its output: a row longer than the planner may emit must be an error here, not lost data
    assert row_len >= pl['longest'] and row_len >= pl['max_len'], (row_len, pl['longest'], pl['max_len'], row_cap)
    seg_b = np.zeros((nseg, 4), dtype=seg.dtype)
    seg_b[:seg.shape[0]] = seg
    seg_b[seg.shape[0]:, 0] = -1
    table_b = np.zeros((rows, table.shape[1]), dtype=table.dtype)
    table_b[:table.shape[0]] = table
    table_b[table.shape[0]:, 0] = 1
    out = dict(pl, seg=seg_b, table=table_b, nrow=rows, longest=row_len, max_len=row_len, nrow_real=pl['nrow'], longest_real=pl['longest'])
    if 'sel' in pl:
        sel, n = pl['sel'], seg.shape[0]
        out['sel'] = np.concatenate((sel[:n], np.zeros(nseg - n, dtype=sel.dtype), sel[n:]))
    return out


def pad_seq_tables(built, rows, row_len):
    """The two sequence descriptions of a bucketed batch (`GraphedUpdate._build_seqs`: [(idx, cu, max_seqlen, table)] for the batch and
    its one-slot shift) padded into one shared bucket; `rows`, `row_len`: the bucketed batch shape.
      tokens     Tb = min(max(ladder(largest token count), MIN_TOKENS), rows * row_len) - idx padded to Tb (the tail is in range and
                 never read: the kernels take the real count from cu[Sb]);
      sequences  Sb = max(MIN_SEQS, next power of two of the larger sequence count) - cu padded to Sb + 1 by REPEATING its last
                 value (sequences of length zero; cu[Sb] stays the real token count);
      longest    ATTN_BLOCK * nqb with nqb = ceil(row_len / ATTN_BLOCK): no sequence is longer than a row; it only sizes the
                 attention grids, the kernels read the real lengths from cu.
    Returns (padded [(idx, cu, longest, table)], (Tb, Sb + 1, nqb)) - the second is the tables' part of the graph key."""
    cap = int(rows) * int(row_len)
    n_tok = max(int(b[0].size) for b in built)
    n_seq = max(int(b[1].size) - 1 for b in built)
    assert n_tok <= cap, (n_tok, rows, row_len)
    tb = min(max(ladder(n_tok), MIN_TOKENS), cap)
    sb = max(MIN_SEQS, 1 << max(n_seq - 1, 0).bit_length())
    nqb = (int(row_len) + ATTN_BLOCK - 1) // ATTN_BLOCK
    out = []
    for idx, cu, _, table in built:
        idx_b = np.zeros(tb, dtype=np.int64)
        idx_b[:idx.size] = idx
        cu_b = np.full(sb + 1, cu[-1], dtype=np.int32)
        cu_b[:cu.size] = cu
        out.append((idx_b, cu_b, ATTN_BLOCK * nqb, table))
    return out, (tb, sb + 1, nqb)
