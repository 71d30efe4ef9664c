"""Shape buckets of the packed batch (new design; the reference trims every batch to the longest row it drew, nested_replay_memory.py).

A recorded update graph (algorithm/graphed_update.py) is valid for one batch shape, and with early-terminating episodes the exact
shape - rows, row length, plan segments - hardly ever recurs.  Rounding each of the three UP to a coarse ladder makes a handful of
shapes cover every batch.  The extra slots are what the sampler writes behind a short row anyway (`mask = 0, start = 1`), the extra
plan entries carry row -1 and are dropped by the gather kernel, the losses divide by the sum of the mask: the padded update computes
what the exact one does, at up to 1.5x the tokens in the worst case.

Host arithmetic only: no torch in here (the planner runs while the previous update is still on the GPU)."""
import numpy as np

MIN_ROW_LEN = 32                                      # shorter rows are not worth a shape of their own
MIN_NSEG = 16


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
    `longest_real`."""
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
    return dict(pl, seg=seg_b, table=table_b, nrow=rows, longest=row_len, max_len=row_len, nrow_real=pl['nrow'], longest_real=pl['longest'])
