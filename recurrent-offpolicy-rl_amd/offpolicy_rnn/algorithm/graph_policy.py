"""Host bookkeeping of the update graphs (algorithm/graphed_update.py): what a graph key is, whether a pass is replayed, launched
eagerly or recorded, and which of a pass's log slots are neighbours.  Hashable keys and lists only - no torch, no tensor, no trainer
in here, so every rule below runs in a CPU test (tests/test_graph_policy.py)."""
from collections import OrderedDict

REPLAY, EAGER, RECORD = 'replay', 'eager', 'record'


def exact_batch_key(pl):
    """The batch's part of the graph key without buckets: rows, row length, longest drawn row, plan segments."""
    return pl['nrow'], pl['longest'], pl['max_len'], pl['seg'].shape[0]


def exact_table_key(built):
    """The sequence tables' part of the graph key without buckets: tokens, cu entries and longest sequence of both descriptions."""
    return tuple(x for b in built for x in (b[0].size, b[1].size, b[2]))


def graph_key(pl, table_key, bucketed, actor):
    """The key of the graph that can replay the pass of plan `pl` - a graph is valid for ONE batch shape and one launch sequence:
      exact     (rows, row length, longest drawn row, plan segments) [+ `exact_table_key`] + (actor,)
      bucketed  (rows, row length, plan entries) [+ the padded tables' key of `shape_buckets.pad_seq_tables`] + (actor,)
    `pl` is the padded plan then and its `max_len` is the row length (it only sizes the gather grid).  `table_key`: attention layers
    only, () otherwise.  `actor`: is the actor step due in this pass - with and without it are two recordings that alternate."""
    batch = (pl['nrow'], pl['longest'], pl['seg'].shape[0]) if bucketed else exact_batch_key(pl)
    return batch + tuple(table_key) + (bool(actor),)


def slot_runs(slots):
    """[(i, j)]: `slots[i:j]` are the maximal runs of neighbouring, ascending log slots - one copy node each."""
    starts = [i for i in range(len(slots)) if i == 0 or slots[i] != slots[i - 1] + 1]
    return list(zip(starts, starts[1:] + [len(slots)]))


class RecordingPolicy:
    """Which passes are recorded.  Every counter counts PASSES (utd = 1: a pass is an update).
      * The first `warmup` passes without a graph run eagerly (allocator and lazily initialised kernels warm up).
      * A shape is recorded the SECOND time it occurs: one that never recurs is not worth two device synchronisations and an
        activation pool.
      * At most `max_graphs` recordings live at a time (one shared memory pool, they never replay concurrently); the least recently
        used one makes room for a newcomer.  A recording costs a whole capture pass, and with more recurring shapes than `max_graphs`
        evict-and-record-again would turn every pass into capture + replay.  Hence an evicted shape must recur RECAPTURE_HITS times
        before it is recorded again, and at most `max_graphs` recordings happen per CAPTURE_WINDOW passes: the overflow settles into
        eager launches (the same pass from the same static inputs).
      * `buckets`: 'off' exact keys only, 'on' bucketed from the first pass, 'auto' exact until more distinct exact shapes (actor flag
        aside) have been seen than the graphs can hold - `max_graphs` over the launch `sequences` -, then 'on' for good (`tips`); a
        fixed-length workload never switches.  `can_bucket=False` (attention layers without `seq_buckets`): 'auto' stays exact.
    `max_graphs=None`: four exact, BUCKET_SHAPES bucketed shapes per launch sequence.
    `recorded` maps each recorded key to whatever the driver keeps for it, least recently used first; only its keys are read here."""
    SEEN_CAP = 1024                                   # shape keys remembered (variable-length episodes produce many that never recur)
    RECAPTURE_HITS = 8                                # occurrences an EVICTED shape needs before it is recorded again
    CAPTURE_WINDOW = 256                              # at most `max_graphs` recordings per this many passes
    BUCKET_SHAPES = 8                                 # bucketed shapes held per launch sequence when the caller sets no `max_graphs`

    def __init__(self, warmup=3, max_graphs=None, buckets='off', sequences=1, can_bucket=True):
        self.sequences, self.can_bucket = sequences, can_bucket
        self.own_max_graphs = max_graphs is None
        if max_graphs is None:
            max_graphs = (self.BUCKET_SHAPES if buckets == 'on' else 4) * sequences
        self.buckets, self.max_graphs = buckets, max_graphs
        self.eager_left = warmup                      # passes still to run eagerly before anything is recorded
        self.recorded = OrderedDict()
        self.seen = OrderedDict()                     # key -> occurrences without a graph (least recently seen first; pruned to SEEN_CAP)
        self.shapes = set()                           # 'auto': distinct exact shapes so far
        self.captures = []                            # pass numbers of the recordings inside the window
        self.steps = 0                                # passes decided so far
        self.eager_fallbacks = 0                      # ... of which launched eagerly

    def tips(self, exact_key):
        """'auto', asked with the exact key of every pass in front of `decide`: does this shape tip the run into buckets?  -> the number
        of distinct shapes if it is one more than the graphs can hold (the workload is ragged: exact keys would leave most passes eager),
        else 0.  Tipping drops what was recorded and counted for exact keys and re-derives a `max_graphs` the caller did not choose."""
        if not self.can_bucket:
            return 0
        self.shapes.add(exact_key[:-1])
        n = len(self.shapes)
        if n <= max(1, self.max_graphs // self.sequences):
            return 0
        self.buckets = 'on'
        if self.own_max_graphs:
            self.max_graphs = self.BUCKET_SHAPES * self.sequences
        self.recorded.clear()
        self.seen.clear()
        self.captures = []
        self.shapes.clear()
        return n

    def decide(self, key):
        """One pass of `key` -> (REPLAY | EAGER | RECORD, the key evicted to make room or None).  After RECORD the caller stores its
        recording under `recorded[key]`."""
        self.steps += 1
        if key in self.recorded:
            self.recorded.move_to_end(key)
            return REPLAY, None
        seen = self.seen[key] = self.seen.get(key, 0) + 1
        self.seen.move_to_end(key)
        while len(self.seen) > self.SEEN_CAP:
            self.seen.popitem(last=False)
        self.captures = [t for t in self.captures if self.steps - t < self.CAPTURE_WINDOW]
        full = len(self.recorded) >= self.max_graphs
        if self.eager_left > 0 or seen < 2 or (full and len(self.captures) >= self.max_graphs):
            self.eager_left = max(0, self.eager_left - 1)
            self.eager_fallbacks += 1
            return EAGER, None
        evicted = None
        if full:
            evicted, _ = self.recorded.popitem(last=False)         # its activations return to the shared pool
            self.seen[evicted] = 2 - self.RECAPTURE_HITS
        self.captures.append(self.steps)
        return RECORD, evicted
