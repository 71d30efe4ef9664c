"""One whole `train_one_batch()` as ONE hipGraph replay (small per-GPU batches are host-bound: about 500 kernel launches per update,
10 ms of wall time for 7.4 ms of kernels at 8 rows).  New design: the reference loops eagerly (algorithm/sac.py:359-362).

What varies from update to update is moved OUT of the captured region into static buffers that the host refreshes before each replay:
  * the sampling plan - the host half of `sample_trajs_device` (trajectory choice, numpy RNG, packing plan) runs as in the eager update
    and writes the int32 plan into a pinned buffer; the graph holds the H2D copy node and the gather kernel; with randomised loss masks
    (`randomize_mask`) the plan's selection of loss positions (`sel`, nested_replay_memory.py) travels the same way into a static
    buffer of fixed capacity, so the gather node's arguments never vary;
  * the REDQ critic subset - drawn on the host from the same numpy stream as the eager update, copied into static index tensors;
  * the step-dependent AdamW factors - `FlatAdamW.prepare_step()` (device-resident bias corrections), torch's `capturable` AdamW for
    the entropy coefficient;
  * the log scalars - packed into a static device buffer by the graph, copied to pinned memory behind the replay, read on demand like
    `DeferredLog`.
Every host -> device refresh and the log's read-back go through a RING of pinned staging slots and run as ordinary stream-ordered
copies around the replay (not as nodes of it): `step()` never waits for the update it has just launched - the host prepares update
i + 1 (sampling plan, tables, graph launch) while update i runs; a slot is reused three updates later, after its event.
Actor noise comes from torch's CUDA generator, which torch.cuda.graph registers: every replay draws fresh numbers.

A graph is valid for ONE batch shape (rows, row length, number of plan segments, longest segment).  With fixed-length episodes (the
synthetic benches) the exact shape recurs on every update.  With early termination it hardly ever does - the sampler trims a batch
to the longest row it drew - so the shapes are BUCKETED (`buckets`, buffers/transition_buffer/shape_buckets.py): rows, row length
and plan entries are rounded up a coarse ladder (1, 2, 3, 4, 6, 8, 12, ...; rows of at least 32 slots, never past the ring's row
capacity + 1) and the key becomes (rows, row length, plan entries).  The padding is what the sampler writes behind a short row
anyway (`mask = 0, start = 1`; plan entries with row -1 are dropped by the gather kernel; the losses divide by the sum of the mask):
the update computes the same thing on up to 1.5x the tokens, its GEMMs sum in another order (last-bit differences), and the actor
noise is drawn for the padded tensor (another sample of the same distribution).  `buckets='off'`: exact keys only.  `'on'`: bucketed
from the first update.  `'auto'`: exact keys until more distinct shapes (actor flag aside) have been seen than
the graphs can hold, then bucketed for good - a fixed-length workload never switches and stays bit for bit what it was.
Attention layers (cgpt) need more: their token / cu_seqlens tables vary with the batch inside one batch bucket.  By default `'on'`
raises for them and `'auto'` stays exact.  With `seq_buckets` (RESEL_GRAPH_SEQ_BUCKETS=1; opt-in like the bucket mode itself,
profiles/r09_cgpt_buckets.md) the two tables are padded into one more bucket (`shape_buckets.pad_seq_tables`: token count up the
ladder, sequences to a power of two - empty sequences, the real token count stays in cu_seqlens' last element ON THE DEVICE), the
decoder packs / unpacks with kernels that read that count (`ops.pack_tokens` / `unpack_tokens`) and the attention core defines the
token tail (`ops.attn_varlen(padded=True)`); the bucketed key is (rows, row length, plan entries, tokens, cu entries, attention
blocks per row, actor flag) and has in practice as many values as the batch bucket alone.  `train()` takes the mode from RESEL_GRAPH_BUCKETS (`buckets_from_env`: 1, auto; unset = 'off').  Every `step()` is exactly ONE `train_one_batch()`: `utd` PASSES (a pass is one iteration of the update's `utd` loop - one sampled batch,
one target, one critic step, one soft target update and, where `_actor_due` says so, an actor (+ alpha) step), each prepared on the host
and launched from the graph of its own launch sequence - the captured unit is the pass, not the step, and where this text says "update"
for what is recorded, replayed, counted or staged, it means a pass (utd = 1: the same thing).  A step with utd = 4, policy_utd = 2 is four
replays alternating between two recordings; the passes of one step may differ in shape (ragged batches) and mix replays, eager launches
and a recording.  Host random streams: the eager loop draws, per pass, the sampling plan and then the REDQ subset from numpy -
`_prepare` runs pass by pass and keeps that order; the constructor consumes no draw.  The update boundary (`ops.amax_maintenance()`, the
generation check) is once per `step()`, in front of the first pass; `amax_arena_zero`, the dropout base's advance and the restart of the
host's offset count are per recorded body, i.e. per pass - two passes of one step draw different masks.  The log: every key has a fixed slot
in the static buffer, a pass's log node writes its own keys only (a later pass overwrites an earlier one's, actor keys survive from the
last pass that ran the actor step - the eager loop's shared dict), ONE read-back behind the step's last pass into a pinned ring turned
per step; the returned log names the union of the keys the step's passes wrote, so nothing of an earlier step shows.  `eager_fallbacks`,
`_steps`, `_seen`, `warmup` and the capture window count passes.  The first `warmup`
passes run eagerly (allocator and lazily initialised kernels warm up), a shape is recorded the SECOND time it occurs (a shape that
never recurs is not worth two device synchronisations and an activation pool), at most `max_graphs` graphs live at a time in ONE
shared memory pool (they never replay concurrently), the least recently used one is dropped for a newcomer - but an evicted shape must
recur RECAPTURE_HITS times before it is recorded again and at most `max_graphs` recordings happen per CAPTURE_WINDOW updates, so a
workload with more recurring shapes than graphs settles into eager launches for the overflow instead of recording on every update;
any update without a graph runs eagerly from the same static inputs.
Attention layers (cgpt): the token index / cu_seqlens tables of the batch are built by `_prepare` into pinned buffers (copy nodes in the
graph; their sizes and the longest sequence are part of the shape key), and the counter-keyed dropout masks take their offsets from a
per-update host count (0, 4, 8, ... in program order - baked into the kernel nodes) PLUS a device word that a node of the graph
advances (`ops.dropout_offset_base`): every replay draws fresh masks, forward and backward kernels of one replay agree, and an eager
fallback through `step()` draws exactly what a replay would.
`policy_update_per` > 1 (every published launch script of the reference sets 2, gen_tmuxp_mamba_pomdp.py:81): whether the actor step is due
(reference :450-452) is part of the graph key - an update with and an update without the actor step are two recordings that alternate.
Gradient clipping (reference :239-250, 274-287) stays on the device: norm -> coefficient -> the scale word the flat AdamW kernel reads.
Data-parallel groups: the recording is CUT at each gradient exchange (`cut`) - an update is then three graphs replayed back to back with
the two all-reduces issued eagerly between them on the same stream (works with every backend; nothing waits on the host).
Randomised loss masks change the values of one column and no shape or launch; random truncation changes batch shapes like any ragged
workload (exact keys: most of its updates fall to `step()`'s eager launch; buckets absorb it).
Refused at construction (use the eager `train_one_batch`): the three-phase Q-guard exchange (RESEL_DP_GUARD=allreduce).  utd < 1 is an
error of the flag set (ValueError), not a refusal."""
import os
from collections import OrderedDict

import numpy as np
import torch

from ..buffers.transition_buffer.shape_buckets import NO_SEQ_BUCKETS, pad_plan, pad_seq_tables
from ..hip import ops
from ..models.flash_attention.TransformerFlashAttention import PackedSeqs
from ..models.rnn_base import training_pass
from ..utility.deferred_log import DeferredLog


def _exact_batch_key(pl):
    """The batch's part of the graph key without buckets: rows, row length, longest drawn row, plan segments."""
    return pl['nrow'], pl['longest'], pl['max_len'], pl['seg'].shape[0]


def _exact_table_key(built):
    """The sequence tables' part of the graph key without buckets: tokens, cu entries and longest sequence of both descriptions."""
    return tuple(x for b in built for x in (b[0].size, b[1].size, b[2]))


class GraphedUpdate:
    PLAN_CAPACITY = 16384                             # plan segments the static buffers hold (64 KB of pinned memory per slot)
    RING = 3                                          # pinned staging slots: the host may be this many passes (and logs: this many steps) ahead of the device
    SEEN_CAP = 1024                                   # shape keys remembered (variable-length episodes produce many that never recur)
    RECAPTURE_HITS = 8                                # occurrences an EVICTED shape needs before it is recorded again
    CAPTURE_WINDOW = 256                              # at most `max_graphs` recordings per this many passes: more recurring shapes than graphs run eagerly
    LOG_SLOTS = 64                                    # device scalars a run may log, one fixed slot each

    BUCKET_SHAPES = 8                                 # bucketed shapes held per launch sequence when the caller sets no `max_graphs`
    NO_SEQ_BUCKETS = NO_SEQ_BUCKETS + "; use buckets='off' or 'auto'"

    @staticmethod
    def buckets_from_env():
        """The `buckets` mode `train()` asks for: RESEL_GRAPH_BUCKETS = 1 'on', auto 'auto', 0 or unset 'off'; anything else is an error.
        Unset is 'off' (not 'auto') until bucketed replays have been timed against eager launches at the published batch sizes
        (profiles/r08_graph_buckets.md): a ragged workload is moved to padded batches only where its user asks for it."""
        v = os.environ.get('RESEL_GRAPH_BUCKETS', '')
        if v not in ('', '0', '1', 'auto'):
            raise ValueError(f'RESEL_GRAPH_BUCKETS={v!r}: 1 (bucketed from the first update), auto (once the shapes turn out ragged), '
                             f'0 or unset (exact shapes only)')
        return {'': 'off', '0': 'off', '1': 'on', 'auto': 'auto'}[v]

    @staticmethod
    def seq_buckets_from_env():
        """`seq_buckets=None` of the constructor: RESEL_GRAPH_SEQ_BUCKETS = 1 on; 0, empty or unset off; anything else is an error.
        Off until bucketed cgpt replays have been timed at the published sizes (profiles/r09_cgpt_buckets.md)."""
        v = os.environ.get('RESEL_GRAPH_SEQ_BUCKETS', '')
        if v not in ('', '0', '1'):
            raise ValueError(f'RESEL_GRAPH_SEQ_BUCKETS={v!r}: 1 (pad the sequence tables of attention layers into buckets), '
                             f'0 or unset (such layers keep exact shapes)')
        return v == '1'

    def __init__(self, alg, warmup=3, max_graphs=None, buckets='off', seq_buckets=None):
        why = self.refusal(alg)
        if why:
            raise RuntimeError('GraphedUpdate: ' + why)
        if alg.parameter.utd < 1:                     # an error of the flag set, not a reason to launch eagerly: the eager loop would run no pass either
            raise ValueError(f'GraphedUpdate: utd={alg.parameter.utd} (an update is at least one pass)')
        if buckets not in ('off', 'on', 'auto'):
            raise ValueError(f'GraphedUpdate: buckets={buckets!r} (off, on, auto)')
        # read HERE, not by the caller: `train()` builds `GraphedUpdate(self, buckets=GraphedUpdate.buckets_from_env())`
        self.seq_buckets = self.seq_buckets_from_env() if seq_buckets is None else bool(seq_buckets)
        if buckets == 'on' and alg._needs_seq_table and not self.seq_buckets:
            raise RuntimeError('GraphedUpdate: ' + self.NO_SEQ_BUCKETS)
        self.alg, self.device = alg, alg.device
        self.graphs = OrderedDict()                   # batch shape key -> CUDAGraph, least recently used first
        self._sequences = self.launch_sequences(alg)  # launch sequences per shape: with / without the actor step
        self._own_max_graphs = max_graphs is None
        if max_graphs is None:                        # four exact (eight bucketed) batch shapes per launch sequence
            max_graphs = (self.BUCKET_SHAPES if buckets == 'on' else 4) * self._sequences
        self.buckets = buckets                        # 'auto' becomes 'on' at most once (_count_shape)
        self._shapes = set()                          # 'auto': distinct exact shapes seen so far
        self.warmup, self.max_graphs = warmup, max_graphs
        # every counter below counts PASSES (one iteration of the `utd` loop; utd = 1: a pass is an update)
        self._eager_left = warmup                     # passes still to run eagerly before anything is recorded
        self._seen = OrderedDict()                    # batch shape key -> occurrences so far (least recently seen first; pruned to SEEN_CAP)
        self._captures = []                           # pass indices of the most recent recordings (capture-rate limit)
        self._steps = 0                               # passes launched so far
        self._updates = 0                             # `step()` calls so far (the log ring's turn)
        self._pass = (0, 0)                           # (utd_idx, actor steps so far) of the pass being prepared / launched (step, pass_position)
        self._amax_generation = ops.AMAX_GENERATION[0]
        self._pool = torch.cuda.graph_pool_handle()   # memory pool shared by every recorded graph (and by the segments of one update)
        self.eager_fallbacks = 0                      # passes launched eagerly through `step()`
        # data-parallel groups: the process group's watchdog thread polls events while this thread records - harmless, but a capture in the
        # default `global` mode treats such a call from ANOTHER thread as an error and invalidates the recording
        self._capture_mode = 'thread_local' if alg.grad_sync.active else 'global'
        self._rec = None                              # while recording: dict(segs=[(graph, exchange or None), ...], g=<graph being captured>)
        if alg.grad_sync.active:                      # every rank's Q-guard extrema ride behind the gradients: size the buffer before anything is recorded
            alg.values[0].store.ensure_grad_extra(4 + 4 * alg.grad_sync.world)
        E = alg.target_values[0].uni_network.layer_list[-1].num_ensemble
        self.E = E
        # static subset buffers sized WITHOUT consuming a draw: make the trainer's host draw once and put both numpy streams back
        st_np = np.random.get_state()
        alg._subset_stream()                          # data-parallel ranks create their shared stream on first use: create it BEFORE its state is saved
        rng_own = alg._subset_rng
        st_own = None if rng_own is None else rng_own.get_state()
        first = np.asarray(alg._select_target_ensemble(E))
        np.random.set_state(st_np)
        if st_own is not None:
            rng_own.set_state(st_own)
        self.subset_np = np.ascontiguousarray(first, dtype=np.int32)
        self.subset_i32 = torch.from_numpy(self.subset_np.copy()).to(self.device)
        self.subset_i64 = self.subset_i32.long()
        for opt in (alg.optimizer_value, alg.optimizer_policy):
            opt.enable_device_factors()
        oa = alg.optimizer_alpha                                             # torch AdamW over the entropy coefficient: capturable form
        for g in oa.param_groups:
            g['capturable'] = True
        for st in oa.state.values():
            if torch.is_tensor(st.get('step')):
                st['step'] = st['step'].to(self.device)
        self._plan_dev = torch.empty((self.PLAN_CAPACITY, 4), dtype=torch.int32, device=self.device)
        self._log_dev = torch.zeros(self.LOG_SLOTS, dtype=torch.float32, device=self.device)    # static target of the graphs' log nodes
        self._log_slots = {}                          # log key -> its fixed slot in `_log_dev` (handed out on a key's first appearance, log_node)
        # randomised loss masks: one word offset per plan entry + the bitmap words of every entry at the ring's row capacity
        self._sel_capacity = self.PLAN_CAPACITY * (1 + (alg.replay_buffer.max_traj_step + 31) // 32) if alg.parameter.randomize_mask else 0
        self._sel_dev = torch.zeros(self._sel_capacity, dtype=torch.int32, device=self.device) if self._sel_capacity else None
        self._ring = [dict(plan=torch.empty((self.PLAN_CAPACITY, 4), dtype=torch.int32, pin_memory=True),
                           sub=torch.empty(self.subset_np.size, dtype=torch.int32, pin_memory=True),
                           bc=torch.empty(4, dtype=torch.float32, pin_memory=True),
                           sel=torch.empty(self._sel_capacity, dtype=torch.int32, pin_memory=True) if self._sel_capacity else None,
                           evt=torch.cuda.Event(), used=False) for _ in range(self.RING)]
        # the log's read-back has a ring of its own, turned once per `step()`: with utd > RING a staging slot comes round again inside
        # one step, and the log handed out by the step before is still unread then
        self._log_ring = [dict(log=torch.empty(self.LOG_SLOTS, dtype=torch.float32, pin_memory=True), evt=torch.cuda.Event(), handed=None)
                          for _ in range(self.RING)]
        self._turn = 0
        self._slot = self._ring[0]
        self._plan = None                             # the sampling plan of the update being prepared / launched (_prepare)
        self._log_keys = self._log_items = None       # device scalars / host entries of the launch sequence last recorded or replayed (log_node, step)
        self._capture_stream = None                   # side stream the recordings are made on (created by the first one)
        # attention layers: static sequence tables (two descriptions per batch: the batch and its one-slot shift) and the dropout base
        self._seq = None
        self._seq_now = None                          # per description: (tokens, cu entries, longest sequence, table, padded) of this update (_prepare_seqs)
        self._drop_base = None
        self._drop_seed = 0
        if alg._needs_seq_table:
            self._drop_base = torch.zeros(1, dtype=torch.int64, device=self.device)
            ops.dropout_offset_base(self._drop_base)
            if not torch.cuda.default_generators:
                torch.cuda.init()
            dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self._drop_seed = torch.cuda.default_generators[dev_index].initial_seed() & ((1 << 64) - 1)

    DROP_STRIDE = 1 << 16                             # offsets one update may consume (4 per mask: 16 384 masks)

    def close(self):
        """Detach the process-wide dropout base again (eager trainers of the same process go back to torch's generator offsets)."""
        if self._drop_base is not None:
            ops.dropout_offset_base(None)
            self._drop_base = None

    def _seq_buffers(self, n_idx, n_cu):
        """Static pinned + device buffers of the two sequence descriptions; growing them invalidates every recorded graph."""
        sq = self._seq
        if sq is None or sq['cap_idx'] < n_idx or sq['cap_cu'] < n_cu:
            ci, cc = max(2 * n_idx, 1024), max(2 * n_cu, 64)
            self.graphs.clear()
            torch.cuda.synchronize(self.device)       # queued copies may still read the old blocks
            sq = self._seq = dict(cap_idx=ci, cap_cu=cc,
                                  idx_host=[[torch.empty(ci, dtype=torch.int64, pin_memory=True) for _ in range(2)] for _ in range(self.RING)],
                                  cu_host=[[torch.empty(cc, dtype=torch.int32, pin_memory=True) for _ in range(2)] for _ in range(self.RING)],
                                  idx_dev=[torch.empty(ci, dtype=torch.int64, device=self.device) for _ in range(2)],
                                  cu_dev=[torch.empty(cc, dtype=torch.int32, device=self.device) for _ in range(2)])
        return sq

    @staticmethod
    def _build_seqs(pl):
        """Host half of the sequence tables of attention layers (runs while the previous replay is still on the GPU)."""
        return PackedSeqs.build_host_pair(pl['table'], pl['nrow'], pl['longest'])

    def _prepare_seqs(self, built, padded_key=None):
        """Both descriptions into the pinned buffers (the previous replay has read them); returns their part of the shape key
        (`padded_key`: the tables were padded by `pad_seq_tables`, which also made their key)."""
        sq = self._seq_buffers(max(b[0].size for b in built), max(b[1].size for b in built))
        k = self._turn % self.RING
        for i, (idx, cu, mx, tb) in enumerate(built):
            # staged with numpy (a plain memcpy): a torch CPU copy_ of > 32 768 elements opens an intra-op parallel region over all host threads,
            # which on a loaded host took 10-15 ms per call - longer than the replay it is meant to hide behind
            sq['idx_host'][k][i].numpy()[:idx.size] = idx
            sq['cu_host'][k][i].numpy()[:cu.size] = cu
            sq['idx_dev'][i][:idx.size].copy_(sq['idx_host'][k][i][:idx.size], non_blocking=True)      # stream-ordered, outside the graph
            sq['cu_dev'][i][:cu.size].copy_(sq['cu_host'][k][i][:cu.size], non_blocking=True)
        self._seq_now = [(b[0].size, b[1].size, b[2], b[3], padded_key is not None) for b in built]
        return padded_key if padded_key is not None else _exact_table_key(built)

    def packed_seqs(self):
        """Called by the trainer's `_sample` while this object drives the update: views of the static device tables (refreshed by
        `_prepare_seqs` before the replay); None without attention layers."""
        sq = self._seq
        if sq is None:
            return None
        return [PackedSeqs.from_static(sq['idx_dev'][i][:n_idx], sq['cu_dev'][i][:n_cu], mx, tb, padded=padded)
                for i, (n_idx, n_cu, mx, tb, padded) in enumerate(self._seq_now)]

    @staticmethod
    def refusal(alg):
        par = alg.parameter
        if alg.device.type != 'cuda':
            return 'needs a GPU'
        if getattr(alg, 'grad_sync', None) is None:
            return 'not a full-trajectory trainer'
        if alg.grad_sync.active and os.environ.get('RESEL_DP_GUARD', 'bucket') == 'allreduce':
            return 'the three-phase Q-guard exchange (RESEL_DP_GUARD=allreduce) issues collectives inside the target computation'
        if not (alg.device_replay and alg.replay_buffer.device_supported(randomize_mask=par.randomize_mask)):
            return 'needs the device-resident replay ring'
        return None

    @staticmethod
    def pass_schedule(alg):
        """The actor flags of the passes of the coming `train_one_batch()` (one per iteration of its `utd` loop), obtained only by walking
        the trainer's `_actor_due` the way that loop does.  Host only: works on a CPU trainer, touches nothing."""
        flags = []
        for utd_idx in range(alg.parameter.utd):
            flags.append(bool(alg._actor_due(utd_idx, sum(flags))))
        return flags

    @staticmethod
    def launch_sequences(alg):
        """Launch sequences per batch shape: 2 if two passes of a run can differ in their actor flag - within one step (policy_utd < utd
        spreads the actor steps over the passes) or from step to step (policy_update_per > 1) -, 1 otherwise.  Walks `pass_schedule` over
        one period of `grad_num` (the schedule depends on it only through grad_num % policy_update_per); `grad_num` is put back."""
        kept, flags = alg.grad_num, set()
        try:
            for alg.grad_num in range(max(1, alg.parameter.policy_update_per)):
                flags.update(GraphedUpdate.pass_schedule(alg))
        finally:
            alg.grad_num = kept
        return max(1, len(flags))

    # ---- called by the trainer while `alg._graph is self` -------------------------------------------------------------------
    def pass_position(self):
        """The trainer's `_train_one_batch` while this object drives the update: (utd_idx, actor steps so far) of the ONE pass it is to run."""
        return self._pass

    def gather(self):
        pl = self._plan
        n = pl['seg'].shape[0]
        # the whole static selection buffer: its capacity, not this plan's size, is the `sel_words` baked into the graph node
        dev = self.alg.replay_buffer.gather_planned(self.device, self._plan_dev[:n], pl['max_len'], pl['nrow'], pl['longest'],
                                                    sel_dev=self._sel_dev)
        return dev, pl['total_size'], pl.get('nrow_real', pl['nrow'])

    def target_subset(self):
        """The trainer's `_target_subset`: the constructor's draw (its size is every draw's) and the static device copies of the
        subset `_prepare` drew for this update."""
        return self.subset_np, lambda as_long=False: self.subset_i64 if as_long else self.subset_i32

    def cut(self, exchange):
        """Called by the trainer where ranks exchange gradients (`_finish_step`).  Recording: the graph being captured ends here, the
        exchange is remembered behind it and a new graph begins (same pool, same stream) - the exchange is NOT issued while recording
        (nothing has run yet).  Otherwise (eager launch through `step()`): issue it now."""
        rec = self._rec
        if rec is None:
            exchange()
            return
        rec['g'].capture_end()
        rec['segs'].append((rec['g'], exchange))
        rec['g'] = torch.cuda.CUDAGraph()
        rec['g'].capture_begin(pool=self._pool, capture_error_mode=self._capture_mode)

    def _record(self):
        """Record one update as a list of (graph, exchange) segments; one segment unless the trainer cuts (data parallel)."""
        torch.cuda.synchronize(self.device)
        torch.cuda.empty_cache()
        if self._capture_stream is None:
            self._capture_stream = torch.cuda.Stream(device=self.device)
        side = self._capture_stream
        side.wait_stream(torch.cuda.current_stream(self.device))
        rec = self._rec = dict(segs=[], g=torch.cuda.CUDAGraph())
        try:
            with torch.cuda.stream(side):
                rec['g'].capture_begin(pool=self._pool, capture_error_mode=self._capture_mode)
                try:
                    self._body()                      # recorded, not run: the prepared inputs are consumed by the replay that follows
                finally:
                    rec['g'].capture_end()
                rec['segs'].append((rec['g'], None))
        finally:
            self._rec = None
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        return dict(segs=rec['segs'], log_keys=self._log_keys, log_items=self._log_items)

    def log_node(self, keys, packed, host_items):
        """The trainer's `_log` of ONE pass.  Every key has a fixed slot in the static buffer and a pass writes only its own keys (copy
        nodes of the graph, one per run of neighbouring slots): the passes of a step merge on the device, a later pass overwriting an
        earlier one's keys - what the eager loop's shared `scal` does.  The read-back follows the step's last pass (`_finish`)."""
        self._log_keys, self._log_items = keys, host_items
        slots = [self._log_slots.setdefault(k, len(self._log_slots)) for k in keys]
        if len(self._log_slots) > self.LOG_SLOTS:
            raise RuntimeError(f'GraphedUpdate: more than {self.LOG_SLOTS} logged device scalars')
        i = 0
        while i < len(slots):
            j = i + 1
            while j < len(slots) and slots[j] == slots[j - 1] + 1:
                j += 1
            self._log_dev[slots[i]:slots[i] + j - i].copy_(packed[i:j])
            i = j
        return None

    # ---- host side of one pass ------------------------------------------------------------------------------------------------
    def _prepare(self):
        """Host half of the pass at `self._pass`: sampling plan, then the REDQ subset - the order in which the eager loop draws them from
        numpy, pass by pass -, the AdamW factors (the critic's every pass, the policy's only where the actor step is due) into one
        staging slot.  -> the graph key: the batch shape key + the actor flag of this pass."""
        alg, par = self.alg, self.alg.parameter
        pl = alg.replay_buffer.plan_trajs_device(par.sac_batch_size, None, random_trunc_traj=par.random_trunc_traj,
                                                 nest_stack_trajs=alg.allow_nest_stack, buckets=self.buckets == 'on',
                                                 randomize_mask=par.randomize_mask, valid_number_post_randomized=par.valid_number_post_randomized)
        built = None
        if self.buckets == 'auto':
            if self._drop_base is not None and self.seq_buckets:            # the exact key of attention layers holds the table sizes too
                built = self._build_seqs(pl)
            if self._count_shape(pl, built):
                pl = pad_plan(pl, alg.replay_buffer.max_traj_step)          # the plan that tipped the count is the first bucketed one
                built = None
        alg.replay_buffer._mirror(self.device)        # transitions pushed since the last update reach the device ring HERE, outside the graph
        n = pl['seg'].shape[0]
        if n > self.PLAN_CAPACITY:
            raise RuntimeError(f'GraphedUpdate: {n} plan segments exceed the static plan buffer ({self.PLAN_CAPACITY})')
        n_sel = pl['sel'].size if 'sel' in pl else 0
        if n_sel > self._sel_capacity:
            raise RuntimeError(f'GraphedUpdate: {n_sel} selection words exceed the static selection buffer ({self._sel_capacity})')
        # bucketed: `max_len` is the row length (it only sizes the gather grid)
        key = (pl['nrow'], pl['longest'], n) if self.buckets == 'on' else _exact_batch_key(pl)
        if self._drop_base is not None and built is None:
            built = self._build_seqs(pl)
        # staging slot of this pass: its copies of three passes ago have long run
        slot = self._slot = self._ring[self._turn % self.RING]
        if slot['used']:
            slot['evt'].synchronize()
        if built is not None and self.buckets == 'on':                      # reachable with `seq_buckets` only
            padded, seq_key = pad_seq_tables(built, pl['nrow'], pl['longest'])
            key = key + self._prepare_seqs(padded, seq_key)
        elif built is not None:
            key = key + self._prepare_seqs(built)
        slot['plan'].numpy()[:n] = pl['seg']
        self._plan_dev[:n].copy_(slot['plan'][:n], non_blocking=True)        # stream-ordered: behind the previous update's gather
        if n_sel:
            slot['sel'].numpy()[:n_sel] = pl['sel']
            self._sel_dev[:n_sel].copy_(slot['sel'][:n_sel], non_blocking=True)
        self._plan = pl
        sub = np.ascontiguousarray(np.asarray(alg._select_target_ensemble(self.E)), dtype=np.int32)
        slot['sub'].numpy()[...] = sub
        self.subset_i32.copy_(slot['sub'], non_blocking=True)
        self.subset_i64.copy_(self.subset_i32)
        # is the actor step due in this pass?  Part of the key: the two launch sequences are two graphs
        actor_due = alg._actor_due(*self._pass)
        for i, opt in enumerate((alg.optimizer_value, alg.optimizer_policy)):
            if i == 0 or actor_due:
                opt.prepare_step(slot['bc'][2 * i:2 * i + 2])
        self._turn += 1
        return key + (bool(actor_due),)

    def _count_shape(self, pl, built=None):
        """'auto': True once, when this exact shape is one more than the graphs can hold (`max_graphs` over the launch sequences) - the
        workload is ragged, exact keys would leave most updates eager.  Drops what was recorded and counted for exact keys."""
        if self.alg._needs_seq_table and not self.seq_buckets:      # attention layers: no buckets (NO_SEQ_BUCKETS)
            return False
        self._shapes.add(_exact_batch_key(pl) + (() if built is None else _exact_table_key(built)))
        if len(self._shapes) <= max(1, self.max_graphs // self._sequences):
            return False
        self.buckets = 'on'
        if self._own_max_graphs:
            self.max_graphs = self.BUCKET_SHAPES * self._sequences
        self.graphs.clear()
        self._seen.clear()
        self._captures = []
        self.alg.logger(f'update graphs: {len(self._shapes)} batch shapes in {self._steps + 1} {"updates" if self.alg.parameter.utd == 1 else "passes"} - batch shapes are bucketed from here on '
                        f'(RESEL_GRAPH_BUCKETS=0 keeps exact shapes)')
        self._shapes.clear()
        return True

    def _body(self):
        alg = self.alg
        alg._graph = self
        for opt in (alg.optimizer_value, alg.optimizer_policy):
            opt.device_factors_active = True
        if self._drop_base is not None:
            ops.DROP_OVERRIDE = [self._drop_seed, 0]
        try:
            ops.amax_arena_zero(self.device)          # first node: a replay publishes operand magnitudes into the slots / epochs baked into the graph
            if self._drop_base is not None:
                self._drop_base.add_(self.DROP_STRIDE)                       # a node: every replay moves the masks of the whole update on
            with training_pass():
                alg._train_one_batch()                # below the eager entry's update-boundary work: `step()` does that itself
        finally:
            ops.DROP_OVERRIDE = None
            alg._graph = None
            for opt in (alg.optimizer_value, alg.optimizer_policy):
                opt.device_factors_active = False

    def _finish(self, keys, items):
        """The step's ONE read-back, behind its last pass on the stream: the whole slot buffer into this step's pinned block; the log
        names `keys` - the union of the keys its passes wrote, so a step without an actor step shows no actor key of an earlier one."""
        ring = self._log_ring[self._updates % self.RING]
        if ring['handed'] is not None:                # the log handed out RING steps ago is read out before its block is reused
            ring['handed'].resolve()
        n = len(self._log_slots)
        ring['log'][:n].copy_(self._log_dev[:n], non_blocking=True)
        ring['evt'].record()
        pl = self._plan                               # the host entries of the LAST pass, as the eager `_log` takes them
        items = dict(items, **self.alg._host_log(pl['total_size'], pl.get('nrow_real', pl['nrow'])))
        ring['handed'] = DeferredLog(keys, ring['log'][:n], ring['evt'], items, index=[self._log_slots[k] for k in keys])
        self._updates += 1
        return ring['handed']

    def step(self):
        """Exactly one `train_one_batch()`: `utd` passes, each prepared on the host (`_prepare`: plan, then subset - the eager loop's
        order of numpy draws) and launched from its own launch sequence (`_launch_pass`: a replay, an eager launch or a recording, mixed
        freely within one step); the update-boundary work once, in front of the first pass; one log, read back once behind the last."""
        if ops.amax_maintenance() or self._amax_generation != ops.AMAX_GENERATION[0]:
            self.graphs.clear()                       # the magnitude epochs started over: recorded kernel nodes carry epochs of the old generation
            self._amax_generation = ops.AMAX_GENERATION[0]
        alg = self.alg
        keys, items, actor_steps = {}, {}, 0
        for utd_idx in range(alg.parameter.utd):
            self._pass = (utd_idx, actor_steps)       # read by `_prepare` (the key, the AdamW factors) and by the trainer (`pass_position`)
            actor_steps += self._launch_pass()
            keys.update(dict.fromkeys(self._log_keys))                       # device scalars: merged in `_log_dev`, named here
            items.update(self._log_items)             # host entries: a later pass wins, an earlier one's survive (the eager loop's `host`)
        self._pass = (0, 0)
        return self._finish(list(keys), items)

    def _launch_pass(self):
        """One pass: eager while warming up or while its batch shape has no graph, a replay otherwise.  -> did it run the actor step."""
        key = self._prepare()
        g = self.graphs.get(key)
        self._steps += 1
        if g is None:
            seen = self._seen[key] = self._seen.get(key, 0) + 1
            self._seen.move_to_end(key)
            while len(self._seen) > self.SEEN_CAP:
                self._seen.popitem(last=False)
            # a recording costs two device synchronisations and a whole capture pass: with more recurring shapes than `max_graphs` an
            # evict-and-record-again policy would turn every pass into capture + replay.  Hence: an evicted shape has to recur
            # RECAPTURE_HITS times before it is recorded again, and no more than `max_graphs` recordings per CAPTURE_WINDOW passes -
            # whatever has no graph runs eagerly (the same pass from the same static inputs).
            self._captures = [t for t in self._captures if self._steps - t < self.CAPTURE_WINDOW]
            throttled = len(self.graphs) >= self.max_graphs and len(self._captures) >= self.max_graphs
            if self._eager_left > 0 or seen < 2 or throttled:      # warm-up passes / a shape on its first visit: the same pass, launched eagerly
                self._eager_left = max(0, self._eager_left - 1)
                self.eager_fallbacks += 1
                self._body()
                return self._launched(key)
            if len(self.graphs) >= self.max_graphs:
                old_key, _ = self.graphs.popitem(last=False)       # least recently used; its activations return to the shared pool
                self._seen[old_key] = 2 - self.RECAPTURE_HITS
            self._captures.append(self._steps)
            g = self.graphs[key] = self._record()
        self.graphs.move_to_end(key)
        self._log_keys, self._log_items = g['log_keys'], g['log_items']      # of THIS launch sequence (with / without the actor step)
        for seg, exchange in g['segs']:
            seg.replay()
            if exchange is not None:
                exchange()                            # the gradient all-reduce, eagerly between two replays on the same stream
        if ops.AMAX_VERIFY:                           # the recorded pass contains the check kernels: read their verdict behind the replay
            ops.amax_verify_raise(self.device)
        return self._launched(key)

    def _launched(self, key):
        """Behind a pass on the stream: its staging slot is free once this event has passed.  -> the pass's actor flag."""
        self._slot['evt'].record()
        self._slot['used'] = True
        return key[-1]

    @property
    def graph(self):                                  # the most recently recorded graph (tests): its first segment
        return next(reversed(self.graphs.values()))['segs'][0][0] if self.graphs else None
