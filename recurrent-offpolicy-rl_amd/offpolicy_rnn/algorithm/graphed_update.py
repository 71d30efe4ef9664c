"""One whole `train_one_batch()` as hipGraph replays (small per-GPU batches are host-bound: about 500 kernel launches per update,
10 ms of wall time for 7.4 ms of kernels at 8 rows).  New design: the reference loops eagerly (algorithm/sac.py:359-362).

What leaves the captured region.  Whatever varies from update to update sits in static buffers that the host refreshes before each
replay, through pinned staging slots and ordinary stream-ordered copies (graph_staging.py):
  * the sampling plan - the host half of `sample_trajs_device` (trajectory choice, numpy RNG, packing plan) runs as in the eager update;
    the graph holds the gather kernel.  With randomised loss masks (`randomize_mask`) the plan's selection of loss positions (`sel`,
    nested_replay_memory.py) travels the same way into a static buffer of fixed capacity, so the gather node's arguments never vary;
  * the REDQ critic subset - drawn on the host from the same numpy stream as the eager update;
  * the step-dependent AdamW factors - `FlatAdamW.prepare_step()` (device-resident bias corrections), torch's `capturable` AdamW for
    the entropy coefficient;
  * attention layers (cgpt): the token index / cu_seqlens tables of the batch, and the counter-keyed dropout masks, which take their
    offsets from a per-pass host count (0, 4, 8, ... in program order - baked into the kernel nodes) PLUS a device word that a node of
    the graph advances (`ops.dropout_offset_base`): every replay draws fresh masks, forward and backward kernels of one replay agree,
    and an eager launch through `step()` draws exactly what a replay would;
  * the log scalars - packed into a static device buffer by the graph, read back behind the step (graph_staging.UpdateLog).
Actor noise comes from torch's CUDA generator, which torch.cuda.graph registers: every replay draws fresh numbers.  Gradient clipping
(reference :239-250, 274-287) stays on the device: norm -> coefficient -> the scale word the flat AdamW kernel reads.

What a pass is.  Every `step()` is exactly ONE `train_one_batch()`: `utd` PASSES (a pass is one iteration of the update's `utd` loop -
one sampled batch, one target, one critic step, one soft target update and, where `_actor_due` says so, an actor (+ alpha) step), each
prepared on the host and launched from the graph of its own launch sequence.  The captured unit is the pass, not the step (utd = 1:
the same thing): a step with utd = 4, policy_utd = 2 is four replays alternating between two recordings; the passes of one step may
differ in shape (ragged batches) and mix replays, eager launches and a recording.  The eager loop draws, per pass, the sampling plan
and then the REDQ subset from numpy - `_prepare` runs pass by pass and keeps that order; the constructor consumes no draw.  The
update boundary (`ops.amax_maintenance()`, the generation check) is once per `step()`, in front of the first pass; `amax_arena_zero`,
the dropout base's advance and the restart of the host's offset count are per recorded body, i.e. per pass - two passes of one step
draw different masks.  Data-parallel groups: the recording is CUT at each gradient exchange (`cut`) - a pass is then three graphs
replayed back to back with the two all-reduces issued eagerly between them on the same stream (works with every backend; nothing
waits on the host).

What a key is.  A graph is valid for one batch shape and one launch sequence (`graph_policy.graph_key`).  With fixed-length episodes
(the synthetic benches) the exact shape recurs on every update.  With early termination it hardly ever does - the sampler trims a
batch to the longest row it drew - so the shapes are BUCKETED (`buckets`, buffers/transition_buffer/shape_buckets.py): rows, row
length and plan entries are rounded up a coarse ladder (1, 2, 3, 4, 6, 8, 12, ...; rows of at least 32 slots, never past the ring's
row capacity + 1).  The padding is what the sampler writes behind a short row anyway (`mask = 0, start = 1`; plan entries with row -1
are dropped by the gather kernel; the losses divide by the sum of the mask): the update computes the same thing on up to 1.5x the
tokens, its GEMMs sum in another order (last-bit differences), and the actor noise is drawn for the padded tensor (another sample of
the same distribution).  `train()` takes the mode from RESEL_GRAPH_BUCKETS (`buckets_from_env`).
Attention layers need more: their two tables vary with the batch inside one batch bucket.  By default `'on'` raises for them and
`'auto'` stays exact.  With `seq_buckets` (RESEL_GRAPH_SEQ_BUCKETS=1; opt-in like the bucket mode itself, profiles/r09_cgpt_buckets.md)
the tables are padded into one more bucket (`shape_buckets.pad_seq_tables`: token count up the ladder, sequences to a power of two -
empty sequences, the real token count stays in cu_seqlens' last element ON THE DEVICE), the decoder packs / unpacks with kernels that
read that count (`ops.pack_tokens` / `unpack_tokens`) and the attention core defines the token tail (`ops.attn_varlen(padded=True)`);
the key then has in practice as many values as the batch bucket alone.
Randomised loss masks change the values of one column and no shape or launch; random truncation changes batch shapes like any ragged
workload (exact keys: most of its passes fall to `step()`'s eager launch; buckets absorb it).

Where each part lives.  graph_policy.py (host only): the key, and `RecordingPolicy` - is a pass replayed, launched eagerly or recorded,
and when does 'auto' turn to 'on'.  graph_staging.py: `PassStaging`, the pinned slot of a pass, and `UpdateLog`, the log's slots and
read-back.  Here: `GraphedUpdate`, the driver - the static device inputs, the host half of a pass (`_prepare`), the recording
(`_record`, `_body`, `cut`) and the launch (`step`, `_launch_pass`).

Refused at construction (use the eager `train_one_batch`): the three-phase Q-guard exchange (RESEL_DP_GUARD=allreduce).  utd < 1 is an
error of the flag set (ValueError), not a refusal."""
import gc
import os

import numpy as np
import torch

from ..buffers.transition_buffer.shape_buckets import NO_SEQ_BUCKETS, pad_plan, pad_seq_tables
from ..hip import ops
from ..models.flash_attention.TransformerFlashAttention import PackedSeqs
from ..models.rnn_base import training_pass
from .graph_policy import RECORD, REPLAY, RecordingPolicy, exact_table_key, graph_key
from .graph_staging import PassStaging, UpdateLog


class GraphedUpdate:
    PLAN_CAPACITY = 16384                             # plan segments the static buffers hold (64 KB of pinned memory per slot)
    LOG_SLOTS = 64                                    # device scalars a run may log, one fixed slot each
    SEEN_CAP, RECAPTURE_HITS = RecordingPolicy.SEEN_CAP, RecordingPolicy.RECAPTURE_HITS
    CAPTURE_WINDOW, BUCKET_SHAPES = RecordingPolicy.CAPTURE_WINDOW, RecordingPolicy.BUCKET_SHAPES
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
        self.alg, self.device, self.warmup = alg, alg.device, warmup
        self._sequences = self.launch_sequences(alg)  # launch sequences per shape: with / without the actor step
        self.recording = RecordingPolicy(warmup, max_graphs, buckets, self._sequences, can_bucket=self.seq_buckets or not alg._needs_seq_table)
        self.graphs = self.recording.recorded            # key -> dict(segs=[(CUDAGraph, exchange or None), ...], ...), least recently used first
        self._seen = self.recording.seen
        self._pass = (0, 0)                           # (utd_idx, actor steps so far) of the pass being prepared / launched (step, pass_position)
        self._amax_generation = ops.AMAX_GENERATION[0]
        self._pool = torch.cuda.graph_pool_handle()   # memory pool shared by every recorded graph (and by the segments of one pass)
        # data-parallel groups: the process group's watchdog thread polls events while this thread records - harmless, but a capture in the
        # default `global` mode treats such a call from ANOTHER thread as an error and invalidates the recording
        self._capture_mode = 'thread_local' if alg.grad_sync.active else 'global'
        self._rec = None                              # while recording: dict(segs=[(graph, exchange or None), ...], g=<graph being captured>)
        if alg.grad_sync.active:                      # every rank's Q-guard extrema ride behind the gradients: size the buffer before anything is recorded
            alg.values[0].store.ensure_grad_extra(4 + 4 * alg.grad_sync.world)
        self.E = alg.target_values[0].uni_network.layer_list[-1].num_ensemble
        # static subset buffers sized WITHOUT consuming a draw: make the trainer's host draw once and put both numpy streams back
        st_np = np.random.get_state()
        alg._subset_stream()                          # data-parallel ranks create their shared stream on first use: create it BEFORE its state is saved
        rng_own = alg._subset_rng
        st_own = None if rng_own is None else rng_own.get_state()
        first = np.asarray(alg._select_target_ensemble(self.E))
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
        # randomised loss masks: one word offset per plan entry + the bitmap words of every entry at the ring's row capacity
        self._sel_capacity = self.PLAN_CAPACITY * (1 + (alg.replay_buffer.max_traj_step + 31) // 32) if alg.parameter.randomize_mask else 0
        self._sel_dev = torch.zeros(self._sel_capacity, dtype=torch.int32, device=self.device) if self._sel_capacity else None
        self.staging = PassStaging(self.PLAN_CAPACITY, self._sel_capacity, self.subset_np.size, self.device)
        self.log = UpdateLog(self.LOG_SLOTS, self.device)
        self._plan = None                             # the sampling plan of the pass being prepared / launched (_prepare)
        self._log_keys = self._log_items = None       # device scalars / host entries of the launch sequence last recorded or replayed (log_node, step)
        self._capture_stream = None                   # side stream the recordings are made on (created by the first one)
        self._drop_base = None                        # attention layers: the device word the dropout offsets start from
        self._drop_seed = 0
        if alg._needs_seq_table:
            self._drop_base = torch.zeros(1, dtype=torch.int64, device=self.device)
            ops.dropout_offset_base(self._drop_base)
            if not torch.cuda.default_generators:
                torch.cuda.init()
            dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self._drop_seed = torch.cuda.default_generators[dev_index].initial_seed() & ((1 << 64) - 1)

    DROP_STRIDE = 1 << 16                             # offsets one pass may consume (4 per mask: 16 384 masks)

    # read-only views on the recording policy
    buckets = property(lambda self: self.recording.buckets)                     # 'auto' becomes 'on' at most once
    max_graphs = property(lambda self: self.recording.max_graphs)
    eager_fallbacks = property(lambda self: self.recording.eager_fallbacks)     # passes launched eagerly through `step()`
    _steps = property(lambda self: self.recording.steps)                        # passes launched so far

    def close(self):
        """Detach the process-wide dropout base again (eager trainers of the same process go back to torch's generator offsets)."""
        if self._drop_base is not None:
            ops.dropout_offset_base(None)
            self._drop_base = None

    @staticmethod
    def _build_seqs(pl):
        """Host half of the sequence tables of attention layers (runs while the previous replay is still on the GPU)."""
        return PackedSeqs.build_host_pair(pl['table'], pl['nrow'], pl['longest'])

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

    def packed_seqs(self):
        """The trainer's `_sample`: views of the static sequence tables `_prepare` refreshed for this pass; None without attention layers."""
        return self.staging.packed_seqs()

    def target_subset(self):
        """The trainer's `_target_subset`: the constructor's draw (its size is every draw's) and the static device copies of the
        subset `_prepare` drew for this pass."""
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

    def log_node(self, keys, packed, host_items):
        """The trainer's `_log` of ONE pass: its device scalars into their slots of the static log buffer (`UpdateLog.write`)."""
        self._log_keys, self._log_items = keys, host_items
        self.log.write(keys, packed)

    def _record(self):
        """Record one pass as a list of (graph, exchange) segments; one segment unless the trainer cuts (data parallel)."""
        torch.cuda.synchronize(self.device)
        # No cyclic garbage collection while the stream captures: a dead CUDAGraph that only the collector can free (a dropped trainer or
        # GraphedUpdate sits in reference cycles) synchronises the device in its destructor on ROCm, which a capturing stream refuses - the
        # exception leaves a destructor and the process aborts.  Collect such garbage now and keep the collector off until the capture ends.
        gc.collect()
        torch.cuda.empty_cache()
        if self._capture_stream is None:
            self._capture_stream = torch.cuda.Stream(device=self.device)
        side = self._capture_stream
        side.wait_stream(torch.cuda.current_stream(self.device))
        rec = self._rec = dict(segs=[], g=torch.cuda.CUDAGraph())
        gc_was_on = gc.isenabled()
        gc.disable()
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
            if gc_was_on:
                gc.enable()
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        return dict(segs=rec['segs'], log_keys=self._log_keys, log_items=self._log_items)

    # ---- host side of one pass ------------------------------------------------------------------------------------------------
    def _prepare(self):
        """Host half of the pass at `self._pass` -> its graph key.  Sampling plan, then the REDQ subset - the order in which the eager
        loop draws them from numpy, pass by pass -, then the AdamW factors (the critic's every pass, the policy's only where the actor
        step is due), all through one staging slot."""
        alg, par, recording, st = self.alg, self.alg.parameter, self.recording, self.staging
        actor_due = alg._actor_due(*self._pass)       # part of the key: the two launch sequences are two graphs
        pl = alg.replay_buffer.plan_trajs_device(par.sac_batch_size, None, random_trunc_traj=par.random_trunc_traj,
                                                 nest_stack_trajs=alg.allow_nest_stack, buckets=recording.buckets == 'on',
                                                 randomize_mask=par.randomize_mask, valid_number_post_randomized=par.valid_number_post_randomized)
        seqs = self._drop_base is not None            # attention layers: the sequence tables of the batch, their sizes part of the exact key
        built = self._build_seqs(pl) if seqs else None
        if recording.buckets == 'auto':
            shapes = recording.tips(graph_key(pl, exact_table_key(built) if seqs else (), False, actor_due))
            if shapes:
                alg.logger(f'update graphs: {shapes} batch shapes in {recording.steps + 1} {"updates" if par.utd == 1 else "passes"} - batch shapes are bucketed from here on '
                           f'(RESEL_GRAPH_BUCKETS=0 keeps exact shapes)')
                pl = pad_plan(pl, alg.replay_buffer.max_traj_step)          # the plan that tipped the count is the first bucketed one
                built = self._build_seqs(pl) if seqs else None
        alg.replay_buffer._mirror(self.device)        # transitions pushed since the last update reach the device ring HERE, outside the graph
        n = pl['seg'].shape[0]
        if n > self.PLAN_CAPACITY:
            raise RuntimeError(f'GraphedUpdate: {n} plan segments exceed the static plan buffer ({self.PLAN_CAPACITY})')
        n_sel = pl['sel'].size if 'sel' in pl else 0
        if n_sel > self._sel_capacity:
            raise RuntimeError(f'GraphedUpdate: {n_sel} selection words exceed the static selection buffer ({self._sel_capacity})')
        bucketed, table_key = recording.buckets == 'on', ()
        slot = st.take()
        if built is not None:
            # padded: reachable with `seq_buckets` only
            built, table_key = pad_seq_tables(built, pl['nrow'], pl['longest']) if bucketed else (built, exact_table_key(built))
            if st.put_seqs(built, padded=bucketed):
                self.graphs.clear()
        # staged with numpy, not copy_: see PassStaging.put_seqs
        slot['plan'].numpy()[:n] = pl['seg']
        self._plan_dev[:n].copy_(slot['plan'][:n], non_blocking=True)        # stream-ordered: behind the previous pass's gather
        if n_sel:
            slot['sel'].numpy()[:n_sel] = pl['sel']
            self._sel_dev[:n_sel].copy_(slot['sel'][:n_sel], non_blocking=True)
        self._plan = pl
        sub = np.ascontiguousarray(np.asarray(alg._select_target_ensemble(self.E)), dtype=np.int32)
        slot['sub'].numpy()[...] = sub
        self.subset_i32.copy_(slot['sub'], non_blocking=True)
        self.subset_i64.copy_(self.subset_i32)
        for i, opt in enumerate((alg.optimizer_value, alg.optimizer_policy)):
            if i == 0 or actor_due:
                opt.prepare_step(slot['bc'][2 * i:2 * i + 2])
        return graph_key(pl, table_key, bucketed, actor_due)

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
                self._drop_base.add_(self.DROP_STRIDE)                       # a node: every replay moves the masks of the whole pass on
            with training_pass():
                alg._train_one_batch()                # below the eager entry's update-boundary work: `step()` does that itself
        finally:
            ops.DROP_OVERRIDE = None
            alg._graph = None
            for opt in (alg.optimizer_value, alg.optimizer_policy):
                opt.device_factors_active = False

    def step(self):
        """Exactly one `train_one_batch()`: `utd` passes (`_launch_pass`); the update-boundary work once, in front of the first pass; one
        log, read back once behind the last - it names the union of the keys the step's passes wrote."""
        if ops.amax_maintenance() or self._amax_generation != ops.AMAX_GENERATION[0]:
            self.graphs.clear()                       # the magnitude epochs started over: recorded kernel nodes carry epochs of the old generation
            self._amax_generation = ops.AMAX_GENERATION[0]
        alg = self.alg
        keys, items, actor_steps = {}, {}, 0
        for utd_idx in range(alg.parameter.utd):
            self._pass = (utd_idx, actor_steps)       # read by `_prepare` (the key, the AdamW factors) and by the trainer (`pass_position`)
            actor_steps += self._launch_pass()
            keys.update(dict.fromkeys(self._log_keys))                       # device scalars: merged in the log's device buffer, named here
            items.update(self._log_items)             # host entries: a later pass wins, an earlier one's survive (the eager loop's `host`)
        self._pass = (0, 0)
        pl = self._plan                               # the host entries of the LAST pass, as the eager `_log` takes them
        items.update(alg._host_log(pl['total_size'], pl.get('nrow_real', pl['nrow'])))
        return self.log.read_back(list(keys), items)

    def _launch_pass(self):
        """One pass, as the policy decides: replayed from its graph, launched eagerly (the same pass from the same static inputs) or
        recorded and then replayed.  -> did it run the actor step."""
        key = self._prepare()
        what, _ = self.recording.decide(key)
        if what in (REPLAY, RECORD):
            if what == RECORD:
                self.graphs[key] = self._record()
            g = self.graphs[key]
            self._log_keys, self._log_items = g['log_keys'], g['log_items']  # of THIS launch sequence (with / without the actor step)
            for seg, exchange in g['segs']:
                seg.replay()
                if exchange is not None:
                    exchange()                        # the gradient all-reduce, eagerly between two replays on the same stream
            if ops.AMAX_VERIFY:                       # the recorded pass contains the check kernels: read their verdict behind the replay
                ops.amax_verify_raise(self.device)
        else:
            self._body()
        self.staging.release()                        # behind the pass on the stream: its staging slot is free once this event has passed
        return key[-1]

    @property
    def graph(self):                                  # the most recently recorded graph (tests): its first segment
        return next(reversed(self.graphs.values()))['segs'][0][0] if self.graphs else None
