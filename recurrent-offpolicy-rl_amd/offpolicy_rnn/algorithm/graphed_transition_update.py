"""One `train_one_batch()` of a trainer whose passes are fixed-shape batches - the memoryless REDQ trainer
(algorithm/sac_mlp_redq_ensemble_q.py), the slice trainer (algorithm/sac_rnn_slice.py) - as `utd` hipGraph replays.

REDQ's usual setting is utd = 20 on a few hundred transitions: twenty launch-bound passes per environment step, each a few dozen small
kernels.  The captured unit is ONE pass of the `utd` loop (profiles/r17_utd_replay.md), in two recordings - with and without the actor
step - keyed on nothing else: the batch size is fixed.  A step is
    one H2D of a pinned block  [plans int32 [utd, words] | REDQ subsets int32 [utd, redq_m] | pass word (0) | AdamW factors fp32 [utd, 4]],
    `utd` replays, the two parameter norms of the log (launched once, behind the last pass), one D2H of the log block.
How a replay finds its slice: the PASS WORD, a device int32 inside that block.  The gather kernel reads its rows through it
(`ops.gather_transitions(pass_word=...)`), two `index_select`s by it fetch the pass's subset and bias corrections into the buffers the
target and the flat AdamW kernels read (`FlatAdamW._bc_dev`, the device factors of the full-trajectory graphs), and the last node of the
pass advances it with an ordinary add.  The host half of a step draws from numpy in the eager loop's order - per pass the rows, then the
subset - and counts the optimizer steps.  Actor noise inside a recording comes from torch's CUDA generator, which the capture registers:
graph-safe Philox offsets, fresh numbers on every replay.  The recording policy (warm-up passes, record on the second occurrence) and the
log's slots and read-back are those of the full-trajectory driver (graph_policy.py, graph_staging.py).  Recorded kernel nodes carry
magnitude epochs: when `ops.amax_maintenance()` starts a new generation at a step boundary, the recordings are dropped and made again.

What the trainer supplies: `graph_plan_words()` (int32 words of one pass's plan: `batch` rows for the REDQ trainer, `2 * batch` for
the slice trainer's (row, valid rows) pairs), `graph_plan_pass()` (one pass's plan, drawn as the eager pass draws it), `graph_gather(ring,
table [utd, words], pass word)`, `graph_subset_size()` (0: the trainer has no REDQ subset, and the block has no subset part) with
`num_ensemble` when it is not 0, and `graph_optimizers()` -> (those the critic step advances, those the actor step advances)."""
import gc

import numpy as np
import torch

from ..hip import ops
from ..models.rnn_base import training_pass
from ..utility.deferred_log import ScalarLog
from .graph_policy import RECORD, REPLAY, RecordingPolicy
from .graph_staging import RING, UpdateLog


class GraphedTransitionUpdate:
    LOG_SLOTS = 32

    @staticmethod
    def refusal(alg):
        """Why `train()` launches this trainer's updates eagerly (None: they are replayed)."""
        if not getattr(alg, 'transition_level', False):
            return 'not a transition-level trainer'
        if alg.device.type != 'cuda':
            return 'needs a GPU'
        return None

    @staticmethod
    def pass_schedule(alg):
        """The actor flags of the passes of one `train_one_batch()`, obtained by walking the trainer's `_actor_due` as its loop does."""
        flags = []
        for utd_idx in range(alg.parameter.utd):
            flags.append(bool(alg._actor_due(utd_idx, sum(flags))))
        return flags

    def __init__(self, alg, warmup=3):
        why = self.refusal(alg)
        if why:
            raise RuntimeError('GraphedTransitionUpdate: ' + why)
        par = alg.parameter
        if par.utd < 1:
            raise ValueError(f'GraphedTransitionUpdate: utd={par.utd} (an update is at least one pass)')
        self.alg, self.device = alg, alg.device
        self.utd, self.words, self.m = int(par.utd), int(alg.graph_plan_words()), int(alg.graph_subset_size())
        n_rows, n_sub = self.utd * self.words, self.utd * self.m
        words = n_rows + n_sub + 1 + 4 * self.utd
        self._block = torch.zeros(words, dtype=torch.int32, device=self.device)
        self.rows_dev = self._block[:n_rows].view(self.utd, self.words)
        self.sub_dev = self._block[n_rows:n_rows + n_sub].view(self.utd, self.m)
        self.pass_word = self._block[n_rows + n_sub:n_rows + n_sub + 1]
        self.bc_dev = self._block[n_rows + n_sub + 1:].view(torch.float32).view(self.utd, 4)
        self._ring = [dict(host=torch.zeros(words, dtype=torch.int32).pin_memory(), evt=torch.cuda.Event(), used=False) for _ in range(RING)]
        self._turn = 0
        self.subset_i32 = torch.zeros(self.m, dtype=torch.int32, device=self.device)      # this pass's subset, as the target reads it
        self.subset_i64 = torch.zeros(self.m, dtype=torch.int64, device=self.device)      # ... and as `member_index`
        self.critic_opts, self.actor_opts = alg.graph_optimizers()
        for opt in self.critic_opts + self.actor_opts:
            opt.enable_device_factors()
        self.log = UpdateLog(self.LOG_SLOTS, self.device, log_cls=ScalarLog)
        self.recording = RecordingPolicy(warmup, None, 'off', sequences=max(1, len(set(self.pass_schedule(alg)))))
        self.graphs = self.recording.recorded         # (actor step due,) -> dict(graph, log_keys)
        self._pass = (0, 0)
        self._log_keys = None
        self._ring_dev = None                         # the ring's device mirror the recordings read
        self._amax_generation = ops.AMAX_GENERATION[0]
        self._pool = torch.cuda.graph_pool_handle()
        self._capture_stream = None

    eager_fallbacks = property(lambda self: self.recording.eager_fallbacks)     # passes launched eagerly through `step()`

    def close(self):
        pass

    # ---- called by the trainer while `alg._graph is self` -------------------------------------------------------------------
    def pass_position(self):
        return self._pass

    def gather(self):
        return self.alg.graph_gather(self._ring_dev, self.rows_dev, self.pass_word)

    def target_subset(self):
        return self.subset_i32, self.subset_i64

    def log_node(self, keys, packed):
        self._log_keys = keys
        self.log.write(keys, packed)

    # ---- host side of one step ------------------------------------------------------------------------------------------------
    def _prepare(self, schedule):
        """Host half of a whole step into one pinned block, then ONE stream-ordered copy.  numpy draws in the eager loop's order."""
        alg = self.alg
        ring_dev = alg.replay_buffer._mirror(self.device)        # transitions pushed since the last update reach the device ring HERE
        if self._ring_dev is None or ring_dev.data_ptr() != self._ring_dev.data_ptr() or ring_dev.shape != self._ring_dev.shape:
            self.graphs.clear()                       # recorded gathers hold the old mirror's address
            self._ring_dev = ring_dev
        slot = self._slot = self._ring[self._turn % RING]
        self._turn += 1
        if slot['used']:
            slot['evt'].synchronize()
        host = slot['host'].numpy()
        n_rows, n_sub = self.utd * self.words, self.utd * self.m
        rows, sub = host[:n_rows].reshape(self.utd, self.words), host[n_rows:n_rows + n_sub].reshape(self.utd, self.m)
        bc = host[n_rows + n_sub + 1:].view(np.float32).reshape(self.utd, 4)
        for p, actor_due in enumerate(schedule):
            rows[p] = alg.graph_plan_pass()
            if self.m:
                sub[p] = np.random.permutation(alg.num_ensemble)[:self.m]
            for i, opts in enumerate((self.critic_opts, self.actor_opts)):
                if i == 0 or actor_due:
                    for opt in opts:                  # (the optimizers of one step count together: one pair of factors serves them)
                        opt.step_count += 1
                    bc[p, 2 * i:2 * i + 2] = ops.adamw_bias_corrections(opts[0].betas[0], opts[0].betas[1], opts[0].step_count)
        host[n_rows + n_sub] = 0                      # the pass word starts every step at pass 0
        self._block.copy_(slot['host'], non_blocking=True)

    def _body(self):
        alg = self.alg
        opts = self.critic_opts + self.actor_opts
        alg._graph = self
        for opt in opts:
            opt.device_factors_active = True
        try:
            ops.amax_arena_zero(self.device)          # first node: a replay publishes operand magnitudes into the slots / epochs baked into the graph
            # this pass's slice of the step's tables, through the pass word
            if self.m:
                self.subset_i32.copy_(self.sub_dev.index_select(0, self.pass_word).view(-1))
                self.subset_i64.copy_(self.subset_i32)
            bc = self.bc_dev.index_select(0, self.pass_word).view(-1)
            for opt in self.critic_opts:
                opt._bc_dev.copy_(bc[0:2])
            if alg._actor_due(*self._pass):
                for opt in self.actor_opts:
                    opt._bc_dev.copy_(bc[2:4])
            with training_pass():
                alg._train_one_batch()
            self.pass_word.add_(1)                    # last node: the next replay serves the next pass
        finally:
            alg._graph = None
            for opt in opts:
                opt.device_factors_active = False

    def _record(self):
        torch.cuda.synchronize(self.device)
        # no cyclic garbage collection while the stream captures (see GraphedUpdate._record)
        gc.collect()
        torch.cuda.empty_cache()
        if self._capture_stream is None:
            self._capture_stream = torch.cuda.Stream(device=self.device)
        side = self._capture_stream
        side.wait_stream(torch.cuda.current_stream(self.device))
        graph = torch.cuda.CUDAGraph()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(side):
                graph.capture_begin(pool=self._pool)
                try:
                    self._body()                      # recorded, not run: the replay that follows consumes the prepared inputs
                finally:
                    graph.capture_end()
        finally:
            if gc_was_on:
                gc.enable()
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        return dict(graph=graph, log_keys=self._log_keys)

    def step(self):
        """Exactly one `train_one_batch()`: one H2D, `utd` passes, the norms, one D2H of the log."""
        if ops.amax_maintenance() or self._amax_generation != ops.AMAX_GENERATION[0]:
            self.graphs.clear()                       # the magnitude epochs started over: recorded kernel nodes carry epochs of the old generation
            self._amax_generation = ops.AMAX_GENERATION[0]
        alg = self.alg
        schedule = self.pass_schedule(alg)
        self._prepare(schedule)
        keys, actor_steps = {}, 0
        for utd_idx, actor_due in enumerate(schedule):
            self._pass = (utd_idx, actor_steps)
            key = (actor_due,)
            what, _ = self.recording.decide(key)
            if what in (REPLAY, RECORD):
                if what == RECORD:
                    self.graphs[key] = self._record()
                g = self.graphs[key]
                self._log_keys = g['log_keys']
                g['graph'].replay()
                if ops.AMAX_VERIFY:
                    ops.amax_verify_raise(self.device)
            else:
                self._body()
            keys.update(dict.fromkeys(self._log_keys))
            actor_steps += actor_due
        self._pass = (0, 0)
        self._slot['evt'].record()                    # behind the step on the stream: its block is free once this event has passed
        self._slot['used'] = True
        norm_keys, packed = alg._pack(alg._norm_scalars())
        self.log.write(norm_keys, packed)
        keys.update(dict.fromkeys(norm_keys))
        return self.log.read_back(list(keys), {})
