"""Full-trajectory recurrent SAC with an ensemble critic: `train_one_batch()` - THE hot path
(reference offpolicy_rnn/algorithm/sac_full_length_rnn_ensembleQ.py:297-467).

Same contract (no arguments, returns the log dict with the reference's keys, `grad_num` gates the actor step) and the
same arithmetic per update:
    sample packed trajectories -> [no grad] actor + target critics on (s', s, a) -> REDQ / min target with the
    Q-guard clamp -> critic step -> soft target update -> actor step (+ alpha step) on the live critics.
What is organised differently for the MI355X:
  * the sampled batch crosses PCIe ONCE as a single fp32 array (all fields, validity and the derived reset /
    validity flags are columns of it); field tensors are column views on the device;
  * target, Q-guard state and the running extrema stay on the device (`ops.sac_target`);
  * losses are back-propagated as masked SUMS; the 1 / valid_num normalisation is applied inside the flat AdamW
    kernel from a device scalar that rides in the gradient buffer - which is what makes the data-parallel version a
    single all-reduce (parallel/data_parallel.py) with a global normalisation identical to the reference's;
  * the actor step back-propagates only into the actor (`backward(inputs=...)`), skipping the critic weight gradients
    that the reference computes and throws away;
  * every scalar of the log dict is gathered on the device and fetched with one transfer at the end.
"""
from typing import Dict

import contextlib
import functools
import itertools
import math
import os

import numpy as np
import torch

from ..buffers.transition_buffer.nested_replay_memory import NestedMemoryArray as NestedTransitionMemoryArray
from ..buffers.transition_buffer.shape_buckets import NO_SEQ_BUCKETS, pad_seq_tables
from ..hip import ops
from ..models.contextual_model import ContextualModel
from ..models.ensemble_linear_model import EnsembleLinear
from ..models.flash_attention.TransformerFlashAttention import PackedSeqs
from ..models.rnn_base import training_pass
from ..parallel.data_parallel import GradSync
from ..policy_value_models.make_models import make_policy_model
from ..utility.deferred_log import DeferredLog
from ..utility.pinned import PinnedRing
from ..utility.q_value_guard import QValueGuard
from .sac import SAC

FIELDS = ('state', 'last_state', 'action', 'last_action', 'next_state', 'done', 'mask', 'reward', 'reward_input', 'timeout', 'start')


@contextlib.contextmanager
def _frozen_parameters(model):
    params = [p for p in model.parameters() if p.requires_grad]
    for p in params:
        p.requires_grad_(False)
    try:
        yield
    finally:
        for p in params:
            p.requires_grad_(True)


@contextlib.contextmanager
def _ensemble_subset(model, member_index):
    layers = [l for l in model.uni_network.layer_list if isinstance(l, EnsembleLinear)]
    for l in layers:
        l.member_index = member_index
    try:
        yield
    finally:
        for l in layers:
            l.member_index = None


class SACFullLengthRNNEnsembleQ(SAC):
    def __init__(self, parameter):
        super().__init__(parameter)
        assert self.parameter.value_net_num == 1
        for item in self.parameter.value_layer_type:
            assert item.startswith('e'), 'the critic MLP must be an ensemble (efc-<E>) stack'
        for net in (self.values[0].embedding_network.layer_list + self.target_values[0].embedding_network.layer_list
                    + self.values[0].uni_network.layer_list + self.target_values[0].uni_network.layer_list):
            if hasattr(net, 'desire_ndim'):
                net.desire_ndim = 4
            if hasattr(net, 'in_proj') and hasattr(net.in_proj, 'desire_ndim'):
                net.in_proj.desire_ndim = 4
        self.logger(f'replay buffer skip len: {self._get_skip_len()}')
        self.replay_buffer = NestedTransitionMemoryArray(self.parameter.max_buffer_transition_num, self.env_info['max_trajectory_len'],
                                                         additional_history_len=self._get_skip_len())
        self.Q_guard = QValueGuard(guard_min=True, guard_max=True, decay_ratio=1.0 if self.discrete_env else 1 - 1e-3,
                                   device=self.device)
        # kept for API parity: built, hard-copied, never updated; only the non-REDQ TD3 trainer reads it
        self.target_policy = make_policy_model(self.policy_args, self.base_algorithm, self.discrete_env)
        self.target_policy.to(self.device)
        self.target_policy.copy_weight_from(self.policy, tau=0.0)
        self.target_policy.eval()
        self.grad_sync = GradSync()
        self._graph = None                             # set while a captured update is being recorded / replayed (graphed_update.py)
        # eager updates pad their batch into its shape bucket (shape_buckets.py; tests, tools).  Device replay ring only, and not with
        # attention layers unless `seq_buckets` is set as well (then `_packed_seqs` pads their sequence tables into buckets,
        # shape_buckets.pad_seq_tables, and the decoder takes its padded path): `_sample` raises otherwise
        self.shape_buckets = False
        self.seq_buckets = False
        self._subset_rng = None                        # REDQ subset stream: None = numpy's global stream (see _subset_stream)
        self._pinned = PinnedRing(torch.float32)       # staging blocks of the host-built batch (one event per block)
        self._needs_seq_table = any(kind.packs_sequences for kind, _ in self._sequence_layers())
        self._stats = torch.zeros(2, dtype=torch.float32, device=self.device)
        self._planar_idx = {}                          # (flag names, device) -> their column indices on the device (_batch_views)
        self._subset_tables, self._subset_cache = {}, {}     # device copies of critic-subset index vectors (_subset_on_device)
        self._guard_ext = None                         # data parallel: this rank's Q-guard extrema on their way into the critic's gradient bucket
        self._guard_ext_fresh = False                  # ... written by this update's target and not yet exchanged (_guard_exchange, _finish_step)
        self.share_policy_pass = self._policy_pass_shareable()
        # RESEL_GRU_BATCH (default on): the independent embedding passes of a phase (latency-bound gru value embeddings) walk their towers
        # in lockstep and their recurrences share ONE launch (ContextualModel.prefetch_embeddings).  0: serial, one recurrence after
        # another.  Both forms are launch sequences on the current stream.  Not with a shared policy pass: that pass records an autograd
        # graph inside the target computation.
        self.gru_batch = (self.device.type == 'cuda' and os.environ.get('RESEL_GRU_BATCH', '1') != '0' and not self.discrete_env
                          and any(kind.deferred for kind, _ in self.values[0].embedding_network.sequence_layers())
                          and not self.share_policy_pass)

    step = property(lambda self: self.train_one_batch)          # north_star's "algorithm.step()" alias
    device_replay = True        # keep a device mirror of the replay ring and assemble sampled batches on the GPU (CUDA only)
    defer_log = False           # True: the log's device scalars stay in flight until first read (DeferredLog); False: floats on return, as the reference

    def _get_skip_len(self):
        return max((kind.context_len(layer) for kind, layer in self._sequence_layers()), default=0) + 1

    def _policy_pass_shareable(self) -> bool:
        """The target pass evaluates the policy on (s', s, a): the SAME token sequence as the actor pass on (s, s_prev,
        a_prev), one slot earlier (that is what the pre-step slot and the `total_*` flags of the reference build,
        sac_full_length_rnn_ensembleQ.py:338-378), with the SAME parameters (the actor is updated after both).  When every
        layer's output at a token depends only on the tokens of its own trajectory - pointwise layers and sequence layers
        that reset / mask at the trajectory start (`honours_start`; cgpt attends inside per-trajectory segments whose table is
        shifted with the tokens, `target_attention_mask`, reference :358-366) - the actor pass is the target pass shifted by one slot, so ONE policy
        forward (with a graph) serves both and the second is skipped.  Not for `gru` (no reset: the leading padding slots
        differ between the two passes), layers with active dropout (`cgpt_*_p0.1`), the TD3 trainer that smooths a frozen target policy, discrete heads,
        RESEL_SHARE_POLICY_PASS=0."""
        if os.environ.get('RESEL_SHARE_POLICY_PASS', '1') == '0' or self.discrete_env or not self.target_from_live_policy:
            return False
        if self.parameter.randomize_first_hidden:        # the two passes would start from two different random states
            return False
        if type(self)._next_action is not SACFullLengthRNNEnsembleQ._next_action:
            return False
        if self.base_algorithm not in ('sac', 'td3'):
            return False
        if not all(kind.honours_start for kind, _ in self._sequence_layers((self.policy,))):
            return False
        return not any(isinstance(m, torch.nn.Dropout) and m.p > 0 for mod in self.policy.contextual_modules.values() for m in mod.modules())

    # ------------------------------------------------------------------------------------------ batch
    def _upload_batch(self, batch, valid, table):
        """Host fix-ups + ONE host->device copy.  Returns dict of device views."""
        arr = self.replay_buffer._last_batch_array                   # (rows, T', W) fp32: every field is a column range
        rows, T, W = arr.shape
        R = self.replay_buffer.name2range
        need = rows * T * (W + 3)
        staged = self._pinned.stage(need, self.device, rows * self.replay_buffer.max_traj_step * (W + 3)).view(rows, T, W + 3)
        host = staged.numpy()
        host[..., :W] = arr
        start = arr[..., R['start'][0]]
        v = valid[..., 0]
        # flag surgery (reference :338-342): the target pass sees the slot before each sequence as valid / not-start
        tv = v.copy()
        tv[:, :-1][np.diff(v, axis=1) == 1] = 1
        ts = start.copy()
        ts[:, :-1][np.diff(start, axis=1) == -1] = 0
        host[..., W], host[..., W + 1], host[..., W + 2] = v, tv, ts
        d0, t0 = R['done'][0], R['timeout'][0]
        host[..., d0][arr[..., t0] > 0] = 0                          # time-limit terminations bootstrap
        dev = self._pinned.upload(staged, self.device)
        return self._batch_views(dev, self._packed_seqs(table, rows, T))

    def _packed_seqs(self, table, rows, T):
        """Eager updates: the per-row sequence-length table (reference :358-366) as the pair of device descriptions attention layers
        consume - the batch and its one-slot shift; None for every other layer.  Built on the host (the table is host data anyway): token
        indices + cu_seqlens for the var-len attention kernel."""
        if not self._needs_seq_table:
            return None
        built = PackedSeqs.build_host_pair(table, rows, T)
        padded = self.shape_buckets and self.seq_buckets
        if padded:
            built, _ = pad_seq_tables(built, rows, T)
        return [PackedSeqs.from_static(torch.from_numpy(idx).to(self.device), torch.from_numpy(cu).to(self.device), mx, tb, padded=padded)
                for idx, cu, mx, tb in built]

    def _batch_views(self, dev, seqs):
        """Field / flag views of the device batch array (rows, T', W + 3); `seqs`: the pair of `PackedSeqs` of the batch and of its
        one-slot shift (attention layers only), or None."""
        rows, T = dev.shape[:2]
        W = dev.shape[2] - 3
        R = self.replay_buffer.name2range
        out = {name: dev[..., R[name][0]:R[name][1]] for name in FIELDS}
        out['valid'], out['total_valid'], out['total_start'] = dev[..., W:W + 1], dev[..., W + 1:W + 2], dev[..., W + 2:W + 3]
        # the per-token scalars (flags, reward, done ...) as ONE planar [k, rows, T] copy: every kernel that takes them wants a dense
        # [rows * T] vector, and as column views of the batch array (stride W + 3) each use made its own contiguous copy - 24 small
        # launches per update
        ones = [n for n in out if out[n].shape[-1] == 1]
        if ones and dev.is_cuda:
            key = (tuple(ones), dev.device)
            idx = self._planar_idx.get(key)
            if idx is None:
                cols = [R[n][0] if n in R else {'valid': W, 'total_valid': W + 1, 'total_start': W + 2}[n] for n in ones]
                idx = self._planar_idx[key] = torch.tensor(cols, dtype=torch.int64, device=dev.device)
            planar = dev.view(rows * T, W + 3).index_select(1, idx).t().contiguous()          # [k, rows * T]
            for i, n in enumerate(ones):
                out[n] = planar[i].view(rows, T, 1)
        out['attention_mask'], out['target_attention_mask'] = seqs or (None, None)
        return out

    def _make_hidden(self, model, rows, start, mask, attn):
        if self.parameter.randomize_first_hidden:
            h = model.make_rnd_init_state(rows, device=self.device)
        else:
            h = model.make_init_state(rows, device=self.device)
        h.set_rnn_start(start)
        h.set_mask(mask)
        h.set_attention_concat_mask(attn)
        return h

    # ------------------------------------------------------------------------------------------ target
    target_from_live_policy = True        # (the non-REDQ TD3 trainer evaluates its frozen target policy instead)

    def _next_action(self, b, hidden):
        """(a', log pi(a'|s')) on the shifted inputs (s', s, a)."""
        net = self.policy if self.target_from_live_policy else self.target_policy
        mean, _, sample, logp, _, _ = net.forward(b['next_state'], b['state'], b['action'], hidden, b['reward'])
        return self._target_action(mean, sample, logp)

    def _target_action(self, mean, sample, logp):
        """What the target uses from the policy head's (mean, sample, log-prob); TD3 trainers smooth the mean instead."""
        return sample, logp

    def _subset_on_device(self, subset: np.ndarray, num_ensemble: int = 0, as_long: bool = False) -> torch.Tensor:
        """int32 device copy of a critic-subset index vector without a per-update host->device copy (a pageable copy blocks
        the host until the launch queue has drained): all ordered subsets of that size are uploaded ONCE as a table
        (8 critics, REDQ pairs: 56 rows) and a row view is returned; oversized tables fall back to a per-subset cache."""
        sub = np.ascontiguousarray(subset, dtype=np.int32)
        m, E = int(sub.size), int(max(num_ensemble, sub.max() + 1))
        tables = self._subset_tables
        if (E, m) not in tables:
            rows = None
            if math.perm(E, m) <= 4096:
                perms = list(itertools.permutations(range(E), m))
                t32 = torch.tensor(perms, dtype=torch.int32).to(self.device)
                rows = ({p: i for i, p in enumerate(perms)}, t32, t32.long())
            tables[(E, m)] = rows
        rows = tables[(E, m)]
        if rows is not None and tuple(sub.tolist()) in rows[0]:
            return rows[2 if as_long else 1][rows[0][tuple(sub.tolist())]]
        cache = self._subset_cache
        key = (sub.tobytes(), as_long)
        if key not in cache:
            t = torch.from_numpy(sub.copy()).to(self.device)
            cache[key] = t.long() if as_long else t
        return cache[key]

    def _select_target_ensemble(self, num_ensemble: int) -> np.ndarray:
        return np.arange(num_ensemble)                               # plain ensemble-min (REDQ trainers override)

    def _subset_stream(self):
        """numpy stream of the REDQ subset draws.  One process: the global stream, draw for draw as the reference.  Data parallel:
        a dedicated stream seeded identically on every rank (`parameter.seed`), so that all ranks take the minimum over the
        SAME critics while each samples its own rows from its own global stream - the update then equals the single-process
        update over the global batch (tests/test_data_parallel*.py)."""
        if self.grad_sync.active and self._subset_rng is None:
            self._subset_rng = np.random.RandomState(int(self.parameter.seed) + 7919)
        return self._subset_rng if self._subset_rng is not None else np.random

    def _guard_exchange(self):
        """Data parallel: the Q-guard sees the extrema of the GLOBAL batch.  Default: no collective of its own - the rank-local
        extrema ride in the critic's gradient bucket (`_finish_step`) and reach the guard behind that all-reduce; the guard of the
        reference acts on the NEXT update's target only (utility/q_value_guard.py:22-38), so this is the single-process guard, not
        an approximation.  RESEL_DP_GUARD=allreduce keeps the three-phase form with two 2-float MAX all-reduces inside the target."""
        if not self.grad_sync.active:
            return {}
        if os.environ.get('RESEL_DP_GUARD', 'bucket') == 'allreduce':
            return dict(reduce_max=self.grad_sync.all_reduce_max_)
        if self._guard_ext is None or self._guard_ext.device != self.Q_guard.state.device:
            self._guard_ext = torch.zeros(4, dtype=torch.float32, device=self.Q_guard.state.device)
        self._guard_ext_fresh = True
        return dict(local_ext=self._guard_ext)

    def _target_subset(self, num_ensemble: int):
        """The critics this update's target takes its minimum over -> (host index vector: its SIZE decides whether all members are
        evaluated, `index(as_long=False)`: the drawn indices on the device)."""
        if self._graph is not None:                    # captured update: drawn by GraphedUpdate._prepare into static buffers, no draw here
            return self._graph.target_subset()
        subset = np.asarray(self._select_target_ensemble(num_ensemble))
        return subset, functools.partial(self._subset_on_device, subset, num_ensemble)

    def _target_critics(self, b, action, sample, hidden):
        """Q'(s', a') of the drawn target critics -> (q, index).  REDQ (fewer drawn than there are): only those are evaluated (same
        numbers: the others were never used), q holds them in draw order and `index` is None; otherwise q holds every member and
        `index` (`_target_subset`) names the drawn ones."""
        tv = self.target_values[0]
        subset, index = self._target_subset(tv.uni_network.layer_list[-1].num_ensemble)
        # (an `eln-E` norm or an ensemble sequence layer, in the head or in the context encoder, couples the members: every one of them is
        # evaluated, the drawn ones are picked from q as in the reference)
        coupled = tv.uni_network.members_coupled() or tv.embedding_network.emits_member_axis()
        if subset.size < tv.uni_network.layer_list[-1].num_ensemble and not coupled:
            with _ensemble_subset(tv, index(as_long=True)):
                return tv.forward(b['next_state'], b['state'], action, sample, hidden, b['reward'])[0], None
        return tv.forward(b['next_state'], b['state'], action, sample, hidden, b['reward'])[0], index

    def _target_Q_discrete(self, b, policy_hidden, target_hiddens, stats):
        """Discrete-action target (reference sac_full_length_rnn_redq.py:52-72): V(s') = sum_a pi(a|s') (min_subset Q'(s', a) -
        alpha log pi(a|s')); the last action enters the networks as a one-hot vector.  Guard clamp / update, done masking
        and the batch statistics go through the same fused kernel as the continuous target (one pseudo-critic, no log-prob)."""
        with torch.no_grad():
            onehot = self.policy.action2onehot(b['action'])
            _, _, sample, logp, _, _ = self.policy.forward(b['next_state'], b['state'], onehot, policy_hidden, b['reward'])
            q, index = self._target_critics(b, onehot, sample, target_hiddens[0])
            if ops.discrete_fused(q):                   # minimum over the drawn members, entropy term and expectation in one kernel
                v = ops.discrete_value(q, None if index is None else index(), logp, self.log_sac_alpha.detach())
            else:
                if index is not None:
                    q = q[index(as_long=True)]
                alpha = self.log_sac_alpha.detach().exp()
                v = ((q.min(dim=0).values - alpha * logp) * logp.exp()).sum(dim=-1, keepdim=True)
            return ops.sac_target(v.unsqueeze(0).contiguous(), self._subset_on_device(np.arange(1), 1), None, self.log_sac_alpha.detach(),
                                  b['reward'], b['done'], b['mask'], self.parameter.gamma, self.Q_guard.state, stats, **self._guard_exchange())

    def get_target_Q(self, b, policy_hidden, target_hiddens, stats, share_policy_pass=False):
        """-> (target, the policy's head outputs on (s', s, a) WITH a graph for the actor step to reuse one slot later - None unless
        `share_policy_pass`)."""
        if self.discrete_env:
            return self._target_Q_discrete(b, policy_hidden, target_hiddens, stats), None
        shared_out = None
        if share_policy_pass:
            with torch.enable_grad():           # one policy forward with a graph: the actor step reuses it one slot later
                emb_in = self.policy.get_embedding_input(b['next_state'], b['state'], b['action'], b['reward'])
                shared_out = self.policy.meta_forward(emb_in, b['next_state'], policy_hidden, False)[0]
        with torch.no_grad():
            if shared_out is not None:          # same head, same random draws as policy.forward would make
                sample, logp = self._target_action(*self.policy.process_model_out(shared_out.detach()))
            else:
                sample, logp = self._next_action(b, policy_hidden)
            q, index = self._target_critics(b, b['action'], sample, target_hiddens[0])
            idx = self._subset_on_device(np.arange(q.shape[0]), q.shape[0]) if index is None else index()
            target = ops.sac_target(q, idx, logp if self.base_algorithm == 'sac' else None, self.log_sac_alpha.detach(), b['reward'],
                                    b['done'], b['mask'], self.parameter.gamma, self.Q_guard.state, stats, **self._guard_exchange())
        return target, shared_out

    # ------------------------------------------------------------------------------------------ losses
    actor_q_reduce = 'min'                           # how the actor objective reduces the critics (REDQ trainers: 'mean'); names the fused kernel's mode

    def _q_for_policy(self, qs: torch.Tensor) -> torch.Tensor:
        return qs.min(dim=0).values if self.actor_q_reduce == 'min' else qs.mean(dim=0)

    def _actor_objective(self, alpha, logp, q_pi):
        return alpha * logp - q_pi                                   # (TD3 trainers drop the entropy term)

    def _clip(self, store, model, max_norm, emb_max, scale):
        """Optional gradient clipping on the *normalised* gradient (reference :239-250, 274-287).  Nothing here reads a device value on
        the host: the norm stays a device scalar (it joins the log's packed scalars), so a clipped update is capturable."""
        gnorm = 0.0
        if max_norm is None and emb_max is None:
            return gnorm
        if emb_max is None and store.grad.is_cuda:
            # norm clipping alone rewrites nothing: ||g / count|| = scale * sqrt(sum g^2) from ONE read of the flat buffer, and the
            # coefficient min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_) is folded into the scale word AdamW reads
            gnorm = ops.sumsq(store.grad[:store.numel]).sqrt_().mul_(scale)
            scale.mul_((max_norm / (gnorm + 1e-6)).clamp_(max=1.0))
            return gnorm[0]
        store.grad[:store.numel].mul_(scale)
        scale.fill_(1.0)
        if max_norm is not None:
            gnorm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm, norm_type=2)
        if emb_max is not None:
            torch.nn.utils.clip_grad_value_(model.embedding_network.parameters(), emb_max)
            for layer in model.embedding_network.layer_list:
                for sub in getattr(layer, 'layers', []):
                    if hasattr(sub, 'mixer'):
                        torch.nn.utils.clip_grad_value_([sub.mixer.A_log], 1e-3)
            gnorm = 0.0
        return gnorm

    def _finish_step(self, optimizer, store, local_count, overlap=None, guard=False):
        """Exchange (sum) the flat gradient + the local valid count, then AdamW with grad / global count.  Data parallel: the
        all-reduce is issued on the exchange stream as soon as the last gradient is in the flat buffer; `overlap()` (work
        that does not touch the gradient buffer: the step's log scalars) runs on the compute stream meanwhile, which
        joins before anything reads the reduced buffer."""
        store.collect_grads()
        gs = self.grad_sync
        guard_slots = gs.active and guard and self._guard_ext_fresh
        if guard_slots:                                # this rank's row of the [world][4] extrema block behind the four standing slots
            store.ensure_grad_extra(4 + 4 * gs.world)
            o = store.numel + 4 + 4 * gs.rank
            store.grad[o:o + 4] = self._guard_ext
        store.grad[store.numel] = local_count
        if gs.active and self._graph is not None:
            # captured update: the recording is CUT here - the exchange runs eagerly between two graph replays (any backend, gloo included)
            if overlap is not None:
                overlap()
            grad = store.grad
            self._graph.cut(lambda: gs.all_reduce_(grad))
        else:
            gs.all_reduce_async_(store.grad)
            if overlap is not None:
                overlap()
            gs.wait()
        if guard_slots:                                # every rank's extrema are here: initialise / update the guard from the global batch
            ops.guard_apply_slots(store.grad[store.numel + 4:store.numel + 4 + 4 * gs.world], gs.world, self.Q_guard.state)
            self._guard_ext_fresh = False
        return 1.0 / store.grad[store.numel:store.numel + 1]

    # ------------------------------------------------------------------------------------------ the update
    def train_one_batch(self) -> Dict:
        with training_pass():                                    # no pass of an update reads the per-layer output sequences (rnn_base.py)
            if self.device.type == 'cuda':
                ops.amax_maintenance()                           # update boundary: the magnitude epochs may start over here (hip/ops.py)
            log = self._train_one_batch()
            if ops.AMAX_VERIFY and self.device.type == 'cuda':   # RESEL_AMAX_VERIFY=1: every mode-2 product of this update had its handles checked
                ops.amax_verify_raise(self.device)
            return log

    def _train_one_batch(self) -> Dict:
        """One update: `utd` passes (`_one_pass`) -> log.  Entered by the eager `train_one_batch` and, while a GraphedUpdate records or
        launches a pass from its static inputs, by its `_body`: the captured unit is ONE pass - the driver walks the `utd` loop itself and
        hands over where in it this pass stands (`pass_position`); the pass's log goes into the graph's static buffer (`log_node`)."""
        par = self.parameter
        self.policy.to(self.device)
        self.optimizer_policy.to(self.device)
        scal: Dict[str, torch.Tensor] = {}
        host: Dict[str, float] = {}
        if self._graph is not None:
            _, batch_size, real_rows = self._one_pass(*self._graph.pass_position(), scal, host)
        else:
            actor_steps = 0
            for utd_idx in range(par.utd):
                stepped, batch_size, real_rows = self._one_pass(utd_idx, actor_steps, scal, host)
                actor_steps += stepped
        self.policy.to(self.sample_device)
        return self._log(scal, host, batch_size, real_rows)

    def _one_pass(self, utd_idx, actor_steps, scal, host):
        """Pass `utd_idx` of an update, `actor_steps` actor steps into it: sample -> hidden states -> target -> critic step -> soft update ->
        actor step (if due).  Fills `scal` / `host`; -> (did the actor step run, transitions drawn, rows drawn)."""
        par = self.parameter
        b, batch_size, real_rows = self._sample()
        hidden = self._hidden_states(b)
        alpha_detach = self.log_sac_alpha.exp().detach()
        actor_due = self._actor_due(utd_idx, actor_steps)
        target_Q, shared_out = self._target(b, hidden, share_policy_pass=self.share_policy_pass and actor_due)
        valid_num = self._stats[1]
        self._critic_step(b, hidden, target_Q, valid_num, scal, host)
        self._value_update(tau=par.sac_tau)                      # soft target update: one kernel over the flat buffers
        self.values[0].eval()
        self.policy.train()
        if actor_due:
            self._actor_step(b, hidden, shared_out, alpha_detach, valid_num, scal, host)
        return bool(actor_due), batch_size, real_rows

    def _actor_due(self, utd_idx, done_so_far) -> bool:
        """Does the actor (+ alpha) step follow critic step `utd_idx` of this update, `done_so_far` actor steps into it (reference :450-452)?"""
        par = self.parameter
        return self.grad_num % par.policy_update_per == 0 and (utd_idx + 1) / par.utd * par.policy_utd > done_so_far

    def _sample(self):
        """One packed batch -> (its field views on the device, transitions drawn, rows drawn: fewer than the batch has only if bucketed)."""
        par = self.parameter
        self.timer.register_point(tag='sample_trajs', level=2)
        if self._graph is not None:
            # captured update (algorithm/graphed_update.py): the host half of the sampling ran before the replay, the plan sits in
            # static buffers; here only the device half is enqueued (a memcpy node + the gather kernel).  Sequence tables: built by
            # GraphedUpdate._prepare into pinned buffers; copy nodes + static device views
            dev, batch_size, real_rows = self._graph.gather()
            seqs = self._graph.packed_seqs()
        elif self.device_replay and self.device.type == 'cuda' and self.replay_buffer.device_supported(randomize_mask=par.randomize_mask):
            # device-resident ring: the host decides WHICH trajectories go where, the batch array is built on the GPU
            if self.shape_buckets and self._needs_seq_table and not self.seq_buckets:
                raise RuntimeError('shape_buckets: ' + NO_SEQ_BUCKETS)
            dev, batch_size, table = self.replay_buffer.sample_trajs_device(
                self.device, par.sac_batch_size, None, random_trunc_traj=par.random_trunc_traj, nest_stack_trajs=self.allow_nest_stack,
                buckets=self.shape_buckets, randomize_mask=par.randomize_mask, valid_number_post_randomized=par.valid_number_post_randomized)
            real_rows = self.replay_buffer._last_real_rows
            seqs = self._packed_seqs(table, *dev.shape[:2])
        else:
            if self.shape_buckets:
                raise RuntimeError('shape_buckets: only batches assembled from the device replay ring are bucketed')
            batch, batch_size, valid, table = self.replay_buffer.sample_trajs(
                par.sac_batch_size, None, randomize_mask=par.randomize_mask, valid_number_post_randomized=par.valid_number_post_randomized,
                equalize_data_of_each_traj=True, random_trunc_traj=par.random_trunc_traj, nest_stack_trajs=self.allow_nest_stack)
            self.timer.register_end(level=2)
            b = self._upload_batch(batch, valid, table)
            return b, batch_size, b['state'].shape[0]
        self.timer.register_end(level=2)
        return self._batch_views(dev, seqs), batch_size, real_rows or dev.shape[0]

    def _hidden_states(self, b):
        """Hidden states + side channels of the four passes; the target passes use the one-slot-earlier flags (reference :368-378)."""
        rows = b['state'].shape[0]
        value, target_value = self.values[0], self.target_values[0]
        return dict(target_policy=self._make_hidden(self.policy, rows, b['total_start'], b['total_valid'], b['target_attention_mask']),
                    target_value=self._make_hidden(target_value, rows, b['total_start'], b['total_valid'], b['target_attention_mask']),
                    value=self._make_hidden(value, rows, b['start'], b['valid'], b['attention_mask']),
                    policy=self._make_hidden(self.policy, rows, b['start'], b['valid'], b['attention_mask']))

    def _target(self, b, hidden, share_policy_pass):
        """Target (no grad); guard clamp/update + max|target| + sum(mask) happen inside the fused kernel -> `get_target_Q`'s pair."""
        value, target_value = self.values[0], self.target_values[0]
        self.policy.eval()
        if self.gru_batch:
            # latency-bound layers, one stream: the three embedding passes of this phase - (target) policy and target critic on the
            # shifted inputs without a graph, the critic with one - run in lockstep, their recurrences in ONE launch; the target
            # computation and the critic forward below pick their embeddings up
            value.train()
            shifted = (b['next_state'], b['state'], b['action'], b['reward'])
            ContextualModel.prefetch_embeddings([
                (self.policy if self.target_from_live_policy else self.target_policy, shifted, hidden['target_policy'], False),
                (target_value, shifted, hidden['target_value'], False),
                (value, (b['state'], b['last_state'], b['last_action'], b['reward_input']), hidden['value'], True)])
        return self.get_target_Q(b, hidden['target_policy'], [hidden['target_value']], self._stats, share_policy_pass)

    def _critic_step(self, b, hidden, target_Q, valid_num, scal, host):
        par, value, mask = self.parameter, self.values[0], b['mask']
        value.train()
        q = value.forward(b['state'], b['last_state'], b['last_action'], b['action'], hidden['value'], b['reward_input'])[0]
        taken_in_loss = self.discrete_env and ops.discrete_fused(q)
        if self.discrete_env and not taken_in_loss:             # Q of the action taken (reference :158)
            q = q.gather(-1, b['action'].long().unsqueeze(0).expand(q.shape[0], -1, -1, -1))
        if taken_in_loss:                                       # ... picked inside the loss kernels; dq comes back dense, no scatter
            q_loss_sum = ops.masked_q_taken_loss(q, b['action'], target_Q, mask)
        elif q.is_cuda and q.dtype == torch.float32:
            q_loss_sum = ops.masked_q_loss(q, target_Q, mask)         # one forward + one backward kernel (csrc/losses.hip; reference :105-114, :80-81)
        else:                                                   # CPU tensors keep the torch spelling
            q_loss_sum = ((q - target_Q.unsqueeze(0)).pow(2).sum(dim=0) * mask).sum()
        self.optimizer_value.zero_grad()
        q_loss_sum.backward()
        scale = self._finish_step(self.optimizer_value, value.store, valid_num, guard=True,
                                  overlap=lambda: scal.update(critic_loss=q_loss_sum.detach() / valid_num))
        q_grad_norm = self._clip(value.store, value, par.value_max_gradnorm, par.value_embedding_max_gradnorm, scale)
        self.optimizer_value.step(grad_scale=scale)
        host['value_grad_norm'] = q_grad_norm

    def _actor_step(self, b, hidden, shared_out, alpha_detach, valid_num, scal, host):
        """Actor (+ alpha) step on the live critics; `shared_out`: the target pass's head outputs (`get_target_Q`) or None."""
        par, value, mask = self.parameter, self.values[0], b['mask']
        if self.gru_batch:                                 # the actor's pass (with a graph) and the critic's embedding (without) together
            now = (b['state'], b['last_state'], b['last_action'], b['reward_input'])
            ContextualModel.prefetch_embeddings([(self.policy, now, hidden['policy'], True), (value, now, hidden['value'], False)])
        if shared_out is not None:                         # the target pass's head outputs, one slot later
            out2 = torch.nn.functional.pad(shared_out[:, :-1], (0, 0, 1, 0))
            action_mean, act_sample, log_prob = self.policy.process_model_out(out2)
        else:
            action_mean, _, act_sample, log_prob, _, _ = self.policy.forward(b['state'], b['last_state'], b['last_action'],
                                                                            hidden['policy'], b['reward_input'])
        act_in = act_sample if self.base_algorithm == 'sac' else action_mean
        # the actor objective differentiates Q only w.r.t. the action: the critic's parameters are frozen while its graph
        # is recorded, so that the backward does not form the critic weight gradients the reference computes and drops
        with _frozen_parameters(value):
            q_pi = value.forward(b['state'], b['last_state'], b['last_action'], act_in, hidden['value'], b['reward_input'],
                                 detach_embedding=True)[0]
        lp_sum = None
        if self.discrete_env and ops.discrete_fused(q_pi) and self.actor_q_reduce in ('min', 'mean'):
            # expectation over the action distribution (reference redq :85-86): both sums from one pass, d/dlogp from one more
            actor_sum, lp_sum = ops.masked_discrete_actor_loss(log_prob, q_pi, mask, self.log_sac_alpha, self.actor_q_reduce == 'min')
        elif self.discrete_env:
            objective = (self._actor_objective(alpha_detach, log_prob, self._q_for_policy(q_pi)) * log_prob.exp()).sum(dim=-1, keepdim=True)
            log_prob = (log_prob * log_prob.exp()).sum(dim=-1, keepdim=True)          # logged as -entropy (:425)
            actor_sum = (objective * mask).sum()
        elif q_pi.is_cuda and q_pi.dtype == torch.float32 and self.base_algorithm == 'sac' and self.actor_q_reduce in ('min', 'mean'):
            # sum mask (alpha logp - red_e Q) and sum mask logp from one pass, gradients from one more (reference redq :37-49)
            actor_sum, lp_sum = ops.masked_actor_loss(log_prob, q_pi, mask, self.log_sac_alpha, True, self.actor_q_reduce == 'min')
        else:                                               # CPU tensors, TD3: the torch spelling
            objective = self._actor_objective(alpha_detach, log_prob, self._q_for_policy(q_pi))
            actor_sum = (objective * mask).sum()
        if lp_sum is None:
            lp_sum = (log_prob.detach() * mask).sum()
        self.optimizer_policy.zero_grad()
        actor_sum.backward(inputs=self.policy.parameters())
        pstore = self.policy.store
        tune_alpha = not par.no_alpha_auto_tune
        if tune_alpha:     # d/d log_alpha of -sum(mask * log_alpha * (logp + H)) rides in the second spare slot
            pstore.grad[pstore.numel + 1] = -(lp_sum + self.target_entropy * valid_num)
        scale = self._finish_step(self.optimizer_policy, pstore, valid_num, overlap=lambda: scal.update(
            log_prob=lp_sum / valid_num, actor_loss=actor_sum.detach() / valid_num))
        pi_grad_norm = self._clip(pstore, self.policy, par.policy_max_gradnorm, par.policy_embedding_max_gradnorm, scale)
        self.optimizer_policy.step(grad_scale=scale)
        if tune_alpha:
            g_alpha = pstore.grad[pstore.numel + 1:pstore.numel + 2] / pstore.grad[pstore.numel:pstore.numel + 1]
            scal['alpha_loss'] = (self.log_sac_alpha.detach() * g_alpha)[0]
            self.log_sac_alpha.grad = g_alpha.clone()
            self.optimizer_alpha.step()
            with torch.no_grad():
                self.log_sac_alpha.clamp_max_(1)
        scal['policy_l2_norm_square'] = self.policy.l2_norm_square()
        host['policy_grad_norm'] = pi_grad_norm

    def _host_log(self, batch_size, real_rows):
        """The log entries that never were on the device (reference :455-467; no loss scaling here: fp32 / bf16 paths need none)."""
        return dict(real_batch_size=batch_size, real_batch_traj_num=real_rows,
                    average_traj_len=self.replay_buffer.size / len(self.replay_buffer), amp_scalar_pi=0, amp_scalar_q=0)

    def _log(self, scal, host, batch_size, real_rows):
        scal.update(log_alpha=self.log_sac_alpha.detach()[0], target_q_max=self._stats[0], clip_min=self.Q_guard.state[0],
                    clip_max=self.Q_guard.state[1], q1_l2_norm_square=self.values[0].l2_norm_square())
        for k in [k for k, v in host.items() if torch.is_tensor(v)]:      # clipped runs: the norm is a device scalar
            scal[k] = host.pop(k).detach()
        keys = list(scal)
        packed = torch.stack([scal[k].reshape(()).float() for k in keys])
        items = dict({k: float(v) for k, v in host.items()}, **self._host_log(batch_size, real_rows))
        if self._graph is not None:                              # captured update: a copy node into the graph's static buffer, read back behind the replay
            return self._graph.log_node(keys, packed, items)
        log = DeferredLog.from_packed(keys, packed, self.device.type == 'cuda', items)     # ONE device->host copy of all scalars
        if not self.defer_log:
            log.resolve()                                        # reference behaviour: floats in hand when the call returns
        return log
