"""Recurrent SAC trained on fixed-length slices from a zero state (R2D2-style): the baseline the full-trajectory trainers are defined
against (reference offpolicy_rnn/algorithm/sac_rnn_slice.py:11-215, buffers/replay_memory_tail_padding.py).

Same arithmetic per pass of the `utd` loop:
    draw `sac_batch_size` stored transitions (one `randint` of the global numpy stream) -> the slice of a drawn (traj, point) is rows
    point .. point + L - 1 of that trajectory, L = `rnn_slice_length`, all-zero rows (mask 0) behind the trajectory's end ->
    done <- 0 where timeout > 0 -> valid_num = mask.sum() -> [no grad] the policy and every target critic run from a ZERO state over
    the L + 1 window (state_0, next_state_0..L-1 | last_state_0, state_0..L-1 | last_action_0, action_0..L-1 | reward_input_0,
    reward_0..L-1), positions 1..L give y = r + (1 - done) gamma (min over the `value_net_num` target critics - alpha log pi), on
    discrete actions sum_a p (min_i Q_i - alpha log p) -> critic step on sum_i sum(mask (Q_i - y)^2) / valid_num, every critic from a
    zero state on the L window -> soft target update -> where `(utd_idx + 1) / utd * policy_utd > policy_update_cnt`: actor step on
    sum(mask (alpha log pi - min_i Q_i)) / valid_num (or its discrete expectation), alpha step with the reference's loss, log_alpha <= 1.
There is no Q-guard, no gradient clipping and no target policy.  Nothing but the slice draw consumes numpy; actor noise comes through
utility/rng.py.

What is organised differently for the MI355X:
  * the batch is gathered ON THE DEVICE from the ring's mirror: the host draws ranks and maps them to (ring row, valid rows)
    (`MemoryArray.plan_slices`), ONE launch of `ops.gather_slices` writes [batch, L + 1, W]: slot 0 is the pre-step row (state <-
    last_state, next_state <- state, action <- last_action, reward <- reward_input of the slice's first transition), slots 1..L the
    slice.  Both windows are column-block views of that one array - `[:, 1:]` is the batch, `[:, :]` read through the next_state /
    state / action / reward columns is the L + 1 window -, nothing is concatenated (discrete actions: the one-hot of the action index);
  * the critics are separate networks; their outputs are stacked along axis 0 and the target, the losses, AdamW and the soft update are
    the kernels of hip/ops.py; losses are back-propagated as sums and 1 / valid_num stays a device scalar that rides in the scale word
    AdamW reads; the actor step differentiates the frozen critics with respect to the action only;
  * every scalar of the log stays on the device and is fetched with one transfer behind the last pass;
  * `train()` replays one hipGraph per pass (algorithm/graphed_transition_update.py; RESEL_GRAPH_UPDATE=0: eager launches).
A CPU trainer builds the same array on the host (`host_slice_batch`) and keeps the torch spelling of target and losses.

Out of scope: `rnn_slice_length == 1` (a window of one token is what several sequence families treat as a rollout step without a
backward), ensemble layers (the minimum is over critic NETWORKS, not over a member axis), `cgpt*` (its packed-sequence path needs a
sequence table), process groups."""
import contextlib
import re
from typing import Dict

import numpy as np
import torch

from ..hip import ops
from ..models.rnn_base import training_pass
from ..utility.deferred_log import ScalarLog
from ..utility.pinned import PinnedRing
from .sac import SAC
from .sac_full_length_rnn_ensembleQ import _frozen_parameters

FIELDS = ('state', 'last_state', 'last_action', 'action', 'next_state', 'reward', 'mask', 'done', 'reward_input')
_ENSEMBLE_ID = re.compile(r'e[a-z0-9_]*-[0-9]+')
_STACKS = ('policy_embedding_layer_type', 'policy_layer_type', 'value_embedding_layer_type', 'value_layer_type')


def pre_step_pairs(name2range, discrete):
    """The (destination, source) column pairs of a slice's pre-step row, int32 [npairs, 2] (the `pre_pairs` convention of
    `resel_gather_trajs`).  Discrete actions: the action column is an index and cannot hold the one-hot last action; slot 0 keeps
    `last_action` in its own columns instead."""
    R = name2range
    fields = [('next_state', 'state'), ('state', 'last_state'), ('reward', 'reward_input'),
              ('last_action', 'last_action') if discrete else ('action', 'last_action')]
    pairs = []
    for dst, src in fields:
        assert R[dst][1] - R[dst][0] == R[src][1] - R[src][0], (dst, src, R[dst], R[src])
        pairs += list(zip(range(*R[dst]), range(*R[src])))
    return np.asarray(pairs, dtype=np.int32).reshape(-1, 2)


def host_slice_batch(ring, plan, length, pairs, c_done, c_timeout):
    """What `ops.gather_slices` writes for one pass of a slice plan (int32 [batch, 2]), on the host -> fp32 [batch, length + 1, W]."""
    plan = np.asarray(plan).reshape(-1, 2)
    out = np.zeros((len(plan), int(length) + 1, ring.width), dtype=np.float32)
    out[:, 1:] = ring.slices_from_plan(plan, length)
    if c_timeout >= 0:
        out[:, 1:, c_done][out[:, 1:, c_timeout] > 0] = 0
    first = ring.memory_buffer[plan[:, 0]]
    out[:, 0, pairs[:, 0]] = first[:, pairs[:, 1]]
    return out


class SACRNNSlice(SAC):
    transition_level = True     # a pass is one fixed-shape batch: `GraphedTransitionUpdate` replays this trainer's passes
    defer_log = False           # True: the log's device scalars stay in flight until first read; False: floats on return, as the reference

    def __init__(self, parameter):
        L = int(parameter.rnn_slice_length)
        if L == 1:
            raise ValueError('sac_rnn_slice: rnn_slice_length = 1 is not supported: a window of one token is what several sequence '
                             'families treat as a rollout step without a backward; use rnn_slice_length >= 2')
        assert L >= 2, f'sac_rnn_slice needs rnn_slice_length >= 2, got {parameter.rnn_slice_length}'
        assert parameter.value_net_num >= 1, f'value_net_num = {parameter.value_net_num}'
        for which in _STACKS:
            for lid in getattr(parameter, which):
                if _ENSEMBLE_ID.fullmatch(lid):
                    raise ValueError(f'sac_rnn_slice takes the minimum over its value_net_num critic networks, not over a member axis: '
                                     f'the ensemble layer {lid} ({which}) is not supported')
                if lid.startswith('cgpt'):
                    raise NotImplementedError(f'sac_rnn_slice does not support {lid} ({which}): its packed-sequence path needs a sequence table')
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError('sac_rnn_slice runs in one process: a process group of more than one rank is not supported')
        super().__init__(parameter)
        self.slice_length = L
        self._graph = None                             # set while a captured pass is being recorded / launched (graphed_transition_update.py)
        self._plan_ring = PinnedRing(torch.int32, depth=4)     # staging blocks of the eager pass's plan
        self._pairs = None                             # the pre-step column pairs (host, device), once the ring has its layout
        self._stats = torch.zeros(1, dtype=torch.float32, device=self.device)         # max |target| of the last pass
        self._critic_index = torch.arange(len(self.values), dtype=torch.int32, device=self.device)
        self._one_index = torch.zeros(1, dtype=torch.int32, device=self.device)
        # log pi of the last actor step (all actions' on discrete actions): a static buffer, so that a replayed pass without an actor step reads it
        self._logp_keep = torch.zeros(parameter.sac_batch_size, L, self.act_dim if self.discrete_env else 1, dtype=torch.float32, device=self.device)
        if self.device.type == 'cuda':                 # the entropy coefficient's AdamW keeps its step count on the device: the same step eagerly and in a graph
            for g in self.optimizer_alpha.param_groups:
                g['capturable'] = True

    # ------------------------------------------------------------------------------------------ batch
    def _ring_columns(self):
        R = self.replay_buffer.name2range
        return R['done'][0], (R['timeout'][0] if R['timeout'][1] > R['timeout'][0] else -1)

    def _pre_pairs(self):
        if self._pairs is None:
            host = pre_step_pairs(self.replay_buffer.name2range, self.discrete_env)
            self._pairs = (host, torch.from_numpy(host).to(self.device))
        return self._pairs

    def _views(self, g):
        """Field views of the gathered array g [batch, L + 1, W]: `b` the batch (slots 1..L), `full` the L + 1 window of the target pass
        (reference :25-28), all column blocks of g."""
        R = self.replay_buffer.name2range
        col = lambda t, name: t[..., R[name][0]:R[name][1]]
        b = {name: col(g[:, 1:], name) for name in FIELDS}
        full = dict(state=col(g, 'next_state'), last_state=col(g, 'state'), reward=col(g, 'reward'))
        if self.discrete_env:                          # slot 0 keeps last_action_0 in the last_action columns; behind it the one-hot of the action taken
            full['last_action'] = torch.cat((col(g[:, :1], 'last_action'), self.policy.action2onehot(b['action'])), dim=1)
        else:
            full['last_action'] = col(g, 'action')
        return b, full

    # ---- the driver's view of this trainer's plan (graphed_transition_update.py)
    def graph_plan_words(self):
        return 2 * self.parameter.sac_batch_size

    def graph_subset_size(self):
        return 0                                       # no REDQ subset: every target critic enters the minimum

    def graph_plan_pass(self):
        """One pass's plan as the driver's table holds it: the draw of the eager pass."""
        return self.replay_buffer.plan_slices(self.parameter.sac_batch_size, self.slice_length, 1).reshape(-1)

    def graph_gather(self, ring_dev, table, pass_word):
        c_done, c_timeout = self._ring_columns()
        plan = table.view(table.shape[0], self.parameter.sac_batch_size, 2)
        return ops.gather_slices(ring_dev, plan, self.slice_length, self._pre_pairs()[1], pass_word, 0, c_done, c_timeout)

    def graph_optimizers(self):
        """-> (the optimizers the critic step advances, those the actor step advances)."""
        return list(self.optimizers_value), [self.optimizer_policy]

    def _sample(self):
        """One slice batch -> (batch views, L + 1 window views) on the trainer's device, `done` already 0 where the transition timed out."""
        ring, n, L = self.replay_buffer, self.parameter.sac_batch_size, self.slice_length
        if self._graph is not None:                    # captured pass: the plans of every pass of the step sit in a static table
            return self._views(self._graph.gather())
        plan = ring.plan_slices(n, L, 1)               # the pass's one numpy draw
        c_done, c_timeout = self._ring_columns()
        if self.device.type == 'cuda':                 # plan on the host, gather on the device
            host = self._plan_ring.stage(2 * n, self.device)
            host.numpy()[:] = plan.reshape(-1)
            plan_dev = self._plan_ring.upload(host, self.device).view(1, n, 2)
            return self._views(ops.gather_slices(ring._mirror(self.device), plan_dev, L, self._pre_pairs()[1], None, 0, c_done, c_timeout))
        return self._views(torch.from_numpy(host_slice_batch(ring, plan[0], L, self._pre_pairs()[0], c_done, c_timeout)).to(self.device))

    # ------------------------------------------------------------------------------------------ target
    def _target_Q(self, b, full):
        """y over positions 1..L of the L + 1 window, every network from a zero state, no graph."""
        with torch.no_grad():
            _, _, sample, logp, _, _ = self.policy.forward(full['state'], full['last_state'], full['last_action'], None, full['reward'])
            q = torch.stack([tv.forward(full['state'], full['last_state'], full['last_action'], sample, None, full['reward'])[0]
                             for tv in self.target_values])[:, :, 1:]
            logp = logp[:, 1:]
            la = self.log_sac_alpha.detach()
            if q.is_cuda:
                if self.discrete_env:
                    v = ops.discrete_value(q, None, logp, la)
                    return ops.redq_target(v.unsqueeze(0), self._one_index, None, la, b['reward'], b['done'], self.parameter.gamma, self._stats)
                return ops.redq_target(q, self._critic_index, logp, la, b['reward'], b['done'], self.parameter.gamma, self._stats)
            if self.discrete_env:                      # CPU tensors keep the torch spelling
                v = ((q.min(dim=0).values - la.exp() * logp) * logp.exp()).sum(dim=-1, keepdim=True)
            else:
                v = q.min(dim=0).values - la.exp() * logp
            y = b['reward'] + (1 - b['done']) * self.parameter.gamma * v
            self._stats[0] = y.abs().max()
            return y

    # ------------------------------------------------------------------------------------------ steps
    def _critic_step(self, b, target_Q, inv_valid, scal):
        q = torch.stack([value.forward(b['state'], b['last_state'], b['last_action'], b['action'], None, b['reward_input'])[0]
                         for value in self.values])
        if q.is_cuda:
            if self.discrete_env:                      # Q of the action taken, picked inside the loss kernels
                q_loss_sum = ops.masked_q_taken_loss(q, b['action'], target_Q, b['mask'])
            else:
                q_loss_sum = ops.masked_q_loss(q, target_Q, b['mask'])
        else:
            if self.discrete_env:
                q = q.gather(-1, b['action'].long().unsqueeze(0).expand(q.shape[0], -1, -1, -1))
            q_loss_sum = ((q - target_Q.unsqueeze(0)).pow(2).sum(dim=0) * b['mask']).sum()
        for opt in self.optimizers_value:
            opt.zero_grad()
        q_loss_sum.backward()
        for value, opt in zip(self.values, self.optimizers_value):
            value.store.collect_grads()
            opt.step(grad_scale=inv_valid)
        scal['critic_loss'] = q_loss_sum.detach() * inv_valid[0]

    def _actor_step(self, b, inv_valid, scal):
        pstore, mask = self.policy.store, b['mask']
        _, _, sample, logp, _, _ = self.policy.forward(b['state'], b['last_state'], b['last_action'], None, b['reward_input'])
        with contextlib.ExitStack() as frozen:         # Q is differentiated with respect to the action only
            for value in self.values:
                frozen.enter_context(_frozen_parameters(value))
            q_pi = torch.stack([value.forward(b['state'], b['last_state'], b['last_action'], sample, None, b['reward_input'])[0]
                                for value in self.values])
        la = self.log_sac_alpha
        if self.discrete_env:
            # lp_sum = sum mask sum_a p log p: the alpha loss of the reference (:116-119) weighs with p (its log entry does not, `_one_pass`)
            if q_pi.is_cuda:
                actor_sum, lp_sum = ops.masked_discrete_actor_loss(logp, q_pi, mask, la, True)
            else:
                p = logp.exp()
                actor_sum = (((la.detach().exp() * logp - q_pi.min(dim=0).values) * p).sum(dim=-1, keepdim=True) * mask).sum()
                lp_sum = ((p * logp).detach().sum(dim=-1, keepdim=True) * mask).sum()
            # alpha loss -mean_mask(p (-log_alpha (logp + H))): its gradient is +(mean_mask sum_a p logp + H)
            g_alpha = lp_sum * inv_valid + self.target_entropy
        else:
            if q_pi.is_cuda:
                actor_sum, lp_sum = ops.masked_actor_loss(logp, q_pi, mask, la, True, True)
            else:
                actor_sum = ((la.detach().exp() * logp - q_pi.min(dim=0).values) * mask).sum()
                lp_sum = (logp.detach() * mask).sum()
            # alpha loss -mean_mask(log_alpha (logp + H)): its gradient is -(mean_mask logp + H)
            g_alpha = -(lp_sum * inv_valid + self.target_entropy)
        self.optimizer_policy.zero_grad()
        actor_sum.backward(inputs=self.policy.parameters())
        pstore.collect_grads()
        self.optimizer_policy.step(grad_scale=inv_valid)
        scal['alpha_loss'] = (self.log_sac_alpha.detach() * g_alpha)[0]
        self.log_sac_alpha.grad = g_alpha.reshape(self.log_sac_alpha.shape)
        self.optimizer_alpha.step()
        with torch.no_grad():
            self.log_sac_alpha.clamp_max_(1)
        scal['actor_loss'] = actor_sum.detach() * inv_valid[0]
        self._logp_keep.copy_(logp.detach())

    def _actor_due(self, utd_idx, done_so_far) -> bool:
        """Does the actor (+ alpha) step follow critic step `utd_idx`, `done_so_far` actor steps into this update (reference :178)?"""
        par = self.parameter
        return (utd_idx + 1) / par.utd * par.policy_utd > done_so_far

    def _one_pass(self, utd_idx, actor_steps, scal) -> bool:
        """Pass `utd_idx` of an update, `actor_steps` actor steps into it.  Fills `scal`; -> did the actor step run."""
        b, full = self._sample()
        inv_valid = b['mask'].sum().reciprocal().reshape(1)       # 1 / valid_num: a device scalar (the first row of a slice is always valid)
        target_Q = self._target_Q(b, full)
        self._critic_step(b, target_Q, inv_valid, scal)
        self._value_update(tau=self.parameter.sac_tau)
        scal['target_q_max'] = self._stats[0]
        scal['log_alpha'] = self.log_sac_alpha.detach()[0]
        actor_due = self._actor_due(utd_idx, actor_steps)
        if actor_due:
            self._actor_step(b, inv_valid, scal)
            scal['log_alpha'] = self.log_sac_alpha.detach()[0]
        # the reference's log entry (:203) is the LAST actor step's log pi under the LAST pass's mask and valid count - on a pass without
        # an actor step (policy_utd < utd) these come from two different batches; kept (pass 0 of an update always has an actor step)
        scal['log_prob'] = (self._logp_keep * b['mask']).sum() * inv_valid[0]
        return bool(actor_due)

    def _norm_scalars(self):
        """The two parameter norms of the log: formed once per update, behind its last pass (reference :207-208)."""
        return dict(policy_l2_norm_square=self.policy.l2_norm_square(), q1_l2_norm_square=self.values[0].l2_norm_square())

    # ------------------------------------------------------------------------------------------ the update
    def train_one_batch(self) -> Dict:
        with training_pass():
            if self.device.type == 'cuda':
                ops.amax_maintenance()                 # update boundary: the magnitude epochs may start over here (hip/ops.py)
            log = self._train_one_batch()
            if ops.AMAX_VERIFY and self.device.type == 'cuda':
                ops.amax_verify_raise(self.device)
            return log

    def _train_one_batch(self):
        """One update: `utd` passes -> log.  While a GraphedTransitionUpdate records or launches a pass from its static inputs it runs
        ONE pass at the position the driver hands over, and that pass's scalars go into the driver's log buffer."""
        scal: Dict[str, torch.Tensor] = {}
        if self._graph is not None:
            self._one_pass(*self._graph.pass_position(), scal)
            return self._graph.log_node(*self._pack(scal))
        actor_steps = 0
        for utd_idx in range(self.parameter.utd):
            actor_steps += self._one_pass(utd_idx, actor_steps, scal)
        scal.update(self._norm_scalars())
        keys, packed = self._pack(scal)
        log = ScalarLog.from_packed(keys, packed, self.device.type == 'cuda')      # ONE device->host copy of all scalars
        if not self.defer_log:
            log.resolve()
        return log

    def _pack(self, scal):
        """-> (keys, their scalars as one device vector)."""
        keys = list(scal)
        return keys, torch.stack([scal[k].detach().reshape(()).float() for k in keys])

    # ------------------------------------------------------------------------------------------ train()
    def update_driver(self):
        """One graph replay per pass of the `utd` loop (graphed_transition_update.py)."""
        from .graphed_transition_update import GraphedTransitionUpdate
        return GraphedTransitionUpdate
