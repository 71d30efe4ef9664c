"""Memoryless SAC-REDQ with one `efc-<E>` ensemble critic: the baseline recurrent trainers are compared against
(reference offpolicy_rnn/algorithm/sac_mlp_redq_ensemble_q.py:12-207).

Same contract (no sequence layer anywhere, `rnn_fix_length == 0`, one `efc` critic whose layers see `desire_ndim = 3`, the base
class's flat transition ring) and the same arithmetic per pass of the `utd` loop:
    draw `sac_batch_size` transitions -> done <- 0 where timeout > 0 -> [no grad] y = r + (1 - done) gamma (min over the `redq_m`
    critics of permutation(E)[:redq_m] of the target critic at the policy's sampled next action - alpha log pi) -> critic step on
    sum_e mean_m (q - y)^2 -> soft target update -> where `(utd_idx + 1) / utd * policy_utd > policy_update_cnt`: actor step on
    mean_m (alpha log pi - mean_e Q), alpha step, log_alpha <= 1.
There is no Q-guard, no loss mask and no target policy.  The numpy stream is consumed as the reference consumes it: per pass one
`randint(0, transition_count, (batch,))`, then one `permutation(E)`; actor noise comes through utility/rng.py.

What is organised differently for the MI355X (REDQ's usual utd = 20 on batches of a few hundred transitions is launch-bound):
  * the batch is gathered ON THE DEVICE from the ring's mirror: the host draws ranks and maps them to ring rows
    (`MemoryArray.plan_transitions`), `ops.gather_transitions` copies the rows and applies the done fix; fields are column-block
    views of that one array.  A CPU trainer keeps `sample_transitions`;
  * only the drawn members of the target critic are evaluated (`EnsembleLinear.member_index`, embedding stack and head), unless an
    `eln-<E>` norm couples the members;
  * target, losses, clipping, AdamW and the soft update are the kernels of hip/ops.py; losses are back-propagated as sums and the
    1 / batch rides in the scale word AdamW reads; the actor step differentiates the frozen critic with respect to the action only;
  * every scalar of the log stays on the device and is fetched with one transfer behind the last pass;
  * `train()` replays one hipGraph per pass (algorithm/graphed_transition_update.py; RESEL_GRAPH_UPDATE=0: eager launches).
Discrete actions are refused: the reference's own discrete branch cannot run (its `_target_Q_discrete` subtracts from the tuple that
`min(dim=0)` returns).  Process groups are refused as well."""
import contextlib
from typing import Dict

import numpy as np
import torch

from ..hip import ops
from ..models.ensemble_linear_model import EnsembleLinear
from ..models.layer_kinds import is_rnn_layer
from ..models.rnn_base import training_pass
from ..utility.deferred_log import ScalarLog
from ..utility.pinned import PinnedRing
from .sac import SAC
from .sac_full_length_rnn_ensembleQ import _frozen_parameters

FIELDS = ('state', 'last_state', 'last_action', 'action', 'next_state', 'reward', 'done', 'reward_input')


@contextlib.contextmanager
def _ensemble_subset(model, member_index):
    """Evaluate only the members `member_index` (int64, device) of every `efc` layer of `model`: embedding stack and head."""
    layers = [l for net in (model.embedding_network, model.uni_network) for l in net.layer_list if isinstance(l, EnsembleLinear)]
    for l in layers:
        l.member_index = member_index
    try:
        yield
    finally:
        for l in layers:
            l.member_index = None


class SAC_MLP_REDQ_EnsembleQ(SAC):
    transition_level = True     # batches are single transitions: `GraphedTransitionUpdate` replays this trainer's passes
    defer_log = False           # True: the log's device scalars stay in flight until first read; False: floats on return, as the reference

    def __init__(self, parameter):
        # the reference's constructor contract (:13-27), checked on the flag set before anything is built
        for which in ('policy_embedding_layer_type', 'policy_layer_type', 'value_embedding_layer_type', 'value_layer_type'):
            for lid in getattr(parameter, which):
                assert not is_rnn_layer(lid), f'sac mlp does not support sequence layers ({which}: {lid})'
        assert parameter.rnn_fix_length == 0, f'sac mlp only support rnn_fix_length==0, got {parameter.rnn_fix_length}'
        assert parameter.value_net_num == 1, f'one efc-<E> ensemble critic (value_net_num == 1), got {parameter.value_net_num}'
        for item in list(parameter.value_layer_type) + list(parameter.value_embedding_layer_type):
            assert item.startswith('e'), f'the critic stacks must be ensemble (efc-<E>) layers, got {item}'
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError('sac_mlp_redq_ensemble_q runs in one process: a process group of more than one rank is not supported')
        super().__init__(parameter)
        if self.discrete_env:
            raise NotImplementedError('sac_mlp_redq_ensemble_q supports continuous actions only: the discrete branch of the reference '
                                      'trainer cannot run (its target subtracts from the tuple that min(dim=0) returns)')
        value, target = self.values[0], self.target_values[0]
        for net in (value.embedding_network.layer_list + target.embedding_network.layer_list
                    + value.uni_network.layer_list + target.uni_network.layer_list):
            if hasattr(net, 'desire_ndim'):
                net.desire_ndim = 3
        self.num_ensemble = target.uni_network.layer_list[-1].num_ensemble
        assert 1 <= parameter.redq_m <= self.num_ensemble, f'redq_m = {parameter.redq_m} of {self.num_ensemble} critics'
        self._graph = None                             # set while a captured pass is being recorded / launched (graphed_transition_update.py)
        self._rows_ring = PinnedRing(torch.int32, depth=4)    # staging blocks of the eager pass's drawn rows and REDQ subset
        self._drawn_subset = None                      # the eager GPU pass's subset, uploaded with its rows (_sample -> _target_subset)
        self._stats = torch.zeros(1, dtype=torch.float32, device=self.device)         # max |target| of the last pass
        self._inv_batch = torch.full((1,), 1.0 / parameter.sac_batch_size, dtype=torch.float32, device=self.device)
        if self.device.type == 'cuda':                 # the entropy coefficient's AdamW keeps its step count on the device: the same step eagerly and in a graph
            for g in self.optimizer_alpha.param_groups:
                g['capturable'] = True

    # ------------------------------------------------------------------------------------------ batch
    def _ring_columns(self):
        R = self.replay_buffer.name2range
        return R['done'][0], (R['timeout'][0] if R['timeout'][1] > R['timeout'][0] else -1)

    def _views(self, batch):
        """Field views of the batch array [batch, W]: column blocks, as the full-trajectory trainer reads its packed batch."""
        R = self.replay_buffer.name2range
        return {name: batch[:, R[name][0]:R[name][1]] for name in FIELDS}

    # ---- the driver's view of this trainer's plan (graphed_transition_update.py)
    def graph_plan_words(self):
        return self.parameter.sac_batch_size

    def graph_subset_size(self):
        return self.parameter.redq_m

    def graph_plan_pass(self):
        return self.replay_buffer.plan_transitions(self.parameter.sac_batch_size, 1)[0]

    def graph_gather(self, ring_dev, table, pass_word):
        c_done, c_timeout = self._ring_columns()
        return ops.gather_transitions(ring_dev, table, pass_word, 0, c_done, c_timeout)

    def graph_optimizers(self):
        """-> (the optimizers the critic step advances, those the actor step advances)."""
        return [self.optimizer_value], [self.optimizer_policy]

    def _sample(self):
        """One transition batch -> its field views on the trainer's device, `done` already 0 where the transition timed out."""
        ring, n = self.replay_buffer, self.parameter.sac_batch_size
        if self._graph is not None:                    # captured pass: the rows of every pass of the step sit in a static table
            return self._views(self._graph.gather())
        if self.device.type == 'cuda':                 # plan on the host, gather on the device
            # the pass's two numpy draws, in the reference's order (nothing between them draws from numpy), through ONE pinned block
            rows = ring.plan_transitions(n, 1)
            m = self.parameter.redq_m
            host = self._rows_ring.stage(n + m, self.device)
            host.numpy()[:n] = rows.reshape(-1)
            host.numpy()[n:] = np.random.permutation(self.num_ensemble)[:m]
            both = self._rows_ring.upload(host, self.device)
            rows_dev, self._drawn_subset = both[:n].view(1, n), both[n:]
            c_done, c_timeout = self._ring_columns()
            return self._views(ops.gather_transitions(ring._mirror(self.device), rows_dev, None, 0, c_done, c_timeout))
        tr = ring.sample_transitions(n)
        b = {name: torch.from_numpy(np.ascontiguousarray(getattr(tr, name))).to(self.device) for name in FIELDS}
        if tr.timeout is not None:
            b['done'][torch.from_numpy(np.ascontiguousarray(tr.timeout)).to(self.device) > 0] = 0
        return b

    # ------------------------------------------------------------------------------------------ target
    def _target_subset(self):
        """The `redq_m` critics of this pass's target -> (int32 index, int64 index) on the device; one `permutation(E)` of the global
        numpy stream - made by `_sample` beside the rows on the GPU, here on the CPU -, unless a captured pass reads the draw the
        driver made for it."""
        if self._graph is not None:
            return self._graph.target_subset()
        if self._drawn_subset is not None:
            i32, self._drawn_subset = self._drawn_subset, None
            return i32, i32.long()
        sub = np.ascontiguousarray(np.random.permutation(self.num_ensemble)[:self.parameter.redq_m], dtype=np.int32)
        i32 = torch.from_numpy(sub).to(self.device)
        return i32, i32.long()

    def _arange(self, m):
        if getattr(self, '_arange_m', None) is None or self._arange_m.numel() != m:
            self._arange_m = torch.arange(m, dtype=torch.int32, device=self.device)
        return self._arange_m

    def _target_Q(self, b):
        """y = r + (1 - done) gamma (min over the drawn target critics at a' ~ pi(.|s') - alpha log pi(a'|s')), no graph."""
        tv = self.target_values[0]
        with torch.no_grad():
            _, _, sample, logp, _, _ = self.policy.forward(b['next_state'], b['state'], b['action'], None, b['reward'])
            i32, i64 = self._target_subset()
            coupled = tv.uni_network.members_coupled() or tv.embedding_network.members_coupled()
            if i32.numel() < self.num_ensemble and not coupled:    # only the drawn members are evaluated: q holds them in draw order
                with _ensemble_subset(tv, i64):
                    q = tv.forward(b['next_state'], b['state'], b['action'], sample, None, b['reward'])[0]
                index = self._arange(i32.numel())
            else:
                q = tv.forward(b['next_state'], b['state'], b['action'], sample, None, b['reward'])[0]
                index = i32
            if q.is_cuda:
                return ops.redq_target(q, index, logp, self.log_sac_alpha.detach(), b['reward'], b['done'], self.parameter.gamma, self._stats)
            y = b['reward'] + (1 - b['done']) * self.parameter.gamma * (q[index.long()].min(dim=0).values - self.log_sac_alpha.detach().exp() * logp)
            self._stats[0] = y.abs().max()             # CPU tensors keep the torch spelling
            return y

    # ------------------------------------------------------------------------------------------ steps
    def _clip(self, store, max_norm, scale):
        """Optional norm clipping of the mean-loss gradient (reference :159-162, :173-176) without rewriting it: ||g / batch|| from one
        read of the flat buffer, the coefficient min(1, max_norm / (norm + 1e-6)) folded into the scale word AdamW reads.  -> the norm
        (a device scalar) or 0.0"""
        if max_norm is None:
            return 0.0
        gnorm = ops.sumsq(store.grad[:store.numel]).sqrt_().mul_(scale)
        scale.mul_((max_norm / (gnorm + 1e-6)).clamp_(max=1.0))
        return gnorm[0]

    def _critic_step(self, b, target_Q, scal):
        par, value = self.parameter, self.values[0]
        q = value.forward(b['state'], b['last_state'], b['last_action'], b['action'], None, b['reward_input'])[0]
        if q.is_cuda:
            q_loss_sum = ops.masked_q_loss(q, target_Q, None)
        else:
            q_loss_sum = (q - target_Q.unsqueeze(0)).pow(2).sum()
        self.optimizer_value.zero_grad()
        q_loss_sum.backward()
        value.store.collect_grads()
        scale = self._inv_batch.clone()
        scal['q_grad_norm'] = self._clip(value.store, par.value_max_gradnorm, scale)
        self.optimizer_value.step(grad_scale=scale)
        scal['critic_loss'] = q_loss_sum.detach() * self._inv_batch[0]

    def _actor_step(self, b, scal):
        par, value, pstore = self.parameter, self.values[0], self.policy.store
        _, _, sample, logp, _, _ = self.policy.forward(b['state'], b['last_state'], b['last_action'], None, b['reward_input'])
        with _frozen_parameters(value):                # Q is differentiated with respect to the action only
            q_pi = value.forward(b['state'], b['last_state'], b['last_action'], sample, None, b['reward_input'])[0]
        if q_pi.is_cuda:
            actor_sum, lp_sum = ops.masked_actor_loss(logp, q_pi, None, self.log_sac_alpha, True, False)
        else:
            actor_sum = (self.log_sac_alpha.detach().exp() * logp - q_pi.mean(dim=0)).sum()
            lp_sum = logp.detach().sum()
        self.optimizer_policy.zero_grad()
        actor_sum.backward(inputs=self.policy.parameters())
        pstore.collect_grads()
        scale = self._inv_batch.clone()
        scal['pi_grad_norm'] = self._clip(pstore, par.policy_max_gradnorm, scale)
        self.optimizer_policy.step(grad_scale=scale)
        # alpha loss -(log_alpha (logp + H).detach()).mean(): its gradient is -(mean logp + H)
        g_alpha = -(lp_sum * self._inv_batch + self.target_entropy)
        scal['alpha_loss'] = (self.log_sac_alpha.detach() * g_alpha)[0]
        self.log_sac_alpha.grad = g_alpha.reshape(self.log_sac_alpha.shape)
        self.optimizer_alpha.step()
        with torch.no_grad():
            self.log_sac_alpha.clamp_max_(1)
        scal['actor_loss'] = actor_sum.detach() * self._inv_batch[0]
        scal['log_prob'] = lp_sum * self._inv_batch[0]

    def _actor_due(self, utd_idx, done_so_far) -> bool:
        """Does the actor (+ alpha) step follow critic step `utd_idx`, `done_so_far` actor steps into this update (reference :166)?"""
        par = self.parameter
        return (utd_idx + 1) / par.utd * par.policy_utd > done_so_far

    def _one_pass(self, utd_idx, actor_steps, scal) -> bool:
        """Pass `utd_idx` of an update, `actor_steps` actor steps into it.  Fills `scal`; -> did the actor step run."""
        b = self._sample()
        target_Q = self._target_Q(b)
        self._critic_step(b, target_Q, scal)
        self._value_update(tau=self.parameter.sac_tau)
        scal['target_q_max'] = self._stats[0]
        scal['log_alpha'] = self.log_sac_alpha.detach()[0]
        actor_due = self._actor_due(utd_idx, actor_steps)
        if actor_due:
            self._actor_step(b, scal)
            scal['log_alpha'] = self.log_sac_alpha.detach()[0]
        return bool(actor_due)

    def _norm_scalars(self):
        """The two parameter norms of the log: formed once per update, behind its last pass (reference :197-198)."""
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
        """-> (keys, their scalars as one device vector); a norm that was not formed (no clipping) is the reference's 0."""
        keys = list(scal)
        zero = self._stats.new_zeros(())
        return keys, torch.stack([(scal[k] if torch.is_tensor(scal[k]) else zero).detach().reshape(()).float() for k in keys])

    # ------------------------------------------------------------------------------------------ train()
    def update_driver(self):
        """One graph replay per pass of the `utd` loop (graphed_transition_update.py)."""
        from .graphed_transition_update import GraphedTransitionUpdate
        return GraphedTransitionUpdate
