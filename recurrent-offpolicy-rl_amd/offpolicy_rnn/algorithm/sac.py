"""SAC base trainer: construction (env, seeds, actor / critics, optimizers, replay buffer), the environment loop and
checkpoint I/O (reference offpolicy_rnn/algorithm/sac.py:33-420).  The per-update work lives in the full-trajectory
sub-classes (`train_one_batch`).  Evaluation (reference sac.py:284-300,364-379): at the start of every iteration `train()` runs
`test_nprocess * test_nrollout` deterministic episodes of the current policy and logs them as `performance/EpRetTest` and
`performance/EpLenTest` at its end.  The reference's CPU worker pool (`eval_inprocess`) has no counterpart here - this build has no
CPU forward; the episodes run synchronously on the device instead, up to 64 environments per graph replay
(utility/policy_eval.py `BatchedPolicyEval`, hip/graph_step.py `row_reset`)."""
import math
import os
import random
import time
from typing import Dict, List, Union

import numpy as np
import torch

from .._compat import Logger, smart_logger
from ..buffers.transition_buffer.replay_memory import MemoryArray, Transition
from ..env_utils.make_env import make_env
from ..policy_value_models.make_models import make_policy_model, make_value_model
from ..utility.count_parameters import count_parameters
from ..utility.sample_utility import n2t_2dim, norm_act, t2n, unorm_act
from ..utility.timer import Timer
from . import run_state
from .flat_adamw import FlatAdamW


class SAC:
    def __init__(self, parameter):
        self.parameter = parameter
        self.timer = Timer()
        self.logger = Logger(log_name=self.parameter.short_name)
        self.parameter.set_config_path(os.path.join(self.logger.output_dir, 'config'))
        self.parameter.save_config()
        self.logger(self.parameter)
        # environment
        self.env_name = parameter.env_name
        self.env_info = make_env(self.env_name, parameter.seed)
        self.eval_env_info = make_env(self.env_name, parameter.seed + 1)
        self.env, self.eval_env = self.env_info['train_env'], self.eval_env_info['train_env']
        self.max_episode_steps = self.env_info['max_trajectory_len']
        self.discrete_env = not self.env_info['act_continuous']
        self.obs_dim = self.env.observation_space.shape[0]
        self.act_dim = self.env_info['act_dim']
        self._seed(parameter.seed)
        # networks
        self.policy_args = self._make_policy_args(parameter)
        self.value_args = self._make_value_args(parameter)
        self.device = self._pick_device()
        # The reference samples on the CPU unless --cuda_inference (sac.py:45-49).  This build has no CPU forward (every layer
        # is a HIP kernel), so on a GPU the policy always lives - and samples - on the device: the flag is implied.
        if self.device.type == 'cuda' and not parameter.cuda_inference:
            self.logger('cuda_inference is implied on a GPU: the policy stays resident on the device (no CPU forward in this build)')
        self.sample_device = self.device
        self.base_algorithm = getattr(parameter, 'base_algorithm', 'sac')
        self.policy = make_policy_model(self.policy_args, self.base_algorithm, self.discrete_env)
        self.values = [make_value_model(self.value_args, self.base_algorithm, self.discrete_env) for _ in range(parameter.value_net_num)]
        self.target_values = [make_value_model(self.value_args, self.base_algorithm, self.discrete_env) for _ in range(parameter.value_net_num)]
        for v in self.values + self.target_values:
            v.to(self.device)
        self.policy.to(self.sample_device)
        self._value_update(tau=0.0)
        if self.discrete_env:
            parameter.no_alpha_auto_tune = True                  # reference sac.py:72-74: fixed temperature for discrete actions
        if getattr(parameter, 'no_alpha_auto_tune', False):
            alpha0 = math.log(parameter.sac_alpha)
        else:
            alpha0 = 0.0
        self.log_sac_alpha = torch.tensor([alpha0], dtype=torch.float32, device=self.device).requires_grad_(True)
        self.target_entropy = parameter.target_entropy_ratio if self.discrete_env else \
            -float(np.prod(self.env.action_space.shape)) * parameter.target_entropy_ratio
        # optimizers: one flat AdamW per network (a single learning rate here; the *_sep_optim trainers regroup)
        self.optimizer_policy = FlatAdamW(self.policy.store, lambda m: parameter.policy_lr, lambda m: parameter.policy_l2_norm)
        self.optimizers_value = [FlatAdamW(v.store, lambda m: parameter.value_lr, lambda m: parameter.value_l2_norm) for v in self.values]
        self.optimizer_alpha = torch.optim.AdamW([self.log_sac_alpha], lr=parameter.alpha_lr)   # default weight decay, as upstream
        for v in self.values:
            v.train()
        for v in self.target_values:
            v.eval()
        self.policy.train()
        self.replay_buffer = MemoryArray(parameter.max_buffer_transition_num, smart_logger.get_customized_value('MAX_TRAJ_STEP'))
        # rollout state
        self.state_np = np.zeros((1, self.obs_dim))
        self.last_action_np = np.zeros((1, self.act_dim))
        self.last_state_np = np.zeros((1, self.obs_dim))
        self.reward_np = np.zeros((1, 1))
        self.sample_hidden = None
        # on the GPU the per-step policy forward is replayed as one hipGraph (hip/graph_step.py); RESEL_GRAPH_ROLLOUT=0: eager
        self.graph_step = None
        if self.sample_device.type == 'cuda' and os.environ.get('RESEL_GRAPH_ROLLOUT', '1') != '0':
            from ..hip.graph_step import GraphedPolicyStep
            self.graph_step = GraphedPolicyStep(self.policy, self.sample_device, batch_size=1)
        self.evaluator = None                   # BatchedPolicyEval, built by the first evaluate()
        self._eval_refusal_logged = False
        self.collector = None                   # DeviceCollector of the running / last train(), when it collected on the device
        self._collect_refusal_logged = False
        self.sample_num = 0
        self.grad_num = 0
        self.start_time = time.time()
        # the open training episode's running return and length, and the iterations `train()` has completed: part of the run state
        # (algorithm/run_state.py).  While a DeviceCollector runs, the first two live on the device until `sync_host()`
        self.ep_ret, self.ep_len = 0.0, 0
        self.iteration = 0
        self._collecting = False                # inside `train()`'s loop: the collector, when there is one, owns the open episode
        self._host_episode_open = False         # a resumed run finishes the episode its state was taken in through the host loop
        self.allow_nest_stack = self.allow_nest_stack_trajs()
        self.logger(f'policy parameter num: {count_parameters(self.policy)}; value[0] parameter num: {count_parameters(self.values[0])}')

    @staticmethod
    def _pick_device():
        if torch.cuda.is_available():
            return torch.device('cuda', torch.cuda.current_device())
        return torch.device('cpu')

    @property
    def optimizer_value(self):
        return self.optimizers_value[0]

    def allow_nest_stack_trajs(self):
        """Rows may pack several trajectories unless a layer cannot honour resets (gru ignores rnn_start)."""
        return all(kind.honours_start for kind, _ in self._sequence_layers())

    def _sequence_layers(self, models=None):
        """[(kind, module)] of the sequence layers (models/layer_kinds.py) of `models`' networks; default: the live critic and the policy."""
        return [kl for model in models or (self.values[0], self.policy) for net in (model.uni_network, model.embedding_network)
                for kl in net.sequence_layers()]

    def _seed(self, seed: int):
        np.random.seed(seed)
        random.seed(seed + 1)
        torch.manual_seed(seed + 2)
        if torch.cuda.is_available():
            torch.cuda.manual_seed(seed + 3)
            torch.cuda.manual_seed_all(seed + 4)
        self.env.seed(seed + 5)
        self.env.action_space.seed(seed + 6)
        self.env.observation_space.seed(seed + 7)

    def _value_update(self, tau):
        """target <- tau * target + (1 - tau) * online (tau = 0: hard copy)."""
        for value, target in zip(self.values, self.target_values):
            target.copy_weight_from(value, tau)

    def _common_args(self, p, which: str) -> Dict[str, Union[int, float, List[int]]]:
        g = lambda k: getattr(p, f'{which}_{k}')
        return {
            'state_dim': self.obs_dim, 'action_dim': self.act_dim, 'embedding_size': g('embedding_dim'),
            'embedding_hidden': g('embedding_hidden_size'), 'embedding_activations': g('embedding_activations'),
            'embedding_layer_type': g('embedding_layer_type'), 'uni_model_hidden': g('hidden_size'),
            'uni_model_activations': g('activations'), 'uni_model_layer_type': g('layer_type'), 'fix_rnn_length': p.rnn_fix_length,
            'reward_input': p.reward_input, 'last_action_input': not p.no_last_action_input,
            'last_state_input': bool(getattr(p, 'last_state_input', False)),
            'uni_model_input_mapping_dim': g('uni_model_input_mapping_dim'),
            'separate_encoder': bool(getattr(p, 'state_action_encoder', False)),
        }

    def _make_policy_args(self, parameter):
        args = self._common_args(parameter, 'policy')
        if getattr(parameter, 'base_algorithm', 'sac') == 'td3':
            args['sample_std'] = parameter.sample_std
        return args

    def _make_value_args(self, parameter):
        return self._common_args(parameter, 'value')

    # ------------------------------------------------------------------------------------------ environment loop
    def _init_sample_hidden(self):
        # (the reference's branches are swapped - randomize_first_hidden picks the ZERO state, sac.py:143-148; kept)
        if self.parameter.randomize_first_hidden:
            return self.policy.make_init_state(1, self.sample_device)
        return self.policy.make_rnd_init_state(1, self.sample_device)

    def draw_train_task(self):
        """The task of a meta environment's next episode: one draw from the global numpy stream (reference sac.py:150-155)."""
        tasks = self.env_info['train_tasks']
        return tasks[np.random.randint(0, len(tasks))]

    def env_reset(self):
        if hasattr(self.env, 'meta_env_flag') and getattr(self.env, 'n_tasks', None) is not None:
            self.state_np = np.asarray(self.env.reset(self.draw_train_task())).reshape((1, -1))
        else:
            self.state_np = np.asarray(self.env.reset()).reshape((1, -1))
        self.last_action_np = np.zeros((1, self.act_dim))
        self.last_state_np = np.zeros((1, self.obs_dim))
        self.reward_np = np.zeros((1, 1))
        self.sample_hidden = self._init_sample_hidden()
        if self.graph_step is not None:
            self.graph_step.load_hidden(self.sample_hidden)

    def sample_action(self) -> np.ndarray:
        """One policy step on the current rollout state (reference sac.py:319-326) -> sampled action [1, act_dim]; discrete actions:
        the sampled index, int64 [1, 1], whichever way the step is launched."""
        if self.graph_step is not None:
            return self.graph_step(self.state_np, self.last_state_np, self.last_action_np, self.reward_np)[1].reshape(1, -1)
        with torch.no_grad():
            _, _, act_sample, _, self.sample_hidden, _ = self.policy.forward(
                state=n2t_2dim(self.state_np, self.sample_device), lst_state=n2t_2dim(self.last_state_np, self.sample_device),
                lst_action=n2t_2dim(self.last_action_np, self.sample_device), rnn_memory=self.sample_hidden,
                reward=n2t_2dim(self.reward_np, self.sample_device))
        return t2n(act_sample).reshape(1, -1)

    def env_step(self, next_obs, act, reward, done):
        self.last_state_np = self.state_np.copy()
        self.state_np = np.asarray(next_obs).copy().reshape((1, -1))
        if self.discrete_env:                                     # one-hot of the action index (reference :167-169)
            self.last_action_np = np.zeros((1, self.act_dim))
            self.last_action_np[..., int(np.asarray(act).reshape(-1)[0])] = 1
        else:
            self.last_action_np = np.asarray(act).copy().reshape((1, -1))
        self.reward_np = np.array([[reward]])
        if done:
            self.env_reset()

    def _push(self, act_normalized, next_state, reward, done, traj_len):
        self.replay_buffer.mem_push(Transition(
            state=self.state_np, last_state=self.last_state_np, last_action=self.last_action_np, action=act_normalized,
            next_state=np.asarray(next_state).reshape((1, -1)), reward=reward, logp=None, mask=1, done=done,
            timeout=traj_len >= self.max_episode_steps, start=traj_len == 1, reward_input=self.reward_np))

    def warmup(self):
        self.env_reset()
        n = 0
        while n < self.parameter.random_num:
            done, traj_len = False, 0
            while not done:
                act = self.env.action_space.sample()
                next_state, reward, done, _ = self.env.step(act)
                act_n = norm_act(act, self.env.action_space)
                traj_len += 1
                self._push(np.asarray(act_n).reshape((1, -1)), next_state, reward, done, traj_len)
                self.env_step(next_state, act_n, reward, done)
                n += 1
        return n

    def train_one_batch(self) -> Dict:
        return {}

    def update_driver(self):
        """A driver class of the trainer's own that replays its updates as hipGraphs for `train()` - `refusal(alg)` (None: it takes the
        trainer), `driver(alg)` -> an object with `step()` (one `train_one_batch()`) and `close()` -, or None: `GraphedUpdate`, one graph
        per recurring batch shape of a full-trajectory trainer (graphed_update.py)."""
        return None

    def train(self):
        # RESEL_CHECKPOINT_DIR (read here; unset: nothing of this happens): the run state goes there every RESEL_CHECKPOINT_EVERY
        # iterations, and a run that finds a complete state there continues it instead of starting (algorithm/run_state.py)
        ckpt_dir = run_state.checkpoint_dir_from_env()
        ckpt = None
        resumed = False
        if ckpt_dir is not None:
            run_state.refuse_process_groups()
            ckpt = (ckpt_dir, run_state.checkpoint_every_from_env())
            found = run_state.newest_state(ckpt_dir)
            if found is None:
                self.logger(f'no run state in {ckpt_dir}: the run starts from the beginning')
            else:
                self.load_state(found[1])
                resumed = True
                self.logger(f'resumed the run state {found[1]}: {self.iteration} iterations, {self.sample_num} samples and {self.grad_num} updates done')
        if not resumed:
            self.sample_num += self.warmup()
            self.env_reset()
            self.iteration, self.ep_ret, self.ep_len = 0, 0.0, 0
        update = self.train_one_batch
        graphed = None
        if os.environ.get('RESEL_GRAPH_UPDATE', '1') != '0':  # the update as hipGraph replays (`update_driver`)
            from .graphed_update import GraphedUpdate
            driver = self.update_driver() or GraphedUpdate
            why = driver.refusal(self)
            if why:
                self.logger(f'updates are launched eagerly ({why})')
            elif driver is GraphedUpdate:
                # RESEL_GRAPH_BUCKETS (variable-length episodes): 1 = batch shapes bucketed from the first update, auto = once the workload
                # turns out ragged (fixed-length ones never switch), 0 / unset = exact shapes only
                graphed = GraphedUpdate(self, buckets=GraphedUpdate.buckets_from_env())
                update = graphed.step
            else:
                graphed = driver(self)
                update = graphed.step
        # an environment that exists as a kernel (a discrete T-Maze, Wind-v0, Catch: env_utils/device_env.py) is collected on the device
        # (utility/device_collect.py): environment step, transition row and next inputs are the last node of the policy step's graph;
        # RESEL_DEVICE_COLLECT (read here) switches it, every other run keeps the host loop below
        from ..utility.device_collect import DeviceCollector
        why = DeviceCollector.refusal(self)
        # a resumed run captures its graphs at points where the uninterrupted run captured nothing: those captures keep out of the
        # random streams (run_state.generators_kept)
        self.collector = None if why else DeviceCollector(self, keep_generators=resumed)
        if why and not self._collect_refusal_logged:
            self.logger(f'training episodes are collected through the host loop ({why})')
            self._collect_refusal_logged = True
        # a state taken inside an episode: the host loop below finishes that episode (bit for bit the device path), its `env_reset()` is
        # where the collector starts; taken behind `env_reset()`, the collector starts at once
        self._host_episode_open = resumed and self.collector is not None and self.ep_len > 0
        self._collecting = True
        try:
            if resumed and self.graph_step is not None and (self.collector is None or self._host_episode_open):
                with run_state.generators_kept(self.sample_device):
                    self.graph_step.capture(self.obs_dim, self.act_dim)
            self._train_loop(update, self.iteration if resumed else 0, ckpt)
        finally:
            self._collecting = False
            if self.collector is not None:      # rollout mirrors, environment fields and the B = 1 step's state as the host loop leaves them
                self.collector.sync_host()
            if graphed is not None:             # detach the process-wide dropout base: later eager trainers of this process draw from torch's generator again
                graphed.close()

    # ------------------------------------------------------------------------------------------ evaluation
    def eval_refusal(self):
        """Why `train()` does not evaluate the policy (None: it does)."""
        if self.sample_device.type != 'cuda':
            return 'the policy does not sample on a CUDA device (evaluation replays a hipGraph of the policy step)'
        if getattr(self.parameter, 'test_nprocess', 0) * getattr(self.parameter, 'test_nrollout', 0) <= 0:
            return 'test_nprocess * test_nrollout is 0'
        return None

    def evaluate(self):
        """`test_nprocess * test_nrollout` deterministic episodes of the current policy on the evaluation environment (reference
        `eval_inprocess` / `policy_eval`, utility/sample_utility.py:38-131), min(that, 64) environments per graph replay.
        -> {'EpRetTest': [...], 'EpLenTest': [...], ...}.  Touches no global random stream."""
        why = self.eval_refusal()
        if why:
            raise RuntimeError(f'SAC.evaluate: {why}')
        n = self.parameter.test_nprocess * self.parameter.test_nrollout
        if self.evaluator is None:
            self.evaluator = self._make_evaluator()
        return self.evaluator.evaluate(n)

    def _make_evaluator(self):
        from ..utility.policy_eval import BatchedPolicyEval
        n = self.parameter.test_nprocess * self.parameter.test_nrollout
        return BatchedPolicyEval(self.policy, lambda: make_env(self.env_name, self.env_info['seed'])['eval_env'], self.act_dim,
                                 min(n, 64), self.sample_device, seed=self.parameter.seed,
                                 eval_tasks=self.env_info.get('eval_tasks'), discrete=self.discrete_env)

    def _train_loop(self, update, first_iteration=0, ckpt=None):
        why_no_eval = self.eval_refusal()
        if why_no_eval and not self._eval_refusal_logged:
            self.logger(f'the policy is not evaluated during training ({why_no_eval})')
            self._eval_refusal_logged = True
        for it in range(first_iteration, self.parameter.total_iteration):
            test_log = None if why_no_eval else self.evaluate()   # the policy at the start of the iteration (reference :284-300)
            self.policy.train()
            self.policy.to(self.sample_device)
            for _ in range(self.parameter.step_per_iteration):
                if self.collector is not None and not self._host_episode_open:   # the same iteration inside the step's graph; an episode's last step pushes and logs it
                    self.collector.collect_step()
                else:
                    act_sample = self.sample_action()
                    act_env = unorm_act(act_sample[0], self.env.action_space)
                    next_state, reward, done, _ = self.env.step(int(np.asarray(act_env).reshape(-1)[0]) if self.discrete_env else act_env)
                    self.ep_ret += reward
                    self.ep_len += 1
                    self._push(act_sample, next_state, reward, done, self.ep_len)
                    self.env_step(next_state, act_sample, reward, done)
                    if done:
                        self.logger.add_tabular_data(tb_prefix='Train', EpRet=self.ep_ret, EpLength=self.ep_len)
                        self.ep_ret, self.ep_len = 0.0, 0
                        self._host_episode_open = False           # (a resumed run: the collector, when there is one, takes over behind this `env_reset()`)
                if self.sample_num % self.parameter.update_interval == 0 and self.sample_num >= self.parameter.start_train_num:
                    self.logger.add_tabular_data(tb_prefix='train', **update())
                    self.grad_num += 1
                self.sample_num += 1
            if test_log is not None:
                self.logger.add_tabular_data(tb_prefix='performance', **test_log)
            self.logger.log_tabular('iteration', it, tb_prefix='timestep')
            self.logger.log_tabular('timestep', self.sample_num, tb_prefix='timestep')
            self.logger.log_tabular('grad_num', self.grad_num, tb_prefix='timestep')
            self.logger.log_tabular('time', time.time() - self.start_time, tb_prefix='timestep')
            self.logger.dump_tabular()
            if it % 25 == 0:
                self.save()
            self.iteration = it + 1
            if ckpt is not None and (it + 1) % ckpt[1] == 0:
                run_state.write_checkpoint(ckpt[0], it + 1, self.save_state)

    # ------------------------------------------------------------------------------------------ checkpoints
    def save(self, model_dir=None):
        path = os.path.join(self.logger.output_dir, 'model') if model_dir is None else model_dir
        self.policy.save(path)
        for i in range(len(self.values)):
            self.values[i].save(path, index=f'{i}')
            self.target_values[i].save(path, index=f'{i}-target')
        torch.save(self.log_sac_alpha, os.path.join(path, 'log_sac_alpha.pt'))

    def load(self, model_dir=None, load_policy=True, load_value=True):
        path = os.path.join(self.logger.output_dir, 'model') if model_dir is None else model_dir
        if load_policy:
            self.policy.load(path, map_location=self.sample_device)
            if self.graph_step is not None:
                self.graph_step.invalidate()
            if self.evaluator is not None:
                self.evaluator.invalidate()
        if load_value:
            for i in range(len(self.values)):
                self.values[i].load(path, index=f'{i}', map_location=self.device)
                self.target_values[i].load(path, index=f'{i}-target', map_location=self.device)
        # in place: optimizer_alpha holds this tensor (rebinding it, as the reference does, silently freezes the temperature)
        with torch.no_grad():
            self.log_sac_alpha.copy_(torch.load(os.path.join(path, 'log_sac_alpha.pt'), map_location=self.device))

    # ------------------------------------------------------------------------------------------ run state (algorithm/run_state.py)
    def _state_networks(self):
        nets = {'policy': self.policy}
        for i, (value, target) in enumerate(zip(self.values, self.target_values)):
            nets[f'value{i}'], nets[f'target_value{i}'] = value, target
        if getattr(self, 'target_policy', None) is not None:      # the full-trajectory trainers; TD3 updates it
            nets['target_policy'] = self.target_policy
        return nets

    def _state_optimizers(self):
        return dict({'policy': self.optimizer_policy}, **{f'value{i}': opt for i, opt in enumerate(self.optimizers_value)})

    def state_fingerprint(self) -> dict:
        """What must be equal between the trainer that wrote a run state and the one that loads it; a mismatch names its key."""
        p, ring = self.parameter, self.replay_buffer
        out = dict(env_name=p.env_name, alg_name=p.alg_name, base_algorithm=self.base_algorithm, seed=int(p.seed), obs_dim=int(self.obs_dim),
                   act_dim=int(self.act_dim), trainer=type(self).__name__)
        for which in ('policy', 'value'):
            for key in ('embedding_layer_type', 'embedding_hidden_size', 'layer_type', 'hidden_size'):
                out[f'{which}_{key}'] = list(getattr(p, f'{which}_{key}'))
        for name, net in self._state_networks().items():
            out[f'numel_{name}'] = int(net.store.numel)
        has_layout = ring.memory_buffer is not None               # (fixed by the first trajectory: a fresh trainer has none to compare)
        out['ring_width'] = int(ring.width) if has_layout else None
        out['ring_name2range'] = {k: list(v) for k, v in ring.name2range.items()} if has_layout else None
        return out

    def _collect_state(self):
        """-> (manifest, host payload, tensor payload) of this trainer as it stands (the ring goes separately).  Reads only."""
        dev, cuda = self.sample_device, self.sample_device.type == 'cuda'
        if cuda:
            torch.cuda.synchronize(dev)
        cpu = lambda t: t.detach().cpu().clone()
        ev = self.evaluator
        subset_rng = getattr(self, '_subset_rng', None)
        host = dict(
            python_random=random.getstate(), numpy_random=np.random.get_state(),
            subset_rng=None if subset_rng is None else subset_rng.get_state(),
            env=self.env, state_np=self.state_np, last_state_np=self.last_state_np, last_action_np=self.last_action_np, reward_np=self.reward_np,
            ep_ret=self.ep_ret, ep_len=self.ep_len, sample_num=self.sample_num, grad_num=self.grad_num, iteration=self.iteration,
            elapsed=time.time() - self.start_time, pending=list(self.replay_buffer.memory),
            optimizer_steps={name: opt.step_count for name, opt in self._state_optimizers().items()},
            evaluator=None if ev is None else dict(rs=ev.rs.get_state(), env_seeds=list(ev.env_seeds), envs=ev.envs))
        hidden = self.graph_step._hidden if self.graph_step is not None else self.sample_hidden
        tensors = dict(
            stores={name: cpu(net.store.flat) for name, net in self._state_networks().items()},
            moments={name: dict(m=cpu(opt.m), v=cpu(opt.v)) for name, opt in self._state_optimizers().items()},
            log_sac_alpha=cpu(self.log_sac_alpha), optimizer_alpha=self.optimizer_alpha.state_dict(),
            q_guard=cpu(self.Q_guard.state) if hasattr(self, 'Q_guard') else None,
            torch_cpu_rng=torch.get_rng_state(), device_rng=torch.cuda.get_rng_state(dev) if cuda else None,
            hidden=run_state.hidden_to_host(hidden))
        manifest = dict(iteration=self.iteration, sample_num=self.sample_num, grad_num=self.grad_num, fingerprint=self.state_fingerprint())
        return manifest, host, tensors

    def save_state(self, path):
        """The whole run state into the directory `path` (algorithm/run_state.py): networks, optimizers, guard, counters, the ring's
        occupied rows, every random stream, the environment, the open episode with its recurrent state, the evaluator.  The trainer goes
        on afterwards exactly as if nothing had been written.  `save()` is something else: the reference's model files."""
        run_state.refuse_process_groups()
        ring = self.replay_buffer
        live = self._collecting and self.collector is not None    # the open episode is on the device: fetch the host loop's view of it
        pending = ring.memory
        try:
            if live:
                self.collector.sync_host()
            manifest, host, tensors = self._collect_state()
            return run_state.write_state(path, manifest, ring, host, tensors)
        finally:
            if live:                                              # `sync_host()` left the episode's transitions pending: `push_rows` would refuse
                ring.memory = pending

    def load_state(self, path):
        """A state that `save_state` wrote, into a trainer built from the same `Parameter`: afterwards this trainer is the one that
        wrote it.  Everything is read and checked before anything is touched; `run_state.RunStateMismatch` names what does not fit."""
        run_state.refuse_process_groups()
        manifest, ring_st, host, tensors = run_state.read_state(path)
        current = self.state_fingerprint()
        run_state.check_fingerprint(manifest['fingerprint'], current)
        nets, opts = self._state_networks(), self._state_optimizers()
        for name, net in nets.items():                            # (the fingerprint compared the sizes; the payload itself)
            if tensors['stores'][name].shape != net.store.flat.shape:
                raise run_state.RunStateMismatch(f'stores[{name}].shape', tuple(tensors['stores'][name].shape), tuple(net.store.flat.shape))
        if set(host['optimizer_steps']) != set(opts) or (tensors['q_guard'] is None) != (not hasattr(self, 'Q_guard')):
            raise run_state.RunStateMismatch('optimizers', sorted(host['optimizer_steps']), sorted(opts))
        self._apply_state(ring_st, host, tensors)

    @torch.no_grad()
    def _apply_state(self, ring_st, host, tensors):
        dev, cuda = self.sample_device, self.sample_device.type == 'cuda'
        for name, net in self._state_networks().items():          # in place: parameters, optimizers and graphs hold these buffers
            net.store.flat.copy_(tensors['stores'][name])
            net.store._amax = None
        for name, opt in self._state_optimizers().items():
            opt.m.copy_(tensors['moments'][name]['m'])
            opt.v.copy_(tensors['moments'][name]['v'])
            opt.step_count = int(host['optimizer_steps'][name])
        self.log_sac_alpha.copy_(tensors['log_sac_alpha'])
        self.optimizer_alpha.load_state_dict(tensors['optimizer_alpha'])
        if tensors['q_guard'] is not None:
            self.Q_guard.state.copy_(tensors['q_guard'])
        self.sample_num, self.grad_num, self.iteration = int(host['sample_num']), int(host['grad_num']), int(host['iteration'])
        self.start_time = time.time() - float(host['elapsed'])
        run_state.load_ring(self.replay_buffer, ring_st, host['pending'])
        self.env.__dict__.clear()                                 # in place: `env_info` and whoever else holds the object see the loaded one
        self.env.__dict__.update(host['env'].__dict__)
        self.state_np, self.last_state_np = host['state_np'], host['last_state_np']
        self.last_action_np, self.reward_np = host['last_action_np'], host['reward_np']
        self.ep_ret, self.ep_len = host['ep_ret'], int(host['ep_len'])
        saved_hidden = tensors['hidden']
        if saved_hidden is not None:
            # `sample_hidden` is what `env_reset()` made; behind a reset it equals the step's state, and nobody reads it elsewhere
            self.sample_hidden = self.policy.make_init_state(1, dev)
            run_state.hidden_from_host(self.sample_hidden, saved_hidden, dev, in_place=False)
            if self.graph_step is not None:
                self.graph_step.load_hidden(None)
                run_state.hidden_from_host(self.graph_step._hidden, saved_hidden, dev, in_place=True)
                if any(tag == 'kv' for tag, _ in saved_hidden):   # the KV caches are new tensors: a graph captured earlier reads the old ones
                    self.graph_step.invalidate()
        ev = host['evaluator']
        self.evaluator = None
        if ev is not None:                                        # the evaluator continues its private streams instead of drawing new seeds
            self.evaluator = self._make_evaluator()
            self.evaluator.rs.set_state(ev['rs'])
            self.evaluator.env_seeds, self.evaluator.envs = list(ev['env_seeds']), ev['envs']
        if hasattr(self, '_subset_rng'):
            self._subset_rng = None
            if host['subset_rng'] is not None:
                self._subset_rng = np.random.RandomState()
                self._subset_rng.set_state(host['subset_rng'])
        random.setstate(host['python_random'])
        np.random.set_state(host['numpy_random'])
        torch.set_rng_state(tensors['torch_cpu_rng'])
        if cuda and tensors['device_rng'] is not None:
            torch.cuda.set_rng_state(tensors['device_rng'], dev)
