"""Training rollouts of an environment that exists as a kernel (a discrete T-Maze, Wind-v0, Catch) on the device: one graph replay per environment step, one copy back per episode.

`SAC._train_loop` pays one H2D, one replay, one D2H, one synchronise, a Python `TMaze.step`, a `Transition` / `mem_push` and the numpy
bookkeeping of `env_step` for every environment step.  A T-Maze episode has a fixed length, the ring only admits whole trajectories and the
categorical head samples from the device generator, so none of that has to reach the host before the episode ends: `DeviceCollector` appends
`ops.tmaze_collect_step` (csrc/env_step.hip) to the policy step's graph as its last node.  The kernel reads the SAMPLED index, steps the
environment, writes the transition row the ring stores into an episode block and turns the input block into the next step's input.

Per step the host issues `replay_device()` and counts; at an episode's last step it copies the episode block, the return and the
environment words back with ONE D2H and ONE synchronise, hands the rows to `MemoryArray.push_rows`, logs the episode, draws the next goal
side from the environment's own stream, starts the episode with one init launch outside the graph and loads a fresh recurrent state - the
host loop's order of side effects, which fixes every random stream.  Ring, logs, generators and parameters equal the host loop's bit for bit
(tests/test_device_collect_gpu.py).  `RESEL_DEVICE_COLLECT` switches it (read at `train()`).

Wind-v0 (continuous actions, `ops.wind_collect_step`) goes the same way: the kernel reads the Gaussian head's SAMPLED action, and the next
episode's task is one draw from the global numpy stream where the host loop's `env_reset()` makes it (tests/test_wind_env_gpu.py).  What
differs between the environments lives in their records (env_utils/device_env.py).  Catch (`ops.catch_collect_step`) is the T-Maze's case with a
49-wide observation and a payload of 80 words: nothing here knows a width."""
import os

import numpy as np
import torch

from ..env_utils.device_env import device_env_kind

DEVICE_COLLECT_DEFAULT = '1'                               # RESEL_DEVICE_COLLECT when the variable is not set (measured: profiles/r20_device_collect.md, profiles/r22_wind_env.md)


def device_collect_enabled() -> bool:
    return os.environ.get('RESEL_DEVICE_COLLECT', DEVICE_COLLECT_DEFAULT) != '0'


class DeviceCollector:
    """The environment loop of `alg.train()` for an environment that exists as a kernel, with the environment, the transition rows and the
    next inputs inside the graphed policy step.  Built behind the warm-up and `env_reset()`: the first episode is the one `env_reset()` began
    (the environment's current goal side / wind, no extra draw).  `collect_step()` is one iteration of the loop up to (not including) the
    update; `sync_host()` writes the rollout state back into the trainer and the environment object.  Everything that depends on the
    environment comes from its record (`self.kind`, env_utils/device_env.py)."""

    @staticmethod
    def refusal(alg):
        """Why `alg.train()` collects through the host loop (None: it collects on the device)."""
        kind = device_env_kind(alg.env)
        if kind is None:
            return 'the environment has no device step (a T-Maze with discrete actions, Wind-v0 and Catch up to 40 runs have one)'
        if alg.sample_device.type != 'cuda' or not kind.policy_ok(alg.policy):
            return f'the policy is not {kind.policy_words} sampling on a CUDA device'
        if os.environ.get('RESEL_GRAPH_ROLLOUT', '1') == '0':
            return 'RESEL_GRAPH_ROLLOUT=0'
        if not device_collect_enabled():
            return 'RESEL_DEVICE_COLLECT=0'
        if alg.replay_buffer.memory_buffer is None:
            return 'the ring has no column layout yet (no warm-up trajectory)'
        return None

    def __init__(self, alg, keep_generators: bool = False):
        """keep_generators: the capture in `_begin` leaves every random stream as it found it - a run resumed from a run state
        (algorithm/run_state.py) captures where the uninterrupted run, which captured at its first step, draws nothing."""
        from ..hip.graph_step import GraphedPolicyStep
        self.alg, self.env, self.device = alg, alg.env, alg.sample_device
        self.keep_generators = bool(keep_generators)
        self.kind = kind = device_env_kind(self.env)
        self.cfg = self.env.device_config()
        self.T, self.obs_dim, self.act_dim = kind.episode_length(self.cfg), kind.obs_dim, kind.act_dim
        assert alg.obs_dim == self.obs_dim and alg.act_dim == self.act_dim
        ring = alg.replay_buffer
        self.name2range, self.width = dict(ring.name2range), int(ring.width)
        self.step = GraphedPolicyStep(alg.policy, self.device, batch_size=1, after_step=self._env_step)
        # one device block and one D2H per episode: return fp64 [1] | the row's environment state | episode rows fp32 [1, T, width]
        head = 8 + kind.state_bytes
        self._res_dev = torch.zeros(head + 4 * self.T * self.width, dtype=torch.uint8, device=self.device)
        self._res_host = torch.zeros(self._res_dev.numel(), dtype=torch.uint8).pin_memory()
        self._ret = self._res_dev[:8].view(torch.float64)
        self._env_state = kind.state_views(self._res_dev[8:head], 1)       # zeros: the row is stopped until the first init
        self._traj = self._res_dev[head:].view(torch.float32).view(1, self.T, self.width)
        res = self._res_host.numpy()
        self._ret_np, self._state_np = res[:8].view(np.float64), res[8:head]
        self._rows_np = res[head:].view(np.float32).reshape(self.T, self.width)
        self._payload_host = torch.zeros((1, kind.payload_width), dtype=kind.payload_dtype).pin_memory()
        self._payload_dev = torch.zeros((1, kind.payload_width), dtype=kind.payload_dtype, device=self.device)
        self._counters = []
        self.t = 0                                         # steps of the running episode that have been replayed
        self.started = False
        self.replays = self.episode_syncs = self.init_launches = 0

    # ------------------------------------------------------------------------------------------ graph side
    def _launch(self, init: bool):
        from ..hip import ops
        step = self.step
        self.kind.collect_step(ops, self.cfg, self.name2range, init, self.kind.action(step._out_dev, True), self._payload_dev, self._env_state,
                               self._ret, self._traj, self.alg.max_episode_steps, step._in_dev)

    def _env_step(self, step):
        self._launch(False)

    def _init_episode(self, payload):
        self._payload_host[0] = torch.as_tensor(payload, dtype=self.kind.payload_dtype)
        self._payload_dev.copy_(self._payload_host, non_blocking=True)
        self._launch(True)
        self.init_launches += 1
        self.t = 0

    def _begin(self):
        """The first sample behind the warm-up, where the host loop captures its step: capture (the warm-up passes run the hook on a
        stopped row, so they see the zero input block the host loop's capture sees), then the episode `env_reset()` began."""
        assert self.kind.behind_reset(self.env), 'the collector starts behind env_reset()'
        self.step.load_hidden(self.alg.sample_hidden)
        if self.keep_generators:
            from ..algorithm.run_state import generators_kept
            with generators_kept(self.device):
                self.step.capture(self.obs_dim, self.act_dim)
        else:
            self.step.capture(self.obs_dim, self.act_dim)
        self._counters = self.step._counters()
        self._init_episode(self.kind.current_payload(self.env))
        self.started = True

    # ------------------------------------------------------------------------------------------ the loop body
    @torch.no_grad()
    def collect_step(self):
        if not self.started:
            self._begin()
        for ip in self._counters:                          # what `GraphedPolicyStep.__call__` raises at the step that would overrun
            if ip.seqlen_offset >= ip.max_seqlen:
                raise RuntimeError(f'cgpt rollout: KV cache is full ({ip.seqlen_offset} tokens, max_seqlen {ip.max_seqlen})')
        self.step.replay_device()
        self.replays += 1
        for ip in self._counters:
            ip.seqlen_offset += 1
        self.t += 1
        if self.t >= self.T:
            self._finish_episode()

    def _finish_episode(self):
        alg = self.alg
        self._res_host.copy_(self._res_dev, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        self.episode_syncs += 1
        length, running = self.kind.finished(self._state_np)
        assert length == self.T and not running, (length, self.T, self._state_np.tolist())
        alg.replay_buffer.push_rows(self._rows_np[:length])
        alg.logger.add_tabular_data(tb_prefix='Train', EpRet=float(self._ret_np[0]), EpLength=length)
        self._init_episode(self.kind.next_payload(alg))     # `env_reset()`: the draw of the next episode, then the fresh recurrent state
        alg.sample_hidden = alg._init_sample_hidden()
        self.step.load_hidden(alg.sample_hidden)

    # ------------------------------------------------------------------------------------------ back to the host loop's state
    @torch.no_grad()
    def sync_host(self):
        """On return from `train()`: the trainer's rollout mirrors, the environment object's fields, the B = 1 step's recurrent state,
        the open episode's running return and length and the ring's pending transitions (that episode) hold what the host loop would
        have left there.  The collector itself is not changed: it may go on afterwards, once the pending transitions are taken out of the
        ring again (`SAC.save_state`)."""
        if not self.started:
            return
        alg, env, o, a = self.alg, self.env, self.obs_dim, self.act_dim
        row = self.step._in_dev[0].cpu().numpy()            # (synchronises)
        alg.ep_ret, alg.ep_len = float(self._ret.cpu()[0]), self.t
        state, last_state, last_action = self.kind.sync_env(env, self._env_state, row, o, a)
        alg.state_np = state
        if self.t == 0:                                    # behind `env_reset()`
            alg.last_state_np, alg.last_action_np, alg.reward_np = np.zeros((1, o)), np.zeros((1, a)), np.zeros((1, 1))
        else:
            alg.last_state_np, alg.last_action_np = last_state, last_action
            alg.reward_np = np.array([[env.last_reward()]])  # the double the float32 in the block was rounded from
            ring = alg.replay_buffer                       # the open episode's transitions wait in the ring's `memory`, as `mem_push` leaves them
            rows = self._traj[0, :self.t].cpu().numpy()
            ring.memory = [ring.array_to_transition(rows[k:k + 1].copy()) for k in range(self.t)]
        if alg.graph_step is not None:                     # the recurrent state mid-episode lives in the step object, as in the host loop
            alg.graph_step.load_hidden(self.step._hidden)
            for dst, src in zip(alg.graph_step._counters(), self.step._counters()):
                dst.key_value_memory_dict = {k: v.clone() for k, v in src.key_value_memory_dict.items()}
                dst.seqlen_offset = src.seqlen_offset
                dst.device_offset.fill_(src.seqlen_offset)
