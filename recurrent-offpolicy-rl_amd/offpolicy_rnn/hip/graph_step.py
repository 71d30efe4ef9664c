"""hipGraph replay of the per-environment-step policy forward (reference algorithm/sac.py:319-326).

Between two updates the outer loop calls `policy.forward` on ONE token per environment; at batch 1 that is 40-150
kernels of a few microseconds each, so the step is bound by host launch overhead, not by the GPU.  `GraphedPolicyStep`
captures the whole step once - encoders, the recurrent layer's state update, MLP head, action sampling, and the copy of
the new recurrent state over the old one - and replays it with one `hipGraphLaunch`:

  * the four inputs live in one pinned host block and one device block (a single H2D copy per step);
  * recurrent state is held in static device tensors that the graph updates in place; a cgpt KV cache takes its
    position from a device counter (`InferenceParams.device_offset`) that the graph advances;
  * the outputs (mean | sample | log-prob) land in one device block, copied back with a single D2H.

A categorical policy (discrete actions, `policy.categorical`) replays the same way.  Its last-action input is the one-hot of the
previous index, so the input block is unchanged; its output block is [B, 2 + A] = (mode | sample | logp[A]), which the head kernel
(`ops.categorical_step`) fills directly - the indices travel as fp32 and come back as int64.

`row_reset=True` lets the B rows run episodes that start at different steps (batched evaluation, utility/policy_eval.py): the input
block carries one reset flag per row, the FIRST node of the graph (`ops.step_state_reset`) zeroes the recurrent state and the cgpt
position of the flagged rows, and every cgpt KV cache takes one position per row (`device_offset` int32 [B],
`resel_attn_decode_rows`).  The object issues the resets, so it mirrors the per-row positions on the host and refuses a step that
would overrun a row's cache.

`after_step=hook` appends work to the captured step: `hook(self)` runs as the last thing of the forward - in the warm-up and in the
capture - and sees `_in_dev`, `_flags_dev` and `_out_dev`.  An environment that exists as a kernel (utility/policy_eval.py `DeviceEnvEval`,
`ops.tmaze_step`) turns the output block into the next step's input block there; `capture()` then records the graph without a first host
call and `replay_device()` replays it with no copy and no synchronise.  Without a hook the captured graph is what it was.

Parameters are read through their storage, so in-place optimiser steps are seen by the next replay; call
`invalidate()` after anything that re-allocates them (`load`, `.to`)."""
import gc
from typing import Callable, Optional

import numpy as np
import torch

from ..models.RNNHidden import RNNHidden
from . import ops


class GraphedPolicyStep:
    def __init__(self, policy, device, batch_size: int = 1, warmup: int = 2, row_reset: bool = False,
                 after_step: Optional[Callable[['GraphedPolicyStep'], None]] = None):
        if torch.device(device).type != 'cuda':
            raise RuntimeError('GraphedPolicyStep replays a hipGraph: it needs a CUDA (ROCm) device')
        self.policy, self.device, self.B, self._warmup = policy, torch.device(device), batch_size, warmup
        self.row_reset = bool(row_reset)
        self.after_step = after_step                              # last thing in the captured step (None: the graph ends at the state copies)
        self.categorical = bool(getattr(policy, 'categorical', False))
        self._row_pos = np.zeros(batch_size, dtype=np.int64)      # row_reset: host mirror of the per-row cgpt positions
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._hidden: Optional[RNNHidden] = None
        self._layout = None

    # ------------------------------------------------------------------------------------------ state
    def invalidate(self):
        self._graph = None

    def _counters(self):
        return [h for h in self._hidden._data if not torch.is_tensor(h) and not isinstance(h, tuple)]

    def load_hidden(self, hidden: Optional[RNNHidden] = None):
        """Start of an episode: overwrite the static recurrent state with `hidden` (None: the zero state)."""
        if self._hidden is None:
            self._hidden = self.policy.make_init_state(self.B, self.device)
            for ip in self._counters():
                ip.device_offset = torch.zeros(self.B if self.row_reset else 1, dtype=torch.int32, device=self.device)
        self._row_pos[:] = 0
        for i, h in enumerate(self._hidden._data):
            src = None if hidden is None else hidden[i]
            if torch.is_tensor(h):
                h.zero_() if src is None else h.copy_(src)
            elif isinstance(h, tuple):
                for j, t in enumerate(h):
                    t.zero_() if src is None else t.copy_(src[j])
            else:                                        # KV-cache handle: stale rows beyond the position are never read
                h.reset(h.max_seqlen, h.max_batch_size)

    # ------------------------------------------------------------------------------------------ capture
    def _state_tensors(self):
        return [t for h in self._hidden._data for t in (h if isinstance(h, tuple) else (h,)) if torch.is_tensor(t)]

    def _forward(self):
        o, a = self._layout['obs'], self._layout['act']
        if self.row_reset:                      # first node: flagged rows start from the zero state at position 0
            ops.step_state_reset(self._flags_dev, self._state_tensors(), [ip.device_offset for ip in self._counters()])
        x = self._in_dev.unsqueeze(1)           # [B, 1, .]: B environments, one token each (a 2-D input would be ONE sequence of length B)
        state, lst_state = x[..., :o], x[..., o:2 * o]
        lst_action, reward = x[..., 2 * o:2 * o + a], x[..., 2 * o + a:2 * o + a + 1]
        if self.categorical:                    # the policy's forward with the head writing (mode | sample | logp) into the block
            emb_in = self.policy.get_embedding_input(state, lst_state, lst_action, reward)
            logits, new_hidden, _, _ = self.policy.meta_forward(emb_in, state, self._hidden, False)
            self.policy.step_head(logits, out=self._out_dev)
        else:
            mean, _, sample, logp, new_hidden, _ = self.policy.forward(state=state, lst_state=lst_state, lst_action=lst_action,
                                                                       rnn_memory=self._hidden, reward=reward)
            self._out_dev[:, :a].copy_(mean.reshape(self.B, a))
            self._out_dev[:, a:2 * a].copy_(sample.reshape(self.B, a))
            self._out_dev[:, 2 * a:].copy_(logp.reshape(self.B, -1)[:, :1])
        for i, h in enumerate(self._hidden._data):
            if torch.is_tensor(h):                   # (conv1d / mamba return the reference's [B, 1, W]: the same memory layout as [1, B, W])
                h.copy_(new_hidden[i].reshape(h.shape))
            elif isinstance(h, tuple):
                for j, t in enumerate(h):
                    t.copy_(new_hidden[i][j].reshape(t.shape))
        if self.after_step is not None:              # e.g. an environment step that turns `_out_dev` into the next `_in_dev` / `_flags_dev`
            self.after_step(self)

    def _capture(self, obs_dim: int, act_dim: int):
        self._layout = dict(obs=obs_dim, act=act_dim)
        width = 2 * obs_dim + act_dim + 1
        # row_reset: B more words behind the rows - the reset flags (int32 through a view), still one block and one H2D
        words = self.B * width + (self.B if self.row_reset else 0)
        self._blk_host = torch.zeros(words, dtype=torch.float32).pin_memory()
        self._blk_dev = torch.zeros(words, dtype=torch.float32, device=self.device)
        self._in_host = self._blk_host[:self.B * width].view(self.B, width)
        self._in_dev = self._blk_dev[:self.B * width].view(self.B, width)
        if self.row_reset:
            self._flags_host = self._blk_host[self.B * width:].view(torch.int32)
            self._flags_dev = self._blk_dev[self.B * width:].view(torch.int32)
        out_width = 2 + act_dim if self.categorical else 2 * act_dim + 1
        self._out_dev = torch.zeros((self.B, out_width), dtype=torch.float32, device=self.device)
        self._out_host = torch.zeros((self.B, out_width), dtype=torch.float32).pin_memory()
        if self._hidden is None:
            self.load_hidden(None)
        keep = [h.clone() if torch.is_tensor(h) else None for h in self._hidden._data]
        counts = [ip.seqlen_offset for ip in self._counters()]
        if self.row_reset:                      # the host integer (the furthest row) must not stop the warm-up: a row that has filled its cache
            for ip in self._counters():         # decodes NaN there and writes nothing (resel_attn_decode_rows), and every state comes back below
                ip.seqlen_offset = 0
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side), torch.no_grad():   # eager warm-up: lazy allocations (KV caches, slopes, GEMM handles)
            for _ in range(self._warmup):
                self._forward()
        torch.cuda.current_stream(self.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        # No cyclic garbage collection while the stream captures (as `GraphedUpdate._record`): a dead captured graph that only the collector
        # can free - a dropped trainer or evaluator is a cycle through its step object and the `after_step` hook - synchronises the device
        # in its destructor, which a capturing stream refuses, and the process aborts.  When the collector runs is the allocator's choice.
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.no_grad(), torch.cuda.graph(graph):
                self._forward()
        finally:
            if gc_was_on:
                gc.enable()
        # the warm-up really ran (and capture advanced the host counters): put the episode state back
        for h, k in zip(self._hidden._data, keep):
            if k is not None:
                h.copy_(k)
        for ip, c in zip(self._counters(), counts):
            ip.seqlen_offset = c
            if self.row_reset:
                ip.device_offset.copy_(torch.from_numpy(self._row_pos.astype(np.int32)))
            else:
                ip.device_offset.fill_(c)
        self._graph = graph

    def capture(self, obs_dim: int, act_dim: int):
        """Capture for rows of (obs_dim, act_dim) without a first host call (a no-op when that graph exists)."""
        if self._graph is None or self._layout != dict(obs=obs_dim, act=act_dim):
            with torch.no_grad():
                self._capture(obs_dim, act_dim)

    def replay_device(self):
        """Replay only: no H2D, no D2H, no synchronise.  The inputs are what is in `_in_dev` / `_flags_dev` (an `after_step` hook
        wrote them); the caller owns the host mirrors of the cgpt positions (`_row_pos`, `seqlen_offset`) and the full-cache check."""
        self._graph.replay()

    # ------------------------------------------------------------------------------------------ step
    @torch.no_grad()
    def __call__(self, state, lst_state, lst_action, reward, reset=None):
        """Numpy / CPU rows [B, dim] in -> (action_mean, action_sample, log_prob) as numpy rows; a categorical policy takes one-hot
        last actions [B, A] and returns (mode int64 [B, 1], sample int64 [B, 1], logp float32 [B, A]).  One H2D, one graph launch,
        one D2H.  reset (row_reset=True only): bool / int [B], non-zero = this row starts an episode from the zero state on this step."""
        if reset is not None and not self.row_reset:
            raise ValueError('reset= needs GraphedPolicyStep(..., row_reset=True); without it use load_hidden() for a joint reset')
        state = np.asarray(state, dtype=np.float32).reshape(self.B, -1)
        lst_action = np.asarray(lst_action, dtype=np.float32).reshape(self.B, -1)
        o, a = state.shape[1], lst_action.shape[1]
        if self._graph is None or self._layout != dict(obs=o, act=a):
            self._capture(o, a)
        if self.row_reset:
            flags = np.zeros(self.B, dtype=np.int32) if reset is None else (np.asarray(reset).reshape(self.B) != 0).astype(np.int32)
            pos = np.where(flags != 0, 0, self._row_pos)            # the position each row decodes at on this step
            for ip in self._counters():
                full = np.nonzero(pos >= ip.max_seqlen)[0]
                if full.size:
                    raise RuntimeError(f'cgpt rollout: KV cache is full (row {int(full[0])}: {int(pos[full[0]])} tokens, max_seqlen {ip.max_seqlen})')
            self._flags_host.numpy()[:] = flags
        else:
            for ip in self._counters():
                if ip.seqlen_offset >= ip.max_seqlen:
                    raise RuntimeError(f'cgpt rollout: KV cache is full ({ip.seqlen_offset} tokens, max_seqlen {ip.max_seqlen})')
        buf = self._in_host.numpy()
        buf[:, :o] = state
        buf[:, o:2 * o] = np.asarray(lst_state, dtype=np.float32).reshape(self.B, -1)
        buf[:, 2 * o:2 * o + a] = lst_action
        buf[:, 2 * o + a:] = np.asarray(reward, dtype=np.float32).reshape(self.B, 1)
        self._blk_dev.copy_(self._blk_host, non_blocking=True)
        self._graph.replay()
        self._out_host.copy_(self._out_dev, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        if self.row_reset:
            self._row_pos = pos + 1
            for ip in self._counters():         # the host integer follows the furthest row
                ip.seqlen_offset = int(self._row_pos.max())
        else:
            for ip in self._counters():
                ip.seqlen_offset += 1
        out = self._out_host.numpy()
        if self.categorical:
            return out[:, :1].astype(np.int64), out[:, 1:2].astype(np.int64), out[:, 2:].copy()
        return out[:, :a].copy(), out[:, a:2 * a].copy(), out[:, 2 * a:].copy()
