"""`gru` layer: torch.nn.GRU's parameters and formula, recurrence on the HIP step kernels.

The reference builds `torch.nn.GRU(in, out, batch_first=True)` (rnn_base.py:59,247) and calls it without reset or
mask handling (:453-454).  This module keeps the parameter names of nn.GRU (`weight_ih_l0`, `weight_hh_l0`,
`bias_ih_l0`, `bias_hh_l0`) so checkpoints load unchanged; the input projection is hoisted out of the time loop as
one GEMM over all B*T' tokens, the recurrence runs in `ops.gru_seq`."""
import torch
import torch.nn as nn

from ..hip import ops


class GRU(nn.Module):
    def __init__(self, input_size: int, hidden_size: int, batch_first: bool = True):
        super().__init__()
        assert batch_first
        self.input_size, self.hidden_size = input_size, hidden_size
        k = 1.0 / hidden_size ** 0.5
        self.weight_ih_l0 = nn.Parameter(torch.empty(3 * hidden_size, input_size).uniform_(-k, k))
        self.weight_hh_l0 = nn.Parameter(torch.empty(3 * hidden_size, hidden_size).uniform_(-k, k))
        self.bias_ih_l0 = nn.Parameter(torch.empty(3 * hidden_size).uniform_(-k, k))
        self.bias_hh_l0 = nn.Parameter(torch.empty(3 * hidden_size).uniform_(-k, k))

    def recurrence_job(self, x, hidden=None):
        """The hoisted input projection and what the recurrence needs besides: (gi, W_hh, b_hh, h0), the arguments of `ops.gru_seq`
        and the head of an `ops.gru_seq_multi` job (RNNBase's lockstep walk runs several networks' recurrences in one launch)."""
        H = self.hidden_size
        Hk, native = ops.gru_width_plan(H) if x.is_cuda else (H, True)       # the kernels' widths bind GPU passes only
        h0 = None if hidden is None else hidden[0]
        if native:
            return ops.linear(x, self.weight_ih_l0, self.bias_ih_l0), self.weight_hh_l0, self.bias_hh_l0, h0
        # a width the kernels have no instantiation for: the job runs at Hk on zero-padded PARAMETERS (one node, one launch each way),
        # so the projection writes gi [B, T, 3Hk] directly and only `finish` touches an activation.  The parameters themselves - what the
        # flat store, the optimizer and the checkpoints see - keep nn.GRU's shapes.
        w_ih, b_ih, w_hh, b_hh = ops.gru_pad_params(self.weight_ih_l0, self.bias_ih_l0, self.weight_hh_l0, self.bias_hh_l0, Hk)
        return ops.linear(x, w_ih, b_ih), w_hh, b_hh, ops.gru_pad_state(h0, H, Hk)

    def finish(self, y):
        """y: the recurrence's output for `recurrence_job` - at the kernel width, narrowed here to the true units."""
        if y.shape[-1] != self.hidden_size:
            y = ops.gru_narrow(y, self.hidden_size, y.shape[-1])
        return y, y[:, -1:, :].transpose(0, 1)

    def forward(self, x, hidden=None):
        """x [B, T, in]; hidden [1, B, H] -> (y [B, T, H], last hidden [1, B, H])."""
        return self.finish(ops.gru_seq(*self.recurrence_job(x, hidden)))
