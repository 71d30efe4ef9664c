"""`econv1d[_K]-<E>` layer - E depthwise causal convolutions over time, one per member of an `efc-<E>` ensemble critic (reference
offpolicy_rnn/models/conv1d/econv1d.py:3-87).  No activation and no feed-forward block inside the layer.

Parameters as the reference's nn.Conv1d over E * D grouped channels: `conv1d.weight` [E * D, 1, K], `conv1d.bias` [E * D]; channel e D + d
belongs to member e.  Input: member-major [E, B, T, D], or a shared [B, T, D] which every member reads; `mask` is shared.
State [B, 1, E (K - 1) D] viewed [B, E, K - 1, D]: each member's last K - 1 masked inputs.
RESEL_MEMBER_SEQ (read per call) - 1: all members in ONE launch each way (`ops.member_conv1d`; a shared input without a carried window
is read in place by every member and its gradient summed over the members in a fixed order); 0: E launches of `ops.causal_conv1d_fn`."""
import torch
import torch.nn as nn

from ...hip import ops


class EConv1d(nn.Module):
    def __init__(self, in_channels, out_channels, num_ensemble, d_conv=4, bias=True):
        super().__init__()
        assert in_channels == out_channels, f'econv1d requires input_dim == output_dim, while got {in_channels} and {out_channels}'
        self.in_channels, self.out_channels, self.num_ensemble, self.d_conv = in_channels, out_channels, num_ensemble, d_conv
        ch = in_channels * num_ensemble
        self.conv1d = nn.Conv1d(ch, ch, kernel_size=d_conv, groups=ch, padding=0, bias=bias)
        self.desired_hidden_dim = in_channels * (d_conv - 1) * num_ensemble
        self.desire_ndim = 4

    def forward(self, x, hidden=None, mask=None):
        E, D, K = self.num_ensemble, self.in_channels, self.d_conv
        assert x.dim() in (3, 4) and (x.dim() == 3 or x.shape[0] == E), f'econv1d-{E}: input {tuple(x.shape)} is neither [B, T, D] nor [{E}, B, T, D]'
        if x.shape[-2] == 1 and not torch.is_grad_enabled():
            raise NotImplementedError(f'econv1d-{E}: one-token rollout steps are not built - ensemble sequence layers live in critic stacks, '
                                      f'and critics are never stepped')
        Bsz, T = x.shape[-3], x.shape[-2]
        w = self.conv1d.weight.view(E, D, K)
        b = None if self.conv1d.bias is None else self.conv1d.bias.view(E, D)
        # the carried window is kept as it is (it holds masked inputs already): mask 1 over its K - 1 slots
        mrow = None
        if mask is not None:
            mrow = torch.cat((torch.ones(Bsz, K - 1, dtype=torch.float32, device=x.device), mask.reshape(Bsz, T).float()), dim=1)
        if x.dim() == 3 and hidden is None:
            rows = torch.cat((torch.zeros(Bsz, K - 1, D, dtype=x.dtype, device=x.device), x), dim=1)          # shared by the members
        else:
            if hidden is None:
                window = torch.zeros(E, Bsz, K - 1, D, dtype=x.dtype, device=x.device)
            else:
                window = hidden.reshape(Bsz, E, K - 1, D).transpose(0, 1)
            if x.dim() == 3:
                x = x.unsqueeze(0).expand(E, Bsz, T, D)
            rows = torch.cat((window, x), dim=2)                                                            # [E, B, K - 1 + T, D]
        if ops.member_seq_on():
            y = ops.member_conv1d(rows, w, b, mrow)
        else:
            y = torch.stack([ops.causal_conv1d_fn(rows if rows.dim() == 3 else rows[e], w[e], None if b is None else b[e], mrow, False)
                             for e in range(E)])
        y = y[:, :, K - 1:]
        tail = rows[..., rows.shape[-2] - (K - 1):, :]
        if mrow is not None:
            tail = tail * mrow[:, mrow.shape[1] - (K - 1):, None]
        if tail.dim() == 3:
            tail = tail.unsqueeze(0).expand(E, Bsz, K - 1, D)
        return y, tail.transpose(0, 1).reshape(Bsz, 1, -1)
