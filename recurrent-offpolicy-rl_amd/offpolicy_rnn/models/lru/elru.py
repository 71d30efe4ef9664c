"""`elru-<E>` layer - E independent complex diagonal Linear Recurrent Units, one per member of an `efc-<E>` ensemble critic (reference
offpolicy_rnn/models/lru/elru.py:17-214).

Per member e:  h_t = lambda_e (1 - rnn_start_t) h_{t-1} + gamma_e (u0_t + i u1_t),  out = middle_proj(Re h | Im h)[0] - [1] + u2, then the
ensemble feed-forward block.  Input: member-major [E, B, T, C], or a shared [B, T, C] which every member reads; `rnn_start` is shared.
State [1, B, 2 E C]: 2 E chunks of width C, Re h of members 0 .. E-1 first, then Im h.
RESEL_MEMBER_SEQ (read per call) - 1: the recurrence of all members is ONE launch each way (`ops.complex_scan_ensemble`, rows
e B .. (e + 1) B - 1 take member e's lambda / gamma); 0: E launches of the single-member scan on each member's rows."""
import math

import torch
import torch.nn as nn

from ..gilr.gilr import EnsemblePositionWiseFeedForward
from ..multi_ensemble_linear_model import MultiEnsembleLinear
from ...hip import ops


class EnsembleLRULayer(nn.Module):
    def __init__(self, input_dim, output_dim, num_ensemble, dropout=0.0, batch_first=True, use_ff=True, squash_inproj=False):
        super().__init__()
        assert batch_first, 'LRU only support batch_first==True'
        # the reference builds middle_proj on the INPUT width (elru.py:34) and applies it to the d_model-wide state: only equal widths run
        assert input_dim == output_dim, f'elru requires input_dim == output_dim, while got {input_dim} and {output_dim}'
        self.d_model = output_dim
        self.num_ensemble = num_ensemble
        self.in_proj = MultiEnsembleLinear(input_dim, self.d_model, num_ensemble, 3, desire_ndim=4, bias=True)
        self.middle_proj = MultiEnsembleLinear(input_dim, self.d_model, num_ensemble, 2, desire_ndim=4, bias=True)
        self.dropout = nn.Dropout(dropout)
        self.params_log = nn.Parameter(self._init_params(num_ensemble, self.d_model))
        self.use_ff, self.squash_inproj = use_ff, squash_inproj
        if use_ff:
            self.ff = EnsemblePositionWiseFeedForward(self.d_model, num_ensemble, dropout, desire_ndim=4)

    @staticmethod
    def _init_params(E, c, r_min=0.9, r_max=0.999):
        """Ring initialisation per member (arXiv 2303.06349 sec. 3.2.2) -> [3, E, C] = (nu_log | theta_log | gamma_log)."""
        u1, u2 = torch.rand(E, c), torch.rand(E, c)
        nu_log = torch.log(-0.5 * torch.log(u1 * (r_max ** 2 - r_min ** 2) + r_min ** 2))
        theta_log = torch.log(u2 * math.pi * 2)
        gamma_log = torch.log(torch.sqrt(1 - torch.exp(-torch.exp(nu_log)) ** 2))
        return torch.stack((nu_log, theta_log, gamma_log))

    def rnn_parameters(self):
        return self.parameters(recurse=True)

    def forward(self, x, hidden=None, rnn_start=None, grad_detach=None):
        E, C = self.num_ensemble, self.d_model
        assert x.dim() in (3, 4) and (x.dim() == 3 or x.shape[0] == E), f'elru-{E}: input {tuple(x.shape)} is neither [B, T, C] nor [{E}, B, T, C]'
        if x.shape[-2] == 1 and not torch.is_grad_enabled():
            raise NotImplementedError(f'elru-{E}: one-token rollout steps are not built - ensemble sequence layers live in critic stacks, '
                                      f'and critics are never stepped')
        Bsz = x.shape[-3]
        u = self.in_proj(x)                                         # [3, E, B, T, C]
        if self.squash_inproj:
            u = torch.tanh(u)
        h0r = h0i = None
        if hidden is not None:
            h0 = hidden[0].reshape(Bsz, 2, E, C).permute(1, 2, 0, 3)           # [2, E, B, C]
            h0r, h0i = h0[0], h0[1]
        lam3 = ops.lru_params(self.params_log)                      # [3, E, C]: element-wise, one launch for all members
        if ops.member_seq_on():
            h2, u2 = ops.complex_scan_ensemble(u, lam3, rnn_start, h0r, h0i)   # h2 [2, E, B, T, C]
        else:
            parts = [ops.complex_scan_members(u[:, e], lam3[:, e], rnn_start, None if h0r is None else h0r[e], None if h0i is None else h0i[e])
                     for e in range(E)]
            h2 = torch.stack([p[0] for p in parts], dim=1)
            u2 = torch.stack([p[1] for p in parts], dim=0)
        out = ops.SubAddMembers.apply(self.middle_proj(h2), u2)     # [E, B, T, C]
        if self.use_ff:
            out = self.ff(out)
        hidden = h2[:, :, :, -1, :].permute(2, 0, 1, 3).reshape(1, Bsz, 2 * E * C)
        return out, hidden
