"""MultiEnsembleLinear: `multi_num` stacked EnsembleLinear layers, weight [c, E, in, out] and bias [c, E, 1, out] (reference
offpolicy_rnn/models/multi_ensemble_linear_model.py:8-65 - names and shapes kept).  The `elru-<E>` layer builds its input projection
(c = 3: Re / Im of the recurrence input, skip term) and its middle projection (c = 2: applied to Re h | Im h) from it.

No GEMM of its own: every contraction is one of the member products of ensemble_linear_model.py over contiguous weight slices.
  * shared input [B, T, in] (every member of every slice reads the same rows): ONE shared-input product with c * E members;
  * stacked input [c, E, B, T, in] (`middle_proj` on the (Re h | Im h) the scan writes): ONE batched product with c * E members;
  * member-major input [E, B, T, in] (each member's rows go through its c slices): c batched products of E members on the same
    operand, written into one [c, E, M, out] tensor; the input gradient accumulates over the slices in the GEMM epilogue."""
import torch
import torch.nn as nn

from ..hip import ops
from .ensemble_linear_model import _PerMember, _SharedInput, _member_wgrad, _unit


class _MultiMember(torch.autograd.Function):
    """y[i, e] = x3[e] W[i, e] + b[i, e] for x3 [E, M, in], W [c, E, in, out], b [c, E, 1, out] or None -> y [c, E, M, out]."""

    @staticmethod
    def forward(ctx, x3, weight, bias, ax=None):
        c, E, n_in, n_out = weight.shape
        M = x3.shape[1]
        x3 = _unit(x3)
        y = torch.empty(c, E, M, n_out, dtype=torch.float32, device=x3.device)
        for i in range(c):
            ops.gemm_f32(x3, weight[i], True, False, None if bias is None else bias[i], None, out=y[i], amax_a=ax)
        ax = ax if ax is not None else ops.amax_of(x3)
        ctx.save_for_backward(x3, weight)
        ctx.ax = ops.keep_handles(ax)[0]
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x3, weight = ctx.saved_tensors
        c, E, n_in, n_out = weight.shape
        M = x3.shape[1]
        g = g.float().contiguous()
        db = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            if n_out % 4 == 0:
                db = ops.bias_act_bwd(g.view(c * E * M, n_out), None, M, None, True)[1].view(c, E, 1, n_out)
            else:
                db = g.sum(dim=2, keepdim=True)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(E, M, n_in, dtype=torch.float32, device=g.device)
            for i in range(c):            # slice 0 writes, the others accumulate: a fixed order
                ops.gemm_f32(g[i], weight[i], True, True, None, None if i == 0 else ops.GEMM_ACCUMULATE, out=dx)
        dw = None
        if ctx.needs_input_grad[1]:
            ax = ops.handle_alive(ctx.ax)
            dw = torch.stack([_member_wgrad(x3, g[i], ax) for i in range(c)])
        return dx, dw, db, None


class MultiEnsembleLinear(nn.Module):
    def __init__(self, input_dim: int, output_dim: int, num_ensemble: int, multi_num: int, bias: bool = True, desire_ndim: int = None):
        super().__init__()
        self.use_bias = bias
        self.desire_ndim = desire_ndim
        self.num_ensemble = num_ensemble
        self.multi_num = multi_num
        self.weight = nn.Parameter(torch.zeros(multi_num, num_ensemble, input_dim, output_dim))
        if bias:
            self.bias = nn.Parameter(torch.zeros(multi_num, num_ensemble, 1, output_dim))
        nn.init.trunc_normal_(self.weight, std=1 / (2 * input_dim ** 0.5))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, T, in] (shared), [E, B, T, in] (member-major) or [c, E, B, T, in] (stacked) -> [c, E, B, T, out]."""
        assert self.desire_ndim == 4, 'the sequence layers call MultiEnsembleLinear on [.., B, T, C] activations (desire_ndim = 4)'
        c, E, n_in, n_out = self.weight.shape
        W, b = self.weight, self.bias if self.use_bias else None
        ax = ops.amax_of(x)
        nd = x.dim()
        if nd == 3:
            lead = tuple(x.shape[:-1])
            y = ops.apply_tagged(_SharedInput.apply, True, x.reshape(-1, n_in), W.view(c * E, n_in, n_out),
                                 None if b is None else b.view(c * E, 1, n_out), None, None, 0, ax)
        elif nd == 4:
            assert x.shape[0] == E, f'member-major input carries {x.shape[0]} members, the layer has {E}'
            lead = tuple(x.shape[1:-1])
            y = ops.apply_tagged(_MultiMember.apply, False, x.reshape(E, -1, n_in), W, b, ax)
        elif nd == 5:
            assert tuple(x.shape[:2]) == (c, E), (tuple(x.shape), tuple(W.shape))
            lead = tuple(x.shape[2:-1])
            y = ops.apply_tagged(_PerMember.apply, True, x.reshape(c * E, -1, n_in), W.view(c * E, n_in, n_out),
                                 None if b is None else b.view(c * E, 1, n_out), None, ax)
        else:
            raise NotImplementedError(f'MultiEnsembleLinear: input of {nd} dimensions')
        return y.reshape((c, E) + lead + (n_out,))
