"""torch.autograd wrappers over the C-ABI kernels (include/resel_hip.h).

Every function here requires CUDA (ROCm) tensors and the in-tree `libresel_hip.so`; there is deliberately NO
CPU / eager fallback - a missing library or a CPU tensor raises.  PyTorch only provides device memory, the
current stream and autograd bookkeeping.

Layout: activations are token-major `[B, L, C]` (channel stride 1).  Column slices of a wider row-major
tensor (e.g. the `x` / `z` halves of `in_proj`'s output) are passed by stride, never copied.
"""
import collections
import ctypes
import os
from typing import Optional

import torch

from ._lib import check, lib


def _need_cuda(name, *ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f'RESeL-HIP: {name} needs CUDA tensors (got a {t.device} tensor); the HIP kernels are the '
                               f'only implementation of this op - there is no CPU fallback.')


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


if hasattr(torch._C, '_cuda_getCurrentRawStream') and hasattr(torch._C, '_cuda_getDevice'):
    def _stream():
        """Raw handle of the current HIP stream of the current device (the two C calls are what
        `torch.cuda.current_stream().cuda_stream` wraps in a Stream object: 11 us per call there, ~1700 calls per update)."""
        return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
else:                                                   # another torch build: the public (slower) spelling
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tok_major(t: torch.Tensor) -> torch.Tensor:
    """Return a [B, L, C] view/copy with channel stride 1, batch stride L*ld, ld % 4 == 0 and a 16-byte aligned base."""
    if t.dtype != torch.float32:
        t = t.float()
    B, L, C = t.shape
    ok = (C == 1 or t.stride(2) == 1) and t.stride(1) % 4 == 0 and (B == 1 or t.stride(0) == L * t.stride(1)) \
        and t.data_ptr() % 16 == 0 and t.stride(1) >= C
    return t if ok else t.contiguous()


def _flags(t: Optional[torch.Tensor], B: int, L: int) -> Optional[torch.Tensor]:
    """[B, L] / [B, L, 1] float flags -> dense fp32 [B*L]."""
    if t is None:
        return None
    return t.reshape(B, L).to(torch.float32).contiguous()


def _h0(h0: Optional[torch.Tensor], B: int, C: int) -> Optional[torch.Tensor]:
    """Initial state of a recurrence -> dense fp32 [B, C]."""
    return None if h0 is None else h0.float().reshape(B, C).contiguous()


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


PROF_SLOTS = ('sscan_fwd_kernel', 'sscan_bwd_kernel', 'attn_fwd_kernel', 'attn_dq_kernel', 'attn_dkv_kernel', 'linrec_real_fwd_kernel',
              'linrec_real_bwd_kernel', 'linrec_complex_fwd_kernel', 'linrec_complex_bwd_kernel', 'gru_fwd_kernel', 'gru_bwd_kernel',
              'conv_fwd_kernel', 'conv_bwd_kernel', 'gemm_f32_kernel', 'sscan_fwd_local_kernel',
              'sscan_bwd_local_kernel', 'sscan_gate_fwd_kernel', 'sscan_gate_bwd_kernel',
              'sscan_group_reduce_kernel')                                      # RESEL_PROF_* of include/resel_hip.h, in id order
GEMM_FLOPS = [0.0]            # 2 M N K of every resel_gemm_f32 call since the caller last reset it (bench.py's GEMM line)


def profile_enable(on: bool):
    """Bind a (start, stop) HIP event pair to every sequence-layer kernel dispatch (bench.py's roofline measurement)."""
    check(lib().resel_profile_enable(int(bool(on))), 'profile_enable')


def profile_collect():
    """-> {kernel: (launches, avg_us)} for the dispatches recorded since the last call."""
    out = {}
    for kid, name in enumerate(PROF_SLOTS):
        tot, n = ctypes.c_double(0.0), ctypes.c_int(0)
        check(lib().resel_profile_collect(kid, ctypes.byref(tot), ctypes.byref(n)), 'profile_collect')
        if n.value:
            out[name] = (n.value, tot.value / n.value)
    return out


# ---------------------------------------------------------------------------------------------- selective scan
# 0: the library cuts small batches into time segments scanned in parallel (resel_hip.h); 1: never; k > 1: k segments (tests)
SSCAN_TIME_SEGMENTS = int(os.environ.get('RESEL_SSCAN_TIME_SEGMENTS', '0'))


# The marshalling sites of the scan and conv entries (one per entry; `SelectiveScanFn`, `CausalConv1dFn` and `MambaInnerFn` call them).  A
# token-major operand is a [B, L, C] tensor or an [M = B L, C] column block of a wider matrix, unit stride on its last axis: the kernel
# gets its `data_ptr()` and, as token stride, its `stride(-2)`.  The caller allocates every output; the workspace belongs to the helper.
def _sscan_fwd(Bsz, L, u, delta, z, A, Bm, Cm, D, delta_bias, start, out, ck, last, softplus, amax_out=None, epoch=0):
    """softplus: the entry's `delta_softplus` code (0 / 1, or the mixer's 6); amax_out, epoch: magnitude slot of `out` (pointer) or None."""
    Di, N = A.shape
    nb = lib().resel_selective_scan_fwd_workspace_bytes(Bsz, L, Di, N, SSCAN_TIME_SEGMENTS)
    check(lib().resel_selective_scan_fwd(
        _p(u), u.stride(-2), _p(delta), delta.stride(-2), _p(z), 0 if z is None else z.stride(-2), _p(A),
        _p(Bm), Bm.stride(-2), _p(Cm), Cm.stride(-2), _p(D), _p(delta_bias), _p(start),
        _p(out), out.stride(-2), _p(ck), _p(last), _p(_ws(nb, u.device) if nb else None), Bsz, L, Di, N, softplus,
        SSCAN_TIME_SEGMENTS, amax_out, epoch, _stream()), 'selective_scan_fwd')


def _sscan_bwd(Bsz, L, u, delta, z, A, Bm, Cm, D, delta_bias, start, dout, ck, du, ddelta, dz, dB, dC, dA, dD, dbias, softplus,
               amax_dz=None, amax_ddelta=None, epoch=0):
    Di, N = A.shape
    ws = _ws(lib().resel_selective_scan_bwd_workspace_bytes(Bsz, L, Di, N, SSCAN_TIME_SEGMENTS), u.device)
    check(lib().resel_selective_scan_bwd(
        _p(u), u.stride(-2), _p(delta), delta.stride(-2), _p(z), 0 if z is None else z.stride(-2), _p(A),
        _p(Bm), Bm.stride(-2), _p(Cm), Cm.stride(-2), _p(D), _p(delta_bias), _p(start),
        _p(dout), dout.stride(-2), _p(ck),
        _p(du), du.stride(-2), _p(ddelta), ddelta.stride(-2), _p(dz), 0 if dz is None else dz.stride(-2),
        _p(dB), dB.stride(-2), _p(dC), dC.stride(-2), _p(dA), _p(dD), _p(dbias), _p(ws),
        Bsz, L, Di, N, softplus, SSCAN_TIME_SEGMENTS, amax_dz, amax_ddelta, epoch, _stream()), 'selective_scan_bwd')


# ---- every d_state from 1 to 256 on the five native kernels (include/resel_hip.h "state groups") --------------------------------------
SSCAN_NATIVE_STATES = (4, 8, 16, 32, 64)     # the sizes resel_selective_scan_fwd / _bwd are built for
SSCAN_MAX_GROUPS = 4                         # RESEL_SSCAN_MAX_GROUPS
SSCAN_MAX_STATES = SSCAN_NATIVE_STATES[-1] * SSCAN_MAX_GROUPS


def sscan_state_plan(N: int):
    """How a scan over N states runs: [(first_state, states, kernel_N), ...], one native scan per entry.  A native N is itself; any other
    N <= 64 is one group on the next native size (zero B / C columns: a padded state stays exactly 0 and adds exactly 0); 64 < N <= 256 is
    N // 64 groups of 64 and the remainder on the smallest native size that holds it.  Only the last group is ever padded, so the padded
    operands are the real columns followed by zeros.  Host-only; both training nodes consult this and nothing else."""
    N = int(N)
    if N < 1 or N > SSCAN_MAX_STATES:
        raise ValueError(f'selective scan: d_state {N} is not supported: accepted are 1 to {SSCAN_MAX_STATES} ({", ".join(map(str, SSCAN_NATIVE_STATES))} '
                         f'native, other sizes up to 64 zero-padded to the next of these, larger ones as groups of 64 plus a remainder); '
                         f'{SSCAN_MAX_STATES} is this build\'s bound: {SSCAN_MAX_GROUPS} groups')
    if N in SSCAN_NATIVE_STATES:
        return [(0, N, N)]
    top = SSCAN_NATIVE_STATES[-1]
    plan = [(top * g, top, top) for g in range(N // top)] if N > top else []
    rest = N - top * len(plan)
    if rest:
        plan.append((top * len(plan), rest, next(w for w in SSCAN_NATIVE_STATES if w >= rest)))
    return plan


def sscan_padded_states(plan) -> int:
    """Columns of the B / C / A operands a plan's kernels read: the real states and the zero tail of the last group."""
    return plan[-1][0] + plan[-1][2]


def _group_A(A, plan):
    """The dense [Di, kernel_N] `A` (or A_log) of every group: a native N takes the tensor itself, any other plan one `place_blocks` launch per
    group, which copies the group's columns and zero-fills a padded tail (A_log = 0 there; any finite value would do)."""
    Di, N = A.shape
    if len(plan) == 1 and plan[0][2] == N:
        return [A.float().contiguous()]
    A = A.detach()
    return [place_blocks(Di, k, [(0, 0)], A[:, f:f + s]) for f, s, k in plan]


def _join_states(pieces, plan, N):
    """Per-group [rows, kernel_N] results (dA, last state) -> [rows, N]: the real columns of every group, one launch."""
    if len(plan) == 1 and plan[0][2] == N:
        return pieces[0]
    return place_blocks(pieces[0].shape[0], N, [(0, f) for f, _, _ in plan], *[t[:, :s] for t, (_, s, _) in zip(pieces, plan)])


def _sscan_gate_fwd(parts, u, D, z, out, amax_out=None, epoch=0):
    """parts [G, M, Di] dense; u, z, out token-major [M, Di] blocks (or [B, L, Di])."""
    G, M, Di = parts.shape
    check(lib().resel_sscan_gate_fwd(_p(parts), parts.stride(0), G, _p(u), u.stride(-2), _p(D), _p(z), 0 if z is None else z.stride(-2),
                                     _p(out), out.stride(-2), M, Di, amax_out, epoch, _stream()), 'sscan_gate_fwd')


def _sscan_gate_bwd(dout, parts, G, M, Di, u, D, z, g, dz, dD, amax_dz=None, epoch=0):
    """parts: the forward's [G, M, Di] (None without z); g, dz: None iff z is None; dD: None iff D is None."""
    ws = _ws(lib().resel_sscan_gate_bwd_workspace_bytes(M, Di), dout.device) if D is not None else None
    check(lib().resel_sscan_gate_bwd(_p(dout), dout.stride(-2), _p(parts), 0 if parts is None else parts.stride(0), G, _p(u), u.stride(-2), _p(D),
                                     _p(z), 0 if z is None else z.stride(-2), _p(g), 0 if g is None else g.stride(-2),
                                     _p(dz), 0 if dz is None else dz.stride(-2), _p(dD), _p(ws), M, Di, amax_dz, epoch, _stream()), 'sscan_gate_bwd')


def _sscan_group_reduce(du_parts, dd_parts, db_parts, g, D, du, ddelta, dbias, amax_ddelta=None, epoch=0):
    G, M, Di = du_parts.shape
    check(lib().resel_sscan_group_reduce(_p(du_parts), _p(dd_parts), du_parts.stride(0), _p(db_parts), G, _p(g), g.stride(-2), _p(D),
                                         _p(du), du.stride(-2), _p(ddelta), ddelta.stride(-2), _p(dbias), M, Di, amax_ddelta, epoch, _stream()),
          'sscan_group_reduce')


def _plan_fwd(plan, A_g, Bsz, L, u, delta, z, Bm, Cm, D, delta_bias, start, out, need_grad, want_last, softplus, amax_out=None, epoch=0):
    """The scan forward of a plan.  A_g: `_group_A`; Bm, Cm: `sscan_padded_states` columns wide.  One group: the scan itself, gate and skip
    included.  More: every group scans its own columns in place with z = D = None into its slab of `parts`, then ONE gate pass.
    -> (checkpoints per group, parts or None, last states per group or None)."""
    dev, Di = u.device, A_g[0].shape[0]
    cks = [_ws(lib().resel_selective_scan_ckpt_bytes(Bsz, L, Di, k), dev) if need_grad else None for _, _, k in plan]
    lasts = [torch.empty(Bsz, Di, k, dtype=torch.float32, device=dev) for _, _, k in plan] if want_last else None
    if len(plan) == 1:
        _sscan_fwd(Bsz, L, u, delta, z, A_g[0], Bm, Cm, D, delta_bias, start, out, cks[0], lasts[0] if want_last else None, softplus, amax_out, epoch)
        return cks, None, lasts
    parts = torch.empty(len(plan), Bsz * L, Di, dtype=torch.float32, device=dev)
    for i, (f, _, k) in enumerate(plan):
        _sscan_fwd(Bsz, L, u, delta, None, A_g[i], Bm[..., f:f + k], Cm[..., f:f + k], None, delta_bias, start, parts[i], cks[i],
                   lasts[i] if want_last else None, softplus)
    _sscan_gate_fwd(parts, u, D, z, out, amax_out, epoch)
    return cks, (parts if z is not None else None), lasts                  # the backward needs the pre-gate sum for dz only


def _plan_bwd(plan, A_g, Bsz, L, u, delta, z, Bm, Cm, D, delta_bias, start, dout, cks, parts, du, ddelta, dz, dB, dC, dD, dbias, softplus,
              amax_dz=None, amax_ddelta=None, epoch=0):
    """The scan backward of a plan: dB, dC as wide as Bm, Cm; -> dA per group.  More than one group: ONE gate pass forms the pre-gate gradient
    every group takes as its dout (with dz and dD), the groups write their column blocks of dB / dC and their own du / ddelta, ONE pass sums
    those (with the skip term's share of du and ddelta_bias)."""
    dev, Di = u.device, A_g[0].shape[0]
    dA_g = [torch.empty(Di, k, dtype=torch.float32, device=dev) for _, _, k in plan]
    if len(plan) == 1:
        _sscan_bwd(Bsz, L, u, delta, z, A_g[0], Bm, Cm, D, delta_bias, start, dout, cks[0], du, ddelta, dz, dB, dC, dA_g[0], dD, dbias, softplus,
                   amax_dz, amax_ddelta, epoch)
        return dA_g
    G, M = len(plan), Bsz * L
    g = torch.empty(M, Di, dtype=torch.float32, device=dev) if z is not None else None
    if z is not None or D is not None:
        _sscan_gate_bwd(dout, parts, G, M, Di, u, D, z, g, dz, dD, amax_dz, epoch)
    gin = dout if g is None else g
    du_p = torch.empty(G, M, Di, dtype=torch.float32, device=dev)
    dd_p = torch.empty_like(du_p)
    db_p = torch.empty(G, Di, dtype=torch.float32, device=dev) if dbias is not None else None
    for i, (f, _, k) in enumerate(plan):
        _sscan_bwd(Bsz, L, u, delta, None, A_g[i], Bm[..., f:f + k], Cm[..., f:f + k], None, delta_bias, start, gin, cks[i], du_p[i], dd_p[i], None,
                   dB[..., f:f + k], dC[..., f:f + k], dA_g[i], None, None if db_p is None else db_p[i], softplus)
    _sscan_group_reduce(du_p, dd_p, db_p, gin, D, du, ddelta, dbias, amax_ddelta, epoch)
    return dA_g


def _conv_fwd(Bsz, L, x, w, bias, mask, y, act, amax_y=None, epoch=0):
    Di, K = w.shape
    check(lib().resel_causal_conv1d_fwd(_p(x), x.stride(-2), _p(w), _p(bias), _p(mask), _p(y), y.stride(-2), Bsz, L, Di, K, act,
                                        amax_y, epoch, _stream()), 'causal_conv1d_fwd')


def _conv_bwd(Bsz, L, x, w, bias, mask, dy, dy2, dx, dw, db, act, amax_dx=None, epoch=0):
    """dy2: second part of the output gradient, summed with dy on load, or None (then this is the library's `resel_causal_conv1d_bwd`)."""
    Di, K = w.shape
    ws = _ws(lib().resel_causal_conv1d_bwd_workspace_bytes(Bsz, L, Di, K), x.device)
    check(lib().resel_causal_conv1d_bwd2(_p(x), x.stride(-2), _p(w), _p(bias), _p(mask), _p(dy), dy.stride(-2),
                                         _p(dy2), 0 if dy2 is None else dy2.stride(-2), _p(dx), dx.stride(-2), _p(dw), _p(db), _p(ws),
                                         Bsz, L, Di, K, act, amax_dx, epoch, _stream()), 'causal_conv1d_bwd')


class SelectiveScanFn(torch.autograd.Function):
    """Token-major selective scan with start resets.  Interface counterpart of the reference's
    `SelectiveScanFn` (mamba_ssm/ops/selective_scan_interface_new.py:19-84)."""

    @staticmethod
    def forward(ctx, u, delta, A, Bm, Cm, D, z, delta_bias, start, delta_softplus, return_last_state, grad_mode=True):
        """grad_mode: torch.is_grad_enabled() of the CALLER (inside forward it is always off, and `needs_input_grad` still names every
        parameter that requires grad under no_grad): without it no checkpoints are written."""
        _need_cuda('selective_scan', u, delta, A, Bm, Cm)
        u, delta, Bm, Cm = _tok_major(u), _tok_major(delta), _tok_major(Bm), _tok_major(Cm)
        z = None if z is None else _tok_major(z)
        A = A.float().contiguous()
        D = None if D is None else D.float().contiguous()
        delta_bias = None if delta_bias is None else delta_bias.float().contiguous()
        Bsz, L, Di = u.shape
        N = A.shape[1]
        plan = sscan_state_plan(N)                                         # raises for a d_state outside 1 .. 256
        Np = sscan_padded_states(plan)
        A_g = _group_A(A, plan)
        if Np != N:                                                        # [M, N] beside [M, Di] activations: padded copies, zero tail
            Bm = place_blocks(Bsz * L, Np, [(0, 0)], Bm).view(Bsz, L, Np)
            Cm = place_blocks(Bsz * L, Np, [(0, 0)], Cm).view(Bsz, L, Np)
        start = _flags(start, Bsz, L)
        out = torch.empty(Bsz, L, Di, dtype=torch.float32, device=u.device)
        need_grad = bool(grad_mode) and any(ctx.needs_input_grad)
        cks, parts, lasts = _plan_fwd(plan, A_g, Bsz, L, u, delta, z, Bm, Cm, D, delta_bias, start, out, need_grad, return_last_state,
                                      int(bool(delta_softplus)))
        ctx.save_for_backward(u, delta, Bm, Cm, D, z, delta_bias, start, parts, *A_g, *cks)
        ctx.softplus = bool(delta_softplus)
        ctx.plan, ctx.N = plan, N
        if return_last_state:
            last = _join_states([t.view(Bsz * Di, -1) for t in lasts], plan, N).view(Bsz, Di, N)
            ctx.mark_non_differentiable(last)
            return out, last
        return out

    @staticmethod
    def backward(ctx, dout, *_):
        plan, N = ctx.plan, ctx.N
        u, delta, Bm, Cm, D, z, delta_bias, start, parts = ctx.saved_tensors[:9]
        A_g, cks = ctx.saved_tensors[9:9 + len(plan)], ctx.saved_tensors[9 + len(plan):]
        Bsz, L, Di = u.shape
        Np = Bm.shape[-1]
        dout = _tok_major(dout)
        dev = u.device
        du = torch.empty(Bsz, L, Di, dtype=torch.float32, device=dev)
        ddelta = torch.empty_like(du)
        dz = torch.empty_like(du) if z is not None else None
        dB = torch.empty(Bsz, L, Np, dtype=torch.float32, device=dev)
        dC = torch.empty_like(dB)
        dD = torch.empty(Di, dtype=torch.float32, device=dev) if D is not None else None
        dbias = torch.empty(Di, dtype=torch.float32, device=dev) if delta_bias is not None else None
        dA_g = _plan_bwd(plan, A_g, Bsz, L, u, delta, z, Bm, Cm, D, delta_bias, start, dout, cks, parts, du, ddelta, dz, dB, dC, dD, dbias,
                         int(ctx.softplus))
        if Np != N:                                                        # whatever the backward computed for padded states is dropped
            dB, dC = dB[..., :N], dC[..., :N]
        return du, ddelta, _join_states(dA_g, plan, N), dB, dC, dD, dz, dbias, None, None, None, None


def selective_scan_tm(u, delta, A, Bm, Cm, D=None, z=None, delta_bias=None, start=None, delta_softplus=True,
                      return_last_state=False):
    """Token-major entry: u, delta, z [B, L, Di]; Bm, Cm [B, L, N]; start [B, L] or [B, L, 1]."""
    return SelectiveScanFn.apply(u, delta, A, Bm, Cm, D, z, delta_bias, start, delta_softplus, return_last_state, torch.is_grad_enabled())


def selective_scan_fn(u, delta, A, B, C, start, D=None, z=None, delta_bias=None, delta_softplus=False,
                      return_last_state=False):
    """Reference signature (selective_scan_interface_new.py:87-93): u, delta, z, start (B, D, L); B, C (B, N, L).
    Channel-major VIEWS of token-major storage are accepted without copies; anything else is re-laid-out."""
    tm = lambda t: None if t is None else t.transpose(1, 2)
    st = None if start is None else start[:, 0, :]
    res = selective_scan_tm(tm(u), tm(delta), A, tm(B), tm(C), D, tm(z), delta_bias, st, delta_softplus, return_last_state)
    if return_last_state:
        return res[0].transpose(1, 2), res[1]
    return res.transpose(1, 2)


# ---------------------------------------------------------------------------------------------- fused Mamba mixer


class MambaInnerFn(torch.autograd.Function):
    """in_proj -> masked causal conv + SiLU -> x_proj -> dt_proj -> selective scan (gate, skip, resets) -> out_proj as ONE
    autograd node (interface counterpart of the reference's `MambaInnerFn`, selective_scan_interface_new.py:169-335, which
    only exists for d_conv <= 4).  Everything is token-major; the backward writes every gradient straight into its slot of
    two buffers - dxz [M, 2Di] (conv backward fills the x half, scan backward the z half) and dx_dbl [M, R+2N] (scan
    backward fills the B / C columns) - through the kernels' token strides, so autograd's slice-backward zero-fill + copy +
    add passes (8 x 273 MB per update at config 2) disappear.  GEMMs: `mm_nt` / `mm_nn` / `wgrad` (hand-written, every pass)."""

    @staticmethod
    def forward(ctx, x, in_w, conv_w, conv_b, xproj_w, dt_w, dt_b, A_log, D, out_w, mask, start, grad_mode=True):
        """grad_mode: the caller's torch.is_grad_enabled() (see `SelectiveScanFn.forward`): a no_grad pass writes no scan checkpoints."""
        _need_cuda('mamba_inner', x, in_w, conv_w, xproj_w, dt_w, A_log, out_w)
        Bsz, L, Dm = x.shape
        Di, N = A_log.shape
        R = dt_w.shape[1]
        K = conv_w.shape[-1]
        M = Bsz * L
        plan = sscan_state_plan(N)                                         # raises for a d_state outside 1 .. 256
        Np = sscan_padded_states(plan)
        x2 = x.reshape(M, Dm)
        maskf, startf = _flags(mask, Bsz, L), _flags(start, Bsz, L)
        xz = mm_nt(x2, in_w)                                               # [M, 2Di] = (x | z)
        ctx.ax = amax_of(x2)                                               # magnitude handle of the block input (for d in_proj.weight)
        cw = conv_w.reshape(Di, K).contiguous()
        xc = torch.empty(M, Di, dtype=torch.float32, device=x.device)
        track = amax_tracking() and M * Di >= (1 << 20)                    # publish the magnitudes of the tensors the projections read
        h_xc, p_xc, e_xc = _slot_args(track, x.device)
        _conv_fwd(Bsz, L, xz, cw, conv_b, maskf, xc, 1, p_xc, e_xc)          # reads the x half: the first Di columns of xz's rows
        tag_amax(xc, h_xc)
        # a padded d_state: x_proj's weight gets zero rows behind its B rows and behind its C rows (one launch, as w32 below), so x_dbl and
        # dx_dbl simply are Np states wide and no [M, .] activation is ever re-laid-out
        xw = xproj_w if Np == N else place_blocks(R + 2 * Np, Di, [(0, 0), (R + Np, 0)], xproj_w.detach()[:R + N], xproj_w.detach()[R + N:])
        x_dbl = mm_nt(xc, xw)                                              # [M, R + 2Np] = (delta_r | B | C)
        # delta = softplus(dt_proj(.) + bias) leaves the GEMM epilogue: the scan kernels spend no vector issue on it
        if narrow_on() and narrow_k_ok(x_dbl[:, :R], dt_w):
            # K = dt_rank = 16 against 137 MB of output: the streaming kernel with the weight resident in registers (no padded weight, no
            # operand magnitudes; nothing multiplies delta again, so none is published for it either)
            dt = narrow_k(x_dbl[:, :R], dt_w.detach(), dt_b, GEMM_SOFTPLUS)
        elif R < 32 <= R + 2 * N and os.environ.get('RESEL_DT_PAD', '1') != '0' and gemm_split() == 2:
            # dt_proj has K = dt_rank = 16: one PARTIAL K step, which only the fp32-MFMA first edition takes (58 us for a product whose floor
            # is its 137 MB of output: 28 us).  Read 32 columns of x_dbl instead - the 16 behind delta_r are B's, finite - against the weight
            # padded with 16 zero columns (one launch): a whole K step, so the producer / consumer edition with its full-line stores runs it.
            w32 = place_blocks(Di, 32, [(0, 0)], dt_w.detach())
            dt = gemm_f32(x_dbl[:, :32], w32, True, True, dt_b, GEMM_SOFTPLUS, amax_a=amax_of(x_dbl), amax_b=weight_amax(dt_w))
        else:
            dt = gemm_f32(x_dbl[:, :R], dt_w, True, True, dt_b, GEMM_SOFTPLUS)
        # delta_softplus code 6 = 4 (the kernels form A = -exp(A_log) themselves) + 2 (delta arrives finished: no delta_bias)
        A_g = _group_A(A_log, plan)
        need_grad = bool(grad_mode) and any(ctx.needs_input_grad)
        y = torch.empty(M, Di, dtype=torch.float32, device=x.device)
        h_y, p_y, e_y = _slot_args(track, x.device)
        cks, parts, _ = _plan_fwd(plan, A_g, Bsz, L, xc, dt, xz[:, Di:], x_dbl[:, R:R + Np], x_dbl[:, R + Np:], D, None, startf, y, need_grad, False,
                                  6, p_y, e_y)
        tag_amax(y, h_y)
        out = mm_nt(y, out_w)
        ctx.handles = keep_handles(ctx.ax, h_xc, h_y)                      # saved tensors come back untagged
        ctx.save_for_backward(x2, in_w, cw, conv_b, xw, dt_w, dt_b, D, out_w, maskf, startf, xz, xc, x_dbl, dt, y, parts, *A_g, *cks)
        ctx.dims = (Bsz, L, Dm, Di, N, R, K, conv_w.shape)
        ctx.plan = plan
        return out.view(Bsz, L, -1)

    @staticmethod
    def backward(ctx, dout):
        plan = ctx.plan
        (x2, in_w, cw, conv_b, xw, dt_w, dt_b, D, out_w, maskf, startf, xz, xc, x_dbl, dt, y, parts) = ctx.saved_tensors[:17]
        A_g, cks = ctx.saved_tensors[17:17 + len(plan)], ctx.saved_tensors[17 + len(plan):]
        Bsz, L, Dm, Di, N, R, K, cw_shape = ctx.dims
        Np = sscan_padded_states(plan)
        M = Bsz * L
        dev = x2.device
        do2 = dout.reshape(M, -1)
        if not do2.is_contiguous():
            do2 = do2.contiguous()
        ax, h_xc, h_y = live_handles(ctx.handles)
        d_out_w = wgrad(do2, y, amax_x=h_y)
        dy = mm_nn(do2, out_w)                                             # [M, Di]
        dxz = torch.empty(M, 2 * Di, dtype=torch.float32, device=dev)      # fully written: conv bwd -> [:, :Di], scan bwd -> [:, Di:]
        dx_dbl = torch.empty(M, R + 2 * Np, dtype=torch.float32, device=dev)
        dxc = torch.empty(M, Di, dtype=torch.float32, device=dev)
        ddt = torch.empty(M, Di, dtype=torch.float32, device=dev)
        dD = torch.empty(Di, dtype=torch.float32, device=dev)
        ddt_b = torch.empty(Di, dtype=torch.float32, device=dev)
        track = amax_tracking() and M * Di >= (1 << 20)
        h_dxz, p_dxz, e_b = _slot_args(track, dev)                         # ONE handle for dxz: the scan fills its z half, the conv its x half
        h_ddt, p_ddt, _ = _slot_args(track, dev)                           # (published under the same epoch e_b)
        dA_g = _plan_bwd(plan, A_g, Bsz, L, xc, dt, xz[:, Di:], x_dbl[:, R:R + Np], x_dbl[:, R + Np:], D, None, startf, dy, cks, parts,
                         dxc, ddt, dxz[:, Di:], dx_dbl[:, R:R + Np], dx_dbl[:, R + Np:], dD, ddt_b, 6, p_dxz, p_ddt, e_b)
        dA = _join_states(dA_g, plan, N)                                   # the real columns (a padded state's are dropped)
        tag_amax(ddt, h_ddt)
        # [Di, R] with a 66 752-long reduction: hand-written MFMA kernel (the library reaches 7 TFLOP/s on this shape)
        if narrow_on() and narrow_n_pair_ok(ddt, dt_w, x_dbl[:, :R]):
            # ONE pass over ddt (137 MB) for both products it feeds; dx_dbl[:, :R] is written in place
            _, d_dt_w = narrow_n_pair(ddt, dt_w, x_dbl[:, :R], dx_out=dx_dbl[:, :R])
        else:
            d_dt_w = atb(ddt, x_dbl[:, :R]) if R <= 32 and Di % 4 == 0 and ddt.stride(1) == 1 and ddt.stride(0) % 4 == 0 \
                else gemm_f32(ddt, x_dbl[:, :R], False, False)
            mm_nn(ddt, dt_w, out=dx_dbl[:, :R])                              # straight into its column block of dx_dbl
        d_xproj_w = wgrad(dx_dbl, xc, amax_x=h_xc)
        if Np != N:                                                        # the real rows; a padded state's dB / dC columns are exactly 0 (its C is)
            d_xproj_w = place_blocks(R + 2 * N, Di, [(0, 0), (R + N, 0)], d_xproj_w[:R + N], d_xproj_w[R + Np:R + Np + N])
        # the conv output's gradient = the scan's du (in dxc) + the x_proj input gradient: handed to the conv backward as TWO tensors
        # (summed on load) - the accumulating GEMM epilogue cost 150-214 us per call against 67 for the plain product
        gx = mm_nn(dx_dbl, xw)
        dcw = torch.empty(Di, K, dtype=torch.float32, device=dev)
        dcb = torch.empty(Di, dtype=torch.float32, device=dev) if conv_b is not None else None
        _conv_bwd(Bsz, L, xz, cw, conv_b, maskf, dxc, gx, dxz, dcw, dcb, 1, p_dxz, e_b)       # x halves of xz and dxz: their rows' first Di columns
        tag_amax(dxz, h_dxz)
        d_in_w = wgrad(dxz, x2, amax_x=ax)
        dx = mm_nn(dxz, in_w).view(Bsz, L, Dm) if ctx.needs_input_grad[0] else None
        return (dx, d_in_w, dcw.reshape(cw_shape), dcb, d_xproj_w, d_dt_w, ddt_b, dA, dD, d_out_w, None, None, None)      # dA: already dL/dA_log


def mamba_inner_fn(x, in_w, conv_w, conv_b, xproj_w, dt_w, dt_b, A_log, D, out_w, mask=None, start=None):
    """x [B, L, D] -> [B, L, D]: the whole Mamba mixer of the training path (no biases on in/out projections)."""
    return MambaInnerFn.apply(x.float().contiguous(), in_w, conv_w, conv_b, xproj_w, dt_w, dt_b, A_log, D, out_w, mask, start,
                              torch.is_grad_enabled())


# ---------------------------------------------------------------------------------------------- causal conv1d
class CausalConv1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mask, activation):
        _need_cuda('causal_conv1d', x, weight)
        x = _tok_major(x)
        Bsz, L, Di = x.shape
        w = weight.float().reshape(Di, -1).contiguous()
        bias = None if bias is None else bias.float().contiguous()
        mask = _flags(mask, Bsz, L)
        y = torch.empty(Bsz, L, Di, dtype=torch.float32, device=x.device)
        _conv_fwd(Bsz, L, x, w, bias, mask, y, int(bool(activation)))
        ctx.save_for_backward(x, w, bias, mask)
        ctx.act = bool(activation)
        ctx.wshape = weight.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, bias, mask = ctx.saved_tensors
        Bsz, L, Di = x.shape
        K = w.shape[1]
        dy = _tok_major(dy)
        dx = torch.empty(Bsz, L, Di, dtype=torch.float32, device=x.device)
        dw = torch.empty(Di, K, dtype=torch.float32, device=x.device)
        db = torch.empty(Di, dtype=torch.float32, device=x.device) if bias is not None else None
        _conv_bwd(Bsz, L, x, w, bias, mask, dy, None, dx, dw, db, int(ctx.act))
        return dx, dw.reshape(ctx.wshape), db, None, None


def causal_conv1d_fn(x, weight, bias=None, mask=None, activation=True):
    """x [B, L, Di] token-major; weight [Di, K] or Conv1d's [Di, 1, K]; mask [B, L(,1)]: y = silu(conv(mask * x) + b)."""
    return CausalConv1dFn.apply(x, weight, bias, mask, activation)


# ---------------------------------------------------------------------------------------------- ensemble sequence layers: the switch
MEMBER_SEQ_DEFAULT = '1'        # what an unset RESEL_MEMBER_SEQ means (README; measured in profiles/r35_ensemble_encoders.md)


def member_seq_on() -> bool:
    """RESEL_MEMBER_SEQ, read per call.  1: the `elru-<E>` / `econv1d[_<K>]-<E>` layers run the member editions of the scan, the causal
    convolution and the add + LayerNorm (one launch over all members); 0: E launches of the single-member entries on each member's rows
    plus the separate add.  Anything else is an error."""
    v = os.environ.get('RESEL_MEMBER_SEQ', MEMBER_SEQ_DEFAULT)
    if v not in ('0', '1'):
        raise ValueError(f'RESEL_MEMBER_SEQ={v!r}: expected 0 or 1')
    return v == '1'


class MemberConv1dFn(torch.autograd.Function):
    """Depthwise causal convolution of E members in one launch each way (include/resel_hip.h `resel_member_conv1d_*`): x [E, B, L, D]
    member-major, or [B, L, D] read by every member (its gradient is then the sum over the members, formed in a fixed order); weight
    [E, D, K], bias [E, D] or None, mask [B, L(, 1)] shared -> y [E, B, L, D].  No activation."""

    @staticmethod
    def forward(ctx, x, weight, bias, mask):
        _need_cuda('member_conv1d', x, weight)
        E, D, K = weight.shape
        shared = x.dim() == 3
        assert x.shape[-1] == D and (shared or (x.dim() == 4 and x.shape[0] == E)), (tuple(x.shape), tuple(weight.shape))
        Bsz, L = x.shape[-3], x.shape[-2]
        x3 = _tok_major(x if shared else x.reshape(E * Bsz, L, D))
        w = weight.float().contiguous()
        bias = None if bias is None else _aligned_param(bias)
        mask = _flags(mask, Bsz, L)
        y = torch.empty(E, Bsz, L, D, dtype=torch.float32, device=x.device)
        slot, slot_p, epoch = _slot_args(amax_tracking() and y.numel() >= (1 << 20), x.device)
        check(lib().resel_member_conv1d_fwd(_p(x3), x3.stride(-2), int(shared), _p(w), _p(bias), _p(mask), _p(y), D, E, Bsz, L, D, K,
                                            slot_p, epoch, _stream()), 'member_conv1d_fwd')
        publish_amax(slot)
        ctx.save_for_backward(x3, w, bias, mask)
        ctx.cfg = (E, Bsz, L, D, K, shared, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        x3, w, bias, mask = ctx.saved_tensors
        E, Bsz, L, D, K, shared, xshape = ctx.cfg
        dy = _tok_major(dy.reshape(E * Bsz, L, D))
        dx = torch.empty(E, Bsz, L, D, dtype=torch.float32, device=dy.device)
        dx_sum = torch.empty(Bsz, L, D, dtype=torch.float32, device=dy.device) if shared else None
        dw = torch.empty(E, D, K, dtype=torch.float32, device=dy.device)
        db = torch.empty(E, D, dtype=torch.float32, device=dy.device) if bias is not None else None
        ws = _ws(lib().resel_member_conv1d_bwd_workspace_bytes(E, Bsz, L, D, K), dy.device)
        slot, slot_p, epoch = _slot_args(not shared and amax_tracking() and dx.numel() >= (1 << 20), dy.device)
        check(lib().resel_member_conv1d_bwd(_p(x3), x3.stride(-2), int(shared), _p(w), _p(bias), _p(mask), _p(dy), dy.stride(-2), _p(dx), D,
                                            _p(dx_sum), _p(dw), _p(db), _p(ws), E, Bsz, L, D, K, slot_p, epoch, _stream()), 'member_conv1d_bwd')
        return (dx_sum if shared else tag_amax(dx.view(xshape), slot)), dw, db, None


def member_conv1d(x, weight, bias=None, mask=None):
    """The `econv1d[_<K>]-<E>` convolution: see `MemberConv1dFn`."""
    return apply_tagged(MemberConv1dFn.apply, False, x, weight, bias, mask)


# ---------------------------------------------------------------------------------------------- add + norm
class AddNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps, rms, prenorm, act=None):
        _need_cuda('add_layernorm', x, weight)
        assert act in (None, 'elu')
        shape = x.shape
        C = shape[-1]
        x2 = x.float().reshape(-1, C).contiguous()
        r2 = None if residual is None else residual.float().reshape(-1, C).contiguous()
        M = x2.shape[0]
        w = weight.float().contiguous()
        b = None if bias is None else bias.float().contiguous()
        y = torch.empty_like(x2)
        need_res = residual is not None or prenorm
        res_out = torch.empty_like(x2) if need_res else None
        stats = torch.empty(M, 2, dtype=torch.float32, device=x.device)
        slot, slot_p, epoch = _slot_args(amax_tracking() and M * C >= (1 << 20), x.device)
        check(lib().resel_add_layernorm_fwd(_p(x2), _p(r2), _p(w), _p(b), _p(y), _p(res_out), _p(stats), M, C, float(eps),
                                            int(bool(rms)), int(act == 'elu'), slot_p, epoch, _stream()), 'add_layernorm_fwd')
        publish_amax(slot)
        ctx.save_for_backward(res_out if res_out is not None else x2, w, stats, b if act else None)
        ctx.rms, ctx.has_bias, ctx.has_res, ctx.prenorm, ctx.shape = bool(rms), b is not None, residual is not None, prenorm, shape
        ctx.act = int(act == 'elu')
        if prenorm:
            return y.reshape(shape), res_out.reshape(shape)
        return y.reshape(shape)

    @staticmethod
    def backward(ctx, dy, dres=None):
        res, w, stats, b = ctx.saved_tensors
        M, C = res.shape
        dy2 = dy.float().reshape(M, C).contiguous()
        dr2 = None if (dres is None or not ctx.prenorm) else dres.float().reshape(M, C).contiguous()
        dx = torch.empty_like(res)
        dw = torch.empty(C, dtype=torch.float32, device=res.device)
        db = torch.empty(C, dtype=torch.float32, device=res.device) if ctx.has_bias else None
        ws = _ws(lib().resel_add_layernorm_bwd_workspace_bytes(M, C), res.device)
        slot, slot_p, epoch = _slot_args(amax_tracking() and M * C >= (1 << 20), res.device)
        check(lib().resel_add_layernorm_bwd(_p(dy2), _p(dr2), _p(res), _p(w), _p(b), _p(stats), _p(dx), _p(dw), _p(db), _p(ws),
                                            M, C, int(ctx.rms), int(ctx.has_bias), ctx.act, slot_p, epoch, _stream()), 'add_layernorm_bwd')
        dx = tag_amax(dx.reshape(ctx.shape), slot, whole=True)      # the gradient the block below multiplies with its out_proj weight
        return dx, (dx if ctx.has_res else None), dw, db, None, None, None, None


def _add_norm(x, residual, weight, bias, eps, rms, prenorm, act=None):
    # the normalised output (the first one under prenorm) feeds a projection: its magnitude came out of the same pass
    return apply_tagged(AddNormFn.apply, True, x, residual, weight, bias, eps, rms, prenorm, act)


def layer_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False, act=None):
    """Signature of the reference's fused add+LayerNorm (mamba_ssm/ops/triton/layernorm.py `layer_norm_fn`).  act='elu' (this library's
    addition): the plain ELU that follows the layer, applied where the normalised output is stored."""
    return _add_norm(x, residual, weight, bias, eps, False, prenorm, act)


def rms_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False):
    return _add_norm(x, residual, weight, bias, eps, True, prenorm)


# ---------------------------------------------------------------------------------------------- ln / eln tails of the dense stacks
MEMBER_NORM_MAX = 2048          # E * C of a token the kernels take (csrc/member_layernorm.hip `MAX_ROW`)
NORM_FUSED_DEFAULT = '1'        # what an unset RESEL_NORM_FUSED means (README; measured in profiles/r26_norm_blocks.md)


def norm_fused_on():
    """RESEL_NORM_FUSED, read per call: 0 keeps the `ln+` / `eln-E+` tails of the dense stacks on the torch spelling."""
    return os.environ.get('RESEL_NORM_FUSED', NORM_FUSED_DEFAULT) != '0'


def member_layer_norm_ok(E, C):
    """The shapes `resel_member_layernorm_*` take (anything else is RESEL_EINVAL there)."""
    return C % 4 == 0 and 0 < E * C <= MEMBER_NORM_MAX


def _member_tokens(t, E, C):
    """t: [E, ..., C] (E == 1: [..., C]) -> (t3 [E, M, C] addressable in place, ld_e, ld_m): segment e of token m at
    `t3.data_ptr() + 4 (m ld_m + e ld_e)`.  The [E, ..., C] view of a shared-input EnsembleLinear's [M, E C] output qualifies as it is
    (ld_e = C, ld_m = E C), so does a dense tensor (ld_e = M C, ld_m = C) and a column block of a wider matrix; anything whose token
    axes do not collapse to ONE stride, or that is not 16-byte addressable, is copied to dense."""
    if t.dtype != torch.float32:
        t = t.float()
    try:
        t3 = t.view(E, -1, C)
    except RuntimeError:
        t3 = None
    if t3 is not None:
        se, sm, sc = t3.stride()
        M = t3.shape[1]
        if not (sc == 1 and t3.data_ptr() % 16 == 0 and (E == 1 or (se % 4 == 0 and se >= C)) and (M == 1 or (sm % 4 == 0 and sm >= C))):
            t3 = None
    if t3 is None:
        t3 = t.contiguous().view(E, -1, C)
    M = t3.shape[1]
    return t3, (t3.stride(0) if E > 1 else C), (t3.stride(1) if M > 1 else E * C)


def _like_tokens(t3, ld_e, ld_m):
    """Uninitialised [E, M, C] in t3's layout when that is one of the two dense ones (token-major [M, E C] seen as [E, M, C], or
    member-major), else member-major -> (tensor, ld_e, ld_m)."""
    E, M, C = t3.shape
    if E > 1 and M > 1 and (ld_e, ld_m) == (C, E * C):
        return torch.empty(M, E, C, dtype=torch.float32, device=t3.device).transpose(0, 1), C, E * C
    return torch.empty(E, M, C, dtype=torch.float32, device=t3.device), M * C, C


def _aligned_param(p):
    p = p.float().contiguous()
    return p if p.data_ptr() % 16 == 0 else p.clone()


class MemberLayerNormFn(torch.autograd.Function):
    """y = act(LayerNorm over the E C features of a token), weight / bias [E, C] (`eln-E`) or [C] (`ln`, E = 1), on the activations
    where their producer left them (include/resel_hip.h `resel_member_layernorm_*`); the gradient goes back in the input's layout."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, act):
        _need_cuda('member_layer_norm', x, weight, bias)
        assert act in (None, 'elu')
        C = x.shape[-1]
        E = weight.shape[0] if weight.dim() == 2 else 1
        assert weight.shape[-1] == C and (weight.dim() == 1 or (x.dim() >= 2 and x.shape[0] == E)), (tuple(x.shape), tuple(weight.shape))
        x3, lxe, lxm = _member_tokens(x, E, C)
        M = x3.shape[1]
        w = _aligned_param(weight)
        b = None if bias is None else _aligned_param(bias)
        y3, lye, lym = _like_tokens(x3, lxe, lxm)
        stats = torch.empty(M, 2, dtype=torch.float32, device=x.device)
        slot, slot_p, epoch = _slot_args(amax_tracking() and M * E * C >= (1 << 20), x.device)
        check(lib().resel_member_layernorm_fwd(_p(x3), lxe, lxm, _p(w), _p(b), _p(y3), lye, lym, _p(stats), M, E, C, float(eps),
                                               int(act == 'elu'), slot_p, epoch, _stream()), 'member_layernorm_fwd')
        publish_amax(slot)
        ctx.save_for_backward(x3, w, b, stats)
        ctx.cfg = (E, C, int(act == 'elu'), x.shape, weight.shape)
        return y3.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x3, w, b, stats = ctx.saved_tensors
        E, C, act, shape, wshape = ctx.cfg
        M = x3.shape[1]
        g3, lge, lgm = _member_tokens(dy, E, C)
        _, lxe, lxm = _member_tokens(x3, E, C)
        dx3, lde, ldm = _like_tokens(x3, lxe, lxm)
        dw = torch.empty(wshape, dtype=torch.float32, device=x3.device)
        db = None if b is None else torch.empty(wshape, dtype=torch.float32, device=x3.device)
        ws = _ws(lib().resel_member_layernorm_bwd_workspace_bytes(M, E, C), x3.device)
        slot, slot_p, epoch = _slot_args(amax_tracking() and M * E * C >= (1 << 20), x3.device)
        check(lib().resel_member_layernorm_bwd(_p(g3), lge, lgm, _p(x3), lxe, lxm, _p(w), _p(b), _p(stats), _p(dx3), lde, ldm, _p(dw), _p(db),
                                               _p(ws), M, E, C, act, slot_p, epoch, _stream()), 'member_layernorm_bwd')
        dx = tag_amax(dx3.view(shape), slot, whole=True)            # the gradient the layer in front multiplies with its weights
        return dx, dw, db, None, None


def member_layer_norm(x, weight, bias, eps=1e-5, act=None):
    """The `ln+<act>` / `eln-<E>+<act>` norm of a dense stack (reference rnn_base.py:250-258,461-467) with the ELU, if `act='elu'`, in the same
    pass.  x: [E, ..., C] with weight / bias [E, C] - one LayerNorm over all E x C features of a token, jointly across the members, what
    the reference spells `LayerNorm([E, C])(x.transpose(-2, 0)).transpose(-2, 0)` - or [..., C] with weight / bias [C].  The output
    carries the magnitude bound the kernel published, for the GEMM behind it."""
    return apply_tagged(MemberLayerNormFn.apply, True, x, weight, bias, eps, act)


class MemberAddLayerNormFn(torch.autograd.Function):
    """y = act(LN_[E, C](a + r)) for member-major a, r [E, ..., C]: the closing residual add + joint member LayerNorm of the ensemble
    feed-forward block in one pass (`resel_member_add_layernorm_fwd`); the backward is `resel_member_layernorm_bwd` on the saved sum,
    whose dx is the gradient of both addends."""

    @staticmethod
    def forward(ctx, a, r, weight, bias, eps, act):
        _need_cuda('member_add_layer_norm', a, r, weight, bias)
        assert act in (None, 'elu') and a.shape == r.shape and weight.dim() == 2
        E, C = weight.shape
        assert a.shape[0] == E and a.shape[-1] == C, (tuple(a.shape), tuple(weight.shape))
        a3, r3 = a.float().contiguous().view(E, -1, C), r.float().contiguous().view(E, -1, C)      # dense member-major: one stride pair
        M = a3.shape[1]
        w = _aligned_param(weight)
        b = None if bias is None else _aligned_param(bias)
        xsum, y3 = torch.empty_like(a3), torch.empty_like(a3)
        stats = torch.empty(M, 2, dtype=torch.float32, device=a.device)
        slot, slot_p, epoch = _slot_args(amax_tracking() and M * E * C >= (1 << 20), a.device)
        check(lib().resel_member_add_layernorm_fwd(_p(a3), _p(r3), _p(xsum), M * C, C, _p(w), _p(b), _p(y3), M * C, C, _p(stats), M, E, C,
                                                   float(eps), int(act == 'elu'), slot_p, epoch, _stream()), 'member_add_layernorm_fwd')
        publish_amax(slot)
        ctx.save_for_backward(xsum, w, b, stats)
        ctx.cfg = (E, C, int(act == 'elu'), a.shape, weight.shape)
        return y3.view(a.shape)

    @staticmethod
    def backward(ctx, dy):
        dx, dw, db, _, _ = MemberLayerNormFn.backward(ctx, dy)
        return dx, dx, dw, db, None, None


def member_add_layer_norm(a, r, weight, bias, eps=1e-5, act=None):
    """`member_layer_norm(a + r, ...)` with the add inside the norm's pass; shapes outside `member_layer_norm_ok` are the caller's to route."""
    return apply_tagged(MemberAddLayerNormFn.apply, True, a, r, weight, bias, eps, act)


# ---------------------------------------------------------------------------------------------- linear recurrences
def _token_rows(*ts):
    """[B, L, C] fp32 operands of a scan -> (operands usable in place, ld): their (b, t) axes collapse to token rows `ld` floats apart with unit
    column stride (dense tensors, or column blocks of one wider token-major matrix); anything else is copied to dense."""
    t0 = ts[0]
    ld = t0.stride(1)
    if all(t.dtype == torch.float32 and t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == ld and t.stride(0) == t.shape[1] * ld and ld >= t.shape[2]
           for t in ts):
        return ts, ld
    return tuple(t.float().contiguous() for t in ts), t0.shape[2]


def _member_rows(u):
    """u [E, B, L, C]: the members as token-row operands (see `_token_rows`) - the [E, B, T, C] view of a shared-input EnsembleLinear's
    [M, E C] output qualifies as it is (ld = E C), so does a dense tensor (ld = C).  Returns (u or a dense copy, ld)."""
    E, Bsz, L, C = u.shape
    if not (u.dtype == torch.float32 and u.stride(3) == 1 and u.stride(1) == L * u.stride(2) and u.stride(2) >= C):
        u = u.float().contiguous()
    return u, u.stride(2)


def _like_members(u):
    """Uninitialised tensor with u's shape AND memory layout (gradients of the members go back in the layout the producer reads)."""
    return torch.empty_strided(u.shape, u.stride(), dtype=torch.float32, device=u.device)


def _real_fwd(v, f, ld, start, h0, fuse_act):
    Bsz, L, C = v.shape
    h = torch.empty(Bsz, L, C, dtype=torch.float32, device=v.device)
    slot, slot_p, epoch = _slot_args(amax_tracking() and h.numel() >= (1 << 20), v.device)
    check(lib().resel_linrec_real_fwd(_p(v), _p(f), ld, _p(start), _p(h0), _p(h), Bsz, L, C, int(bool(fuse_act)), slot_p, epoch, _stream()),
          'linrec_real_fwd')
    publish_amax(slot)
    return h


def _real_bwd(v, f, ld, start, h0, h, dh, dv, df, ld_d, fuse_act, amax_d=None, epoch=0):
    """dv, df: token rows `ld_d` floats apart (dense tensors, or the two members of one tensor whose magnitude slot is amax_d)."""
    Bsz, L, C = v.shape
    check(lib().resel_linrec_real_bwd(_p(v), _p(f), ld, _p(start), _p(h0), _p(h), _p(dh), _p(dv), _p(df), ld_d, Bsz, L, C,
                                      int(fuse_act), amax_d, epoch, _stream()), 'linrec_real_bwd')


class GilrScanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, f, start, h0, fuse_act):
        _need_cuda('linrec_real', v, f)
        (v, f), ld = _token_rows(v, f)
        Bsz, L, C = v.shape
        start = _flags(start, Bsz, L)
        h0 = _h0(h0, Bsz, C)
        h = _real_fwd(v, f, ld, start, h0, fuse_act)
        ctx.save_for_backward(v, f, start, h0, h)
        ctx.act, ctx.ld = bool(fuse_act), ld
        return h

    @staticmethod
    def backward(ctx, dh):
        v, f, start, h0, h = ctx.saved_tensors
        Bsz, L, C = v.shape
        dh = dh.float().contiguous()
        dv = torch.empty(Bsz, L, C, dtype=torch.float32, device=v.device)
        df = torch.empty_like(dv)
        _real_bwd(v, f, ctx.ld, start, h0, h, dh, dv, df, C, ctx.act)
        return dv, df, None, None, None


class GilrMembersFn(torch.autograd.Function):
    """The gilr recurrence on u = (v | f) [2, B, T, C] as its producer left it (reference gilr.py:60-62 slices u[0], u[1]): the kernels
    read the two members through their row stride and write both gradients into ONE tensor of u's layout - no dense copies of the
    members going in (2 x 2 per call), no zero-filled [2, B, T, C] per member plus an add coming back (autograd's select_backward)."""

    @staticmethod
    def forward(ctx, u, start, h0, fuse_act):
        _need_cuda('linrec_real', u)
        assert u.dim() == 4 and u.shape[0] == 2
        u, ld = _member_rows(u)
        _, Bsz, L, C = u.shape
        start = _flags(start, Bsz, L)
        h0 = _h0(h0, Bsz, C)
        h = _real_fwd(u[0], u[1], ld, start, h0, fuse_act)
        ctx.save_for_backward(u, start, h0, h)
        ctx.act, ctx.ld = bool(fuse_act), ld
        return h

    @staticmethod
    def backward(ctx, dh):
        u, start, h0, h = ctx.saved_tensors
        dh = dh.float().contiguous()
        du = _like_members(u)
        slot, slot_p, epoch = _slot_args(amax_tracking() and du.numel() >= (1 << 20), u.device)
        _real_bwd(u[0], u[1], ctx.ld, start, h0, h, dh, du[0], du[1], du.stride(2), ctx.act, slot_p, epoch)
        return tag_amax(du, slot), None, None, None


def gilr_scan(v, f, start=None, h0=None, fuse_act=True):
    """h_t = f'_t h_{t-1} + (1 - f'_t) v'_t with v' = tanh(v), f' = sigmoid(f) (1 - start) when fuse_act."""
    return apply_tagged(GilrScanFn.apply, False, v, f, start, h0, fuse_act)


def gilr_scan_members(u, start=None, h0=None, fuse_act=True):
    """`gilr_scan(u[0], u[1], ...)` for u [2, B, T, C], reading the members in place (see `GilrMembersFn`)."""
    return apply_tagged(GilrMembersFn.apply, False, u, start, h0, fuse_act)


def real_scan_tie_input_gate(v, f):
    """Reference name (gilr/scan_triton/real_rnn_tie_input_gate.py:170-214): post-activation v, f; zero initial state."""
    return GilrScanFn.apply(v, f, None, None, False)


def _complex_fwd(vr, vi, ld, lam_re, lam_im, gamma, start, h0r, h0i):
    """-> h2 [2, B, L, C] = (Re h | Im h) stacked (the layer's next product wants exactly that), its magnitude handle."""
    Bsz, L, C = vr.shape
    h2 = torch.empty(2, Bsz, L, C, dtype=torch.float32, device=vr.device)
    slot, slot_p, epoch = _slot_args(amax_tracking() and h2.numel() >= (1 << 20), vr.device)
    check(lib().resel_linrec_complex_fwd(_p(vr), _p(vi), ld, _p(lam_re), _p(lam_im), _p(gamma), _p(start), _p(h0r), _p(h0i),
                                         _p(h2[0]), _p(h2[1]), Bsz, L, C, slot_p, epoch, _stream()), 'linrec_complex_fwd')
    return h2, slot


def _complex_args(lam_re, lam_im, gamma, start, h0r, h0i, Bsz, L, C):
    lam_re, lam_im = lam_re.float().contiguous(), lam_im.float().contiguous()
    gamma = None if gamma is None else gamma.float().contiguous()
    start = _flags(start, Bsz, L)
    return lam_re, lam_im, gamma, start, _h0(h0r, Bsz, C), _h0(h0i, Bsz, C)


def _complex_bwd(vr, vi, ld, lam_re, lam_im, gamma, start, h0r, h0i, h2, dh2, dvr, dvi, ld_du, dlr, dli, dg):
    """dvr, dvi: token rows `ld_du` floats apart; dlr, dli, dg [C]: separate tensors or the rows of one [3, C] tensor (dg None without gamma)."""
    Bsz, L, C = vr.shape
    ws = _ws(lib().resel_linrec_complex_bwd_workspace_bytes(Bsz, L, C), vr.device)
    check(lib().resel_linrec_complex_bwd(_p(vr), _p(vi), ld, _p(lam_re), _p(lam_im), _p(gamma), _p(start), _p(h0r), _p(h0i),
                                         _p(h2[0]), _p(h2[1]), _p(dh2[0]), _p(dh2[1]), _p(dvr), _p(dvi), ld_du, _p(dlr), _p(dli), _p(dg),
                                         _p(ws), Bsz, L, C, _stream()), 'linrec_complex_bwd')


class LruScanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vr, vi, lam_re, lam_im, gamma, start, h0r, h0i):
        _need_cuda('linrec_complex', vr, vi, lam_re, lam_im)
        (vr, vi), ld = _token_rows(vr, vi)
        Bsz, L, C = vr.shape
        lam_re, lam_im, gamma, start, h0r, h0i = _complex_args(lam_re, lam_im, gamma, start, h0r, h0i, Bsz, L, C)
        h2, _ = _complex_fwd(vr, vi, ld, lam_re, lam_im, gamma, start, h0r, h0i)
        ctx.save_for_backward(vr, vi, lam_re, lam_im, gamma, start, h0r, h0i, h2)
        ctx.ld = ld
        return h2[0], h2[1]

    @staticmethod
    def backward(ctx, dhr, dhi):
        vr, vi, lam_re, lam_im, gamma, start, h0r, h0i, h2 = ctx.saved_tensors
        Bsz, L, C = vr.shape
        dh2 = (dhr.float().contiguous(), dhi.float().contiguous())
        dvr = torch.empty(Bsz, L, C, dtype=torch.float32, device=vr.device)
        dvi = torch.empty_like(dvr)
        dlr, dli = torch.empty_like(lam_re), torch.empty_like(lam_im)
        dg = torch.empty_like(lam_re) if gamma is not None else None
        _complex_bwd(vr, vi, ctx.ld, lam_re, lam_im, gamma, start, h0r, h0i, h2, dh2, dvr, dvi, C, dlr, dli, dg)
        return dvr, dvi, dlr, dli, dg, None, None, None


class LruParamsFn(torch.autograd.Function):
    """params_log [3, C] (or [3, E, C]: the kernels are element-wise over the rows' E C entries) = (nu_log | theta_log | gamma_log) -> lam3 of the
    same shape = (lam_re | lam_im | gamma), lambda = exp(-exp(nu_log)) e^{i exp(theta_log)},
    gamma = exp(gamma_log) (reference lru.py:104-110): one launch each way instead of ~25 element-wise launches on [C] tensors per layer call."""

    @staticmethod
    def forward(ctx, params_log):
        _need_cuda('lru_params', params_log)
        p = params_log.float().contiguous()
        out = torch.empty_like(p)
        check(lib().resel_lru_params_fwd(_p(p), _p(out), p.numel() // 3, _stream()), 'lru_params_fwd')
        ctx.save_for_backward(p)
        return out

    @staticmethod
    def backward(ctx, dout):
        (p,) = ctx.saved_tensors
        dout = dout.float().contiguous()
        dp = torch.empty_like(p)
        check(lib().resel_lru_params_bwd(_p(p), _p(dout), _p(dp), p.numel() // 3, _stream()), 'lru_params_bwd')
        return dp


def lru_params(params_log):
    return LruParamsFn.apply(params_log)


class LruMembersFn(torch.autograd.Function):
    """The lru recurrence on u [E >= 2, B, T, C] as its producer left it (reference lru.py:112-120: members 0 / 1 are Re / Im of the
    input, member 2 the skip term): reads the members through their row stride, returns h2 = (Re h | Im h) stacked [2, B, T, C] (what
    `middle_proj` multiplies - no `torch.stack` copy) and, for E = 3, member 2 as a pass-through output so that ALL of u's gradient
    comes back through this node as one tensor of u's layout (blocks 0 / 1 written by the kernel, block 2 one copy).
    lam3 [3, C] = (lam_re | lam_im | gamma) (`lru_params`); its gradient comes back as one [3, C] tensor too."""

    @staticmethod
    def forward(ctx, u, lam3, start, h0r, h0i):
        _need_cuda('linrec_complex', u, lam3)
        assert u.dim() == 4 and u.shape[0] in (2, 3) and lam3.shape == (3, u.shape[3])
        u, ld = _member_rows(u)
        E, Bsz, L, C = u.shape
        lam3 = lam3.float().contiguous()
        _, _, _, start, h0r, h0i = _complex_args(lam3[0], lam3[1], lam3[2], start, h0r, h0i, Bsz, L, C)
        h2, slot = _complex_fwd(u[0], u[1], ld, lam3[0], lam3[1], lam3[2], start, h0r, h0i)
        publish_amax(slot)
        ctx.save_for_backward(u, lam3, start, h0r, h0i, h2)
        ctx.ld = ld
        return (h2, u[2]) if E == 3 else (h2, None)

    @staticmethod
    def backward(ctx, dh2, du2):
        u, lam3, start, h0r, h0i, h2 = ctx.saved_tensors
        dh2 = dh2.float().contiguous()
        du = _like_members(u)
        dlam3 = torch.empty_like(lam3)
        _complex_bwd(u[0], u[1], ctx.ld, lam3[0], lam3[1], lam3[2], start, h0r, h0i, h2, dh2, du[0], du[1], du.stride(2),
                     dlam3[0], dlam3[1], dlam3[2])
        if u.shape[0] == 3:
            if du2 is None:
                du[2].zero_()
            else:
                du[2].copy_(du2)
        return du, dlam3, None, None, None


def complex_scan(vr, vi, lam_re, lam_im, gamma=None, start=None, h0r=None, h0i=None):
    """h_t = lambda (1 - start_t) h_{t-1} + gamma (vr_t + i vi_t); lambda, gamma per channel [C]."""
    return LruScanFn.apply(vr, vi, lam_re, lam_im, gamma, start, h0r, h0i)


def complex_scan_members(u, lam3, start=None, h0r=None, h0i=None):
    """`complex_scan(u[0], u[1], lam3[0], lam3[1], lam3[2], ...)` for u [2 or 3, B, T, C] read in place and lam3 = `lru_params(params_log)`
    -> (h2 [2, B, T, C] = (Re h | Im h), u[2] or None); see `LruMembersFn`."""
    return apply_tagged(LruMembersFn.apply, False, u, lam3, start, h0r, h0i)


class LruEnsembleFn(torch.autograd.Function):
    """The lru recurrence of E members in one launch each way (`resel_linrec_complex_members_*`): u [3, E, B, T, C] (Re / Im of the
    input, skip term; reference elru.py:81-90), lam3 [3, E, C] = `lru_params` of the [3, E, C] parameters, start [B, T(, 1)] shared by the
    members, h0r / h0i [E, B, C] -> (h2 [2, E, B, T, C] = (Re h | Im h) stacked, what `middle_proj` multiplies; u[2] passed through so
    that all of u's gradient comes back as one tensor).  The gradient of lam3 is [3, E, C], reduced per member."""

    @staticmethod
    def forward(ctx, u, lam3, start, h0r, h0i):
        _need_cuda('linrec_complex_members', u, lam3)
        assert u.dim() == 5 and u.shape[0] == 3 and lam3.shape == (3, u.shape[1], u.shape[4]), (tuple(u.shape), tuple(lam3.shape))
        _, E, Bsz, L, C = u.shape
        if not (u.dtype == torch.float32 and u.stride(4) == 1 and u.stride(2) == L * u.stride(3) and u.stride(1) == Bsz * u.stride(2)
                and u.stride(3) >= C):
            u = u.float().contiguous()
        ld = u.stride(3)
        lam3 = lam3.float().contiguous()
        start = _flags(start, Bsz, L)
        h0r, h0i = _h0(h0r, E * Bsz, C), _h0(h0i, E * Bsz, C)
        h2 = torch.empty(2, E, Bsz, L, C, dtype=torch.float32, device=u.device)
        slot, slot_p, epoch = _slot_args(amax_tracking() and h2.numel() >= (1 << 20), u.device)
        check(lib().resel_linrec_complex_members_fwd(_p(u[0]), _p(u[1]), ld, _p(lam3[0]), _p(lam3[1]), _p(lam3[2]), _p(start), _p(h0r), _p(h0i),
                                                     _p(h2[0]), _p(h2[1]), E, Bsz, L, C, slot_p, epoch, _stream()), 'linrec_complex_members_fwd')
        publish_amax(slot)
        ctx.save_for_backward(u, lam3, start, h0r, h0i, h2)
        return h2, u[2]

    @staticmethod
    def backward(ctx, dh2, du2):
        u, lam3, start, h0r, h0i, h2 = ctx.saved_tensors
        _, E, Bsz, L, C = u.shape
        dh2 = dh2.float().contiguous()
        du = _like_members(u)
        dlam3 = torch.empty_like(lam3)
        ws = _ws(lib().resel_linrec_complex_members_bwd_workspace_bytes(E, Bsz, L, C), u.device)
        check(lib().resel_linrec_complex_members_bwd(_p(u[0]), _p(u[1]), u.stride(3), _p(lam3[0]), _p(lam3[1]), _p(lam3[2]), _p(start),
                                                     _p(h0r), _p(h0i), _p(h2[0]), _p(h2[1]), _p(dh2[0]), _p(dh2[1]), _p(du[0]), _p(du[1]),
                                                     du.stride(3), _p(dlam3[0]), _p(dlam3[1]), _p(dlam3[2]), _p(ws), E, Bsz, L, C, _stream()),
              'linrec_complex_members_bwd')
        if du2 is None:
            du[2].zero_()
        else:
            du[2].copy_(du2)
        return du, dlam3, None, None, None


def complex_scan_ensemble(u, lam3, start=None, h0r=None, h0i=None):
    """The `elru-<E>` recurrence, every member in one launch: see `LruEnsembleFn`."""
    return apply_tagged(LruEnsembleFn.apply, False, u, lam3, start, h0r, h0i)


class SubAddMembers(torch.autograd.Function):
    """m [2, ...] , r [...] -> m[0] - m[1] + r (lru.py:120 `mid[0] - mid[1] + u[2]`); the backward writes (g | -g) into ONE tensor of m's
    shape (autograd: a negation pass, two zero-filled [2, ...] tensors with one member copied in, and their sum)."""

    @staticmethod
    def forward(ctx, m, r):
        out = torch.sub(m[0], m[1])
        if r is not None:
            out.add_(r)
        ctx.has_r = r is not None
        return out

    @staticmethod
    def backward(ctx, g):
        dm = torch.empty((2,) + tuple(g.shape), dtype=g.dtype, device=g.device)
        dm[0].copy_(g)
        torch.neg(g, out=dm[1])
        return dm, (g if ctx.has_r else None)


# ---------------------------------------------------------------------------------------------- GRU
def _gru_operands(gi, w_hh, b_hh, h0):
    """The operands of a GRU recurrence as the kernels read them: dense fp32 gi [B, L, 3H], w_hh, b_hh and h0 [B, H] (or None)."""
    gi = gi.float().contiguous()
    Bsz, _, H3 = gi.shape
    return gi, w_hh.float().contiguous(), b_hh.float().contiguous(), _h0(h0, Bsz, H3 // 3)


class GruSeqFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gi, w_hh, b_hh, h0):
        _need_cuda('gru_seq', gi, w_hh, b_hh)
        gi, w_hh, b_hh, h0 = _gru_operands(gi, w_hh, b_hh, h0)
        Bsz, L, H3 = gi.shape
        H = H3 // 3
        need_grad = any(ctx.needs_input_grad)
        h_all = torch.empty(Bsz, L, H, dtype=torch.float32, device=gi.device)
        gates = torch.empty(Bsz, L, 4 * H, dtype=torch.float32, device=gi.device) if need_grad else None
        ws = _ws(lib().resel_gru_workspace_bytes(Bsz, L, H), gi.device)
        check(lib().resel_gru_seq_fwd(_p(gi), _p(w_hh), _p(b_hh), _p(h0), _p(h_all), _p(gates), _p(ws), Bsz, L, H, _stream()),
              'gru_seq_fwd')
        ctx.save_for_backward(w_hh, h0, h_all, gates)
        return h_all

    @staticmethod
    def backward(ctx, dh_all):
        w_hh, h0, h_all, gates = ctx.saved_tensors
        Bsz, L, H = h_all.shape
        dh_all = dh_all.float().contiguous()
        dgi = torch.empty(Bsz, L, 3 * H, dtype=torch.float32, device=h_all.device)
        dgh = torch.empty_like(dgi)
        ws = _ws(lib().resel_gru_workspace_bytes(Bsz, L, H), h_all.device)
        check(lib().resel_gru_seq_bwd(_p(w_hh), _p(h0), _p(h_all), _p(gates), _p(dh_all), _p(dgi), _p(dgh), _p(ws),
                                      Bsz, L, H, _stream()), 'gru_seq_bwd')
        # dW_hh = dgh^T h_prev over the B*L rows (`wgrad`: the K-split hand-written GEMM) and db_hh = sum dgh
        h_prev = torch.cat((torch.zeros(Bsz, 1, H, device=h_all.device) if h0 is None else h0.unsqueeze(1), h_all[:, :-1]), dim=1)
        dw_hh = wgrad(dgh.reshape(-1, 3 * H), h_prev.reshape(-1, H))
        db_hh = dgh.sum(dim=(0, 1))
        return dgi, dw_hh, db_hh, None


GRU_MAX_HIDDEN = 1024
# widths csrc/gru_seq.hip accepts (`pick_kc`): every multiple of 16 up to 256; the multiples of 16 up to 512 that split into 4 to 16
# pieces of 24 or 32; and 640, 768, 896, 1024, named one by one
GRU_NATIVE_WIDTHS = tuple(range(16, 257, 16)) + (288, 320, 336, 352, 384, 416, 448, 480, 512) + (640, 768, 896, 1024)
GruWidthPlan = collections.namedtuple('GruWidthPlan', 'Hk native')


def gru_width_plan(H: int) -> GruWidthPlan:
    """The kernel width a GRU of hidden width H runs at: (Hk, native).  A native width is itself; every other width from 1 to 1024 is
    zero-padded per gate block onto the smallest native width above it (a padded unit has zero parameters and a zero initial state: it
    stays exactly 0 and adds exactly 0 to the real units, forward and backward).  Host-only; the module, `gru_seq` and `gru_seq_multi`
    consult this and nothing else."""
    H = int(H)
    if H < 1 or H > GRU_MAX_HIDDEN:
        raise ValueError(f'gru: hidden width {H} is not supported: accepted are 1 to {GRU_MAX_HIDDEN} (native widths: the multiples of 16 up to 256 and '
                         f'{", ".join(map(str, GRU_NATIVE_WIDTHS[16:]))}; every other width zero-padded to the next of these); '
                         f'{GRU_MAX_HIDDEN} is this build\'s bound')
    Hk = next(w for w in GRU_NATIVE_WIDTHS if w >= H)
    return GruWidthPlan(Hk, Hk == H)


def gru_pad_rows(x, G, H, Hk):
    """x [..., G * H] -> [..., G * Hk], each of the G blocks zero-filled from H to Hk (`resel_gru_pad_rows`; no autograd)."""
    x = x.float().contiguous()
    out = torch.empty(x.shape[:-1] + (G * Hk,), dtype=torch.float32, device=x.device)
    check(lib().resel_gru_pad_rows(_p(x), _p(out), x.numel() // (G * H), G, H, Hk, _stream()), 'gru_pad_rows')
    return out


def gru_unpad_rows(x, G, H, Hk):
    """x [..., G * Hk] -> [..., G * H]: the first H of each block (`resel_gru_unpad_rows`; no autograd)."""
    x = x.float().contiguous()
    out = torch.empty(x.shape[:-1] + (G * H,), dtype=torch.float32, device=x.device)
    check(lib().resel_gru_unpad_rows(_p(x), _p(out), x.numel() // (G * Hk), G, H, Hk, _stream()), 'gru_unpad_rows')
    return out


class GruPadRowsFn(torch.autograd.Function):
    """Widen (`widen`) or narrow the G blocks of the last axis between H and Hk; the backward is the other pass."""

    @staticmethod
    def forward(ctx, x, G, H, Hk, widen):
        ctx.geom = (G, H, Hk, widen)
        return (gru_pad_rows if widen else gru_unpad_rows)(x, G, H, Hk)

    @staticmethod
    def backward(ctx, g):
        G, H, Hk, widen = ctx.geom
        return (gru_unpad_rows if widen else gru_pad_rows)(g, G, H, Hk), None, None, None, None


class GruPadParamsFn(torch.autograd.Function):
    """nn.GRU's parameters at the true width -> the same at the kernel width Hk, padded per gate block: (W_ih [3Hk, in], b_ih [3Hk],
    W_hh [3Hk, Hk], b_hh [3Hk]).  ONE node per forward, one launch each way (`resel_gru_pad_params` / `resel_gru_unpad_params`); the
    backward slices the four gradients back.  w_ih and b_ih may both be None (the recurrent parameters alone)."""

    @staticmethod
    def forward(ctx, w_ih, b_ih, w_hh, b_hh, Hk):
        _need_cuda('gru_pad_params', w_ih, b_ih, w_hh, b_hh)
        H = w_hh.shape[1]
        srcs = [None if t is None else t.float().contiguous() for t in (w_ih, b_ih, w_hh, b_hh)]
        n_in = 0 if w_ih is None else w_ih.shape[1]
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=w_hh.device)
        outs = [None if w_ih is None else new(3 * Hk, n_in), None if b_ih is None else new(3 * Hk), new(3 * Hk, Hk), new(3 * Hk)]
        check(lib().resel_gru_pad_params(*[_p(t) for t in srcs], *[_p(t) for t in outs], n_in, H, Hk, _stream()), 'gru_pad_params')
        ctx.geom = (n_in, H, Hk)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        n_in, H, Hk = ctx.geom
        grads = [None if g is None else g.float().contiguous() for g in grads]
        dev = grads[2].device
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        outs = [None if grads[0] is None else new(3 * H, n_in), None if grads[1] is None else new(3 * H), new(3 * H, H), new(3 * H)]
        check(lib().resel_gru_unpad_params(*[_p(t) for t in grads], *[_p(t) for t in outs], n_in, H, Hk, _stream()), 'gru_unpad_params')
        return tuple(outs) + (None,)


def gru_pad_params(w_ih, b_ih, w_hh, b_hh, Hk):
    return GruPadParamsFn.apply(w_ih, b_ih, w_hh, b_hh, Hk)


def gru_pad_state(h0, H, Hk):
    """Initial state [.., B, H] (or None) -> [B, Hk] with a zero tail: the state of a padded unit."""
    return None if h0 is None else gru_pad_rows(h0.detach().reshape(-1, H), 1, H, Hk)


def gru_narrow(y, H, Hk):
    """Hidden states at the kernel width [B, L, Hk] -> the true units [B, L, H]; the backward widens the gradient with zeros."""
    return GruPadRowsFn.apply(y, 1, H, Hk, False)


def _gru_widen_job(gi, w_hh, b_hh, h0, H, Hk):
    """A job at a true width that is not native -> the same job at Hk.  (The module pads its PARAMETERS and projects straight to
    [B, L, 3Hk]; a caller that arrives here with gi at the true width pays one pass over gi instead.)"""
    _need_cuda('gru_seq', gi, w_hh, b_hh, h0)
    _, _, w_hh_k, b_hh_k = gru_pad_params(None, None, w_hh, b_hh, Hk)
    return GruPadRowsFn.apply(gi, 3, H, Hk, True), w_hh_k, b_hh_k, gru_pad_state(h0, H, Hk)


def gru_seq(gi, w_hh, b_hh, h0=None):
    """gi = x W_ih^T + b_ih [B, L, 3H] -> all hidden states [B, L, H] (torch.nn.GRU gate order / formula).  Any H from 1 to 1024
    (`gru_width_plan`); a native width takes the kernels as it is."""
    H = gi.shape[-1] // 3
    Hk, native = gru_width_plan(H)
    if native:
        return GruSeqFn.apply(gi, w_hh, b_hh, h0)
    return gru_narrow(GruSeqFn.apply(*_gru_widen_job(gi, w_hh, b_hh, h0, H, Hk)), H, Hk)


GRU_MULTI_MAX = 4             # networks one `resel_gru_multi_fwd` launch takes


class _GruSeqAttachFn(torch.autograd.Function):
    """The autograd node of ONE differentiated job of `gru_seq_multi`: its forward ran in the shared launch (`done` = its h_all and
    saved gates), the backward is `GruSeqFn`'s - one `resel_gru_seq_bwd` + `wgrad` per job."""

    @staticmethod
    def forward(ctx, gi, w_hh, b_hh, h0, done):
        h_all, gates = done
        _, w_hh, _, h0 = _gru_operands(gi, w_hh, b_hh, h0)
        ctx.save_for_backward(w_hh, h0, h_all, gates)
        return h_all

    @staticmethod
    def backward(ctx, dh_all):
        return GruSeqFn.backward(ctx, dh_all) + (None,)


def gru_multi_form(n_net, Bsz, H) -> int:
    """1: `gru_seq_multi` runs n_net recurrences of this shape as one persistent launch, 0: as one launch per step."""
    form = lib().resel_gru_multi_form(int(n_net), int(Bsz), int(H))
    check(min(form, 0), 'gru_multi_form')
    return form


def gru_seq_multi(jobs):
    """jobs = [(gi, w_hh, b_hh, h0, need_grad), ...] (1 to 4 of them, equal [B, L, 3H]) -> [h_all, ...]: independent GRU recurrences
    that share ONE launch (`resel_gru_multi_fwd`) instead of one stream each.  Every output is bit for bit what `gru_seq` returns for
    that job alone.  A job with need_grad saves its gates and takes part in autograd; the others are constants whatever their
    tensors' `requires_grad` says (target networks, no-grad passes).  Jobs at a width that is not native are widened as `gru_seq`
    widens them (they share H, so they share the kernel width) and their outputs narrowed."""
    n = len(jobs)
    if not 1 <= n <= GRU_MULTI_MAX:
        raise ValueError(f'gru_seq_multi takes 1 to {GRU_MULTI_MAX} jobs, got {n}')
    H_true = jobs[0][0].shape[-1] // 3
    Hk, native = gru_width_plan(H_true)
    if not native:
        if any(tuple(j[0].shape) != tuple(jobs[0][0].shape) for j in jobs):
            raise ValueError('gru_seq_multi: the jobs of one launch share (B, L, H)')
        wide = []
        for gi, w_hh, b_hh, h0, need_grad in jobs:
            with torch.set_grad_enabled(bool(need_grad) and torch.is_grad_enabled()):
                wide.append(_gru_widen_job(gi, w_hh, b_hh, h0, H_true, Hk) + (need_grad,))
        return [gru_narrow(y, H_true, Hk) for y in gru_seq_multi(wide)]
    prep = []
    for gi, w_hh, b_hh, h0, need_grad in jobs:
        _need_cuda('gru_seq_multi', gi, w_hh, b_hh, h0)
        prep.append(_gru_operands(gi, w_hh, b_hh, h0))
    Bsz, L, H3 = prep[0][0].shape
    H = H3 // 3
    if any(tuple(p[0].shape) != (Bsz, L, H3) for p in prep):
        raise ValueError('gru_seq_multi: the jobs of one launch share (B, L, H)')
    dev = prep[0][0].device
    outs, saved = [], []
    for (gi, w_hh, b_hh, h0, need_grad), p in zip(jobs, prep):
        need = bool(need_grad) and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (gi, w_hh, b_hh))
        outs.append(torch.empty(Bsz, L, H, dtype=torch.float32, device=dev))
        saved.append(torch.empty(Bsz, L, 4 * H, dtype=torch.float32, device=dev) if need else None)
    ws = _ws(lib().resel_gru_multi_workspace_bytes(n, Bsz, L, H), dev)
    VP = ctypes.c_void_p * n
    arr = lambda ts: VP(*[None if t is None else t.data_ptr() for t in ts])
    check(lib().resel_gru_multi_fwd(n, arr([p[0] for p in prep]), arr([p[1] for p in prep]), arr([p[2] for p in prep]),
                                    arr([p[3] for p in prep]), arr(outs), arr(saved), _p(ws), Bsz, L, H, _stream()), 'gru_multi_fwd')
    res = []
    for (gi, w_hh, b_hh, h0, need_grad), p, h_all, gates in zip(jobs, prep, outs, saved):
        if gates is None:
            res.append(h_all)
        else:           # the node sees the caller's tensors (gradients flow to them) and saves the dense copies the kernel read
            res.append(_GruSeqAttachFn.apply(gi, w_hh, b_hh, h0, (h_all, gates)))
    return res


# ---------------------------------------------------------------------------------------------- attention (cgpt)
ATTN_KERNEL_WIDTHS = (32, 64, 128)           # head widths the attention and decode kernels are built for (csrc/attention.hip, rollout_step.hip)


def attn_head_pad(hd: int) -> int:
    """The kernel width a head width runs on: 32, 64 and 128 themselves, every other multiple of 8 up to 120 the next of them (zero
    columns: exact).  Anything else raises - flash-attn's 136..256 included, which this build does not cover."""
    hd = int(hd)
    if hd <= 0 or hd % 8 != 0 or hd > ATTN_KERNEL_WIDTHS[-1]:
        raise ValueError(f'cgpt attention: head width {hd} (embedding width / heads) is not supported: accepted are the multiples of 8 from 8 '
                         f'to 128 (32, 64 and 128 native, the others zero-padded to the next of these); flash-attn\'s 136 to 256 are out of scope')
    return next(w for w in ATTN_KERNEL_WIDTHS if w >= hd)


def _head_pad(x, hdp):
    """[T, n, H, hd] bf16 -> [T, n, H, hdp] with a zero tail (`resel_head_pad`)."""
    T, n, H, hd = x.shape
    out = torch.empty(T, n, H, hdp, dtype=torch.bfloat16, device=x.device)
    check(lib().resel_head_pad(_p(x), _p(out), T, n, H, hd, hdp, _stream()), 'head_pad')
    return out


def _head_unpad(x, hd):
    """[T, n, H, hdp] bf16 -> the first hd columns of every row, [T, n, H, hd] (`resel_head_unpad`)."""
    T, n, H, hdp = x.shape
    out = torch.empty(T, n, H, hd, dtype=torch.bfloat16, device=x.device)
    check(lib().resel_head_unpad(_p(x), _p(out), T, n, H, hd, hdp, _stream()), 'head_unpad')
    return out


class AttnVarlenFn(torch.autograd.Function):
    """A head width that is no kernel width runs zero-padded to the next one (`attn_head_pad`): qkv is padded once, the padded qkv / out
    are what the backward keeps, dout is padded and dqkv unpadded there.  `scale` is the caller's - that of the TRUE width."""

    @staticmethod
    def forward(ctx, qkv, cu_seqlens, max_seqlen, slopes, scale, p_drop, seed, offset, padded=False):
        _need_cuda('attn_varlen', qkv, cu_seqlens)
        assert qkv.dtype == torch.bfloat16 and qkv.dim() == 4 and qkv.shape[1] == 3
        hd_true = qkv.shape[-1]
        hdp = attn_head_pad(hd_true)
        qkv = qkv.contiguous()
        if hdp != hd_true:
            qkv = _head_pad(qkv, hdp)
        T, _, H, hd = qkv.shape
        cu = cu_seqlens.to(torch.int32).contiguous()
        S = cu.numel() - 1
        slopes = None if slopes is None else slopes.float().contiguous()
        out = torch.empty(T, H, hd, dtype=torch.bfloat16, device=qkv.device)
        lse = torch.empty(H, T, dtype=torch.float32, device=qkv.device)
        ws = _ws(lib().resel_attn_varlen_fwd_workspace_bytes(S, int(max_seqlen)), qkv.device)
        fwd = lib().resel_attn_varlen_fwd_padded if padded else lib().resel_attn_varlen_fwd
        check(fwd(_p(qkv), _p(cu), _p(slopes), _p(out), _p(lse), _p(ws), T, S, H, hd, int(max_seqlen), float(scale),
                  float(p_drop), int(seed), int(offset), _stream()), 'attn_varlen_fwd')
        ctx.save_for_backward(qkv, cu, slopes, out, lse)
        ctx.max_seqlen, ctx.scale, ctx.drop = int(max_seqlen), float(scale), (float(p_drop), int(seed), int(offset))
        ctx.padded, ctx.hd_true = bool(padded), hd_true
        return out if hd == hd_true else _head_unpad(out.view(T, 1, H, hd), hd_true).view(T, H, hd_true)

    @staticmethod
    def backward(ctx, dout):
        qkv, cu, slopes, out, lse = ctx.saved_tensors
        T, _, H, hd = qkv.shape
        dout = dout.to(torch.bfloat16).contiguous()
        if hd != ctx.hd_true:
            dout = _head_pad(dout.view(T, 1, H, ctx.hd_true), hd).view(T, H, hd)
        dqkv = torch.empty_like(qkv)
        ws = _ws(lib().resel_attn_varlen_bwd_workspace_bytes(T, cu.numel() - 1, H, hd, ctx.max_seqlen), qkv.device)
        bwd = lib().resel_attn_varlen_bwd_padded if ctx.padded else lib().resel_attn_varlen_bwd
        check(bwd(_p(qkv), _p(cu), _p(slopes), _p(out), _p(lse), _p(dout), _p(dqkv), _p(ws), T, cu.numel() - 1, H, hd,
                  ctx.max_seqlen, ctx.scale, *ctx.drop, _stream()), 'attn_varlen_bwd')
        if hd != ctx.hd_true:
            dqkv = _head_unpad(dqkv, ctx.hd_true)
        return dqkv, None, None, None, None, None, None, None, None


_MASK64 = (1 << 64) - 1


DROP_OVERRIDE = None           # [seed, next offset] while a GraphedUpdate body runs (recorded or eager): see dropout_offset_base
_DROP_BASE_KEEP = []           # the device words handed to resel_dropout_offset_base stay alive as long as the process


def dropout_offset_base(word):
    """Install (None: remove) the device int64 word that every counter-keyed mask kernel adds to its offset when it runs
    (include/resel_hip.h `resel_dropout_offset_base`): a captured update advances it with a node of its own graph, so that a replay
    - whose kernel nodes carry the host-drawn offsets of the recording - draws fresh masks."""
    if word is not None:
        assert word.is_cuda and word.dtype == torch.int64 and word.numel() == 1
        _DROP_BASE_KEEP.append(word)
    check(lib().resel_dropout_offset_base(_p(word)), 'dropout_offset_base')


def dropout_counter(device):
    """(seed, offset) for one counter-keyed dropout mask, taken from the device's default torch generator the way ATen's
    own dropout kernels reserve Philox offsets: host-side bookkeeping only (no sync), deterministic under
    `torch.manual_seed`, and every call gets a fresh offset.  Inside a GraphedUpdate body (torch's generator may not be
    queried while a stream is capturing) the draws count up from 0 per update and the device-side base makes updates differ."""
    if DROP_OVERRIDE is not None:
        off = DROP_OVERRIDE[1]
        DROP_OVERRIDE[1] = off + 4
        return DROP_OVERRIDE[0], off
    if not torch.cuda.default_generators:            # first CUDA touch of the process: the generator tuple is filled by the lazy init
        torch.cuda.init()
    gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
    off = gen.get_offset()
    gen.set_offset(off + 4)
    return gen.initial_seed() & _MASK64, off & _MASK64


def attn_varlen(qkv, cu_seqlens, max_seqlen, slopes=None, scale=None, p_drop=0.0, seed=0, offset=0, padded=False):
    """qkv [T, 3, H, hd] bf16 packed tokens -> out [T, H, hd] bf16: causal softmax(q k^T * scale - slope_h (i - j)) v per sequence.
    p_drop > 0: dropout on the attention probabilities with the keep mask keyed on (seed, offset) (see resel_hip.h).
    `padded`: the tables of a shape bucket - T may exceed cu_seqlens[-1] and sequences may be empty; the same kernels, then a pass
    that writes the token tail of out / lse (backward: dqkv) as zero (`resel_attn_varlen_fwd_padded`).
    hd: a multiple of 8 up to 128 (`attn_head_pad`; ValueError otherwise); the default scale is hd ** -0.5 of the width given here."""
    scale = qkv.shape[-1] ** -0.5 if scale is None else scale
    return AttnVarlenFn.apply(qkv, cu_seqlens, max_seqlen, slopes, scale, p_drop, seed, offset, padded)


# ------------------------------------------------------------------ token packing with a device-side count (padded sequence tables)
def _pack_rows(src, idx, n_dev):
    T, C = idx.numel(), src.shape[1]
    out = torch.empty(T, C, dtype=torch.float32, device=src.device)
    check(lib().resel_pack_rows(_p(src), src.stride(0), _p(idx), _p(n_dev), _p(out), C, T, C, _stream()), 'pack_rows')
    return out


def _unpack_rows(packed, idx, n_dev, M):
    T, C = packed.shape
    dst = torch.empty(M, C, dtype=torch.float32, device=packed.device)
    check(lib().resel_unpack_rows(_p(packed), packed.stride(0), _p(idx), _p(n_dev), _p(dst), C, M, T, C, _stream()), 'unpack_rows')
    return dst


def _rows_arg(name, x, idx, n_dev):
    _need_cuda(name, x, idx, n_dev)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] % 4 == 0, (name, x.dtype, tuple(x.shape))
    assert idx.dtype == torch.int64 and idx.dim() == 1 and idx.is_contiguous() and n_dev.dtype == torch.int32 and n_dev.numel() >= 1
    return x if x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 else x.contiguous()


class PackTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, idx, n_dev):
        flat = _rows_arg('pack_tokens', flat, idx, n_dev)
        ctx.save_for_backward(idx, n_dev)
        ctx.rows = flat.shape[0]
        return _pack_rows(flat, idx, n_dev)

    @staticmethod
    def backward(ctx, g):
        idx, n_dev = ctx.saved_tensors
        return _unpack_rows(_rows_arg('pack_tokens backward', g, idx, n_dev), idx, n_dev, ctx.rows), None, None


class UnpackTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, packed, idx, n_dev, rows):
        packed = _rows_arg('unpack_tokens', packed, idx, n_dev)
        assert packed.shape[0] == idx.numel(), (tuple(packed.shape), idx.numel())
        ctx.save_for_backward(idx, n_dev)
        return _unpack_rows(packed, idx, n_dev, int(rows))

    @staticmethod
    def backward(ctx, g):
        idx, n_dev = ctx.saved_tensors
        return _pack_rows(_rows_arg('unpack_tokens backward', g, idx, n_dev), idx, n_dev), None, None, None


def pack_tokens(flat, idx, n_dev):
    """flat [M, C] fp32, idx int64 [T] (a padded token table), n_dev int32 device word (its first element: the real token count, e.g.
    `cu_seqlens[-1:]`) -> [T, C]: row t is flat[idx[t]] for t < n, zero behind.  Backward: `unpack_tokens` of the gradient."""
    return PackTokensFn.apply(flat, idx, n_dev)


def unpack_tokens(packed, idx, n_dev, rows):
    """packed [T, C] fp32 -> [rows, C]: row idx[t] is packed[t] for t < n, every other row zero (all rows written by one kernel; idx
    strictly increasing over its real prefix).  Backward: `pack_tokens` of the gradient - a padded token gets a zero gradient."""
    return UnpackTokensFn.apply(packed, idx, n_dev, rows)


class CounterDropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p_drop, seed, offset):
        _need_cuda('dropout', x)
        assert x.dtype == torch.float32
        x = x.contiguous()
        y = torch.empty_like(x)
        check(lib().resel_dropout(_p(x), _p(y), x.numel(), float(p_drop), int(seed), int(offset), _stream()), 'dropout')
        ctx.drop = (float(p_drop), int(seed), int(offset))
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(lib().resel_dropout(_p(dy), _p(dx), dy.numel(), *ctx.drop, _stream()), 'dropout')
        return dx, None, None, None


def counter_dropout(x, p_drop, seed=None, offset=None):
    """Training-mode dropout of an fp32 tensor with a mask keyed on (seed, offset, flat element index); seed / offset default
    to a fresh `dropout_counter` draw."""
    if p_drop <= 0.0:
        return x
    if seed is None:
        seed, offset = dropout_counter(x.device)
    return CounterDropoutFn.apply(x, p_drop, seed, offset)


class GeluDropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p_drop, seed, offset):
        _need_cuda('gelu_dropout', x)
        assert x.dtype == torch.float32
        x = x.contiguous()
        y = torch.empty_like(x)
        slot, slot_p, epoch = _slot_args(amax_tracking() and x.numel() >= (1 << 20), x.device)
        check(lib().resel_gelu_dropout_fwd(_p(x), _p(y), x.numel(), float(p_drop), int(seed), int(offset), slot_p, epoch, _stream()), 'gelu_dropout_fwd')
        publish_amax(slot)
        ctx.save_for_backward(x)
        ctx.drop = (float(p_drop), int(seed), int(offset))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        slot, slot_p, epoch = _slot_args(amax_tracking() and dy.numel() >= (1 << 20), dy.device)
        check(lib().resel_gelu_dropout_bwd(_p(x), _p(dy), _p(dx), dy.numel(), *ctx.drop, slot_p, epoch, _stream()), 'gelu_dropout_bwd')
        return tag_amax(dx, slot), None, None, None


def gelu_dropout(x, p_drop, seed=None, offset=None):
    """dropout(gelu(x)) (erf GELU) as one kernel forward and one backward; the mask is the `counter_dropout` mask of the same
    (seed, offset) - one `dropout_counter` draw when p_drop > 0, none otherwise (plain GELU)."""
    if p_drop > 0.0 and seed is None:
        seed, offset = dropout_counter(x.device)
    return apply_tagged(GeluDropoutFn.apply, False, x, p_drop if p_drop > 0.0 else 0.0, seed or 0, offset or 0)


# ---------------------------------------------------------------------------------------------- SAC / TD3 arithmetic
class TanhGaussianFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out2, noise):
        _need_cuda('tanh_gaussian', out2, noise)
        shape = out2.shape
        A = shape[-1] // 2
        o2 = out2.float().reshape(-1, 2 * A).contiguous()
        nz = noise.float().reshape(-1, A).contiguous()
        M = o2.shape[0]
        mean, samp = torch.empty_like(nz), torch.empty_like(nz)
        logp = torch.empty(M, dtype=torch.float32, device=o2.device)
        check(lib().resel_tanh_gaussian_fwd(_p(o2), _p(nz), _p(mean), _p(samp), _p(logp), M, A, _stream()), 'tanh_gaussian_fwd')
        ctx.save_for_backward(o2, nz)
        ctx.shape = shape
        ctx.mark_non_differentiable(mean)
        out_shape = shape[:-1] + (A,)
        return mean.reshape(out_shape), samp.reshape(out_shape), logp.reshape(shape[:-1] + (1,))

    @staticmethod
    def backward(ctx, _dmean, dsamp, dlogp):
        o2, nz = ctx.saved_tensors
        M, A = nz.shape
        ds = None if dsamp is None else dsamp.float().reshape(M, A).contiguous()
        dl = None if dlogp is None else dlogp.float().reshape(M).contiguous()
        d2 = torch.empty_like(o2)
        check(lib().resel_tanh_gaussian_bwd(_p(o2), _p(nz), _p(ds), _p(dl), _p(d2), M, A, _stream()), 'tanh_gaussian_bwd')
        return d2.reshape(ctx.shape), None


def tanh_gaussian(out2, noise):
    """(logstd | mean) [..., 2A], noise [..., A] -> tanh(mean) (no grad), tanh(sample), log_prob [..., 1]."""
    return TanhGaussianFn.apply(out2, noise)


@torch.no_grad()
def sac_target(q, subset, next_logp, log_alpha, reward, done, mask, gamma, guard, stats=None, reduce_max=None, local_ext=None):
    """q [E, ...]; subset int32 [m] (device); guard fp32[4] device state {min, max, initialised, decay}.
    Data parallel, either
      local_ext (fp32 [4], default of the trainer): the target of the rank's own rows with the guard as it stands; the rank-local
        extrema go to local_ext, travel in the gradient bucket and reach the guard through `guard_apply_slots` - no collective here;
      reduce_max: in-place MAX all-reduce of a small device tensor - three phases with two 2-float exchanges inside the target."""
    _need_cuda('sac_target', q, reward, done, guard)
    E = q.shape[0]
    M = reward.numel()
    qf = q.float().reshape(E, M).contiguous()
    target = torch.empty(M, dtype=torch.float32, device=q.device)
    ws = _ws(lib().resel_sac_target_workspace_bytes(M), q.device)
    f = lambda t: None if t is None else t.float().reshape(-1).contiguous()
    nl, rw, dn, mk = f(next_logp), f(reward), f(done), f(mask)
    if local_ext is not None:
        check(lib().resel_sac_target_local(_p(qf), _p(subset), int(subset.numel()), _p(nl), _p(log_alpha), _p(rw), _p(dn), _p(mk),
                                           float(gamma), _p(guard), _p(target), _p(stats), _p(local_ext), _p(ws), E, M, _stream()), 'sac_target_local')
        return target.reshape(reward.shape)
    if reduce_max is not None:
        ext = torch.empty(4, dtype=torch.float32, device=q.device)
        for phase in range(3):
            check(lib().resel_sac_target_phase(phase, _p(qf), _p(subset), int(subset.numel()), _p(nl), _p(log_alpha), _p(rw), _p(dn), _p(mk),
                                               float(gamma), _p(guard), _p(target), _p(stats), _p(ext), _p(ws), E, M, _stream()), 'sac_target_phase')
            if phase < 2:
                reduce_max(ext[2 * phase:2 * phase + 2])
        return target.reshape(reward.shape)
    check(lib().resel_sac_target(_p(qf), _p(subset), int(subset.numel()), _p(nl), _p(log_alpha), _p(rw), _p(dn), _p(mk),
                                 float(gamma), _p(guard), _p(target), _p(stats), _p(ws), E, M, _stream()), 'sac_target')
    return target.reshape(reward.shape)


@torch.no_grad()
def redq_target(q, subset, next_logp, log_alpha, reward, done, gamma, stats=None):
    """The guard-less, mask-less target of the memoryless REDQ trainer (`resel_redq_target`): q [E, ...]; subset int32 [m] (device);
    -> reward + (1 - done) gamma (min over the subset - exp(log_alpha) next_logp), shaped like reward; stats[0] = max |target|."""
    _need_cuda('redq_target', q, subset, reward, done)
    assert subset.dtype == torch.int32 and subset.is_contiguous()
    E = q.shape[0]
    M = reward.numel()
    qf = q.float().reshape(E, M).contiguous()
    target = torch.empty(M, dtype=torch.float32, device=q.device)
    ws = _ws(lib().resel_sac_target_workspace_bytes(M), q.device)
    f = lambda t: None if t is None else t.float().reshape(-1).contiguous()
    nl, rw, dn = f(next_logp), f(reward), f(done)
    check(lib().resel_redq_target(_p(qf), _p(subset), int(subset.numel()), _p(nl), _p(log_alpha), _p(rw), _p(dn), float(gamma), _p(target),
                                  _p(stats), _p(ws), E, M, _stream()), 'redq_target')
    return target.reshape(reward.shape)


class MaskedQLossFn(torch.autograd.Function):
    """sum_m mask[m] sum_e (q[e, m] - y[m])^2 as ONE node (include/resel_hip.h `resel_q_loss_*`)."""

    @staticmethod
    def forward(ctx, q, y, mask):
        _need_cuda('q_loss', q, y)
        E = q.shape[0]
        q2, y1, m1 = q.float().reshape(E, -1).contiguous(), y.float().reshape(-1).contiguous(), None if mask is None else mask.float().reshape(-1).contiguous()
        M = y1.numel()
        out = torch.empty(2, dtype=torch.float32, device=q.device)
        ws = _ws(lib().resel_masked_loss_workspace_bytes(), q.device)
        check(lib().resel_q_loss_fwd(_p(q2), _p(y1), _p(m1), _p(out), _p(ws), E, M, _stream()), 'q_loss_fwd')
        ctx.save_for_backward(q2, y1, m1)
        ctx.shape = q.shape
        return out[0]

    @staticmethod
    def backward(ctx, g):
        q2, y1, m1 = ctx.saved_tensors
        E, M = q2.shape
        dq = torch.empty_like(q2)
        check(lib().resel_q_loss_bwd(_p(q2), _p(y1), _p(m1), _p(g.float().reshape(1).contiguous()), _p(dq), E, M, _stream()), 'q_loss_bwd')
        return dq.view(ctx.shape), None, None


def masked_q_loss(q, y, mask):
    return MaskedQLossFn.apply(q, y, mask)


class MaskedActorLossFn(torch.autograd.Function):
    """(sum_m mask (use_logp alpha logp - red_e q[e]), sum_m mask logp) as ONE node; red = mean (REDQ) or min (ensemble-min); alpha =
    exp(log_alpha) is a constant of the objective (the entropy coefficient has its own loss).  The second output carries no gradient."""

    @staticmethod
    def forward(ctx, logp, q, mask, log_alpha, use_logp, reduce_min):
        _need_cuda('actor_loss', q)
        E = q.shape[0]
        q2 = q.float().reshape(E, -1).contiguous()
        M = q2.shape[1]
        lp = None if logp is None else logp.float().reshape(-1).contiguous()
        m1 = None if mask is None else mask.float().reshape(-1).contiguous()
        la = log_alpha.detach().float().reshape(-1).contiguous()
        out = torch.empty(2, dtype=torch.float32, device=q.device)
        ws = _ws(lib().resel_masked_loss_workspace_bytes(), q.device)
        check(lib().resel_actor_loss_fwd(_p(lp), _p(q2), _p(m1), _p(la), _p(out), _p(ws), E, M, int(bool(use_logp)), int(bool(reduce_min)), _stream()),
              'actor_loss_fwd')
        ctx.save_for_backward(q2, m1, la)
        ctx.cfg = (bool(use_logp), bool(reduce_min), q.shape, None if logp is None else logp.shape)
        return out                                    # ONE output [2] = (objective sum, sum mask logp): the caller indexes it

    @staticmethod
    def backward(ctx, g2):
        q2, m1, la = ctx.saved_tensors
        g = g2[0:1]                                   # the second entry is a statistic (used detached)
        use_logp, reduce_min, qshape, lshape = ctx.cfg
        E, M = q2.shape
        dq = torch.empty_like(q2)
        dlp = torch.empty(M, dtype=torch.float32, device=q2.device) if use_logp else None
        check(lib().resel_actor_loss_bwd(_p(q2), _p(m1), _p(la), _p(g.float().reshape(1).contiguous()), _p(dlp), _p(dq), E, M, int(use_logp),
                                         int(reduce_min), _stream()), 'actor_loss_bwd')
        return (None if dlp is None or lshape is None else dlp.view(lshape)), dq.view(qshape), None, None, None, None


def masked_actor_loss(logp, q, mask, log_alpha, use_logp=True, reduce_min=False):
    out = MaskedActorLossFn.apply(logp, q, mask, log_alpha, use_logp, reduce_min)
    return out[0], out[1].detach()


# ---------------------------------------------------------------------------------------------- discrete-action update
def discrete_fused(t) -> bool:
    """RESEL_DISCRETE_FUSED (default on; 0: the torch spelling): the discrete-action update runs its head, target value and losses
    through the kernels below.  Only fp32 device tensors take the fused form."""
    return os.environ.get('RESEL_DISCRETE_FUSED', '1') != '0' and t.is_cuda and t.dtype == torch.float32


class CategoricalHeadFn(torch.autograd.Function):
    """logits [..., A] -> (mode [...] fp32, no grad; logp [..., A]; probs [..., A]) as ONE node (include/resel_hip.h
    `resel_categorical_fwd` / `_bwd`); the backward recomputes the softmax from the saved logits."""

    @staticmethod
    def forward(ctx, logits, floor):
        _need_cuda('categorical_head', logits)
        shape = logits.shape
        A = shape[-1]
        x = logits.float().reshape(-1, A).contiguous()
        M = x.shape[0]
        logp, probs = torch.empty_like(x), torch.empty_like(x)
        mode = torch.empty(M, dtype=torch.float32, device=x.device)
        if M > 0:
            check(lib().resel_categorical_fwd(_p(x), float(floor), _p(logp), _p(probs), _p(mode), M, A, _stream()), 'categorical_fwd')
        ctx.save_for_backward(x)
        ctx.cfg = (shape, float(floor))
        ctx.set_materialize_grads(False)
        mode = mode.reshape(shape[:-1])
        ctx.mark_non_differentiable(mode)
        return mode, logp.reshape(shape), probs.reshape(shape)

    @staticmethod
    def backward(ctx, _dmode, dlogp, dprobs):
        x, = ctx.saved_tensors
        shape, floor = ctx.cfg
        if dlogp is None and dprobs is None:
            return None, None
        M, A = x.shape
        f = lambda t: None if t is None else t.float().reshape(M, A).contiguous()
        dl, dp = f(dlogp), f(dprobs)
        dx = torch.empty_like(x)
        if M > 0:
            check(lib().resel_categorical_bwd(_p(x), floor, _p(dl), _p(dp), _p(dx), M, A, _stream()), 'categorical_bwd')
        return dx.reshape(shape), None


def categorical_head(logits, floor=0.01):
    """Whole-row categorical head (reference contextual_sac_discrete_policy.py:106-121): p = renormalised twice (softmax + floor)
    -> (mode = lowest argmax of p as fp32 [...], log p [..., A], p [..., A]); differentiable in logp and probs, one autograd node."""
    return CategoricalHeadFn.apply(logits, floor)


@torch.no_grad()
def discrete_value(q, subset, logp, log_alpha):
    """q [E, ..., A], logp [..., A], subset int32 [m] on the device or None (all E members), log_alpha a device scalar
    -> v [..., 1] = sum_a exp(logp) (min_{e in subset} q[e] - exp(log_alpha) logp)   (include/resel_hip.h `resel_discrete_value`)."""
    _need_cuda('discrete_value', q, logp, log_alpha, subset)
    E, A = q.shape[0], logp.shape[-1]
    lp = logp.float().reshape(-1, A).contiguous()
    M = lp.shape[0]
    q3 = q.float().reshape(E, M, A).contiguous()
    la = log_alpha.float().reshape(-1).contiguous()
    v = torch.empty(M, dtype=torch.float32, device=q.device)
    if subset is not None:
        assert subset.dtype == torch.int32
        subset = subset.reshape(-1).contiguous()
    if M > 0:
        check(lib().resel_discrete_value(_p(q3), _p(subset), 0 if subset is None else int(subset.numel()), _p(lp), _p(la), _p(v), E, M, A,
                                         _stream()), 'discrete_value')
    return v.reshape(logp.shape[:-1] + (1,))


class MaskedQTakenLossFn(torch.autograd.Function):
    """sum_m mask[m] sum_e (q[e, m, a_m] - y[m])^2 over q [E, ..., A] as ONE node (include/resel_hip.h `resel_q_taken_loss_*`): no gather
    in front, no zero-fill + scatter behind - the backward writes the dense dq the GEMM backward consumes."""

    @staticmethod
    def forward(ctx, q, action, y, mask):
        _need_cuda('q_taken_loss', q, action, y)
        E, A = q.shape[0], q.shape[-1]
        f = lambda t: None if t is None else t.float().reshape(-1).contiguous()
        a1, y1, m1 = f(action), f(y), f(mask)
        M = y1.numel()
        q3 = q.float().reshape(E, M, A).contiguous()
        assert a1.numel() == M and (m1 is None or m1.numel() == M)
        out = (torch.empty if M > 0 else torch.zeros)(2, dtype=torch.float32, device=q.device)
        ws = _ws(lib().resel_masked_loss_workspace_bytes(), q.device)
        if M > 0:
            check(lib().resel_q_taken_loss_fwd(_p(q3), _p(a1), _p(y1), _p(m1), _p(out), _p(ws), E, M, A, _stream()), 'q_taken_loss_fwd')
        ctx.save_for_backward(q3, a1, y1, m1)
        ctx.shape = q.shape
        return out[0]

    @staticmethod
    def backward(ctx, g):
        q3, a1, y1, m1 = ctx.saved_tensors
        E, M, A = q3.shape
        dq = torch.empty_like(q3)
        if M > 0:
            check(lib().resel_q_taken_loss_bwd(_p(q3), _p(a1), _p(y1), _p(m1), _p(g.float().reshape(1).contiguous()), _p(dq), E, M, A, _stream()),
                  'q_taken_loss_bwd')
        return dq.view(ctx.shape), None, None, None


def masked_q_taken_loss(q, action, y, mask):
    """q [E, ..., A]; action [..., 1]: the fp32 action index as the batch stores it; y, mask [..., 1]."""
    return MaskedQTakenLossFn.apply(q, action, y, mask)


class MaskedDiscreteActorLossFn(torch.autograd.Function):
    """(sum_m mask sum_a p (alpha logp - red_e q[e]), sum_m mask sum_a p logp) with p = exp(logp) as ONE node (include/resel_hip.h
    `resel_discrete_actor_loss_*`); the second output is a statistic and carries no gradient.  dq is formed only when q asks for one."""

    @staticmethod
    def forward(ctx, logp, q, mask, log_alpha, reduce_min):
        _need_cuda('discrete_actor_loss', logp, q)
        E, A = q.shape[0], logp.shape[-1]
        lp = logp.float().reshape(-1, A).contiguous()
        M = lp.shape[0]
        q3 = q.float().reshape(E, M, A).contiguous()
        m1 = None if mask is None else mask.float().reshape(-1).contiguous()
        assert m1 is None or m1.numel() == M
        la = log_alpha.detach().float().reshape(-1).contiguous()
        out = (torch.empty if M > 0 else torch.zeros)(2, dtype=torch.float32, device=q.device)
        ws = _ws(lib().resel_masked_loss_workspace_bytes(), q.device)
        if M > 0:
            check(lib().resel_discrete_actor_loss_fwd(_p(lp), _p(q3), _p(m1), _p(la), _p(out), _p(ws), E, M, A, int(bool(reduce_min)), _stream()),
                  'discrete_actor_loss_fwd')
        ctx.save_for_backward(lp, q3, m1, la)
        ctx.cfg = (bool(reduce_min), logp.shape, q.shape)
        total, stat = out[0], out[1]                  # two outputs, so that no select-backward (zero-fill + copy) sits behind the node
        ctx.mark_non_differentiable(stat)
        return total, stat

    @staticmethod
    def backward(ctx, g, _dstat):
        lp, q3, m1, la = ctx.saved_tensors
        reduce_min, lshape, qshape = ctx.cfg
        E, M, A = q3.shape
        g = g.float().reshape(1).contiguous()
        dlp = torch.empty_like(lp)
        dq = torch.empty_like(q3) if ctx.needs_input_grad[1] else None
        if M > 0:
            check(lib().resel_discrete_actor_loss_bwd(_p(lp), _p(q3), _p(m1), _p(la), _p(g), _p(dlp), _p(dq), E, M, A, int(reduce_min), _stream()),
                  'discrete_actor_loss_bwd')
        return dlp.view(lshape), (None if dq is None else dq.view(qshape)), None, None, None


def masked_discrete_actor_loss(logp, q, mask, log_alpha, reduce_min=False):
    """logp [..., A], q [E, ..., A], mask [..., 1] -> (objective sum, sum mask sum_a p logp (detached))."""
    total, stat = MaskedDiscreteActorLossFn.apply(logp, q, mask, log_alpha, reduce_min)
    return total, stat.detach()


@torch.no_grad()
def guard_apply_slots(slots, world, guard):
    """slots fp32 [world * 4] (every rank's extrema, delivered by the gradient all-reduce) -> first-call initialisation + running
    update of the Q guard from the extrema of the global batch (include/resel_hip.h `resel_guard_apply_slots`)."""
    _need_cuda('guard_apply_slots', slots, guard)
    check(lib().resel_guard_apply_slots(_p(slots), int(world), _p(guard), _stream()), 'guard_apply_slots')


# ---------------------------------------------------------------------------------------------- bias + activation tail
# codes 6 .. 9: the dense stacks' other activations (leaky_relu: torch's default slope 0.01); 4 / 5 are the fused critic forms' own entries
ACT_IDS = {None: 0, 'linear': 0, 'elu': 1, 'relu': 6, 'leaky_relu': 7, 'tanh': 8, 'sigmoid': 9}
GEMM_SOFTPLUS = 'softplus'           # resel_gemm_f32x only: softplus(product + bias) (epilogue code 3)
GEMM_ACCUMULATE = 'accumulate'       # resel_gemm_f32 only: C += product (epilogue code 2)
GEMM_EPILOGUES = {None: 0, 'linear': 0, 'elu': 1, GEMM_ACCUMULATE: 2, GEMM_SOFTPLUS: 3,       # `act` of resel_gemm_f32x (ACT_IDS: the ones bias_act knows)
                  'relu': 6, 'leaky_relu': 7, 'tanh': 8, 'sigmoid': 9}


def act_fused_on():
    """RESEL_ACT_FUSED (read per call so that one process can run both routes): relu, leaky_relu, tanh and sigmoid behind an fc / efc-E
    layer ride in the layer's GEMM epilogue like ELU (default); 0 = the torch modules of before.  ELU is not affected."""
    v = os.environ.get('RESEL_ACT_FUSED', '1')
    if v not in ('0', '1'):
        raise ValueError(f'RESEL_ACT_FUSED={v!r}: 0 or 1')
    return v == '1'


def dense_act_name(act_mod, x):
    """The epilogue name of the activation module behind an fc / efc-E layer whose input is x, or None when the module stays a module:
    a plain ELU always (as before); nn.ReLU, nn.LeakyReLU at torch's default slope, nn.Tanh, nn.Sigmoid on an fp32 GPU pass while
    RESEL_ACT_FUSED is on.  (gelu is not derivable from its output; another slope has no code.)"""
    if isinstance(act_mod, torch.nn.ELU):
        return 'elu' if act_mod.alpha == 1.0 else None
    name = {torch.nn.ReLU: 'relu', torch.nn.LeakyReLU: 'leaky_relu', torch.nn.Tanh: 'tanh', torch.nn.Sigmoid: 'sigmoid'}.get(type(act_mod))
    if name is None or (name == 'leaky_relu' and act_mod.negative_slope != 0.01):
        return None
    return name if (x.is_cuda and x.dtype == torch.float32 and act_fused_on()) else None


@torch.no_grad()
def bias_act_(y2, bias2, rows_per_seg, act):
    """In place on the GEMM output y2 [rows, C] (contiguous): y2 <- act(y2 + bias2[row // rows_per_seg]); bias2 [nseg, C] or None."""
    _need_cuda('bias_act', y2, bias2)
    assert y2.is_contiguous() and y2.dtype == torch.float32 and (bias2 is None or bias2.is_contiguous())
    check(lib().resel_bias_act_fwd(_p(y2), _p(bias2), y2.shape[0], y2.shape[1], int(rows_per_seg), ACT_IDS[act], _stream()), 'bias_act_fwd')
    tag_amax(y2, None)                                # rewritten in place
    return y2


@torch.no_grad()
def bias_act_bwd(g2, a2, rows_per_seg, act, need_dbias):
    """gy = g2 * act'(.) computed from the forward OUTPUT a2, dbias [nseg, C] = per-segment column sums of gy (or None)."""
    _need_cuda('bias_act_bwd', g2, a2)
    # a column block of a wider gradient (the halves of a `cat` backward) is read in place through its row stride
    if not (g2.dim() == 2 and g2.stride(1) == 1 and g2.stride(0) >= g2.shape[1] and g2.stride(0) % 4 == 0 and g2.data_ptr() % 16 == 0):
        g2 = g2.contiguous()
    rows, C = g2.shape
    aid = ACT_IDS[act]
    if aid == 0 and not need_dbias:
        return g2, None
    if aid and not (a2.dim() == 2 and a2.stride(1) == 1 and a2.stride(0) >= C and a2.stride(0) % 4 == 0 and a2.data_ptr() % 16 == 0):
        a2 = a2.contiguous()                          # (a block of a row buffer qualifies as it is)
    gy = torch.empty(rows, C, dtype=torch.float32, device=g2.device) if aid else g2
    nseg = rows // int(rows_per_seg)
    db = torch.empty(nseg, C, dtype=torch.float32, device=g2.device) if need_dbias else None
    ws = _ws(lib().resel_bias_act_bwd_workspace_bytes(rows, C, int(rows_per_seg)), g2.device) if need_dbias else None
    slot, slot_p, epoch = _slot_args(amax_tracking() and rows * C >= (1 << 20), g2.device)
    check(lib().resel_bias_act_bwd(_p(g2), g2.stride(0), _p(a2) if aid else None, a2.stride(0) if aid else 0, _p(gy) if aid else None, _p(db), _p(ws), rows, C, int(rows_per_seg), aid,
                                   slot_p, epoch, _stream()), 'bias_act_bwd')
    tag_amax(gy, slot)
    return gy, db


@torch.no_grad()
def ensemble_head_fwd_(y3, b2, w3, b3):
    """y3 [E, M, H] (GEMM output, overwritten with a = elu(y + b2)), b2 / w3 [E, H], b3 [E] -> q [E, M]."""
    _need_cuda('ensemble_head', y3, b2, w3, b3)
    E, M, H = y3.shape
    q = torch.empty(E, M, dtype=torch.float32, device=y3.device)
    check(lib().resel_ensemble_head_fwd(_p(y3), _p(b2), _p(w3), _p(b3), _p(q), E * M, H, M, _stream()), 'ensemble_head_fwd')
    tag_amax(y3, None)                                # rewritten in place: the GEMM's magnitude no longer describes it
    return q


@torch.no_grad()
def ensemble_head_bwd(gq, a3, w3):
    """gq [E, M], a3 [E, M, H], w3 [E, H] -> gy [E, M, H], db2 [E, H], dw3 [E, H]."""
    _need_cuda('ensemble_head_bwd', gq, a3, w3)
    E, M, H = a3.shape
    gq = gq if gq.is_contiguous() else gq.contiguous()
    gy = torch.empty_like(a3)
    db2 = torch.empty(E, H, dtype=torch.float32, device=a3.device)
    dw3 = torch.empty(E, H, dtype=torch.float32, device=a3.device)
    ws = _ws(lib().resel_ensemble_head_bwd_workspace_bytes(E * M, H, M), a3.device)
    slot, slot_p, epoch = _slot_args(amax_tracking() and E * M * H >= (1 << 20), a3.device)
    check(lib().resel_ensemble_head_bwd(_p(gq), _p(a3), _p(w3), _p(gy), _p(db2), _p(dw3), _p(ws), E * M, H, M, slot_p, epoch, _stream()),
          'ensemble_head_bwd')
    tag_amax(gy, slot)
    return gy, db2, dw3


class LinearAct(torch.autograd.Function):
    """act(x W^T + b) for nn.Linear weights (reference rnn_base.py:462-474: `fc` layer followed by its activation module):
    one GEMM with the bias / activation tail (`mm_nt`); the backward needs the layer OUTPUT only.  An input width (17- / 6-wide
    encoders) or an output width (6-wide TD3 action head) that is not a multiple of 4 is zero-padded inside the node - exact zeros
    in every dot product, the padding rows / columns of the gradients are dropped - so that every contraction runs on the
    matrix-core editions of the hand-written GEMM."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, dest=None):
        """dest: a `ColDest` - the column block of a row buffer the output should be written to in place (when it fits and no output
        column is padded; otherwise the output is a fresh tensor and whoever assembles the buffer copies it in)."""
        x2 = x.reshape(-1, x.shape[-1])
        x2 = x2 if x2.stride(-1) == 1 else x2.contiguous()
        ctx.kpad = (-x2.shape[1]) % 4
        ctx.npad = (-weight.shape[0]) % 4
        n_out = weight.shape[0]
        if ctx.kpad or ctx.npad:
            x2 = torch.nn.functional.pad(x2, (0, ctx.kpad)) if ctx.kpad else x2
            weight = torch.nn.functional.pad(weight, (0, ctx.kpad, 0, ctx.npad))
            bias = torch.nn.functional.pad(bias, (0, ctx.npad)) if (bias is not None and ctx.npad) else bias
        if dest is not None and not ctx.npad and dest.fits(x2.shape[0], weight.shape[0]):
            y2 = mm_nt(x2, weight, bias, act, out=dest.view(), amax_out=dest.rb.amax if dest.rb.handle() is not None else None)
            dest.note(y2)
        else:
            y2 = mm_nt(x2, weight, bias, act)
        ctx.ax = keep_handles(amax_of(x2))[0]         # the input's magnitude handle, for the weight gradient (saved tensors come back untagged)
        ctx.save_for_backward(x2, weight, y2)
        ctx.act, ctx.has_bias, ctx.xshape = act, bias is not None, x.shape
        out = y2[:, :n_out] if ctx.npad else y2
        return out.reshape(*x.shape[:-1], n_out)

    @staticmethod
    def backward(ctx, g):
        x2, weight, y2 = ctx.saved_tensors
        n_out = y2.shape[1] - ctx.npad
        g2 = g.reshape(y2.shape[0], n_out)
        if ctx.npad:
            g2 = torch.nn.functional.pad(g2, (0, ctx.npad))
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        gy, db = bias_act_bwd(g2, y2, y2.shape[0], ctx.act, need_db)
        dx = mm_nn(gy, weight) if ctx.needs_input_grad[0] else None
        dw = wgrad(gy, x2, amax_x=handle_alive(ctx.ax)) if ctx.needs_input_grad[1] else None
        if ctx.kpad or ctx.npad:                      # drop the padding rows / columns again
            k = x2.shape[1] - ctx.kpad
            dx = None if dx is None else dx[:, :k]
            dw = None if dw is None else dw[:n_out, :k]
            db = None if db is None else db.reshape(-1)[:n_out]
        dx = None if dx is None else dx.reshape(ctx.xshape)
        return dx, dw, None if db is None else db.reshape(-1), None, None


class PlaceBlocksFn(torch.autograd.Function):
    """out [rows, cols] = zeros with the source blocks copied in at their (r0, c0) (include/resel_hip.h `resel_place_blocks`): ONE launch for what
    block_diag / cat / pad assemble in several; the backward hands every source the matching slice of the gradient as a VIEW.
    srcs: fp32 tensors [..., nc_i]; their leading axes collapse to the nr_i rows of the block."""

    @staticmethod
    def forward(ctx, rows, cols, origins, *srcs):
        _need_cuda('place_blocks', *srcs)
        n = len(srcs)
        assert 1 <= n <= 8 and len(origins) == n
        s2 = []
        for t in srcs:
            t2 = t.reshape(-1, t.shape[-1])                                    # a view whenever the leading axes collapse
            s2.append(t2 if (t2.dtype == torch.float32 and t2.stride(1) == 1) else t2.float().contiguous())
        out = torch.empty(rows, cols, dtype=torch.float32, device=srcs[0].device)
        VP, LL, II = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
        check(lib().resel_place_blocks(_p(out), cols, rows, cols, n, VP(*[t.data_ptr() for t in s2]), LL(*[t.stride(0) for t in s2]),
                                       II(*[o[0] for o in origins]), II(*[t.shape[0] for t in s2]), II(*[o[1] for o in origins]),
                                       II(*[t.shape[1] for t in s2]), _stream()), 'place_blocks')
        ctx.meta = [(o[0], o[1], t2.shape[0], t2.shape[1], tuple(t.shape)) for o, t2, t in zip(origins, s2, srcs)]
        return out

    @staticmethod
    def backward(ctx, g):
        outs = []
        for need, (r0, c0, nr, nc, shape) in zip(ctx.needs_input_grad[3:], ctx.meta):
            outs.append(g[r0:r0 + nr, c0:c0 + nc].reshape(shape) if need else None)    # a view of g (rows of a block keep g's row stride)
        return (None, None, None) + tuple(outs)


def place_blocks(rows, cols, origins, *srcs):
    return PlaceBlocksFn.apply(int(rows), int(cols), tuple((int(r), int(c)) for r, c in origins), *srcs)


def linear_act(x, weight, bias, act, dest=None):
    # (an output written into a row buffer is a view of it: its magnitude must not be taken for the whole buffer's)
    return apply_tagged(LinearAct.apply, dest is None, x, weight, bias, act, dest)


# ---- row buffers: the column blocks of ONE token-major matrix written in place by the GEMMs that produce them -----------------------
class RowBuffer:
    """[M, width] fp32 with M = prod(lead): what `torch.cat([...], -1)` of several layer outputs would build, allocated up front so that
    each producer's GEMM writes its column block directly (`dest=` of `linear_act`; reference contextual_model.py cat of the input
    encoding and the embedding, contextual_sac_value.py:101-107).  The producers publish into ONE magnitude handle (the buffer's);
    `cat_into` hands the buffer on - copying in whatever did not land in place - as one autograd node whose backward slices."""

    def __init__(self, lead, width, device):
        self.lead, self.width = tuple(int(v) for v in lead), int(width)
        self.rows = 1
        for v in self.lead:
            self.rows *= v
        self.buf = torch.empty(self.rows, self.width, dtype=torch.float32, device=device)
        self.amax = _slot_args(amax_tracking() and self.rows * self.width >= (1 << 20), self.buf.device)     # (handle, pointer, epoch)
        # the handle's tenant serial AT ALLOCATION: the arena has 2 048 slots and a deep embedding tower (or RESEL_AMAX_VERIFY) may hand
        # out more than that between this constructor and `cat_into` - the slot then belongs to another tensor and no tag may name it
        self.serial = getattr(self.amax[0], '_resel_serial', None)
        self.published = 0                               # columns whose producer published into the handle

    def handle(self):
        """The buffer's magnitude handle while its arena slot still has the tenant it had at allocation, else None."""
        h = self.amax[0]
        return h if h is not None and getattr(h, '_resel_serial', None) == self.serial else None

    def block(self, col0, n):
        return ColDest(self, col0, n)


class ColDest:
    def __init__(self, rb, col0, n):
        self.rb, self.col0, self.n = rb, int(col0), int(n)

    def view(self):
        return self.rb.buf[:, self.col0:self.col0 + self.n]

    def fits(self, rows, n):
        return rows == self.rb.rows and n == self.n and self.col0 % 4 == 0 and self.n % 4 == 0

    def holds(self, t):
        """t (any leading shape) IS this block of the buffer."""
        if t.shape[-1] != self.n or t.numel() != self.rb.rows * self.n or t.dtype != torch.float32:
            return False
        v = self.view()
        return t.data_ptr() == v.data_ptr() and t.stride(-1) == 1 and (t.dim() < 2 or t.stride(-2) == self.rb.width) and \
            t.untyped_storage().data_ptr() == v.untyped_storage().data_ptr()

    def note(self, y2):
        if self.holds(y2):
            self.rb.published += self.n


class CatInto(torch.autograd.Function):
    """pieces (tensor_i at column col0_i of the row buffer) -> the whole buffer as [lead..., width]; pieces that are already in place cost
    nothing, the others one strided copy each.  Backward: column slices of the gradient (views)."""

    @staticmethod
    def forward(ctx, rb, col0s, *pieces):
        for c0, t in zip(col0s, pieces):
            d = rb.block(c0, t.shape[-1])
            if not d.holds(t):
                # copied by this library's own kernel: an ATen copy_ would bump the version counter the buffer shares with the views that the
                # in-place producers saved for their backward
                t2 = t.reshape(rb.rows, t.shape[-1])
                t2 = t2 if (t2.dtype == torch.float32 and t2.stride(1) == 1) else t2.float().contiguous()
                _need_cuda('cat_into', t2)
                check(lib().resel_place_blocks(_p(d.view()), rb.width, rb.rows, d.n, 1, (ctypes.c_void_p * 1)(t2.data_ptr()), (ctypes.c_int64 * 1)(t2.stride(0)),
                                               (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(rb.rows), (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(d.n), _stream()),
                      'cat_into')
        ctx.meta = [(c0, t.shape[-1], tuple(t.shape)) for c0, t in zip(col0s, pieces)]
        return rb.buf.detach().view(*rb.lead, rb.width)

    @staticmethod
    def backward(ctx, g):
        g2 = g.reshape(-1, g.shape[-1])
        outs = [g2[:, c0:c0 + n].view(shape) if need else None for need, (c0, n, shape) in zip(ctx.needs_input_grad[2:], ctx.meta)]
        return (None, None) + tuple(outs)


def cat_into(rb, pieces):
    """pieces: [(tensor, col0), ...] covering the buffer's columns."""
    complete = all(rb.block(c, t.shape[-1]).holds(t) for t, c in pieces) and sum(t.shape[-1] for t, _ in pieces) == rb.width \
        and rb.published == rb.width
    out = CatInto.apply(rb, tuple(int(c) for _, c in pieces), *[t for t, _ in pieces])
    return tag_amax(out, rb.handle() if complete else None, whole=True)


def linear(x, weight, bias=None):
    """x W^T + b for an fp32 nn.Linear: the `LinearAct` node (hand-written GEMM forward, input and weight gradients) for every pass -
    the whole trajectories of an update and the single token of a rollout step alike (`resel_gemm_f32x` takes every shape: the matrix-core
    editions where the layout allows them, csrc/gemm_any.hip for the rest).  An input width that is not a multiple of 4 (the 17-wide
    observation / 6-wide action encoders) is zero-padded to 16-byte rows inside the node.  There is no library GEMM behind this module;
    CPU tensors raise in `gemm_f32`."""
    return linear_act(x, weight, bias, None)


def gemm_f32_ok(*mats):
    """True when `resel_gemm_f32` takes these operands as they are: on the GPU, fp32, unit column stride (any row count and alignment: the
    C entry routes shapes the matrix-core editions cannot read to csrc/gemm_any.hip)."""
    return all(t.is_cuda and t.dtype == torch.float32 and t.stride(-1) == 1 for t in mats)


def rows_aligned16(*mats):
    """Every row of every operand starts on a 16-byte boundary and is a whole number of float4s: what the matrix-core editions (and their
    fused epilogues, which have no other form) read: the host-side mirror of `gemm_mfma_readable` (csrc/gemm_call.h), which decides."""
    return all(t.data_ptr() % 16 == 0 and t.shape[-1] % 4 == 0 and all(st % 4 == 0 for st in t.stride()[:-1])
               and (t.dim() < 2 or t.stride(-2) < (1 << 22)) for t in mats)


def _unit(t):
    """t with unit column stride (what the C entry's row-stride description needs); a copy only for exotic views."""
    return t if t.stride(-1) == 1 else t.contiguous()


def mm_nt(x2, w, bias=None, act=None, out=None, amax_out=None):
    """act(x2 [M, K] w[N, K]^T + bias): forward of an nn.Linear-shaped layer over the tokens of a pass, bias / ELU in the GEMM epilogue.
    out (with amax_out): a column block of a row buffer to write in place."""
    ACT_IDS[act]                                                       # 0: identity ('linear' / None), 1: ELU; anything else is a KeyError
    x2, w = _unit(x2), _unit(w)
    if out is not None and out.stride(-1) == 1:
        return gemm_f32(x2, w, True, True, bias, act, out=out, amax_out=amax_out)
    return gemm_f32(x2, w, True, True, bias, act)


def mm_nn(g2, w, out=None):
    """g2 [M, N] w[N, K] -> [M, K]: input gradient of such a layer.  out: a (possibly row-strided) destination, e.g. a column block of a
    wider buffer."""
    return gemm_f32(_unit(g2), _unit(w), True, False, out=out)


def wgrad(gy, x2, amax_x=None):
    """dW [out, in] = gy[M, out]^T x2[M, in] over the M tokens of a pass: the hand-written K-split GEMM (at 66 752 tokens:
    [128, 256] 49 us against the library's 234, [2048, 384] 731 against 1217, [256, 256] 86 against 123; `tools/bench_gemm_f32.py`)."""
    return gemm_f32(_unit(gy), _unit(x2), False, False, amax_b=amax_x)


@torch.no_grad()
def gather_trajs(buffer, segments, max_len, skip, rows, row_len, c_mask, c_start, c_done, c_timeout, pre_pairs, sel=None):
    """Packed batch [rows, row_len, W + 3] from the device ring `buffer` [capacity, W] and the int32 plan `segments` [nseg, 4]
    (row, first slot, length incl. skip, first transition); see include/resel_hip.h `resel_gather_trajs`.  `sel`: the int32 selection
    of loss positions that goes with the plan ([nseg word offsets | bitmap words], `resel_gather_trajs_sel`; it may be longer than the
    plan needs - a static buffer)."""
    _need_cuda('gather_trajs', buffer, segments, pre_pairs, *(() if sel is None else (sel,)))
    assert buffer.dtype == torch.float32 and buffer.is_contiguous() and segments.dtype == torch.int32 and segments.is_contiguous()
    assert sel is None or (sel.dtype == torch.int32 and sel.dim() == 1 and sel.is_contiguous())
    W = buffer.shape[1]
    out = torch.empty(rows, row_len, W + 3, dtype=torch.float32, device=buffer.device)
    check(lib().resel_gather_trajs_sel(_p(buffer), W, buffer.shape[0], _p(segments), segments.shape[0], int(max_len), int(skip), int(rows),
                                       int(row_len), int(c_mask), int(c_start), int(c_done), int(c_timeout), _p(pre_pairs), pre_pairs.shape[0],
                                       None if sel is None else _p(sel), 0 if sel is None else sel.numel(), _p(out), _stream()), 'gather_trajs')
    return out


@torch.no_grad()
def gather_transitions(buffer, rows_dev, pass_word=None, p=0, c_done=0, c_timeout=-1):
    """Transition batch [batch, W] from the device ring `buffer` [capacity, W]: row n is ring row `rows_dev[p, n]` (int32
    [passes, batch]); the pass is `p`, or the int32 device word `pass_word` when given.  `c_timeout >= 0`: done is 0 where timeout > 0.
    See include/resel_hip.h `resel_gather_transitions`."""
    _need_cuda('gather_transitions', buffer, rows_dev, *(() if pass_word is None else (pass_word,)))
    assert buffer.dtype == torch.float32 and buffer.dim() == 2 and buffer.is_contiguous()
    assert rows_dev.dtype == torch.int32 and rows_dev.dim() == 2 and rows_dev.is_contiguous()
    assert pass_word is None or (pass_word.dtype == torch.int32 and pass_word.numel() >= 1)
    W = buffer.shape[1]
    passes, batch = rows_dev.shape
    out = torch.empty(batch, W, dtype=torch.float32, device=buffer.device)
    check(lib().resel_gather_transitions(_p(buffer), W, buffer.shape[0], _p(rows_dev), int(passes), int(batch), int(p), _p(pass_word),
                                         int(c_done), int(c_timeout), _p(out), _stream()), 'gather_transitions')
    return out


@torch.no_grad()
def gather_slices(buffer, plan_dev, length, pre_pairs, pass_word=None, p=0, c_done=0, c_timeout=-1):
    """Slice batch [batch, length + 1, W] from the device ring `buffer` [capacity, W] and the int32 plan `plan_dev` [passes, batch, 2] =
    (ring row of the slice's first transition, valid rows): slot 0 is the pre-step row (zero but for the int32 [npairs, 2] (dst, src)
    column pairs `pre_pairs`), slots 1 .. n the ring rows with done 0 where timeout > 0, the rest zero.  The pass is `p`, or the int32
    device word `pass_word` when given.  See include/resel_hip.h `resel_gather_slices`."""
    _need_cuda('gather_slices', buffer, plan_dev, pre_pairs, *(() if pass_word is None else (pass_word,)))
    assert buffer.dtype == torch.float32 and buffer.dim() == 2 and buffer.is_contiguous()
    assert plan_dev.dtype == torch.int32 and plan_dev.dim() == 3 and plan_dev.shape[2] == 2 and plan_dev.is_contiguous()
    assert pre_pairs.dtype == torch.int32 and pre_pairs.dim() == 2 and pre_pairs.shape[1] == 2 and pre_pairs.is_contiguous()
    assert pass_word is None or (pass_word.dtype == torch.int32 and pass_word.numel() >= 1)
    W = buffer.shape[1]
    passes, batch = plan_dev.shape[:2]
    out = torch.empty(batch, int(length) + 1, W, dtype=torch.float32, device=buffer.device)
    check(lib().resel_gather_slices(_p(buffer), W, buffer.shape[0], _p(plan_dev), int(passes), int(batch), int(length), int(p), _p(pass_word),
                                    int(c_done), int(c_timeout), _p(pre_pairs), pre_pairs.shape[0], _p(out), _stream()), 'gather_slices')
    return out


@torch.no_grad()
def atb(wide, narrow, transposed=False):
    """wide [K, Wd] (column stride 1, Wd % 4 == 0), narrow [K, Nd <= 96] -> wide^T narrow [Wd, Nd] (or [Nd, Wd] if transposed):
    the long-reduction weight-gradient GEMMs of the narrow Mamba projections on a hand-written fp32 MFMA kernel."""
    _need_cuda('atb', wide, narrow)
    K, Wd = wide.shape
    Nd = narrow.shape[1]
    assert narrow.shape[0] == K and wide.stride(1) == 1 and narrow.stride(1) == 1
    out = torch.empty((Nd, Wd) if transposed else (Wd, Nd), dtype=torch.float32, device=wide.device)
    ws = _ws(lib().resel_atb_workspace_bytes(K, Wd, Nd), wide.device)
    check(lib().resel_atb(_p(wide), wide.stride(0), Wd, _p(narrow), narrow.stride(0), Nd, _p(out), int(bool(transposed)), _p(ws), K,
                          _stream()), 'atb')
    return out


# ---- products with one side at most 48 wide on the streaming fp32-MFMA kernels of csrc/skinny_gemm.hip -------------------------------
def narrow_on():
    """RESEL_NARROW (default on; read per call so that one process can run both routes): 0 = the GEMM / atb launches of before."""
    return os.environ.get('RESEL_NARROW', '1') != '0'


def _narrow_block(t, mult, align):
    """t [M, C]: unit column stride, row stride a multiple of `mult` floats, base aligned to `align` bytes."""
    return t.dim() == 2 and t.is_cuda and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % mult == 0 \
        and t.stride(0) >= t.shape[1] and t.data_ptr() % align == 0


def narrow_k_ok(a, w, out=None):
    """Shapes and layouts `resel_narrow_k` takes (include/resel_hip.h); everything else stays on `gemm_f32`."""
    K, N = a.shape[1], w.shape[0]
    return 4 <= K <= 48 and K % 4 == 0 and N % 4 == 0 and a.shape[0] > 0 and w.shape[1] == K and _narrow_block(a, 2, 8) \
        and _narrow_block(w, 2, 8) and (out is None or _narrow_block(out, 4, 16))


@torch.no_grad()
def narrow_k(a, w, bias=None, act=None, out=None, amax_out=None):
    """act(a [M, K <= 48] w[N, K]^T + bias) -> [M, N]; a may be a column block of a wider matrix, out (optional) one too.  act: None, 'elu'
    or GEMM_SOFTPLUS.  amax_out: (handle, pointer, epoch) as `_slot_args` returns it - the output is tagged with the handle."""
    _need_cuda('narrow_k', a, w)
    assert narrow_k_ok(a, w, out) and act != GEMM_ACCUMULATE
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    assert out.shape == (M, N)
    if bias is not None:
        bias = bias if (bias.dtype == torch.float32 and bias.is_contiguous()) else bias.float().contiguous()
        assert bias.numel() == N
    slot, slot_p, epoch = amax_out if amax_out is not None else (None, None, 0)
    check(lib().resel_narrow_k(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), M, N, K, GEMM_EPILOGUES[act],
                               slot_p, epoch, _stream()), 'narrow_k')
    return tag_amax(out, slot)


def narrow_n_pair_ok(g, w, x):
    """Shapes and layouts `resel_narrow_n_pair` takes: g [M, Wd <= 512], w [Wd, Nn <= 48] or None, x [M, Nn] or None."""
    M, Wd = g.shape
    ok = M > 0 and Wd % 4 == 0 and Wd <= 512 and _narrow_block(g, 4, 16)
    for t, rows in ((w, Wd), (x, M)):
        ok = ok and (t is None or (_narrow_block(t, 1, 4) and t.shape[0] == rows and 0 < t.shape[1] <= 48))
    return ok and (w is None or x is None or w.shape[1] == x.shape[1])


@torch.no_grad()
def narrow_n_pair(g, w=None, x=None, dx_out=None):
    """One pass over g [M, Wd]: (g w [M, Nn] if w is given - written to dx_out, e.g. a column block of a wider buffer, when that is
    given - , g^T x [Wd, Nn] if x is given); the output whose operand is missing is None."""
    _need_cuda('narrow_n_pair', g, w, x)
    assert (w is not None or x is not None) and narrow_n_pair_ok(g, w, x)
    M, Wd = g.shape
    Nn = (w if w is not None else x).shape[1]
    dx = dw = ws = None
    if w is not None:
        dx = dx_out if dx_out is not None else torch.empty(M, Nn, dtype=torch.float32, device=g.device)
        assert dx.shape == (M, Nn) and _narrow_block(dx, 1, 4)
    if x is not None:
        dw = torch.empty(Wd, Nn, dtype=torch.float32, device=g.device)
        ws = _ws(lib().resel_narrow_n_pair_workspace_bytes(M, Wd, Nn), g.device)
    check(lib().resel_narrow_n_pair(_p(g), g.stride(0), Wd, _p(w), 0 if w is None else w.stride(0), _p(x), 0 if x is None else x.stride(0), Nn,
                                    _p(dx), 0 if dx is None else dx.stride(0), _p(dw), _p(ws), M, _stream()), 'narrow_n_pair')
    return dx, dw


# ---------------------------------------------------------------------------------------------- bf16 projections (cgpt)
@torch.no_grad()
def gemm_bf16(A, B, a_kcontig=True, b_kcontig=True, bias=None, out_dtype=torch.bfloat16, round_out=False):
    """C [M, N] = bf16(A) (.) bf16(B) + bf16(bias), fp32 accumulation (include/resel_hip.h `resel_gemm_bf16`).  A: [M, K]
    (a_kcontig) or [K, M]; B: [N, K] (b_kcontig) or [K, N]; each fp32 or bf16 (rounded to bf16 on the way into LDS); bias fp32.
    round_out (fp32 output only): store the bf16-ROUNDED value as fp32 - what `F.linear(...).to(float32)` leaves under bf16 autocast."""
    _need_cuda('gemm_bf16', A, B)
    assert A.dim() == 2 and B.dim() == 2 and A.stride(-1) == 1 and B.stride(-1) == 1
    assert A.dtype in (torch.float32, torch.bfloat16) and B.dtype in (torch.float32, torch.bfloat16)
    M, K = (A.shape[0], A.shape[1]) if a_kcontig else (A.shape[1], A.shape[0])
    N = B.shape[0] if b_kcontig else B.shape[1]
    assert (B.shape[1] if b_kcontig else B.shape[0]) == K
    out = torch.empty((M, N), dtype=out_dtype, device=A.device)
    L = lib()
    ws = _ws(L.resel_gemm_bf16_workspace_bytes(M, N, K), A.device)
    check(L.resel_gemm_bf16(_p(A), A.stride(0), int(a_kcontig), int(A.dtype == torch.bfloat16), _p(B), B.stride(0), int(b_kcontig),
                            int(B.dtype == torch.bfloat16), _p(bias), _p(out), out.stride(0), 1 if out_dtype == torch.bfloat16 else (2 if round_out else 0), _p(ws),
                            M, N, K, _stream()), 'gemm_bf16')
    return out


def gemm_bf16_ok(x, w):
    """Operands the mixed-precision GEMM node takes: token rows on the GPU, fp32 master weight (any row count and alignment since round 6:
    `resel_gemm_bf16` routes what its matrix-core kernel cannot read, and the few rows of a decode step, to csrc/gemm_any.hip)."""
    return (x.is_cuda and x.dim() == 2 and x.stride(-1) == 1 and x.dtype in (torch.float32, torch.bfloat16) and w.dtype == torch.float32
            and w.is_contiguous())


@torch.no_grad()
def colsum_bf16(x):
    """x [M, N] bf16 -> column sums fp32 [N] (include/resel_hip.h `resel_colsum_bf16`); shapes the kernel does not take go to ATen."""
    M, N = x.shape
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.stride(1) == 1 and N % 8 == 0 and N <= 2048 and x.stride(0) % 8 == 0
            and x.data_ptr() % 16 == 0 and M >= 256):
        return torch.sum(x, 0, dtype=torch.float32)
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = _ws(lib().resel_colsum_bf16_workspace_bytes(M, N), x.device)
    check(lib().resel_colsum_bf16(_p(x), x.stride(0), M, N, _p(out), _p(ws), _stream()), 'colsum_bf16')
    return out


class LinearBf16(torch.autograd.Function):
    """F.linear under the reference's bf16 autocast (flash-attn MHA's Wqkv / out_proj, TransformerFlashAttention.py:67-70) as ONE
    node on `resel_gemm_bf16`: x fp32 or bf16, fp32 master weight and bias; forward output in `out_dtype`; the input gradient comes
    back in x's dtype, the weight / bias gradients in fp32 - the casts of the autocast graph (activation -> bf16, weight -> bf16 per
    call, gradients back to fp32) happen inside the GEMMs."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_dtype, round_out=False):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return gemm_bf16(x, weight, True, True, bias, out_dtype, round_out)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy if gy.stride(-1) == 1 and gy.stride(0) % 4 == 0 and gy.data_ptr() % 16 == 0 else gy.contiguous()
        dx = gemm_bf16(gy, weight, True, False, None, x.dtype) if ctx.needs_input_grad[0] else None
        dw = gemm_bf16(gy, x, False, False, None, torch.float32) if ctx.needs_input_grad[1] else None
        db = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            if gy.dtype == torch.float32 and gy.shape[1] % 4 == 0 and gy.shape[0] >= 256:
                db = bias_act_bwd(gy, gy, gy.shape[0], None, True)[1].reshape(-1)          # fp32 column sums (one read of gy, fixed order)
            else:
                db = colsum_bf16(gy)
        return dx, dw, db, None, None


def linear_bf16(x, weight, bias, out_dtype=torch.bfloat16, round_out=False):
    return LinearBf16.apply(x, weight, bias, out_dtype, round_out)


# product formation of resel_gemm_f32 (include/resel_hip.h): 0 fp32 MFMA; 9 / 6 exact three-way bf16 split on the bf16 MFMA; 2 fp16 planes
# of the scaled operands, three products (all of these fp32-accurate against fp64, tests/test_hip_ops.py); 3 two bf16 planes per operand
# ("bf16x3").  None (no RESEL_GEMM_SPLIT): follow torch.get_float32_matmul_precision() the way torch's own GEMMs do - 'highest' (torch's
# default, the reference's setting) = 2 where the operand magnitudes are at hand and 6 elsewhere, 'high' / 'medium' = 3.
GEMM_SPLIT = int(os.environ['RESEL_GEMM_SPLIT']) if os.environ.get('RESEL_GEMM_SPLIT') else None


def gemm_split():
    if GEMM_SPLIT is not None:
        return GEMM_SPLIT
    return 2 if torch.get_float32_matmul_precision() == 'highest' else 3


_GEMM_WS_BYTES = {}           # (M, N, K, batch) -> workspace bytes of resel_gemm_f32 (a pure function of the shape)


# ---- operand magnitudes for GEMM mode 2 (include/resel_hip.h "magnitude slots") ---------------------------------------------
# A tensor written by one of this library's kernels carries a HANDLE to max |x| on the device - `t._resel_amax = (handle, version)` -
# so that a later `gemm_f32` on it (or on a view of it: `_base`) needs no extra pass; handles are 8-byte slots of a per-device
# arena ({float bits | epoch}; never zeroed: every producer call takes a fresh epoch) or the float32 [1] result of `amax()`.
# Tags die with an in-place modification that torch sees (`_version`); this module's own in-place kernels re-tag or clear.
AMAX_SLOTS = 2048             # handles per device arena (1 KiB each: eight 8-byte words, 128 bytes apart)
AMAX_WORDS = 128              # int64 words per handle
AMAX_PREPASS_FRACTION = 0.16  # of the estimated GEMM time one may spend on reading an untagged operand (measured: profiles/r04_gemm.md)
_AMAX_ARENA = {}              # device -> [int64 tensor [AMAX_SLOTS], next index]
_AMAX_EPOCH = [0]
LAST_AMAX = None              # the side channel from a Function's forward to `apply_tagged` around its .apply: written by `publish_amax` only
LAST_SPLIT = [None]


def publish_amax(slot):
    """Called by a producer inside an `autograd.Function.forward` (outputs of `.apply` come back untagged): hand the magnitude handle of
    the output (or None) to the `apply_tagged` that wraps the `.apply`."""
    global LAST_AMAX
    LAST_AMAX = slot


def apply_tagged(fn, whole, *args):
    """fn(*args) with its output (the first one of several) tagged with the handle that a producer inside fn published through
    `publish_amax`, and with none if nothing inside published - never with what an earlier producer left behind.  whole: as `tag_amax`."""
    global LAST_AMAX
    LAST_AMAX = None
    out = fn(*args)
    tag_amax(out[0] if type(out) is tuple else out, LAST_AMAX, whole)
    LAST_AMAX = None
    return out


_AMAX_SERIAL = [0]            # handles handed out so far; every arena handle object carries the serial of its current tenant (`_resel_serial`)
AMAX_GENERATION = [0]         # bumped by `amax_maintenance` when the epoch counter starts over: captured updates hold epochs of the old generation
_EPOCH_RESET_AT = 0x60000000  # epochs are 31-bit device words; start over at an update boundary long before they run out
_STORES = None                # weak set of FlatParameterStores (their weight handles carry epochs too); filled by `register_store`


def register_store(store):
    global _STORES
    if _STORES is None:
        import weakref
        _STORES = weakref.WeakSet()
    _STORES.add(store)


def amax_slot(device):
    """A fresh (handle: int64 view [AMAX_WORDS], epoch) pair for a producer kernel."""
    _AMAX_SERIAL[0] += 1
    ar = _AMAX_ARENA.get(device)
    if ar is None:
        buf = torch.zeros(AMAX_SLOTS * AMAX_WORDS, dtype=torch.int64, device=device)
        ar = _AMAX_ARENA[device] = [buf, 0, list(buf.view(AMAX_SLOTS, AMAX_WORDS).unbind(0))]     # handle views made once (this sits on the launch path)
    if _AMAX_EPOCH[0] >= _EPOCH_RESET_AT and not torch.cuda.is_current_stream_capturing():
        # a long-lived user of this module that never reaches an update boundary (evaluation / inference loops, soak tools): start the
        # epochs over HERE, long before the 31-bit device word runs out, instead of failing after weeks of uptime.  Safe between two
        # producer calls: the reset synchronises the device first (see amax_maintenance), so no kernel with an old epoch is in flight.
        # Handles the caller still holds become void (`handle_alive` / `amax_of` see the changed tenant serial).
        amax_maintenance(force=True)
    if _AMAX_EPOCH[0] >= 0x7ffffff0:
        raise RuntimeError('RESeL-HIP: magnitude epochs exhausted inside one captured region')
    _AMAX_EPOCH[0] += 1
    i = ar[1]
    ar[1] = (i + 1) % AMAX_SLOTS
    h = ar[2][i]
    h._resel_serial = _AMAX_SERIAL[0]               # whoever kept this handle for its previous tenant sees the change (`handle_alive`)
    return h, _AMAX_EPOCH[0]


def amax_maintenance(force=False):
    """Call at an UPDATE BOUNDARY (the trainers do, eager and graphed).  Epochs are 31 bits on the device: long before they run out
    everything that carries one starts over together - arenas zeroed, every arena handle evicted (tags and kept handles become void),
    the weight handles of every FlatParameterStore dropped (re-published on next use), and `AMAX_GENERATION` bumped so that holders of
    captured updates (epochs baked into kernel nodes) drop their graphs.  Returns True when it reset."""
    if not force and _AMAX_EPOCH[0] < _EPOCH_RESET_AT:
        return False
    _AMAX_EPOCH[0] = 0
    AMAX_GENERATION[0] += 1
    PARAM_EPOCH[0] += 1
    for ar in _AMAX_ARENA.values():
        # every stream of the device must be idle before the words are zeroed: a producer still running on a side / target stream with an
        # old-generation epoch (>= 0x60000000) that published AFTER the zero would outrank every new small epoch in its slot, and readers
        # would scale with a stale magnitude.  Once per ~1.6e9 producer calls: the stall does not matter.
        torch.cuda.synchronize(ar[0].device)
        ar[0].zero_()
        for h in ar[2]:
            h._resel_serial = None
    for st in (list(_STORES) if _STORES is not None else []):
        st._amax = None
    return True


def amax_arena_zero(device):
    """Zero the arena of `device` on the launch stream: FIRST node of a captured update - a replay publishes into the slots and
    epochs baked into the graph, which must not inherit the previous replay's maxima."""
    ar = _AMAX_ARENA.get(device)
    if ar is not None:
        ar[0].zero_()


def keep_handles(*hs):
    """For `ctx`: (handle, tenant serial) pairs - saved tensors come back untagged, and between a layer's forward and its backward a
    deep model may hand out more handles than the arena holds, so a kept handle is only used while its slot still has the same tenant."""
    return tuple((h, getattr(h, '_resel_serial', None)) for h in hs)


def handle_alive(kept):
    """The handle of a `keep_handles` pair, or None once the arena has given its slot to another tensor."""
    h, serial = kept
    return h if h is not None and getattr(h, '_resel_serial', None) == serial else None


def live_handles(kept):
    return tuple(handle_alive(k) for k in kept)


def _taggable(t):
    """Tags live on activations and gradients - tensors that are written once and die with the update.  Parameters are NOT tagged:
    this library's optimizer and soft-update kernels rewrite them through the flat buffers without bumping `_version`, so a tag
    would outlive the values it describes (their magnitudes come from a pre-pass per call: a few KB)."""
    return not (isinstance(t, torch.nn.Parameter) or (t.is_leaf and t.requires_grad))


def tag_amax(t, handle, whole=False):
    """whole: t covers ALL of the tensor it is a view of (a reshape of a fresh output) - tag that base too, so that other views of it
    (the [M, C] form of a [B, L, C] activation) find the magnitude.  A tag = (handle, tensor version, tenant serial of the handle)."""
    if t is not None:
        ok = handle is not None and _taggable(t)
        serial = getattr(handle, '_resel_serial', None) if ok else None
        t._resel_amax = (handle, t._version, serial) if ok else None
        base = getattr(t, '_base', None)
        if whole and base is not None:
            base._resel_amax = (handle, base._version, serial) if (ok and _taggable(base)) else None
    return t


def amax_of(t):
    """Handle of a bound on max |t| if one is known (t itself or the tensor t is a view of), else None.  A tag is void once torch has
    seen an in-place write to its tensor, or once the arena has handed the handle's slot to another tensor."""
    for obj in (t, getattr(t, '_base', None)):
        if obj is not None:
            tg = getattr(obj, '_resel_amax', None)
            if tg is not None and tg[1] == obj._version and getattr(tg[0], '_resel_serial', None) == tg[2]:
                return tg[0]
    return None


# ---- verify mode: RESEL_AMAX_VERIFY=1 checks, in front of EVERY mode-2 product, that the handles it scales with really bound its
# operands (one extra pass per operand: slow, for tests and debugging).  Violations are collected in a device word block; the trainers
# read it at the end of each update (`amax_verify_raise`) - also after a replayed update, whose graph then contains the check kernels.
AMAX_VERIFY = os.environ.get('RESEL_AMAX_VERIFY', '0') == '1'
_VERIFY_ERR = {}              # device -> int32 [4] (resel_amax_check)
_VERIFY_CALLS = []            # ring of (tag, description) of the most recent checks
_VERIFY_TAG = [0]


class AmaxBoundError(RuntimeError):
    pass


@torch.no_grad()
def amax_check(x, handle, what=''):
    """Queue a device-side check `max |x| <= value(handle)` (x as in `amax`)."""
    assert x.dtype == torch.float32 and x.stride(-1) == 1 and x.dim() in (2, 3)
    err = _VERIFY_ERR.get(x.device)
    if err is None:
        err = _VERIFY_ERR[x.device] = torch.zeros(4, dtype=torch.int32, device=x.device)
    _VERIFY_TAG[0] += 1
    _VERIFY_CALLS.append((_VERIFY_TAG[0], f'{what} {tuple(x.shape)} strides {tuple(x.stride())}'))
    del _VERIFY_CALLS[:-4096]
    batch = x.shape[0] if x.dim() == 3 else 1
    check(lib().resel_amax_check(_p(x), x.stride(-2), x.stride(0) if x.dim() == 3 and batch > 1 else 0, x.shape[-2], x.shape[-1], batch,
                                 _p(handle), _p(err), _VERIFY_TAG[0], _stream()), 'amax_check')


def amax_verify_raise(device=None):
    """Synchronise and raise AmaxBoundError if any check since the last call found an operand above its handle's bound."""
    for dev, err in list(_VERIFY_ERR.items()):
        if device is not None:
            d = torch.device(device)
            if d.type != dev.type or (d.index is not None and d.index != dev.index):       # 'cuda' names every cuda device
                continue
        e = err.cpu()
        if int(e[0]) == 0:
            continue
        err.zero_()
        tag = int(e[2])
        what = dict(_VERIFY_CALLS).get(tag, '?')
        got = float(e[1:2].view(torch.float32)[0])
        bound = float(e[3:4].view(torch.float32)[0])
        raise AmaxBoundError(f'RESeL-HIP: GEMM mode 2 was given a magnitude handle BELOW its operand: max |x| = {got:.6g} > bound {bound:.6g} '
                             f'(first report: check #{tag}: {what}; {int(e[0])} reporting waves) - the fp16 planes would overflow to inf')


@torch.no_grad()
def amax(x):
    """max |x| of a GEMM operand (2-D, or 3-D with a leading batch axis; last axis contiguous and a multiple of 4) as a magnitude
    handle on the device: one HBM-bound pass, no host synchronisation (include/resel_hip.h `resel_amax`)."""
    _need_cuda('amax', x)
    assert x.dtype == torch.float32 and x.stride(-1) == 1 and x.dim() in (2, 3)
    out, epoch = amax_slot(x.device)
    batch = x.shape[0] if x.dim() == 3 else 1
    # stateless since ABI 7: pre-passes on different streams cannot disturb each other
    check(lib().resel_amax(_p(x), x.stride(-2), x.stride(0) if x.dim() == 3 and batch > 1 else 0, x.shape[-2], x.shape[-1], batch,
                           _p(out), epoch, None, _stream()), 'amax')
    return out


def amax_value(handle):
    """Host value of a magnitude handle (tests / tools: synchronises)."""
    w = handle.view(torch.int64).cpu()[::16][:8]
    ep = (w >> 32) & 0xffffffff
    lo = (w[ep == ep.max()] & 0xffffffff).to(torch.int32)
    return float(lo.view(torch.float32).max())


PARAM_EPOCH = [0]             # bumped by every kernel of this module that rewrites parameters in place (flat AdamW, soft update)


@torch.no_grad()
def amax_segments(flat, begin, length, handles):
    """One launch: max |.| of every segment flat[begin[g] : begin[g] + length[g]] into the g-th handle of `handles` (int64 [nseg * AMAX_WORDS])."""
    _need_cuda('amax_segments', flat, begin, length, handles)
    _AMAX_EPOCH[0] += 1
    check(lib().resel_amax_segments(_p(flat), _p(begin), _p(length), int(begin.numel()), _p(handles), _AMAX_EPOCH[0], _stream()), 'amax_segments')


def weight_amax(p):
    """Magnitude handle of a parameter held in a FlatParameterStore (models/flat_params.py keeps one handle per tensor, refreshed by ONE
    launch after the buffer was rewritten), or None (the caller's GEMM then decides about a pre-pass)."""
    ref = getattr(p, '_resel_store', None)
    if ref is None or not amax_tracking():
        return None
    return ref[0].amax_handle(ref[1], p)


def _slot_args(want, device):
    """(slot tensor or None, pointer, epoch) for a producer kernel's amax output."""
    if not want:
        return None, None, 0
    slot, epoch = amax_slot(device)
    return slot, _p(slot), epoch


def amax_tracking():
    """Producers publish magnitudes only while the GEMMs would use them (product mode 2)."""
    return gemm_split() == 2


def _operand_handles(A, B, amax_a, amax_b):
    """Magnitude handles of a product's operands as far as they are known without a pass: the caller's, a producer's tag, the
    parameter store's (None where none of them has one)."""
    ha = amax_a if amax_a is not None else amax_of(A)
    hb = amax_b if amax_b is not None else amax_of(B)
    return weight_amax(A) if ha is None else ha, weight_amax(B) if hb is None else hb


def _prepass(x):
    """One `amax` pass over an operand nobody has a handle for; tagged for reuse."""
    h = amax(x)
    tag_amax(x, h)
    return h


def _mode2_shape(M, K):
    """False for the shapes the library never runs in product mode 2 (it takes mode 6 for M <= 128 and the fp32 instruction for K < 32):
    no pre-pass is spent on them.  `gemm_route` in csrc/gemm_f32.hip is the authority; this mirrors its two shape rules and nothing else."""
    return K >= 32 and M > 128


def _gemm_operands(A, B, a_kcontig, b_kcontig):
    """The one reading of a product's operands (layouts as `gemm_f32` describes them) -> batch, M, N, K, multi, and the argument block every
    fp32 GEMM entry starts with: (pointer, row stride, batch stride, kcontig) of A and of B.  (Outputs and side operands with the product's
    shape follow in the same form, (pointer, row stride, batch stride if multi else 0), written out at the call: a helper call is 0.5 us.)"""
    sa_, sb_, ta, tb = A.shape, B.shape, A.stride(), B.stride()       # one call each: this runs 80 times per update
    assert ta[-1] == 1 and tb[-1] == 1 and A.dtype == torch.float32 and B.dtype == torch.float32
    batched = len(sa_) == 3
    batch = sa_[0] if batched else 1
    M, K = (sa_[-2], sa_[-1]) if a_kcontig else (sa_[-1], sa_[-2])
    N = sb_[-2] if b_kcontig else sb_[-1]
    assert (sb_[-1] if b_kcontig else sb_[-2]) == K and (not batched or sb_[0] == batch)
    multi = batch > 1
    return batch, M, N, K, multi, (_p(A), ta[-2], ta[0] if multi else 0, int(a_kcontig), _p(B), tb[-2], tb[0] if multi else 0, int(b_kcontig))


def _gemm_run(fn, name, A, B, args, M, N, K, batch, split, ha, hb, out, track=True, amax_out=None, publish=False):
    """The shared tail of the three GEMM forms.  `args`: everything in front of the handles; ha / hb: the operands' magnitude handles in product
    mode 2, else None.  The output gets a magnitude slot - max |C| for whoever multiplies C next - while mode 2 is the product mode and it is worth
    a pass (`track`; amax_out: (handle, pointer, epoch) of a row buffer this product fills a column block of - its producers share one handle)."""
    GEMM_FLOPS[0] += 2.0 * M * N * K * batch
    if AMAX_VERIFY and ha is not None:
        what = f'{name.replace("_f32", "", 1)} M={M} N={N} K={K} batch={batch}'
        amax_check(A, ha, 'A of ' + what)
        amax_check(B, hb, 'B of ' + what)
    slot, slot_p, epoch = amax_out if amax_out is not None else _slot_args(M * N * batch >= (1 << 20) and track and amax_tracking(), A.device)
    check(fn(*args, _p(ha), _p(hb), slot_p, epoch, _stream()), name)
    if publish:
        publish_amax(slot)                           # for `linear_act` / `EnsembleLinear.forward`, which run this product inside a Function
    LAST_SPLIT[0] = split                            # tools/gemm_census.py: which product mode the call took
    return tag_amax(out, slot)


@torch.no_grad()
def gemm_f32(A, B, a_kcontig=True, b_kcontig=True, bias=None, act=None, out=None, split=None, amax_a=None, amax_b=None, amax_out=None):
    """C[b] = act(A[b] (.) B[b] + bias[b]) on the matrix cores, fp32 in / out (include/resel_hip.h `resel_gemm_f32`).
    A: [M, K] (a_kcontig) or [K, M]; B: [N, K] (b_kcontig) or [K, N]; optionally a leading batch (ensemble) dimension on all of
    A, B, bias [N] / [batch, N], out.  Row stride free (column stride 1); returns C [M, N] / [batch, M, N].
    (The wrapper is on the host's critical path at small batches: 79 calls per update - no temporary views, cached sizes.)"""
    _need_cuda('gemm_f32', A, B)
    batch, M, N, K, multi, operands = _gemm_operands(A, B, a_kcontig, b_kcontig)
    batched = A.dim() == 3
    if out is None:
        out = torch.empty((batch, M, N) if batched else (M, N), dtype=torch.float32, device=A.device)
    assert out.stride(-1) == 1
    L = lib()
    key = (M, N, K, batch)
    nb = _GEMM_WS_BYTES.get(key)
    if nb is None:
        nb = _GEMM_WS_BYTES[key] = L.resel_gemm_f32_workspace_bytes(M, N, K, batch)
    ws = _ws(nb, A.device) if nb else None
    bs = 0
    if bias is not None:
        if bias.dim() != (2 if batched else 1):          # [N] / [batch, N] as they are: a reshape is a view, and a view is 3 us of host time
            bias = bias.reshape(batch, N) if batched else bias.reshape(N)
        assert bias.shape[-1] == N and (not batched or bias.shape[0] == batch)
        bs = bias.stride(0) if batched else 0
    split = gemm_split() if split is None else int(split)
    ha = hb = None
    if split == 2:
        # mode 2 (fp16 planes of the scaled operands) needs a bound on max |A|, max |B| on the device: a producer's tag, the
        # caller's handle, or - when reading the operand once more is cheap next to the GEMM - one resel_amax pass (tagged for reuse)
        if not _mode2_shape(M, K):
            split = 6
        else:
            ha, hb = _operand_handles(A, B, amax_a, amax_b)
            if ha is None or hb is None:
                t_gemm = 2.0 * M * N * K * batch / 1.5e8                       # us at 150 TFLOP/s
                cost = (0.0 if ha is not None else 4.0 * M * K * batch / 4.5e6 + 2.5) + (0.0 if hb is not None else 4.0 * N * K * batch / 4.5e6 + 2.5)
                if cost <= AMAX_PREPASS_FRACTION * t_gemm:
                    ha = _prepass(A) if ha is None else ha
                    hb = _prepass(B) if hb is None else hb
                else:
                    split, ha, hb = 6, None, None
    return _gemm_run(L.resel_gemm_f32x, 'gemm_f32', A, B, operands + (_p(bias), bs, GEMM_EPILOGUES[act], _p(out), out.stride(-2), out.stride(0) if multi else 0, _p(ws), M, N, K, batch, split),
                     M, N, K, batch, split, ha, hb, out, act != GEMM_ACCUMULATE, amax_out, True)


# ---- fused epilogues of the producer / consumer GEMM (include/resel_hip.h `resel_gemm_f32_dact` / `resel_gemm_f32_head`) ----------
def _forced_handles(A, B, amax_a, amax_b):
    """Magnitude handles of both operands for a product that exists in mode 2 only: the caller's, a producer's tag, the parameter
    store's - or one pre-pass (tagged for reuse)."""
    ha, hb = _operand_handles(A, B, amax_a, amax_b)
    return _prepass(A) if ha is None else ha, _prepass(B) if hb is None else hb


def gemm_fused_ok(kind, M, N, K, *mats):
    """True when a fused-epilogue form (kind 4: dact, 5: head) may take a product of this shape: product mode 2, the
    producer / consumer edition's shape rules (K a multiple of 32, M > 128; dact: N a multiple of 128), 16-byte aligned rows."""
    if os.environ.get('RESEL_GEMM_FUSED', '1') == '0' or gemm_split() != 2 or not gemm_f32_ok(*mats) or not rows_aligned16(*mats):
        return False
    ld = max(int(t.stride(-2)) for t in mats)
    return bool(lib().resel_gemm_f32_fused_supported(int(kind), int(M), int(N), int(K), ld, ld))


@torch.no_grad()
def gemm_f32_dact(A, B, b_kcontig, Y, out, need_dbias=True, amax_a=None, amax_b=None):
    """out[b] = (A[b] (.) B[b]) * elu'(Y[b]) with elu' taken from the ELU OUTPUT Y (y > 0 ? 1 : y + 1), and dbias[b][n] = column sums of
    out[b]: the input gradient of a layer whose input was the ELU output of the layer below, with that ELU's backward and that layer's
    bias gradient in the GEMM epilogue.  A [batch, M, K] / [M, K] (K contiguous); B [batch, N, K] (b_kcontig) or [batch, K, N]; Y and out
    [batch, M, N] with free row / batch strides.  -> (out, dbias [batch, N] or None)."""
    _need_cuda('gemm_f32_dact', A, B, Y, out)
    batch, M, N, K, multi, operands = _gemm_operands(A, B, True, b_kcontig)
    assert Y.shape[-2:] == (M, N) and out.shape[-2:] == (M, N) and Y.stride(-1) == 1 and out.stride(-1) == 1
    ha, hb = _forced_handles(A, B, amax_a, amax_b)
    L = lib()
    ws = _ws(L.resel_gemm_f32_fused_workspace_bytes(M, N, K, batch, 4), A.device)
    dbias = torch.empty(batch, N, dtype=torch.float32, device=A.device) if need_dbias else None
    args = operands + (_p(Y), Y.stride(-2), Y.stride(0) if multi else 0, _p(out), out.stride(-2), out.stride(0) if multi else 0, _p(dbias), _p(ws), M, N, K, batch)
    return _gemm_run(L.resel_gemm_f32_dact, 'gemm_f32_dact', A, B, args, M, N, K, batch, 2, ha, hb, out), dbias


@torch.no_grad()
def gemm_f32_head(A, B, b_kcontig, bias, w3, b3, amax_a=None, amax_b=None):
    """a[b] = elu(A[b] (.) B[b] + bias[b]) and q[b][m] = sum_n a[b][m][n] w3[b][n] + b3[b]: the hidden layer and the width-1 output layer of
    an efc-E critic head in one GEMM.  A [batch, M, K]; B [batch, N, K] / [batch, K, N]; bias, w3 [batch, N]; b3 [batch] or None.
    -> (a [batch, M, N], q [batch, M])."""
    _need_cuda('gemm_f32_head', A, B, bias, w3)
    batch, M, N, K, multi, operands = _gemm_operands(A, B, True, b_kcontig)
    assert A.dim() == 3 and w3.shape == (batch, N) and w3.is_contiguous() and bias.shape == (batch, N) and bias.stride(-1) == 1
    ha, hb = _forced_handles(A, B, amax_a, amax_b)
    L = lib()
    ws = _ws(L.resel_gemm_f32_fused_workspace_bytes(M, N, K, batch, 5), A.device)
    a = torch.empty(batch, M, N, dtype=torch.float32, device=A.device)
    q = torch.empty(batch, M, dtype=torch.float32, device=A.device)
    args = operands + (_p(bias), bias.stride(0) if multi else 0, _p(w3), N, _p(b3), _p(a), a.stride(-2), a.stride(0) if multi else 0, _p(q), _p(ws), M, N, K, batch)
    return _gemm_run(L.resel_gemm_f32_head, 'gemm_f32_head', A, B, args, M, N, K, batch, 2, ha, hb, a), q


# ---- one-token rollout step (T = 1, no autograd) ----------------------------------------------------------------------
@torch.no_grad()
def conv_step(x, window, weight, bias, d_conv, layout, act):
    """Depthwise conv on one token with a rolling window.  x [B, Di] (row-strided view), window [B, *] rows holding
    layout 'dk': [Di, K] per row (smamba) or 'kd': time-major [K - 1, Di] (s6 mamba / conv1d).  -> (xc [B, Di], new window)."""
    _need_cuda('conv_step', x, window)
    B, Di, K = x.shape[0], x.shape[1], d_conv
    W, sd, sk = (K, K, 1) if layout == 'dk' else (K - 1, 1, Di)
    assert window.shape == (B, Di * W) and window.stride(1) == 1 and x.stride(1) == 1
    new = torch.empty((B, Di * W), dtype=torch.float32, device=x.device)
    xc = torch.empty((B, Di), dtype=torch.float32, device=x.device)
    check(lib().resel_mamba_conv_step(_p(x), x.stride(0), _p(window), window.stride(0), _p(new), new.stride(0), sd, sk, W,
                                      _p(weight), _p(bias), _p(xc), B, Di, K, int(bool(act)), _stream()), 'mamba_conv_step')
    return xc, new


@torch.no_grad()
def selective_state_update(state, xc, x_db, dt_w, dt_b, A_log, D, z=None):
    """state [B, Di*N] (row-strided view), xc [B, Di], x_db [B, R + 2N] = (dt low-rank | B | C), z [B, Di] view or None.
    -> (y [B, Di], new state [B, Di*N])   (reference selective_state_update.py:123-154 with dt_proj folded in)."""
    _need_cuda('selective_state_update', state, xc, x_db)
    B, Di = xc.shape
    R = dt_w.shape[1]
    N = (x_db.shape[1] - R) // 2
    assert state.shape == (B, Di * N) and state.stride(1) == 1 and x_db.stride(1) == 1 and xc.is_contiguous()
    new = torch.empty((B, Di * N), dtype=torch.float32, device=xc.device)
    y = torch.empty_like(xc)
    check(lib().resel_selective_state_update(_p(state), state.stride(0), _p(new), new.stride(0), _p(xc), _p(x_db), x_db.stride(0),
                                             _p(dt_w), _p(dt_b), _p(A_log), _p(D), _p(z), 0 if z is None else z.stride(0), _p(y),
                                             B, Di, N, R, _stream()), 'selective_state_update')
    return y, new


@torch.no_grad()
def mamba_step(hidden, xz, conv_w, conv_b, xproj_w, dt_w, dt_b, A_log, D, d_conv, d_state):
    """smamba mixer state update for one token (reference smamba/mamba.py:257-305).
    hidden [B, Di*K + Di*N] = (conv window | ssm state), xz [B, 2 Di] = in_proj output.  -> (y [B, Di], new hidden)."""
    Di, K = xz.shape[1] // 2, d_conv
    xc, window = conv_step(xz[:, :Di], hidden[:, :Di * K], conv_w, conv_b, K, 'dk', True)
    x_db = gemm_f32(xc, xproj_w, True, True)                                         # [B, R + 2N]: the rows form of resel_gemm_f32x
    y, state = selective_state_update(hidden[:, Di * K:], xc, x_db, dt_w, dt_b, A_log, D, xz[:, Di:])
    return y, torch.cat((window, state), dim=-1)


@torch.no_grad()
def attn_decode(qkv, kv_cache, pos, slopes, scale):
    """Append this token's k, v to kv_cache [Bmax, S, 2, H, hd] (bf16, in place) and attend over positions 0..pos.
    qkv [B, 3, H, hd] bf16; pos: host int, or an int32 device tensor (graph replay) - of one element: the position of all rows; of
    B > 1 elements: one position per row (rows at different points of their episodes, `resel_attn_decode_rows`).  -> [B, H, hd] bf16.
    The cache is held at the kernel width hdp = attn_head_pad(hd): [Bmax, S, 2, H, hdp], its columns [hd, hdp) zero; qkv is padded to it
    and the result unpadded.  `scale` is that of the true width hd."""
    _need_cuda('attn_decode', qkv, kv_cache)
    B, _, H, hd_true = qkv.shape
    hd = attn_head_pad(hd_true)
    assert qkv.dtype == torch.bfloat16 and kv_cache.dtype == torch.bfloat16 and qkv.is_contiguous() and kv_cache.is_contiguous()
    assert kv_cache.shape[0] >= B and kv_cache.shape[2:] == (2, H, hd), 'the KV cache is [Bmax, S, 2, H, attn_head_pad(hd)]'
    if hd != hd_true:
        out = _attn_decode_run(_head_pad(qkv, hd), kv_cache, pos, slopes, scale)
        return _head_unpad(out.view(B, 1, H, hd), hd_true).view(B, H, hd_true)
    return _attn_decode_run(qkv, kv_cache, pos, slopes, scale)


def _attn_decode_run(qkv, kv_cache, pos, slopes, scale):
    B, _, H, hd = qkv.shape
    out = torch.empty((B, H, hd), dtype=torch.bfloat16, device=qkv.device)
    dev = pos if torch.is_tensor(pos) else None
    if dev is not None and dev.numel() > 1:
        assert dev.dtype == torch.int32 and dev.is_cuda and dev.is_contiguous() and dev.numel() == B, 'one int32 position per row'
        check(lib().resel_attn_decode_rows(_p(qkv), 3 * H * hd, _p(kv_cache), _p(dev), _p(slopes), _p(out), float(scale), B, H, hd,
                                           kv_cache.shape[1], _stream()), 'attn_decode_rows')
        return out
    check(lib().resel_attn_decode(_p(qkv), 3 * H * hd, _p(kv_cache), _p(dev), 0 if dev is not None else int(pos), _p(slopes), _p(out),
                                  float(scale), B, H, hd, kv_cache.shape[1], _stream()), 'attn_decode')
    return out


@torch.no_grad()
def step_state_reset(flags, tensors, counters):
    """Episode start for some rows of a B-row step: for every row b with flags[b] != 0, zeros over row b of every tensor in `tensors`
    and 0 to c[b] of every int32 [B] array in `counters`; other rows untouched.  flags int32 [B] on the device.  A tensor is fp32 with
    shape [B, W] or [1, B, W], unit stride along W and any row stride >= W (a column view of wider rows is fine).  One launch per 16
    tensors / 8 counters, nothing else on the stream, no allocation: capturable."""
    from ._lib import RESET_MAX_COUNTERS, RESET_MAX_SEGS, ResetCounters, ResetSegs
    _need_cuda('step_state_reset', flags, *tensors, *counters)
    assert flags.dtype == torch.int32 and flags.dim() == 1 and flags.is_contiguous()
    B = flags.numel()
    segs = []
    for t in tensors:
        assert t.dtype == torch.float32 and t.dim() >= 2 and t.shape[-2] == B and t.numel() == B * t.shape[-1], 'state rows are [B, W] fp32'
        W = t.shape[-1]
        assert W > 0 and (t.stride(-1) == 1 or W == 1) and (t.stride(-2) >= W or B == 1), 'unit stride along a row, rows do not overlap'
        segs.append((t.data_ptr(), max(t.stride(-2), W), W))
    for c in counters:
        assert c.dtype == torch.int32 and c.is_contiguous() and c.numel() == B, 'one int32 position per row'
    counters = [c.data_ptr() for c in counters]
    L, s0, c0 = lib(), 0, 0
    while s0 < len(segs) or c0 < len(counters):
        st, ct = ResetSegs(), ResetCounters()
        part, cpart = segs[s0:s0 + RESET_MAX_SEGS], counters[c0:c0 + RESET_MAX_COUNTERS]
        for i, (base, stride, width) in enumerate(part):
            st.seg[i].base, st.seg[i].row_stride, st.seg[i].width = base, stride, width
        for i, ptr in enumerate(cpart):
            ct.pos[i] = ptr
        check(L.resel_step_state_reset(_p(flags), B, st, len(part), ct, len(cpart), _stream()), 'step_state_reset')
        s0, c0 = s0 + len(part), c0 + len(cpart)


@torch.no_grad()
def categorical_step(logits, u, floor=0.01, out=None):
    """Categorical head of one policy step (reference contextual_sac_discrete_policy.py:106-121) as one launch: per row of logits [M, A]
    p = renormalised twice (softmax + floor), logp = log p, mode = lowest argmax of p, sample = the first k with u < p_0 + ... + p_k.
    u [M]: one uniform draw in [0, 1) per row.  out: an fp32 block [M, 2 + A] with unit column stride that receives
    (mode | sample | logp[A]) - the output block of a graphed step; None: logp is a dense [M, A].
    -> (mode [M], sample [M], logp [M, A]); the indices are fp32 (views of `out` when it is given).  Nothing else on the stream, no
    host read, no device assert: capturable, and a NaN row shows up as NaN log-probabilities."""
    _need_cuda('categorical_step', logits, u, out)
    assert logits.dim() == 2 and logits.dtype == torch.float32 and u.dtype == torch.float32
    M, A = logits.shape
    if logits.stride(1) != 1 and A > 1:
        logits = logits.contiguous()
    u = u.reshape(-1).contiguous()
    assert u.numel() == M, 'one uniform draw per row'
    if out is None:
        logp = torch.empty((M, A), dtype=torch.float32, device=logits.device)
        idx = torch.empty((M, 2), dtype=torch.float32, device=logits.device)
        mode, sample = idx[:, 0], idx[:, 1]
    else:
        assert out.dtype == torch.float32 and out.shape == (M, 2 + A) and out.stride(1) == 1 and (M <= 1 or out.stride(0) >= 2 + A)
        mode, sample, logp = out[:, 0], out[:, 1], out[:, 2:]
    if M == 0:                                           # empty tensors have no address to hand over
        return mode, sample, logp
    check(lib().resel_categorical_step(_p(logits), max(logits.stride(0), A), _p(u), float(floor), _p(logp), max(logp.stride(0), A),
                                       _p(mode), _p(sample), max(mode.stride(0), 1), M, A, _stream()), 'categorical_step')
    return mode, sample, logp


# ---- environment steps inside the graphed policy step (csrc/env_step.hip): what the entries of every environment check alike ----------
def _env_rows(what, B, A, action, action_width, ret_acc, in_block, obs=2):
    """The blocks every entry takes: action fp32 [B] (action_width 1) or [B, action_width], unit column stride, any row stride; ret_acc
    fp64 [B]; in_block fp32 [B, >= 2 * obs + A + 1], unit column stride (obs: the width of an observation, A: of lst_action).
    -> (ld_action, ld_in)."""
    width = 2 * obs + A + 1
    assert action.dtype == torch.float32 and (action.shape == (B,) if action_width == 1 else
                                              action.shape == (B, action_width) and action.stride(1) == 1), f'{what}: the action view'
    assert ret_acc.dtype == torch.float64 and ret_acc.is_contiguous() and ret_acc.numel() == B
    assert in_block.dtype == torch.float32 and in_block.dim() == 2 and in_block.shape[0] == B and in_block.shape[1] >= width
    assert (in_block.stride(1) == 1) and (B <= 1 or in_block.stride(0) >= in_block.shape[1]), 'unit stride along a row, rows do not overlap'
    return max(action.stride(0), action_width), max(in_block.stride(0), width)


def _env_eval_tables(B, flags, n_episodes, ep_ret, ep_len):
    """The tables of an evaluation: flags / n_episodes int32 [B], ep_ret fp64 / ep_len int32 [B, J], all contiguous.  -> J."""
    assert flags.dtype == torch.int32 and flags.dim() == 1 and flags.is_contiguous() and flags.numel() == B
    assert n_episodes.dtype == torch.int32 and n_episodes.is_contiguous() and n_episodes.numel() == B
    assert ep_ret.dtype == torch.float64 and ep_len.dtype == torch.int32 and ep_ret.dim() == 2 and ep_ret.shape == ep_len.shape
    assert ep_ret.shape[0] == B and ep_ret.is_contiguous() and ep_len.is_contiguous()
    return ep_ret.shape[1]


def _env_episode_block(B, traj):
    """The episode block of a rollout, fp32 [B, T_cap, width] with unit column stride.  -> (T_cap, ld_row)."""
    assert traj.dtype == torch.float32 and traj.dim() == 3 and traj.shape[0] == B and traj.shape[1] >= 1 and traj.shape[2] >= 1
    T_cap, ld_row = traj.shape[1], traj.stride(1) if traj.shape[1] > 1 else max(traj.stride(1), traj.shape[2])
    assert traj.stride(2) == 1 and ld_row >= traj.shape[2] and (B <= 1 or traj.stride(0) == T_cap * ld_row), 'rows of one episode block'
    return T_cap, ld_row


def _collect_layout(what, name2range, widths, ring_width):
    """`MemoryArray.name2range` -> the `CollectLayout`: first columns, -1 for an empty range.  widths: of the fields not one column wide."""
    from ._lib import COLLECT_FIELDS, CollectLayout
    lay = CollectLayout()
    for name in COLLECT_FIELDS:
        a, b = name2range[name]
        if b > a:
            assert b - a == widths.get(name, 1) and a >= 0, f'{what}: field {name} is {b - a} wide in the ring'
            assert b <= ring_width, f'{what}: field {name} ends at column {b} of {ring_width}'
        setattr(lay, name, a if b > a else -1)
    return lay


def _tmaze_cfg(cfg: dict, B, env_state):
    """`TMaze.device_config()` -> the entries' cfg struct, behind the check of the environment's state block."""
    from ._lib import TMAZE_STATE_WORDS, TMazeCfg
    assert env_state.dtype == torch.int32 and env_state.is_contiguous() and env_state.shape == (B, TMAZE_STATE_WORDS)
    return TMazeCfg(int(cfg['corridor_length']), int(cfg['oracle_length']), int(cfg['episode_length']), float(cfg['goal_reward']),
                    float(cfg['penalty']), float(cfg['distract_reward']))


def _wind_cfg(cfg: dict, B, env_pos, env_words):
    """`Wind.device_config()` -> the entries' cfg struct, behind the check of the environment's two state blocks."""
    from ._lib import WIND_CFG_DOUBLES, WIND_STATE_DOUBLES, WIND_STATE_WORDS, WindCfg
    assert env_pos.dtype == torch.float64 and env_pos.is_contiguous() and env_pos.shape == (B, WIND_STATE_DOUBLES)
    assert env_words.dtype == torch.int32 and env_words.is_contiguous() and env_words.shape == (B, WIND_STATE_WORDS)
    return WindCfg(int(cfg['episode_length']), *[float(cfg[name]) for name in WIND_CFG_DOUBLES])


@torch.no_grad()
def tmaze_step(cfg: dict, init: bool, action, goals, n_episodes, env_state, ret_acc, ep_ret, ep_len, in_block, flags):
    """One T-Maze environment step (or, init: the start of an evaluation) for the B rows of a graphed policy step, as one launch:
    include/resel_hip.h `resel_tmaze_step`, host twin env_utils/tmaze.py.  cfg: `TMaze.device_config()`.
    action: fp32 [B] view, any stride - the action indices (column 0 of the categorical step's output block);
    goals int32 [B, J], n_episodes int32 [B] (each at most J), env_state int32 [B, 8], ret_acc fp64 [B], ep_ret fp64 / ep_len int32 [B, J];
    in_block fp32 [B, >= 9] with unit column stride (state[2] | lst_state[2] | lst_action[4] | reward[1]), flags int32 [B].
    Everything is updated in place; nothing else on the stream, no host read, no allocation: capturable."""
    _need_cuda('tmaze_step', action, goals, n_episodes, env_state, ret_acc, ep_ret, ep_len, in_block, flags)
    B, A = flags.numel(), 4
    ld_action, ld_in = _env_rows('tmaze_step', B, A, action, 1, ret_acc, in_block)
    J = _env_eval_tables(B, flags, n_episodes, ep_ret, ep_len)
    assert goals.dtype == torch.int32 and goals.shape == (B, J) and (goals.stride(1) == 1 or J == 1)
    c = _tmaze_cfg(cfg, B, env_state)
    if B == 0:                                           # empty tensors have no address to hand over
        return
    check(lib().resel_tmaze_step(c, int(bool(init)), _p(action), ld_action, _p(goals), max(goals.stride(0), J), _p(n_episodes), J,
                                 _p(env_state), _p(ret_acc), _p(ep_ret), _p(ep_len), J, _p(in_block), ld_in, A, _p(flags), B, _stream()), 'tmaze_step')


@torch.no_grad()
def tmaze_collect_step(cfg: dict, name2range: dict, init: bool, action, goal, env_state, ret_acc, traj, max_episode_steps: int, in_block):
    """One iteration of the training rollout on a discrete T-Maze (or, init: `env_reset()` with the goal sides in `goal`) for the B rows of a
    graphed policy step, as one launch: include/resel_hip.h `resel_tmaze_collect_step`, host twin `SAC._train_loop` / `_push` / `env_step`.
    cfg: `TMaze.device_config()`.  name2range: `MemoryArray.name2range`, field -> (first column, end); an empty range is a field the ring does
    not store, and a stored field must have the width the rollout produces (observations 2, last action 4, scalars 1; no log-probability).
    action: fp32 [B] view, any stride - the SAMPLED indices (column 1 of the categorical step's output block); goal int32 [B];
    env_state int32 [B, 8], ret_acc fp64 [B]; traj fp32 [B, T_cap, >= the layout's width] with unit column stride: the episode block;
    in_block fp32 [B, >= 9] with unit column stride.  Everything is updated in place; no host read, no allocation: capturable."""
    _need_cuda('tmaze_collect_step', action, goal, env_state, ret_acc, traj, in_block)
    B, A = goal.numel(), 4
    assert goal.dtype == torch.int32 and goal.dim() == 1 and goal.is_contiguous()
    ld_action, ld_in = _env_rows('tmaze_collect_step', B, A, action, 1, ret_acc, in_block)
    c = _tmaze_cfg(cfg, B, env_state)
    T_cap, ld_row = _env_episode_block(B, traj)
    lay = _collect_layout('tmaze_collect_step', name2range, dict(state=2, last_state=2, next_state=2, last_action=A, logp=0), traj.shape[2])
    if B == 0:                                           # empty tensors have no address to hand over
        return
    check(lib().resel_tmaze_collect_step(c, lay, int(bool(init)), _p(action), ld_action, _p(goal), _p(env_state), _p(ret_acc), _p(traj), T_cap,
                                         ld_row, int(max_episode_steps), _p(in_block), ld_in, A, B, _stream()), 'tmaze_collect_step')


@torch.no_grad()
def wind_step(cfg: dict, init: bool, action, winds, n_episodes, env_pos, env_words, ret_acc, ep_ret, ep_len, in_block, flags):
    """One Wind-v0 environment step (or, init: the start of an evaluation) for the B rows of a graphed policy step, as one launch:
    include/resel_hip.h `resel_wind_step`, host twin env_utils/wind.py.  cfg: `Wind.device_config()`.
    action: fp32 [B, 2] view, any row stride - the action means (columns 0:2 of the Gaussian head's output block);
    winds fp64 [B, J, 2], n_episodes int32 [B] (each at most J), env_pos fp64 [B, 6], env_words int32 [B, 4], ret_acc fp64 [B],
    ep_ret fp64 / ep_len int32 [B, J]; in_block fp32 [B, >= 7] with unit column stride (state[2] | lst_state[2] | lst_action[2] | reward[1]),
    flags int32 [B].  Everything is updated in place; nothing else on the stream, no host read, no allocation: capturable."""
    _need_cuda('wind_step', action, winds, n_episodes, env_pos, env_words, ret_acc, ep_ret, ep_len, in_block, flags)
    B, A = flags.numel(), 2
    ld_action, ld_in = _env_rows('wind_step', B, A, action, A, ret_acc, in_block)
    J = _env_eval_tables(B, flags, n_episodes, ep_ret, ep_len)
    assert winds.dtype == torch.float64 and winds.shape == (B, J, 2) and winds.is_contiguous()
    c = _wind_cfg(cfg, B, env_pos, env_words)
    if B == 0:                                           # empty tensors have no address to hand over
        return
    check(lib().resel_wind_step(c, int(bool(init)), _p(action), ld_action, _p(winds), 2 * J, _p(n_episodes), J, _p(env_pos), _p(env_words),
                                _p(ret_acc), _p(ep_ret), _p(ep_len), J, _p(in_block), ld_in, A, _p(flags), B, _stream()), 'wind_step')


@torch.no_grad()
def wind_collect_step(cfg: dict, name2range: dict, init: bool, action, wind, env_pos, env_words, ret_acc, traj, max_episode_steps: int, in_block):
    """One iteration of the training rollout on Wind-v0 (or, init: `env_reset()` with the winds in `wind`) for the B rows of a graphed policy
    step, as one launch: include/resel_hip.h `resel_wind_collect_step`, host twin `SAC._train_loop` / `_push` / `env_step`.
    cfg: `Wind.device_config()`.  name2range: `MemoryArray.name2range`; a stored field must have the width the rollout produces
    (observations, last action and action 2, scalars 1; no log-probability).  action: fp32 [B, 2] view, any row stride - the SAMPLED actions
    (columns 2:4 of the Gaussian head's output block); wind fp64 [B, 2]; env_pos fp64 [B, 6], env_words int32 [B, 4], ret_acc fp64 [B];
    traj fp32 [B, T_cap, >= the layout's width] with unit column stride: the episode block; in_block fp32 [B, >= 7] with unit column stride.
    Everything is updated in place; no host read, no allocation: capturable."""
    _need_cuda('wind_collect_step', action, wind, env_pos, env_words, ret_acc, traj, in_block)
    assert wind.dtype == torch.float64 and wind.dim() == 2 and wind.shape[1] == 2 and wind.is_contiguous()
    B, A = wind.shape[0], 2
    ld_action, ld_in = _env_rows('wind_collect_step', B, A, action, A, ret_acc, in_block)
    c = _wind_cfg(cfg, B, env_pos, env_words)
    T_cap, ld_row = _env_episode_block(B, traj)
    widths = dict(state=2, last_state=2, next_state=2, last_action=A, action=A, logp=0)
    lay = _collect_layout('wind_collect_step', name2range, widths, traj.shape[2])
    if B == 0:                                           # empty tensors have no address to hand over
        return
    check(lib().resel_wind_collect_step(c, lay, int(bool(init)), _p(action), ld_action, _p(wind), _p(env_pos), _p(env_words), _p(ret_acc),
                                        _p(traj), T_cap, ld_row, int(max_episode_steps), _p(in_block), ld_in, A, B, _stream()), 'wind_collect_step')


def _catch_cfg(cfg: dict, B, env_state):
    """`Catch.device_config()` -> the entries' cfg struct, behind the check of the environment's state block."""
    from ._lib import CATCH_STATE_WORDS, CatchCfg
    assert env_state.dtype == torch.int32 and env_state.is_contiguous() and env_state.shape == (B, CATCH_STATE_WORDS)
    return CatchCfg(int(cfg['num_catches']), int(cfg['episode_length']))


@torch.no_grad()
def catch_step(cfg: dict, init: bool, action, draws, n_episodes, env_state, ret_acc, ep_ret, ep_len, in_block, flags):
    """One Catch environment step (or, init: the start of an evaluation) for the B rows of a graphed policy step, as one launch:
    include/resel_hip.h `resel_catch_step`, host twin env_utils/catch.py.  cfg: `Catch.device_config()`.
    action: fp32 [B] view, any stride - the action indices (column 0 of the categorical step's output block);
    draws int32 [B, J, 80] (ns[40] | ms[40] per episode, zeros behind the runs), n_episodes int32 [B] (each at most J), env_state int32
    [B, 90], ret_acc fp64 [B], ep_ret fp64 / ep_len int32 [B, J]; in_block fp32 [B, >= 102] with unit column stride
    (state[49] | lst_state[49] | lst_action[3] | reward[1]), flags int32 [B].
    Everything is updated in place; nothing else on the stream, no host read, no allocation: capturable."""
    from ._lib import CATCH_PAYLOAD_WORDS as W
    _need_cuda('catch_step', action, draws, n_episodes, env_state, ret_acc, ep_ret, ep_len, in_block, flags)
    B, A = flags.numel(), 3
    ld_action, ld_in = _env_rows('catch_step', B, A, action, 1, ret_acc, in_block, obs=49)
    J = _env_eval_tables(B, flags, n_episodes, ep_ret, ep_len)
    assert draws.dtype == torch.int32 and draws.shape == (B, J, W) and draws.is_contiguous()
    c = _catch_cfg(cfg, B, env_state)
    if B == 0:                                           # empty tensors have no address to hand over
        return
    check(lib().resel_catch_step(c, int(bool(init)), _p(action), ld_action, _p(draws), W * J, _p(n_episodes), J, _p(env_state), _p(ret_acc),
                                 _p(ep_ret), _p(ep_len), J, _p(in_block), ld_in, A, _p(flags), B, _stream()), 'catch_step')


@torch.no_grad()
def catch_collect_step(cfg: dict, name2range: dict, init: bool, action, draws, env_state, ret_acc, traj, max_episode_steps: int, in_block):
    """One iteration of the training rollout on Catch (or, init: `env_reset()` with the episode's draws in `draws`) for the B rows of a
    graphed policy step, as one launch: include/resel_hip.h `resel_catch_collect_step`, host twin `SAC._train_loop` / `_push` / `env_step`.
    cfg: `Catch.device_config()`.  name2range: `MemoryArray.name2range`; a stored field must have the width the rollout produces
    (observations 49, last action 3, scalars 1; no log-probability).  action: fp32 [B] view, any stride - the SAMPLED indices (column 1
    of the categorical step's output block); draws int32 [B, 80]; env_state int32 [B, 90], ret_acc fp64 [B]; traj fp32 [B, T_cap, >= the
    layout's width] with unit column stride: the episode block; in_block fp32 [B, >= 102] with unit column stride.
    Everything is updated in place; no host read, no allocation: capturable."""
    from ._lib import CATCH_PAYLOAD_WORDS as W
    _need_cuda('catch_collect_step', action, draws, env_state, ret_acc, traj, in_block)
    assert draws.dtype == torch.int32 and draws.dim() == 2 and draws.shape[1] == W and draws.is_contiguous()
    B, A = draws.shape[0], 3
    ld_action, ld_in = _env_rows('catch_collect_step', B, A, action, 1, ret_acc, in_block, obs=49)
    c = _catch_cfg(cfg, B, env_state)
    T_cap, ld_row = _env_episode_block(B, traj)
    lay = _collect_layout('catch_collect_step', name2range, dict(state=49, last_state=49, next_state=49, last_action=A, logp=0), traj.shape[2])
    if B == 0:                                           # empty tensors have no address to hand over
        return
    check(lib().resel_catch_collect_step(c, lay, int(bool(init)), _p(action), ld_action, _p(draws), _p(env_state), _p(ret_acc), _p(traj), T_cap,
                                         ld_row, int(max_episode_steps), _p(in_block), ld_in, A, B, _stream()), 'catch_collect_step')


@torch.no_grad()
def soft_update_(target_flat, online_flat, tau):
    _need_cuda('soft_update', target_flat, online_flat)
    PARAM_EPOCH[0] += 1
    check(lib().resel_soft_update(_p(target_flat), _p(online_flat), float(tau), target_flat.numel(), _stream()), 'soft_update')


def adamw_bias_corrections(beta1, beta2, step):
    """(1 - beta1^t, sqrt(1 - beta2^t)) of AdamW step t, in fp64: the one spelling the eager (`adamw_flat_`, by value) and the captured
    (`FlatAdamW.prepare_step`, device words) form of the optimizer step share."""
    t = float(step)
    return 1.0 - beta1 ** t, (1.0 - beta2 ** t) ** 0.5


@torch.no_grad()
def adamw_flat_(p, g, m, v, seg_end, seg_lr, seg_wd, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=None):
    _need_cuda('adamw_flat', p, g, m, v, seg_end, seg_lr, seg_wd)
    PARAM_EPOCH[0] += 1
    # the step-dependent factors as the captured update gets them (`adamw_bias_corrections`: fp64 on the host, rounded once), by value:
    # an eagerly launched and a replayed update then take bit-identical steps (`resel_adamw_flat` forms them in fp32 from `step`)
    bc1, bc2_sqrt = adamw_bias_corrections(beta1, beta2, step)
    check(lib().resel_adamw_flat_bc(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(seg_end), _p(seg_lr), _p(seg_wd), int(seg_end.numel()),
                                    float(beta1), float(beta2), float(eps), bc1, bc2_sqrt, _p(grad_scale), _stream()), 'adamw_flat')


@torch.no_grad()
def adamw_flat_dev_(p, g, m, v, seg_end, seg_lr, seg_wd, bias_corrections, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=None):
    """`adamw_flat_` with (1 - beta1^t, sqrt(1 - beta2^t)) read from the 2-element device tensor `bias_corrections` (captured updates)."""
    _need_cuda('adamw_flat_dev', p, g, m, v, seg_end, seg_lr, seg_wd, bias_corrections)
    PARAM_EPOCH[0] += 1
    check(lib().resel_adamw_flat_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(seg_end), _p(seg_lr), _p(seg_wd), int(seg_end.numel()),
                                     float(beta1), float(beta2), float(eps), _p(bias_corrections), _p(grad_scale), _stream()), 'adamw_flat_dev')


@torch.no_grad()
def sumsq(x, out=None):
    _need_cuda('sumsq', x)
    out = torch.empty(1, dtype=torch.float32, device=x.device) if out is None else out
    ws = _ws(lib().resel_sumsq_workspace_bytes(x.numel()), x.device)
    check(lib().resel_sumsq(_p(x), x.numel(), _p(out), _p(ws), _stream()), 'sumsq')
    return out
