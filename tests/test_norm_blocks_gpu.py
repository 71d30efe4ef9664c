"""The `ln+<act>` / `eln-<E>+<act>` norm blocks of the dense stacks on cuda:0.

1. the kernels (`ops.member_layer_norm` over `resel_member_layernorm_*`) against an fp64 LayerNorm, in both layouts, at the bounds
   tests/test_hip_ops.py holds the add + LayerNorm kernels to (`close_fwd` for outputs; `close(rtol=2e-4, atol_scale=5e-5)` for gradients);
2. whole stacks against the oracle restatement (oracle/network.py) at the output bound of tests/test_layers_gpu.py (rtol 1e-4, atol 2e-5);
3. the path: with the kernels in force ATen sees no layer norm and no activation-sized copy around it;
4. a trainer with such specs in all four stacks: the oracle trainer, graphed update and policy step, checkpoints."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_ops import close, close_fwd

pytestmark = pytest.mark.gpu
EPS = 1e-5


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from offpolicy_rnn.hip import ops as o
    return o


# ------------------------------------------------------------------------------------------------ 1. kernels against fp64
def _operand(layout, E, M, C, g, lead=None):
    """x on the CPU and a function that puts it on the device in `layout`: 'token' = the strided [E, M, C] view of a token-major
    [M, E C] buffer (what a shared-input EnsembleLinear returns), 'member' = dense [E, M, C]; E = 1 with a 1-D weight: [M, C].
    lead: split M into these leading axes ([E, *lead, C], as the trainers' [E, rows, T, C])."""
    x = torch.randn(E, M, C, generator=g) * 2.0 + 0.5

    def to_device(t):
        if layout == 'token':
            d = t.transpose(0, 1).contiguous().cuda().view(M, E * C).view(M, E, C).transpose(0, 1)
            assert d.stride() == (C, E * C, 1) or E == 1 or M == 1
        else:
            d = t.contiguous().cuda()
        return d if lead is None else d.view((E,) + tuple(lead) + (C,))
    return x, to_device


def _reference(x, w, b, act, dy):
    """F.layer_norm over the (E, C) features of a token, in double on the CPU -> y, dx, dw, db."""
    E, C = w.shape
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    y = F.layer_norm(x64.transpose(-2, 0), (E, C), w64, b64, EPS).transpose(-2, 0)
    y = F.elu(y) if act else y
    (y * dy.double()).sum().backward()
    return y.detach(), x64.grad, w64.grad, b64.grad


CASES = [('token', 1, 37, 12, None), ('token', 8, 3, 256, None), ('member', 3, 5, 8, None), ('member', 2, 1, 64, None),
         ('member', 8, 67, 256, None), ('member', 8, 130, 32, (10, 13)),
         # where the library takes another path: a token of 512 floats is the widest a single wave holds, 768 and 528 are a workgroup's
         # with one float4 per thread (8 x 256 above: two); 8200 narrow tokens are more than the 2048 x 4 the persistent backward grid holds
         # at once, 2100 wide ones more than twice its 1024 workgroups (both of a workgroup's LDS slot pairs are used again)
         ('token', 2, 9, 256, None), ('member', 3, 7, 256, None), ('token', 1, 8200, 12, None), ('member', 3, 2100, 176, None)]


@pytest.mark.parametrize('act', [None, 'elu'])
@pytest.mark.parametrize('layout,E,M,C,lead', CASES)
def test_kernel_vs_fp64(ops, layout, E, M, C, lead, act):
    g = torch.Generator().manual_seed(1000 * E + 10 * M + C)
    x, put = _operand(layout, E, M, C, g, lead)
    w, b = 1.0 + 0.3 * torch.randn(E, C, generator=g), 0.3 * torch.randn(E, C, generator=g)
    dy = torch.randn(E, M, C, generator=g)
    y_ref, dx_ref, dw_ref, db_ref = _reference(x, w, b, act, dy)
    plain = E == 1                                                  # `ln`: [M, C] rows with a 1-D weight
    xd = (put(x)[0] if plain else put(x)).requires_grad_(True)
    wd = (w[0] if plain else w).cuda().requires_grad_(True)
    bd = (b[0] if plain else b).cuda().requires_grad_(True)
    y = ops.member_layer_norm(xd, wd, bd, EPS, act)
    assert y.shape == xd.shape and y.stride() == xd.stride(), 'the output lies where the producer left the input: no densifying copy'
    y.backward((put(dy)[0] if plain else put(dy)).view(y.shape))
    assert xd.grad.stride() == xd.stride(), 'the gradient goes back in the layout of the input'
    close_fwd(y.reshape(E, M, C), y_ref, name='y')
    close(xd.grad.reshape(E, M, C), dx_ref, rtol=2e-4, atol_scale=5e-5, name='dx')
    close(wd.grad.reshape(E, C), dw_ref, rtol=2e-4, atol_scale=5e-5, name='dw')
    close(bd.grad.reshape(E, C), db_ref, rtol=2e-4, atol_scale=5e-5, name='db')


@pytest.mark.parametrize('act', [None, 'elu'])
def test_kernel_takes_a_gradient_in_another_layout_than_the_input(ops, act):
    """x is the [E, M, C] view of a token-major buffer, the arriving gradient is member-major dense (and the other way round)."""
    E, M, C = 3, 11, 16
    g = torch.Generator().manual_seed(7)
    w, b = 1.0 + 0.3 * torch.randn(E, C, generator=g), 0.3 * torch.randn(E, C, generator=g)
    for lx, lg in (('token', 'member'), ('member', 'token')):
        x, put_x = _operand(lx, E, M, C, g)
        dy, put_g = torch.randn(E, M, C, generator=g), _operand(lg, E, M, C, g)[1]
        y_ref, dx_ref, dw_ref, db_ref = _reference(x, w, b, act, dy)
        xd, wd, bd = put_x(x).requires_grad_(True), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        y = ops.member_layer_norm(xd, wd, bd, EPS, act)
        y.backward(put_g(dy))
        close_fwd(y, y_ref, name='y')
        close(xd.grad, dx_ref, rtol=2e-4, atol_scale=5e-5, name='dx')
        close(wd.grad, dw_ref, rtol=2e-4, atol_scale=5e-5, name='dw')
        close(bd.grad, db_ref, rtol=2e-4, atol_scale=5e-5, name='db')


@pytest.mark.parametrize('layout', ['token', 'member'])
def test_constant_token_is_finite_and_equals_the_reference(ops, layout):
    """Zero variance: rstd = eps^-1/2 = 316 multiplies x - mean, which must be an exact zero (0.3 has no short binary form: a mean formed
    as sum / N carries a rounding residue that the factor would blow up to 1e-5 of the value)."""
    E, M, C = 3, 5, 8
    g = torch.Generator().manual_seed(3)
    x, put = _operand(layout, E, M, C, g)
    x[:, 2, :] = 0.3
    x[:, 4, :] = -1234.567
    w, b = 1.0 + 0.3 * torch.randn(E, C, generator=g), 0.3 * torch.randn(E, C, generator=g)
    dy = torch.randn(E, M, C, generator=g)
    for act in (None, 'elu'):
        y_ref, dx_ref, dw_ref, db_ref = _reference(x, w, b, act, dy)
        xd, wd, bd = put(x).requires_grad_(True), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        y = ops.member_layer_norm(xd, wd, bd, EPS, act)
        y.backward(put(dy))
        assert torch.isfinite(y).all() and torch.isfinite(xd.grad).all()
        if act is None:
            assert torch.equal(y[:, 2].cpu(), b) and torch.equal(y[:, 4].cpu(), b), 'a constant token normalises to exactly the bias'
        else:
            torch.testing.assert_close(y[:, 2].cpu(), F.elu(b), rtol=1e-6, atol=1e-7)
        close_fwd(y, y_ref, name='y')
        close(xd.grad, dx_ref, rtol=2e-4, atol_scale=5e-5, name='dx')
        close(wd.grad, dw_ref, rtol=2e-4, atol_scale=5e-5, name='dw')
        close(bd.grad, db_ref, rtol=2e-4, atol_scale=5e-5, name='db')


def test_unaddressable_layouts_are_copied_not_misread(ops):
    """A column stride of 2 and a token axis that does not collapse to one stride: the node falls back to a dense copy."""
    E, M, C = 2, 6, 8
    g = torch.Generator().manual_seed(5)
    w, b = 1.0 + 0.3 * torch.randn(E, C, generator=g), 0.3 * torch.randn(E, C, generator=g)
    wide = torch.randn(E, M, 2 * C, generator=g)
    x1 = wide[..., ::2]                                             # column stride 2
    x2 = torch.randn(E, 3, 4, C, generator=g)[:, :, :2]             # [E, 3, 2, C]: the (3, 2) token axes have strides (4 C, C)
    for x in (x1, x2):
        y_ref = F.layer_norm(x.double().transpose(-2, 0), (E, C), w.double(), b.double(), EPS).transpose(-2, 0)
        xd = wide.cuda()[..., ::2] if x is x1 else x.contiguous().cuda().repeat(1, 1, 2, 1)[:, :, :2]
        assert xd.stride() != xd.contiguous().stride()
        y = ops.member_layer_norm(xd, w.cuda(), b.cuda(), EPS, None)
        close_fwd(y, y_ref, name='y')


def test_output_carries_a_magnitude_bound_the_next_gemm_uses(ops, monkeypatch):
    """At update size the forward publishes sqrt(E C) max|w| + max|b| for its output and `apply_tagged` hangs it on the tensor: the GEMM
    behind runs mode 2 without a pre-pass, and RESEL_AMAX_VERIFY finds the bound above every element."""
    monkeypatch.setattr(ops, 'AMAX_VERIFY', True)
    assert ops.gemm_split() == 2
    E, M, C = 8, 520, 256                                           # E M C >= 2^20: the size from which producers publish
    g = torch.Generator().manual_seed(9)
    w, b = (1.0 + 0.3 * torch.randn(E, C, generator=g)).cuda(), (0.3 * torch.randn(E, C, generator=g)).cuda()
    W = torch.randn(E, C, 64, generator=g).cuda()
    for layout in ('token', 'member'):
        x = _operand(layout, E, M, C, g)[1](torch.randn(E, M, C, generator=g) * 3.0)
        for act in (None, 'elu'):
            y = ops.member_layer_norm(x, w, b, EPS, act)
            h = ops.amax_of(y)
            assert h is not None, 'no magnitude handle on the output'
            bound = ops.amax_value(h)
            assert bound == pytest.approx(float((E * C) ** 0.5 * w.abs().max() + b.abs().max()), rel=1e-6)
            assert float(y.abs().max()) <= bound
            n0 = ops._VERIFY_TAG[0]
            ops.gemm_f32(y, W, True, False, amax_b=ops.amax(W))      # the operand's handle is the tag: no amax_a given
            assert ops._VERIFY_TAG[0] > n0, 'the product did not run in mode 2'
            ops.amax_verify_raise(x.device)


# ------------------------------------------------------------------------------------------------ 2. stacks against the oracle
STACKS = {'efc': (['efc-3'] * 3, ['eln-3+elu', 'eln-3+tanh', 'linear'], 4),
          'gru': (['fc', 'gru', 'fc'], ['ln+elu', 'ln+elu', 'linear'], None)}
N_IN, N_OUT, HIDDEN, ROWS, T = 20, 4, [24, 48], 3, 9          # (the gru kernels take widths that are multiples of 16)
_stack_cache = {}


def _stack(name):
    """-> (net on cuda:0, x, weights of the loss, oracle output and parameter gradients in double): computed once per stack."""
    if name not in _stack_cache:
        from offpolicy_rnn.models.rnn_base import RNNBase
        from oracle import network as NW
        lt, act, nd = STACKS[name]
        torch.manual_seed(11)
        net = RNNBase(N_IN, N_OUT, HIDDEN, act, lt)
        with torch.no_grad():
            for p in net.activation_list.parameters():
                p.add_(torch.randn_like(p) * 0.3)
            for layer in net.layer_list:
                if hasattr(layer, 'desire_ndim'):
                    layer.desire_ndim = nd                          # as the trainers set it: a [rows, T, C] batch is a shared input
                for k, p in layer.named_parameters():
                    if 'bias' in k:
                        p.add_(torch.randn_like(p) * 0.1)
        x = torch.randn(ROWS, T, N_IN)
        lw = torch.randn((3, ROWS, T, N_OUT) if name == 'efc' else (ROWS, T, N_OUT))
        p64 = {k: v.detach().double().requires_grad_(True) for k, v in net.state_dict().items()}
        ref = NW.rnn_base_forward(p64, dict(layer_type=lt, activation=act), x.double(), NW.Flags(), desire_ndim=nd)
        (ref * lw.double()).sum().backward()
        _stack_cache[name] = (net.cuda(), x, lw, ref.detach(), {k: v.grad for k, v in p64.items()})
    return _stack_cache[name]


def _run_stack(net, x, lw):
    net.zero_grad()
    y, _, _ = net.meta_forward(x.cuda())
    (y * lw.cuda()).sum().backward()
    return y.detach().cpu(), {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize('name', list(STACKS))
def test_stack_vs_oracle(ops, name, monkeypatch):
    monkeypatch.delenv('RESEL_NORM_FUSED', raising=False)
    net, x, lw, ref, gref = _stack(name)
    y, grads = _run_stack(net, x, lw)
    np.testing.assert_allclose(y, ref, rtol=1e-4, atol=2e-5)
    assert set(grads) == set(gref)
    for k, v in gref.items():
        np.testing.assert_allclose(grads[k], v, rtol=1e-4, atol=2e-5, err_msg=k)


# ------------------------------------------------------------------------------------------------ 3. the path
NORM_OPS = ('aten::layer_norm', 'aten::native_layer_norm', 'aten::native_layer_norm_backward')
COPY_OPS = ('aten::copy_', 'aten::clone', 'aten::contiguous')


def _recorded(fn, min_numel):
    """Run fn under the dispatcher recorder -> (ATen norm ops seen, [(op, shape)] of the copies of tensors with at least min_numel elements)."""
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU], record_shapes=True) as prof:
        out = fn()
        torch.cuda.synchronize()
    norms = sorted({e.name for e in prof.events() if e.name in NORM_OPS})
    copies = []
    for e in prof.events():
        if e.name in COPY_OPS and e.input_shapes and e.input_shapes[0]:
            if int(np.prod(e.input_shapes[0])) >= min_numel:
                copies.append((e.name, tuple(e.input_shapes[0])))
    return out, norms, copies


@pytest.mark.parametrize('name', list(STACKS))
def test_the_path_is_the_hand_written_one(ops, name, monkeypatch):
    """Forward + backward of the stacks above.  Fused (the default the switch earned, or RESEL_NORM_FUSED=1): the dispatcher sees no
    ATen layer norm, and no more copies of activation-sized tensors than the SAME stack without the norms makes - the norm reads and
    writes the producer's layout.  RESEL_NORM_FUSED=0: the ATen norm is back, and both spellings agree within the bounds above."""
    from offpolicy_rnn.models.rnn_base import RNNBase
    net, x, lw, ref, gref = _stack(name)
    E = 3 if name == 'efc' else 1
    act_numel = E * ROWS * T * min(HIDDEN)                          # the smallest normalised activation
    assert act_numel > ROWS * T * N_IN and act_numel > E * ROWS * T * N_OUT     # ... is larger than the stack's input and output
    monkeypatch.setenv('RESEL_NORM_FUSED', '1')
    _run_stack(net, x, lw)                                          # first call: lazy handles, weight magnitudes
    (y1, g1), norms, copies = _recorded(lambda: _run_stack(net, x, lw), act_numel)
    assert norms == [], f'ATen norm ops on the fused path: {norms}'
    lt, act, nd = STACKS[name]
    torch.manual_seed(11)
    bare = RNNBase(N_IN, N_OUT, HIDDEN, [a.split('+')[-1] for a in act], lt)
    for layer in bare.layer_list:
        if hasattr(layer, 'desire_ndim'):
            layer.desire_ndim = nd
    bare.cuda()
    _run_stack(bare, x, lw)
    _, _, bare_copies = _recorded(lambda: _run_stack(bare, x, lw), act_numel)
    print(f'{name}: activation-sized copies with the norms {copies}, without {bare_copies}')
    assert len(copies) <= len(bare_copies), f'copies of activation-sized tensors around the norm: {copies} (the stack without norms: {bare_copies})'
    monkeypatch.setenv('RESEL_NORM_FUSED', '0')
    (y0, g0), norms0, copies0 = _recorded(lambda: _run_stack(net, x, lw), act_numel)
    assert 'aten::native_layer_norm' in norms0 and 'aten::native_layer_norm_backward' in norms0
    np.testing.assert_allclose(y1, y0, rtol=1e-4, atol=2e-5)
    for k in g0:
        np.testing.assert_allclose(g1[k], g0[k], rtol=1e-4, atol=2e-5, err_msg=k)


def test_a_width_the_kernels_refuse_keeps_the_torch_norm_and_says_so_once(ops, monkeypatch, capsys):
    """Width 6 is no multiple of 4: `RESEL_EINVAL` at the entry, so the layer keeps the torch LayerNorm (same results as the oracle) and
    the log says so once, not per call; the 8-wide layer beside it runs in the kernel."""
    from offpolicy_rnn.models.rnn_base import RNNBase
    from oracle import network as NW
    monkeypatch.setenv('RESEL_NORM_FUSED', '1')
    lt, act = ['fc', 'fc', 'fc'], ['ln+elu', 'ln+elu', 'linear']
    torch.manual_seed(2)
    net = RNNBase(5, 3, [6, 8], act, lt)
    with torch.no_grad():
        for p in net.activation_list.parameters():
            p.add_(torch.randn_like(p) * 0.3)
    x = torch.randn(4, 7, 5)
    ref = NW.rnn_base_forward({k: v.double() for k, v in net.state_dict().items()}, dict(layer_type=lt, activation=act), x.double())
    net.cuda()
    capsys.readouterr()
    (y1, _, _), norms, _ = _recorded(lambda: net.meta_forward(x.cuda()), 1)
    y2, _, _ = net.meta_forward(x.cuda())
    out = capsys.readouterr().out
    assert out.count('keeps the torch LayerNorm') == 1 and 'ln+elu behind layer 0' in out
    assert norms == ['aten::layer_norm', 'aten::native_layer_norm'] and net._norm_refused == {0}
    np.testing.assert_allclose(y1.detach().cpu(), ref, rtol=1e-4, atol=2e-5)
    assert torch.equal(y1, y2)


def test_library_exports_the_norm_symbols(ops):
    from offpolicy_rnn.hip import _lib
    h = _lib.lib()
    for name in ('resel_member_layernorm_fwd', 'resel_member_layernorm_bwd', 'resel_member_layernorm_bwd_workspace_bytes'):
        assert name in _lib.SIGNATURES and hasattr(h, name)
    assert h.resel_abi_version() == 11


# ------------------------------------------------------------------------------------------------ 4. trainer
NORM_SPECS = dict(value_activations=['eln-2+elu', 'eln-2+elu', 'linear'], value_layer_type=['efc-2'] * 3,
                  policy_activations=['ln+elu', 'ln+elu', 'linear'], value_embedding_activations=['ln+elu', 'ln+elu', 'linear'],
                  policy_embedding_activations=['ln+elu', 'ln+elu', 'linear'])
LENS = [12, 5, 7, 12, 4, 9, 6]


def _norm_parameters(net):
    """[(name, parameter)] of the LayerNorm parameters of a policy / value model's stacks."""
    return [(f'{mod}.{k}', p) for mod, m in net.contextual_modules.items() for k, p in m.named_parameters() if 'activation_list' in k]


def _fill(alg, lens, seed=9, also=None):
    from test_host_logic import _push, _synth
    rs = np.random.RandomState(seed)
    for n in lens:
        o, a, r = _synth(rs, n, 5, 3)
        _push(alg.replay_buffer, o, a, r, early_done=(n != 12))
        if also is not None:
            also(o, a, r, n)


def _val(v):
    return v[0] if isinstance(v, tuple) else v


def test_two_updates_vs_oracle_trainer(ops, monkeypatch):
    """gru SAC-REDQ, D = 32, 4 rows x 12 steps, `eln-2+elu` critic layers, `ln+elu` policy and encoder layers: two chained updates
    against the CPU oracle trainer at the bounds of tests/test_trainer_gpu.py (scalars 2e-3 / 5e-4, parameters 1e-3 / 2e-5)."""
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.utility import rng
    from oracle.trainer import OracleTrainer, default_parameter
    from test_host_logic import make_parameter
    from test_oracle_golden import _push as opush
    monkeypatch.delenv('RESEL_NORM_FUSED', raising=False)
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.randn(tuple(shape), dtype=dtype).to(device))
    torch.manual_seed(11)
    alg = alg_init(make_parameter('gru', sac_batch_size=4 * 12, **NORM_SPECS))
    assert alg.device.type == 'cuda'
    with torch.no_grad():                                           # norms away from their (1, 0) initialisation
        for net in (alg.policy, alg.values[0]):
            assert len(_norm_parameters(net)) == 8                 # two norms in the encoder, two in the head: weight and bias each
            for _, p in _norm_parameters(net):
                p.add_(torch.randn_like(p) * 0.2)
    alg._value_update(tau=0.0)
    cpu = lambda sd: {m: {k: v.detach().cpu().clone() for k, v in d.items()} for m, d in sd.items()}
    par = default_parameter(rnn='gru', D=32, sac_batch_size=4 * 12, policy_embedding_dim=16, value_embedding_dim=16,
                            policy_uni_model_input_mapping_dim=16, value_uni_model_input_mapping_dim=16, max_buffer_transition_num=5000, **NORM_SPECS)
    tr = OracleTrainer(par, 5, 3, 12, policy_state=cpu(alg.policy.state_dict()), value_state=cpu(alg.values[0].state_dict()))
    _fill(alg, LENS, also=lambda o, a, r, n: opush(tr.buffer, o, a, r, early_done=(n != 12)))
    logs = []
    for runner in (alg, tr):
        torch.manual_seed(200)
        np.random.seed(200)
        out = []
        for _ in range(2):
            out.append(dict(runner.train_one_batch()))
            runner.grad_num += 1
        logs.append(out)
    for it, (a, b) in enumerate(zip(*logs)):
        for k, v in b.items():
            assert _val(a[k]) == pytest.approx(_val(v), rel=2e-3, abs=5e-4), (it, k, _val(a[k]), _val(v))
    for net, ref in ((alg.policy, tr.policy), (alg.values[0], tr.value), (alg.target_values[0], tr.target_value)):
        sd = net.state_dict()
        assert any('activation_list' in k for k in sd['universal_model'])
        for mod, d in ref.items():
            for k, v in d.items():
                np.testing.assert_allclose(sd[mod][k].detach().cpu(), v.detach(), rtol=1e-3, atol=2e-5, err_msg=f'{mod}.{k}')


def _graph_trainer(**over):
    from offpolicy_rnn import alg_init
    from test_host_logic import make_parameter
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter('gru', sac_batch_size=4 * 12 - 1, cuda_inference=True, **dict(NORM_SPECS, **over)))
    _fill(alg, [12] * 8, seed=3)
    np.random.seed(11)
    return alg


def test_graphed_update_equals_the_eager_update(ops, monkeypatch):
    """`GraphedUpdate.refusal` is None for such a trainer, and four updates stepped through it (one warm-up, one recording, replays) leave the
    logs and every parameter where five eager updates leave them, at the 2e-5 of tests/test_trainer_gpu.py."""
    from offpolicy_rnn.algorithm.graphed_update import GraphedUpdate
    from offpolicy_rnn.utility import rng
    monkeypatch.delenv('RESEL_NORM_FUSED', raising=False)
    monkeypatch.setattr(rng, 'randn', lambda shape, device, dtype=torch.float32: torch.zeros(tuple(shape), dtype=dtype, device=device))
    state = lambda alg: [alg.policy.store.flat.detach().clone(), alg.values[0].store.flat.detach().clone(),
                         alg.target_values[0].store.flat.detach().clone(), alg.log_sac_alpha.detach().clone()]
    eager = _graph_trainer()
    assert GraphedUpdate.refusal(eager) is None
    logs_e = []
    for _ in range(5):
        logs_e.append(dict(eager.train_one_batch()))
        eager.grad_num += 1
    graphed = _graph_trainer()
    g = GraphedUpdate(graphed, warmup=1)
    try:
        logs_g = []
        for _ in range(5):
            logs_g.append(dict(g.step()))
            graphed.grad_num += 1
        torch.cuda.synchronize()
        assert len(g.graphs) == 1 and 1 <= g.eager_fallbacks <= 3, (len(g.graphs), g.eager_fallbacks)
    finally:
        g.close()
    for nm, a, b in zip(('policy', 'value', 'target value', 'log alpha'), state(graphed), state(eager)):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=2e-7, err_msg=nm)
    for le, lg in zip(logs_e, logs_g):
        assert set(le) == set(lg)
        for k in le:
            assert abs(_val(le[k]) - _val(lg[k])) <= 2e-5 * max(1.0, abs(_val(le[k]))), (k, le[k], lg[k])


@pytest.mark.parametrize('B', [1, 3])
def test_graphed_policy_step_equals_the_eager_step(ops, B, monkeypatch):
    """The rollout step (one token per environment: M = 1 and M = B rows for the norm) replayed from its graph, against the eager forward;
    B = 3 is the batched form the evaluator steps."""
    from offpolicy_rnn.hip.graph_step import GraphedPolicyStep
    monkeypatch.delenv('RESEL_NORM_FUSED', raising=False)
    alg = _graph_trainer()
    dev = alg.device
    rows = lambda a: torch.as_tensor(a, dtype=torch.float32, device=dev).unsqueeze(1)      # [B, 1, width]: B rows of one step
    with torch.no_grad():
        for _, p in _norm_parameters(alg.policy):
            p.add_(torch.randn_like(p) * 0.2)
    rs = np.random.RandomState(3)
    n = 6
    obs, acts, rew = rs.randn(n + 1, B, alg.obs_dim), np.tanh(rs.randn(n + 1, B, alg.act_dim)), rs.randn(n + 1, B, 1)
    step = GraphedPolicyStep(alg.policy, dev, batch_size=B)
    hid = alg.policy.make_init_state(B, dev)
    step.load_hidden(None)
    for t in range(n):
        with torch.no_grad():
            mean, _, _, _, hid, _ = alg.policy.forward(state=rows(obs[t + 1]), lst_state=rows(obs[t]), lst_action=rows(acts[t]), rnn_memory=hid,
                                                       reward=rows(rew[t]))
        gmean, gsample, glogp = step(obs[t + 1], obs[t], acts[t], rew[t])
        np.testing.assert_allclose(gmean, mean.reshape(B, -1).cpu().numpy(), rtol=1e-5, atol=1e-5, err_msg=f'step {t}')
        assert np.isfinite(gsample).all() and np.isfinite(glogp).all()
    assert step._graph is not None


def test_verify_mode_and_checkpoint_round_trips(ops, monkeypatch, tmp_path):
    """RESEL_AMAX_VERIFY=1 raises nothing over two updates; `save()` / `load()` and `save_state()` / `load_state()` hand a fresh trainer
    the parameters (the norm weights among them) bit for bit."""
    monkeypatch.delenv('RESEL_NORM_FUSED', raising=False)
    monkeypatch.setattr(ops, 'AMAX_VERIFY', True)
    monkeypatch.chdir(tmp_path)
    alg = _graph_trainer()
    for _ in range(2):
        log = dict(alg.train_one_batch())                          # raises AmaxBoundError itself at the end of the update
        alg.grad_num += 1
    ops.amax_verify_raise(alg.device)
    assert all(np.isfinite(_val(v)) for v in log.values())
    monkeypatch.setattr(ops, 'AMAX_VERIFY', False)
    nets = lambda a: (a.policy, a.values[0], a.target_values[0])
    norm_w = [p for k, p in _norm_parameters(alg.values[0]) if k.endswith('weight')]
    assert norm_w and not any(torch.equal(p, torch.ones_like(p)) for p in norm_w), 'the norm weights were trained'
    alg.save(str(tmp_path / 'model'))
    reader = _graph_trainer()
    assert not torch.equal(reader.values[0].store.flat, alg.values[0].store.flat)
    reader.load(str(tmp_path / 'model'))
    for a, b in zip(nets(reader), nets(alg)):
        assert torch.equal(a.store.flat, b.store.flat)
        assert list(a.state_dict()) == list(b.state_dict())
    assert torch.equal(reader.log_sac_alpha, alg.log_sac_alpha)
    alg.env_reset()
    path = alg.save_state(str(tmp_path / 'states' / 'one'))
    reader2 = _graph_trainer()
    reader2.load_state(path)
    for a, b in zip(nets(reader2), nets(alg)):
        assert torch.equal(a.store.flat, b.store.flat)
    assert torch.equal(reader2.optimizers_value[0].m, alg.optimizers_value[0].m) and reader2.grad_num == alg.grad_num
    log2 = dict(reader2.train_one_batch())                          # ... and goes on training
    assert all(np.isfinite(_val(v)) for v in log2.values())


def test_discrete_actions_one_update(ops, monkeypatch):
    """The categorical head sits behind the same stacks: one update of the discrete-action trainer with the norm specs."""
    from offpolicy_rnn import alg_init
    from offpolicy_rnn.buffers.transition_buffer.replay_memory import Transition
    from test_host_logic import make_parameter
    from test_oracle_golden import push_discrete
    monkeypatch.delenv('RESEL_NORM_FUSED', raising=False)
    torch.manual_seed(0)
    np.random.seed(0)
    alg = alg_init(make_parameter('gru', env='synthetic-o5-d4-T12', sac_batch_size=4 * 12, **NORM_SPECS))
    assert alg.discrete_env and alg.device.type == 'cuda'
    rs = np.random.RandomState(9)
    for n in LENS:
        push_discrete(alg.replay_buffer, Transition, rs, n, 5, 4, 12)
    before = [alg.policy.store.flat.clone(), alg.values[0].store.flat.clone()]
    log = dict(alg.train_one_batch())
    assert 'critic_loss' in log and all(np.isfinite(_val(v)) for v in log.values())
    assert not torch.equal(before[0], alg.policy.store.flat) and not torch.equal(before[1], alg.values[0].store.flat)
    for net in (alg.policy, alg.values[0]):
        assert all(torch.isfinite(p).all() for p in net.parameters())
