"""RNNBase: a stack of layers selected by layer-id strings, with a per-layer (norm, activation) tail
(reference offpolicy_rnn/models/rnn_base.py:31-532).

Layer-id grammar kept from the reference (:101-247): the dense ids `fc` and `efc-<E>` are handled here; what a sequence-layer id means -
how the layer is built, called and what the trainers may assume about it - is one record of `layer_kinds.py`, resolved per layer at
construction (`layer_kind`).  Module / parameter naming (`layer_list.<i>.…`, `activation_list.<i>.0.…`) matches the reference so that
its per-module checkpoints load."""
import copy
import os
from typing import List, Optional, Tuple, Union

import torch

from ..hip import ops
from .RNNHidden import RNNHidden
from .ensemble_linear_model import EnsembleLinear, critic_mlp, critic_mlp_fusable, ensemble_head, head_fusable
from .flash_attention.TransformerFlashAttention import TransformerDecoder
from .conv1d.conv1d import Conv1d
from .conv1d.econv1d import EConv1d
from .gilr.gilr import GILRLayer
from .gilr_lstm.gilr_lstm import GILRLSTMLayer
from .s6.mamba import MambaResidualBlock
from .lru.elru import EnsembleLRULayer
from .lru.lru import LRULayer
from .smamba.mamba import BlockList as MambaBlockList
from .layer_kinds import is_rnn_layer, kind_of, parse_cgpt_id, parse_mamba_id, parse_smamba_id  # noqa: F401  (the parsers: part of this module's surface)
from .linear import Linear

ACTIVATIONS = {'tanh': torch.nn.Tanh, 'relu': torch.nn.ReLU, 'sigmoid': torch.nn.Sigmoid, 'leaky_relu': torch.nn.LeakyReLU,
               'linear': torch.nn.Identity, 'elu': torch.nn.ELU, 'gelu': torch.nn.GELU}


# Set by the trainers around an update (`training_pass()`): nobody reads the per-layer output sequences (`full_rnn_memory`) of a training
# pass, so a sequence layer may hand back its output with the following plain ELU already applied by its last GEMM's epilogue (the
# reference's full hidden holds the PRE-activation sequence, rnn_base.py:456-460: outside a training pass nothing changes).  The entry of
# such a layer in the returned `full` RNNHidden is None.
# Per THREAD: a rollout / evaluation forward running on another thread while an update is in flight (the reference samples from the policy
# between updates; a user may do so concurrently) must keep getting the pre-activation sequences.  Autograd's backward threads never read it.
import threading
_TRAINING_PASS = threading.local()


def _in_training_pass() -> bool:
    return getattr(_TRAINING_PASS, 'depth', 0) > 0


class training_pass:
    def __enter__(self):
        _TRAINING_PASS.depth = getattr(_TRAINING_PASS, 'depth', 0) + 1

    def __exit__(self, *exc):
        _TRAINING_PASS.depth -= 1
        return False


class RNNBase(torch.nn.Module):
    def __init__(self, input_size: int, output_size: int, hidden_size_list: List[int], activation: List[str],
                 layer_type: List[str]):
        super().__init__()
        assert len(activation) - 1 == len(hidden_size_list), 'number of activation should be larger by 1 than size of hidden layers.'
        assert len(activation) == len(layer_type), 'number of layer type should equal to the activate'
        self.activation_dict = ACTIVATIONS
        self.check_is_rnn = is_rnn_layer
        self.layer_type = copy.deepcopy(layer_type)
        self.activation_type = copy.deepcopy(activation)
        self.layer_list = torch.nn.ModuleList()
        self.activation_list = torch.nn.ModuleList()
        self.layer_kind = []                    # per layer: its layer_kinds record, None for a dense layer (unknown ids raise here)
        self.rnn_hidden_state_input_size, self.rnn_layer_type = [], []
        self.rnn_num = 0
        self.input_size = input_size
        self.output_size = output_size
        width_in = input_size
        for ind, width in enumerate(list(hidden_size_list) + [output_size]):
            lid = self.layer_type[ind]
            self.layer_kind.append(kind_of(lid))
            layer, hidden_width = self._make_layer(lid, self.layer_kind[ind], width_in, width)
            self.layer_list.append(layer)
            if hidden_width is not None:
                self.rnn_num += 1
                self.rnn_hidden_state_input_size.append(hidden_width)
                self.rnn_layer_type.append(lid)
            self.activation_list.append(self._make_activation(activation[ind], width))
            width_in = width
        self.rnn_layer_kind = [kind for kind in self.layer_kind if kind is not None]           # beside rnn_layer_type
        self._check_member_counts()
        self._norm_refused = set()              # layers whose `+` norm the HIP kernels refused (logged once each)
        self.xavier_initialize_weights()

    @staticmethod
    def _make_layer(lid: str, kind, n_in: int, n_out: int):
        """-> (module, state width; None for a dense layer)."""
        if kind is not None:
            return kind.build(lid, n_in, n_out)
        if lid == 'fc':
            return Linear(n_in, n_out), None
        return EnsembleLinear(n_in, n_out, int(lid.split('-')[-1])), None

    def _check_member_counts(self):
        """An ensemble sequence layer (`elru-<E>`, `econv1d[_K]-<E>`) runs E members: the `efc-<E>` layers of its stack must agree."""
        for lid, kind, layer in zip(self.layer_type, self.layer_kind, self.layer_list):
            if kind is None or not kind.member_axis:
                continue
            for other, mod in zip(self.layer_type, self.layer_list):
                if isinstance(mod, (EnsembleLinear, EnsembleLRULayer, EConv1d)) and mod.num_ensemble != layer.num_ensemble:
                    raise ValueError(f'layer {lid!r} runs {layer.num_ensemble} members but layer {other!r} of the same stack runs '
                                     f'{mod.num_ensemble}: the member counts of a stack must agree')

    @staticmethod
    def _make_activation(spec: str, width: int):
        if '+' not in spec:
            return ACTIVATIONS[spec]()
        norm, act = spec.split('+')
        if norm.startswith('eln'):
            shape = [int(norm.split('-')[-1]), width]
        elif norm == 'ln':
            shape = width
        else:
            raise NotImplementedError(f'norm {norm}')
        return torch.nn.ModuleList([torch.nn.LayerNorm(shape), ACTIVATIONS[act]()])

    def xavier_initialize_weights(self):
        """Xavier-uniform weights / zero biases for the plain layers; smamba keeps its own init (reference :267-354)."""
        def xavier_ensemble(efc):
            with torch.no_grad():
                for i in range(efc.weight.shape[0]):
                    torch.nn.init.xavier_uniform_(efc.weight[i].transpose(0, 1))
                if getattr(efc, 'bias', None) is not None:
                    efc.bias.zero_()
        for m in self.layer_list:
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    torch.nn.init.constant_(m.bias, 0)
            elif isinstance(m, EnsembleLinear):
                xavier_ensemble(m)
            elif isinstance(m, LRULayer):
                xavier_ensemble(m.in_proj)
                xavier_ensemble(m.middle_proj)
            elif isinstance(m, EnsembleLRULayer):           # Xavier per [i, j] slice, zero biases (reference rnn_base.py:284-290)
                with torch.no_grad():
                    for efc in (m.in_proj, m.middle_proj):
                        for i in range(efc.weight.shape[0]):
                            for j in range(efc.weight.shape[1]):
                                torch.nn.init.xavier_uniform_(efc.weight[i, j].transpose(0, 1))
                        if getattr(efc, 'bias', None) is not None:
                            efc.bias.zero_()
            elif isinstance(m, GILRLayer):
                torch.nn.init.xavier_uniform_(m.out_proj.weight)
                torch.nn.init.constant_(m.out_proj.bias, 0)
                xavier_ensemble(m.in_proj)
            elif isinstance(m, GILRLSTMLayer):
                torch.nn.init.xavier_uniform_(m.out_proj.weight)
                torch.nn.init.constant_(m.out_proj.bias, 0)
                xavier_ensemble(m.in_proj)
                xavier_ensemble(m.middle_proj)
            elif isinstance(m, (MambaBlockList, TransformerDecoder, MambaResidualBlock, Conv1d, EConv1d)):
                pass
            else:
                for name, param in m.named_parameters():
                    if 'weight' in name:
                        torch.nn.init.xavier_uniform_(param.data)
                    elif 'bias' in name:
                        torch.nn.init.constant_(param.data, 0)

    def sequence_layers(self):
        """[(kind, module)] of the sequence layers, in stack order: what the trainers ask about a network's layers, they ask here."""
        return [(kind, layer) for kind, layer in zip(self.layer_kind, self.layer_list) if kind is not None]

    def members_coupled(self) -> bool:
        """An `eln-<E>` norm normalises a token over ALL members jointly: the members of this stack cannot be evaluated as a subset.  Nor
        can those of a stack with an ensemble sequence layer: its feed-forward block holds the same joint norm, and its state and
        activations are laid out for all E members."""
        return any(spec.startswith('eln') for spec in self.activation_type) or self.emits_member_axis()

    def emits_member_axis(self) -> bool:
        """The stack holds an ensemble sequence layer: what it hands on carries a leading member axis [E, B, T, C]."""
        return any(kind is not None and kind.member_axis for kind in self.layer_kind)

    def rnn_parameters(self, recursive=True):
        out = []
        for _, layer in self.sequence_layers():
            out += list(layer.rnn_parameters()) if hasattr(layer, 'rnn_parameters') else list(layer.parameters(recursive))
        return out

    # ------------------------------------------------------------------------------------------ hidden state
    def _make_state(self, batch_size, device, random: bool) -> RNNHidden:
        st = RNNHidden(self.rnn_num, self.rnn_layer_type, device)
        make = st.init_random_hidden_by_type if random else st.init_hidden_by_type
        for width, lid, kind in zip(self.rnn_hidden_state_input_size, self.rnn_layer_type, self.rnn_layer_kind):
            st.append(kind.make_state(width, batch_size) if kind.make_state else make(lid, batch_size, width, device))
        return st

    def make_init_state(self, batch_size: int, device: Union[str, torch.device] = torch.device('cpu')) -> RNNHidden:
        return self._make_state(batch_size, device, False)

    def make_rnd_init_state(self, batch_size: int, device: Union[str, torch.device] = torch.device('cpu')) -> RNNHidden:
        return self._make_state(batch_size, device, True)

    # ------------------------------------------------------------------------------------------ forward
    def _fuse_out_act(self, ind, x) -> bool:
        """The activation module behind sequence layer `ind` is a plain ELU and this is a training pass over whole fp32 GPU sequences: a
        layer whose kind can (`LayerKind.fuses_out_act`) may apply it in its last kernel (`out_act='elu'`)."""
        act_mod = self.activation_list[ind]
        return (_in_training_pass() and isinstance(act_mod, torch.nn.ELU) and act_mod.alpha == 1.0 and x.is_cuda
                and x.dtype == torch.float32 and x.dim() == 3 and x.shape[-2] > 1)

    def meta_forward(self, x: torch.Tensor, hidden_state: Optional[RNNHidden] = None, require_full_hidden: bool = False,
                     first_grad_part=None, out_dest=None) -> Tuple[torch.Tensor, RNNHidden, Optional[RNNHidden]]:
        """The forward pass.  (Runs `_forward_steps` with every `gru` recurrence on its own, `ops.gru_seq`.)"""
        steps = self._forward_steps(x, hidden_state, require_full_hidden, first_grad_part, out_dest)
        try:
            job = next(steps)
            while True:
                job = steps.send(ops.gru_seq(*job))
        except StopIteration as done:
            return done.value

    @staticmethod
    def lockstep_forward(passes):
        """passes = [(network, x, hidden_state, with_grad), ...] -> [(out, out_state, full), ...], each what `network.meta_forward(x,
        hidden_state, require_full_hidden=True)` returns under `torch.set_grad_enabled(with_grad)`.  The networks are walked together:
        every pass runs up to its next `gru` layer (the other layers one network after the other, as `meta_forward` does them), then the
        recurrences that are waiting and agree in (B, L, H) go out as ONE `ops.gru_seq_multi` launch - independent latency-bound
        recurrences share the chip without a stream each, on the current stream.  Passes that do not line up (other layer lists or
        shapes) simply get launches of their own: same results, one after the other."""
        ambient = torch.is_grad_enabled()
        gens = [net._forward_steps(x, hidden, True, None, None) for net, x, hidden, _ in passes]
        grads = [bool(g) and ambient for _, _, _, g in passes]
        results, jobs, reply = [None] * len(passes), {}, {}
        live = set(range(len(passes)))
        while live:
            for i in sorted(live):
                with torch.set_grad_enabled(grads[i]):
                    try:
                        jobs[i] = gens[i].send(reply.pop(i)) if i in reply else next(gens[i])
                    except StopIteration as done:
                        results[i] = done.value
                        live.discard(i)
            groups = {}
            for i in sorted(jobs):
                gi = jobs[i][0]
                key = tuple(gi.shape) if gi.is_cuda and gi.dim() == 3 else ('alone', i)
                groups.setdefault(key, []).append(i)
            for members in groups.values():
                for at in range(0, len(members), ops.GRU_MULTI_MAX):
                    part = members[at:at + ops.GRU_MULTI_MAX]
                    with torch.set_grad_enabled(ambient):       # each job says for itself whether it is differentiated
                        ys = ops.gru_seq_multi([tuple(jobs[i]) + (grads[i],) for i in part])
                    for i, y in zip(part, ys):
                        reply[i] = y
            jobs.clear()
        return results

    def _forward_steps(self, x: torch.Tensor, hidden_state: Optional[RNNHidden] = None, require_full_hidden: bool = False,
                       first_grad_part=None, out_dest=None):
        """Generator form of the forward pass: yields the (gi, W_hh, b_hh, h0) of every `gru` layer (a `deferred` kind), is sent that
        recurrence's output sequence, and returns (out, out_state, full) - so that ONE walk serves `meta_forward` and `lockstep_forward`.
        Per layer: a dense step or a sequence step (through the layer's kind), then the activation tail.
        first_grad_part = (x_part, col0): the first layer (a shared-input efc layer) differentiates x only through that
        column block (EnsembleLinear.forward); anything else keeps the ordinary path.
        out_dest: an `ops.ColDest` - if the LAST layer is an `fc` on the hand-written GEMM, its output is written straight into that column
        block of a row buffer (the caller checks with `dest.holds`)."""
        assert x.shape[-1] == self.input_size, f'inputting size does not match!!!! input is {x.shape[-1]}, expected: {self.input_size}'
        if hidden_state is None:
            hidden_state = self.make_init_state(x.shape[0], x.device)
        assert len(hidden_state) == self.rnn_num, f'rnn num does not match, input is {len(hidden_state)}, expected: {self.rnn_num}'
        squeeze = x.dim() == 2 and self.rnn_num > 0
        if squeeze:
            x = x.unsqueeze(0)
        out_state = RNNHidden(self.rnn_num, self.rnn_layer_type, device=x.device, batch_first=False)
        full = RNNHidden(self.rnn_num, self.rnn_layer_type, device=x.device, batch_first=True) if require_full_hidden else None
        k = 0
        fused_next = 0
        for ind, layer in enumerate(self.layer_list):
            if fused_next:                          # consumed by the ensemble head / critic MLP node of the dense step
                fused_next -= 1
                continue
            kind = self.layer_kind[ind]
            if kind is None:
                x, fused_next, act_done = self._dense_step(ind, layer, x, first_grad_part, out_dest)
            else:
                # the plain ELU behind the layer rides in the layer's last kernel (training passes only, see _TRAINING_PASS): its entry
                # in the full record is None and the activation module below is skipped
                out_act = 'elu' if kind.fuses_out_act(layer, x) and self._fuse_out_act(ind, x) else None
                if kind.deferred:
                    x, h = layer.finish((yield layer.recurrence_job(x, hidden_state[k])))
                else:
                    x, h = kind.call(layer, x, hidden_state[k], hidden_state, out_act)
                k += 1
                out_state.append(h)
                act_done = out_act is not None
                if require_full_hidden:
                    full.append(None if act_done else x)
            if act_done:
                continue
            act = self.activation_list[ind]
            if isinstance(act, torch.nn.ModuleList):
                x = self._norm_tail(ind, act, x)
            else:
                x = act(x)
        if squeeze:
            x = x.squeeze(0)
        return x, out_state, full

    def _norm_fused(self, ind, norm, x) -> bool:
        """The `ln+` / `eln-E+` norm behind layer `ind` runs in `ops.member_layer_norm`: an fp32 GPU tensor of a shape the kernels take -
        for `eln-E`, one whose axis 0 is the E members the norm was built for - unless RESEL_NORM_FUSED=0 (read per call)."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.numel() > 0 and norm.elementwise_affine and ops.norm_fused_on()):
            return False
        shape = tuple(norm.normalized_shape)
        if len(shape) == 2 and not (x.dim() >= 3 and x.shape[0] == shape[0]):
            return False
        E, C = (shape[0], shape[1]) if len(shape) == 2 else (1, shape[0])
        if x.shape[-1] != C:
            return False
        if not ops.member_layer_norm_ok(E, C):
            if ind not in self._norm_refused:                 # said once per layer
                self._norm_refused.add(ind)
                print(f'[ WARNING ] {self.activation_type[ind]} behind layer {ind}: {E} x {C} is outside what the HIP norm kernels take '
                      f'(width % 4 == 0, E * width <= {ops.MEMBER_NORM_MAX}); this layer keeps the torch LayerNorm')
            return False
        return True

    def _norm_tail(self, ind, act, x):
        """The (norm, activation) tail of a `+` spec (reference rnn_base.py:461-467).  On the GPU the norm is one pass over the activations
        where the layer left them, with a plain ELU riding in it; any other activation module runs behind it.  Parameters stay those of
        `activation_list.<ind>.0` (a torch LayerNorm), which also is the spelling for everything the kernels do not take."""
        norm, tail = act[0], act[1]
        if self._norm_fused(ind, norm, x):
            elu = isinstance(tail, torch.nn.ELU) and tail.alpha == 1.0
            x = ops.member_layer_norm(x, norm.weight, norm.bias, norm.eps, 'elu' if elu else None)
            return x if elu else tail(x)
        if self.activation_type[ind].startswith('eln'):
            x = norm(x.transpose(-2, 0)).transpose(-2, 0)
        else:
            x = norm(x)
        return tail(x)

    def _dense_step(self, ind, layer, x, first_grad_part, out_dest):
        """The `fc` / `efc-<E>` layer `ind` -> (x, number of following layers its node consumed, their / its activation already applied)."""
        n_layers = len(self.layer_list)
        act = self.activation_list[ind]
        # efc-E ELU -> efc-E(H) ELU -> efc-E(1) = the published critic: ONE node whose GEMM epilogues carry the head and the
        # ELU backward / bias gradient between the layers (ensemble_linear_model._CriticMLP)
        if ind + 3 == n_layers and critic_mlp_fusable(layer, act, self.layer_list[ind + 1], self.activation_list[ind + 1],
                                                      self.layer_list[ind + 2], self.activation_list[ind + 2], x):
            x = critic_mlp(layer, self.layer_list[ind + 1], self.layer_list[ind + 2], x, grad_part=first_grad_part if ind == 0 else None)
            return x, 2, True
        # efc-E(H) ELU -> efc-E(1) at the end of the stack (the critic head): one fused node
        if ind + 2 == n_layers and head_fusable(layer, act, self.layer_list[ind + 1], self.activation_list[ind + 1], x):
            x = ensemble_head(layer, self.layer_list[ind + 1], x)
            return x, 1, True
        # a fusable activation behind fc / efc-E - a plain ELU; on fp32 GPU passes also relu, leaky_relu (slope 0.01), tanh, sigmoid
        # (`ops.dense_act_name`, RESEL_ACT_FUSED) - rides in the layer's GEMM epilogue; the backward runs from the output
        name = ops.dense_act_name(act, x) if isinstance(layer, (EnsembleLinear, torch.nn.Linear)) and x.dtype == torch.float32 else None
        if name is not None:
            if isinstance(layer, EnsembleLinear):
                x = layer(x, act=name, grad_part=first_grad_part if ind == 0 else None)
            else:
                assert not (ind == 0 and first_grad_part is not None)
                x = ops.linear_act(x, layer.weight, layer.bias, name, dest=out_dest if ind == n_layers - 1 else None)
            return x, 0, True
        assert not (ind == 0 and first_grad_part is not None), 'first_grad_part needs an efc first layer with a fusable activation'

        if isinstance(layer, torch.nn.Linear):                    # the bias rides in the GEMM epilogue (every pass: whole trajectories and rollout steps)
            x = ops.linear_act(x, layer.weight, layer.bias, None, dest=out_dest if ind == n_layers - 1 else None)
        else:
            x = layer(x)
        return x, 0, False

    # ------------------------------------------------------------------------------------------ weights
    @staticmethod
    def _copy_weight_from(dst_net: torch.nn.Module, src_net: torch.nn.Module, tau: float):
        """dst <- tau * dst + (1 - tau) * src  (tau = 0: hard copy).  Per-tensor form; ContextualModel overrides this
        with one flat-buffer kernel for whole networks."""
        with torch.no_grad():
            if tau == 0.0:
                dst_net.load_state_dict(src_net.state_dict())
                return
            if tau == 1.0:
                return
            src, dst = list(src_net.parameters(True)), list(dst_net.parameters(True))
            assert len(src) == len(dst), 'parameter number show be equal!'
            for s, d in zip(src, dst):
                d.data.mul_(tau).add_(s.data, alpha=1 - tau)

    def copy_weight_from(self, src_net: 'RNNBase', tau: float):
        RNNBase._copy_weight_from(self, src_net, tau)

    def save(self, path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save(self.state_dict(), path)

    def load(self, path, **kwargs):
        self.load_state_dict(torch.load(path, map_location=kwargs.get('map_location')))

    def l2_norm_square(self) -> torch.Tensor:
        return sum(torch.sum(p ** 2) for p in self.parameters(True))
