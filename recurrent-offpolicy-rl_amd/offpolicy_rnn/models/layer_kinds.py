"""The sequence-layer families and what the rest of the package needs to know about each: ONE record per family (`LayerKind`) and ONE
function that looks inside a layer-id string (`kind_of`).  RNNBase resolves the kind of each of its layers once, at construction; its walk,
its state factory and the trainers read the records and never test an id themselves.

Ids (reference rnn_base.py:101-247): `gru`, `gilr`, `gilr_lstm`, `lru` by exact name; `smamba[_s<N>][_c<K>][_b<blocks>][_n<ln|...>][_ff]`,
`mamba[_s<N>][_c<K>][_noff]`, `conv1d[_<K>]`, `cgpt[_h<H>][_l<L>][_p<drop>][_ml<M>][_rms]` by prefix; the ensemble sequence layers
`elru-<E>` and `econv1d[_<K>]-<E>` (E >= 1, K from 1 to 32, plain decimal digits) by a regular expression - they give every member of an
`efc-<E>` critic its own context encoder and belong in value stacks only.  The dense ids `fc` / `efc-<E>` have no record (`kind_of`
returns None): RNNBase keeps a branch of its own for them.  Ids of reference layers that are outside this build (`lstm`, `egilr-<E>`,
`egilr_lstm-<E>`, `gpt*`, `transformer*`, `cgru`) are recognised and rejected with an explicit message."""
import re
from dataclasses import dataclass
from typing import Callable, Optional

from .conv1d.conv1d import Conv1d
from .conv1d.econv1d import EConv1d
from .flash_attention.TransformerFlashAttention import InferenceParams, TransformerDecoder
from .gilr.gilr import GILRLayer
from .gilr_lstm.gilr_lstm import GILRLSTMLayer
from .gru import GRU
from .lru.elru import EnsembleLRULayer
from .lru.lru import LRULayer
from .s6.mamba import MambaResidualBlock
from .smamba.mamba import BlockList as MambaBlockList

_UNSUPPORTED_PREFIXES = ('lstm', 'gpt', 'transformer', 'cgru', 'egilr')
_E_SEQ_ID = re.compile(r'(elru|econv1d)(?:_([0-9]+))?-([0-9]+)')          # int('4_4') is 44 in Python: the digits are matched, not converted
ECONV1D_MAX_TAPS = 32                       # what csrc/causal_conv1d.hip takes


def parse_smamba_id(layer_id: str) -> dict:
    cfg = dict(d_conv=4, d_state=16, block_num=2, rms_norm=True, use_ff=False)
    for tok in layer_id.split('_')[1:]:
        if tok.startswith('s'):
            cfg['d_state'] = int(tok[1:])
        elif tok.startswith('c'):
            cfg['d_conv'] = int(tok[1:])
        elif tok.startswith('b'):
            cfg['block_num'] = int(tok[1:])
        elif tok.startswith('n'):
            cfg['rms_norm'] = tok[1:] != 'ln'
        elif tok.startswith('f'):
            cfg['use_ff'] = cfg['use_ff'] or tok[1:] == 'f'
        else:
            raise ValueError(f'Pattern {tok} has not been implemented!')
    return cfg


def parse_mamba_id(layer_id: str) -> dict:
    """`mamba[_s<N>][_c<K>][_noff]` (reference rnn_base.py:118-135)."""
    cfg = dict(d_conv=4, d_state=16, use_ff=True)
    for tok in layer_id.split('_')[1:]:
        if tok.startswith('s'):
            cfg['d_state'] = int(tok[1:])
        elif tok.startswith('c'):
            cfg['d_conv'] = int(tok[1:])
        elif tok.startswith('no'):
            if tok[2:] == 'ff':
                cfg['use_ff'] = False
        else:
            raise ValueError(f'Pattern {tok} has not been implemented!')
    return cfg


def parse_cgpt_id(layer_id: str) -> dict:
    cfg = dict(nhead=8, nlayer=4, pdrop=0.1, maxlength=1024, ln=True)
    for tok in layer_id.split('_')[1:]:
        if tok.startswith('h'):
            cfg['nhead'] = int(tok[1:])
        elif tok.startswith('l'):
            cfg['nlayer'] = int(tok[1:])
        elif tok.startswith('p'):
            cfg['pdrop'] = float(tok[1:])
        elif tok.startswith('ml'):
            cfg['maxlength'] = int(tok[2:])
        elif tok.startswith('rms'):
            cfg['ln'] = False
        else:
            raise ValueError(f'Pattern {tok} has not been implemented!')
    return cfg


def parse_e_seq_id(layer_id: str) -> dict:
    """`elru-<E>` / `econv1d[_<K>]-<E>` -> dict(family, num_ensemble, d_conv); anything else behind these prefixes raises."""
    m = _E_SEQ_ID.fullmatch(layer_id)
    bad = NotImplementedError(f'layer id {layer_id!r}: expected elru-<E> or econv1d[_<K>]-<E> with E >= 1 and K from 1 to '
                              f'{ECONV1D_MAX_TAPS} in plain decimal digits')
    if m is None:
        raise bad
    family, k, e = m.group(1), m.group(2), int(m.group(3))
    if e < 1 or (family == 'elru' and k is not None):
        raise bad
    d_conv = 4 if k is None else int(k)
    if family == 'econv1d' and not 1 <= d_conv <= ECONV1D_MAX_TAPS:
        raise bad
    return dict(family=family, num_ensemble=e, d_conv=d_conv)


def _never(layer, x) -> bool:
    return False


def _no_context(layer) -> int:
    return 0


@dataclass(frozen=True)
class LayerKind:
    """build(lid, n_in, n_out) -> (module, state width).
    call(layer, x, state, side, out_act) -> (y, new state): `side` is the incoming RNNHidden (rnn_start, mask, grad_detach,
        attention_concat_mask); each kind hands its module exactly the arguments that module's `forward` takes (they mirror the reference's).
        None for a `deferred` kind.
    fuses_out_act(layer, x): the layer can apply a plain ELU behind it in its own last kernel (`out_act='elu'`) - the per-kind half of the
        condition; RNNBase._fuse_out_act holds the half that is the same for every kind.
    deferred: the walk does not run the recurrence itself: it yields `layer.recurrence_job(x, state)` and is sent the output sequence
        (`layer.finish`), so that several towers' recurrences can share one launch (RNNBase.lockstep_forward).
    honours_start: the state is cleared / masked at the first token of a trajectory (`rnn_start`, `mask`, or per-trajectory attention
        segments), so rows may pack several trajectories and a pass shifted by one slot computes the same tokens.
    context_len(layer): tokens in front of a sampled sequence that the layer reads (a causal convolution's window).
    packs_sequences: consumes the per-row sequence-length table (`attention_concat_mask`).
    make_state(width, batch_size): the rollout state where it is no zero tensor of (1, batch, width).
    member_axis: an ensemble sequence layer - its output carries a leading member axis [E, B, T, C] (it takes member-major or shared
        input), every member of the stack has to be evaluated (`RNNBase.members_coupled`), it cannot sit in a policy stack and is
        never stepped one token at a time."""
    name: str
    build: Callable
    call: Optional[Callable]
    fuses_out_act: Callable = _never
    deferred: bool = False
    honours_start: bool = True
    context_len: Callable = _no_context
    packs_sequences: bool = False
    make_state: Optional[Callable] = None
    member_axis: bool = False

    def __reduce__(self):                   # a copied / pickled network keeps pointing at the one record of its family
        return kind_by_name, (self.name,)


def _whole_rows(x) -> bool:
    return x.dim() == 3 and x.shape[-2] > 1            # whole packed rows (training) vs one rollout step


def _build_mamba(lid, n_in, n_out):
    cfg = parse_mamba_id(lid)
    layer = MambaResidualBlock(n_in, n_out, d_conv=cfg['d_conv'], d_state=cfg['d_state'], use_ff=cfg['use_ff'])
    return layer, layer.mixer.desired_hidden_dim


def _build_conv1d(lid, n_in, n_out):
    layer = Conv1d(n_in, n_out, d_conv=int(lid.split('_')[-1]) if '_' in lid else 4)
    return layer, layer.desired_hidden_dim


def _build_elru(lid, n_in, n_out):
    E = parse_e_seq_id(lid)['num_ensemble']
    return EnsembleLRULayer(n_in, n_out, E, batch_first=True), n_out * 2 * E


def _build_econv1d(lid, n_in, n_out):
    cfg = parse_e_seq_id(lid)
    layer = EConv1d(n_in, n_out, num_ensemble=cfg['num_ensemble'], d_conv=cfg['d_conv'])
    return layer, layer.desired_hidden_dim


def _build_smamba(lid, n_in, n_out):
    cfg = parse_smamba_id(lid)
    assert n_in == n_out, f'mamba_simple require input_dim == output_dim, while got {n_in} and {n_out}'
    layer = MambaBlockList(cfg['block_num'], n_in, d_conv=cfg['d_conv'], d_state=cfg['d_state'], rms_norm=cfg['rms_norm'],
                           use_ff=cfg['use_ff'])
    return layer, layer.desired_hidden_dim


def _build_cgpt(lid, n_in, n_out):
    cfg = parse_cgpt_id(lid)              # its "state width" is the KV cache's length
    return TransformerDecoder(n_in, cfg['nhead'], 4 * n_in, cfg['nlayer'], cfg['pdrop'], cfg['ln']), cfg['maxlength']


def _call_cgpt(layer, x, state, side, out_act):
    multi = _whole_rows(x)
    y = layer(x, inference_params=None if multi else state, seqlens=side.attention_concat_mask if multi else None, out_act=out_act)
    if not multi:
        state.seqlen_offset += y.shape[-2]        # reference :451-452
    return y, state


GRU_KIND = LayerKind(                                   # no reset / mask handling (reference :453-454)
    'gru', build=lambda lid, n_in, n_out: (GRU(n_in, n_out, batch_first=True), n_out), call=None, deferred=True, honours_start=False)
GILR = LayerKind(
    'gilr', build=lambda lid, n_in, n_out: (GILRLayer(n_in, n_out, batch_first=True), n_out),
    call=lambda layer, x, state, side, out_act: layer(x, state, side.rnn_start, out_act=out_act),
    fuses_out_act=lambda layer, x: layer.use_ff)        # the ELU rides in the closing add + LayerNorm kernel of the feed-forward block
GILR_LSTM = LayerKind(
    'gilr_lstm', build=lambda lid, n_in, n_out: (GILRLSTMLayer(n_in, n_out, batch_first=True), n_out * 2),
    call=lambda layer, x, state, side, out_act: layer(x, state, side.rnn_start))
LRU = LayerKind(
    'lru', build=lambda lid, n_in, n_out: (LRULayer(n_in, n_out, batch_first=True), n_out * 2),
    call=lambda layer, x, state, side, out_act: layer(x, state, side.rnn_start, side.grad_detach, out_act=out_act),
    fuses_out_act=lambda layer, x: layer.use_ff)
MAMBA = LayerKind(
    'mamba', build=_build_mamba,
    call=lambda layer, x, state, side, out_act: layer(x, state, side.rnn_start, side.mask, side.grad_detach),
    context_len=lambda layer: layer.mixer.d_conv)
SMAMBA = LayerKind(
    'smamba', build=_build_smamba,
    call=lambda layer, x, state, side, out_act: layer(x, state, side.rnn_start, side.mask, out_act=out_act),
    fuses_out_act=lambda layer, x: not layer.use_ff,    # the ELU rides in the head GEMM's epilogue
    context_len=lambda layer: layer.d_conv)
CONV1D = LayerKind(
    'conv1d', build=_build_conv1d, call=lambda layer, x, state, side, out_act: layer(x, state, side.mask),
    context_len=lambda layer: layer.d_conv)
CGPT = LayerKind(                                       # the ELU rides in the decoder's output GEMM
    'cgpt', build=_build_cgpt, call=_call_cgpt, fuses_out_act=lambda layer, x: _whole_rows(x), packs_sequences=True,
    make_state=lambda width, batch_size: InferenceParams(max_seqlen=width, max_batch_size=batch_size))

ELRU = LayerKind(                                       # (no ELU rides in its closing add + norm: the activation module runs behind it)
    'elru', build=_build_elru, call=lambda layer, x, state, side, out_act: layer(x, state, side.rnn_start, side.grad_detach),
    member_axis=True)
ECONV1D = LayerKind(
    'econv1d', build=_build_econv1d, call=lambda layer, x, state, side, out_act: layer(x, state, side.mask),
    context_len=lambda layer: layer.d_conv, member_axis=True)

_EXACT = {k.name: k for k in (GRU_KIND, GILR, GILR_LSTM, LRU)}
_PREFIXED = (SMAMBA, MAMBA, CONV1D, CGPT)
_E_SEQ = {k.name: k for k in (ELRU, ECONV1D)}
_BY_NAME = {k.name: k for k in (GRU_KIND, GILR, GILR_LSTM, LRU, SMAMBA, MAMBA, CONV1D, CGPT, ELRU, ECONV1D)}


def kind_by_name(name: str) -> LayerKind:
    return _BY_NAME[name]


def is_rnn_layer(layer_id: str) -> bool:
    return layer_id != 'fc' and not layer_id.startswith('efc')


def kind_of(lid: str) -> Optional[LayerKind]:
    """The family of a layer id; None for the dense ids.  Exact names first, then prefixes: `gilr_lstm` is not a `gilr` with a suffix, and
    `smamba*` never reaches the `mamba` prefix.  Raises for ids outside this build."""
    if not is_rnn_layer(lid):
        return None
    if lid in _EXACT:
        return _EXACT[lid]
    for kind in _PREFIXED:
        if lid.startswith(kind.name):
            return kind
    if lid.startswith(('elru', 'econv1d')):
        return _E_SEQ[parse_e_seq_id(lid)['family']]
    if lid.startswith('egilr'):
        # `egilr-<E>` does not run in the reference: EnsembleGILRLayer transposes the [1, B, E C] state RNNBase hands it and then scans
        # E B rows of width C (gilr/egilr.py:72-76), so its first forward raises, at layer level and in the trainers; `egilr_lstm-<E>`
        # is mapped to the ensemble LRU class there (rnn_base.py:110-113) - use `elru-<E>` for that
        raise NotImplementedError(f"layer id {lid!r}: the reference's EnsembleGILRLayer raises on its first forward (it transposes the "
                                  f"[1, B, E*C] state and scans E*B rows of width C, gilr/egilr.py:72-76), and it maps egilr_lstm-<E> to "
                                  f"its ensemble LRU class (rnn_base.py:110-113): use elru-<E>")
    if lid == 'lstm':
        # the reference lists `lstm` (rnn_base.py:58) but cannot run it on this path either: ContextualModel.meta_forward asks every
        # embedding network for its full hidden sequence (contextual_model.py:92-94, 113-115) and RNNHidden refuses to hold one for an
        # LSTM (RNNHidden.py:23-25: 'It is not supported to store full RNN output of LSTM!!!')
        raise NotImplementedError("layer id 'lstm': the reference's full-trajectory path rejects it as well (RNNHidden.py:23-25 asserts "
                                  "when ContextualModel.meta_forward requests the full hidden sequence, contextual_model.py:92-94)")
    if lid.startswith(_UNSUPPORTED_PREFIXES):
        raise NotImplementedError(f'layer id {lid!r} exists in the reference but is outside the MI355X hot path of this build '
                                  f'(supported: fc, efc-<E>, gru, gilr, lru, gilr_lstm, smamba_*, mamba_*, conv1d_*, cgpt_*, elru-<E>, econv1d_*-<E>)')
    raise NotImplementedError(f'unknown layer id {lid!r}')
