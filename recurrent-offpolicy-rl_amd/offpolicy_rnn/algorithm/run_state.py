"""The whole state of a `train()` run on disk, so that a run that was stopped continues as the run it was (`SAC.save_state` /
`SAC.load_state`, `RESEL_CHECKPOINT_DIR` / `RESEL_CHECKPOINT_EVERY` read at `train()`).  `SAC.save()` / `load()` keep the reference's
model files and know nothing of this.

One state is one directory:

    manifest.json   format version, completed iterations, the fingerprint of the trainer that wrote it - written LAST
    ring.npz        the replay ring's occupied rows and its tables (numpy, no pickle)
    host.pkl        what lives on the host: random streams, the environment object, rollout mirrors, counters, the open episode's
                    pending transitions, the evaluator's streams and environments
    tensors.pt      what lives in tensors: flat parameter stores, optimizer moments, Q-guard, the device generator, recurrent state

A state is written into `tmp-<pid>` beside its final place and renamed there (`os.replace`), so a directory without a manifest is never
a state: `complete_states` skips it and the next successful `write_checkpoint` removes it.  `write_checkpoint` keeps the two newest
states of a checkpoint directory.

Everything in this module is host code over plain objects (a ring, a dict of fields): the trainer's side - what goes into the three
payload files and how it comes back - is `SAC._collect_state` / `SAC._apply_state` (algorithm/sac.py)."""
import contextlib
import json
import os
import pickle
import random
import re
import shutil
from typing import Dict, List, Optional, Tuple

import numpy as np

FORMAT_VERSION = 1
MANIFEST, RING, HOST, TENSORS = 'manifest.json', 'ring.npz', 'host.pkl', 'tensors.pt'
KEEP = 2                                                   # complete states a checkpoint directory holds after a write
CHECKPOINT_EVERY_DEFAULT = 25                              # RESEL_CHECKPOINT_EVERY when the variable is not set: the cadence of `save()`
_STATE = re.compile(r'^state-(\d{6,})$')


class RunStateMismatch(Exception):
    """The state on disk was written by another trainer: `field` names what differs (`saved` there, `current` here)."""

    def __init__(self, field: str, saved, current):
        super().__init__(f'run state does not fit this trainer: {field} is {saved!r} in the state and {current!r} here')
        self.field, self.saved, self.current = field, saved, current


# ---------------------------------------------------------------------------------------------------- switches
def checkpoint_dir_from_env() -> Optional[str]:
    return os.environ.get('RESEL_CHECKPOINT_DIR') or None


def checkpoint_every_from_env() -> int:
    raw = os.environ.get('RESEL_CHECKPOINT_EVERY')
    if raw is None:
        return CHECKPOINT_EVERY_DEFAULT
    try:
        every = int(raw)
    except ValueError:
        every = 0
    if every < 1 or str(every) != raw.strip():
        raise ValueError(f'RESEL_CHECKPOINT_EVERY must be an integer >= 1 (iterations between run states), got {raw!r}')
    return every


def refuse_process_groups():
    """Data-parallel resume is out of scope: every rank holds its own ring and streams, and a state is one rank's."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(f'run states are not implemented for a process group of {dist.get_world_size()} ranks: '
                                  'save_state / load_state / RESEL_CHECKPOINT_DIR work in a single process only')


# ---------------------------------------------------------------------------------------------------- the ring
def occupied_rows(ring) -> int:
    """Row 0 up to the furthest row any trajectory table entry reaches (the block behind it was never written, or holds evicted rows)."""
    return max((s + n for s, n in zip(ring.trajectory_start, ring.trajectory_length)), default=0)


def ring_state(ring) -> Dict[str, np.ndarray]:
    """The ring as numpy arrays: the occupied rows, the tables, `ptr` / `transition_count` and the column layout.  Not the pending
    transitions (objects: they travel with the host payload) and not the ring object (its device mirror would come along)."""
    hi = occupied_rows(ring)
    has_layout = ring.memory_buffer is not None
    names = sorted(ring.name2range)
    return dict(rows=ring.memory_buffer[:hi].copy() if has_layout else np.zeros((0, 0), dtype=ring.STORE_DTYPE),
                trajectory_start=np.asarray(ring.trajectory_start, dtype=np.int64), trajectory_length=np.asarray(ring.trajectory_length, dtype=np.int64),
                scalars=np.asarray([ring.ptr, ring.transition_count, int(has_layout), int(getattr(ring, 'width', 0))], dtype=np.int64),
                layout_names=np.asarray(names, dtype=np.str_), layout_ranges=np.asarray([ring.name2range[n] for n in names], dtype=np.int64).reshape(-1, 2))


def save_ring(ring, path: str):
    with open(path, 'wb') as f:
        np.savez(f, **ring_state(ring))


def read_ring(path: str) -> Dict[str, np.ndarray]:
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def ring_layout(st) -> Dict[str, Tuple[int, int]]:
    return {str(n): (int(a), int(b)) for n, (a, b) in zip(st['layout_names'], st['layout_ranges'])}


def load_ring(ring, st, pending=()):
    """Put `st` (`ring_state` / `read_ring`) and the pending transitions into `ring`, an object of the capacity that wrote it.  The
    block is allocated as the first trajectory would have allocated it, and the device mirror is dropped: the next sample builds it anew."""
    ptr, count, has_layout, width = (int(v) for v in st['scalars'])
    ring.reset()
    if has_layout:
        ring.name2range = ring_layout(st)
        ring.width = width
        ring.memory_buffer = np.zeros((ring.max_transition_num + int(ring.max_traj_step), width), dtype=ring.STORE_DTYPE)
        rows = st['rows']
        assert rows.dtype == ring.STORE_DTYPE and rows.shape[1] == width and len(rows) <= len(ring.memory_buffer), (rows.dtype, rows.shape)
        ring.memory_buffer[:len(rows)] = rows
    else:
        ring.memory_buffer, ring.name2range = None, {}
    ring.trajectory_start, ring.trajectory_length = [int(v) for v in st['trajectory_start']], [int(v) for v in st['trajectory_length']]
    ring.ptr, ring.transition_count = ptr, count
    ring.memory = list(pending)
    ring.__dict__.pop('_dev_state', None)
    ring._dirty = []


# ---------------------------------------------------------------------------------------------------- fingerprint
def check_fingerprint(saved: dict, current: dict):
    """Raise `RunStateMismatch` for the first field of `current` that `saved` holds another value for.  JSON turns tuples into lists,
    so both sides are compared after one trip through it.  A `None` on this side is not compared: a fresh trainer's ring has no column
    layout before its first trajectory."""
    saved, current = json.loads(json.dumps(saved)), json.loads(json.dumps(current))
    for field in current:
        if current[field] is None:
            continue
        if field not in saved or saved[field] != current[field]:
            raise RunStateMismatch(field, saved.get(field), current[field])


# ---------------------------------------------------------------------------------------------------- one state directory
def _flush(path: str):
    fd = os.open(path, os.O_RDONLY)
    try:
        os.fsync(fd)
    finally:
        os.close(fd)


def write_state(path: str, manifest: dict, ring, host: dict, tensors: dict):
    """One state at `path`: the payload files into a temporary sibling, the manifest last, then one rename."""
    import torch
    path = os.path.abspath(path)
    parent = os.path.dirname(path)
    os.makedirs(parent, exist_ok=True)
    tmp = os.path.join(parent, f'tmp-{os.getpid()}')
    if os.path.isdir(tmp):
        shutil.rmtree(tmp)
    os.makedirs(tmp)
    save_ring(ring, os.path.join(tmp, RING))
    with open(os.path.join(tmp, HOST), 'wb') as f:
        pickle.dump(host, f, protocol=4)
    torch.save(tensors, os.path.join(tmp, TENSORS))
    for name in (RING, HOST, TENSORS):                     # on the disk before the manifest says they are: a machine that goes down
        _flush(os.path.join(tmp, name))                    # must not leave a manifest beside half-written payload
    with open(os.path.join(tmp, MANIFEST), 'w') as f:
        json.dump(dict(manifest, format_version=FORMAT_VERSION), f, indent=1, sort_keys=True)
    _flush(os.path.join(tmp, MANIFEST))
    if os.path.isdir(path):                                # a state of the same name (a run restarted from an older state): replaced whole
        shutil.rmtree(path)
    os.replace(tmp, path)
    return path


def read_manifest(path: str) -> Optional[dict]:
    """The manifest of the state directory `path`; None when it is not a complete state of this format."""
    try:
        with open(os.path.join(path, MANIFEST)) as f:
            manifest = json.load(f)
    except (OSError, ValueError):
        return None
    if not isinstance(manifest, dict) or manifest.get('format_version') != FORMAT_VERSION:
        return None
    return manifest


def read_state(path: str):
    """-> (manifest, ring arrays, host dict, tensors on the CPU), all of it or an exception: nothing is applied from here."""
    import torch
    manifest = read_manifest(path)
    if manifest is None:
        raise FileNotFoundError(f'{path} holds no complete run state of format {FORMAT_VERSION} (no readable {MANIFEST})')
    with open(os.path.join(path, HOST), 'rb') as f:
        host = pickle.load(f)
    tensors = torch.load(os.path.join(path, TENSORS), map_location='cpu', weights_only=False)
    return manifest, read_ring(os.path.join(path, RING)), host, tensors


# ---------------------------------------------------------------------------------------------------- a checkpoint directory
def state_name(iterations: int) -> str:
    return f'state-{int(iterations):06d}'


def complete_states(directory: str) -> List[Tuple[int, str]]:
    """[(completed iterations, path)] of the complete states in `directory`, oldest first."""
    out = []
    if not os.path.isdir(directory):
        return out
    for name in os.listdir(directory):
        m = _STATE.match(name)
        path = os.path.join(directory, name)
        if m and os.path.isdir(path) and read_manifest(path) is not None:
            out.append((int(m.group(1)), path))
    return sorted(out)


def newest_state(directory: str) -> Optional[Tuple[int, str]]:
    states = complete_states(directory)
    return states[-1] if states else None


def prune(directory: str, keep: int = KEEP):
    """After a successful write: remove what is not a state (`tmp-*` leftovers, `state-*` without a manifest) and all but the `keep`
    newest states.  Nothing else in the directory is touched."""
    states = complete_states(directory)
    good = {path for _, path in states[-keep:]}
    for name in os.listdir(directory):
        path = os.path.join(directory, name)
        if os.path.isdir(path) and (_STATE.match(name) or name.startswith('tmp-')) and path not in good:
            shutil.rmtree(path, ignore_errors=True)


def write_checkpoint(directory: str, iterations: int, save_state) -> str:
    """`save_state(path)` into `directory/state-<iterations>`, then `prune`."""
    path = os.path.join(directory, state_name(iterations))
    save_state(path)
    prune(directory)
    return path


# ---------------------------------------------------------------------------------------------------- random streams
@contextlib.contextmanager
def generators_kept(device):
    """Python's, numpy's and torch's CPU generator and `device`'s generator leave the block as they entered it.  A resumed run captures
    its graphs again, at points where the uninterrupted run captured nothing: the warm-up passes of such a capture draw from the device
    generator, and the run must not see that (`BatchedPolicyEval.evaluate` keeps its own captures out of the streams the same way)."""
    import torch
    device = torch.device(device)
    cuda = device.type == 'cuda'
    saved = (random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state(device) if cuda else None)
    try:
        yield
    finally:
        random.setstate(saved[0])
        np.random.set_state(saved[1])
        torch.set_rng_state(saved[2])
        if cuda:
            torch.cuda.set_rng_state(saved[3], device)


# ---------------------------------------------------------------------------------------------------- recurrent state
def hidden_to_host(hidden) -> Optional[list]:
    """An `RNNHidden`'s per-layer state as CPU tensors: ('t', tensor), ('tuple', [tensors]) or ('kv', {position, caches}) per layer."""
    import torch
    if hidden is None:
        return None
    out = []
    for h in hidden._data:
        if torch.is_tensor(h):
            out.append(('t', h.detach().cpu().clone()))
        elif isinstance(h, tuple):
            out.append(('tuple', [t.detach().cpu().clone() for t in h]))
        else:                                              # a cgpt KV-cache handle: the caches and the position they are filled to
            out.append(('kv', dict(seqlen_offset=int(h.seqlen_offset), max_seqlen=int(h.max_seqlen), max_batch_size=int(h.max_batch_size),
                                   caches={k: v.detach().cpu().clone() for k, v in h.key_value_memory_dict.items()})))
    return out


def hidden_from_host(hidden, saved: list, device, in_place: bool):
    """Put `saved` (`hidden_to_host`) into `hidden`.  in_place: the tensors of `hidden` are static (a graphed step reads their
    addresses) and are written through; otherwise they are replaced, shapes as saved."""
    import torch
    assert len(saved) == len(hidden._data), (len(saved), len(hidden._data))
    for i, ((tag, val), h) in enumerate(zip(saved, hidden._data)):
        if tag == 't':
            if in_place:
                h.copy_(val.reshape(h.shape))
            else:
                hidden._data[i] = val.to(device)
        elif tag == 'tuple':
            if in_place:
                for t, v in zip(h, val):
                    t.copy_(v.reshape(t.shape))
            else:
                hidden._data[i] = tuple(v.to(device) for v in val)
        else:
            assert not torch.is_tensor(h) and not isinstance(h, tuple), 'the state holds a KV cache where this policy has none'
            h.max_seqlen, h.max_batch_size, h.seqlen_offset = val['max_seqlen'], val['max_batch_size'], val['seqlen_offset']
            h.key_value_memory_dict = {k: v.to(device) for k, v in val['caches'].items()}
            if h.device_offset is not None:
                h.device_offset.fill_(val['seqlen_offset'])
