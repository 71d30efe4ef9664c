"""Pinned host memory around the update graphs (algorithm/graphed_update.py): the staging slot a pass's inputs travel through and the
log's way back.  Every copy here is an ordinary stream-ordered copy around the replay, not a node of it, so the host never waits for
the pass it has just launched: it prepares pass i + 1 while pass i runs."""
import torch

from ..models.flash_attention.TransformerFlashAttention import PackedSeqs
from ..utility.deferred_log import DeferredLog
from .graph_policy import slot_runs

RING = 3                                              # the host may be this many passes (the log: this many steps) ahead of the device


class PassStaging:
    """The pinned slot of a pass: the plan, the selection words of randomised loss masks, the REDQ subset, the AdamW factors and - for
    attention layers - the host halves of the two sequence tables (the batch and its one-slot shift), all behind ONE event.  `take`
    hands out the next of RING slots and waits for its event if the slot was used (its copies of RING passes ago have long run);
    `release` records the event behind the pass.  The sequence tables' static device halves live here too: they grow with their
    host halves (`put_seqs`)."""

    def __init__(self, plan_capacity, sel_capacity, subset_size, device):
        self.device = device
        self._ring = [dict(plan=torch.empty((plan_capacity, 4), dtype=torch.int32, pin_memory=True),
                           sub=torch.empty(subset_size, dtype=torch.int32, pin_memory=True),
                           bc=torch.empty(4, dtype=torch.float32, pin_memory=True),
                           sel=torch.empty(sel_capacity, dtype=torch.int32, pin_memory=True) if sel_capacity else None,
                           idx=None, cu=None, evt=torch.cuda.Event(), used=False) for _ in range(RING)]
        self._turn = 0
        self.slot = self._ring[0]
        self._seq = None                              # capacities and static device halves of the sequence tables
        self.seq_now = None                           # per description: (tokens, cu entries, longest sequence, table, padded) of this pass

    def take(self):
        slot = self.slot = self._ring[self._turn % RING]
        self._turn += 1
        if slot['used']:
            slot['evt'].synchronize()
        return slot

    def release(self):
        self.slot['evt'].record()
        self.slot['used'] = True

    def put_seqs(self, built, padded):
        """Both descriptions `built` ([(idx, cu, longest, table)]) through the slot taken into the static device tables.  -> True if
        the tables had to grow: every recorded graph holds the old addresses and must be dropped (the device is synchronised once -
        queued copies may still read the old blocks)."""
        n_idx, n_cu = max(b[0].size for b in built), max(b[1].size for b in built)
        sq, grown = self._seq, False
        if sq is None or sq['cap_idx'] < n_idx or sq['cap_cu'] < n_cu:
            ci, cc = max(2 * n_idx, 1024), max(2 * n_cu, 64)
            torch.cuda.synchronize(self.device)
            for slot in self._ring:
                slot['idx'] = [torch.empty(ci, dtype=torch.int64, pin_memory=True) for _ in range(2)]
                slot['cu'] = [torch.empty(cc, dtype=torch.int32, pin_memory=True) for _ in range(2)]
            sq = self._seq = dict(cap_idx=ci, cap_cu=cc, idx_dev=[torch.empty(ci, dtype=torch.int64, device=self.device) for _ in range(2)],
                                  cu_dev=[torch.empty(cc, dtype=torch.int32, device=self.device) for _ in range(2)])
            grown = True
        slot = self.slot
        for i, (idx, cu, mx, tb) in enumerate(built):
            # staged with numpy (a plain memcpy): a torch CPU copy_ of > 32 768 elements opens an intra-op parallel region over all host threads,
            # which on a loaded host took 10-15 ms per call - longer than the replay it is meant to hide behind
            slot['idx'][i].numpy()[:idx.size] = idx
            slot['cu'][i].numpy()[:cu.size] = cu
            sq['idx_dev'][i][:idx.size].copy_(slot['idx'][i][:idx.size], non_blocking=True)
            sq['cu_dev'][i][:cu.size].copy_(slot['cu'][i][:cu.size], non_blocking=True)
        self.seq_now = [(b[0].size, b[1].size, b[2], b[3], padded) for b in built]
        return grown

    def packed_seqs(self):
        """Views of the static device tables as `put_seqs` last filled them; None before any."""
        sq = self._seq
        if sq is None:
            return None
        return [PackedSeqs.from_static(sq['idx_dev'][i][:n_idx], sq['cu_dev'][i][:n_cu], mx, tb, padded=padded)
                for i, (n_idx, n_cu, mx, tb, padded) in enumerate(self.seq_now)]


class UpdateLog:
    """The log scalars of the graphs.  Every key has a fixed slot in ONE static device buffer, handed out on the key's first appearance.
    A pass writes only its own keys (`write`: copy nodes of its graph, one per run of neighbouring slots), so the passes of a step
    merge on the device: a later pass overwrites an earlier one's keys, actor keys survive from the last pass that ran the actor
    step - what the eager loop's shared dict does.  ONE read-back per step (`read_back`), behind its last pass, into a pinned ring
    of its own turned once per step: with utd > RING a staging slot comes round again inside one step, and the log handed out by the
    step before is still unread then."""

    def __init__(self, capacity, device, log_cls=DeferredLog):
        self.log_cls = log_cls                        # the dict class `read_back` hands out
        self.dev = torch.zeros(capacity, dtype=torch.float32, device=device)
        self.slots = {}                               # key -> its slot in `dev`
        self._ring = [dict(log=torch.empty(capacity, dtype=torch.float32, pin_memory=True), evt=torch.cuda.Event(), handed=None)
                      for _ in range(RING)]
        self._turn = 0

    def write(self, keys, packed):
        slots = [self.slots.setdefault(k, len(self.slots)) for k in keys]
        if len(self.slots) > self.dev.numel():
            raise RuntimeError(f'GraphedUpdate: more than {self.dev.numel()} logged device scalars')
        for i, j in slot_runs(slots):
            self.dev[slots[i]:slots[i] + j - i].copy_(packed[i:j])

    def read_back(self, keys, items):
        """The whole slot buffer into this step's pinned block -> the DeferredLog of `keys` - the union of the keys the step's passes
        wrote, so a step without an actor step shows no actor key of an earlier one - and the host entries `items`."""
        ring = self._ring[self._turn % RING]
        self._turn += 1
        if ring['handed'] is not None:                # the log handed out RING steps ago is read out before its block is reused
            ring['handed'].resolve()
        n = len(self.slots)
        ring['log'][:n].copy_(self.dev[:n], non_blocking=True)
        ring['evt'].record()
        ring['handed'] = self.log_cls(keys, ring['log'][:n], ring['evt'], items, index=[self.slots[k] for k in keys])
        return ring['handed']
