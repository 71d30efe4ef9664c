import torch


class DeferredLog(dict):
    """The update's log dict.  Host-side entries are plain items; the device scalars travel in one asynchronous copy into
    pinned memory and become floats on first access (`resolve()`), so a caller that does not read them - a training loop
    logging every n-th update, bench.py - never stalls the launch queue on the update it has just enqueued."""

    TUPLE_KEYS = ('actor_loss',)

    def __init__(self, keys, buf, event, host_items=(), index=None):
        """`buf`: host tensor the scalars named by `keys` arrive in, readable once `event` (None: at once) has passed; `index`: where in
        `buf` each key's scalar sits (None: in the order of `keys`) - a buffer with a fixed slot per key, of which this log names some."""
        super().__init__()
        self._keys, self._buf, self._event, self._index = keys, buf, event, index
        self.set_host(host_items)

    @classmethod
    def from_packed(cls, keys, packed, pinned, host_items=()):
        """The log of the scalars `packed` on the device: ONE device->host copy, asynchronous into pinned memory if `pinned`."""
        if not pinned:
            return cls(keys, packed.detach().cpu(), None, host_items)
        buf = torch.empty(packed.shape, dtype=packed.dtype, pin_memory=True)
        buf.copy_(packed, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        return cls(keys, buf, event, host_items)

    def set_host(self, items):
        dict.update(self, items)

    def resolve(self):
        if self._keys is not None:
            if self._event is not None:
                self._event.synchronize()
            got = self._buf.tolist()
            vals = dict(zip(self._keys, got if self._index is None else [got[i] for i in self._index]))
            for k in self.TUPLE_KEYS:
                if k in vals:
                    vals[k] = (vals[k],)                        # a 1-tuple upstream (reference :430); kept
            self._keys = None
            pending = dict(self)                                # host entries override / follow, as in the reference order
            dict.clear(self)
            dict.update(self, vals)
            dict.update(self, pending)
        return self

    def __getitem__(self, k):
        if not dict.__contains__(self, k):
            self.resolve()
        return dict.__getitem__(self, k)

    def get(self, k, default=None):
        if not dict.__contains__(self, k):
            self.resolve()
        return dict.get(self, k, default)

    def __contains__(self, k):
        return dict.__contains__(self, k) or dict.__contains__(self.resolve(), k)

    def __iter__(self):
        return dict.__iter__(self.resolve())

    def __len__(self):
        return dict.__len__(self.resolve())

    def keys(self):
        return dict.keys(self.resolve())

    def items(self):
        return dict.items(self.resolve())

    def values(self):
        return dict.values(self.resolve())

    def __repr__(self):
        return dict.__repr__(self.resolve())


class ScalarLog(DeferredLog):
    """The log of the memoryless trainers: every entry a float, `actor_loss` included (reference sac_mlp_redq_ensemble_q.py:189-200)."""
    TUPLE_KEYS = ()
