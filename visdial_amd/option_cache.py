"""Host index of the answer-encoding cache (decoder disc, evaluation only).

The discriminative decoder's encoding of a candidate answer depends on the candidate's tokens, on To (the option LSTM has no
maskZero: trailing pads are zero-vector inputs that still advance the state) and on the weights alone (decoders/disc.lua:4-15).
While the weights stand still, the final hidden state of every distinct (token row, To) can therefore be kept in a device table
[rows x H] and the option recurrence run over the rows not seen before only.  This class is the host half: it maps candidate
rows to table rows.  Pure numpy, no device: the operator-level host (visdial_amd/model.py) drives it, the model-level runtime
keeps the same policy in C++ (csrc/rt_core.h OptionCache), and the CPU tests run it over the dataloader's real batches.

    slots, miss_rows = index.resolve(rows)     # rows [n x To] int32
    ... encode miss_rows, write their final h to table rows index.count .. index.count + len(miss_rows) - 1 ...
    index.commit()

`slots[r] >= 0` is the table slot of row r: a committed entry, or -- for the i-th miss, while it fits -- the slot `count + i` it
will own once committed.  When the table is full nothing more is inserted: the i-th miss then resolves to `-(1 + i)`, "row i of
miss_rows, not stored" (`gather_rows` turns both forms into rows of a table whose tail holds this batch's misses).  `resolve`
inserts nothing: a batch that is resolved and then replaced or never stepped leaves no entry that points at an unfilled slot.
`commit` inserts the misses of the last `resolve` that fit; it is called when their fill has been enqueued.
"""
import numpy as np


DEFAULT_ROWS = 262144        # = VD_OPTION_CACHE_DEFAULT_ROWS (csrc/rt_core.h): 512 MiB of fp32 state at H = 512


class OptionIndex(object):
    def __init__(self, capacity=DEFAULT_ROWS):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError('OptionIndex: capacity must be at least 1 row, got %d' % capacity)
        self.capacity = capacity
        self.To = None
        self._slot = {}          # key bytes (the row's int32 tokens; To = the key's length) -> slot
        self._pending = None     # (keys of the misses that fit, count they were numbered from)
        self.flushes = 0

    @property
    def count(self):
        return len(self._slot)

    def flush(self):
        """forget every entry (the weights changed); the slots are handed out again from 0"""
        self._slot = {}
        self._pending = None
        self.flushes += 1

    def resolve(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        if rows.ndim != 2:
            raise ValueError('OptionIndex.resolve: rows must be [n x To], got shape %s' % (rows.shape,))
        n, To = rows.shape
        if self.To != To:        # To is part of the key: the same tokens at another To are another encoding
            if self._slot:
                self.flush()
            self.To = To
        count, fit = self.count, self.capacity - self.count
        slots = np.empty(n, np.int32)
        if n == 0:
            self._pending = ([], count)
            return slots, rows[:0]
        # distinct rows of the batch first (opaque byte strings, like Model.prepare_inputs), in order of first occurrence
        key = rows.view(np.dtype((np.void, 4 * To))).reshape(-1)
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        order = np.argsort(first, kind='stable')
        uslot = np.empty(first.shape[0], np.int64)
        miss_first, miss_keys = [], []
        for u in order:
            k = rows[first[u]].tobytes()
            s = self._slot.get(k)
            if s is None:
                i = len(miss_first)
                s = count + i if i < fit else -(1 + i)
                miss_first.append(first[u])
                if i < fit:
                    miss_keys.append(k)
            uslot[u] = s
        slots[:] = uslot[inv.reshape(-1)]
        self._pending = (miss_keys, count)
        return slots, rows[np.asarray(miss_first, np.int64)]

    def commit(self):
        """insert the misses of the last resolve() that fit; returns how many"""
        if self._pending is None:
            return 0
        keys, count = self._pending
        self._pending = None
        if count != self.count:
            raise RuntimeError('OptionIndex.commit: the index changed since resolve() (%d -> %d entries)' % (count, self.count))
        for i, k in enumerate(keys):
            self._slot[k] = count + i
        return len(keys)

    @staticmethod
    def gather_rows(slots, base):
        """table row of every resolved row, for a table whose rows [base, base + misses) hold the batch's misses (base = `count`
        at resolve time): a slot is its own row, an unstored miss -(1 + i) lies at base + i"""
        slots = np.asarray(slots, np.int64)
        return np.where(slots >= 0, slots, base - slots - 1).astype(np.int32)
