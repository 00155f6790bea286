"""Per-step derived state of the convolutions, keyed by raw device addresses: the copies made of a weight (its
transpose, its fragment-major form, its 16-bit form) and the zeroed gradient arena.

An address says nothing about WHOSE it is: a model that is garbage-collected leaves its records behind and the allocator
hands the freed addresses to the next model's tensors -- same shape, same version counter.  So ONE rule decides whether
a copy may be used (Registry.lookup), and every record names its owner.

Pure Python on tensor attributes (data_ptr(), _version, shape): no library call, runs on CPU tensors.
"""
import collections
import weakref

WT, FRAG, LOWP, HEAD, WT16 = "wt", "frag", "lowp", "head", "wt16"
# kind -> what a lookup must expect of the copy:
#   WT    W^T [Cin][R][S][Cout] of a weight         (scaled: eval-BatchNorm scale folded in or not, shape of the weight)
#   FRAG  fragment-major copy of a 1x1 matrix       (rows, cols)
#   LOWP  16-bit copy, flat or shaped like the source   (dtype, numel)
#   HEAD  re-laid-out 16-bit operand of a head layer on 16-bit crops (head16.py), possibly stacked from several tensors and
#         with an fp32 bias next to it; the record is the FIRST tensor's   (what, dtype, ((address, version) of each
#         further tensor))
#   WT16  16-bit data-gradient operand of a layer on 16-bit activations (grad16.py): W^T [Cin][R][S][Cout] with the taps
#         flipped and the eval-BatchNorm scale folded in, rounded once   (dtype, the fold's key: conv._fold_key)

WITH_SOURCE = object()      # the version of a record whose source is itself a copy (a W^T tensor): the batched transpose
                            # rewrites it in place without a version bump; its copies are dropped when it is republished
MAX_PINNED = 4096


class Record(object):
    """owner: a weak reference to the tensor that owns the address.  pin: None for a plan-owned source (a parameter, a
    W^T tensor a plan holds); for a temporary the tensor itself, so that its address cannot be reused while the record
    exists.  version: the owner's version counter the copies were made from, or WITH_SOURCE.  copies: kind -> (copy,
    expectation)."""
    __slots__ = ("owner", "pin", "version", "copies")

    def __init__(self, source, version, pinned):
        self.owner = weakref.ref(source)
        self.pin = source if pinned else None
        self.version = version
        self.copies = {}


class Registry(object):
    """table: source address -> Record.  pinned: the addresses of the temporaries' records.  epoch: how often the table
    was cleared."""

    def __init__(self):
        self.table, self.pinned, self.epoch = {}, set(), 0

    def _speaks_of(self, rec, key, w):
        """THE rule: the record's owner is alive and still at that address, and the copies were made from the version
        `w` has (or are republished with their source)."""
        if rec.version is not WITH_SOURCE and rec.version != w._version:
            return False
        owner = rec.owner()
        return owner is not None and (owner is w or owner.data_ptr() == key)

    def lookup(self, w, kind, expect):
        """The copy of `w` of that kind, or None.  `w` is the owner or an alias of it (same address, same version
        counter: a saved tensor in backward, a permuted view of a channels-last parameter)."""
        key = w.data_ptr()
        rec = self.table.get(key)
        if rec is None:
            return None
        entry = rec.copies.get(kind)
        if entry is None or entry[1] != expect or not self._speaks_of(rec, key, w):
            return None
        return entry[0]

    def publish(self, source, kind, copy, expect, pinned=False, with_source=False):
        """`copy` was just made from `source` as it is now.  A record of other contents at that address (another owner,
        another version) is replaced with all its copies.  A new W^T voids what was derived from the tensor it lives in.
        `pinned` and `with_source` say how to open a record; a record that already speaks of `source` is added to."""
        key = source.data_ptr()
        rec = self.table.get(key)
        if rec is None or not self._speaks_of(rec, key, source) or (with_source and rec.version is not WITH_SOURCE):
            rec = self.table[key] = Record(source, WITH_SOURCE if with_source else source._version, pinned)
            (self.pinned.add if pinned else self.pinned.discard)(key)
        rec.copies[kind] = (copy, expect)
        if kind == WT:
            self.table.pop(copy.data_ptr(), None)
            self.pinned.discard(copy.data_ptr())

    def having(self, kind):
        """[(address, record)] of the records that hold a copy of that kind."""
        return [(k, r) for k, r in self.table.items() if kind in r.copies]

    def sweep(self):
        """Drop the records whose owner is gone -- and then those of the W^T tensors that only such a record kept alive."""
        while True:
            dead = [k for k, r in self.table.items() if r.owner() is None]
            if not dead:
                return
            for k in dead:
                del self.table[k]

    def drop_pinned(self):
        """Release the temporaries: a training step does so once its weights are republished, so that those of one
        step (and the fp32 sources they pin) do not pile up behind the next.  Plan-owned records stay."""
        for k in self.pinned:
            self.table.pop(k, None)
        self.pinned.clear()

    def bound(self):
        """An inference loop republishes nothing: past MAX_PINNED temporaries they all go."""
        if len(self.pinned) > MAX_PINNED:
            self.drop_pinned()

    def clear(self):
        """Everything published so far is void; plans compare `epoch` with the one they last published in."""
        self.table.clear()
        self.pinned.clear()
        self.epoch += 1


Slot = collections.namedtuple("Slot", "offset numel owner partner")      # owner: weak reference to the parameter


class GradArena(object):
    """This step's zero-filled gradient buffer and the slots laid out in it: key ("dw" | "db" | "bn", address) -> Slot."""

    def __init__(self):
        self.buf, self.slots, self.used = None, {}, set()

    def arm(self, slots, buf):
        """buf None: the slots are known but there is no cleared buffer this step (take gives nothing)."""
        self.buf, self.slots, self.used = buf, slots, set()

    def disarm(self):
        self.buf = None

    def take(self, key, numel, partner=None):
        """(slot, first): the slot reserved for `key` in this step's arena (zeroed at the start of the step) and
        whether this is its first use in the step.  A layer applied several times per step (the RPN on 5 levels, the
        feature extractor on small and big boxes) ACCUMULATES all its gradient contributions in the one slot -- the
        kernels add with atomics anyway -- and hands the slot to autograd only the first time (later calls return no
        gradient for the parameter), so there is no per-use buffer, fill and add.  (None, False): no slot."""
        slot = self.slots.get(key)
        if slot is None or self.buf is None or slot.numel != numel:
            return None, False
        owner = slot.owner()
        if owner is None or owner.data_ptr() != key[1]:
            return None, False        # the model this arena belongs to is gone and its address was reused
        if partner is not None and slot.partner is not None and slot.partner != partner:
            return None, False        # a BatchNorm block laid out for another convolution's bias: private buffers instead
        first = key not in self.used
        self.used.add(key)
        return self.buf[slot.offset:slot.offset + numel], first
