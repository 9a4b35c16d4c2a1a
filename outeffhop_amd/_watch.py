"""One answer to "did a tensor change?" for every host-side cache that bakes tensor values in (weight forms, quantiser grids, the INT8
layer plan, the packed gate and fused q/k/v weights).  A watch is built from SLOTS `(holder_dict, name)` - `(m._parameters, "weight")`,
`(qz._buffers, "_delta")` - and keeps, per slot, the tensor OBJECT (None is a legal value), its version counter and its storage address.
It holds the tensors: the address of a held object is not handed to another tensor, so - unlike a key of `(data_ptr, _version)` pairs
looked up at call time - two different tensors can never look alike.  The object catches a slot rebound to another tensor (a buffer
assigned by `set_quant_range`, `.to()`), the version an in-place write, the address `p.data = other` (object and version stay)."""
from __future__ import annotations


class TensorWatch:
    __slots__ = ("entries",)

    def __init__(self, slots):
        self.entries = []
        for holder, name in slots:
            t = holder.get(name)
            self.entries.append((holder, name, t, None if t is None else t._version, None if t is None else t.data_ptr()))

    def unchanged(self) -> bool:
        for holder, name, t, version, address in self.entries:
            cur = holder.get(name)
            if cur is not t or (t is not None and (t._version != version or t.data_ptr() != address)):
                return False
        return True

    def tensors(self):
        return (e[2] for e in self.entries if e[2] is not None)


def cached(store: dict, name: str, key, slots, build):
    """The value kept as store[name] = (key, watch, value), rebuilt by `build()` when `key` - the plain, non-tensor part: flags, numbers,
    the holder modules (compared by identity; never a tensor) - differs or a watched slot changed.  `slots()` lists the slots; it is
    called on a rebuild only."""
    hit = store.get(name)
    if hit is None or hit[0] != key or not hit[1].unchanged():
        hit = (key, TensorWatch(slots()), build())
        store[name] = hit
    return hit[2]
