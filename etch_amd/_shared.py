"""Tensors built once and handed to many callers (occupancy ones, identity sample tables, offset tensors, index tables).  A caller holds the cached
object itself, so Shared remembers the `_version` each tensor was built at and rebuilds an entry whose version has moved: torch bumps it on every
in-place op, also through a view (views share their base's counter), _lib.wrote() for writes through raw pointers.  An integer compare, no launch."""
import torch


class Shared:
    def __init__(self, limit=None):
        self.limit = limit        # more entries than this: cleared before the next insert (shapes come and go; the working set is small)
        self._d = {}

    def get(self, key, make, fill=None, keep=None):
        """The tensor of `key`, built by make() under no_grad on a miss or when the cached one was written to since.  fill: the value make() fills
        the tensor with, for constant_value().  keep: tensors whose addresses are part of `key`, held so that the addresses stay unique."""
        hit = self._d.get(key)
        if hit is not None and hit[0]._version == hit[1]:
            return hit[0]
        if hit is None and self.limit is not None and len(self._d) > self.limit:
            self._d.clear()
        with torch.no_grad():
            t = make()
        if fill is not None:
            t._shared_fill = (fill, t._version)
        self._d[key] = (t, t._version, keep)
        return t

    @staticmethod
    def constant_value(t):
        """The value `t` was registered as being filled with (get(..., fill=)); None for any other tensor, a view included, and once `t` was written to."""
        tag = getattr(t, "_shared_fill", None)
        return tag[0] if tag is not None and tag[1] == t._version else None


constant_value = Shared.constant_value
