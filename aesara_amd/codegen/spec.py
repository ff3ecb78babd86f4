"""Common base of the kernel specs: ONE declaration of what determines a kernel's source.

A spec lists that once (``source_fields``).  The digest that names the kernel is a SHA-256 over the
JSON of the list; the signature that memoises the digest is derived from the same list, so the two
cannot drift apart (a field that changed the source but not the signature would hand out the wrong
kernel under the right name).
"""
from __future__ import annotations

import hashlib
import json

# Computing the digest for every launch of every call cost ~50 us of Python per step.  The scalar
# programs are long-lived objects owned by the plan / the fused steps, so their identity plus the
# (small, hashable) layout fields memoises it; the memo keeps the objects alive so ids stay valid.
_DIGEST_MEMO = {}


def _signature(x, scalars):
    """Hashable form of ``x`` with every scalar program (a dict with "nodes" and "out") replaced by
    its identity; the programs met are appended to ``scalars``."""
    if isinstance(x, dict):
        if "nodes" in x and "out" in x:
            scalars.append(x)
            return ("@", id(x))
        # (in insertion order: equal dicts built in another order only miss the memo)
        return tuple([(k, _signature(v, scalars)) for k, v in x.items()])
    if isinstance(x, (list, tuple)):
        return tuple([_signature(v, scalars) for v in x])
    return x


class Spec:
    """Everything that determines the generated source of one kernel.  Subclasses give
    ``source_fields()`` (JSON-serialisable; scalar programs as the plan's own dict objects) and
    ``generate()`` -> (source, kernel names); the kernel cache needs ``key()`` and ``generate()``."""

    def digest(self):
        """24 hex digits of the SHA-256 over the source fields (part of the kernel's name)."""
        fields = self.source_fields()
        scalars = []
        sig = _signature(fields, scalars)
        hit = _DIGEST_MEMO.get(sig)
        if hit is None:
            if len(_DIGEST_MEMO) > 8192:       # ad-hoc scalar programs (casts) come and go
                _DIGEST_MEMO.clear()
            blob = json.dumps(fields, sort_keys=True)
            hit = _DIGEST_MEMO[sig] = (hashlib.sha256(blob.encode()).hexdigest()[:24], scalars)
        return hit[0]

    def key(self):
        """Key of the spec in the kernel cache."""
        return self.digest()
