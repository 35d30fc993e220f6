"""Payload filters of ``VectorStore.search``: which points a search may return.

The reference searches Qdrant with ``filter: None`` (vector_memory_service/src/main.rs:280); the
conditions here are the subset of Qdrant's filter a caller of this store asks for first, evaluated
on the host against the ``PayloadStore`` into a row set and handed to the shard as a ``RowMask``
(index/shard.py): the search is exact over the rows that pass.
"""
from __future__ import annotations

import numpy as np

FILTER_FIELDS = ("original_document_id", "source_url", "model_name")


def _cond(m) -> tuple:
    """{field: value | [values]} -> ((field, (values...)), ...) in a canonical order."""
    if not m:
        return ()
    out = []
    for f in sorted(m):
        if f not in FILTER_FIELDS:
            raise ValueError(f"filter field must be one of {FILTER_FIELDS}, got {f!r}")
        v = m[f]
        vals = [v] if isinstance(v, str) or not hasattr(v, "__iter__") else list(v)
        out.append((f, tuple(sorted(set(vals), key=repr))))
    return tuple(out)


class Filter:
    """``must`` / ``must_not``: payload field -> a value or a list of values (any-of), over
    ``original_document_id``, ``source_url`` and ``model_name``.  ``point_ids``: only these points
    (Qdrant's ``has_id``).

    A row passes if it matches every ``must`` entry, no ``must_not`` entry and, with
    ``point_ids``, is one of those points.  A row without a stored payload never matches a
    ``must`` and always passes a ``must_not``."""

    __slots__ = ("must", "must_not", "point_ids")

    def __init__(self, must=None, must_not=None, point_ids=None):
        self.must = _cond(must)
        self.must_not = _cond(must_not)
        self.point_ids = None if point_ids is None else tuple(sorted(set(point_ids)))

    def key(self) -> tuple:
        """Hashable value of the filter (two filters with equal keys pass the same rows)."""
        return (self.must, self.must_not, self.point_ids)

    def __eq__(self, other):
        return isinstance(other, Filter) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def evaluate(self, payloads, n: int) -> np.ndarray:
        """The passing rows below ``n``: sorted int64 row numbers when ``must`` or ``point_ids``
        narrows the search, else a bool array of length ``n`` (``must_not`` alone passes nearly
        every row, payload or not)."""
        keep = None
        for f, vals in self.must:
            hit = set()
            for v in vals:
                hit |= payloads.rows_with(f, v)
            keep = hit if keep is None else keep & hit
        if self.point_ids is not None:
            ids = {payloads.id_to_row[p] for p in self.point_ids if p in payloads.id_to_row}
            keep = ids if keep is None else keep & ids
        drop = set()
        for f, vals in self.must_not:
            for v in vals:
                drop |= payloads.rows_with(f, v)
        if keep is not None:
            return np.fromiter(sorted(r for r in keep - drop if r < n), dtype=np.int64)
        allow = np.ones(n, dtype=bool)
        gone = np.fromiter((r for r in drop if r < n), dtype=np.int64)
        allow[gone] = False
        return allow
