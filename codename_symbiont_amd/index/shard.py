"""In-HBM brute-force cosine index shard (the Qdrant replacement of vector_memory_service).

Reference behaviour (services/vector_memory_service/src/main.rs):
* collection ``symbiont_document_embeddings``, Distance::Cosine (:19-22, :36): scores are cosine
  similarities in [-1, 1], results sorted descending, fewer than k if the collection is small;
* upsert one point per sentence with a fresh UUIDv4 id and a 6-field payload (:142-177).

Layout here: one contiguous bf16 slab ``rows[capacity_pad, D]`` of UNIT vectors (cosine ==
dot product), sized up front for the shard (288 GB of HBM per MI355X holds 100M x 384 bf16 =
76.8 GB with room to spare), rows appended in place; the fused HIP scan (``_hip.index_scan``)
streams the slab once per query batch and never materialises scores.  Point ids and payloads
live host-side in a sparse ``PayloadStore`` keyed by row (rows without a point cost nothing).
"""
from __future__ import annotations

import collections
import math
import os
import threading
from dataclasses import dataclass

import numpy as np
import torch

# (neither module loads an extension when imported; the masked routes, a few launches per search,
# use these names without a per-call import)
from ..ops import kernels as K
from ..ops._ext import hip, stream_handle
from ..ops.kernels import MASK_GROUPS   # masks one grouped scan carries

TILE_ROWS = 64  # scan tile: 2 MFMA sub-tiles per barrier interval


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def dedupe_last(point_ids) -> list[int]:
    """Input positions that survive a batch upsert: the LAST occurrence of each point id, in
    input order."""
    last = {pid: i for i, pid in enumerate(point_ids)}
    return sorted(last.values())


@dataclass
class Payload:
    original_document_id: str = ""
    source_url: str = ""
    sentence_text: str = ""
    sentence_order: int = 0
    model_name: str = ""
    processed_at_ms: int = 0


class PayloadStore:
    """Host store: row -> (point id, payload fields), SPARSE -- only rows that carry a point id
    or a payload are held (dicts keyed by row).  Rows without payload (synthetic benchmark rows,
    often the bulk of a 100M-row shard) cost nothing here and decode to the reference's defaults
    ("" / 0, main.rs:337-390).  A dense layout kept 7 Python lists of n slots: 560 MB of list
    pointers per 10M rows, traversed by every full GC pass of the service process (the e2e
    benchmark's ~100 ms tail).

    Filtered searches (index/filter.py) need value -> rows for the filterable fields.  That index
    is built lazily, per field, by the first filter that names the field, and kept current by
    ``set`` and ``truncate`` from then on: a dict of row sets over 100M payload rows is gigabytes
    of small objects for the same GC passes to walk, so a store that is never filtered (the
    service as it runs today) pays nothing for it."""

    FIELDS = ("original_document_id", "source_url", "sentence_text", "sentence_order",
              "model_name", "processed_at_ms")

    def __init__(self):
        self.n = 0
        self.point_ids: dict[int, str] = {}          # row -> point id
        self.fields: dict[int, tuple] = {}           # row -> payload field tuple (FIELDS order)
        self.id_to_row: dict[str, int] = {}
        # rows whose point id / payload changed since the last snapshot cut (index/persist.py),
        # recorded only while a persister tracks this store
        self.track = False
        self.dirty: set[int] = set()
        # field -> value -> rows, only for fields some filter has named (rows_with)
        self._by_value: dict[str, dict[object, set[int]]] = {}

    def _field_value(self, t: tuple, field: str):
        v = t[self.FIELDS.index(field)]
        return "" if v is None else v

    def rows_with(self, field: str, value) -> set[int]:
        """Rows whose stored payload has ``field`` == ``value`` (the field's index is built on
        its first use; do not modify the returned set)."""
        idx = self._by_value.get(field)
        if idx is None:
            idx = {}
            for row, t in self.fields.items():
                idx.setdefault(self._field_value(t, field), set()).add(row)
            self._by_value[field] = idx
        return idx.get(value, set())

    def _unindex(self, row: int) -> None:
        t = self.fields.get(row)
        if t is None:
            return
        for field, idx in self._by_value.items():
            v = self._field_value(t, field)
            rows = idx.get(v)
            if rows is not None:
                rows.discard(row)
                if not rows:
                    del idx[v]

    def __len__(self):
        return self.n

    def extend_empty(self, n: int) -> None:
        self.n += n

    def set(self, row: int, point_id: str | None, payload: Payload | None) -> None:
        if not 0 <= row < self.n:
            raise IndexError(f"row {row} outside the store ({self.n} rows)")
        old = self.point_ids.pop(row, None)
        if old is not None and self.id_to_row.get(old) == row:
            del self.id_to_row[old]
        if point_id is not None:
            self.point_ids[row] = point_id
            self.id_to_row[point_id] = row
        if self._by_value:
            self._unindex(row)
        if payload is not None:
            t = self.fields[row] = tuple(getattr(payload, f) for f in self.FIELDS)
            for field, idx in self._by_value.items():
                idx.setdefault(self._field_value(t, field), set()).add(row)
        else:
            self.fields.pop(row, None)
        if self.track:
            self.dirty.add(row)

    def remove(self, row: int) -> None:
        """Forget the row's point id, payload and value-index entries (a deleted point); the row
        is marked dirty, so the next snapshot's payload delta records it as empty."""
        self.set(row, None, None)

    def get(self, row: int) -> tuple[str | None, Payload]:
        t = self.fields.get(row)
        if t is None:
            return self.point_ids.get(row), Payload()
        vals = {}
        for f, v in zip(self.FIELDS, t):
            if v is None:
                v = 0 if f in ("sentence_order", "processed_at_ms") else ""
            vals[f] = v
        return self.point_ids.get(row), Payload(**vals)

    def truncate(self, n: int) -> None:
        """Forget rows >= n."""
        if n >= self.n:
            return
        for r in [r for r in self.point_ids if r >= n]:
            pid = self.point_ids.pop(r)
            if self.id_to_row.get(pid) == r:
                del self.id_to_row[pid]
        for r in [r for r in self.fields if r >= n]:
            if self._by_value:
                self._unindex(r)
            del self.fields[r]
        self.dirty = {r for r in self.dirty if r < n}
        self.n = n

    def remap(self, new_row_of, n: int) -> None:
        """Renumber the rows (a compaction): ``new_row_of`` maps an int64 array of old rows to
        their new rows, ``n`` is the new row count.  Point ids and payloads follow their rows;
        the value index is dropped (the next filter rebuilds it, rows_with) and ``dirty`` is
        emptied: the caller makes the next snapshot a full one."""
        def moved(d: dict) -> dict:
            if not d:
                return {}
            old = np.fromiter(d.keys(), dtype=np.int64, count=len(d))
            return dict(zip(new_row_of(old).tolist(), d.values()))

        self.point_ids = moved(self.point_ids)
        self.fields = moved(self.fields)
        self.id_to_row = {pid: r for r, pid in self.point_ids.items()}
        self._by_value = {}
        self.dirty = set()
        self.n = int(n)


FP8_SCALE = K.FP8_SCALE  # 256.0: unit vectors -> |S x_i| <= 256 < 448 (e4m3 max)


def resolve_prune(mode: str | None, dtype: str = "bf16", dim: int = 384,
                  prefilter: str | None = None, device=None) -> str | None:
    """``SYMB_INDEX_PRUNE``: "auto" (default) = the exact int8-pruned search wherever it applies
    (384- or 768-wide bf16 shards without an fp8 prefilter, on a GPU), "i8" = require it, "" / "none" =
    plain scan.  ``device``: the shard's device; "auto" on a CPU shard is None (the CPU backend
    searches by matmul and would only pay for the int8 image on every write)."""
    mode = (mode or "").strip().lower()
    if mode in ("", "none", "0", "off"):
        return None
    if mode == "auto":
        if device is not None and torch.device(device).type != "cuda":
            return None
        return "i8" if (dtype == "bf16" and dim in AUTO_PRUNE_DIMS and not prefilter) else None
    return mode


FP8_DIMS = (256, 384, 512, 768, 1024)   # row widths the fp8 scan kernel takes
MQ_DIMS = (384, 768, 1024)              # ... the emitting bf16 scan (index_mq.hip)
PRUNE_DIMS = (384, 768, 1024)           # ... the int8-pruned scan (1024: stream scan only)
AUTO_PRUNE_DIMS = (384, 768)            # ... where SYMB_INDEX_PRUNE=auto takes it
SPLIT_DIMS = (384, 768)                 # ... its split image (calibrate_prune)
# ... where a shard takes the split image by itself (SYMB_I8_SPLIT=auto, the write-time triggers);
# at 768 only an explicit calibrate_prune() or SYMB_I8_SPLIT=on does (profiles/r7_split768/)
AUTO_SPLIT_DIMS = (384,)
# leading components the split image keeps as fp16, per row width (768: 13 k-steps of 64 bytes;
# 128 would bound slightly tighter for 8 % more image bytes, profiles/r7_split768/)
SPLIT_HEAVY = {384: 64, 768: 64}
MX4_DIMS = (384, 768, 1024)             # ... the MX-fp4 first tier (384-only on the LDS-ring scan)
# widths of the streaming pruning scan (index_stream.hip): fragment-major int8 / MX-fp4 images,
# one wave per SIMD, no LDS ring (SYMB_PRUNE_STREAM=0: the round-4 LDS-ring scan, index_i8.hip,
# 384 / 768 only)
STREAM_DIMS = (384, 768, 1024)
STREAM_SUB = 32                         # rows per sub-tile record of the stream images
# ... where the int8 tier runs the LDS-ring scan (index_i8.hip) beside the stream fp4 tier: 100M x
# 768 held-out 21.6 ms against 25.4 ms for the LDS-query stream form (profiles/r6_768/)
I8_RING_DIMS = (768,)


FILTER_DIMS = (384, 768, 1024)          # ... the masked list scan (index_filter.hip)
FILTER_FP8_DIMS = (256, 384, 512, 768, 1024)   # ... its e4m3 form (index_filter_fp8.hip)
FILTER_LARGE_K_DIMS = (384, 768, 1024)  # ... the masked emitting scan (index_mq_filter.hip)
FILTER_LARGE_K_FP8_DIMS = FILTER_FP8_DIMS      # ... its e4m3 form (index_emit_fp8.hip)


def filter_large_k_threshold(cand_s: torch.Tensor, k: int, margin: float) -> torch.Tensor:
    """Per-query threshold of the masked large-k search from a seed pass's candidate block
    ``cand_s`` [NQ, m]: the k-th largest FINITE entry less ``margin``, -inf where fewer than k
    entries are finite.  Every finite entry is a distinct allowed row's real score, so the k-th
    best of them is a lower bound on the k-th best allowed score."""
    NQ, m = cand_s.shape
    if m < k:
        return torch.full((NQ,), -math.inf, dtype=torch.float32, device=cand_s.device)
    s = torch.where(torch.isfinite(cand_s), cand_s, torch.full_like(cand_s, -math.inf))
    kth = torch.topk(s, k, dim=1).values[:, k - 1]
    return (kth - margin).float().contiguous()


def filter_large_k_threshold_ulp(cand_s: torch.Tensor, k: int) -> torch.Tensor:
    """``filter_large_k_threshold`` for a seed pass and an emitting scan that score a row bit for
    bit alike (the fp8 pair, which shares one MFMA chain): the k-th largest FINITE entry moved one
    ulp towards -inf, so the emitting scan's strict ``score > T`` keeps every row scoring at
    least that entry; -inf where fewer than k entries are finite.  NaN entries (a gated-off seed
    pass leaves its workspace unwritten) count as missing, and the result is never NaN."""
    kth = filter_large_k_threshold(cand_s, k, 0.0)
    return torch.nextafter(kth, torch.full_like(kth, -math.inf)).contiguous()


def _pack_bits(allow: torch.Tensor, n_words: int) -> torch.Tensor:
    """bool [n <= 64 n_words] -> uint8 [8 n_words]: bit r % 8 of byte r // 8 = allow[r]
    (numpy.packbits(bitorder="little")), zero-padded to whole 64-bit words."""
    pad = torch.zeros(n_words * 64, dtype=torch.uint8, device=allow.device)
    pad[:allow.numel()] = allow
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=allow.device)
    return (pad.view(-1, 8) * w).sum(1, dtype=torch.uint8)


_POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def _unpack_bits(packed: torch.Tensor) -> torch.Tensor:
    """uint8 [m] -> bool [8 m] (the inverse of _pack_bits)."""
    sh = torch.arange(8, dtype=torch.uint8, device=packed.device)
    return ((packed[:, None] >> sh) & 1).bool().reshape(-1)


class RowMask:
    """The rows of one shard a search may return, built once by ``HbmIndexShard.make_mask`` and
    reused by every search under the same filter.

    ``bits``: packed uint8 on the shard's device, one bit per row, little-endian within a byte,
    whole 64-bit words; bits at or past ``visible`` are clear.  ``visible``: the shard's visible
    rows when the mask was built -- rows appended later are disallowed under it.  ``tiles`` /
    ``n_live`` (shards the masked scan serves, else None): the ascending 64-row tiles that hold
    an allowed row and their count, device tensors from ``filter_tiles``.  ``dead_gen``: the
    shard's delete generation when the mask was built (tombstoned rows are cleared in it); a
    search refuses a mask from before a later delete, which could return a deleted row."""

    __slots__ = ("bits", "visible", "tiles", "n_live", "dead_gen")

    def __init__(self, bits: torch.Tensor, visible: int, tiles=None, n_live=None,
                 dead_gen: int = 0):
        self.bits, self.visible, self.tiles, self.n_live = bits, int(visible), tiles, n_live
        self.dead_gen = int(dead_gen)

    @property
    def words(self) -> torch.Tensor:
        return self.bits.view(torch.int64)

    def bool_rows(self, s: int, e: int) -> torch.Tensor:
        """bool [e - s]: rows [s, e) allowed (rows past the mask are not)."""
        b0 = s // 8
        u = _unpack_bits(self.bits[b0:(e + 7) // 8])[s - b0 * 8:e - b0 * 8]
        if u.numel() < e - s:
            u = torch.cat([u, torch.zeros(e - s - u.numel(), dtype=torch.bool, device=u.device)])
        return u

    def count(self) -> int:
        """Allowed rows (reads the device: diagnostics and tests)."""
        return int(_unpack_bits(self.bits).sum())



class MaskGroups:
    """A mask per query: the distinct ``RowMask``s of one search and, for each of its NQ
    queries, which of them it runs under.  Built by ``HbmIndexShard.make_mask_groups`` and passed
    as ``search(q, k, allow=...)``; reusable for every search with the same query-to-mask
    assignment.

    ``masks``: the distinct RowMasks (same shard, ``visible`` and ``dead_gen``).  ``group_of``:
    host list, query i runs under ``masks[group_of[i]]``.  The grouped scan (of a bf16 or an fp8
    GPU shard alike: the words and the tile list do not depend on the row format) takes the
    masks in chunks of up to MASK_GROUPS; ``chunk(c)`` builds, once, what the scan of chunk c
    reads:

    * ``idx``: the chunk's query indices (device int64, ascending), ``qgroup``: their group
      within the chunk (device int32);
    * ``mask8``: int64 [n_words, 8], slot g of a tile = the word of the chunk's g-th mask;
    * ``tiles`` / ``n_live``: ``filter_tiles`` of the OR of the chunk's masks;
    * ``groups``: (first group, number of groups), ``nq_of``: queries per group, ``live``: the
      live-tile counts of each mask and, last, of the union as host ints (read once when the
      chunk is built), or None where a mask carries no tile list."""

    __slots__ = ("masks", "group_of", "visible", "dead_gen", "device", "_chunks")

    def __init__(self, masks: list, group_of: list):
        self.masks, self.group_of = list(masks), [int(g) for g in group_of]
        self.visible, self.dead_gen = masks[0].visible, masks[0].dead_gen
        self.device = masks[0].bits.device
        self._chunks: dict = {}

    def __len__(self) -> int:
        return len(self.masks)

    @property
    def n_chunks(self) -> int:
        return (len(self.masks) + MASK_GROUPS - 1) // MASK_GROUPS

    def queries_of(self, g: int) -> list:
        return [i for i, x in enumerate(self.group_of) if x == g]

    def chunk(self, c: int) -> dict:
        ch = self._chunks.get(c)
        if ch is None:
            from ..ops.kernels import filter_tiles

            g0 = c * MASK_GROUPS
            ms = self.masks[g0:g0 + MASK_GROUPS]
            sel = [(i, g - g0) for i, g in enumerate(self.group_of) if g0 <= g < g0 + len(ms)]
            dev = self.device
            words = torch.stack([m.words for m in ms], 1)             # [n_words, G_c]
            mask8 = torch.zeros(words.shape[0], MASK_GROUPS, dtype=torch.int64, device=dev)
            mask8[:, :len(ms)] = words
            union = ms[0].words.clone()
            for m in ms[1:]:
                union.bitwise_or_(m.words)
            tiles, n_live = filter_tiles(union, self.visible)
            # live tiles of each mask and of the union, read once here (the route condition of
            # HbmIndexShard._loop_keeps_chunk; no search reads the device for it)
            live = None
            if all(m.n_live is not None for m in ms):
                live = torch.cat([m.n_live for m in ms] + [n_live]).tolist()
            ch = self._chunks[c] = {
                "idx": torch.tensor([i for i, _ in sel], dtype=torch.int64, device=dev),
                "qgroup": torch.tensor([g for _, g in sel], dtype=torch.int32, device=dev),
                "mask8": mask8, "tiles": tiles, "n_live": n_live, "groups": (g0, len(ms)),
                "live": live, "nq_of": [sum(1 for _, g in sel if g == j) for j in range(len(ms))]}
        return ch


COMPACT_STAGE_BYTES = 256 << 20   # default staging budget of HbmIndexShard.compact


def _dead_bytes(dead_host, count: int) -> np.ndarray:
    """The packed bitmap over the whole tiles of rows [0, count), bits at or past ``count`` (and
    bytes the input does not hold) clear; a copy."""
    n_tiles = (count + TILE_ROWS - 1) // TILE_ROWS
    h = np.zeros(n_tiles * 8, dtype=np.uint8)
    if dead_host is not None:
        m = min(len(dead_host), (count + 7) // 8)
        h[:m] = np.asarray(dead_host[:m], dtype=np.uint8)
        if count % 8:
            h[count // 8] &= (1 << (count % 8)) - 1
    return h


def compact_plan(dead_host, count: int, stage_rows: int):
    """How a compaction moves the live rows of a slab down over the dead ones, in place.

    ``dead_host``: the packed tombstone bitmap (bit r % 8 of byte r // 8); rows at or past
    ``count`` are not live.  Returns ``(c, windows)``: ``c`` (int64 [n_tiles + 1]) is the
    exclusive prefix over 64-row tiles of the live rows per tile -- c[t] is the new row of tile
    t's first live row, c[n_tiles] the live count -- and ``windows`` a list of ``(t0, t1, mode)``
    over source tiles that tiles [tile of the first dead row, n_tiles) exactly (empty without a
    dead row: rows below the first dead row never move).  Each window is one kernel launch
    (index_compact.hip), run in order on one stream; with t1* the largest tile such that
    c[t1*] <= 64 t0, and stage_tiles = stage_rows // 64:

    * ``"direct"`` when t1* - t0 >= stage_tiles, the window [t0, t1*): every destination row
      lies below every source row of the window, so the launch's workgroups move rows straight
      into place in any order;
    * ``"staged"`` otherwise, the window [t0, min(n_tiles, t0 + stage_tiles)): its live rows are
      gathered into a staging buffer of ``stage_rows`` rows, and one contiguous copy behind the
      gather writes them to rows [c[t0], c[t1]).

    A window's destinations end at c[t1] <= 64 t1, below every later window's sources, so
    stream order between windows is the only synchronisation."""
    count = int(count)
    stage_tiles = max(1, int(stage_rows) // TILE_ROWS)
    n_tiles = (count + TILE_ROWS - 1) // TILE_ROWS
    c = np.zeros(n_tiles + 1, dtype=np.int64)
    if n_tiles == 0:
        return c, []
    dead_t = _POPCOUNT8[_dead_bytes(dead_host, count)].reshape(n_tiles, 8).sum(1)
    rows_t = np.full(n_tiles, TILE_ROWS, dtype=np.int64)
    rows_t[-1] = count - TILE_ROWS * (n_tiles - 1)
    np.cumsum(rows_t - dead_t, out=c[1:])
    holed = np.flatnonzero(dead_t)
    windows = []
    t0 = int(holed[0]) if holed.size else n_tiles
    while t0 < n_tiles:
        t1 = int(np.searchsorted(c, TILE_ROWS * t0, side="right")) - 1
        mode = "direct"
        if t1 - t0 < stage_tiles:
            t1, mode = min(n_tiles, t0 + stage_tiles), "staged"
        windows.append((t0, t1, mode))
        t0 = t1
    return c, windows


def compact_new_rows(dead_host, c, rows) -> np.ndarray:
    """New row numbers of the LIVE rows ``rows`` (int array) under the plan's prefix ``c``:
    c[tile] plus the live rows of the tile below the row."""
    r = np.asarray(rows, dtype=np.int64)
    h = _dead_bytes(dead_host, TILE_ROWS * (len(c) - 1))
    t, b = r >> 6, r & 63
    below = (np.arange(8, dtype=np.int64)[None, :] * 8)       # first bit of each byte
    nb = np.clip(b[:, None] - below, 0, 8)                    # bits of each byte below the row
    by = h.reshape(-1, 8)[t] & ((1 << nb) - 1).astype(np.uint8)
    return np.asarray(c, dtype=np.int64)[t] + b - _POPCOUNT8[by].sum(1)


class HbmIndexShard:
    """``dtype="bf16"`` (default) or ``"fp8"``: OCP e4m3 rows of FP8_SCALE * x (half the HBM bytes
    and twice the MFMA rate; BASELINE config #5).  Scores returned are cosines either way.

    ``prefilter="fp8"`` (bf16 shards only): the shard also keeps an e4m3 copy of every row and a
    search scans THAT (half the bytes, twice the MFMA rate) for ``oversample * k`` candidates per
    query, which are then re-scored exactly against the bf16 rows -- Qdrant's scalar quantization
    with ``rescore`` + ``oversampling``.  Returned scores are the exact bf16 cosines; a true
    neighbour is missed only if e4m3 rounding moves it below the candidate cut (recall measured in
    tests/test_kernels_gpu.py and profiles/); the default (None) is the exact bf16 scan."""

    def __init__(self, dim: int, capacity: int, device="cuda", kmax: int = 16, dtype: str = "bf16",
                 prefilter: str | None = None, oversample: int = 3, prune: str | None = None):
        if dtype not in ("bf16", "fp8"):
            raise ValueError(f"index dtype must be bf16 or fp8, got {dtype!r}")
        if dtype == "fp8" and dim not in FP8_DIMS:
            raise ValueError(f"fp8 index rows must be one of {FP8_DIMS} wide, got {dim}")
        if prefilter not in (None, "", "fp8"):
            raise ValueError(f"index prefilter must be fp8 or None, got {prefilter!r}")
        prefilter = prefilter or None
        if prefilter and (dtype != "bf16" or dim not in FP8_DIMS):
            raise ValueError(f"an fp8 prefilter needs a bf16 shard of width {FP8_DIMS}")
        self.prefilter = prefilter
        self.oversample = int(oversample)
        prune = prune or None
        if prune not in (None, "i8"):
            raise ValueError(f"index prune must be i8 or None, got {prune!r}")
        if prune and (dtype != "bf16" or dim not in PRUNE_DIMS):
            raise ValueError(f"the int8 pruned search needs a bf16 shard of width {PRUNE_DIMS}")
        if (prune and dim not in (384, 768)
                and os.environ.get("SYMB_PRUNE_STREAM", "1") in ("", "0")):
            raise ValueError(f"the {dim}-wide pruned search runs on the stream scan only")
        self.prune = prune
        self.dim = dim
        self.dtype = dtype
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity = int(capacity)
        # (zeroed: the int8 stream image quantises whole 32-row sub-tiles with one shared scale, so
        # the not-yet-written rows of a sub-tile enter its scale)
        self.rows = torch.zeros(_round_up(max(self.capacity, 1), TILE_ROWS), dim,
                                dtype=torch.uint8 if dtype == "fp8" else torch.bfloat16,
                                device=self.device)
        # e4m3 image of the bf16 rows for the prefilter scan (kept in step by every write)
        self.rows8 = (torch.empty(self.rows.shape, dtype=torch.uint8, device=self.device)
                      if prefilter else None)
        # prune="i8": int8 image of the bf16 rows (per-row scale) for the EXACT bound-pruned
        # search (csrc/hip/index_i8.hip), plus the two global maxima its error bound needs:
        # E = max |x - x~| and X = max |x~| over every row ever written (monotone, so conservative)
        self.rows_i8 = self.sx_i8 = self.i8_bounds = None
        # the image's form (calibrate_prune): 0 = plain int8 rows; SPLIT_HEAVY[dim] = the split
        # image of PCA-rotated rows (leading components fp16, the rest int8) for anisotropic
        # corpora.  SYMB_I8_SPLIT: "auto" (default) = chosen by the rows' spectrum, at write time
        # for the widths in AUTO_SPLIT_DIMS and by an explicit calibrate_prune() for every width
        # in SPLIT_DIMS; "on" = forced at every width in SPLIT_DIMS; "off" = always plain
        self.i8_split = os.environ.get("SYMB_I8_SPLIT", "auto").strip().lower()
        self._i8_heavy = 0
        self._i8_rot = None          # fp64 [D, D] orthogonal basis (rows: components) or None
        self._calib_gen = 0
        self._calib_next = self.CALIB_MIN_ROWS
        self.calib_share = None      # variance share of the leading components at calibration
        # the stream images (index_stream.hip) for the plain int8 form and the MX-fp4 tier:
        # [n_sub, REC] bytes, 32-row sub-tiles in fragment-major order (img_i8 / img_mx4)
        self.stream = bool(prune) and dim in STREAM_DIMS and os.environ.get(
            "SYMB_PRUNE_STREAM", "1") not in ("", "0")
        # the int8 tier's kernel, chosen apart from the fp4 tier's: "stream"
        # = the fragment-major image (index_stream.hip) or "ring" = the row-major image with
        # per-row scales on the LDS-ring scan (index_i8.hip, round 4's I8Dim<768>); the MX-fp4
        # tier keeps its stream image either way.
        # SYMB_PRUNE_I8=auto takes I8_RING_DIMS.
        i8k = os.environ.get("SYMB_PRUNE_I8", "auto").strip().lower()
        self.i8_ring = bool(self.stream and dim in (384, 768) and (
            i8k == "ring" or (i8k == "auto" and dim in I8_RING_DIMS)))
        self.img_i8 = self.img_mx4 = None
        if prune:
            # padded to whole 128-row tiles: the int8 scan's DMA reads whole tiles; one flat byte
            # store (viewed per form), at 384 sized for the widest form that applies, at 768 for
            # the form in use (_i8_store_bytes)
            n_alloc = _round_up(self.rows.shape[0], 128)
            self.sx_i8 = torch.ones(n_alloc, dtype=torch.float32, device=self.device)
            self._i8_store = torch.zeros(self._i8_store_bytes(0), dtype=torch.int8,
                                         device=self.device)
            self._set_i8_view(0)
            # (E, X) of the plain form; (E_l, X_l, E_h, X_h) of the split form
            self.i8_bounds = torch.zeros(4, dtype=torch.float32, device=self.device)
        # the MX-fp4 image (a first tier below the int8 one, _pruned_end): 192 bytes of e2m1
        # nibbles + 16 bytes of block scales per 384-wide row, and its (E4, X4) maxima
        self.rows_mx4 = self.sc_mx4 = self.mx4_bounds = None
        if (prune and dim in (MX4_DIMS if self.stream else (384,))
                and os.environ.get("SYMB_PRUNE_MX4", "1") not in ("", "0")):
            n_alloc = _round_up(self.rows.shape[0], 128)
            if self.stream:
                self.img_mx4 = torch.zeros(n_alloc // STREAM_SUB, self._stream_rec(1),
                                           dtype=torch.uint8, device=self.device)
            else:
                self.rows_mx4 = torch.zeros(n_alloc, dim // 2, dtype=torch.uint8, device=self.device)
                self.sc_mx4 = torch.zeros(n_alloc, 16, dtype=torch.uint8, device=self.device)
            self.mx4_bounds = torch.zeros(2, dtype=torch.float32, device=self.device)
        # the prefix tier (_pruned_begin): the fp4 stream scan over the first prefix_ksteps
        # k-steps (64 dims each) of every record.  mx4_pbounds = (E_P, X_P, XR), the maxima over
        # every row written of |x_P - x~_P|, |x~_P| and |x_R|, tracked beside mx4_bounds for this
        # one prefix length (SYMB_PREFIX_KSTEPS for A/B runs); None: not tracked, the tier is off
        self.prefix_ksteps = int(os.environ.get("SYMB_PREFIX_KSTEPS", "") or self.PREFIX_KSTEPS)
        self.mx4_pbounds = None
        if self.img_mx4 is not None and dim == 384 and self.prefix_ksteps in (2, 3):
            self.mx4_pbounds = torch.zeros(3, dtype=torch.float32, device=self.device)
        self.prefix_tier = int(os.environ.get("SYMB_PREFIX_TIER", "") or self.PREFIX_TIER)
        # the share of mP the tier's choice allows between a row's prefix estimate and its exact
        # partial score (PREFIX_BAND; SYMB_PREFIX_BAND for A/B runs, 1 = the worst case)
        self.prefix_band = float(os.environ.get("SYMB_PREFIX_BAND", "") or self.PREFIX_BAND)
        self._pfx_tot = None     # searches whose first tier was the prefix scan (device int32 [1])
        self._pfx_last = None
        self.count = 0      # rows reserved (payload slots exist)
        # rows searches may read: published only after their writes are ENQUEUED on the stream
        # the scans share, so a search racing an upsert in another thread never scans a reserved
        # but unwritten row (stream order then guarantees the write lands first)
        self.visible = 0
        self.payloads = PayloadStore()
        # smallest row block (in 64-row tiles) of the 256-query list scan: small scans (threshold
        # seeding, the fresh-row tail) are latency-bound, so fewer tiles per block = more CUs
        self.scan_min_tiles = 16
        # ... and of the two small list scans on the sampled searches' critical path (seed
        # sub-sample ~49k rows, fresh-row tail 4096-8191 rows at 100M): one tile per workgroup
        # spreads them over every CU (106 -> 52 us and 211 -> 57 us; profiles/r2_min_tiles/)
        self.prepass_min_tiles = 1
        self.scan_aux = -1   # index-stream cache policy (-1 = auto: non-temporal when read once)
        self.seed_threshold = True  # sample pre-pass seeds per-query top-k thresholds
        # masked search (_search_filtered): a stride-64 pass over the live tiles first, whose k-th
        # best allowed score seeds the full pass's thresholds (FILTER_SEED_DEFAULT has the A/B)
        self.filter_seed = self.FILTER_SEED_DEFAULT
        # (candidate counts, overflow flag) of the last masked large-k search (tests, benchmarks)
        self._filter_large_k_last = None
        # > 256 queries: put the query blocks of each row block on one XCD (row stream shared
        # through that XCD's L2 instead of re-read from HBM once per query block)
        self.scan_xcd = 1
        # >= 512 seeded queries on a 384-wide bf16 shard (the per-rank shape of the sharded search
        # at N >= 2 GPUs): the 512-query-per-workgroup candidate-emitting kernel (index_mq.hip)
        self.scan_cus = 0      # 0 = every CU (see _n_cus)
        # CUs the fp4 stream scan of a split-phase search (search_begin / search_end) leaves
        # whole for the work its caller runs beside it; 0 = none, the thin form (_scan_reserve;
        # SYMB_SCAN_RESERVE for A/B runs).  scan_depth: the fp4 scan's sub-tiles in flight per
        # wave at dim 384 (0 = the kernel's 3; 4, 5; SYMB_SCAN_DEPTH)
        self.scan_reserve = int(os.environ.get("SYMB_SCAN_RESERVE", "") or self.SCAN_RESERVE)
        self.scan_depth = int(os.environ.get("SYMB_SCAN_DEPTH", "") or 0)
        # scan_nt: the fp4 stream scan at dim 384 loads its rows non-temporally (index_stream.hip
        # NT_; SYMB_SCAN_NT for A/B runs) -- the one form whose sub-tiles are read once each
        self.scan_nt = int(os.environ.get("SYMB_SCAN_NT", "") or self.SCAN_NT)
        # prune_fused_finish: the pruned search ends in one launch (prune_finish.hip: re-score,
        # top-k, tier word) instead of rescore_bf16 + topk_select_counted + a host copy.
        # route_at_begin: a split-phase search enqueues the candidate prefill and the bf16 scan of
        # the routed blocks in its begin half (they read nothing the stream scan writes).
        # Both shorten the compute stream's tail between two scans and both are OFF by default:
        # the headline step is paced by the encoder stream, and with them on it measured the same
        # within the run-to-run spread (profiles/r17_step/README.md); SYMB_PRUNE_FINISH=1 /
        # SYMB_ROUTE_AT_BEGIN=1 switch them on for A/B runs.
        self.prune_fused_finish = os.environ.get("SYMB_PRUNE_FINISH", "0") not in ("", "0")
        self.route_at_begin = os.environ.get("SYMB_ROUTE_AT_BEGIN", "0") not in ("", "0")
        self._tier_words = None   # pinned ring of tier words (prune_finish writes them)
        self._tier_slot = 0
        self.scan_mq = True
        self.mq_min_nq = 256   # smallest batch for the emitting kernel (< 512: a 256-query form)
        # smallest batch for the int8-pruned search: its scan costs about the same for 1..256
        # queries (one 256-query block per row block), and a service's bursts under load are
        # often smaller than 256 -- they would otherwise take the full bf16 list scan
        self.prune_min_nq = 16
        # 256-query form: True = 4 query sets per wave, waves w / w + 4 splitting each tile's rows
        # (half the LDS fragment reads per tile); False = 2 sets per wave, every wave all rows
        self.mq_rsplit = True
        self.mq_stats = False  # accumulate overflow count / max candidates (diagnostics)
        # int8 pruned scan at >= 512 queries: False = 512 queries per workgroup (each row tile
        # streamed once per 512 queries), True = the 256-query fused form (twice the L2 reads)
        self.i8_rsplit2 = False
        self._mq_tot = None
        self._mx4_tot = None     # searches whose first tier was the MX-fp4 scan (mq_stats)
        self.tier_stats = True   # ... counted even without mq_stats (one tiny add per search)
        self._mx4_last = None
        self._tier_last = None
        # the tier recent searches took, read back without a sync: (pinned int, event) of each
        # search's MX-fp4 flag, and the last one known to have landed (True: the fp4 tier ran)
        self._tier_pending = collections.deque()
        self._tier_lock = threading.Lock()   # concurrent searches drain / append it
        self._tier_mx4 = False
        # snapshot change record (index/persist.py ShardPersister): rows covered by the last cut
        # and the covered rows overwritten since; kept only while ``payloads.track`` is on
        self._persisted = 0
        self._dirty: set[int] = set()
        self._persist_key = None
        # tombstones (delete_rows): the device bitmap of deleted rows (uint8, whole 64-bit words
        # over the slab, packed as a RowMask: bit r % 64 of word r // 64), allocated by the first
        # delete so a shard that never deletes pays nothing; its host copy (what persistence
        # writes); the dead rows below ``count``; and the delete generation, bumped by every
        # delete (RowMasks carry it, the live mask and the snapshot cut compare it)
        self.dead = None
        self._dead_host = None
        self.n_dead = 0
        self.dead_gen = 0
        self._dead_cut_gen = 0       # dead_gen the last snapshot cut / load saw
        # how a search treats tombstones: "zero" = the unmasked route + the dead-id check + the
        # gated masked scan (_search_tombstoned), "mask" = always the masked scan
        self.delete_route = self.DELETE_ROUTE_DEFAULT[dtype]
        self.last_dead_hits = None   # device int32 [1]: dead ids the last search's route returned
        self._live_mask = None
        self._live_key = None
        self._all_rows_mask = None   # _all_rows: the all-ones RowMask of the rows visible then
        self._zero_hits = None
        # compactions that moved rows (compact): row numbers handed out before one are stale
        self.compact_gen = 0
        self.last_compact = None

    # ------------------------------------------------------------------ pruning images
    def _stream_rec(self, form: int) -> int:
        """Bytes per 32-row sub-tile of the stream image (form 0 = int8, 1 = MX-fp4); the same
        numbers as index_stream.hip SDim (checked against the extension on a GPU)."""
        nks = self.dim // (64 if form else 32)
        return nks * 1024 + ((nks + 3) // 4 * 256 if form else 16)

    def _i8_store_bytes(self, heavy: int) -> int:
        """Bytes of the flat int8 store for the form.  A 384-wide shard keeps one store sized for
        its widest form; wider shards (100M x 768 fills most of a card) hold only the form in
        use, so one that stays plain pays nothing for the split image."""
        n_alloc = self.sx_i8.shape[0]
        if self.dim == 384:
            heavy = SPLIT_HEAVY[384]
        nbytes = n_alloc * (self.dim + heavy)
        if self.stream and not self.i8_ring and (self.dim == 384 or not heavy):
            nbytes = max(nbytes, n_alloc // STREAM_SUB * self._stream_rec(0))
        return nbytes

    def _set_i8_view(self, heavy: int) -> None:
        """Views of the flat int8 store for the form: the stream image (plain form on a stream
        shard) or the row-major image [n_alloc, D + heavy] (split form, or stream off).  A store
        of another form's size is released first, then allocated anew (the caller re-images
        every row)."""
        n_alloc = self.sx_i8.shape[0]
        nbytes = self._i8_store_bytes(heavy)
        if self._i8_store.numel() != nbytes:
            self._i8_store = self.rows_i8 = self.img_i8 = None
            self._i8_store = torch.zeros(nbytes, dtype=torch.int8, device=self.device)
        if self.stream and not heavy and not self.i8_ring:
            rec = self._stream_rec(0)
            self.img_i8 = self._i8_store[:n_alloc // STREAM_SUB * rec].view(torch.uint8).view(
                n_alloc // STREAM_SUB, rec)
            self.rows_i8 = None
        else:
            rb = self.dim + heavy
            self.img_i8 = None
            self.rows_i8 = self._i8_store[:n_alloc * rb].view(n_alloc, rb)

    @property
    def prune_on(self) -> bool:
        """The shard keeps a pruning image (prune="i8")."""
        return self.i8_bounds is not None

    @property
    def mx4_on(self) -> bool:
        """The shard keeps the MX-fp4 first-tier image."""
        return self.mx4_bounds is not None

    def _stream_subtiles_cpu(self, img, form: int, r0: int, r1: int) -> None:
        """CPU backend: recompute the stream records of the sub-tiles covering rows [r0, r1) from
        the bf16 rows (per-row images: the other rows' bytes come out unchanged)."""
        from ..ops import reference as R

        g0, g1 = r0 // STREAM_SUB, (r1 + STREAM_SUB - 1) // STREAM_SUB
        hi = min(g1 * STREAM_SUB, self.count)
        src = self.rows[g0 * STREAM_SUB:hi]
        if form:
            rec, nr = R.stream_mx4_ref(src)
            w = nr[r0 - g0 * STREAM_SUB:r1 - g0 * STREAM_SUB]
            torch.maximum(self.mx4_bounds, w[:, :2].amax(0), out=self.mx4_bounds)
            if self.mx4_pbounds is not None:
                pn = R.mx4_prefix_norms_ref(src[r0 - g0 * STREAM_SUB:r1 - g0 * STREAM_SUB],
                                            self.prefix_ksteps)
                torch.maximum(self.mx4_pbounds, pn[:, [0, 1, 3]].amax(0), out=self.mx4_pbounds)
        else:
            rec, err, xtn = R.stream_i8_ref(src)
            # (every row of the re-imaged sub-tiles: their shared scale may have changed)
            torch.maximum(self.i8_bounds[:2], torch.stack([err.max(), xtn.max()]),
                          out=self.i8_bounds[:2])
        img[g0:g0 + rec.shape[0]] = rec

    def _image_rows(self, r0: int = 0, n: int = 0, rows=None) -> None:
        """(Re)write the pruning images (int8 / split form and MX-fp4) of bf16 rows [r0, r0 + n)
        or of the listed rows (a distinct int tensor), bounds raised."""
        if rows is not None:
            rows = torch.as_tensor(rows).to(self.device, torch.int32).contiguous()
            n = rows.numel()
        if n <= 0:
            return
        gpu = self.device.type == "cuda"
        if gpu:
            from ..ops._ext import hip, stream_handle

            h, st = hip(), stream_handle(self.device)
            rp = 0 if rows is None else rows.data_ptr()
        if self.prune_on:
            if self.img_i8 is not None:
                if gpu:
                    h.quant_stream_i8(self.rows.data_ptr(), r0, rp, n, self.dim,
                                      self.img_i8.data_ptr(), self.i8_bounds.data_ptr(), st)
                elif rows is None:
                    self._stream_subtiles_cpu(self.img_i8, 0, r0, r0 + n)
                else:
                    for r in rows.tolist():
                        self._stream_subtiles_cpu(self.img_i8, 0, r, r + 1)
            elif rows is None:
                self._i8_image(self.rows[r0:r0 + n], self.rows_i8[r0:r0 + n],
                               self.sx_i8[r0:r0 + n], self.i8_bounds)
            else:
                ri = rows.long()
                img = torch.empty(n, self.rows_i8.shape[1], dtype=torch.int8, device=self.device)
                sc = torch.empty(n, dtype=torch.float32, device=self.device)
                self._i8_image(self.rows[ri], img, sc, self.i8_bounds)
                self.rows_i8.index_copy_(0, ri, img)
                self.sx_i8.index_copy_(0, ri, sc)
        if self.mx4_on:
            if self.img_mx4 is not None:
                if gpu:
                    pb = self.mx4_pbounds
                    h.quant_stream_mx4(self.rows.data_ptr(), r0, rp, n, self.dim,
                                       self.img_mx4.data_ptr(), 0, 0, self.mx4_bounds.data_ptr(),
                                       0, st, pbounds=0 if pb is None else pb.data_ptr(),
                                       nkp=0 if pb is None else self.prefix_ksteps)
                elif rows is None:
                    self._stream_subtiles_cpu(self.img_mx4, 1, r0, r0 + n)
                else:
                    for r in rows.tolist():
                        self._stream_subtiles_cpu(self.img_mx4, 1, r, r + 1)
            elif rows is None:
                self._mx4_image(self.rows[r0:r0 + n], self.rows_mx4[r0:r0 + n],
                                self.sc_mx4[r0:r0 + n], self.mx4_bounds)
            else:
                ri = rows.long()
                img4 = torch.empty(n, self.dim // 2, dtype=torch.uint8, device=self.device)
                sc4 = torch.empty(n, 16, dtype=torch.uint8, device=self.device)
                self._mx4_image(self.rows[ri], img4, sc4, self.mx4_bounds)
                self.rows_mx4.index_copy_(0, ri, img4)
                self.sc_mx4.index_copy_(0, ri, sc4)

    @property
    def prefix_on(self) -> bool:
        """The shard tracks the prefix tier's bounds (mx4_pbounds)."""
        return self.mx4_pbounds is not None

    @property
    def prefix_runs(self) -> int:
        """Searches whose first tier was the prefix scan (a device counter; this reads it back)."""
        return 0 if self._pfx_tot is None else int(self._pfx_tot.item())

    def mx4_query_image(self, q_unit: torch.Tensor, prefix: bool = False):
        """(nibbles, scale record, margin) of unit queries for the MX-fp4 tier: the stream form
        (quant_stream_mx4: [NQ][D / 2], [NQ][2 NSC] dwords) or the LDS-ring form (quant_rows_mx4:
        [NQ][192], [NQ][16] bytes); margin = |q| E4 + |q - q~| X4 + 1e-5.
        ``prefix`` (a shard with prefix bounds): also (mP, qR), the prefix tier's margin
        |q_P| E_P + |q_P - q~_P| X_P + 1e-5 and |q_R|."""
        NQ, dev = q_unit.shape[0], self.device
        if prefix and (self.mx4_pbounds is None or self.img_mx4 is None):
            raise ValueError("mx4_query_image: the shard tracks no prefix bounds")
        q4 = torch.empty(NQ, self.dim // 2, dtype=torch.uint8, device=dev)
        m4 = torch.empty(NQ, dtype=torch.float32, device=dev)
        mP = torch.empty(NQ, dtype=torch.float32, device=dev) if prefix else None
        qR = torch.empty(NQ, dtype=torch.float32, device=dev) if prefix else None
        if self.img_mx4 is None:
            qs4 = torch.empty(NQ, 16, dtype=torch.uint8, device=dev)
            self._mx4_image(q_unit, q4, qs4, self.mx4_bounds, margin=m4)
            return q4, qs4, m4
        nsc = (self.dim // 64 + 3) // 4
        qs4 = torch.empty(NQ, 2 * nsc, dtype=torch.int32, device=dev)
        if dev.type == "cuda":
            from ..ops._ext import hip, stream_handle

            pk = dict(pbounds=self.mx4_pbounds.data_ptr(), nkp=self.prefix_ksteps,
                      mP=mP.data_ptr(), qR=qR.data_ptr()) if prefix else {}
            hip().quant_stream_mx4(q_unit.data_ptr(), 0, 0, NQ, self.dim, 0, q4.data_ptr(),
                                   qs4.data_ptr(), self.mx4_bounds.data_ptr(), m4.data_ptr(),
                                   stream_handle(dev), **pk)
            return (q4, qs4, m4, mP, qR) if prefix else (q4, qs4, m4)
        from ..ops.reference import mx4_prefix_norms_ref, stream_mx4_query_ref

        img, qs, _, nr = stream_mx4_query_ref(q_unit)
        q4.copy_(img)
        qs4.copy_(qs)
        m4.copy_(nr[:, 2] * self.mx4_bounds[0] + nr[:, 0] * self.mx4_bounds[1] + 1e-5)
        if prefix:
            pn = mx4_prefix_norms_ref(q_unit, self.prefix_ksteps)
            mP.copy_(pn[:, 2] * self.mx4_pbounds[0] + pn[:, 0] * self.mx4_pbounds[1] + 1e-5)
            qR.copy_(pn[:, 3])
            return q4, qs4, m4, mP, qR
        return q4, qs4, m4

    # ------------------------------------------------------------------ inserts
    def _reserve(self, n: int) -> int:
        if self.count + n > self.capacity:
            raise MemoryError(f"index shard full ({self.count}+{n} > {self.capacity})")
        r0 = self.count
        self.count += n
        self.payloads.extend_empty(n)
        return r0

    def truncate(self, n: int) -> None:
        """Forget rows >= n (their payload slots too)."""
        if n >= self.count:
            return
        self.payloads.truncate(n)
        self.count = n
        self.visible = min(self.visible, n)
        self._persisted = min(self._persisted, n)
        self._dirty = {r for r in self._dirty if r < n}
        if self.n_dead:
            # the forgotten slots are written anew by later appends: their tombstones go
            h = self._dead_host
            h[(n + 7) // 8:] = 0
            if n % 8:
                h[n // 8] &= (1 << (n % 8)) - 1
            self.dead.copy_(torch.from_numpy(h))
            left = int(_POPCOUNT8[h].sum())
            if left != self.n_dead:
                self.n_dead = left
                self.dead_gen += 1

    def _mark_written(self, rows) -> None:
        """Rows overwritten in place: remember the ones the last snapshot already covers."""
        if self.payloads.track and self._persisted:
            self._dirty.update(int(r) for r in rows if r < self._persisted)

    def publish(self) -> None:
        """Make every reserved row searchable (call after its write is enqueued)."""
        self.visible = self.count

    def append_unit(self, unit_bf16: torch.Tensor) -> int:
        """Append already unit-norm bf16 rows (e.g. the encoder's pooled+normalised output)."""
        n = unit_bf16.shape[0]
        r0 = self._reserve(n)
        if self.dtype == "fp8":
            self._store(r0, unit_bf16.to(self.device), normalize=False)
        elif not self._append_fused(unit_bf16, r0, n):
            self.rows[r0:r0 + n].copy_(unit_bf16, non_blocking=True)
            self.rows_written(r0, n)
        self.publish()
        return r0

    def _append_fused(self, src: torch.Tensor, r0: int, n: int) -> bool:
        """One-launch append (prepass.hip append_rows_kernel: the bf16 rows, their int8 and
        MX-fp4 stream images and both bound pairs) when the shard keeps plain stream images, no
        fp8 prefilter image and no re-calibration is due; False: the caller takes the general
        path (copy + rows_written)."""
        if (self.device.type != "cuda" or n <= 0 or self.rows8 is not None
                or self.img_i8 is None or self._i8_heavy or not self.prune_on
                or self.dim not in STREAM_DIMS or self.mx4_on != (self.img_mx4 is not None)):
            return False
        due = r0 + n >= self._calib_next or (self.i8_split == "on" and not self._i8_heavy)
        if due and self._split_at_write():
            return False
        if (src.device != self.device or src.dtype != torch.bfloat16 or not src.is_contiguous()
                or src.shape[-1] != self.dim):
            return False
        from ..ops._ext import hip, stream_handle

        m4 = self.img_mx4 is not None
        pb = self.mx4_pbounds if m4 else None
        hip().append_rows(src.data_ptr(), n, self.dim, self.rows.data_ptr(), r0,
                          self.img_i8.data_ptr(), self.i8_bounds.data_ptr(),
                          self.img_mx4.data_ptr() if m4 else 0,
                          self.mx4_bounds.data_ptr() if m4 else 0, stream_handle(self.device),
                          pb4=0 if pb is None else pb.data_ptr(),
                          nkp=0 if pb is None else self.prefix_ksteps)
        return True

    def _split_at_write(self) -> bool:
        """The write-time triggers may (re-)calibrate this shard's image: SYMB_I8_SPLIT=on at every
        width the split image exists for, auto only where a shard changes form by itself."""
        if self.i8_split == "off":
            return False
        return self.dim in (SPLIT_DIMS if self.i8_split == "on" else AUTO_SPLIT_DIMS)

    def rows_written(self, r0: int, n: int) -> None:
        """bf16 rows [r0, r0+n) changed: refresh their e4m3 prefilter image and their int8
        pruning image (no-ops without them).  Callers that write ``rows`` directly (snapshot loads)
        must call this too."""
        if self.prune_on and n > 0:
            due = r0 + n >= self._calib_next or (self.i8_split == "on" and not self._i8_heavy)
            if due and self._split_at_write():
                # (re-images every row below r0 + n when the image's form changes; the new
                # rows' MX-fp4 image below)
                self.calibrate_prune(r0 + n, lo=r0)
                if self.mx4_on:
                    saved, self.i8_bounds = self.i8_bounds, None
                    try:
                        self._image_rows(r0, n)
                    finally:
                        self.i8_bounds = saved
            else:
                self._image_rows(r0, n)
        elif self.mx4_on and n > 0:
            self._image_rows(r0, n)
        if self.rows8 is None or n <= 0:
            return
        src, dst = self.rows[r0:r0 + n], self.rows8[r0:r0 + n]
        if self.device.type == "cuda":
            from ..ops import kernels as K

            K.quant_fp8(src, dst, FP8_SCALE, False)
        else:
            dst.copy_((src.float() * FP8_SCALE).to(torch.float8_e4m3fn).view(torch.uint8))

    # ------------------------------------------------------------------ int8 image form
    CALIB_MIN_ROWS = 1 << 16   # first calibration once this many rows are written ...
    CALIB_GROWTH = 16          # ... and again each time the shard grows this many times over
    CALIB_SAMPLE = 1 << 16     # rows the second-moment matrix is estimated from
    # the split form pays (+17 % image bytes and MFMA work) once the leading SPLIT_HEAVY principal
    # components hold this share of the rows' energy: 64 / 384 = 0.17 for isotropic rows; the
    # anisotropic corpus (index/synth.py) holds ~0.8, sentence-embedding spaces typically 0.4+
    SPLIT_MIN_SHARE = 0.3

    def calibrate_prune(self, hi: int | None = None, lo: int | None = None) -> None:
        """Choose the pruning image's form from the rows [0, hi) and re-image them all.

        The int8 bound |q| E + |q - q~| X is a Cauchy-Schwarz bound with the scale set by each
        row's largest component.  Where a few directions carry most of the energy (an anisotropic
        corpus: a shared mean direction plus a power-law spread, as in sentence-embedding spaces)
        those components set every row's int8 step, the bound covers a wide band of the crowded
        scores and the route sends every block to the bf16 scan (profiles/r3_real: pruned = 1.00x
        plain).  The split form rotates rows and queries into the principal basis of the rows'
        second-moment matrix (fp64, orthogonal: q . x = (R q) . (R x)), keeps the leading
        SPLIT_HEAVY components as fp16 (~11 bits, their rounding in the bound) and quantises only
        the trailing ones to int8 with their own, much finer, per-row step.  On the anisotropic
        corpus the candidates per query drop ~30x (tests/test_index_cpu.py); exactness never
        depends on R, only the cost does, so R is fixed between calibrations (first at
        CALIB_MIN_ROWS rows, then at every CALIB_GROWTH-fold growth).

        ``lo``: rows [0, lo) already carry the current image.  When the chosen form stays the
        plain int8 one (no basis), only [lo, hi) is imaged and the generation is kept: a
        re-image of every row would change nothing."""
        if not self.prune_on:
            return
        hi = self.count if hi is None else int(hi)
        if hi <= 0:
            return
        heavy, rot, share = 0, None, None
        if self.dim in SPLIT_DIMS and self.i8_split != "off":
            stride = max(1, hi // self.CALIB_SAMPLE)
            smp = self.rows[0:hi:stride][:self.CALIB_SAMPLE].double()
            m2 = smp.t() @ smp / smp.shape[0]
            ev, vec = torch.linalg.eigh(m2)                 # ascending
            ev, vec = ev.flip(0), vec.flip(1)
            share = float(ev[:SPLIT_HEAVY[self.dim]].sum() / ev.sum().clamp_min(1e-30))
            if self.i8_split == "on" or share >= self.SPLIT_MIN_SHARE:
                heavy, rot = SPLIT_HEAVY[self.dim], vec.t().contiguous()
        # (the int8 / split image only)
        mx4_saved, self.mx4_bounds = self.mx4_bounds, None
        try:
            if heavy == 0 and self._i8_heavy == 0 and lo is not None:
                self.calib_share = share
                self._image_rows(lo, hi - lo)
                self._calib_next = max(hi * self.CALIB_GROWTH, self.CALIB_MIN_ROWS)
                return
            self._i8_heavy, self._i8_rot, self.calib_share = heavy, rot, share
            self._set_i8_view(heavy)
            self.i8_bounds.zero_()
            chunk = 1 << 18
            for s in range(0, hi, chunk):
                self._image_rows(s, min(hi, s + chunk) - s)
        finally:
            self.mx4_bounds = mx4_saved
        self._calib_gen += 1
        self._calib_next = max(hi * self.CALIB_GROWTH, self.CALIB_MIN_ROWS)

    def _mx4_image(self, src, dst, sc, bounds, margin=None) -> None:
        """MX-fp4 image of bf16 rows (bounds raised) or, with ``margin``, of queries (margin
        = |q| E4 + |q - q~| X4 + 1e-5 from bounds): index_i8.hip quant_rows_mx4."""
        n = src.shape[0]
        if n == 0:
            return
        if self.device.type == "cuda":
            from ..ops._ext import hip, stream_handle

            hip().quant_rows_mx4(src.data_ptr(), n, self.dim, dst.data_ptr(), sc.data_ptr(),
                                 bounds.data_ptr(), 0 if margin is None else margin.data_ptr(),
                                 stream_handle(self.device))
            return
        from ..ops.reference import quant_rows_mx4_ref

        img, scr, _, nr = quant_rows_mx4_ref(src)
        dst.copy_(img)
        sc.copy_(scr)
        if margin is None:
            torch.maximum(bounds, nr[:, :2].amax(0), out=bounds)
        else:
            margin.copy_(nr[:, 2] * bounds[0] + nr[:, 0] * bounds[1] + 1e-5)

    def prune_query_image(self, q_unit: torch.Tensor, zero: torch.Tensor | None = None):
        """(image, scale, margin) of unit queries in the shard's current form: the int8 image and
        |q| E + |q - q~| X + 1e-5 (prune_qquant), or the split image in the shard's basis and
        |q_l| E_l + |q_l - q~_l| X_l + |q_h| E_h + |q_h - q^_h| X_h + 1e-5 (quant_rows_split).
        ``zero`` (int32, optional): a workspace cleared on the way (by the quantiser itself on the
        plain form: no memset launch)."""
        NQ, dev, heavy = q_unit.shape[0], self.device, self._i8_heavy
        q8 = torch.empty(NQ, self.dim + heavy, dtype=torch.int8, device=dev)
        sq = torch.empty(NQ, dtype=torch.float32, device=dev)
        margin = torch.empty(NQ, dtype=torch.float32, device=dev)
        if dev.type != "cuda":
            from ..ops import reference as R

            b = self.i8_bounds
            if heavy:
                img, sc, nr = R.quant_rows_split_ref(self._rotate(q_unit), heavy)
                m = nr[:, 2] * b[0] + nr[:, 0] * b[1] + nr[:, 5] * b[2] + nr[:, 3] * b[3]
            else:
                img, sc, err, _ = R.quant_rows_i8_ref(q_unit)
                m = q_unit.float().norm(dim=1) * b[0] + err * b[1]
            q8.copy_(img)
            sq.copy_(sc)
            margin.copy_(m + 1e-5)
            if zero is not None:
                zero.zero_()
            return q8, sq, margin
        from ..ops._ext import hip, stream_handle

        st = stream_handle(dev)
        if heavy:
            qr = self._rotate(q_unit)
            hip().quant_rows_split(qr.data_ptr(), NQ, self.dim, q8.data_ptr(), sq.data_ptr(),
                                   self.i8_bounds.data_ptr(), margin.data_ptr(), st)
            if zero is not None:
                zero.zero_()
        else:
            hip().prune_qquant(q_unit.data_ptr(), NQ, self.dim, self.i8_bounds.data_ptr(),
                               q8.data_ptr(), sq.data_ptr(), margin.data_ptr(), st,
                               zero=0 if zero is None else zero.data_ptr(),
                               zero_n=0 if zero is None else zero.numel())
        return q8, sq, margin

    def prune_estimate(self, q8: torch.Tensor, sq: torch.Tensor, r0: int = 0,
                       r1: int | None = None) -> torch.Tensor:
        """The int8 scan's estimate of every (query, row) score over rows [r0, r1) (torch; the
        bound oracle of the tests): sq sx (q8 . x8), or the split form's q^_h . x^_h + sq sx
        (q8_l . x8_l)."""
        from ..ops import reference as R

        r1 = self.count if r1 is None else r1
        if self.img_i8 is not None:
            g0, g1 = r0 // STREAM_SUB, (r1 + STREAM_SUB - 1) // STREAM_SUB
            x8, sx = R.stream_i8_decode(self.img_i8[g0:g1], (g1 - g0) * STREAM_SUB, self.dim)
            x8, sx = x8[r0 - g0 * STREAM_SUB:r1 - g0 * STREAM_SUB], sx[r0 - g0 * STREAM_SUB:r1 - g0 * STREAM_SUB]
        else:
            x8, sx = self.rows_i8[r0:r1], self.sx_i8[r0:r1]
        if self._i8_heavy:
            return R.split_estimate_ref(q8, sq, x8, sx, self._i8_heavy)
        return (q8.float() @ x8.float().t()) * sq[:, None] * sx[None, :]

    def _rotate(self, x: torch.Tensor) -> torch.Tensor:
        """Rows / queries in the split form's basis: fp64 product, rounded once to fp32."""
        return (x.double() @ self._i8_rot.t()).float().contiguous()

    def _i8_image(self, src, dst8, scale, bounds) -> None:
        """The pruning image of bf16 rows ``src`` in the shard's current form (bounds raised)."""
        n = src.shape[0]
        if n == 0:
            return
        if not self._i8_heavy:
            self._quant_i8(src, dst8, scale, bounds)
            return
        # bounds the fp64 / fp32 rotation temporaries (~1.2 GB at every width)
        chunk = max(1, (1 << 18) * 384 // self.dim)
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            xr = self._rotate(src[s:e])
            if self.device.type == "cuda":
                from ..ops._ext import hip, stream_handle

                hip().quant_rows_split(xr.data_ptr(), e - s, self.dim, dst8[s:e].data_ptr(),
                                       scale[s:e].data_ptr(), bounds.data_ptr(), 0,
                                       stream_handle(self.device))
            else:
                from ..ops.reference import quant_rows_split_ref

                img, sc, nrm = quant_rows_split_ref(xr, self._i8_heavy)
                dst8[s:e].copy_(img)
                scale[s:e].copy_(sc)
                m = nrm.amax(0)
                torch.maximum(bounds, torch.stack([m[0], m[1], m[3], m[4]]), out=bounds)

    def _quant_i8(self, src, dst8, scale, bounds=None):
        """Per-row int8 image of bf16 rows (index_i8.hip quant_rows_i8).  With ``bounds`` (the
        shard's (E, X)) the maxima of |x - x~| and |x~| are folded into it (on the GPU inside the
        kernel, returning (None, None)); without, the per-row norms are returned (queries)."""
        n = src.shape[0]
        if self.device.type == "cuda":
            from ..ops._ext import hip, stream_handle

            if bounds is not None:   # row writes: the kernel folds the maxima in (one launch)
                hip().quant_rows_i8(src.data_ptr(), n, self.dim, dst8.data_ptr(), scale.data_ptr(),
                                    0, 0, stream_handle(self.device), bounds.data_ptr())
                return None, None
            err = torch.empty(n, dtype=torch.float32, device=self.device)
            xtn = torch.empty(n, dtype=torch.float32, device=self.device)
            hip().quant_rows_i8(src.data_ptr(), n, self.dim, dst8.data_ptr(), scale.data_ptr(),
                                err.data_ptr(), xtn.data_ptr(), stream_handle(self.device))
            return err, xtn
        else:
            from ..ops.reference import quant_rows_i8_ref

            q8, sc, err, xtn = quant_rows_i8_ref(src)
            dst8.copy_(q8)
            scale.copy_(sc)
        if bounds is not None:
            torch.maximum(bounds[:2], torch.stack([err.max(), xtn.max()]), out=bounds[:2])
        return err, xtn

    def _store(self, r0: int, x: torch.Tensor, normalize: bool) -> None:
        """Write rows (f32 or bf16 on self.device) at r0, unit-normalising them if asked."""
        n = x.shape[0]
        dst = self.rows[r0:r0 + n]
        if self.device.type == "cuda":
            from ..ops import kernels as K

            if self.dtype == "fp8":
                K.quant_fp8(x.contiguous(), dst, FP8_SCALE, normalize)
            elif normalize:
                K.l2norm_cast(x.float().contiguous(), dst)
            else:
                dst.copy_(x)
        else:
            y = torch.nn.functional.normalize(x.float(), dim=-1) if normalize else x.float()
            if self.dtype == "fp8":
                dst.copy_((y * FP8_SCALE).to(torch.float8_e4m3fn).view(torch.uint8))
            else:
                dst.copy_(y.bfloat16())
        self.rows_written(r0, n)

    def append_f32(self, vecs: torch.Tensor) -> int:
        """Append raw float vectors (wire embeddings); normalised + cast by the l2norm_cast kernel."""
        n = vecs.shape[0]
        if vecs.shape[1] != self.dim:
            raise ValueError(f"dimension mismatch: got {vecs.shape[1]}, index is {self.dim}")
        r0 = self._reserve(n)
        self.write_f32(r0, vecs)
        self.publish()
        return r0

    def write_f32(self, r0: int, vecs: torch.Tensor) -> None:
        if r0 < self._persisted:
            self._mark_written(range(r0, min(r0 + vecs.shape[0], self._persisted)))
        self._store(r0, vecs.to(self.device, torch.float32).contiguous(), normalize=True)

    def write_rows_f32(self, rows, vecs: torch.Tensor) -> None:
        """Overwrite arbitrary existing rows (an upsert of known point ids) in ONE batched pass:
        the vectors are normalised and encoded into a scratch block by the same kernels as an
        append (with their int8 / e4m3 images), then scattered by index_copy_ -- a few launches
        per batch instead of a write per row.  ``rows`` must be distinct."""
        idx = torch.as_tensor(rows, dtype=torch.int64).flatten()
        n = idx.numel()
        if n == 0:
            return
        if vecs.shape[0] != n or vecs.shape[1] != self.dim:
            raise ValueError(f"write_rows_f32: {n} rows but vectors of shape {tuple(vecs.shape)}")
        if n == 1 or bool((idx[1:] - idx[:-1] == 1).all()):      # one contiguous range
            self.write_f32(int(idx[0]), vecs)
            return
        if int(idx.min()) < 0 or int(idx.max()) >= self.count:
            raise IndexError("write_rows_f32: row outside the shard")
        self._mark_written(idx.tolist())
        scratch = HbmIndexShard(self.dim, n, self.device, dtype=self.dtype,
                                prefilter=self.prefilter)
        scratch.append_f32(vecs)
        di = idx.to(self.device)
        self.rows.index_copy_(0, di, scratch.rows[:n])
        if self.rows8 is not None:
            self.rows8.index_copy_(0, di, scratch.rows8[:n])
        # the pruning images in THIS shard's form (its basis, its bounds), from the new rows
        self._image_rows(rows=di)

    def upsert(self, point_ids: list[str], vecs: torch.Tensor, payloads: list[Payload]) -> list[int]:
        """Qdrant-style upsert: existing ids are overwritten in place, new ids appended.  An id
        repeated inside one batch is one point and its last occurrence wins (Qdrant semantics);
        every input position gets that point's row."""
        pos = list(dedupe_last(point_ids))
        id_to_row = self.payloads.id_to_row
        new_pos = [i for i in pos if point_ids[i] not in id_to_row]
        old_pos = [i for i in pos if point_ids[i] in id_to_row]
        row_of: dict[str, int] = {}
        if new_pos:
            r0 = self.append_f32(vecs[new_pos])
            for j, i in enumerate(new_pos):
                row_of[point_ids[i]] = r0 + j
        if old_pos:
            rows = [id_to_row[point_ids[i]] for i in old_pos]
            self.write_rows_f32(rows, vecs[old_pos])
            for i, r in zip(old_pos, rows):
                row_of[point_ids[i]] = r
        for i in pos:
            self.payloads.set(row_of[point_ids[i]], point_ids[i], payloads[i])
        self.publish()
        return [row_of[pid] for pid in point_ids]

    # ------------------------------------------------------------------ deletes (tombstones)
    # ``delete_route`` a new shard starts with, per row format (profiles/r10_delete/ has the A/B,
    # 100M rows, 256 held-out queries).  bf16: "zero" keeps the pruned search at its own speed,
    # 10.9 ms against 18-21 ms for the masked scan.  fp8: both routes are the same seeded list
    # scan; "zero" is 0.1-0.8 ms ahead after uniform deletes, but after deletes by document
    # (runs of rows, what VectorStore.delete(filter=) produces) the masked scan skips the dead
    # tiles and is 1.1 ms (4.6 %) ahead at 10 % dead, so there the default is "mask"
    DELETE_ROUTE_DEFAULT = {"bf16": "zero", "fp8": "mask"}

    @property
    def live_count(self) -> int:
        """Rows that are not tombstoned (``count`` stays the physical row count)."""
        return self.count - self.n_dead

    def delete_rows(self, rows) -> int:
        """Tombstone rows; returns how many were newly deleted (duplicates and rows already
        dead are ignored, a row outside [0, count) raises IndexError).

        A deleted row is zeroed everywhere -- the bf16 / e4m3 row, the prefilter image, and the
        pruning images, re-imaged from the zero row -- and its bit is set in ``dead``.  A zero
        row scores exactly 0 in every scan and image (the quantisers guard amax > 0) and the
        tracked bounds only grow, so every unmasked route stays exact over the PHYSICAL rows;
        ``search`` then checks the returned ids against ``dead`` (_search_tombstoned).  The row's
        point id and payload go; the slot is never reused, and capacity comes back only through
        ``compact``."""
        if isinstance(rows, torch.Tensor):
            rows = rows.flatten().cpu().numpy()
        elif not isinstance(rows, np.ndarray):
            rows = list(rows)
        ra = np.unique(np.asarray(rows, dtype=np.int64))      # sorted, distinct
        if ra.size and (ra[0] < 0 or ra[-1] >= self.count):
            raise IndexError(f"delete_rows: row outside the shard's {self.count} rows")
        if self._dead_host is not None:
            ra = ra[(self._dead_host[ra >> 3] >> (ra & 7).astype(np.uint8)) & 1 == 0]
        if not ra.size:
            return 0
        if self.dead is None:
            nbytes = self.rows.shape[0] // 8     # (the slab is whole 64-row tiles)
            self.dead = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
            self._dead_host = np.zeros(nbytes, dtype=np.uint8)
        h = self._dead_host
        np.bitwise_or.at(h, ra >> 3, (1 << (ra & 7)).astype(np.uint8))
        if self.payloads.track and self._persisted:
            # a snapshot patches the zeros over the rows it covers
            self._mark_written(ra[ra < self._persisted].tolist())
        idx = torch.from_numpy(ra.astype(np.int32)).to(self.device)
        if self.device.type == "cuda":
            from ..ops import kernels as K

            K.tombstone_rows(idx, self.count, self.dead.view(torch.int64), self.rows, self.rows8)
        else:
            self.rows.index_fill_(0, idx.long(), 0)
            if self.rows8 is not None:
                self.rows8.index_fill_(0, idx.long(), 0)
            self.dead.copy_(torch.from_numpy(h))
        if self.prune_on or self.mx4_on:
            self._image_rows(rows=idx)
        # (the payload store is sparse: walk whichever of the two is shorter)
        ps = self.payloads
        if len(ps.point_ids) + len(ps.fields) < ra.size:
            gone = {r for d in (ps.point_ids, ps.fields) for r in d if (h[r >> 3] >> (r & 7)) & 1}
        else:
            gone = [r for r in ra.tolist() if r in ps.point_ids or r in ps.fields]
        for r in gone:
            ps.remove(r)
        self.n_dead += int(ra.size)
        self.dead_gen += 1
        return int(ra.size)

    def delete_points(self, point_ids) -> int:
        """Delete the points with these ids; unknown ids are ignored (as Qdrant does).  Returns
        the number of points deleted.  A later upsert of a deleted id appends a new row."""
        id_to_row = self.payloads.id_to_row
        return self.delete_rows([id_to_row[p] for p in point_ids if p in id_to_row])

    def compact(self, stage_bytes: int = COMPACT_STAGE_BYTES) -> int:
        """Reclaim the tombstoned rows: the live rows move down over them, in place and in order,
        and ``count`` drops to the live count.  Returns the rows reclaimed; without a dead row
        it returns 0 and changes nothing.

        The move follows ``compact_plan`` over the ``dead`` bitmap: a few windows, each one
        launch of compact_rows (index_compact.hip) that either writes rows straight into place
        or gathers them into a staging buffer of ``stage_bytes`` (allocated for this call, split
        by the row bytes of the slabs, at least one tile) that one copy then lays down.  A CPU
        shard runs the same plan with torch indexing.  The freed tail is zeroed (the slab's
        invariant: unwritten rows are zero), the pruning images of every sub-tile from the
        first moved row on are re-quantised from the rows (they are per sub-tile and
        fragment-major: not movable), the tracked bounds and the image's form stay (a bound over
        a superset of the rows is a bound), and the payload store is renumbered.

        Every row at or above the first dead one changes its number: the delete generation is
        bumped, so RowMasks made before are refused, ``compact_gen`` counts the compactions, and
        the next snapshot is a full one.  Searches afterwards take the unmasked route as on a
        shard that never deleted.  The caller orders this against running searches, as for any
        write."""
        if self.n_dead == 0:
            return 0
        old_count, h = self.count, self._dead_host
        gpu = self.device.type == "cuda"
        slabs = [self.rows] + ([self.rows8] if self.rows8 is not None else [])
        row_bytes = sum(t.shape[1] * t.element_size() for t in slabs)
        stage_rows = max(TILE_ROWS, int(stage_bytes) // row_bytes // TILE_ROWS * TILE_ROWS)
        c, windows = compact_plan(h, old_count, stage_rows)
        live = int(c[-1])
        b = int(np.flatnonzero(h)[0])                      # the byte of the first dead row
        first = 8 * b + (int(h[b]) & -int(h[b])).bit_length() - 1
        stage_rows = min(stage_rows, max((int(c[t1] - c[t0]) for t0, t1, m in windows
                                          if m == "staged"), default=0))
        if gpu:
            from ..ops import kernels as K

            c_dev = torch.from_numpy(c.astype(np.int32)).to(self.device)
            dead_w = self.dead.view(torch.int64)
            stages = [torch.empty(stage_rows, t.shape[1], dtype=t.dtype, device=self.device)
                      if stage_rows else None for t in slabs]
            stages += [None] * (2 - len(stages))
        else:
            bits = np.unpackbits(_dead_bytes(h, old_count), bitorder="little")[:old_count]
        for t0, t1, mode in windows:
            d0, d1 = int(c[t0]), int(c[t1])
            if d1 == d0:
                continue
            if gpu:
                staged = mode == "staged"
                K.compact_rows(dead_w, c_dev, t0, t1, old_count, self.rows,
                               stages[0] if staged else None, self.rows8,
                               stages[1] if staged else None, n_rows=d1 - d0)
                if staged:
                    for t, g in zip(slabs, stages):
                        t[d0:d1].copy_(g[:d1 - d0])
            else:
                s0, s1 = t0 * TILE_ROWS, min(t1 * TILE_ROWS, old_count)
                src = torch.from_numpy(s0 + np.flatnonzero(bits[s0:s1] == 0))
                for t in slabs:
                    t[d0:d1] = t[src]
        for t in slabs:
            t[live:old_count].zero_()
        # the images of every sub-tile from the one holding the first moved row, up to the old
        # count (the zeroed tail quantises to zero images); in the image's current form
        if self.prune_on or self.mx4_on:
            r0 = first // STREAM_SUB * STREAM_SUB
            chunk = 1 << 18
            for s in range(r0, old_count, chunk):
                self._image_rows(s, min(old_count, s + chunk) - s)
        self.payloads.remap(lambda rows: compact_new_rows(h, c, rows), live)
        self.dead.zero_()
        h[:] = 0
        self.n_dead = 0
        self.count = self.visible = live
        self.dead_gen += 1
        self._live_mask = self._live_key = None
        self.last_dead_hits = None
        self._persisted, self._dirty, self._persist_key = 0, set(), None
        self.compact_gen += 1
        self.last_compact = {
            "reclaimed": old_count - live, "first_row": first,
            "direct_windows": sum(m == "direct" for _, _, m in windows),
            "staged_windows": sum(m == "staged" for _, _, m in windows),
            "rows_moved": live - first}
        return old_count - live

    def _live(self) -> RowMask:
        """The RowMask of the rows that are not tombstoned: ~dead over the packed words (no bool
        per row), with its tile list; rebuilt when a delete or the visible rows changed."""
        key = (self.dead_gen, self.visible)
        if self._live_mask is None or self._live_key != key:
            v = self.visible
            nw = max(1, (v + TILE_ROWS - 1) // TILE_ROWS)
            words = ~self.dead.view(torch.int64)[:nw]
            if v < nw * 64:      # bits at or past ``visible`` are clear in a RowMask
                words[v // 64:v // 64 + 1].bitwise_and_((1 << (v % 64)) - 1)
            tiles = n_live = None
            if self.device.type == "cuda" and self._mask_tiles_wanted():
                from ..ops.kernels import filter_tiles

                tiles, n_live = filter_tiles(words, v)
            self._live_mask = RowMask(words.view(torch.uint8), v, tiles, n_live, self.dead_gen)
            self._live_key = key
        return self._live_mask

    def _all_rows(self) -> RowMask:
        """The RowMask that allows every visible row, with its tile list: what the unmasked fp8
        search at 32 < k <= 128 runs the masked emitting scan under (on fp8 a masked and an
        unmasked search are the same list scan).  Built once per number of visible rows.
        Internal: it ignores tombstones and is never checked against ``dead_gen``."""
        v = self.visible
        cached = self._all_rows_mask
        if cached is None or cached.visible != v:
            nw = max(1, (v + TILE_ROWS - 1) // TILE_ROWS)
            words = torch.full((nw,), -1, dtype=torch.int64, device=self.device)
            if v < nw * 64:      # bits at or past ``visible`` are clear in a RowMask
                words[v // 64:v // 64 + 1].bitwise_and_((1 << (v % 64)) - 1)
            tiles = n_live = None
            if self.device.type == "cuda":
                from ..ops.kernels import filter_tiles

                tiles, n_live = filter_tiles(words, v)
            cached = self._all_rows_mask = RowMask(words.view(torch.uint8), v, tiles, n_live,
                                                   self.dead_gen)
        return cached

    def fill_random(self, n: int, seed: int = 0, chunk: int = 1 << 20) -> None:
        """Synthetic unit rows straight into HBM (benchmark corpus; no payloads)."""
        g = torch.Generator(device=self.device)
        g.manual_seed(seed)
        r0 = self._reserve(n)
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            x = torch.randn(e - s, self.dim, generator=g, device=self.device, dtype=torch.float32)
            self._store(r0 + s, x, normalize=True)
        self.publish()

    # ------------------------------------------------------------------ search
    def search(self, q_unit: torch.Tensor, k: int, n_cus: int | None = None, *, allow=None):
        """Top-k cosine over this shard for unit bf16 queries [NQ, D].

        ``allow`` (a ``RowMask``, or anything ``make_mask`` takes): only those rows may be
        returned; the search is exact over them (_search_masked).

        Tombstoned rows (``delete_rows``) are never returned (_search_tombstoned).

        On a bf16 GPU shard of width 384 / 768 / 1024 both run on the HIP scans up to k = 128
        (k <= 32: the masked list scan; above: the masked emitting scan); beyond that, and on
        shards those scans do not serve, they take the chunked matmul under the mask.  A GPU fp8
        shard (256 / 384 / 512 / 768 / 1024) has the e4m3 forms of both: the list scan at
        k <= 32, and at 32 < k <= 128, from FP8_LARGE_K_MIN_ROWS visible rows on, the emitting
        e4m3 scan -- unmasked searches too, under an all-ones mask.  Every HIP route of an fp8
        shard scores e4m3(q) . e4m3(x); its matmul (smaller shards at k > 32, k > 128) scores
        float(q) . decode(x).

        ``allow`` may also be a ``MaskGroups`` (``make_mask_groups``): a mask per query, each
        query exact over its own mask's rows (_search_grouped).

        Returns (scores f32 [NQ, k], rows int32 [NQ, k]); missing slots are (-inf, -1)."""
        if isinstance(allow, MaskGroups):
            return self._search_grouped(q_unit, k, n_cus, allow)
        if allow is not None:
            return self._search_masked(q_unit, k, n_cus, allow)
        if self.n_dead == 0:
            return self._search_route(q_unit, k, n_cus)
        return self._search_tombstoned(q_unit, k, n_cus)

    def _search_route(self, q_unit: torch.Tensor, k: int, n_cus):
        """The unmasked search, exact over every physical row (zeroed tombstones included)."""
        NQ = q_unit.shape[0]
        k = int(k)
        if NQ == 0 or k <= 0:
            return (torch.empty(NQ, max(k, 0), device=self.device),
                    torch.empty(NQ, max(k, 0), dtype=torch.int32, device=self.device))
        if self.device.type != "cuda" or k > self.K_MAX_HIP:
            return self._search_matmul(q_unit, k)
        q_unit = q_unit.to(torch.bfloat16).contiguous()
        if self.prefilter and k < 32:
            return self._search_prefilter(q_unit, k, n_cus)
        if k > 16:
            # exact over the bf16 rows (a prefilter shard keeps them too): the large-k emitting
            # scan, else the list scan up to its kmax = 32, else the chunked GEMM
            out = self._search_large_k(q_unit, k, n_cus)
            if out is not None:
                return out
            if k > 32 and self.dtype == "fp8" and self._filter_large_k_serves(k):
                # an fp8 shard of FP8_LARGE_K_MIN_ROWS rows or more: the emitting e4m3 scan
                # under the all-ones mask (masked and unmasked are one list scan on fp8)
                return self._search_filtered_large_k(q_unit, k, self._all_rows(), n_cus)
            if k > 32:
                return self._search_matmul(q_unit, k)
        if self.prune and k <= 16 and NQ >= self.prune_min_nq and self._seed_rows(self.visible, k):
            out = self._search_pruned(q_unit, k, n_cus)
            if out is not None:
                return out
        out_s, out_i = self._search_scan(q_unit, k, self.rows, self.dtype, n_cus)
        if self.dtype == "fp8":
            out_s.mul_(1.0 / (FP8_SCALE * FP8_SCALE))
        return out_s, out_i

    def _zero_route_serves(self, NQ: int, k: int) -> bool:
        """A search over tombstones runs the unmasked route plus the gated masked scan (else:
        the masked scan or the masked matmul, directly)."""
        return (self.delete_route == "zero" and self.device.type == "cuda" and NQ > 0
                and ((0 < k <= 32 and self._filter_scan_serves())
                     or self._filter_large_k_serves(k)))

    def _search_tombstoned(self, q_unit: torch.Tensor, k: int, n_cus):
        """``search`` on a shard with tombstones, exact over the live rows, no host sync.

        Every unmasked route is exact over the physical rows, and a dead row is a zero row there
        (delete_rows).  If the top-k over that superset holds no dead row it IS the top-k over
        the live rows, so: run the route unchanged, count the returned ids that are dead into a
        device flag (results_dead), and enqueue the exact masked scan under the live mask (the
        list scan at k <= 32, the emitting scan of _search_filtered_large_k at 32 < k <= 128)
        gated on that flag -- with no hit its launches exit at once -- then take
        where(hit, fallback, route).  No hit is the only outcome while every query has at least
        k live rows scoring above 0, so each route keeps its own speed after deletes.
        ``delete_route = "mask"`` goes straight to the masked scan; CPU shards, k > 128, fp8
        shards below FP8_LARGE_K_MIN_ROWS rows at k > 32 and widths no masked scan serves take
        the masked matmul.  On a larger fp8 shard at 32 < k <= 128 the route under "zero" is the
        emitting e4m3 scan under the all-ones mask and the fallback the same scan under the live
        mask."""
        NQ, k = q_unit.shape[0], int(k)
        if NQ == 0 or k <= 0:
            return self._search_route(q_unit, k, n_cus)
        live = self._live()
        large_k = self._filter_large_k_serves(k)
        if self.device.type != "cuda" or not (large_k or (k <= 32 and self._filter_scan_serves())):
            self.last_dead_hits = None
            return self._search_matmul(q_unit, k, mask=live)
        q = q_unit.to(torch.bfloat16).contiguous()
        if self.delete_route != "zero":
            if self._zero_hits is None:
                self._zero_hits = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.last_dead_hits = self._zero_hits
            if large_k:
                return self._search_filtered_large_k(q, k, live, n_cus)
            return self._search_filtered(q, k, live, n_cus)
        out_s, out_i = self._search_route(q, k, n_cus)
        return self._dead_fallback(q, k, n_cus, live, out_s, out_i)

    def _dead_fallback(self, q, k: int, n_cus, live: RowMask, out_s, out_i):
        """The dead-id check of a route's result and the gated exact fallback (its own
        buffers: garbage while the flag is 0, never selected then)."""
        from ..ops import kernels as K

        hit = torch.zeros(1, dtype=torch.int32, device=self.device)
        K.results_dead(out_i.contiguous(), self.dead.view(torch.int64), hit)
        masked = self._search_filtered_large_k if k > 32 else self._search_filtered
        fb_s, fb_i = masked(q, k, live, n_cus, gate=hit)
        self.last_dead_hits = hit
        take = hit > 0
        return torch.where(take, fb_s, out_s), torch.where(take, fb_i, out_i)

    def search_begin(self, q_unit: torch.Tensor, k: int, n_cus: int | None = None, *,
                     allow=None) -> dict:
        """First half of ``search`` for a pipelined caller: on the pruned path, the query-side
        work (int8 queries, exact sample, thresholds, route) runs now on the current stream and
        ``search_end`` runs the full-shard scan later, possibly on another stream -- the bench
        overlaps batch i + 1's begin with batch i's scan.  Any other path (a masked search
        among them) runs whole here."""
        if allow is not None:
            return {"full": self.search(q_unit, k, n_cus, allow=allow)}
        q = q_unit.to(torch.bfloat16).contiguous()
        k = int(k)
        tomb = self.n_dead > 0
        if tomb and not self._zero_route_serves(q.shape[0], k):
            return {"full": self.search(q_unit, k, n_cus)}
        if (self.device.type == "cuda" and self.prune and not self.prefilter and 0 < k <= 16
                and q.shape[0] >= self.prune_min_nq and self._seed_rows(self.visible, k)):
            ctx = self._pruned_begin(q, k, n_cus, split=True)
            if ctx is not None:
                if tomb:   # search_end checks the result against the live mask of THIS begin
                    ctx["live"] = self._live()
                return ctx
        return {"full": self.search(q, k, n_cus)}

    def search_end(self, ctx: dict):
        """-> (scores f32 [NQ, k], rows int32 [NQ, k]) of a ``search_begin`` context."""
        if "full" in ctx:
            return ctx["full"]
        out_s, out_i = self._pruned_end(ctx)
        live = ctx.get("live")
        if live is None:
            return out_s, out_i
        return self._dead_fallback(ctx["q"], ctx["k"], ctx["n_cus"], live, out_s, out_i)

    # ------------------------------------------------------------------ search under a row mask
    # seed pass of the masked scan on by default?  (profiles/r8_filter/ has the A/B)
    FILTER_SEED_DEFAULT = True
    FILTER_SEED_STRIDE = 64
    # row-block floor of the masked scan's grid, in 64-row tiles (smaller than the unmasked list
    # scan's 16: under a sparse mask most of a block's tiles are dead; not tuned)
    FILTER_MIN_TILES = 4

    def make_mask(self, allow) -> RowMask:
        """Rows a search may return -> ``RowMask`` at the rows visible now.  ``allow`` is one of

        * a bool tensor / array of length up to ``visible`` (shorter: the rest is disallowed);
        * a list / int tensor / int array of row numbers (each in [0, visible));
        * the packed bits themselves: ``bytes`` or a uint8 tensor / array, bit r % 8 of byte
          r // 8 = row r (numpy.packbits(bitorder="little")); bits at or past ``visible`` are
          cleared.

        A device tensor is packed on the device without a host sync (row numbers outside the
        shard are then dropped instead of refused).  On a GPU shard the masked scan serves, the
        live-tile list is built here, once (``filter_tiles``)."""
        if isinstance(allow, RowMask):
            return allow
        v, dev = self.visible, self.device
        if isinstance(allow, (bytes, bytearray, memoryview)):
            allow = torch.frombuffer(bytearray(allow), dtype=torch.uint8)
        on_dev = isinstance(allow, torch.Tensor) and allow.device.type != "cpu"
        if isinstance(allow, (list, tuple, range)):
            allow = torch.tensor(list(allow), dtype=torch.int64)
        a = torch.as_tensor(allow).flatten()
        if a.dtype == torch.bool:
            if a.numel() > v:
                raise ValueError(f"make_mask: {a.numel()} mask entries for {v} visible rows")
            ok = a.to(dev)
        elif a.dtype == torch.uint8:
            ok = _unpack_bits(a.to(dev))[:v]
        elif a.dtype in (torch.int16, torch.int32, torch.int64):
            if not on_dev and a.numel() and (int(a.min()) < 0 or int(a.max()) >= v):
                raise IndexError(f"make_mask: row outside the {v} visible rows")
            r = a.to(dev, torch.int64)
            hit = torch.zeros(v + 1, dtype=torch.bool, device=dev)
            hit[torch.where((r >= 0) & (r < v), r, torch.full_like(r, v))] = True
            ok = hit[:v]
        else:
            raise TypeError(f"make_mask: bool mask, int rows or packed uint8 bits, got {a.dtype}")
        nw = max(1, (v + TILE_ROWS - 1) // TILE_ROWS)
        bits = _pack_bits(ok, nw)
        if self.n_dead:      # a tombstoned row passes no mask
            bits = (bits.view(torch.int64) & ~self.dead.view(torch.int64)[:nw]).view(torch.uint8)
        tiles = n_live = None
        if dev.type == "cuda" and self._mask_tiles_wanted():
            from ..ops.kernels import filter_tiles

            tiles, n_live = filter_tiles(bits.view(torch.int64), v)
        return RowMask(bits, v, tiles, n_live, self.dead_gen)

    def _filter_scan_serves(self) -> bool:
        """A masked list scan exists for this shard's row format and width."""
        return ((self.dtype == "bf16" and self.dim in FILTER_DIMS)
                or (self.dtype == "fp8" and self.dim in FILTER_FP8_DIMS))

    def _filter_large_k_serves(self, k: int) -> bool:
        """The masked emitting scan serves a search at this k, 32 < k <= K_MAX_HIP: a bf16 shard
        on a GPU at a width in FILTER_LARGE_K_DIMS with the emitting scan on, or an fp8 shard on
        a GPU at a width in FILTER_LARGE_K_FP8_DIMS with FP8_LARGE_K_MIN_ROWS visible rows or
        more (below them the matmul costs milliseconds)."""
        if self.device.type != "cuda" or not 32 < k <= self.K_MAX_HIP:
            return False
        if self.dtype == "fp8":
            return (self.dim in FILTER_LARGE_K_FP8_DIMS
                    and self.visible >= self.FP8_LARGE_K_MIN_ROWS)
        return (self.dtype == "bf16" and bool(self.scan_mq) and self.dim in FILTER_LARGE_K_DIMS)

    def _mask_tiles_wanted(self) -> bool:
        """Some masked scan of this shard walks a RowMask's live-tile list."""
        return self._filter_scan_serves() or self._filter_large_k_serves(self.K_MAX_HIP)

    def _empty_result(self, NQ: int, k: int):
        """The result of a search with no queries or k <= 0."""
        return (torch.empty(NQ, max(k, 0), device=self.device),
                torch.empty(NQ, max(k, 0), dtype=torch.int32, device=self.device))

    def _refuse_stale(self, device, dead_gen: int) -> None:
        """Refuse a RowMask (or MaskGroups) of another device or from before a delete."""
        if device != self.device:
            raise ValueError(f"RowMask on {device}, shard on {self.device}")
        if dead_gen != self.dead_gen:
            raise ValueError("RowMask made before a delete (it may allow a deleted row): make "
                             "it again with make_mask")

    def _search_masked(self, q_unit, k: int, n_cus, allow):
        """``search`` under a row mask, exact over the allowed rows.  A GPU shard at k <= 32 takes
        the masked list scan of its row format (bf16 at a width in FILTER_DIMS, fp8 at one in
        FILTER_FP8_DIMS); at 32 < k <= 128 a bf16 GPU shard at a width in FILTER_LARGE_K_DIMS, and
        an fp8 one at a width in FILTER_LARGE_K_FP8_DIMS with FP8_LARGE_K_MIN_ROWS visible rows or
        more, the masked emitting scan (_search_filtered_large_k); everything else (CPU shards,
        k > 128, smaller fp8 shards at k > 32, other widths) the chunked matmul
        with the score block masked.  On an fp8 shard both scans score e4m3(q) . e4m3(x), as
        the unmasked GPU search does; the matmul scores float(q) . decode(x).  The cheap routes of
        the unmasked search do not apply: their thresholds come from a sample of ALL rows, which
        is no lower bound on the k-th allowed score."""
        NQ = q_unit.shape[0]
        k = int(k)
        if NQ == 0 or k <= 0:
            return self._empty_result(NQ, k)
        mask = self.make_mask(allow)
        self._refuse_stale(mask.bits.device, mask.dead_gen)
        if (self.device.type == "cuda" and self._filter_scan_serves() and k <= 32
                and mask.tiles is not None):
            return self._search_filtered(q_unit.to(torch.bfloat16).contiguous(), k, mask, n_cus)
        if self._filter_large_k_serves(k) and mask.tiles is not None:
            return self._search_filtered_large_k(q_unit.to(torch.bfloat16).contiguous(), k, mask,
                                                 n_cus)
        return self._search_matmul(q_unit, k, mask=mask)

    # ------------------------------------------------------------------ a row mask per query
    # distinct masks from which a search takes the grouped scan instead of one masked search
    # per mask (README, round 14, has the measurement behind it)
    GROUP_SCAN_MIN_GROUPS = 2

    def make_mask_groups(self, masks, group_of) -> MaskGroups:
        """Masks and each query's mask -> ``MaskGroups``.  ``masks``: a sequence whose entries
        are anything ``make_mask`` takes; ``group_of``: for each query of the searches to come,
        the index into ``masks`` of the mask it runs under.  Entries that are the same object,
        or RowMasks with equal bits, merge into one group (groups no query names are dropped).
        All masks must be of this shard at one ``visible`` and delete generation."""
        masks = list(masks)
        group_of = [int(g) for g in (group_of.tolist() if hasattr(group_of, "tolist")
                                     else group_of)]
        if not masks:
            raise ValueError("make_mask_groups: no masks")
        if any(g < 0 or g >= len(masks) for g in group_of):
            raise IndexError(f"make_mask_groups: group outside the {len(masks)} masks")
        by_obj: dict = {}
        made = []
        for m in masks:
            if id(m) not in by_obj:
                by_obj[id(m)] = self.make_mask(m)
            made.append(by_obj[id(m)])
        for m in made:
            self._refuse_stale(m.bits.device, m.dead_gen)
            if m.visible != made[0].visible or m.bits.numel() != made[0].bits.numel():
                raise ValueError("make_mask_groups: masks made at different visible rows")
        # merge: the same RowMask object first, then equal bits (one unique over the distinct
        # objects' words, reordered to first appearance)
        distinct, slot_of = [], {}
        for g in group_of:
            m = made[g]
            if id(m) not in slot_of:
                slot_of[id(m)] = len(distinct)
                distinct.append(m)
        if len(distinct) > 1:
            inv = torch.unique(torch.stack([m.words for m in distinct]), dim=0,
                               return_inverse=True)[1].tolist()
            first: dict = {}
            merged, remap = [], []
            for j, u in enumerate(inv):
                if u not in first:
                    first[u] = len(merged)
                    merged.append(distinct[j])
                remap.append(first[u])
        else:
            merged, remap = distinct, [0] * len(distinct)
        if not merged:      # no queries: keep the first mask so the object stays usable
            merged = [made[0]]
        return MaskGroups(merged, [remap[slot_of[id(made[g])]] for g in group_of])

    def _group_scan_serves(self, k: int, groups: MaskGroups) -> bool:
        """The grouped masked list scan serves this search (bf16: index_filter_group.hip; fp8:
        index_filter_group_fp8.hip, built at every width and both kmax of the single-mask fp8
        scan)."""
        return (self.device.type == "cuda" and 0 < k <= 32
                and len(groups) >= self.GROUP_SCAN_MIN_GROUPS and self._filter_scan_serves())

    def _group_large_k_serves(self, k: int, groups: MaskGroups) -> bool:
        """The grouped emitting e4m3 scan (index_emit_group_fp8.hip) serves this search: an fp8
        shard the single-mask emitting scan serves at this k (_filter_large_k_serves: its
        FP8_LARGE_K_MIN_ROWS gate too, below which the per-mask loop's matmul keeps the search)
        with GROUP_SCAN_MIN_GROUPS masks or more."""
        return (self.dtype == "fp8" and len(groups) >= self.GROUP_SCAN_MIN_GROUPS
                and self._filter_large_k_serves(k))

    def _search_grouped(self, q_unit, k: int, n_cus, groups: MaskGroups):
        """``search`` under a mask per query, each query exact over its own mask's rows.

        * One distinct mask: ``_search_masked`` under it, unchanged.
        * A GPU shard at k <= 32 with GROUP_SCAN_MIN_GROUPS masks or more -- bf16 of width
          384 / 768 / 1024, or fp8 of width 256 / 384 / 512 / 768 / 1024: the grouped masked list
          scan of its row format, one scan of the union's live tiles per chunk of up to 8 masks
          over that chunk's queries (_search_group_chunk).  It scores bf16(q) . bf16(x), on fp8
          e4m3(q) . e4m3(x), with the MFMA chain of the single-mask scan, bit for bit alike.
          (A chunk of two to four large disjoint masks whose queries grouping would spread
          over one more query block stays with the next route: _loop_keeps_chunk.)
        * A GPU fp8 shard of FP8_LARGE_K_MIN_ROWS visible rows or more at 32 < k <= 128 with
          GROUP_SCAN_MIN_GROUPS masks or more: per chunk, the grouped list scan as the seed
          passes and the grouped emitting e4m3 scan (_search_group_chunk_large_k), under the
          same _loop_keeps_chunk rule.  A chunk whose candidates overflow LARGE_K_CAP goes to
          the next route.
        * Everything else: one ``_search_masked`` per mask over its queries, scattered back.
          Those are the existing routes, exact as they stand: a CPU shard, k > 128, other
          widths and small fp8 shards at k > 32 score float(q) . float(x) (fp8:
          float(q) . decode(x)) in the masked matmul; a GPU fp8 shard's emitting scan
          (32 < k <= 128) scores e4m3(q) . e4m3(x); a bf16 GPU shard at 32 < k <= 128 takes the
          masked emitting scan, bf16(q) . bf16(x).

        Tombstones need nothing here: ``make_mask`` clears them in every mask, and a
        ``MaskGroups`` from before a later delete is refused as a RowMask is."""
        NQ = q_unit.shape[0]
        k = int(k)
        if len(groups.group_of) != NQ:
            raise ValueError(f"MaskGroups for {len(groups.group_of)} queries, search has {NQ}")
        self._refuse_stale(groups.device, groups.dead_gen)
        if NQ == 0 or k <= 0:
            return self._empty_result(NQ, k)
        if len(groups) == 1:
            return self._search_masked(q_unit, k, n_cus, groups.masks[0])
        out_s = torch.empty(NQ, k, device=self.device)
        out_i = torch.empty(NQ, k, dtype=torch.int32, device=self.device)
        def loop(g0, g1):
            for g in range(g0, g1):
                idx = torch.tensor(groups.queries_of(g), dtype=torch.int64, device=self.device)
                s, i = self._search_masked(q_unit[idx], k, n_cus, groups.masks[g])
                out_s[idx], out_i[idx] = s, i.to(torch.int32)

        large_k = self._group_large_k_serves(k, groups)
        if large_k or self._group_scan_serves(k, groups):
            q = q_unit.to(torch.bfloat16).contiguous()
            if self.dtype == "fp8":
                # e4m3 bytes, once per search (as _search_filtered quantises them per mask)
                from ..ops.kernels import quant_fp8

                q = quant_fp8(q, scale=FP8_SCALE)
            for c in range(groups.n_chunks):
                ch = groups.chunk(c)
                if self._loop_keeps_chunk(ch, k):
                    loop(ch["groups"][0], sum(ch["groups"]))
                    continue
                if large_k:
                    res = self._search_group_chunk_large_k(q[ch["idx"]], k, groups, ch, n_cus)
                    if res is None:     # candidates past LARGE_K_CAP: the parent's route, exact
                        loop(ch["groups"][0], sum(ch["groups"]))
                        continue
                    s, i = res
                else:
                    s, i = self._search_group_chunk(q[ch["idx"]], k, groups, ch, n_cus)
                out_s[ch["idx"]], out_i[ch["idx"]] = s, i
            return out_s, out_i
        loop(0, len(groups))
        return out_s, out_i

    # The measured case the per-mask loop keeps (README, round 14): a chunk of two to four masks
    # whose tiles are disjoint, on a width where each group's queries fit one query block but
    # all of them together need two (768 / 1024 above 128 queries).  The loop then walks each
    # mask's tiles once with one block; the grouped scan walks the union with both blocks, half
    # of it for nothing.  At 50M x 768 under disjoint 1 % document masks the two tied at 2 and 4
    # groups (0.713 / 1.317 against 0.709 / 1.347 ms in one run, 0.688 / 1.325 against
    # 0.689 / 1.310 in the next; 20 263 / 39 986 union tiles), the scan led by 5-6 % at 8 groups
    # in both, and by 2.1x at 2 052 union tiles, where the launches dominate: the tile floor
    # sits between 2 052 and 20 263.  An fp8 shard has 256 queries per block at every width, so
    # its case starts above 256 queries; there the scan does not tie but lose (README, round 15:
    # 100M rows, 512 queries, disjoint 1 % masks, 2 / 4 groups: 1.571 / 2.819 against the loop's
    # 1.042 / 1.898 ms at 1024, 1.019 / 1.702 against 0.741 / 1.361 at 384), so the same
    # constants serve it; 8 groups and the tile floor are unmeasured on fp8.
    #
    # At 32 < k <= 128 (the grouped emitting scan of an fp8 shard; README, round 16) the same
    # case was measured at k = 100 with the scan forced, 100M rows, 512 queries, disjoint 1 %
    # masks, 2 / 4 groups, scan against loop (its min-max): at 1024 2.306 against 2.125
    # (2.124-2.128) and 3.704 against 3.676 (3.653-3.680) ms, behind and tied, so the rule holds
    # there; at 384 1.798 against 1.904 (1.893-1.915) and 2.584 against 3.406 (3.401-3.419),
    # ahead by more than the loop's spread (at this k a masked search is three launches and a
    # select, and the scan saves them per mask), so 384 is exempt.  256 / 512 / 768 are
    # unmeasured and keep the rule: the loop is what the parent of that change did everywhere.
    GROUP_LOOP_MAX_GROUPS = 4
    GROUP_LOOP_MIN_TILES = 16384
    GROUP_LOOP_LARGE_K_SCAN_DIMS = (384,)

    def _loop_keeps_chunk(self, ch: dict, k: int) -> bool:
        live = ch["live"]
        if live is None or not 2 <= len(ch["nq_of"]) <= self.GROUP_LOOP_MAX_GROUPS:
            return False
        if k > 32 and self.dim in self.GROUP_LOOP_LARGE_K_SCAN_DIMS:
            return False
        # queries per block of the list scans (256 on fp8: the rule can then hold above 256
        # queries only)
        qpb = self._masked_format()[0](16 if k <= 16 else 32)[1]
        blocks = lambda nq: (nq + qpb - 1) // qpb
        union = live[-1]
        return (blocks(sum(ch["nq_of"])) > max(blocks(nq) for nq in ch["nq_of"])
                and union >= self.GROUP_LOOP_MIN_TILES and union >= 0.9 * sum(live[:-1]))

    # ------------------------------------------------------------------ the masked scans' bodies
    # One list-scan body and one large-k body serve every masked route.  They take what differs
    # between the routes as values: the kernels (_masked_kernels), the mask operands the
    # wrappers take between ``n_valid`` and the queries -- (words, tiles, n_live) of a RowMask,
    # (mask8, qgroup, tiles, n_live) of a MaskGroups chunk -- the queries as the kernels read
    # them, and the row format's own numbers (_masked_format).
    def _masked_kernels(self, grouped: bool):
        """(list scan, emitting scan) of this shard's row format, under one mask or a mask per
        query (bf16 has no grouped emitting scan)."""
        if self.dtype == "fp8":
            return ((K.index_scan_filter_group_fp8, K.index_scan_emit_group_fp8) if grouped
                    else (K.index_scan_filter_fp8, K.index_scan_emit_fp8))
        return ((K.index_scan_filter_group, None) if grouped
                else (K.index_scan_filter, K.index_scan_mq_filter))

    def _masked_format(self):
        """What the masked bodies take from the row format, (geometry, emit_form, threshold,
        rescale): ``geometry(kmax)`` -> (lists, queries per block) of the list scan;
        ``emit_form(NQ)`` -> (queries per block, extra arguments) of the emitting scan;
        ``threshold(cand_s, k)`` -> T from a seed pass's candidates; ``rescale``: the factor
        from raw scores to cosines, or None."""
        if self.dtype == "fp8":
            # 2 lists and 256 queries per block at every width and kmax.  All e4m3 kernels run
            # one MFMA chain, so a row's raw score (S^2 * cosine) is the same bits in each: T is
            # the k-th largest finite raw candidate less one ulp, with no margin.
            return (lambda kmax: (2, 256), lambda NQ: (256, ()), filter_large_k_threshold_ulp,
                    1.0 / (FP8_SCALE * FP8_SCALE))
        h = hip()

        def emit_form(NQ):
            form = self._mq_filter_form(NQ)
            return h.mq_queries_per_blk(*form), form

        # (MQ_THR_MARGIN: the list scan and the emitting scan sum in different orders)
        return (lambda kmax: h.topk_geometry(self.dim, kmax), emit_form,
                lambda cand_s, k: filter_large_k_threshold(cand_s, k, self.MQ_THR_MARGIN), None)

    def _masked_queries(self, q_unit, visible: int):
        """The queries as this shard's masked scans read them: bf16 as they are; on an fp8 shard
        their e4m3 bytes (an empty search launches nothing, this neither)."""
        if self.dtype != "fp8" or min(visible, self.visible) <= 0:
            return q_unit
        return K.quant_fp8(q_unit, scale=FP8_SCALE)

    def _masked_rblk(self, n: int, NQ: int, qpb: int, n_cus) -> int:
        """Row slots per query block of a masked scan's grid: the CUs shared among the query
        blocks, with FILTER_MIN_TILES tiles or more to a slot."""
        if n_cus is None:
            n_cus = self._n_cus()
        return max(1, min(math.ceil(n / (TILE_ROWS * self.FILTER_MIN_TILES)),
                          max(1, round(n_cus / math.ceil(NQ / qpb)))))

    def _masked_list_scan(self, scan, visible: int, operands: tuple, q, k: int, n_cus, gate=None):
        """The masked list scan ``scan`` + merge, k <= 32, over the rows below ``visible`` that
        ``operands`` allow.  The grid and the candidate workspace are sized as if every tile
        were live; the kernel reads the live count on the device.  ``filter_seed``: a first pass
        over every FILTER_SEED_STRIDE-th live tile of each workgroup's slice sees allowed rows
        only (under a mask per query: rows of that query's own mask), so its k-th best is a
        lower bound on the final k-th allowed score (-inf where it found fewer than k rows); the
        full pass starts from it.  Exact either way.  ``gate`` (int32 device flag): every scan
        and merge launch runs only if it is non-zero (the outputs are then left unwritten; the
        torch glue between the passes runs on whatever they hold).  Raw e4m3 scores are rescaled
        once at the end."""
        h, dev = hip(), self.device
        NQ = q.shape[0]
        kmax = 16 if k <= 16 else 32
        n = min(visible, self.visible)
        out_s = torch.empty(NQ, k, device=dev)
        out_i = torch.empty(NQ, k, dtype=torch.int32, device=dev)
        if n <= 0:
            return out_s.fill_(-math.inf), out_i.fill_(-1)
        geometry, _, _, rescale = self._masked_format()
        lists, qpb = geometry(kmax)
        n_rblk = self._masked_rblk(n, NQ, qpb, n_cus)
        ncand = n_rblk * lists * kmax
        cs = torch.empty(NQ, ncand, device=dev)
        ci = torch.empty(NQ, ncand, dtype=torch.int32, device=dev)
        st = stream_handle(dev)

        def one_pass(thr, stride):
            scan(self.rows, n, *operands, q, kmax, n_rblk, cs, ci, thr, stride, self.scan_xcd,
                 gate)
            h.topk_merge(cs.data_ptr(), ci.data_ptr(), NQ, ncand, kmax, k, out_s.data_ptr(),
                         out_i.data_ptr(), 0, 0, st, 0 if gate is None else gate.data_ptr())

        thr = None
        if self.filter_seed:
            one_pass(None, self.FILTER_SEED_STRIDE)
            kth = out_s[:, k - 1].contiguous()
            thr = torch.nextafter(kth, torch.full_like(kth, -math.inf))
        one_pass(thr, 1)
        if rescale is not None:
            out_s.mul_(rescale)   # (-inf stays -inf)
        return out_s, out_i

    def _search_filtered(self, q_unit, k: int, mask: RowMask, n_cus, gate=None):
        """The masked list scan + merge under one RowMask (index_filter.hip; index_filter_fp8.hip
        on an fp8 shard, whose queries are quantised to e4m3 here)."""
        return self._masked_list_scan(
            self._masked_kernels(False)[0], mask.visible, (mask.words, mask.tiles, mask.n_live),
            self._masked_queries(q_unit, mask.visible), k, n_cus, gate)

    def _search_group_chunk(self, q_unit, k: int, groups: MaskGroups, ch: dict, n_cus):
        """The grouped masked list scan + merge over one chunk's queries: the chunk's eight mask
        words per tile and the union's live-tile list.  On an fp8 shard ``q_unit`` holds the
        queries' e4m3 bytes (quantised once per search by _search_grouped)."""
        return self._masked_list_scan(
            self._masked_kernels(True)[0], groups.visible,
            (ch["mask8"], ch["qgroup"], ch["tiles"], ch["n_live"]), q_unit, k, n_cus)

    # seed pass of the masked large-k search: every S-th live tile of each workgroup's slice.
    # 32 is the unmasked route's sample rate (PRUNE_TILE_SHIFT = 5).  A query emits about k * S
    # candidates (at most 1.3 k * S over 256 queries): at 100M x 384, k = 100, S = 64 is 6 %
    # faster on the all-ones mask with 1.9x of head room to LARGE_K_CAP instead of 3.5x, and
    # S = 128 overflows into the matmul (profiles/r11_filter_largek/ has the A/B).
    FILTER_LARGE_K_STRIDE = 32
    # the seed pass's own seed: every 16th tile of its sample (1: off).  100M x 384, k = 100:
    # all-ones mask 21.6 -> 18.1 ms, documents 10 % 3.13 -> 2.73, uniform 1 % 8.51 -> 8.72 (the
    # extra launch where the lists hardly fill); same T, same candidates (profiles/r11_filter_largek/)
    FILTER_LARGE_K_COARSE = 16

    def _mq_filter_form(self, NQ: int):
        """(sets, rsplit) of the masked emitting scan: _mq_form's, except that at D = 384 below
        512 queries it is always the row-split form (there is no masked (2, 1) form)."""
        if self.dim != 384:
            return (2 if self.dim == 768 else 1), 1
        return (4, 1) if NQ >= 512 else (4, 2)

    def _masked_large_k(self, scan, emit, visible: int, operands: tuple, q, k: int, n_cus,
                        gate=None, seed: bool = True):
        """EXACT top-k for 32 < k <= 128 over the rows below ``visible`` that ``operands``
        allow, at any number of visible rows; ``scan`` / ``emit``: the masked list scan and the
        masked emitting scan of the row format (_masked_kernels).

        1. T[q], a lower bound on query q's final k-th ALLOWED score from allowed rows only: the
           list scan (kmax 32) over every FILTER_LARGE_K_STRIDE-th live tile of each workgroup's
           slice leaves [NQ, n_rblk * lists * 32] candidates, each a distinct allowed row's real
           score (under a mask per query: a row of that query's own mask), and T is the k-th
           largest finite one (-inf below k of them: a mask with few allowed rows emits every
           one), less what the format's two kernels may differ by (_masked_format).  On shards
           of SEED_MIN_ROWS rows or more that pass is itself seeded, by a kmax = 16 pass over
           every FILTER_LARGE_K_COARSE-th tile of its sample, which changes its time and not T.
           ``seed=False``: T = -inf.
        2. the emitting scan over the whole list keeps every allowed row above T in LARGE_K_CAP
           slots per query, and the radix select takes the top k: descending, (-inf, -1) past
           the allowed rows.  Raw e4m3 scores are rescaled once, after the select.
        3. a query whose candidates overflow the cap raises the select's flag (read back once,
           as _search_large_k reads its own): the body then returns None, and its caller
           answers by a route without a cap.

        ``gate`` (int32 device flag): every launch runs only if it is non-zero; at 0 the
        overflow flag stays 0 and the outputs hold garbage the caller never selects."""
        h, dev = hip(), self.device
        NQ = q.shape[0]
        n = min(visible, self.visible)
        out_s = torch.empty(NQ, k, device=dev)
        out_i = torch.empty(NQ, k, dtype=torch.int32, device=dev)
        if n <= 0:
            return out_s.fill_(-math.inf), out_i.fill_(-1)
        geometry, emit_form, threshold, rescale = self._masked_format()
        if seed:
            lists, qpb = geometry(32)
            n_rblk = self._masked_rblk(n, NQ, qpb, n_cus)
            cs = torch.empty(NQ, n_rblk * lists * 32, device=dev)
            ci = torch.empty(NQ, n_rblk * lists * 32, dtype=torch.int32, device=dev)
            T0 = None
            if self.FILTER_LARGE_K_COARSE > 1 and n >= self.SEED_MIN_ROWS:
                # The seed pass's register lists start empty and take their first rows through
                # the serial 32-slot insert, most of its time.  A coarser pass first (kmax = 16,
                # every COARSE-th tile of the seed pass's own sample: the same slices, so a
                # subset of it) gives the seed pass a threshold of its own; the seed pass's
                # k best rows all lie above it, so T is what the unseeded seed pass gives.
                # (Not on small shards, where its launch costs more than it saves.)
                l16, _ = geometry(16)
                c0 = torch.empty(NQ, n_rblk * l16 * 16, device=dev)
                i0 = torch.empty(NQ, n_rblk * l16 * 16, dtype=torch.int32, device=dev)
                scan(self.rows, n, *operands, q, 16, n_rblk, c0, i0, None,
                     self.FILTER_LARGE_K_STRIDE * self.FILTER_LARGE_K_COARSE, self.scan_xcd, gate)
                T0 = threshold(c0, k)
            scan(self.rows, n, *operands, q, 32, n_rblk, cs, ci, T0, self.FILTER_LARGE_K_STRIDE,
                 self.scan_xcd, gate)
            T = threshold(cs, k)
        else:
            T = torch.full((NQ,), -math.inf, device=dev)
        # (the emitting scan's queries per block, and so its grid, are not the list scan's)
        qpb, form = emit_form(NQ)
        n_rblk = self._masked_rblk(n, NQ, qpb, n_cus)
        cap = self.LARGE_K_CAP
        es = torch.empty(NQ, cap, device=dev)
        ei = torch.empty(NQ, cap, dtype=torch.int32, device=dev)
        cnt = torch.empty(NQ, dtype=torch.int32, device=dev)
        # this search's own overflow flag; zeroed here, so a closed gate leaves it 0
        ovf = torch.zeros(1, dtype=torch.int32, device=dev)
        emit(self.rows, n, *operands, q, T, es, ei, cnt, cap, n_rblk, *form, self.scan_xcd, gate)
        h.topk_select_counted(es.data_ptr(), ei.data_ptr(), cnt.data_ptr(), cap, NQ, 128, k,
                              out_s.data_ptr(), out_i.data_ptr(), ovf.data_ptr(),
                              stream_handle(dev), gate=0 if gate is None else gate.data_ptr(),
                              reset_ovf=False)
        if rescale is not None:
            out_s.mul_(rescale)   # (-inf stays -inf)
        self._filter_large_k_last = (cnt, ovf)   # candidate counts / overflow flag (tests)
        if int(ovf.item()):
            return None
        return out_s, out_i

    def _search_filtered_large_k(self, q_unit, k: int, mask: RowMask, n_cus, gate=None,
                                 seed: bool = True):
        """The masked large-k search under one RowMask (bf16: index_filter.hip and
        index_mq_filter.hip at a width in FILTER_LARGE_K_DIMS; fp8: index_filter_fp8.hip and
        index_emit_fp8.hip at one in FILTER_LARGE_K_FP8_DIMS, the queries quantised to e4m3
        here).  On overflow the search takes the masked matmul -- on an fp8 shard over the
        DECODED quantised queries, so it differs from the scan by summation order only, not by
        the queries' e4m3 rounding."""
        scan, emit = self._masked_kernels(False)
        q = self._masked_queries(q_unit, mask.visible)
        res = self._masked_large_k(scan, emit, mask.visible,
                                   (mask.words, mask.tiles, mask.n_live), q, k, n_cus, gate, seed)
        if res is not None:
            return res
        if self.dtype == "fp8":
            q = K.fp8_to_float(q, FP8_SCALE)
        return self._search_matmul(q, k, mask=mask)

    def _search_group_chunk_large_k(self, q8, k: int, groups: MaskGroups, ch: dict, n_cus,
                                    seed: bool = True):
        """The masked large-k search under a mask per query, over one chunk's queries (``q8``:
        their e4m3 bytes, quantised once per search by _search_grouped): the grouped e4m3 list
        scan (index_filter_group_fp8.hip) and the grouped emitting scan
        (index_emit_group_fp8.hip) over the union's live-tile list.  Returns None when a query's
        candidates overflow LARGE_K_CAP (the flag is read once per chunk); the caller then
        answers the chunk's groups one mask at a time."""
        scan, emit = self._masked_kernels(True)
        return self._masked_large_k(
            scan, emit, groups.visible, (ch["mask8"], ch["qgroup"], ch["tiles"], ch["n_live"]),
            q8, k, n_cus, seed=seed)

    def _search_scan(self, q_unit, k: int, rows, dtype: str, n_cus):
        """Seeded fused scan + merge over ``rows`` (bf16 slab, or e4m3 bytes for dtype fp8)."""
        kmax = 16 if k <= 16 else 32
        if dtype == "fp8":
            from ..ops.kernels import quant_fp8

            q_unit = quant_fp8(q_unit, scale=FP8_SCALE)  # scores come back as S^2 * cosine
        n = self.visible
        thr = None
        m = self._seed_rows(n, k)
        mq = m and self._mq_ok(q_unit.shape[0], k, rows, dtype)
        plan = self._tile_sample_plan(n) if (m and mq) else None
        if plan is not None:
            # Threshold sample = one pseudo-random 64-row tile of every 64 in the first nv groups,
            # scanned IN PLACE by the emitting kernel (gathering n/64 rows cost 0.45 ms at 100M),
            # plus every row after them -- the last 4096..8191 rows, where fresh inserts (often
            # a query's best matches) sit -- by the 256-query kernel.  Disjoint real rows, so the
            # k-th best of the union lower-bounds the final k-th score.
            ts, nv, t0, idx = plan
            sub = torch.index_select(self.rows, 0, idx)       # whole tiles: already tile-padded
            pm = self.prepass_min_tiles
            s0, _ = self._scan(sub.shape[0], q_unit, kmax, k, None, n_cus, sub, dtype, min_tiles=pm)
            thr0 = s0[:, k - 1].contiguous() - self.MQ_THR_MARGIN
            pre_s, _ = self._scan_mq(nv * TILE_ROWS, q_unit, kmax, k, thr0, n_cus, tshift=ts)
            # (seeded with thr0 too: a tail row below it cannot enter the union's top k, whose
            # k-th best is the sample's, >= thr0; unseeded this small scan took 0.2 ms)
            tail_s, _ = self._scan(n - t0, q_unit, kmax, k, thr0, n_cus, self.rows[t0:], dtype,
                                   min_tiles=pm)
            kth = torch.topk(torch.cat([pre_s, tail_s], 1), k, dim=1).values[:, k - 1]
            thr = kth.contiguous() - self.MQ_THR_MARGIN
            return self._scan_mq(n, q_unit, kmax, k, thr, n_cus)
        if m and mq:
            # the emitting kernel keeps EVERY row above the threshold, so it needs a threshold
            # near the true k-th score for any row order: one pseudo-random row per 64-row block
            # (no row twice, so the sample's k-th best is a lower bound), not the first n/64 rows
            # (rows appended last, e.g. fresh embeddings, are often the best matches).  The margin
            # covers the two kernels' different fp32 summation orders (16x16x32 vs 32x32x16).
            ms, sample = self._block_sample(n)
            # the sample is scanned the same way, seeded from ITS first 1/64 (a uniform
            # sub-sample; the 256-query kernel over the whole sample took ~6 % of the search)
            m2 = _round_up(max(ms // self.SEED_DIV, k), TILE_ROWS)
            if m2 < ms:
                s0, _ = self._scan(m2, q_unit, kmax, k, None, n_cus, sample, dtype)
                thr0 = s0[:, k - 1].contiguous() - self.MQ_THR_MARGIN
                pre_s, _ = self._scan_mq(ms, q_unit, kmax, k, thr0, n_cus, rows=sample)
            else:
                pre_s, _ = self._scan(ms, q_unit, kmax, k, None, n_cus, sample, dtype)
            thr = pre_s[:, k - 1].contiguous() - self.MQ_THR_MARGIN
            return self._scan_mq(n, q_unit, kmax, k, thr, n_cus)
        if m:
            # threshold seeding: the k-th best score over the first m rows lower-bounds the final
            # k-th score, so the full scan may drop anything below it (exact; see the kernel note)
            pre_s, _ = self._scan(m, q_unit, kmax, k, None, n_cus, rows, dtype)
            kth = pre_s[:, k - 1].contiguous()
            # (full_like, not torch.tensor(-inf, device=...): a pageable H2D copy would block the
            # host on the stream every search and leave the GPU idle while the scan is enqueued)
            thr = torch.nextafter(kth, torch.full_like(kth, -math.inf))
        return self._scan(n, q_unit, kmax, k, thr, n_cus, rows, dtype)

    MQ_CAP = 4096             # candidate slots per query (expected use ~64 k)
    MQ_THR_MARGIN = 2.0 ** -12
    MQ_TILE_SHIFT = 6         # threshold sample: one 64-row tile in 2^6
    MQ_TAIL_ROWS = 4096       # ... plus at least the last 4096 rows

    def _tile_sample_plan(self, n: int, ts: int | None = None, want_idx: bool = True):
        """In-place threshold sample over n visible rows, or None when n is too small.

        Returns (ts, nv, t0, idx): the emitting kernel's virtual tile v < nv reads physical tile
        (v << ts) + h(v) (h = top ts bits of v * 0x9E3779B1, as in index_mq.hip), i.e. one tile
        of each group of 2^ts; rows [t0, n) (4096..8191 of them) are the exact tail; idx are the
        rows of every SEED_DIV-th sampled tile (the sub-sample that seeds the sample scan, a
        subset of the sample; None unless ``want_idx`` -- dense_scores computes the same rows
        in-kernel).  Every sampled row lies below t0 <= n - MQ_TAIL_ROWS."""
        ts = self.MQ_TILE_SHIFT if ts is None else ts
        group = TILE_ROWS << ts                                # rows per tile group
        nv = (n - self.MQ_TAIL_ROWS) // group if n > self.MQ_TAIL_ROWS else 0
        if nv < self.SEED_DIV:
            return None
        t0 = nv * group
        if t0 > n:   # (a launch past the rows would fault the GPU)
            raise RuntimeError("tile sample past the visible rows")
        if not want_idx:
            return ts, nv, t0, None
        # idx depends on (nv, ts) only, and nv changes once per 2^ts tiles of appends: cached
        # (rebuilding it was ~8 small kernels on every search's critical path)
        key = (nv, ts, self.SEED_DIV)
        cached = getattr(self, "_plan_idx", None)
        if cached is None or cached[0] != key:
            v = torch.arange(0, nv, self.SEED_DIV, device=self.device, dtype=torch.int64)
            ph = (v << ts) + (((v * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - ts))
            idx = (ph[:, None] * TILE_ROWS + torch.arange(TILE_ROWS, device=self.device)).reshape(-1)
            self._plan_idx = cached = (key, idx)
        return ts, nv, t0, cached[1]

    def _mq_ok(self, NQ: int, k: int, rows, dtype: str) -> bool:
        return (self.scan_mq and dtype == "bf16" and self.dim in MQ_DIMS and rows is self.rows
                and NQ >= self.mq_min_nq and k <= 16)

    def _mq_form(self, NQ: int):
        """(sets, rsplit) of the emitting scan: 16-query sets per wave and waves sharing a query
        group.  D = 384: 4 sets (512 queries per workgroup, or 256 with the row split); wider rows
        hold fewer resident query sets (768: 2, 1024: 1)."""
        if self.dim != 384:
            return (2 if self.dim == 768 else 1), 1
        return (4, 1) if NQ >= 512 else ((4, 2) if self.mq_rsplit else (2, 1))

    def _block_sample(self, n: int):
        """Row sample for threshold seeding: row 64 i + h(i) of every full 64-row block i (h a
        fixed hash into [0, 64)), gathered into a tile-padded buffer."""
        m = n // self.SEED_DIV
        cached = getattr(self, "_sample_idx", None)
        if cached is None or cached[0] != m:
            i = torch.arange(m, device=self.device, dtype=torch.int64)
            self._sample_idx = (m, i * self.SEED_DIV + (((i * 0x9E3779B1) & 0xFFFFFFFF) >> 26))
        buf = torch.empty(_round_up(m, TILE_ROWS), self.dim, dtype=self.rows.dtype,
                          device=self.device)
        torch.index_select(self.rows, 0, self._sample_idx[1], out=buf[:m])
        return m, buf

    def _scan_mq(self, n: int, q_unit: torch.Tensor, kmax: int, k: int, thr, n_cus, rows=None,
                 tshift: int = 0, gate=None, out=None, fallback: bool = True, cand: bool = False,
                 cap: int | None = None, min_tiles: int = 16, cnt=None):
        """512-query-per-workgroup scan emitting every score above ``thr`` (index_mq.hip), top-k
        of each query's candidates, and the exact 256-query kernel as a fallback that runs on the
        GPU only if some query's candidate buffer overflowed (a device flag gates it).
        ``tshift`` > 0: ``n`` virtual rows of the in-place 1-in-2^tshift tile sample; its
        fallback scans every row (the exact top-k of all rows is a valid threshold too).
        ``gate`` (int32 device flag): the scan and its select run only if it is non-zero (they
        then write ``out`` and OR into its overflow flag, ``out[2]``).  ``fallback=False``: no
        overflow re-scan -- for a threshold sample that is still sound, since the top-k of ANY
        subset of real rows lower-bounds the k-th best.  ``cand``: also return the candidate
        buffers (scores, rows, count) for the route estimate of _search_pruned.  ``min_tiles``:
        row-block floor in 64-row tiles (1 spreads a small scan over every CU).  ``cnt``: the
        caller's candidate counters, already zeroed together with ``out``'s overflow flag (no
        memset launches)."""
        from ..ops._ext import hip, stream_handle

        h = hip()
        NQ = q_unit.shape[0]
        sets, rsplit = self._mq_form(NQ)
        n_qblk = math.ceil(NQ / h.mq_queries_per_blk(sets, rsplit))
        if n_cus is None:
            n_cus = self._n_cus()
        n_rblk = max(1, min(math.ceil(n / (TILE_ROWS * min_tiles)), max(1, round(n_cus / n_qblk))))
        rows_per_blk = _round_up(max(1, math.ceil(n / n_rblk)), TILE_ROWS)
        n_rblk = max(1, math.ceil(n / rows_per_blk))
        rows = self.rows if rows is None else rows
        cap, dev = cap or self.MQ_CAP, self.device
        cs = torch.empty(NQ, cap, device=dev)
        ci = torch.empty(NQ, cap, dtype=torch.int32, device=dev)
        zeroed = cnt is not None
        if cnt is None:
            cnt = torch.empty(NQ, dtype=torch.int32, device=dev)
        if out is None:
            out = (torch.empty(NQ, k, device=dev), torch.empty(NQ, k, dtype=torch.int32, device=dev),
                   torch.empty(1, dtype=torch.int32, device=dev))
        out_s, out_i, ovf = out
        st = stream_handle(dev)
        gp = 0 if gate is None else gate.data_ptr()
        h.index_scan_mq(rows.data_ptr(), n, rows_per_blk, n_rblk, q_unit.data_ptr(), NQ,
                        thr.data_ptr(), cs.data_ptr(), ci.data_ptr(), cnt.data_ptr(), cap,
                        self.scan_xcd, st, sets, tshift, rsplit, gp, zero_cnt=not zeroed,
                        dim=self.dim)
        h.topk_select_counted(cs.data_ptr(), ci.data_ptr(), cnt.data_ptr(), cap, NQ, kmax, k,
                              out_s.data_ptr(), out_i.data_ptr(), ovf.data_ptr(), st, gate=gp,
                              reset_ovf=gate is None and not zeroed)
        if gate is None and fallback:
            if tshift:
                self._scan(self.visible, q_unit, kmax, k, thr, n_cus, gate=ovf, out=(out_s, out_i))
            else:
                self._scan(n, q_unit, kmax, k, thr, n_cus, rows, gate=ovf, out=(out_s, out_i))
        self._mq_last = (cnt, ovf)   # candidate counts / overflow flag (tests, diagnostics)
        if gate is None and fallback:   # (a sample's overflow only steers the route)
            self._stats(ovf, cnt)
        if cand:
            return out_s, out_i, cs, ci, cnt
        return out_s, out_i

    def _stats(self, ovf, cnt, dense=None, blk=None) -> None:
        """``mq_stats``: running totals on the device (a few tiny kernels per search; off by
        default) -- batches whose candidates overflowed, the most candidates any query emitted,
        pruned searches routed whole to the bf16 scan by their sample, pruned searches that
        routed only some row blocks there, and the row blocks so routed."""
        if not self.mq_stats:
            return
        if self._mq_tot is None:
            self._mq_tot_buf = torch.zeros(5, dtype=torch.int32, device=self.device)
            self._mq_tot = tuple(self._mq_tot_buf[i:i + 1] for i in range(5))
        if (self.device.type == "cuda" and ovf.dtype == torch.int32 and cnt.dtype == torch.int32
                and cnt.is_contiguous() and (dense is None or dense.dtype == torch.int32)
                and (blk is None or blk.dtype == torch.int32)):
            from ..ops._ext import hip, stream_handle

            # (one launch: prepass statistics kernel, index_i8.hip prune_stats_kernel)
            hip().prune_stats(ovf.data_ptr(), cnt.data_ptr(), cnt.numel(),
                              0 if dense is None else dense.data_ptr(),
                              0 if blk is None else blk.data_ptr(), self._mq_tot_buf.data_ptr(),
                              stream_handle(self.device))
            return
        self._mq_tot[0].add_(ovf)
        torch.maximum(self._mq_tot[1], cnt.max().view(1), out=self._mq_tot[1])
        if dense is not None:
            self._mq_tot[2].add_(dense)
        if blk is not None and dense is not None:
            part = (blk[:1] > 0).int() * (1 - dense)
            self._mq_tot[3].add_(part)
            self._mq_tot[4].add_(blk[:1] * part)

    # pruned search: its exact threshold sample is 1 tile in 2^5.  Sparser samples win the
    # headline (+2-3 % at 2^7) only because its queries' best matches sit in the exact fresh-row
    # tail; for queries near random stored rows (the per-rank shapes 12.5M x 2048 and 50M x 512)
    # 2^6 is 4-9 % slower and 2^7 overflows the candidate slots, 3x slower
    # (profiles/r2_prune_shift_rank/).  A shard too small for SEED_DIV groups at 2^5 (none at
    # the default; the override knob may raise the shift) samples more densely, down to
    # PRUNE_MIN_SHIFT.
    PRUNE_TILE_SHIFT = 5
    PRUNE_MIN_SHIFT = 5
    # the split image's own sample density: 2^6 (half the sample, max 3.7k candidates per query)
    # measured the same as 2^5 (13.07 vs 13.05 ms at 100M x 256 anisotropic, profiles/r4_split/)
    PRUNE_TILE_SHIFT_SPLIT = 5
    # ... and 2^7 while recent searches took the MX-fp4 tier (self / near-duplicate queries: each
    # query's k-th score sits far above the bulk, so a quarter of the sample finds the same T):
    # headline 7.19-7.25 -> 6.88-6.97 ms per step, while held-out random queries, whose T a
    # sparser sample loosens, keep 2^5 (11.36 vs 12.36 ms at 2^7; profiles/r4_final/shift/).
    # Decided from the last search whose tier flag has reached the host (no sync); exactness
    # never depends on it
    PRUNE_TILE_SHIFT_MX4 = 7
    # candidate slots per query: ~1-2k expected at 100M x 384 on random data, but the busiest of
    # 256 held-out queries emitted 6k (profiles/r3_real/); slots cost memory only (the re-score
    # and select walk the emitted count), 256 MiB at 1024 queries
    PRUNE_CAP = 32768
    SAMPLE_CAP = 16384        # candidate slots per query of the sampled searches' sample scan

    # route a row block to the bf16 emitting scan when the sample predicts more than this share
    # of PRUNE_CAP int8 candidates from it for some query, and EVERY block when some query's
    # estimate over the blocks left to the int8 scan still exceeds PRUNE_DENSE_FRAC of it
    # (estimates c << ts have a ~sqrt(c) << ts spread).  A block in the bf16 scan costs ~1.7x its
    # int8 scan but spreads over the whole chip; 1024 int8 candidates from one block per query
    # cost about as much to emit and re-score.
    PRUNE_DENSE_FRAC = 0.6
    # batches up to this many queries score the exact tail densely (see _pruned_begin; the
    # MX-fp4 tier's choice needs those dense scores, so 2048 covers the gathered batches of the
    # 8-GPU step); SYMB_TAIL_DENSE_MAX_NQ=0 keeps the emitting tail scan (A/B)
    tail_dense_max_nq = int(os.environ.get("SYMB_TAIL_DENSE_MAX_NQ", "2048"))
    PRUNE_BLOCK_FRAC = 1 / 32
    # the MX-fp4 first tier runs when every query's estimated fp4 band holds at most this share
    # of PRUNE_CAP (its candidates are re-scored exactly like the int8 ones)
    MX4_LIMIT_FRAC = 0.25
    prune_route = True   # False: always take the int8 pass (tests of the overflow fallback)

    def _search_pruned(self, q_unit, k: int, n_cus):
        """EXACT top-k through the int8 image (index_i8.hip has the bound): an exact bf16 sample
        gives T <= each query's final k-th score; every row whose int8 score reaches T - margin is
        emitted, re-scored in bf16 and the top-k of those is returned.  A query whose candidates
        overflow PRUNE_CAP raises the flag that gates the exact bf16 list scan.

        Route (decided on the GPU from the same sample, no host sync, per row block of the int8
        scan): counting the sample's emitted rows at or above T - margin (extrapolated when that
        band reaches below the sample's seed threshold), binned by block, estimates each query's
        int8 candidates per block.  A block that some query would flood -- a crowd of
        near-duplicates the int8 bound cannot separate, such as the freshly ingested rows of a
        corpus whose embeddings all sit together -- goes to the bf16 emitting scan at the exact
        threshold T, spread over the whole chip, and the int8 scan skips it; both emit into the
        same candidate buffers.  On data whose scores crowd the k-th best everywhere (an
        anisotropic corpus: every pair of rows at cosine ~0.3) every block goes to the bf16
        scan, instead of an int8 pass that would overflow and then pay the full fallback scan on
        top (profiles/r3_real/, profiles/r3_sustain/)."""
        ctx = self._pruned_begin(q_unit, k, n_cus)
        return None if ctx is None else self._pruned_end(ctx)

    def _pruned_begin(self, q_unit, k: int, n_cus, split: bool = False):
        """Query-side half of the pruned search: int8 queries, the exact sample, T, thresholds and
        the route flag -- everything before the full-shard scan, on the current stream, for the
        rows visible NOW (a pipelined caller runs it for batch i + 1 under batch i's scan).
        ``split``: the caller is ``search_begin`` and left ``n_cus`` to the shard (_scan_reserve)."""
        from ..ops._ext import hip, stream_handle

        n, NQ, kmax = self.visible, q_unit.shape[0], 16
        shift = self.PRUNE_TILE_SHIFT_SPLIT if self._i8_heavy else self.PRUNE_TILE_SHIFT
        with self._tier_lock:
            while self._tier_pending and self._tier_pending[0][1].query():
                self._tier_mx4 = int(self._tier_pending.popleft()[0].item()) == 0
        if self._tier_mx4 and self.mx4_on:
            shift = max(shift, self.PRUNE_TILE_SHIFT_MX4)
        self._sample_shift_last = shift   # (diagnostics / tests)
        plan, ts = None, shift
        while plan is None and ts >= min(self.PRUNE_MIN_SHIFT, shift):
            plan, ts = self._tile_sample_plan(n, ts, want_idx=False), ts - 1
        if plan is None:
            return None
        two_phase = split
        split = split and n_cus is None
        if n_cus is None:
            n_cus = self._n_cus()
        reserve = self._scan_reserve(split, n_cus, NQ)
        h, dev, cap = hip(), self.device, self.PRUNE_CAP
        st = stream_handle(dev)
        ts, nv, t0, _ = plan
        tcap = n - t0
        dense_tail = NQ <= self.tail_dense_max_nq
        geo = self._i8_geometry(n, NQ, n_cus, reserve)
        n_rblk = geo[2]
        # one int32 workspace for every counter and flag of the search, cleared by the query
        # quantiser on its way (no memset launches): the sample's and the final scan's candidate
        # counters, flags (WS_* below) and the route's per-block maxima
        ws = torch.empty(2 * NQ + self.WS_FLAGS + n_rblk, dtype=torch.int32, device=dev)
        cnt_p, cnt_f = ws[:NQ], ws[NQ:2 * NQ]
        flags = ws[2 * NQ:2 * NQ + self.WS_FLAGS]
        blkmax = ws[2 * NQ + self.WS_FLAGS:]
        # 0. the int8 queries and each query's bound margin |q| E + |q - q~| X (prune_qquant), or
        #    their split image in the shard's basis and its margin (quant_rows_split)
        heavy = self._i8_heavy
        q8, sq, margin = self.prune_query_image(q_unit, zero=ws)
        # 1. T: the k-th best exact score of a sample of real rows (1 tile in 2^ts, plus the last
        #    4096+ rows where fresh inserts sit), as in _search_scan; its emitted candidates also
        #    estimate the int8 band's population (prune_route).  The sample scan is seeded by the
        #    exact scores of every SEED_DIV-th sampled tile, and a batch of up to
        #    tail_dense_max_nq queries scores the tail [t0, n) densely in the same launch
        #    (dense_scores: the seed tiles' rows are computed in-kernel, no gather); the selects
        #    read their columns in place and write the seed threshold directly
        m_seed = -(-nv // self.SEED_DIV) * TILE_ROWS
        ld = _round_up(m_seed + (tcap if dense_tail else 0), 4)
        S = torch.empty(NQ, ld, device=dev)
        # the prefix tier is enqueued too (step 3): the same launch keeps each score's partial sum
        # over the prefix dims for its choice
        pfx = self._prefix_enqueued(dense_tail)
        SP = torch.empty(NQ, ld, device=dev) if pfx else None
        pk = dict(outp=SP.data_ptr(), prefix_dims=64 * self.prefix_ksteps) if pfx else {}
        h.dense_scores(self.rows.data_ptr(), self.dim, 0, m_seed, t0, tcap if dense_tail else 0,
                       q_unit.data_ptr(), NQ, S.data_ptr(), ld, st, ts=ts, div=self.SEED_DIV, **pk)
        thr0 = torch.empty(NQ, dtype=torch.float32, device=dev)
        seed_s = torch.empty(NQ, k, device=dev)
        seed_i = torch.empty(NQ, k, dtype=torch.int32, device=dev)
        # (a dense tail is selected in the same launch: its columns follow the seed tiles' in S)
        tail_s = torch.empty(NQ, k, device=dev)
        tail_i = torch.empty(NQ, k, dtype=torch.int32, device=dev) if dense_tail else None
        fuse_tail = dense_tail and tcap > 0
        tcs_p = S.data_ptr() + 4 * m_seed
        h.topk_select_counted(S.data_ptr(), 0, 0, m_seed, NQ, kmax, k, seed_s.data_ptr(),
                              seed_i.data_ptr(), flags[self.WS_SCRATCH].data_ptr(), st,
                              reset_ovf=False, ld=ld, kth_out=thr0.data_ptr(),
                              kth_margin=self.MQ_THR_MARGIN,
                              seg2_s=tcs_p if fuse_tail else 0, seg2_cap=tcap if fuse_tail else 0,
                              seg2_out_s=tail_s.data_ptr() if fuse_tail else 0,
                              seg2_out_i=tail_i.data_ptr() if fuse_tail else 0)
        pm = self.prepass_min_tiles
        pre_s, _, cs_p, ci_p, cnt_p = self._scan_mq(
            nv * TILE_ROWS, q_unit, kmax, k, thr0, n_cus, tshift=ts, fallback=False, cand=True,
            cap=self.SAMPLE_CAP, cnt=cnt_p,
            out=(torch.empty(NQ, k, device=dev), torch.empty(NQ, k, dtype=torch.int32, device=dev),
                 flags[self.WS_SAMPLE_OVF:self.WS_SAMPLE_OVF + 1]))
        # the fresh-row tail [t0, n) (never sampled) is scored exactly and the route counts every
        # tail row >= the band one by one -- a crowd of fresh near-duplicates sits there first.
        # The emitting tail scan (larger batches) reserved one slot per emitted row with a global
        # atomic on the query's counter: with a fresh near-duplicate crowd in the tail every
        # (query, row) pair emitted and the counters serialized (0.6 ms per headline step,
        # profiles/r3_step_trace/)
        if dense_tail:
            if not fuse_tail:
                h.topk_select_counted(tcs_p, 0, 0, tcap, NQ, kmax, k, tail_s.data_ptr(),
                                      tail_i.data_ptr(), flags[self.WS_SCRATCH].data_ptr(), st,
                                      reset_ovf=False, ld=ld)
            tci = tcnt = None
            tail_ld = ld
        else:
            tail_s, _, tcs, tci, tcnt = self._scan_mq(tcap, q_unit, kmax, k, thr0, n_cus,
                                                      rows=self.rows[t0:], fallback=False,
                                                      cand=True, cap=tcap, min_tiles=pm)
            tcs_p, tail_ld = tcs.data_ptr(), tcap
        # 2. T (k-th best of the union), the per-query emission threshold (T - margin) / sq and
        #    the per-row-block route (prune_route): the blocks some query would flood with int8
        #    candidates go to the bf16 emitting scan at T, the rest to the int8 scan
        T = torch.empty(NQ, dtype=torch.float32, device=dev)
        thr = torch.empty(NQ, dtype=torch.float32, device=dev)
        dense = flags[self.WS_DENSE:self.WS_DENSE + 1]
        est = torch.empty(NQ, n_rblk, dtype=torch.float32, device=dev)
        blk = torch.empty(2 + 2 * n_rblk, dtype=torch.int32, device=dev)
        inf = float("inf")
        limit = self.PRUNE_DENSE_FRAC * cap if self.prune_route else inf
        blk_limit = self.PRUNE_BLOCK_FRAC * cap if self.prune_route else inf
        h.prune_route(NQ, pre_s.data_ptr(), tail_s.data_ptr(), k, self.MQ_THR_MARGIN,
                      sq.data_ptr(), margin.data_ptr(), thr0.data_ptr(), cs_p.data_ptr(),
                      ci_p.data_ptr(), cnt_p.data_ptr(), self.SAMPLE_CAP, ts, geo[1], n_rblk,
                      blk_limit, limit, self._mq_slots(NQ, n_cus)[3], T.data_ptr(),
                      thr.data_ptr(), dense.data_ptr(), est.data_ptr(), blkmax.data_ptr(),
                      blk.data_ptr(), st, tail_cs=tcs_p,
                      tail_ci=0 if tci is None else tci.data_ptr(),
                      tail_cnt=0 if tcnt is None else tcnt.data_ptr(), tail_cap=tcap, tail_off=t0,
                      tail_ld=tail_ld, zeroed=True)
        ctx = dict(q=q_unit, k=k, n=n, n_cus=n_cus, q8=q8, sq=sq, thr=thr, T=T, dense=dense,
                   blk=blk, geo=geo, heavy=heavy, gen=self._calib_gen, mx4=None, ws=ws,
                   wide=reserve > 0, hint_mx4=bool(self._tier_mx4 and self.mx4_on))
        # 3. the MX-fp4 first tier (mx4_select): when every query's k-th score sits so far above
        #    the corpus bulk that even the coarse fp4 bound (|q| E4 + |q - q~| X4, ~0.25 on unit
        #    rows) leaves few rows in its band -- self / near-duplicate queries, such as the
        #    headline's freshly inserted random-init embeddings -- the scan streams the fp4 image
        #    at twice the int8 MFMA rate instead of the int8 one.  Decided on the GPU from the same
        #    exact scores (the probe: every 4th seed tile, read in place; the band must lie above
        #    the sample's seed threshold, so the sample counted it): the int8 / split scan and
        #    the fp4 scan are both enqueued, each gated on the flag, and exactly one runs.
        nvf = flags[self.WS_NV:self.WS_NV + 1]
        n_probe = TILE_ROWS * -(-(m_seed // TILE_ROWS) // 4)
        if self.mx4_on and self.prune_route and dense_tail:
            q4, qs4, m4, *pq = self.mx4_query_image(q_unit, prefix=pfx)
            thr4 = torch.empty(NQ, dtype=torch.float32, device=dev)
            h.mx4_select(NQ, T.data_ptr(), m4.data_ptr(), margin.data_ptr(), S.data_ptr(), m_seed,
                         float(t0) / n_probe, tcs_p, tcap, self.MX4_LIMIT_FRAC * cap,
                         thr4.data_ptr(), nvf.data_ptr(), st, ld=ld, tile_stride=4, tail_ld=ld,
                         nv_zeroed=True)
            ctx["mx4"] = dict(q4=q4, qs4=qs4, thr4=thr4, nv=nvf)
            if pfx:
                # 3'. the prefix tier (mx4_prefix_select): where T stands so high that even with
                #     the remainder dims bounded by |q_R| XR the prefix estimate separates the
                #     rows that can matter -- the same self / near-duplicate regime -- the fp4 scan
                #     reads only the first prefix_ksteps k-steps of every record, half the bytes
                #     at 3.  A second flag word says which fp4 form runs (0: prefix, 1: whole
                #     rows); the fp4 tier's one launch reads it and runs that form.
                mP, qR = pq
                thrP = torch.empty(NQ, dtype=torch.float32, device=dev)
                nvp = flags[self.WS_PFX:self.WS_PFX + 1]
                h.mx4_prefix_select(NQ, T.data_ptr(), mP.data_ptr(), qR.data_ptr(),
                                    self.mx4_pbounds.data_ptr(), margin.data_ptr(), S.data_ptr(),
                                    SP.data_ptr(), m_seed, float(t0) / n_probe, tcs_p,
                                    SP.data_ptr() + 4 * m_seed, tcap,
                                    inf if self.prefix_tier == 2 else self.MX4_LIMIT_FRAC * cap,
                                    thrP.data_ptr(), nvp.data_ptr(), st, ld=ld, tile_stride=4,
                                    tail_ld=ld, nvp_zeroed=True, band=self.prefix_band)
                ctx["mx4"].update(thrP=thrP, nvp=nvp)
            if self.img_mx4 is not None and self.mx4_centroid:
                # the query-side bound (index_stream.hip mx4_centroids_kernel): per 32-query set
                # the centroid image and radius R, so the scan skips a set's MFMAs on sub-tiles
                # where c~ . x~ + R X4 stays below every threshold of the set
                n_sets = -(-NQ // 32)
                c4 = torch.empty(n_sets, self.dim // 2, dtype=torch.uint8, device=dev)
                cqs = torch.empty(n_sets, qs4.shape[1], dtype=torch.int32, device=dev)
                cR = torch.empty(n_sets, dtype=torch.float32, device=dev)
                h.mx4_centroids(q4.data_ptr(), qs4.data_ptr(), NQ, self.dim, c4.data_ptr(),
                                cqs.data_ptr(), cR.data_ptr(), st)
                ctx["mx4"].update(c4=c4, cqs=cqs, cR=cR)
        if two_phase and self.route_at_begin:
            # What the full-shard half does not need the stream scan for runs here, under the
            # previous search's scan: the candidate buffers, the partial sub-tile's prefill (first:
            # it STORES the counters) and the bf16 scan of the routed blocks.  They read the bf16
            # rows below n, T and the route's list -- nothing a later append (rows at or past n),
            # a tombstone (a zeroed row is re-scored as such by the finish, and search_end checks
            # the result against the live mask) or the stream scan writes; a re-calibration
            # between the halves drops these candidates with the rest (the gen check), and a
            # compaction is ordered against running searches by the caller as any write is.
            cs, ci = self._cand_buffers(NQ)
            n_scan = self._cand_prefill(h, st, NQ, n, ci, cnt_f)
            self._route_scan(h, st, q_unit, n_scan, n_cus, T, blk, geo[1], cs, ci, cnt_f)
            ctx["cand"] = (cs, ci, n_scan)
        return ctx

    def _cand_buffers(self, NQ: int):
        """(scores, ids) of the pruned search's candidates: [NQ, PRUNE_CAP] each."""
        return (torch.empty(NQ, self.PRUNE_CAP, device=self.device),
                torch.empty(NQ, self.PRUNE_CAP, dtype=torch.int32, device=self.device))

    def _cand_prefill(self, h, st, NQ: int, n: int, ci, cnt) -> int:
        """-> n_scan, the rows the first-pass scans cover.  They stop at the last whole 32-row
        sub-tile: an append into a partly filled one re-quantises its rows under a new shared
        int8 scale (and raises E past what this search's margins assumed), and a pipelined
        caller appends batch i + 1 while batch i's scan runs.  The < 32 rows past the boundary
        enter every query's candidate list unconditionally (prefill_candidates, which stores the
        counters: before any scan adds to them) and are re-scored exactly like any candidate."""
        n_scan = n - n % STREAM_SUB if self.stream else n
        if n_scan < n:
            h.prefill_candidates(NQ, n_scan, n - n_scan, ci.data_ptr(), cnt.data_ptr(),
                                 self.PRUNE_CAP, st)
        return n_scan

    def _route_scan(self, h, st, q_unit, n_scan: int, n_cus: int, T, blk, rows_per_blk: int,
                    cs, ci, cnt) -> None:
        """The bf16 emitting scan of the blocks the route listed, at the exact threshold T, into
        the candidate buffers (no launch work when none is listed)."""
        if not self.prune_route:
            return
        NQ = q_unit.shape[0]
        sets, mrs, _, slots = self._mq_slots(NQ, n_cus)
        h.index_scan_mq(self.rows.data_ptr(), n_scan, TILE_ROWS, slots, q_unit.data_ptr(), NQ,
                        T.data_ptr(), cs.data_ptr(), ci.data_ptr(), cnt.data_ptr(),
                        self.PRUNE_CAP, self.scan_xcd, st, sets, 0, mrs, blist=blk.data_ptr(),
                        list_tiles=rows_per_blk // TILE_ROWS, zero_cnt=False, dim=self.dim)

    def _tier_word(self):
        """-> (pinned int32 [1] view, its device address) for one search's tier word, from a ring
        of pinned, device-mapped words the finish kernel stores into; (None, 0) when the pinned
        memory has no device address (the caller copies the word as before)."""
        from ..ops._ext import hip

        if self._tier_words is None:
            w = torch.zeros(64, dtype=torch.int32, pin_memory=True)
            self._tier_words = (w, int(hip().host_device_ptr(w.data_ptr())))
        w, base = self._tier_words
        if not base:
            return None, 0
        with self._tier_lock:
            slot = self._tier_slot
            self._tier_slot = (slot + 1) % w.numel()
        return w[slot:slot + 1], base + 4 * slot

    # the search workspace's flag slots (_pruned_begin): route "every block dense", the MX-fp4
    # tier's "not viable" flag, the sample's and the final select's overflow flags, and a slot
    # the dense selects may write (they never overflow)
    WS_DENSE, WS_NV, WS_SAMPLE_OVF, WS_OVF, WS_SCRATCH, WS_FLAGS = 0, 1, 2, 3, 4, 8
    WS_PFX = 5   # the fp4 tier's form: 0 the prefix scan, 1 the whole-row scan (mx4_prefix_select)

    # the prefix tier's defaults: k-steps read per record, on / off (the prefix form runs at its
    # deep depth, ops/kernels.py SCAN_PREFIX_DEEP; profiles/prefix_tier/README.md has the
    # measurements)
    PREFIX_KSTEPS = 3
    PREFIX_TIER = 1   # (2: the candidate estimate is skipped, the tier runs whenever thrP > 0; A/B)
    # The tier's choice counts probe rows whose exact partial score reaches thrP - PREFIX_BAND mP.
    # mP bounds |q~_P . x~_P - q_P . x_P| by Cauchy-Schwarz with the maxima over every row: the
    # worst case (band 1) needs each row's quantisation error to point along the query.  Errors
    # of unrelated direction reach mP / sqrt(64 PREFIX_KSTEPS) at one standard deviation (0.07 mP
    # at 192 dims), so a quarter of mP is about 3.5 of them.  At band 1 the headline's thrP - mP
    # is 0.08, 2.2 standard deviations of the bulk's partial scores: the estimate is 1.4M
    # candidates per query where the scan emits none beyond the whole-row scan's, and the tier
    # never ran (0 of 100 batches).  The choice is an estimate either way: a batch that emits
    # more than foreseen overflows PRUNE_CAP and takes the exact fall-back.
    PREFIX_BAND = 0.25

    def _prefix_enqueued(self, dense_tail: bool) -> bool:
        """Does this search enqueue the prefix scan beside the whole-row fp4 scan?  Only on a
        shard that tracked the prefix bounds over every row it wrote, and where both forms exist
        behind the second gate: the non-temporal stream scans at the default depth."""
        from ..ops import kernels as K

        return bool(self.prefix_tier and self.mx4_pbounds is not None and self.mx4_on
                    and self.img_mx4 is not None and self.prune_route and dense_tail
                    and self.scan_nt and K.scan_stream_nt_ok(self.dim, 1, self.scan_depth)
                    and K.scan_stream_prefix_ok(self.dim, 1, 0, self.prefix_ksteps))

    # the MX-fp4 tier's query-side centroid test (SYMB_MX4_CENTROID=0: off, A/B)
    mx4_centroid = os.environ.get("SYMB_MX4_CENTROID", "1") not in ("", "0")

    def _cent_args(self, m4, prefix: bool = False) -> dict:
        """index_scan_stream's centroid-test arguments for an MX-fp4 query context (none when the
        context has no centroids).  ``prefix``: for the prefix scan, whose rows' norm bound is
        X_P = mx4_pbounds[1] (the kernel reads element 1 of ``bounds4``): |x~_P| <= X_P <= X4, so
        the test c~_P . x~_P + R_s X_P skips more than with X4."""
        if m4 is None or "c4" not in m4:
            return {}
        b = self.mx4_pbounds if prefix else self.mx4_bounds
        return dict(cent4=m4["c4"].data_ptr(), centqs=m4["cqs"].data_ptr(),
                    centR=m4["cR"].data_ptr(), bounds4=b.data_ptr())

    # default of ``scan_reserve`` (profiles/r7_reserve/README.md has the sweep)
    SCAN_RESERVE = 96
    # default of ``scan_nt`` (profiles/r17_step/README.md has the A/B)
    SCAN_NT = 1

    def _scan_reserve(self, split: bool, n_cus: int, NQ: int) -> int:
        """CUs the stream scans of this search leave whole (``scan_reserve``), 0 outside the one
        case it is for: a split-phase search (``search_begin`` with ``n_cus=None``: its caller
        splits to run work beside the scan) while the tier hint says MX-fp4, on a shard whose
        two tiers are the stream scans.  That scan is HBM-bound and keeps its bandwidth on fewer
        CUs; the int8 scan is MFMA-bound and would lose its CUs' share, so a search the hint
        gives to int8 -- like a plain ``search`` -- keeps every CU.  A wrong hint costs only
        speed: the other tier runs on the same, smaller block grid."""
        if not (split and self.scan_reserve > 0 and self._tier_mx4 and self.mx4_on and self.stream
                and self.img_mx4 is not None and self.img_i8 is not None
                and not self._i8_heavy and not self.i8_ring
                and self.prune_route and NQ <= self.tail_dense_max_nq):   # (the tier is enqueued)
            return 0
        return max(0, min(int(self.scan_reserve), n_cus - 1))

    def _i8_geometry(self, n: int, NQ: int, n_cus: int, reserve: int = 0):
        """(rsplit, rows_per_blk, n_rblk) of the int8 scan over n rows: ~one workgroup per CU
        slot, whole tiles per block.  ``reserve`` (_scan_reserve; the stream scans only): CUs the
        CU-granular scan leaves whole."""
        from ..ops._ext import hip

        h = hip()
        heavy = self._i8_heavy
        rsplit = 2 if (NQ < 512 or self.i8_rsplit2) else 1
        if heavy and self.dim == 768:
            # (2 query sets per wave: the row-split form holds 128 queries per workgroup, the
            # other 256 -- a larger batch streams each row tile once per 256 queries)
            rsplit = 2 if (NQ <= h.i8_split_queries_per_blk(2, self.dim) or self.i8_rsplit2) else 1
        if self.stream:
            # the stream scans (one wave per SIMD): one block grid for both tiers, sized for the
            # tier with more workgroups per CU; rows_per_blk a multiple of 128 (the bf16 list
            # scan of routed blocks reads 64-row tiles).  A split-form shard runs its int8 tier
            # on the LDS-ring kernel: 64-row tiles there too.
            if heavy:
                n_qblk, wpc = math.ceil(NQ / h.i8_split_queries_per_blk(rsplit, self.dim)), 1
            elif self.i8_ring:   # (the LDS-ring int8 scan beside the stream fp4 tier)
                n_qblk, wpc = math.ceil(NQ / h.i8_queries_per_blk(rsplit)), h.i8_wgs_per_cu()
            else:
                qpb, wpc = h.stream_geometry(self.dim, 0)
                n_qblk = math.ceil(NQ / qpb)
            if self.mx4_on:
                qpbf, wpcf = h.stream_geometry(self.dim, 1)
                n_qblk, wpc = max(n_qblk, math.ceil(NQ / qpbf)), max(wpc, wpcf)
            # (>= 8192 rows per block: the route estimates each block from the exact sample's
            # 1-in-2^5 tiles, so a block needs a few sampled tiles -- ~1k-row blocks saw 0 or 1
            # and left crowded blocks to the int8 scan)
            # With a reserve R the scans run in the CU-granular form (index_stream.hip, PACK):
            # 4 waves per workgroup and one workgroup per CU, so wpc n_rblk n_qblk / 4 workgroups
            # occupy n_cus - R CUs: n_rblk ~ 4 (n_cus - R) / n_qblk for the fp4 form.  The same
            # limits hold: >= 8192 rows per block, <= 1024 blocks (ROUTE_MAX_BLOCKS),
            # rows_per_blk a multiple of 128.
            slots = (n_cus - reserve) * wpc if reserve > 0 else n_cus * wpc
            n_rblk = max(1, min(math.ceil(n / 8192), 1024, max(1, round(slots / n_qblk))))
            rows_per_blk = _round_up(max(1, math.ceil(n / n_rblk)), 128)
            n_rblk = max(1, math.ceil(n / rows_per_blk))
            return rsplit, rows_per_blk, n_rblk
        tr = h.i8_tile_rows(self.dim, heavy)
        if self.mx4_on and rsplit == 2:   # (one block grid for both tiers)
            tr = max(tr, h.mx4_tile_rows())
        if heavy:   # (the split image always runs 8-wave workgroups, one per CU)
            n_qblk, wpc = math.ceil(NQ / h.i8_split_queries_per_blk(rsplit, self.dim)), 1
        else:
            n_qblk, wpc = math.ceil(NQ / h.i8_queries_per_blk(rsplit)), h.i8_wgs_per_cu()
        n_rblk = max(1, min(math.ceil(n / (tr * 16)), max(1, round(n_cus * wpc / n_qblk))))
        rows_per_blk = _round_up(max(1, math.ceil(n / n_rblk)), tr)
        n_rblk = max(1, math.ceil(n / rows_per_blk))
        return rsplit, rows_per_blk, n_rblk

    def _mq_slots(self, NQ: int, n_cus: int):
        """(sets, rsplit, n_qblk, row slots) of a full-chip emitting-scan launch for NQ queries
        (as _scan_mq)."""
        from ..ops._ext import hip

        sets, rsplit = self._mq_form(NQ)
        n_qblk = math.ceil(NQ / hip().mq_queries_per_blk(sets, rsplit))
        return sets, rsplit, n_qblk, max(1, round(n_cus / n_qblk))

    def _pruned_end(self, ctx):
        """The full-shard half of the pruned search over the rows ``_pruned_begin`` saw, on the
        current stream (which may differ from the one the begin ran on: its tensors are marked
        as used here, so the allocator cannot recycle them under this stream's kernels)."""
        from ..ops._ext import hip, stream_handle

        h, dev, cap, kmax = hip(), self.device, self.PRUNE_CAP, 16
        cur = torch.cuda.current_stream(dev)
        for t in ("q", "q8", "sq", "thr", "T", "dense", "blk", "ws"):
            ctx[t].record_stream(cur)
        q_unit, k, n, n_cus = ctx["q"], ctx["k"], ctx["n"], ctx["n_cus"]
        q8, thr, T, dense, blk = ctx["q8"], ctx["thr"], ctx["T"], ctx["dense"], ctx["blk"]
        rsplit, rows_per_blk, n_rblk = ctx["geo"]
        NQ = q_unit.shape[0]
        st = stream_handle(dev)
        if ctx["gen"] != self._calib_gen:
            # the image was re-calibrated between the halves (a new basis / bounds): its query
            # image no longer matches -- the exact bf16 list scan, seeded with the exact T
            out = (torch.empty(NQ, k, device=dev), torch.empty(NQ, k, dtype=torch.int32, device=dev))
            self._scan(n, q_unit, kmax, k, T.contiguous(), n_cus, out=out)
            return out
        # 3. int8 scan of the blocks the route kept: emit every row with (q8 . x8) * sx >= thr
        #    (candidate counters and overflow flag: the workspace _pruned_begin cleared)
        ws = ctx["ws"]
        cnt = ws[NQ:2 * NQ]
        early = ctx.get("cand")   # (_pruned_begin: prefill and routed blocks already enqueued)
        if early is None:
            cs, ci = self._cand_buffers(NQ)
            n_scan = self._cand_prefill(h, st, NQ, n, ci, cnt)
        else:
            cs, ci, n_scan = early
            cs.record_stream(cur)
            ci.record_stream(cur)
        ovf = ws[2 * NQ + self.WS_OVF:2 * NQ + self.WS_OVF + 1]
        out_s = torch.empty(NQ, k, device=dev)
        out_i = torch.empty(NQ, k, dtype=torch.int32, device=dev)
        skip = blk[2 + n_rblk:].data_ptr() if self.prune_route else 0
        # both tiers are enqueued, gated on the MX-fp4 flag (0: the fp4 tier runs, 1: the int8 /
        # split tier): exactly one runs
        m4 = ctx.get("mx4")
        if m4 is not None:
            for t in ("q4", "qs4", "thr4", "c4", "cqs", "cR", "thrP"):
                if t in m4:
                    m4[t].record_stream(cur)
        tier = None if m4 is None else m4["nv"]
        gate, want = (0, 0) if tier is None else (tier.data_ptr(), 1)
        wide = int(ctx["wide"])   # the CU-granular stream scans on the reserve's block grid

        def tier_i8():
            if self.img_i8 is not None and not ctx["heavy"]:   # the stream scan (index_stream.hip)
                h.index_scan_stream(self.img_i8.data_ptr(), n_scan,
                                    self.img_i8.shape[0] * STREAM_SUB, rows_per_blk, n_rblk,
                                    q8.data_ptr(), 0, NQ, thr.data_ptr(), cs.data_ptr(),
                                    ci.data_ptr(), cnt.data_ptr(), cap, self.scan_xcd, st,
                                    skip=skip, dim=self.dim, form=0, gate=gate, gate_want=want,
                                    zero_cnt=0, wide=wide)
            else:
                h.index_scan_i8(self.rows_i8.data_ptr(), self.sx_i8.data_ptr(), n_scan,
                                self.rows_i8.shape[0], rows_per_blk, n_rblk,
                                q8.data_ptr(), NQ, thr.data_ptr(), cs.data_ptr(), ci.data_ptr(),
                                cnt.data_ptr(), cap, self.scan_xcd, st, rsplit, skip=skip,
                                dim=self.dim, heavy=ctx["heavy"], sq=ctx["sq"].data_ptr(),
                                gate=gate, gate_want=want, zero_cnt=0)

        def tier_mx4():
            from ..ops import kernels as K

            if self.img_mx4 is not None:
                # (runs: the device counter of searches whose first tier was this scan)
                runs = 0
                if self.mq_stats or self.tier_stats:
                    if self._mx4_tot is None:
                        self._mx4_tot = torch.zeros(1, dtype=torch.int32, device=dev)
                    runs = self._mx4_tot.data_ptr()
                depth = self.scan_depth if self.dim == 384 else 0
                pk = {}
                if "thrP" in m4:
                    # one launch for the fp4 tier: the kernel reads the form word and runs the
                    # prefix form (thrP, X_P in the centroid test) or the whole-row form (thr4)
                    if self._pfx_tot is None:
                        self._pfx_tot = torch.zeros(1, dtype=torch.int32, device=dev)
                    depth = K.SCAN_PREFIX_DEEP[self.prefix_ksteps]
                    pk = dict(prefix=self.prefix_ksteps, pbounds=self.mx4_pbounds,
                              thr_prefix=m4["thrP"].data_ptr(), gate2=m4["nvp"].data_ptr(),
                              runs2=self._pfx_tot.data_ptr())
                K.index_scan_stream(self.img_mx4.data_ptr(), n_scan,
                                    self.img_mx4.shape[0] * STREAM_SUB, rows_per_blk, n_rblk,
                                    m4["q4"].data_ptr(), m4["qs4"].data_ptr(), NQ,
                                    m4["thr4"].data_ptr(), cs.data_ptr(), ci.data_ptr(),
                                    cnt.data_ptr(), cap, self.scan_xcd, st, skip=skip,
                                    dim=self.dim, form=1, gate=m4["nv"].data_ptr(), gate_want=0,
                                    zero_cnt=0, runs=runs, wide=wide, depth=depth,
                                    nt=int(bool(self.scan_nt)
                                           and (bool(pk) or K.scan_stream_nt_ok(self.dim, 1, depth))),
                                    **pk, **self._cent_args(m4))
            else:
                h.index_scan_i8(self.rows_mx4.data_ptr(), self.sc_mx4.data_ptr(), n_scan,
                                self.rows_mx4.shape[0], rows_per_blk, n_rblk, m4["q4"].data_ptr(),
                                NQ, m4["thr4"].data_ptr(), cs.data_ptr(), ci.data_ptr(),
                                cnt.data_ptr(), cap, self.scan_xcd, st, rsplit, skip=skip,
                                dim=self.dim, sq=m4["qs4"].data_ptr(), form=1,
                                gate=m4["nv"].data_ptr(), gate_want=0)

        # The tier the hint expects goes first: the other launch exits at its gate, but even a
        # no-op launch of these kernels waits for SIMDs (the CU-granular form: a CU) with a free
        # register file, and in front of the real scan that wait is on the step's critical path.
        # Both write the same buffers and exactly one runs, so the order changes no result.
        if m4 is None:
            tier_i8()
        elif ctx["hint_mx4"]:
            tier_mx4()
            tier_i8()
        else:
            tier_i8()
            tier_mx4()
        # 3'. the bf16 emitting scan of the blocks the route listed, into the same candidate
        #     buffers (a split-phase search ran it in its begin half)
        if early is None:
            self._route_scan(h, st, q_unit, n_scan, n_cus, T, blk, rows_per_blk, cs, ci, cnt)
        # 4. exact bf16 re-score of every candidate, 5. top-k -- one launch (prune_finish.hip),
        #    which also stores the tier word for a later search's hint into a pinned host word
        flag, host_word = None, 0
        if self.prune_fused_finish:
            from ..ops import kernels as K

            if tier is not None and dev.type == "cuda":
                flag, host_word = self._tier_word()
            K.prune_finish(self.rows, q_unit, ci, cnt, cs, k, out_s, out_i, ovf,
                           tier=tier if host_word else None, host_word=host_word)
        else:
            h.rescore_bf16(self.rows.data_ptr(), q_unit.data_ptr(), NQ, self.dim, ci.data_ptr(),
                           cnt.data_ptr(), cap, cs.data_ptr(), st)
            h.topk_select_counted(cs.data_ptr(), ci.data_ptr(), cnt.data_ptr(), cap, NQ, kmax, k,
                                  out_s.data_ptr(), out_i.data_ptr(), ovf.data_ptr(), st,
                                  reset_ovf=False)
        # overflow (some query had more than cap candidates): the exact bf16 scan, seeded with T
        self._scan(n, q_unit, kmax, k, T.contiguous(), n_cus, gate=ovf, out=(out_s, out_i))
        self._mq_last = (cnt, ovf)
        self._route_last = dense
        self._mx4_last = None if m4 is None else m4["nv"]   # 0: the MX-fp4 tier ran
        self._tier_last = tier   # 0 fp4, 1 int8 / split
        # 0: the prefix form ran if an fp4 tier did (None: the prefix scan was not enqueued)
        self._pfx_last = None if m4 is None else m4.get("nvp")
        if tier is not None and dev.type == "cuda":
            if flag is None:   # (no fused finish, or no device address for the pinned word)
                flag = torch.empty(1, dtype=torch.int32, pin_memory=True)
                flag.copy_(tier, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cur)
            with self._tier_lock:
                self._tier_pending.append((flag, ev))
                while len(self._tier_pending) > 8:    # (a caller that never begins another search)
                    self._tier_pending.popleft()
        if (self.mq_stats or self.tier_stats) and m4 is not None and self.img_mx4 is None:
            if self._mx4_tot is None:
                self._mx4_tot = torch.zeros(1, dtype=torch.int32, device=dev)
            self._mx4_tot.add_(1 - m4["nv"])   # (the LDS-ring fp4 scan counts no runs itself)
        self._route_blk_last = blk
        if self.mq_stats:   # (diagnostics: the scan's inputs and grid)
            self._pruned_last = dict(q8=q8, thr=thr, sq=ctx["sq"], rows_per_blk=rows_per_blk,
                                     n_rblk=n_rblk, cap=cap, cs=cs, ci=ci, cnt=cnt, q=q_unit,
                                     m4=m4, heavy=ctx["heavy"])
        self._stats(ovf, cnt, dense, blk)
        return out_s, out_i

    def _prune_thresholds_torch(self, q_unit, pre_s, tail_s, k: int):
        """Torch composition of prune_qprep (test oracle): (T, q8, sq, thr)."""
        NQ = q_unit.shape[0]
        T = torch.topk(torch.cat([pre_s, tail_s], 1), k, dim=1).values[:, k - 1] - self.MQ_THR_MARGIN
        q8 = torch.empty(NQ, self.dim, dtype=torch.int8, device=self.device)
        sq = torch.empty(NQ, dtype=torch.float32, device=self.device)
        eq, _ = self._quant_i8(q_unit, q8, sq)
        E, X = self.i8_bounds[0], self.i8_bounds[1]
        margin = q_unit.float().norm(dim=1) * E + eq * X + 1e-5
        return T, q8, sq, ((T - margin) / sq).contiguous()

    K_MAX_HIP = 128          # top_k up to this runs on the HIP scans (radix select); above: matmul
    LARGE_K_CAP = 16384      # candidate slots per query of the large-k emitting scan

    def _search_large_k(self, q_unit, k: int, n_cus):
        """EXACT top-k for 16 < k <= 128 on a bf16 shard (D = 384 / 768 / 1024): T = the k-th best exact score
        of a 1-in-32 tile sample of real rows (seeded from a 1-in-2048 sub-sample scored by an
        fp32 GEMM) plus the fresh-row tail, then the bf16 emitting scan keeps every row scoring
        >= T (a lower bound on each query's final k-th score), and the radix select
        (topk_select_radix_kernel) takes each query's top k.  A query whose candidates overflow
        LARGE_K_CAP sends the batch to the exact chunked GEMM (host check; rare).  None when the
        shard is too small or not a bf16 shard of an emitting-scan width (the caller takes the
        list scan / GEMM)."""
        n, NQ = self.visible, q_unit.shape[0]
        if (self.dtype != "bf16" or self.dim not in MQ_DIMS or not self.scan_mq
                or k > self.K_MAX_HIP):
            return None
        if n < self.SEED_MIN_ROWS:
            return None
        plan = self._tile_sample_plan(n, self.PRUNE_TILE_SHIFT)
        if plan is None:
            return None
        ts, nv, t0, idx = plan
        if idx.numel() < k or n - t0 < 1:
            return None
        if n_cus is None:
            n_cus = self._n_cus()
        qf = q_unit.float()
        sub = torch.index_select(self.rows, 0, idx)
        s0 = torch.topk(qf @ sub.float().t(), k, dim=1).values
        thr0 = (s0[:, k - 1] - self.MQ_THR_MARGIN).contiguous()
        pre_s, _ = self._scan_mq(nv * TILE_ROWS, q_unit, 128, k, thr0, n_cus, tshift=ts,
                                 fallback=False, cap=self.SAMPLE_CAP)
        ts_ = qf @ self.rows[t0:n].float().t()
        kk = min(k, n - t0)
        tail_s = torch.topk(ts_, kk, dim=1).values
        T = torch.topk(torch.cat([pre_s, tail_s], 1), k, dim=1).values[:, k - 1]
        T = (T - self.MQ_THR_MARGIN).contiguous()
        # this search's own overflow flag (self._mq_last is shared by concurrent searches)
        ovf = torch.empty(1, dtype=torch.int32, device=self.device)
        out_s = torch.empty(NQ, k, device=self.device)
        out_i = torch.empty(NQ, k, dtype=torch.int32, device=self.device)
        self._scan_mq(n, q_unit, 128, k, T, n_cus, fallback=False, cap=self.LARGE_K_CAP,
                      out=(out_s, out_i, ovf))
        if int(ovf.item()):
            return self._search_matmul(q_unit, k)
        return out_s, out_i

    def _search_prefilter(self, q_unit, k: int, n_cus):
        """fp8 scan for oversample*k candidates, exact bf16 re-score, top-k (see the class doc)."""
        kc = min(32, max(16, self.oversample * k))
        _, cand = self._search_scan(q_unit, kc, self.rows8, "fp8", n_cus)    # [NQ, kc] rows
        if self.dim in MQ_DIMS:
            # the pruned search's kernels: exact bf16 re-score of the candidate rows (8 waves per
            # query gather them) and the counted select; the scan's list is score-sorted, so the
            # valid candidates are a prefix of each row
            from ..ops._ext import hip, stream_handle

            NQ, st, h = q_unit.shape[0], stream_handle(self.device), hip()
            cand = cand.contiguous()
            cnt = (cand >= 0).sum(1, dtype=torch.int32)
            cs = torch.empty(NQ, kc, device=self.device)
            h.rescore_bf16(self.rows.data_ptr(), q_unit.data_ptr(), NQ, self.dim, cand.data_ptr(),
                           cnt.data_ptr(), kc, cs.data_ptr(), st)
            out_s = torch.empty(NQ, k, device=self.device)
            out_i = torch.empty(NQ, k, dtype=torch.int32, device=self.device)
            ovf = torch.empty(1, dtype=torch.int32, device=self.device)
            h.topk_select_counted(cs.data_ptr(), cand.data_ptr(), cnt.data_ptr(), kc, NQ,
                                  16 if kc <= 16 else 32, k, out_s.data_ptr(), out_i.data_ptr(),
                                  ovf.data_ptr(), st)
            return out_s, out_i
        valid = cand >= 0
        rows = self.rows[cand.clamp_min(0).long()]                           # [NQ, kc, D] bf16
        exact = torch.bmm(rows.float(), q_unit.float().unsqueeze(-1)).squeeze(-1)
        exact = torch.where(valid, exact, torch.full_like(exact, -math.inf))
        top_s, j = torch.topk(exact, k, dim=1)
        top_i = torch.gather(cand, 1, j)
        return top_s, torch.where(torch.isfinite(top_s), top_i, torch.full_like(top_i, -1))

    SEED_DIV = 64            # sample = first n/64 rows (~1.6% extra scan work)
    SEED_MIN_ROWS = 1 << 20  # below this the record-breaking inserts are cheap anyway
    # visible rows from which an fp8 shard at 32 < k <= 128 takes the emitting e4m3 scan (the gate
    # _search_large_k applies on bf16): below it the chunked matmul costs milliseconds
    FP8_LARGE_K_MIN_ROWS = SEED_MIN_ROWS

    def _seed_rows(self, n: int, k: int) -> int:
        if not self.seed_threshold or n < self.SEED_MIN_ROWS:
            return 0
        return max(_round_up(n // self.SEED_DIV, TILE_ROWS), _round_up(k, TILE_ROWS))

    def _n_cus(self) -> int:
        """Workgroups (CUs) a scan spreads over: all of them unless ``scan_cus`` leaves some to
        work running beside the search on another stream (e.g. the next batch's encoder)."""
        n = getattr(self, "_cus", None)
        if n is None:
            n = self._cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        return min(n, self.scan_cus) if self.scan_cus else n

    def _scan(self, n: int, q_unit: torch.Tensor, kmax: int, k: int, thr, n_cus, rows=None,
              dtype=None, gate=None, out=None, min_tiles: int | None = None):
        """Fused 256-query scan + merge.  ``gate`` (int32 device flag): the kernels skip
        themselves unless it is non-zero; ``out``: (scores, rows) tensors to write;
        ``min_tiles``: row-block floor in 64-row tiles (default ``scan_min_tiles``)."""
        from ..ops._ext import hip, stream_handle

        rows = self.rows if rows is None else rows
        dtype = dtype or self.dtype
        NQ = q_unit.shape[0]
        if dtype == "fp8":
            lists, qpb = 2, 256
        else:
            lists, qpb = hip().topk_geometry(self.dim, kmax)
        n_qblk = math.ceil(NQ / qpb)
        if n_cus is None:
            n_cus = self._n_cus()
        min_tiles = self.scan_min_tiles if min_tiles is None else min_tiles
        n_rblk = max(1, min(math.ceil(n / (TILE_ROWS * min_tiles)),
                            max(1, round(n_cus / n_qblk))))
        rows_per_blk = _round_up(max(1, math.ceil(n / n_rblk)), TILE_ROWS)
        n_rblk = max(1, math.ceil(n / rows_per_blk))
        ncand = n_rblk * lists * kmax
        # candidate workspace per call: concurrent searches (service executor threads share the
        # stream) must never read each other's candidates; the caching allocator makes this free
        cs = torch.empty(NQ, ncand, device=self.device)
        ci = torch.empty(NQ, ncand, dtype=torch.int32, device=self.device)
        if out is None:
            out = (torch.empty(NQ, k, device=self.device),
                   torch.empty(NQ, k, dtype=torch.int32, device=self.device))
        out_s, out_i = out
        gate_p = 0 if gate is None else gate.data_ptr()
        st = stream_handle(self.device)
        h = hip()
        thr_p = 0 if thr is None else thr.data_ptr()
        if dtype == "fp8":
            h.index_scan_fp8(rows.data_ptr(), n, self.dim, rows_per_blk, n_rblk,
                             q_unit.data_ptr(), NQ, kmax, cs.data_ptr(), ci.data_ptr(), st,
                             self.scan_aux, thr_p, self.scan_xcd)
        else:
            h.index_scan(rows.data_ptr(), n, self.dim, rows_per_blk, n_rblk, q_unit.data_ptr(),
                         NQ, kmax, cs.data_ptr(), ci.data_ptr(), st, self.scan_aux, thr_p,
                         self.scan_xcd, gate_p)
        h.topk_merge(cs.data_ptr(), ci.data_ptr(), NQ, ncand, kmax, k, out_s.data_ptr(),
                     out_i.data_ptr(), 0, 0, st, gate_p)
        return out_s, out_i

    def _search_matmul(self, q_unit: torch.Tensor, k: int, chunk: int = 1 << 22, mask=None):
        """Chunked exact fallback (CPU backend; on the GPU k > 128, k > 32 where no emitting scan
        serves the shard -- an fp8 shard below FP8_LARGE_K_MIN_ROWS rows among them -- and a
        large-k search whose candidates overflowed).  Each chunk's fp32 score block
        stays <= 512 MiB: one GEMM output past 2 GiB came back with its tail unwritten on the
        GPU stack (benchmarks/diag/gemm_2g.py).  ``mask`` (RowMask): disallowed rows score -inf;
        score column j of a chunk is row s + j, so the chunk takes the mask's rows [s, e)."""
        NQ = q_unit.shape[0]
        chunk = max(min(chunk, 4096), min(chunk, (1 << 27) // max(1, NQ)))
        best_s = torch.full((NQ, k), -math.inf, device=self.device)
        best_i = torch.full((NQ, k), -1, dtype=torch.int64, device=self.device)
        q = q_unit.to(self.device).float()
        n = self.visible
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            sc = q @ self._rows_f32(s, e).t()
            if mask is not None:
                sc.masked_fill_(~mask.bool_rows(s, e)[None, :], -math.inf)
            kk = min(k, e - s)
            ts, ti = torch.topk(sc, kk, dim=1)
            cat_s = torch.cat([best_s, ts], 1)
            cat_i = torch.cat([best_i, ti + s], 1)
            best_s, idx = torch.topk(cat_s, k, dim=1)
            best_i = torch.gather(cat_i, 1, idx)
        best_i = torch.where(torch.isfinite(best_s), best_i, torch.full_like(best_i, -1))
        return best_s, best_i.to(torch.int32)

    def _rows_f32(self, s: int, e: int) -> torch.Tensor:
        r = self.rows[s:e]
        if self.dtype == "fp8":
            return r.view(torch.float8_e4m3fn).float() / FP8_SCALE
        return r.float()

    def unit_rows(self) -> torch.Tensor:
        """The stored rows as bf16 (fp8 shards: decoded, a copy)."""
        if self.dtype == "fp8":
            return self._rows_f32(0, self.count).bfloat16()
        return self.rows[:self.count]
