#!/usr/bin/env python3
"""Search over a shard with tombstones (HbmIndexShard.delete_rows, csrc/hip/index_delete.hip): what
a delete costs every later search under the two routes, on one shard of random unit rows with
held-out random queries.

    delete_route = "zero"   the unmasked route (pruned / list scan) + the dead-id check + the
                            gated masked scan, which exits at once while no dead row came back
    delete_route = "mask"   every search with tombstones is the masked list scan under ~dead

First the search before any delete, in two alternated runs of the same call (``search_a`` /
``search_b``): the spread between them is what the no-delete search shows by itself.  Then, after
each cumulative delete level (shares of the rows, as uniform random rows or as runs of 200 rows,
"documents"), in alternated rounds on the same shard, one JSON line per variant:

  route_only   shard._search_route(q, k): the search code as it runs before any delete, over the
               same bytes (zeroed rows included) -- the yardstick of the "zero" route's overhead
  zero         shard.search(q, k) under delete_route = "zero"
  mask         shard.search(q, k) under delete_route = "mask"

Every line carries ``last_dead_hits`` (must be 0: each query keeps k live rows scoring above 0),
``rows_equal_mask`` (the result against the masked scan's: same rows outside runs of equal scores)
and ``max_abs_vs_mask``; the ``delete`` lines carry the cost of the delete itself per 1k rows.

k > 32 (the masked emitting scan is the masked route: index_mq_filter.hip on bf16 shards,
index_emit_fp8.hip on fp8 shards of FP8_LARGE_K_MIN_ROWS rows or more, where it is the unmasked
route too, under an all-ones mask): the ``mask`` line, and on fp8 every line but ``zero``, also
carries ``overflow`` (the candidate-overflow flag: 1 = the search fell back to the masked matmul)
and ``max_candidates``; --fallback adds ``matmul_mask``, one iteration of the chunked matmul
under ~dead, the route of such a search before the masked emitting scan.

--compact adds, after the last level's lines (nothing above changes), the in-place compaction
(HbmIndexShard.compact, csrc/hip/index_compact.hip) of what the levels left:

  tombstoned     shard.search(q, k) under the shard's default delete route, just before
  compact_torch  the same plan run with torch on a copy of the row slab: index_select per window
                 plus copy_ (the route without the kernel; it needs that second slab, the int64
                 index of every window and a bool per row); the copy is then the check of
                 compact()'s rows, ``rows_equal``
  compact        shard.compact() itself, plan, moves, zeroed tail and re-imaging included;
                 ``reimage_ms`` is the re-imaging alone (run once more: it is idempotent),
                 ``gbps`` the bytes of the rows above the first dead row over the time less that
  compacted /    shard.search(q, k) on the compacted shard and on a fresh shard of the same rows
  fresh          that never saw a delete, alternated (``fresh`` is skipped where both do not fit)

    python benchmarks/delete_bench.py [--rows 100000000] [--dim 384] [--dtype bf16|fp8]
        [--prune i8|none] [--pattern uniform|docs] [--levels 0.01,1,10] [--nq 256] [--k 10]
        [--rounds 3] [--iters 5] [--out FILE] [--fallback] [--compact]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

DOC_ROWS = 200


def pick_rows(pattern: str, n: int, n_new: int, live: torch.Tensor, g) -> torch.Tensor:
    """~n_new live rows to delete: uniform random rows, or whole runs of DOC_ROWS rows."""
    dev = live.device
    if pattern == "uniform":
        hit = (torch.rand(n, device=dev, generator=g) < n_new / max(1, int(live.sum()))) & live
        return torch.nonzero(hit).flatten()
    n_docs = max(1, round(n_new / DOC_ROWS))
    starts = torch.randint(0, n - DOC_ROWS, (n_docs,), device=dev, generator=g)
    edge = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    one = torch.ones(n_docs, dtype=torch.int32, device=dev)
    edge.index_add_(0, starts, one)
    edge.index_add_(0, starts + DOC_ROWS, -one)
    return torch.nonzero((torch.cumsum(edge[:n], 0, dtype=torch.int32) > 0) & live).flatten()


def rows_equal_outside_ties(s, r, ref_s, ref_r, tol: float) -> bool:
    tie = torch.zeros_like(r, dtype=torch.bool)
    for a in (s, ref_s):
        tie[:, 1:] |= (a[:, 1:] - a[:, :-1]).abs() <= tol
        tie[:, :-1] |= (a[:, :-1] - a[:, 1:]).abs() <= tol
    return bool(((r == ref_r) | tie).all())


def timed(fn, iters: int) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--dtype", choices=("bf16", "fp8"), default="bf16")
    ap.add_argument("--prune", default="i8", help="i8 (bf16 shards) or none")
    ap.add_argument("--pattern", choices=("uniform", "docs"), default="uniform")
    ap.add_argument("--levels", default="0.01,1,10", help="cumulative dead shares, percent")
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--fallback", action="store_true",
                    help="also time the chunked matmul under ~dead (one iteration per level)")
    ap.add_argument("--compact", action="store_true",
                    help="after the last level: compact the shard, against the torch route")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("delete_bench needs the GPU: nothing here is measured without one")
    from codename_symbiont_amd.index.shard import HbmIndexShard

    dev = torch.device("cuda")
    n, k = a.rows, a.k
    prune = "i8" if (a.prune == "i8" and a.dtype == "bf16") else None
    shard = HbmIndexShard(a.dim, n, device=dev, dtype=a.dtype, prune=prune)
    shard.fill_random(n, seed=1)
    g = torch.Generator(device=dev).manual_seed(77)      # held out: not rows of the shard
    q = torch.nn.functional.normalize(torch.randn(a.nq, a.dim, device=dev, generator=g),
                                      dim=-1).bfloat16()
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    base = {"bench": "delete_bench", "rows": n, "dim": a.dim, "dtype": a.dtype,
            "prune": prune or "none", "pattern": a.pattern, "nq": a.nq, "k": k,
            "rounds": a.rounds, "iters": a.iters}
    tol = 2e-3

    def run(variants: dict, info: dict, ref=None) -> dict:
        """Alternated rounds of every variant; one line each; returns (medians, all times)."""
        res, hits, large = {}, {}, {}
        for v, fn in variants.items():               # results first (also the warm-up)
            shard.last_dead_hits = None
            shard._filter_large_k_last = None
            res[v] = fn()
            hits[v] = 0 if shard.last_dead_hits is None else int(shard.last_dead_hits)
            last = shard._filter_large_k_last
            # (not "zero": its gated fallback runs last, and behind a closed gate it leaves the
            # counts unwritten)
            if v != "zero" and last is not None:
                large[v] = {"overflow": int(last[1]), "max_candidates": int(last[0].max())}
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for _ in range(a.rounds):
            for v, fn in variants.items():
                times[v].append(timed(fn, a.iters))
        med = {}
        for v, ts in times.items():
            extra = {}
            if ref is not None:
                s, r = res[v]
                extra = {"rows_equal_mask": rows_equal_outside_ties(s, r, ref[0], ref[1], tol),
                         "max_abs_vs_mask": float((s - ref[0]).abs().max())}
            med[v] = statistics.median(ts)
            emit(dict(info, variant=v, ms=round(med[v], 3), ms_min=round(min(ts), 3),
                      ms_max=round(max(ts), 3), last_dead_hits=hits[v], **extra,
                      **large.get(v, {})))
        return med, times

    def search(route):
        shard.delete_route = route
        return shard.search(q, k)

    # before any delete: the same call in two alternated runs
    plain, pt = run({"search_a": lambda: shard.search(q, k),
                     "search_b": lambda: shard.search(q, k)}, dict(base, dead=0, dead_share=0.0))
    # (the range of every round of both runs)
    spread = max(pt["search_a"] + pt["search_b"]) - min(pt["search_a"] + pt["search_b"])
    live = torch.ones(n, dtype=torch.bool, device=dev)
    for li, level in enumerate(float(x) for x in a.levels.split(",")):
        want = round(level / 100.0 * n) - shard.n_dead
        rows = pick_rows(a.pattern, n, want, live, g)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_new = shard.delete_rows(rows)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        live[rows] = False
        del rows
        info = dict(base, dead=shard.n_dead, dead_share=round(shard.n_dead / n, 6))
        emit(dict(info, variant="delete", deleted=n_new, ms=round(dt, 3),
                  ms_per_1k_rows=round(dt / max(1, n_new) * 1e3, 4)))
        ref = search("mask")
        torch.cuda.synchronize()
        med, _ = run({"route_only": lambda: shard._search_route(q, k, None),
                      "zero": lambda: search("zero"), "mask": lambda: search("mask")}, info, ref)
        if a.fallback:
            ms = timed(lambda: shard._search_matmul(q, k, mask=shard._live()), 1)
            emit(dict(info, variant="matmul_mask", ms=round(ms, 3), ms_min=round(ms, 3),
                      ms_max=round(ms, 3), iters=1, rounds=1))
        over = med["zero"] - med["route_only"]
        emit(dict(info, variant="summary", no_delete_ms=round(plain["search_a"], 3),
                  no_delete_spread_ms=round(spread, 3), zero_overhead_ms=round(over, 3),
                  zero_overhead_within_spread=bool(over <= spread),
                  zero_vs_no_delete_ms=round(med["zero"] - plain["search_a"], 3),
                  zero_beats_mask=bool(med["zero"] < med["mask"])))
    if a.compact and shard.n_dead:
        compact_section(shard, a, q, k, run, emit, base)


def compact_torch(rows: torch.Tensor, dead: torch.Tensor, count: int, c, windows) -> None:
    """The plan of a compaction executed on ``rows`` with torch alone."""
    from codename_symbiont_amd.index.shard import _unpack_bits

    live = ~_unpack_bits(dead)[:count]
    for t0, t1, _mode in windows:
        d0, d1 = int(c[t0]), int(c[t1])
        if d1 == d0:
            continue
        s0, s1 = t0 * 64, min(t1 * 64, count)
        idx = torch.nonzero(live[s0:s1]).flatten() + s0
        rows[d0:d1].copy_(rows.index_select(0, idx))


def compact_section(shard, a, q, k, run, emit, base) -> None:
    import numpy as np

    from codename_symbiont_amd.index.shard import (COMPACT_STAGE_BYTES, STREAM_SUB, TILE_ROWS,
                                                   HbmIndexShard, compact_plan)

    old, n_dead = shard.count, shard.n_dead
    info = dict(base, dead=n_dead, dead_share=round(n_dead / old, 6))
    shard.delete_route = shard.DELETE_ROUTE_DEFAULT[a.dtype]
    run({"tombstoned": lambda: shard.search(q, k)}, dict(info, delete_route=shard.delete_route))
    row_bytes = shard.dim * shard.rows.element_size()
    stage_rows = max(TILE_ROWS, COMPACT_STAGE_BYTES // row_bytes // TILE_ROWS * TILE_ROWS)
    alt = None
    try:
        alt = shard.rows.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c, windows = compact_plan(shard._dead_host, old, stage_rows)
        t1 = time.perf_counter()
        compact_torch(alt, shard.dead, old, c, windows)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        b = int(np.flatnonzero(shard._dead_host)[0])
        first = 8 * b + int(np.flatnonzero(np.unpackbits(shard._dead_host[b:b + 1],
                                                         bitorder="little"))[0])
        moved_bytes = (old - first) * row_bytes
        emit(dict(info, variant="compact_torch", ms=round((t2 - t0) * 1e3, 3),
                  plan_ms=round((t1 - t0) * 1e3, 3), windows=len(windows),
                  direct=sum(m == "direct" for _, _, m in windows),
                  gbps=round(moved_bytes / (t2 - t0) / 1e9, 1)))
    except torch.OutOfMemoryError:
        alt = None
        emit(dict(info, variant="compact_torch", skipped="a second row slab does not fit"))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    shard.compact()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lc = shard.last_compact
    live = shard.count
    r0 = lc["first_row"] // STREAM_SUB * STREAM_SUB
    t0 = time.perf_counter()
    if shard.prune_on or shard.mx4_on:
        for s in range(r0, old, 1 << 18):
            shard._image_rows(s, min(old, s + (1 << 18)) - s)
    torch.cuda.synchronize()
    reimage = time.perf_counter() - t0
    equal = None
    if alt is not None:
        equal = all(torch.equal(alt[s:min(live, s + (1 << 22))],
                                shard.rows[s:min(live, s + (1 << 22))])
                    for s in range(0, live, 1 << 22))
    del alt
    all_bytes = (old - lc["first_row"]) * sum(
        t.shape[1] * t.element_size() for t in (shard.rows, shard.rows8) if t is not None)
    emit(dict(info, variant="compact", ms=round(dt * 1e3, 3), reimage_ms=round(reimage * 1e3, 3),
              rows_equal=equal, **lc,
              gbps=round(all_bytes / max(dt - reimage, 1e-9) / 1e9, 1)))
    info = dict(base, dead=0, dead_share=0.0, rows=live, compacted_from=old)
    variants = {"compacted": lambda: shard.search(q, k)}
    try:
        fresh = HbmIndexShard(shard.dim, live, device=shard.device, dtype=shard.dtype,
                              prune=shard.prune)
        fresh._reserve(live)
        fresh.rows[:live].copy_(shard.rows[:live])
        fresh.rows_written(0, live)
        fresh.publish()
        variants["fresh"] = lambda: fresh.search(q, k)
    except torch.OutOfMemoryError:
        fresh = None
        emit(dict(info, variant="fresh", skipped="a second shard does not fit"))
    med, times = run(variants, info)
    if "fresh" in med:
        s, r = shard.search(q, k)
        fs, fr = fresh.search(q, k)
        emit(dict(info, variant="compact_summary",
                  compacted_vs_fresh_ms=round(med["compacted"] - med["fresh"], 3),
                  fresh_spread_ms=round(max(times["fresh"]) - min(times["fresh"]), 3),
                  rows_equal_fresh=rows_equal_outside_ties(s, r, fs, fr, 2e-3),
                  max_abs_vs_fresh=float((s - fs).abs().max())))


if __name__ == "__main__":
    main()
