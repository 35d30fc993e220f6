#!/usr/bin/env python3
"""Filtered search (exact top-k under a row mask, csrc/hip/index_filter.hip; index_filter_fp8.hip
with --dtype fp8) against what a caller could do before it, on one shard of random unit rows with
held-out random queries.

Per mask, in alternated rounds on the same shard (one JSON line per mask and variant):

  filtered_seed    shard.search(q, k, allow=mask), seed pass on
  filtered_noseed  ... seed pass off
  gather_scan      index_select of the allowed rows, then the unfiltered list scan (_scan) over
                   the copy, ids mapped back (skipped where the copy does not fit)
  search           the unfiltered shard.search(q, k)            (yardstick, mask-independent)
  plain_scan       the unfiltered, unseeded list scan (_scan)  (yardstick, mask-independent)
  matmul_mask      (--fallback) the chunked matmul under the mask, the route of every shard the
                   masked scan does not serve and of fp8 shards before it did: one iteration

k > 32 (the masked emitting scan: index_mq_filter.hip on bf16 shards, index_emit_fp8.hip on fp8
shards of FP8_LARGE_K_MIN_ROWS rows or more): the list scans stop at kmax = 32, so the variants
are ``filtered`` (shard.search(q, k, allow=mask)), ``search`` (the unfiltered top-k; on an fp8
shard the same route under an all-ones mask) and ``search_k32`` (the unfiltered list-scan search
at k = 32, as context), plus matmul_mask with --fallback; every line of a search that took the
emitting route carries ``overflow`` (the route's candidate-overflow flag: 1 means the search fell
back to the masked matmul), ``max_candidates`` (the most candidates one query emitted) and
``cap`` (LARGE_K_CAP).

--dtype fp8: the shard holds e4m3 rows, gather_scan is the fp8 list scan over the index_select-ed
bytes, and every record carries "dtype": "fp8", rows_equal_gather (the masked scan's rows against
gather_scan's: equal outside runs of equal scores, and a last slot that differs without an equal
neighbour proved a tie by searching its two rows alone, rows_equal_outside_ties) and
last_slot_ties_proved (how many such slots there were).  Scores are compared in cosine units
(raw / FP8_SCALE**2).

Masks: all ones; uniform random bits; "documents" = runs of 200 consecutive rows.  The RowMask
(packed bits + live-tile list) and the gather's row list are built once per mask, outside the
timed loops; ``mask_ms`` is that one-off cost of the RowMask.

--groups 2,4,8 (bf16 at k <= 32, --dtype fp8 at k <= 128; replaces the per-mask run): a mask per
query.  For every case of --group-cases and every G, G masks are built and the nq queries dealt over them in turn
(query i under mask i % G); per case and G, alternated in one process:

  grouped       shard.search(q, k, allow=MaskGroups): the grouped scan (index_filter_group.hip;
                index_filter_group_fp8.hip on an fp8 shard; at k > 32 on an fp8 shard the
                grouped emitting scan, index_emit_group_fp8.hip, "emit"), or per chunk whatever
                ``grouped_routes`` names (--force-scan: always the scan)
  group_loop    the same call with the grouped scan off: one single-mask search per group, the
                only way to answer such a burst before the grouped scan
  union_floor   all nq queries under the union of the masks in the single-mask scan (at
                k > 32 the single-mask emitting search): the rows the grouped scan has to walk,
                without its per-lane mask select
  single_mask   all nq queries under mask 0 alone (a search that never enters the new kernel)

Cases: n1 = must_not-style, each mask excludes a different 1 % of the rows (as documents);
d1 / d0.1 = disjoint document masks of 1 % / 0.1 % each; u50 = uniform 50 %, a seed per mask.
Every line carries grouped_equals_loop (scores bit for bit, rows outside runs of equal scores;
on fp8 a last slot that differs without an equal neighbour must be proved a tie as above, and
last_slot_ties_proved counts them).  At k > 32 every line also carries, from the grouped
variant's last chunk, ``overflow`` (1: the chunk's candidates passed LARGE_K_CAP and the per-mask
loop answered it), ``max_candidates`` (the most one query emitted) and ``cap``.

    python benchmarks/filter_bench.py [--rows 100000000] [--dim 384] [--nq 256] [--k 10]
        [--masks ones,u50,u10,u1,d10,d1,d0.1] [--rounds 3] [--iters 5] [--out FILE]
        [--dtype bf16|fp8] [--fallback] [--groups 2,4,8 [--group-cases n1,d1,d0.1,u50] [--force-scan]]
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


def build_allow(name: str, n: int, dev, seed: int) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(seed)
    if name == "ones":
        return torch.ones(n, dtype=torch.bool, device=dev)
    share = float(name[1:]) / 100.0
    if name[0] == "u":
        return torch.rand(n, device=dev, generator=g) < share
    if name[0] == "d":
        n_docs = max(1, round(share * n / DOC_ROWS))
        starts = torch.randint(0, n - DOC_ROWS, (n_docs,), device=dev, generator=g)
        edge = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        one = torch.ones(n_docs, dtype=torch.int32, device=dev)
        edge.index_add_(0, starts, one)
        edge.index_add_(0, starts + DOC_ROWS, -one)
        return torch.cumsum(edge[:n], 0, dtype=torch.int32) > 0
    raise ValueError(f"unknown mask {name!r}")


def rows_equal_outside_ties(shard, q, s, r, ref_r):
    """Rows r against ref_r [NQ, k] for scores s both searches agree on -> (equal?, proved).
    Slots whose score equals a neighbour's are exempt.  A run of equal scores can go on past k,
    where no neighbour shows it: a last slot that differs with no equal neighbour counts as equal
    only if neither row is among the other side's rows and the two rows, searched alone under a
    two-row mask (k = 2), score the same bit for bit, which is the slot's score; ``proved`` counts
    those slots."""
    rr, gg = r.long(), ref_r.long()
    fin = torch.isfinite(s)
    tie = torch.zeros_like(fin)
    tie[:, 1:] |= s[:, 1:] == s[:, :-1]
    tie[:, :-1] |= s[:, :-1] == s[:, 1:]
    diff = (rr != gg) & ~tie & fin
    if bool(diff[:, :-1].any()):
        return False, 0
    proved = 0
    for i in torch.nonzero(diff[:, -1]).flatten().tolist():
        a, b = int(rr[i, -1]), int(gg[i, -1])
        if a < 0 or b < 0 or b in rr[i].tolist() or a in gg[i].tolist():
            return False, proved
        s2, r2 = shard.search(q[i:i + 1], 2, allow=[a, b])
        if sorted(r2[0].tolist()) != sorted((a, b)):
            return False, proved
        if not float(s2[0, 0]) == float(s2[0, 1]) == float(s[i, -1]):
            return False, proved
        proved += 1
    return True, proved


def timed(fn, iters: int) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def run_groups(a, shard, q, emit, base) -> None:
    """The --groups run (module docstring)."""
    dev, n, k = shard.device, a.rows, a.k
    cls = type(shard)
    for ci, case in enumerate(a.group_cases.split(",")):
        for G in [int(x) for x in a.groups.split(",")]:
            masks, taken = [], None
            for g in range(G):
                seed = 1000 + 37 * ci + g
                if case[0] == "n":
                    allow = ~build_allow("d" + case[1:], n, dev, seed)
                else:
                    allow = build_allow(case, n, dev, seed)
                    if case[0] == "d":       # disjoint documents
                        if taken is None:
                            taken = allow.clone()
                        else:
                            allow &= ~taken
                            taken |= allow
                masks.append(shard.make_mask(allow))
                del allow
            del taken
            union = masks[0].words.clone()
            for m in masks[1:]:
                union |= m.words
            umask = shard.make_mask(union.view(torch.uint8))
            group_of = [i % G for i in range(a.nq)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mg = shard.make_mask_groups(masks, group_of)
            for c in range(mg.n_chunks):
                mg.chunk(c)
            torch.cuda.synchronize()
            groups_ms = (time.perf_counter() - t0) * 1e3

            def grouped(min_groups):
                shard.GROUP_SCAN_MIN_GROUPS = min_groups
                try:
                    return shard.search(q, k, allow=mg)
                finally:
                    shard.GROUP_SCAN_MIN_GROUPS = cls.GROUP_SCAN_MIN_GROUPS

            variants = {"grouped": lambda: grouped(2),
                        "group_loop": lambda: grouped(1 << 30),
                        "union_floor": lambda: shard.search(q, k, allow=umask),
                        "single_mask": lambda: shard.search(q, k, allow=masks[0])}
            res = {}
            for v, fn in variants.items():       # results first (also the warm-up)
                res[v] = fn()
                torch.cuda.synchronize()
            large_k_info = {}
            if k > 32:       # the grouped emitting route's record (each search overwrites it)
                shard._filter_large_k_last = None
                grouped(2)
                torch.cuda.synchronize()
                last = shard._filter_large_k_last
                if last is not None:
                    large_k_info = {"overflow": int(last[1]), "max_candidates": int(last[0].max()),
                                    "cap": int(shard.LARGE_K_CAP)}
            (gs, gr), (ls, lr) = res["grouped"], res["group_loop"]
            tie = torch.zeros_like(gs, dtype=torch.bool)
            tie[:, 1:] |= gs[:, 1:] == gs[:, :-1]
            tie[:, :-1] |= gs[:, :-1] == gs[:, 1:]
            same = bool(torch.equal(gs, ls) and ((gr == lr) | tie).all())
            proved = None
            if shard.dtype == "fp8" and torch.equal(gs, ls) and not same:
                same, proved = rows_equal_outside_ties(shard, q, gs, gr, lr)
            del res
            routes = ["loop" if shard._loop_keeps_chunk(mg.chunk(c), k) else
                      "emit" if k > 32 else "scan" for c in range(mg.n_chunks)]
            info = dict(base, case=case, groups=G, len_groups=len(mg), chunks=mg.n_chunks,
                        grouped_routes=routes,
                        union_live_tiles=int(umask.n_live),
                        live_tiles=[int(m.n_live) for m in masks],
                        groups_ms=round(groups_ms, 3), grouped_equals_loop=same, **large_k_info)
            if proved is not None:
                info["last_slot_ties_proved"] = proved
            times = {v: [] for v in variants}
            for _ in range(a.rounds):            # alternated: every variant once per round
                for v, fn in variants.items():
                    times[v].append(timed(fn, a.iters))
            for v, ts in times.items():
                emit(dict(info, variant=v, ms=round(statistics.median(ts), 3),
                          ms_min=round(min(ts), 3), ms_max=round(max(ts), 3)))
            del masks, umask, mg, union
            torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--masks", default="ones,u50,u10,u1,d10,d1,d0.1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--dtype", choices=("bf16", "fp8"), default="bf16")
    ap.add_argument("--fallback", action="store_true",
                    help="also time the chunked matmul under the mask (one iteration)")
    ap.add_argument("--groups", default="",
                    help="a mask per query: comma list of group counts (replaces the per-mask run)")
    ap.add_argument("--group-cases", default="n1,d1,d0.1,u50")
    ap.add_argument("--force-scan", action="store_true",
                    help="--groups: the grouped scan for every chunk, whatever the route rule")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filter_bench needs the GPU: nothing here is measured without one")
    from codename_symbiont_amd.index.shard import FP8_SCALE, TILE_ROWS, HbmIndexShard

    dev = torch.device("cuda")
    n, k = a.rows, a.k
    kmax = 16 if k <= 16 else 32
    fp8 = a.dtype == "fp8"
    shard = HbmIndexShard(a.dim, n, device=dev, dtype=a.dtype)
    shard.fill_random(n, seed=1)
    g = torch.Generator(device=dev).manual_seed(77)      # held out: not rows of the shard
    q = torch.nn.functional.normalize(torch.randn(a.nq, a.dim, device=dev, generator=g),
                                      dim=-1).bfloat16()
    q8 = None
    if fp8:
        from codename_symbiont_amd.ops.kernels import quant_fp8

        q8 = quant_fp8(q, scale=FP8_SCALE)
    row_bytes = a.dim * (1 if fp8 else 2)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    base = {"bench": "filter_bench", "rows": n, "dim": a.dim, "nq": a.nq, "k": k,
            "rounds": a.rounds, "iters": a.iters}
    if fp8:
        base["dtype"] = "fp8"
    if a.groups:
        if k > 32 and not (fp8 and k <= shard.K_MAX_HIP):
            raise SystemExit("--groups at k > 32 measures the grouped emitting scan of an fp8 "
                             f"shard: --dtype fp8, k <= {shard.K_MAX_HIP}")
        if k > 32 and not shard._group_large_k_serves(k, [None, None]):
            raise SystemExit("--groups at k > 32: this shard is below FP8_LARGE_K_MIN_ROWS rows "
                             "or of a width the emitting scan is not built for (the per-mask "
                             "loop would answer both variants)")
        if a.force_scan:
            shard.GROUP_LOOP_MIN_TILES = 1 << 62
        run_groups(a, shard, q, emit, dict(base, bench="filter_bench_groups"))
        return
    for mi, name in enumerate(a.masks.split(",")):
        allow = build_allow(name, n, dev, 100 + mi)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mask = shard.make_mask(allow)
        torch.cuda.synchronize()
        mask_ms = (time.perf_counter() - t0) * 1e3
        n_allowed, n_live = int(allow.sum()), int(mask.n_live)
        info = dict(base, mask=name, allowed=n_allowed, allowed_share=round(n_allowed / n, 5),
                    live_tiles=n_live, live_share=round(n_live / ((n + 63) // 64), 5),
                    mask_ms=round(mask_ms, 3))
        idx = torch.nonzero(allow).flatten()
        del allow
        m = idx.numel()
        m_pad = (m + TILE_ROWS - 1) // TILE_ROWS * TILE_ROWS
        free, _ = torch.cuda.mem_get_info(dev)
        large_k = k > 32                   # no list scan at this k: filtered / search only
        gather_ok = not large_k and m > 0 and m_pad * row_bytes < free - (8 << 30)
        sub = (torch.zeros(m_pad, a.dim, dtype=shard.rows.dtype, device=dev) if gather_ok
               else None)

        def filtered(seed):
            shard.filter_seed = seed
            return shard.search(q, k, allow=mask)

        def gather():
            torch.index_select(shard.rows, 0, idx, out=sub[:m])
            if fp8:
                s, r = shard._scan(m, q8, kmax, k, None, None, rows=sub, dtype="fp8")
                s = s * (1.0 / (FP8_SCALE * FP8_SCALE))
            else:
                s, r = shard._scan(m, q, kmax, k, None, None, rows=sub)
            return s, idx[r.long().clamp_min(0)]

        variants = {"filtered_seed": lambda: filtered(True),
                    "filtered_noseed": lambda: filtered(False),
                    "search": lambda: shard.search(q, k),
                    "plain_scan": lambda: shard._scan(n, q8 if fp8 else q, kmax, k, None, None)}
        if gather_ok:
            variants["gather_scan"] = gather
        if large_k:
            variants = {"filtered": lambda: shard.search(q, k, allow=mask),
                        "search": lambda: shard.search(q, k),
                        "search_k32": lambda: shard.search(q, 32)}
        # results first (also the warm-up of every shape): seed on == seed off == gather
        res, same_seed, per_variant = {}, None, {}
        for v, fn in variants.items():
            # (an fp8 shard's unfiltered search at this k is the same route under an all-ones
            # mask and leaves its own counts: read them per variant)
            shard._filter_large_k_last = None
            res[v] = fn()
            torch.cuda.synchronize()
            last = shard._filter_large_k_last
            if large_k and last is not None:
                per_variant[v] = {"overflow": int(last[1]), "max_candidates": int(last[0].max()),
                                  "cap": int(shard.LARGE_K_CAP)}
        if not large_k:
            same_seed = bool(torch.equal(res["filtered_seed"][0], res["filtered_noseed"][0])
                             and torch.equal(res["filtered_seed"][1], res["filtered_noseed"][1]))
        same_gather = None
        if gather_ok:
            same_gather = bool(torch.equal(res["filtered_seed"][0], res["gather_scan"][0]))
        extra = {}
        if fp8 and gather_ok:
            (fs, fr), (gs, gr) = res["filtered_seed"], res["gather_scan"]
            fin = torch.isfinite(gs)
            err = torch.where(fin, (fs - gs).abs(), torch.zeros_like(gs))
            same_rows, proved = rows_equal_outside_ties(shard, q, gs, fr, gr)
            extra = {"max_abs_vs_gather": float(err.max()), "rows_equal_gather": same_rows,
                     "last_slot_ties_proved": proved}
        del res
        times = {v: [] for v in variants}
        for _ in range(a.rounds):            # alternated: every variant once per round
            for v, fn in variants.items():
                times[v].append(timed(fn, a.iters))
        for v, ts in times.items():
            emit(dict(info, variant=v, ms=round(statistics.median(ts), 3),
                      ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
                      seed_on_equals_off=same_seed, scores_equal_gather=same_gather, **extra,
                      **per_variant.get(v, {})))
        if a.fallback:
            ms = timed(lambda: shard._search_matmul(q, k, mask=mask), 1)
            emit(dict(info, variant="matmul_mask", ms=round(ms, 3), ms_min=round(ms, 3),
                      ms_max=round(ms, 3), iters=1, rounds=1))
        del sub, idx, mask
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
