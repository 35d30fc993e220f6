"""In-place compaction of deleted rows, on the CPU: the plan (index.shard.compact_plan) simulated
over every delete pattern with the direct windows' rows moved in random order, CPU shards
(HbmIndexShard.compact runs the same plan with torch indexing), and the store with its snapshots
and log."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from codename_symbiont_amd.index import persist
from codename_symbiont_amd.index.filter import Filter
from codename_symbiont_amd.index.shard import (HbmIndexShard, Payload, compact_new_rows,
                                               compact_plan)
from codename_symbiont_amd.index.store import VectorStore

N = 64 * 37 + 19
STAGE_TILES = 2
PATTERNS = ("none", "first", "last", "all", "every_other", "third_tiles", "run", "uniform_1",
            "uniform_50", "lead_uniform_5")


def pattern(name: str, n: int = N) -> np.ndarray:
    """bool [n]: the rows a delete pattern kills."""
    dead = np.zeros(n, dtype=bool)
    rng = np.random.default_rng(PATTERNS.index(name))
    if name == "first":
        dead[0] = True
    elif name == "last":
        dead[n - 1] = True
    elif name == "all":
        dead[:] = True
    elif name == "every_other":
        dead[::2] = True
    elif name == "third_tiles":
        for t in range(0, (n + 63) // 64, 3):
            dead[t * 64:(t + 1) * 64] = True
    elif name == "run":
        dead[100:300] = True
    elif name == "uniform_1":
        dead[rng.choice(n, n // 100, replace=False)] = True
    elif name == "uniform_50":
        dead[rng.random(n) < 0.5] = True
    elif name == "lead_uniform_5":
        dead[:640] = True
        dead[rng.random(n) < 0.05] = True
    return dead


def packed(dead: np.ndarray) -> np.ndarray:
    """The shard's host bitmap of a bool pattern: whole 64-row tiles, bit r % 8 of byte r // 8."""
    pad = np.zeros((dead.size + 63) // 64 * 64, dtype=bool)
    pad[:dead.size] = dead
    return np.packbits(pad, bitorder="little")


def run_plan(x: np.ndarray, dead: np.ndarray, c, windows, rng) -> None:
    """Execute a plan on the host array ``x`` [count, ...]: a direct window's rows move one at a
    time in a random order (the workgroups of one launch), a staged window gathers then copies."""
    count = dead.size
    for t0, t1, mode in windows:
        s0, s1 = 64 * t0, min(64 * t1, count)
        src = s0 + np.flatnonzero(~dead[s0:s1])
        dst = int(c[t0]) + np.arange(src.size)
        assert dst.size == int(c[t1] - c[t0])
        if mode == "direct":
            for i in rng.permutation(src.size):
                x[dst[i]] = x[src[i]]
        else:
            stage = x[src].copy()
            x[dst[0]:dst[0] + dst.size] = stage


# ---------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("name", PATTERNS)
def test_plan_properties(name):
    dead = pattern(name)
    n_tiles = (N + 63) // 64
    c, windows = compact_plan(packed(dead), N, 64 * STAGE_TILES)
    live_idx = np.flatnonzero(~dead)
    # c: the exclusive prefix of the live rows per tile
    per_tile = np.add.reduceat((~dead).astype(np.int64), np.arange(0, N, 64))
    assert c.shape == (n_tiles + 1,) and c[0] == 0
    assert np.array_equal(np.diff(c), per_tile) and c[-1] == live_idx.size
    if name == "none":
        assert windows == []
        return
    first_tile = int(np.flatnonzero(dead)[0]) // 64
    # the windows tile [first, n_tiles)
    assert windows[0][0] == first_tile and windows[-1][1] == n_tiles
    for (a0, a1, _), (b0, _, _) in zip(windows, windows[1:]):
        assert a0 < a1 == b0
    assert all(t0 < t1 for t0, t1, _ in windows)
    for t0, t1, mode in windows:
        assert mode in ("direct", "staged")
        s0, s1 = 64 * t0, min(64 * t1, N)
        src = s0 + np.flatnonzero(~dead[s0:s1])
        dst = np.arange(int(c[t0]), int(c[t1]))
        if mode == "direct":
            assert c[t1] <= 64 * t0
            assert t1 - t0 >= STAGE_TILES
            assert not set(src.tolist()) & set(dst.tolist())
        else:
            assert t1 - t0 <= STAGE_TILES and c[t1] - c[t0] <= 64 * STAGE_TILES
    # executing it, direct windows in random order, leaves live_idx in [0, live)
    x = np.arange(N)
    run_plan(x, dead, c, windows, np.random.default_rng(5))
    assert np.array_equal(x[:live_idx.size], live_idx)
    modes = [m for _, _, m in windows]
    if name == "lead_uniform_5":
        assert "direct" in modes
    if name == "uniform_1":
        assert "staged" in modes
    # the row renumbering the payload store gets
    assert np.array_equal(compact_new_rows(packed(dead), c, live_idx), np.arange(live_idx.size))


def test_plan_ignores_bits_past_count_and_short_bitmaps():
    dead = pattern("uniform_50")
    h = packed(dead).copy()
    want_c, want_w = compact_plan(h, N, 128)
    h[N // 8] |= 0xFF & ~((1 << (N % 8)) - 1)              # bits at or past count
    h[N // 8 + 1:] = 0xFF
    c, w = compact_plan(h, N, 128)
    assert np.array_equal(c, want_c) and w == want_w
    # a bitmap shorter than the rows: the missing bytes are live rows
    c, w = compact_plan(packed(dead)[:40], N, 128)
    cut = dead.copy()
    cut[320:] = False
    want_c, want_w = compact_plan(packed(cut), N, 128)
    assert np.array_equal(c, want_c) and w == want_w
    c, w = compact_plan(None, 0, 128)
    assert c.tolist() == [0] and w == []


# ---------------------------------------------------------------------------- CPU shards
def _queries(nq, dim, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(nq, dim, generator=g), dim=-1).bfloat16()


def _pl(i):
    return Payload(f"doc-{i % 7}", "u", f"s{i}", i, "m", 0)


def _same_outside_ties(a, b, tol=1e-6):
    """Two lists of per-query [(score, point id)]: equal scores, equal ids outside tied scores."""
    for qa, qb in zip(a, b):
        assert len(qa) == len(qb)
        sa = np.array([s for s, _ in qa])
        sb = np.array([s for s, _ in qb])
        assert np.allclose(sa, sb, atol=tol, rtol=0)
        for j, ((_, pa), (_, pb)) in enumerate(zip(qa, qb)):
            tied = any(abs(sa[j] - sa[i]) <= tol for i in (j - 1, j + 1) if 0 <= i < len(sa))
            assert pa == pb or tied


def _by_point(sh, s, r):
    return [[(float(a), sh.payloads.get(int(b))[0]) for a, b in zip(qs, qr) if b >= 0]
            for qs, qr in zip(s.tolist(), r.tolist())]


@pytest.mark.parametrize("dtype,dim,prune", [("bf16", 64, None), ("fp8", 256, None),
                                             ("bf16", 384, "i8")])
@pytest.mark.parametrize("name", ["lead_uniform_5", "run", "uniform_1", "every_other"])
def test_cpu_shard_compact(dtype, dim, prune, name):
    n = 64 * 9 + 19
    sh = HbmIndexShard(dim, n, device="cpu", dtype=dtype, prune=prune)
    g = torch.Generator().manual_seed(4)
    sh.upsert([f"p{i}" for i in range(n)], torch.randn(n, dim, generator=g),
              [_pl(i) for i in range(n)])
    if name == "lead_uniform_5":                           # (the leading run, at this size: 130)
        dead = np.random.default_rng(8).random(n) < 0.05
        dead[:130] = True
    else:
        dead = pattern(name, n)
    live_idx = np.flatnonzero(~dead)
    live = live_idx.size
    q = _queries(5, dim)
    with pytest.raises(MemoryError):
        sh.upsert(["new"], torch.randn(1, dim, generator=g), [_pl(0)])
    assert sh.compact() == 0 and sh.compact_gen == 0 and sh.last_compact is None   # no dead row
    gen0 = sh.dead_gen
    assert sh.compact() == 0 and sh.dead_gen == gen0
    sh.delete_rows(np.flatnonzero(dead))
    with pytest.raises(MemoryError):                       # dead rows free nothing by themselves
        sh.upsert(["new"], torch.randn(1, dim, generator=g), [_pl(0)])
    old_rows = sh.rows[:n].clone()
    old_mask = sh.make_mask(list(range(0, live_idx[-1] + 1, 3)))
    want = {k: _by_point(sh, *sh.search(q, k)) for k in (5, 40)}
    ids_before = {pid: r for r, pid in sh.payloads.point_ids.items()}
    bounds = None if not prune else (sh.i8_bounds.clone(), sh.mx4_bounds.clone())
    gen = sh.dead_gen
    # a stage of one tile's worth of rows, so that several windows (of both modes) run
    assert sh.compact(stage_bytes=64 * dim * sh.rows.element_size()) == n - live
    assert sh.count == sh.visible == sh.live_count == live and sh.n_dead == 0
    assert len(sh.payloads) == live
    assert sh.dead_gen == gen + 1 and sh.compact_gen == 1
    lc = sh.last_compact
    assert lc["reclaimed"] == n - live and lc["first_row"] == int(np.flatnonzero(dead)[0])
    assert lc["rows_moved"] == live - lc["first_row"]
    assert lc["direct_windows"] + lc["staged_windows"] >= 1
    if name == "lead_uniform_5":
        assert lc["direct_windows"] >= 1
    if name == "run":                                      # staged up to the run, direct past it
        assert lc["direct_windows"] >= 1 and lc["staged_windows"] >= 1
    assert torch.equal(sh.rows[:live].view(torch.uint8),
                       old_rows[torch.from_numpy(live_idx)].view(torch.uint8))
    assert not sh.rows[live:].view(torch.uint8).any()
    assert not sh.dead.any() and not sh._dead_host.any()
    assert sh._persisted == 0 and sh._dirty == set() and sh._persist_key is None
    # ids and payloads follow their rows
    ps = sh.payloads
    assert len(ps.point_ids) == len(ps.fields) == len(ps.id_to_row) == live
    for new, old in enumerate(live_idx.tolist()):
        assert ps.get(new) == (f"p{old}", _pl(old))
        assert ps.id_to_row[f"p{old}"] == new and ids_before[f"p{old}"] == old
    # a filter by document finds the moved rows
    hit = Filter(must={"original_document_id": "doc-3"}).evaluate(ps, sh.visible)
    hit = np.flatnonzero(hit) if hit.dtype == np.bool_ else np.sort(hit)
    assert hit.tolist() == [new for new, old in enumerate(live_idx.tolist()) if old % 7 == 3]
    with pytest.raises(ValueError, match="RowMask made before"):
        sh.search(q, 5, allow=old_mask)
    # the same (score, point id) pairs as the tombstoned search just before
    for k in (5, 40):
        _same_outside_ties(_by_point(sh, *sh.search(q, k)), want[k])
    assert sh.last_dead_hits is None
    if prune:
        # re-imaged up to the old count: a second imaging of the rows changes no byte
        imgs = [t.clone() for t in (sh.img_i8, sh.img_mx4, sh.rows_i8, sh.rows_mx4)
                if t is not None]
        sh._image_rows(0, sh.count)
        now = [t for t in (sh.img_i8, sh.img_mx4, sh.rows_i8, sh.rows_mx4) if t is not None]
        assert imgs and all(torch.equal(a, b) for a, b in zip(imgs, now))
        # ... and the images past the live rows are those of zero rows
        fresh = HbmIndexShard(dim, n, device="cpu", prune=prune)
        fresh._reserve(n)
        fresh.rows[:live] = sh.rows[:live]
        fresh._image_rows(0, n)
        for a, b in ((sh.img_i8, fresh.img_i8), (sh.img_mx4, fresh.img_mx4)):
            assert (a is None) == (b is None)
            assert a is None or torch.equal(a, b)
        assert bool((sh.i8_bounds >= bounds[0]).all()) and bool((sh.mx4_bounds >= bounds[1]).all())
    # the capacity is back
    m = n - live
    sh.upsert([f"n{i}" for i in range(m)], torch.randn(m, dim, generator=g),
              [_pl(i) for i in range(m)])
    assert sh.count == n and sh.payloads.id_to_row["n0"] == live
    with pytest.raises(MemoryError):
        sh.upsert(["more"], torch.randn(1, dim, generator=g), [_pl(0)])


def test_cpu_shard_compact_all_rows_dead():
    sh = HbmIndexShard(32, 200, device="cpu")
    sh.fill_random(150, seed=1)
    sh.delete_rows(range(150))
    assert sh.compact() == 150 and sh.count == 0 and sh.visible == 0
    assert not sh.rows.view(torch.uint8).any()
    sh.fill_random(200, seed=2)
    s, r = sh.search(_queries(2, 32), 3)
    assert torch.isfinite(s).all()


# ---------------------------------------------------------------------------- the store
SD = 16


def _vec(i):
    return np.random.default_rng(1000 + i).standard_normal(SD).astype(np.float32)


def _store(d, n_points=40):
    st = VectorStore(SD, 64, device="cpu", snapshot_dir=d, snapshot_every=10 ** 9)
    if st.count == 0 and n_points:
        st.upsert([f"p{i}" for i in range(n_points)], np.stack([_vec(i) for i in range(n_points)]),
                  [_pl(i) for i in range(n_points)])
    return st


def _points(st):
    """point id -> (payload, row bytes): the store's content whatever its row numbering."""
    sh = st.shard
    return {pid: (sh.payloads.get(r)[1], sh.rows[r].view(torch.uint8).tolist())
            for r, pid in sh.payloads.point_ids.items()}


def _answers(st, k=6):
    q = np.stack([_vec(900 + i) for i in range(4)])
    s, r = st.search(q, k)
    return [[(float(a), st.lookup(int(b))[0]) for a, b in zip(qs, qr) if b >= 0]
            for qs, qr in zip(s, r)]


def test_store_compact_snapshot_and_reopen(tmp_path):
    d = str(tmp_path / "idx")
    st = _store(d)
    st.snapshot()
    assert st.compact() == 0 and st.compact_gen == 0          # nothing deleted: nothing changes
    assert st.delete(filter=Filter(must={"original_document_id": "doc-2"})) == 6
    assert st.delete(point_ids=["p0", "p39"]) == 2
    st.snapshot()
    assert persist.committed_manifest(d)["dead"]["n"] == 8
    f3 = Filter(must={"original_document_id": "doc-3"})
    st.search(np.stack([_vec(900)]), 3, filter=f3)             # a cached mask of the old rows
    st.result_fragments(5)
    want, pts = _answers(st), _points(st)
    gen = persist.committed_manifest(d)["gen"]
    assert st.compact(snapshot=True) == 8
    assert st.compact_gen == 1 and st.count == st.live_count == 32
    assert not st._frag and not st._masks
    man = persist.committed_manifest(d)
    assert man["gen"] > gen and "dead" not in man and man["count"] == 32
    assert len(man["segments"]) == 1 and man["segments"][0]["row0"] == 0 and not man["patches"]
    assert not [f for f in os.listdir(d) if f.startswith("dead.")]
    _same_outside_ties(_answers(st), want)
    s, r = st.search(np.stack([_vec(900)]), 3, filter=f3)      # a new mask, the moved rows
    assert all(st.lookup(int(g))[1].original_document_id == "doc-3" for g in r[0])
    st.wal.close()
    st2 = _store(d, 0)
    assert st2.count == st2.live_count == 32 and st2.shard.n_dead == 0 and st2.shard.dead is None
    assert _points(st2) == pts
    _same_outside_ties(_answers(st2), want)
    # 8 rows came back: 32 more points fit a store of 64, the 33rd does not
    st2.upsert([f"z{i}" for i in range(32)], np.stack([_vec(300 + i) for i in range(32)]),
               [_pl(i) for i in range(32)])
    with pytest.raises(MemoryError):
        st2.upsert(["z99"], _vec(399)[None], [_pl(0)])
    st2.wal.close()


def test_store_compact_without_snapshot_then_crash(tmp_path):
    d = str(tmp_path / "idx")
    st = _store(d)
    st.snapshot()
    st.delete(point_ids=[f"p{i}" for i in range(3, 30, 4)])
    gen = persist.committed_manifest(d)["gen"]
    n = st.compact(snapshot=False)
    assert n == 7 and st.count == 33
    assert persist.committed_manifest(d)["gen"] == gen         # no snapshot was written
    st.upsert(["p3", "w0", "w1"], np.stack([_vec(403), _vec(500), _vec(501)]),
              [_pl(3), _pl(50), _pl(51)])
    assert st.delete(point_ids=["p1", "w0"]) == 2
    want, pts = _answers(st), _points(st)
    assert st.count == 36 and st.live_count == 34
    st.wal.close()                                             # crash: no close(), no snapshot
    st2 = _store(d, 0)
    # the same points, merely uncompacted (the log is by point id)
    assert st2.live_count == 34 and st2.count > 36
    assert _points(st2) == pts
    _same_outside_ties(_answers(st2), want)
    # the next snapshot of the compacted store would have been a full one
    assert st.shard._persist_key is None
    st2.wal.close()


def test_store_snapshot_after_compact_is_full(tmp_path):
    d = str(tmp_path / "idx")
    st = _store(d)
    st.snapshot()
    st.delete(point_ids=["p5", "p6"])
    st.compact(snapshot=False)
    st.upsert(["v0"], _vec(700)[None], [_pl(70)])
    want, pts = _answers(st), _points(st)
    st.close()                                                 # cuts a snapshot: a full one
    man = persist.committed_manifest(d)
    assert "dead" not in man and man["count"] == 39 and man["segments"][0]["row0"] == 0
    st2 = _store(d, 0)
    assert st2.count == 39 and _points(st2) == pts
    _same_outside_ties(_answers(st2), want)
    st2.wal.close()


def test_group_store_refuses_compact():
    class Group:
        def __init__(self):
            self.shard = HbmIndexShard(SD, 64, device="cpu")
            self.shard.fill_random(8, seed=1)
            self.count = 8

    st = VectorStore(SD, 64, device="cpu", group=Group())
    with pytest.raises(ValueError, match="single-shard"):
        st.compact()
