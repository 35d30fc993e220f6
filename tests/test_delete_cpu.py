"""Point deletion on CPU shards and stores: tombstoned rows are zeroed and never returned, ids and
payloads go, masks made before a delete are refused, and the WAL / snapshot round trips restore
the same state (ids, rows, dead bits, search results)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

from codename_symbiont_amd.index import persist
from codename_symbiont_amd.index.filter import Filter
from codename_symbiont_amd.index.persist import Wal
from codename_symbiont_amd.index.shard import HbmIndexShard, Payload
from codename_symbiont_amd.index.store import VectorStore
from codename_symbiont_amd.ops import reference as R

N, K = 3000, 5


def _queries(nq, dim, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(nq, dim, generator=g), dim=-1).bfloat16()


def _dead_bool(sh):
    return torch.from_numpy(np.unpackbits(sh._dead_host, bitorder="little")[:sh.count].astype(bool))


# ---------------------------------------------------------------------------- shard
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_delete_rows_search_equals_reference_over_live_rows(dtype):
    dim = 32 if dtype == "bf16" else 256
    sh = HbmIndexShard(dim, N + 100, device="cpu", dtype=dtype)
    sh.fill_random(N, seed=3)
    q = _queries(7, dim)
    before = sh.unit_rows().clone()
    raw_before = sh.rows[:N].clone()
    # each query's current top 3, a whole 64-row tile, the first and the last row
    _, top = sh.search(q, 3)
    gone = sorted(set(top.flatten().tolist()) | set(range(128, 192)) | {0, N - 1})
    assert sh.live_count == N and sh.n_dead == 0 and sh.dead is None
    assert sh.delete_rows(gone + gone[:4]) == len(gone)            # duplicates count once
    assert sh.n_dead == len(gone) and sh.live_count == N - len(gone) and sh.count == N
    assert sh.dead.dtype == torch.uint8 and sh.dead.numel() == sh.rows.shape[0] // 8
    live = torch.ones(N, dtype=torch.bool)
    live[gone] = False
    assert torch.equal(_dead_bool(sh), ~live)
    assert torch.equal(torch.from_numpy(sh._dead_host), sh.dead)
    # live rows bit-identical, dead rows all zero
    raw = sh.rows[:N]
    assert torch.equal(raw[live].view(torch.uint8), raw_before[live].view(torch.uint8))
    assert not raw[~live].view(torch.uint8).any()
    ref_s, ref_i = R.filtered_topk_ref(before, q, K, live)
    s, r = sh.search(q, K)
    assert torch.equal(r.long(), ref_i)
    torch.testing.assert_close(s, ref_s, atol=1e-6, rtol=0)
    assert r.dtype == torch.int32 and s.dtype == torch.float32
    s2, r2 = sh.search_end(sh.search_begin(q, K))
    assert torch.equal(s, s2) and torch.equal(r, r2)
    # deleting twice deletes nothing and changes no generation; a bad row raises
    gen = sh.dead_gen
    assert sh.delete_rows(gone) == 0 and sh.dead_gen == gen and sh.n_dead == len(gone)
    for bad in ([N], [-1], [5, N + 3]):
        with pytest.raises(IndexError):
            sh.delete_rows(bad)
    assert sh.n_dead == len(gone)


def test_k_above_live_count_gives_inf_tail():
    sh = HbmIndexShard(32, 64, device="cpu")
    sh.fill_random(20, seed=1)
    before = sh.unit_rows().clone()
    q = _queries(3, 32)
    assert sh.delete_rows(range(3, 20)) == 17
    s, r = sh.search(q, K)
    live = torch.zeros(20, dtype=torch.bool)
    live[:3] = True
    ref_s, ref_i = R.filtered_topk_ref(before, q, K, live)
    assert torch.equal(r.long(), ref_i)
    assert torch.isfinite(s[:, :3]).all() and (s[:, 3:] == -float("inf")).all()
    assert (r[:, 3:] == -1).all()
    assert sh.delete_rows([0, 1, 2]) == 3 and sh.live_count == 0
    s, r = sh.search(q, K)
    assert (s == -float("inf")).all() and (r == -1).all()


def test_pruned_cpu_shard_reimages_dead_rows():
    """A CPU shard that keeps pruning images: the images of a deleted row are those of a zero row
    (re-imaged through _image_rows), and the bounds never shrink."""
    sh = HbmIndexShard(384, 256, device="cpu", prune="i8")
    sh.fill_random(200, seed=2)
    b_i8, b_mx4 = sh.i8_bounds.clone(), sh.mx4_bounds.clone()
    fresh = HbmIndexShard(384, 256, device="cpu", prune="i8")
    fresh.fill_random(200, seed=2)
    gone = list(range(32, 64)) + [5, 199]
    sh.delete_rows(gone)
    fresh.rows[gone] = 0
    fresh._image_rows(0, 200)
    for name in ("img_i8", "img_mx4"):
        a, b = getattr(sh, name), getattr(fresh, name)
        assert (a is None) == (b is None)
        if a is not None:
            g0, g1 = 1, 2      # the sub-tile made of dead rows only: the image of zero rows
            assert torch.equal(a[g0:g1], b[g0:g1])
    assert bool((sh.i8_bounds >= b_i8).all()) and bool((sh.mx4_bounds >= b_mx4).all())


# ---------------------------------------------------------------------------- ids and payloads
SD = 16


def _vec(i):
    return np.random.default_rng(1000 + i).standard_normal(SD).astype(np.float32)


def _pl(i):
    return Payload(f"doc-{i % 3}", "u", f"s{i}", i, "m", 0)


def _store(n_points=30, d="", **kw):
    st = VectorStore(SD, 256, device="cpu", snapshot_dir=d, **kw)
    if st.count == 0 and n_points:
        st.upsert([f"p{i}" for i in range(n_points)], np.stack([_vec(i) for i in range(n_points)]),
                  [_pl(i) for i in range(n_points)])
    return st


def test_delete_points_ids_and_reupsert():
    st = _store()
    sh = st.shard
    assert sh.delete_points(["p3", "nope", "p7"]) == 2
    assert st.delete(point_ids=["p3", "ghost"]) == 0          # unknown and already deleted
    assert "p3" not in sh.payloads.id_to_row and st.lookup(3) == (None, Payload())
    assert st.count == 30 and st.live_count == 28
    # the deleted id again: a new row, the old one stays dead
    st.upsert(["p3"], _vec(3)[None], [_pl(3)])
    assert sh.payloads.id_to_row["p3"] == 30 and st.count == 31 and st.live_count == 29
    assert not sh.rows[3].view(torch.uint8).any() and st.lookup(3) == (None, Payload())
    s, r = st.search(_vec(3)[None], 3)
    assert r[0, 0] == 30 and 3 not in r[0] and 7 not in r[0]
    with pytest.raises(ValueError):
        st.delete()
    with pytest.raises(ValueError):
        st.delete(point_ids=["p1"], filter=Filter(point_ids=["p1"]))


def test_masks_and_delete_by_filter():
    st = _store()
    sh = st.shard
    q = torch.nn.functional.normalize(torch.from_numpy(np.stack([_vec(900), _vec(901)])), dim=-1)
    old = sh.make_mask(torch.ones(30, dtype=torch.bool))
    sh.search(q.bfloat16(), 3, allow=old)
    f_not = Filter(must_not={"original_document_id": "doc-1"})
    st.search(q.numpy(), 64, filter=f_not)                      # cached before the delete
    assert len(st._masks) == 1
    # delete by filter removes exactly the document's rows
    doc0 = {i for i in range(30) if i % 3 == 0}
    assert st.delete(filter=Filter(must={"original_document_id": "doc-0"})) == len(doc0)
    assert len(st._masks) == 0
    assert set(np.flatnonzero(_dead_bool(sh).numpy()).tolist()) == doc0
    assert st.delete(filter=Filter(must={"original_document_id": "doc-0"})) == 0
    # a RowMask from before the delete is refused; one made after it excludes the dead rows
    with pytest.raises(ValueError, match="delete"):
        sh.search(q.bfloat16(), 3, allow=old)
    new = sh.make_mask(torch.ones(30, dtype=torch.bool))
    assert new.dead_gen == sh.dead_gen and new.count() == 20
    assert not new.bool_rows(0, 30)[sorted(doc0)].any()
    # a store search under must_not never returns a dead row
    s, r = st.search(q.numpy(), 64, filter=f_not)
    want = {i for i in range(30) if i % 3 == 2}
    for i in range(2):
        assert set(r[i][np.isfinite(s[i])].tolist()) == want
    s, r = st.search(q.numpy(), 64)
    for i in range(2):
        assert set(r[i][np.isfinite(s[i])].tolist()) == set(range(30)) - doc0
    # rows without a point id pass a must_not filter but are skipped by a delete
    sh.append_f32(torch.from_numpy(np.stack([_vec(500), _vec(501)])))
    assert st.delete(filter=Filter(must_not={"original_document_id": ["doc-0", "doc-1"]})) == 10
    assert sh.n_dead == 20 and st.live_count == 12


def test_truncate_clears_dead_bits_above():
    sh = HbmIndexShard(SD, 256, device="cpu")
    sh.fill_random(100, seed=1)
    sh.delete_rows([5, 63, 64, 70, 99])
    gen = sh.dead_gen
    sh.truncate(70)
    assert sh.n_dead == 3 and sh.dead_gen > gen and sh.live_count == 67
    assert np.flatnonzero(_dead_bool(sh).numpy()).tolist() == [5, 63, 64]
    assert torch.equal(torch.from_numpy(sh._dead_host), sh.dead)
    sh.append_f32(torch.from_numpy(np.stack([_vec(i) for i in range(10)])))   # slots 70..79 anew
    s, r = sh.search(torch.nn.functional.normalize(torch.from_numpy(_vec(0)[None]), dim=-1), 1)
    assert r[0, 0] == 70


def test_group_store_refuses_delete():
    class Group:
        def __init__(self):
            self.shard = HbmIndexShard(SD, 64, device="cpu")
            self.shard.fill_random(8, seed=1)
            self.count = 8

    st = VectorStore(SD, 64, device="cpu", group=Group())
    with pytest.raises(ValueError, match="single-shard"):
        st.delete(point_ids=["p0"])
    with pytest.raises(ValueError, match="single-shard"):
        st.delete(filter=Filter(must={"model_name": "m"}))


# ---------------------------------------------------------------------------- WAL and snapshots
def _state(st):
    sh = st.shard
    q = np.stack([_vec(900 + i) for i in range(4)])
    dead = np.zeros(sh.count, bool) if sh._dead_host is None else _dead_bool(sh).numpy()
    return dict(count=sh.count, n_dead=sh.n_dead, dead=dead.tolist(),
                ids=dict(sh.payloads.point_ids), fields=dict(sh.payloads.fields),
                id_to_row=dict(sh.payloads.id_to_row),
                rows=sh.rows[:sh.count].view(torch.int16).clone(),
                search=[a.tolist() for a in st.search(q, 6)])


def _same(a, b):
    for key in a:
        if key == "rows":
            assert torch.equal(a[key], b[key])
        else:
            assert a[key] == b[key], key


def _mutate(st):
    """upsert / delete / upsert of the same id / delete of another, then a delete by filter."""
    st.upsert(["x0", "x1", "x2"], np.stack([_vec(100 + i) for i in range(3)]),
              [_pl(i) for i in range(3)])
    assert st.delete(point_ids=["x1", "p2", "unknown"]) == 2
    st.upsert(["x1", "p4"], np.stack([_vec(201), _vec(204)]), [_pl(1), _pl(4)])
    assert st.delete(point_ids=["x0"]) == 1
    flt = Filter(must={"original_document_id": "doc-0"}, point_ids=["p6", "p9", "p7"])
    assert st.delete(filter=flt) == 2


def test_wal_replays_deletes_in_order(tmp_path):
    d = str(tmp_path / "idx")
    st = _store(d=d, snapshot_every=10 ** 9)
    _mutate(st)
    want = _state(st)
    st.wal.close()                                         # crash: the WAL is all there is
    path = os.path.join(d, "wal.log")
    kinds = [op[0] for op in Wal.replay_ops(path, SD)]
    assert kinds == ["upsert", "upsert", "delete", "upsert", "delete", "delete"]
    ups = list(Wal.replay(path, SD))                       # the upserts only, same signature
    assert len(ups) == 3 and all(len(u) == 3 for u in ups)
    size = os.path.getsize(path)
    assert Wal.repair(path) == size                        # repair keeps the delete records
    st2 = VectorStore(SD, 256, device="cpu", snapshot_dir=d, snapshot_every=10 ** 9)
    _same(want, _state(st2))
    st2.wal.close()
    # a torn delete record at the tail is dropped
    with open(path, "rb") as f:
        data = f.read()
    w = Wal(path, SD)
    w.append_delete(["p11", "p12"])
    w.close()
    with open(path, "rb") as f:
        full = f.read()
    assert len(full) > len(data)
    with open(path, "wb") as f:
        f.write(full[:-3])
    assert [op[0] for op in Wal.replay_ops(path, SD)] == kinds
    assert Wal.repair(path) == len(data)
    st3 = VectorStore(SD, 256, device="cpu", snapshot_dir=d, snapshot_every=10 ** 9)
    _same(want, _state(st3))
    st3.wal.close()


def _dead_files(d):
    return sorted(f for f in os.listdir(d) if f.startswith("dead."))


def test_snapshot_incremental_with_deletes_reloads(tmp_path):
    d = str(tmp_path / "idx")
    st = _store(d=d, snapshot_every=10 ** 9)
    st.snapshot()                                          # gen 1: no tombstones yet
    assert _dead_files(d) == [] and "dead" not in persist.committed_manifest(d)
    _mutate(st)
    st.snapshot()                                          # gen 2: incremental, with the bitmap
    man = persist.committed_manifest(d)
    assert man["dead"] == {"gen": 2, "n": st.shard.n_dead} and _dead_files(d) == ["dead.2.bin"]
    with open(os.path.join(d, "dead.2.bin"), "rb") as f:
        bits = np.unpackbits(np.frombuffer(f.read(), np.uint8), bitorder="little")
    assert bits[:st.count].astype(bool).tolist() == _state(st)["dead"]
    want = _state(st)
    st.wal.close()
    st2 = VectorStore(SD, 256, device="cpu", snapshot_dir=d, snapshot_every=10 ** 9)
    _same(want, _state(st2))
    assert st2.shard._dirty == set() and st2.shard.payloads.dirty == set()   # clean change record
    # a cut without a new delete carries the bitmap file forward; one after a delete replaces it
    st2.upsert(["y0"], _vec(300)[None], [_pl(0)])
    st2.snapshot()
    assert persist.committed_manifest(d)["dead"]["gen"] == 2 and _dead_files(d) == ["dead.2.bin"]
    st2.delete(point_ids=["y0"])
    st2.snapshot()
    g = persist.committed_manifest(d)["gen"]
    assert persist.committed_manifest(d)["dead"] == {"gen": g, "n": st2.shard.n_dead}
    assert _dead_files(d) == [f"dead.{g}.bin"]             # exactly one is left
    want = _state(st2)
    st2.wal.close()
    _same(want, _state(VectorStore(SD, 256, device="cpu", snapshot_dir=d)))


def test_snapshot_crash_before_commit_replays_deletes(tmp_path):
    d = str(tmp_path / "idx")
    st = _store(d=d, snapshot_every=10 ** 9)
    st.snapshot()
    _mutate(st)
    want = _state(st)
    persist.save_snapshot(st.shard, d, _crash_before_commit=True)   # gen 2 written, not committed
    st.wal.close()
    assert open(os.path.join(d, "CURRENT")).read().strip() == "manifest.1.json"
    st2 = VectorStore(SD, 256, device="cpu", snapshot_dir=d, snapshot_every=10 ** 9)
    _same(want, _state(st2))
    st2.snapshot()
    assert len(_dead_files(d)) == 1
    st2.wal.close()
    _same(want, _state(VectorStore(SD, 256, device="cpu", snapshot_dir=d)))


def test_manifest_without_dead_key_loads(tmp_path):
    d = str(tmp_path / "idx")
    st = _store(d=d, snapshot_every=10 ** 9)
    st.delete(point_ids=["p1"])
    st.snapshot()
    st.wal.close()
    # the manifest as an earlier version wrote it: no "dead" key (the zeros are in the segment)
    name = open(os.path.join(d, "CURRENT")).read().strip()
    with open(os.path.join(d, name)) as f:
        man = json.load(f)
    del man["dead"]
    with open(os.path.join(d, name), "w") as f:
        json.dump(man, f)
    st2 = VectorStore(SD, 256, device="cpu", snapshot_dir=d)
    assert st2.count == 30 and st2.shard.n_dead == 0 and st2.shard.dead is None
    assert not st2.shard.rows[1].view(torch.uint8).any()
    st2.wal.close()
