"""Point deletion on GPU shards (csrc/hip/index_delete.hip, the gated masked scans, and the search
over tombstones built on them) against ops/reference.filtered_topk_ref over the rows as they were
BEFORE the delete and the live mask.

Tolerances are test_filter_gpu.py's standing ones: scores and returned rows' true scores atol
2e-3, recall above 0.995 on random data; the conditions on WHICH rows may come back (live rows
only, no row twice, the (-inf, -1) tail exactly where the reference has it) carry no tolerance.
An fp8 shard is compared over the DECODED rows and queries, as in test_filter_fp8_gpu.py.

Where a test claims ``last_dead_hits == 0`` it first asserts, from the oracle, the precondition
under which the unmasked route cannot return a zeroed row: every query has at least k live rows
scoring above 0 (here: above the score tolerance)."""
import math

import numpy as np
import pytest
import torch

from codename_symbiont_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_SMALL = 64 * 37 + 19
N_BIG = 20_011
KNQ = ((10, 1), (10, 300), (32, 130))


def _queries(nq, D, seed=11):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(nq, D, generator=g), dim=-1).bfloat16().to(DEV)


def _decoded(q):
    from codename_symbiont_amd.ops import kernels as K

    return K.fp8_to_float(K.quant_fp8(q))


def _close(out, ref, atol, what):
    err = (out.float() - ref.float()).abs()
    bad = int((err > atol).sum())
    assert bad == 0, f"{what}: {bad} elems off, max err {float(err.max()):.4g}"


def _check(s, r, rows, qd, k, live, what, recall=False):
    """(scores, rows) of a search against the oracle over ``rows`` (as before any delete) under
    the bool mask ``live`` (device); returns the oracle's (scores, rows)."""
    n = rows.shape[0]
    ref_s, ref_i = R.filtered_topk_ref(rows, qd, k, live)
    torch.cuda.synchronize()
    assert s.shape == (qd.shape[0], k) and r.shape == (qd.shape[0], k), what
    assert s.dtype == torch.float32 and r.dtype == torch.int32, what
    fin = torch.isfinite(ref_s)
    assert int(fin[0].sum()) == min(k, int(live.sum())), what
    assert torch.equal(torch.isfinite(s), fin), f"{what}: the -inf tail is misplaced"
    assert bool((s[~fin] == -math.inf).all()) and bool((r[~fin] == -1).all()), what
    rr = r.long()
    got = rr[fin]
    assert bool((got >= 0).all()) and bool((got < n).all()), what
    assert bool(live[got].all()), f"{what}: a dead row came back"
    srt = torch.sort(torch.where(fin, rr, torch.arange(-k, 0, device=DEV).expand_as(rr)), 1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), f"{what}: a row came back twice"
    _close(s[fin], ref_s[fin], 2e-3, f"{what}: scores")
    true = R.row_scores_ref(rows, qd, rr.clamp_min(0))
    _close(s[fin], true[fin], 2e-3, f"{what}: returned rows' true scores")
    if recall:
        hit = ((rr[:, :, None] == ref_i[:, None, :]) & fin[:, :, None]).any(-1).sum()
        assert float(hit) / float(fin.sum()) > 0.995, what
    return ref_s, ref_i


def _same_outside_ties(s, r, s2, r2, what):
    _close(s, s2, 2e-3, f"{what}: scores")
    tie = torch.zeros_like(r, dtype=torch.bool)
    for a in (s, s2):
        tie[:, 1:] |= (a[:, 1:] - a[:, :-1]).abs() <= 2e-3
        tie[:, :-1] |= (a[:, :-1] - a[:, 1:]).abs() <= 2e-3
    assert bool(((r == r2) | tie).all()), f"{what}: rows differ outside ties"


# ---------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("dtype,D", [("bf16", 384), ("bf16", 768), ("bf16", 1024), ("fp8", 256),
                                     ("fp8", 1024)])
def test_tombstone_rows_kernel(dtype, D):
    from codename_symbiont_amd.ops import kernels as K

    n = N_SMALL
    pad = (n + 63) // 64 * 64
    rng = np.random.default_rng(D)
    g = torch.Generator(device="cpu").manual_seed(D)
    if dtype == "bf16":
        slab = torch.randn(pad, D, generator=g).bfloat16().to(DEV)
    else:
        slab = torch.randint(1, 255, (pad, D), generator=g, dtype=torch.uint8).to(DEV)
    # a second slab of one-byte elements beside a bf16 one (a shard's prefilter image)
    slab2 = (torch.randint(1, 255, (pad, D), generator=g, dtype=torch.uint8).to(DEV)
             if (dtype, D) == ("bf16", 384) else None)
    nw = pad // 64
    dead = torch.zeros(nw, dtype=torch.int64, device=DEV)
    want_rows = slab.clone()
    want_rows2 = None if slab2 is None else slab2.clone()
    want_bits = np.zeros(nw * 64, dtype=bool)
    lists = [[0, 63, 64, 65, n - 1], list(range(n // 64 * 64, n)),
             sorted(rng.choice(n, 200, replace=False).tolist()), [1234],
             [7, -1, n, n + 3, pad + 5]]               # entries outside [0, n): skipped
    for rows in lists:
        idx = torch.tensor(rows, dtype=torch.int32, device=DEV)
        ok = [r for r in rows if 0 <= r < n]
        want_rows[ok] = 0
        want_bits[ok] = True
        if want_rows2 is not None:
            want_rows2[ok] = 0
        for rep in range(2):                           # a second call changes nothing
            K.tombstone_rows(idx, n, dead, slab, slab2)
            torch.cuda.synchronize()
            assert torch.equal(slab.view(torch.uint8), want_rows.view(torch.uint8)), (rows[:5], rep)
            if slab2 is not None:
                assert torch.equal(slab2, want_rows2), (rows[:5], rep)
            words = np.packbits(want_bits, bitorder="little").view(np.int64)
            assert np.array_equal(dead.cpu().numpy(), words), (rows[:5], rep)
    # argument checks: dtype, contiguity, a list that could name a row past the slab
    idx = torch.tensor([1], dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError):
        K.tombstone_rows(idx.long(), n, dead, slab)
    with pytest.raises(TypeError):
        K.tombstone_rows(idx, n, dead.int(), slab)
    with pytest.raises(ValueError):
        K.tombstone_rows(idx, pad + 1, dead, slab)
    with pytest.raises(ValueError):
        K.tombstone_rows(idx, n, dead[:nw - 1], slab)
    with pytest.raises(ValueError):
        K.tombstone_rows(idx, n, dead, slab[:, :D - 8])
    with pytest.raises(TypeError):
        K.tombstone_rows(idx, n, dead, slab.float())


@pytest.mark.parametrize("nq,k", [(1, 1), (300, 32)])
def test_results_dead_kernel(nq, k):
    from codename_symbiont_amd.ops import kernels as K

    n = N_SMALL
    nw = (n + 63) // 64
    rng = np.random.default_rng(nq)
    bits = rng.random(nw * 64) < 0.3
    bits[0] = True
    bits[n - 1] = True
    bits[n - 2] = False
    dead = torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int64).copy()).to(DEV)
    ids = rng.integers(-1, n, (nq, k)).astype(np.int32)
    flat = ids.reshape(-1)
    flat[0] = 0                                        # row 0: dead
    if flat.size > 4:
        flat[1:5] = [-1, n - 1, n - 2, (nw - 1) * 64]  # -1, and rows of the last partial word
    want = int(bits[flat[flat >= 0]].sum())
    hits = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.results_dead(torch.from_numpy(ids).to(DEV), dead, hits)
    assert int(hits) == want and want > 0
    K.results_dead(torch.from_numpy(ids).to(DEV), dead, hits)          # it adds
    assert int(hits) == 2 * want
    none = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.results_dead(torch.full((nq, k), -1, dtype=torch.int32, device=DEV), dead, none)
    assert int(none) == 0
    with pytest.raises(TypeError):
        K.results_dead(torch.from_numpy(ids).to(DEV).long(), dead, hits)


@pytest.mark.parametrize("dtype,D", [("bf16", 384), ("bf16", 768), ("bf16", 1024), ("fp8", 256),
                                     ("fp8", 1024)])
def test_masked_scans_gate(dtype, D):
    """gate = 0: the candidate buffers stay as they were; gate = 1: the ungated call's output."""
    from codename_symbiont_amd.index.shard import HbmIndexShard
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import hip

    n, nq, n_rblk = N_SMALL, 70, 5
    sh = HbmIndexShard(D, n + 100, dtype=dtype)
    sh.fill_random(n, seed=D)
    q = _queries(nq, D)
    if dtype == "fp8":
        q, scan = K.quant_fp8(q), K.index_scan_filter_fp8
    else:
        scan = K.index_scan_filter
    mask = sh.make_mask(torch.from_numpy(np.random.default_rng(3).random(n) < 0.4).to(DEV))
    for kmax in (16, 32):
        lists = 2 if dtype == "fp8" else hip().topk_geometry(D, kmax)[0]
        m = n_rblk * lists * kmax
        ref = (torch.empty(nq, m, device=DEV), torch.empty(nq, m, dtype=torch.int32, device=DEV))
        scan(sh.rows, n, mask.words, mask.tiles, mask.n_live, q, kmax, n_rblk, *ref)
        for flag in (0, 1):
            cs = torch.full((nq, m), 123.0, device=DEV)
            ci = torch.full((nq, m), -7, dtype=torch.int32, device=DEV)
            gate = torch.full((1,), flag, dtype=torch.int32, device=DEV)
            scan(sh.rows, n, mask.words, mask.tiles, mask.n_live, q, kmax, n_rblk, cs, ci,
                 gate=gate)
            torch.cuda.synchronize()
            if flag:
                assert torch.equal(cs, ref[0]) and torch.equal(ci, ref[1]), kmax
            else:
                assert bool((cs == 123.0).all()) and bool((ci == -7).all()), kmax
    with pytest.raises(TypeError):
        scan(sh.rows, n, mask.words, mask.tiles, mask.n_live, q, 16, n_rblk, *ref,
             gate=torch.zeros(1, dtype=torch.int64, device=DEV))


# ---------------------------------------------------------------------------- list-scan routes
def _precondition(ref_s, k, what):
    assert bool((ref_s[:, k - 1] > 2e-3).all()), f"{what}: fewer than k live rows score above 0"


@pytest.mark.parametrize("k,nq", KNQ)
@pytest.mark.parametrize("dtype,D", [("bf16", 384), ("bf16", 768), ("bf16", 1024), ("fp8", 256),
                                     ("fp8", 384), ("fp8", 1024)])
def test_search_after_deletes_list_scan_routes(dtype, D, k, nq):
    from codename_symbiont_amd.index.shard import HbmIndexShard

    q = _queries(nq, D)
    qd = _decoded(q) if dtype == "fp8" else q
    for n in (N_SMALL, N_BIG):
        what = f"{dtype} D={D} n={n} k={k} nq={nq}"
        sh = HbmIndexShard(D, n + 100, dtype=dtype)
        sh.fill_random(n, seed=5 + D + n)
        # (an fp8 shard's default is the masked route: profiles/r10_delete/)
        assert sh.delete_route == {"bf16": "zero", "fp8": "mask"}[dtype]
        sh.delete_route = "zero"
        rows = sh.unit_rows()[:n].clone()
        raw = sh.rows[:n].clone()
        live = torch.ones(n, dtype=torch.bool, device=DEV)
        s0, r0 = sh.search(q, k)
        # 1. each query's current top 3: on the parent behaviour these rows would come back
        top = torch.unique(r0[:, :3].long().flatten())
        assert sh.delete_rows(top) == top.numel()
        live[top] = False
        ref_s, _ = _check(*sh.search(q, k), rows, qd, k, live, what + " top-3", recall=True)
        _precondition(ref_s, k, what)
        assert int(sh.last_dead_hits) == 0, what
        s1, r1 = sh.search(q, k)
        #    ... the rows themselves: live ones bit-identical, dead ones zero
        assert torch.equal(sh.rows[:n][live].view(torch.uint8), raw[live].view(torch.uint8))
        assert not bool(sh.rows[:n][~live].view(torch.uint8).any())
        #    ... and the masked route agrees
        sh.delete_route = "mask"
        s2, r2 = sh.search(q, k)
        sh.delete_route = "zero"
        _check(s2, r2, rows, qd, k, live, what + " top-3, mask route", recall=True)
        _same_outside_ties(s1, r1, s2, r2, what + " zero against mask route")
        assert int(sh.last_dead_hits) == 0
        # 2. whole tiles, the partial last one among them
        nt = (n + 63) // 64
        gone = [r for t in (0, 5, nt // 2, nt - 1) for r in range(t * 64, min(n, (t + 1) * 64))]
        sh.delete_rows(gone)
        live[gone] = False
        ref_s, _ = _check(*sh.search(q, k), rows, qd, k, live, what + " whole tiles", recall=True)
        _precondition(ref_s, k, what)
        assert int(sh.last_dead_hits) == 0, what
        # 3. all but k - 1 rows: the route returns zero rows, the fallback must replace them
        keep = np.random.default_rng(n + k).choice(n, k - 1, replace=False)
        live_h = torch.zeros(n, dtype=torch.bool)
        live_h[keep] = True
        live_h &= live.cpu()
        sh.delete_rows(torch.nonzero(~live_h & live.cpu()).flatten())
        live = live_h.to(DEV)
        assert sh.live_count == int(live.sum())
        _check(*sh.search(q, k), rows, qd, k, live, what + " all but k-1")
        assert int(sh.last_dead_hits) > 0, what
        # 4. every row
        sh.delete_rows(torch.nonzero(live).flatten())
        live[:] = False
        s, r = sh.search(q, k)
        assert sh.live_count == 0 and bool((s == -math.inf).all()) and bool((r == -1).all()), what


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_fallback_fires_when_live_scores_are_negative(dtype):
    """Rows around c, queries around -c: every live score is below 0, so the route's top k are
    the zeroed rows and the gated masked scan must run."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    D, n, k, nq = 384, N_BIG, 10, 64
    g = torch.Generator(device="cpu").manual_seed(77)
    c = torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)
    sh = HbmIndexShard(D, n + 100, dtype=dtype)
    sh.delete_route = "zero"
    sh.append_f32(c + 0.5 * torch.randn(n, D, generator=g) / math.sqrt(D))
    rows = sh.unit_rows()[:n].clone()
    qn = torch.nn.functional.normalize(-c + 0.1 * torch.randn(nq, D, generator=g) / math.sqrt(D),
                                       dim=-1).bfloat16().to(DEV)
    gone = np.random.default_rng(5).choice(n, 40, replace=False)
    sh.delete_rows(gone.tolist())
    live = torch.ones(n, dtype=torch.bool, device=DEV)
    live[torch.from_numpy(gone).to(DEV)] = False
    mixed = torch.cat([qn[:nq // 2], _queries(nq // 2, D, seed=78)])
    for what, q in (("negative", qn), ("mixed", mixed)):
        qd = _decoded(q) if dtype == "fp8" else q
        s, r = sh.search(q, k)
        ref_s, _ = _check(s, r, rows, qd, k, live, f"{dtype} {what}")
        neg = ref_s[:nq // 2] if what == "mixed" else ref_s
        full = R.topk_ref(rows[live], qd[:nq // 2] if what == "mixed" else qd, 1)[0]
        assert bool((full < 0).all()), "precondition: every live score of these queries is below 0"
        assert bool((neg < 0).all()) and bool((s[:neg.shape[0]] < 0).all())
        assert int(sh.last_dead_hits) > 0, what


# ---------------------------------------------------------------------------- pruned routes
@pytest.mark.parametrize("D,kind", [(384, "random"), (384, "near"), (768, "random")])
def test_search_after_deletes_pruned_routes(D, kind):
    """The int8-pruned search (stream tiers at 384, the MX-fp4 tier for near-duplicate queries,
    the LDS-ring int8 tier at 768) over a shard with tombstones, whole and through
    search_begin / search_end."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    n0, k, nq = (1 << 20) + 555, 10, 256
    g = torch.Generator(device=DEV).manual_seed(12)
    sh = HbmIndexShard(D, n0 + 8192, prune="i8")
    sh.fill_random(n0, seed=6)
    if kind == "near":
        c = torch.nn.functional.normalize(torch.randn(D, device=DEV, generator=g), dim=0)
        sh.append_f32(c + 0.1 * torch.randn(5000, D, device=DEV, generator=g) / math.sqrt(D))
        q = c + 0.1 * torch.randn(nq, D, device=DEV, generator=g) / math.sqrt(D)
    else:
        q = torch.randn(nq, D, device=DEV, generator=g)
    q = torch.nn.functional.normalize(q, dim=-1).bfloat16()
    n = sh.count
    rows = sh.unit_rows()[:n].clone()
    what = f"pruned D={D} {kind}"
    _, top = R.topk_ref(rows, q, 3)
    rng = np.random.default_rng(D)
    run0 = int(rng.integers(0, n0 - 200))
    gone = (set(top.flatten().tolist()) | set(range(run0, run0 + 200))
            | set(rng.choice(n, n // 100, replace=False).tolist()))
    assert sh.delete_rows(sorted(gone)) == len(gone)
    live = torch.ones(n, dtype=torch.bool, device=DEV)
    live[torch.tensor(sorted(gone), device=DEV)] = False
    for via in ("search", "begin/end"):
        if via == "search":
            s, r = sh.search(q, k)
        else:
            s, r = sh.search_end(sh.search_begin(q, k))
        hits, (cnt, ovf), tier = sh.last_dead_hits, sh._mq_last, sh._mx4_last
        ref_s, _ = _check(s, r, rows, q, k, live, f"{what} {via}", recall=True)
        _precondition(ref_s, k, what)
        assert int(hits) == 0, f"{what} {via}"
        assert int(ovf) == 0, f"{what} {via}: candidate overflow"
        # (the tier flag: 0 = the MX-fp4 tier ran)
        assert tier is not None and (int(tier) == 0) == (kind == "near"), f"{what} {via}"
    assert bool(torch.isfinite(sh.i8_bounds).all()) and bool(torch.isfinite(sh.mx4_bounds).all())
    s1, r1 = sh.search(q, k)
    sh.delete_route = "mask"
    s2, r2 = sh.search(q, k)
    _check(s2, r2, rows, q, k, live, what + " mask route", recall=True)
    _same_outside_ties(s1, r1, s2, r2, what + " zero against mask route")


# ---------------------------------------------------------------------------- the store
@pytest.mark.parametrize("pipeline", ["0", "1"])
def test_vector_store_delete_search_snapshot(pipeline, monkeypatch, tmp_path):
    from codename_symbiont_amd.index.filter import Filter
    from codename_symbiont_amd.index.shard import Payload
    from codename_symbiont_amd.index.store import VectorStore

    monkeypatch.setenv("SYMB_SEARCH_PIPELINE", pipeline)
    D, k = 384, 10
    d = str(tmp_path / "idx")
    st = VectorStore(D, 4096, device="cuda", snapshot_dir=d, snapshot_every=10 ** 9)
    assert (st._streams is not None) == (pipeline == "1")
    sizes = {"doc-a": 5, "doc-b": 40, "doc-c": 300}
    rng = np.random.default_rng(12)
    ids, pls = [], []
    for doc, m in sizes.items():
        for j in range(m):
            ids.append(f"{doc}/{j}")
            pls.append(Payload(doc, f"http://{doc}.example", f"s{j}", j, "m", 0))
    order = rng.permutation(len(ids))
    ids, pls = [ids[i] for i in order], [pls[i] for i in order]
    vecs = rng.standard_normal((len(ids), D)).astype(np.float32)
    st.upsert(ids, vecs, pls)
    q = rng.standard_normal((9, D)).astype(np.float32)
    f_c = Filter(must={"original_document_id": "doc-c"})
    st.search(q, k, filter=f_c)                        # a cached mask from before the delete
    assert st.delete(filter=Filter(must={"original_document_id": "doc-b"})) == 40
    assert st.delete(point_ids=["doc-c/0", "doc-c/1", "nope"]) == 2
    assert st.live_count == 303 and st.count == 345

    def docs_of(s, r):
        fin = np.isfinite(s)
        assert (r[fin] >= 0).all() and (r[~fin] == -1).all()
        hits = [st.lookup(int(g)) for g in r[fin]]
        assert all(pid is not None for pid, _ in hits)            # a dead row has no point
        return [(pid, p.original_document_id) for pid, p in hits]

    def all_checks(st):
        s, r = st.search(q, 345)                                   # k > 32: the masked matmul
        for i in range(9):
            got = docs_of(s[i], r[i])
            assert len(got) == 303 and len(set(got)) == 303
            assert not any(doc == "doc-b" or pid in ("doc-c/0", "doc-c/1") for pid, doc in got)
        s, r = st.search(q, k)                                     # the list scan + dead check
        assert np.isfinite(s).all()
        assert not any(doc == "doc-b" for pid, doc in docs_of(s, r))
        s, r = st.search(q, k, filter=f_c)
        got = docs_of(s, r)
        assert len(got) == 9 * k and all(doc == "doc-c" for _, doc in got)
        assert not any(pid in ("doc-c/0", "doc-c/1") for pid, _ in got)
        s, r = st.search(q, k, filter=Filter(must={"original_document_id": "doc-b"}))
        assert not np.isfinite(s).any() and (r == -1).all()
        # the deleted vectors themselves no longer match anything closely
        s, r = st.search(vecs[[ids.index("doc-c/0")]], 1)
        assert s[0, 0] < 0.9
        return st.search(q, k)

    want = all_checks(st)
    st.snapshot()
    st.delete(point_ids=["doc-a/0"])                               # after the cut: in the WAL
    want = st.search(q, k)
    st.wal.close()
    st2 = VectorStore(D, 4096, device="cuda", snapshot_dir=d, snapshot_every=10 ** 9)
    assert st2.count == 345 and st2.live_count == 302
    assert torch.equal(st2.shard.dead, st.shard.dead)
    assert torch.equal(st2.shard.rows[:345].view(torch.int16),
                       st.shard.rows[:345].view(torch.int16))
    got = st2.search(q, k)
    assert np.array_equal(got[1], want[1]) and np.allclose(got[0], want[0], atol=1e-6)
    st2.wal.close()
