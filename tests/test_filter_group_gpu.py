"""The grouped masked list scan (csrc/hip/filter_scan.h, GROUPED) and the search under a mask per
query built on it: against ops/reference.grouped_filtered_topk_ref, and -- bit for bit in scores --
against the single-mask scan (the same kernel) of each group's queries under that group's mask.

Shapes are test_filter_gpu.py's, the smallest at which the kernel can go wrong: 64 * 37 + 19 rows
(a partial last tile, few workgroups) and 20 011 rows (several workgroups, slices longer than the
ring).  Tolerances are that file's standing ones against the fp32 oracle (scores atol 2e-3,
recall above 0.995 on random masks); the conditions on WHICH rows may come back carry none.
Group ids are interleaved over neighbouring queries (lanes), never sorted."""
import math

import numpy as np
import pytest
import torch

from codename_symbiont_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_SMALL = 64 * 37 + 19
N_BIG = 20_011
CASES = [(D, k, nq) for D in (384, 768, 1024) for k, nq in ((10, 1), (10, 300), (32, 130))]

_shards = {}


def _shard(D, n):
    """One random shard per (width, rows) for the whole module (never written after this)."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    key = (D, n)
    if key not in _shards:
        sh = HbmIndexShard(D, n + 100)
        sh.fill_random(n, seed=5 + D + n)
        _shards[key] = sh
    return _shards[key]


def _queries(nq, D, seed=11):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(nq, D, generator=g), dim=-1).bfloat16().to(DEV)


def _tiles_mask(n, tiles):
    a = torch.zeros(n, dtype=torch.bool)
    for t in tiles:
        a[t * 64:(t + 1) * 64] = True
    return a


def _rows_mask(n, idx):
    return torch.zeros(n, dtype=torch.bool).index_fill_(0, torch.as_tensor(list(idx)), True)


def _mixes(n, k):
    """name -> (list of bool [n] masks on the host, random?)."""
    nt = (n + 63) // 64
    rng = np.random.default_rng(n + k)
    ones, zero = torch.ones(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool)
    uni = lambda share: torch.from_numpy(rng.random(n) < share)
    last = list(range((nt - 1) * 64, n))
    half = _tiles_mask(n, [5])
    half[5 * 64 + 32:] = False
    return {
        "ones next to zero": ([ones, zero], False),
        "eight documents": ([_tiles_mask(n, range(g, nt, 8)) for g in range(8)], False),
        "k-1 rows, none, half": ([_rows_mask(n, rng.choice(n, k - 1, replace=False)), zero,
                                  uni(0.5)], False),
        "one bit per tile": ([_rows_mask(n, [r for r in (t * 64 + (t * 7 + g * 13) % 64
                                                         for t in range(nt)) if r < n])
                              for g in range(4)], False),
        "partial last tile only": ([_rows_mask(n, last), _rows_mask(n, last[::2]),
                                    _rows_mask(n, last[-1:])], False),
        "union of 1 live tile": ([half, _tiles_mask(n, [5]) & ~half, _tiles_mask(n, [5])], False),
        "union of 2 live tiles": ([_tiles_mask(n, [5]), _tiles_mask(n, [nt - 2])], False),
        "union of 3 live tiles": ([_tiles_mask(n, [0]), _tiles_mask(n, [9]), _tiles_mask(n, [20]),
                                   _tiles_mask(n, [0, 20])], False),
        "uniform 50% x 8": ([uni(0.5) for _ in range(8)], True),
        "must_not 1% x 5": ([~_tiles_mask(n, range(g, nt, 100)) for g in range(5)], True),
    }


def _close(out, ref, atol, what):
    err = (out.float() - ref.float()).abs()
    bad = int((err > atol).sum())
    assert bad == 0, f"{what}: {bad} elems off, max err {float(err.max()):.4g}"


def _same(s, r, s1, r1, what):
    """Scores bit for bit; rows too, outside runs of equal scores."""
    assert torch.equal(s, s1), f"{what}: scores differ"
    rr, r1 = r.long(), r1.long()
    tie = torch.zeros_like(rr, dtype=torch.bool)
    if s.shape[1] > 1:
        tie[:, 1:] |= s[:, 1:] == s[:, :-1]
        tie[:, :-1] |= s[:, :-1] == s[:, 1:]
    assert bool(((rr == r1) | tie).all()), f"{what}: rows differ"


def _check(sh, q, k, allows, group_of, what, random_mask=False, per_group=True):
    """One grouped search against the oracle and against the per-group single-mask searches;
    returns (scores, rows)."""
    n, nq = sh.visible, q.shape[0]
    allows_d = [a.to(DEV) for a in allows]
    mg = sh.make_mask_groups(allows_d, group_of)
    s, r = sh.search(q, k, allow=mg)
    rows = sh.unit_rows()[:n]
    ref_s, ref_i = R.grouped_filtered_topk_ref(rows, q, k, allows_d, group_of)
    torch.cuda.synchronize()
    assert s.shape == (nq, k) and r.shape == (nq, k), what
    assert s.dtype == torch.float32 and r.dtype == torch.int32, what
    fin = torch.isfinite(ref_s)
    g_d = torch.tensor(group_of, device=DEV)
    cnt = torch.stack(allows_d).sum(1)[g_d].clamp_max(k)
    assert torch.equal(fin.sum(1), cnt), what
    # the (-inf, -1) tail is exactly where the oracle has it
    assert torch.equal(torch.isfinite(s), fin), what
    assert bool((s[~fin] == -math.inf).all()) and bool((r[~fin] == -1).all()), what
    rr = r.long()
    # hard conditions: rows the query's OWN mask allows, none at or past `visible`, none twice
    # (with the exact tail: a query with k allowed rows or fewer gets exactly its allowed set)
    assert bool((rr[fin] >= 0).all()) and bool((rr[fin] < n).all()), what
    own = torch.stack(allows_d)[g_d[:, None].expand_as(rr), rr.clamp_min(0)]
    assert bool(own[fin].all()), f"{what}: a row another query's mask allows came back"
    srt = torch.sort(torch.where(fin, rr, torch.arange(-k, 0, device=DEV).expand_as(rr)), 1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), f"{what}: a row came back twice"
    _close(s[fin], ref_s[fin], 2e-3, f"{what}: scores")
    true = R.row_scores_ref(rows, q, rr.clamp_min(0))
    _close(s[fin], true[fin], 2e-3, f"{what}: returned rows' true scores")
    if random_mask:
        hit = ((rr[:, :, None] == ref_i[:, None, :]) & fin[:, :, None]).any(-1).sum()
        assert float(hit) / float(fin.sum()) > 0.995, what
    if per_group:
        # same row, same score: each group's queries under the single-mask search
        for g, a in enumerate(allows_d):
            idx = [i for i in range(nq) if group_of[i] == g]
            if idx:
                sg, rg = sh.search(q[idx], k, allow=a)
                _same(s[idx], r[idx], sg, rg, f"{what}: group {g}")
    return s, r


@pytest.mark.parametrize("D,k,nq", CASES)
def test_grouped_search_mixes(D, k, nq):
    """Every group mix against the oracle and, per group, the single-mask search bit for bit
    (all three widths, both kmax).  (nq = 1 names one group: the single-mask route.)"""
    q = _queries(nq, D)
    for n in (N_SMALL, N_BIG):
        sh = _shard(D, n)
        for name, (allows, rnd) in _mixes(n, k).items():
            G = len(allows)
            group_of = [(i * 3 + i // 7) % G for i in range(nq)]   # interleaved over the lanes
            _check(sh, q, k, allows, group_of, f"D={D} n={n} k={k} nq={nq} {name}", rnd)


def _count_scans(monkeypatch):
    from codename_symbiont_amd.ops import kernels as K

    calls = []
    real = K.index_scan_filter_group
    monkeypatch.setattr(K, "index_scan_filter_group",
                        lambda *a, **kw: (calls.append(a[6].shape[0]), real(*a, **kw))[1])
    return calls


@pytest.mark.parametrize("G,scans", [(9, 2), (17, 3)])
def test_chunks_of_eight_masks(G, scans, monkeypatch):
    D, n, k, nq = 384, N_SMALL, 10, 60
    sh = _shard(D, n)
    q = _queries(nq, D, seed=51)
    rng = np.random.default_rng(G)
    allows = [torch.from_numpy(rng.random(n) < 0.3) for _ in range(G)]
    group_of = [(i * 5) % G for i in range(nq)]
    calls = _count_scans(monkeypatch)
    sh.filter_seed = False
    try:
        _check(sh, q, k, allows, group_of, f"{G} masks", True, per_group=False)
    finally:
        sh.filter_seed = type(sh).FILTER_SEED_DEFAULT
    assert len(calls) == scans and sum(calls) == nq
    _check(sh, q, k, allows, group_of, f"{G} masks, seeded", True)


def test_few_disjoint_masks_over_an_extra_query_block_keep_the_loop(monkeypatch):
    """The route condition (_loop_keeps_chunk): two to four disjoint masks, 256 queries at 768
    (one query block per group, two together), a union of GROUP_LOOP_MIN_TILES tiles or more.
    Both routes give the same bits."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    D, n, k, nq = 768, N_BIG, 10, 256
    sh = _shard(D, n)
    q = _queries(nq, D, seed=71)
    nt = (n + 63) // 64
    even, odd = _tiles_mask(n, range(0, nt, 2)), _tiles_mask(n, range(1, nt, 2))
    group_of = [i % 2 for i in range(nq)]
    calls = _count_scans(monkeypatch)
    s, r = _check(sh, q, k, [even, odd], group_of, "below the tile floor")
    assert len(calls) == 2                              # seed pass + full pass
    monkeypatch.setattr(HbmIndexShard, "GROUP_LOOP_MIN_TILES", 1)
    for what, allows, nq_used, scans in (
            ("disjoint, two blocks against one each", [even, odd], nq, 0),
            ("disjoint, one block either way", [even, odd], 128, 2),
            ("overlapping", [even | odd, even], nq, 2),
            ("three overlapping masks", [even, odd, even | odd], nq, 2),
            ("four disjoint masks", [_tiles_mask(n, range(g, nt, 4)) for g in range(4)], nq, 0),
            ("five disjoint masks", [_tiles_mask(n, range(g, nt, 5)) for g in range(5)], nq, 2)):
        calls.clear()
        go = [i % len(allows) for i in range(nq_used)]
        mg = sh.make_mask_groups([a.to(DEV) for a in allows], go)
        s1, r1 = sh.search(q[:nq_used], k, allow=mg)
        assert len(calls) == scans, what
        if len(allows) == 2 and allows[1] is odd:
            _same(s1, r1, s[:nq_used], r[:nq_used], what)


def test_all_queries_in_one_group_is_the_ungrouped_search(monkeypatch):
    """One distinct mask (given once, or twice as equal masks): the single-mask search, and no
    grouped scan.  And the kernel itself with every query in slot 3: the single-mask kernel's
    candidates, bit for bit."""
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import hip

    D, n, k, nq = 768, N_BIG, 10, 130
    sh = _shard(D, n)
    q = _queries(nq, D, seed=52)
    a = torch.from_numpy(np.random.default_rng(53).random(n) < 0.2).to(DEV)
    calls = _count_scans(monkeypatch)
    s0, r0 = sh.search(q, k, allow=a)
    for masks, group_of in (([a], [0] * nq), ([a, a.clone()], [i % 2 for i in range(nq)])):
        mg = sh.make_mask_groups(masks, group_of)
        assert len(mg) == 1
        s, r = sh.search(q, k, allow=mg)
        assert torch.equal(s, s0) and torch.equal(r, r0)
    assert calls == []
    mask = sh.make_mask(a)
    lists, _ = hip().topk_geometry(D, 16)
    n_rblk = 7
    shape = (nq, n_rblk * lists * 16)
    cs0, ci0 = torch.empty(shape, device=DEV), torch.empty(shape, dtype=torch.int32, device=DEV)
    cs1, ci1 = torch.empty(shape, device=DEV), torch.empty(shape, dtype=torch.int32, device=DEV)
    K.index_scan_filter(sh.rows, n, mask.words, mask.tiles, mask.n_live, q, 16, n_rblk, cs0, ci0)
    mask8 = torch.zeros(mask.words.numel(), 8, dtype=torch.int64, device=DEV)
    mask8[:, 3] = mask.words
    qgroup = torch.full((nq,), 3, dtype=torch.int32, device=DEV)
    K.index_scan_filter_group(sh.rows, n, mask8, qgroup, mask.tiles, mask.n_live, q, 16, n_rblk,
                              cs1, ci1)
    torch.cuda.synchronize()
    assert torch.equal(cs0, cs1) and torch.equal(ci0, ci1)


def test_raw_wrapper_on_dirty_words():
    """The kernel on words whose bits at or past `visible` are set in every slot, with copies of
    the queries in the slab's rows past `visible` (a scan that ignored n_valid would return them
    at 1.0), qgroup entries of 8 + g, a closed gate, and the seed pass on and off."""
    from codename_symbiont_amd.index.shard import HbmIndexShard
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import hip, stream_handle

    D, n, k, nq = 384, N_SMALL, 10, 19
    sh = HbmIndexShard(D, n + 100)
    sh.fill_random(n, seed=3)
    q = _queries(nq, D)
    sh.rows[n:n + nq].copy_(q)                      # unpublished rows of the last tile and beyond
    rng = np.random.default_rng(4)
    slots = (0, 2, 7)
    allows = [torch.from_numpy(rng.random(n) < share) for share in (0.2, 0.5, 0.03)]
    group_of = [i % 3 for i in range(nq)]
    s0, r0 = _check(sh, q, k, allows, group_of, "bool masks")
    nw = (n + 63) // 64
    mask8 = np.zeros((nw, 8), dtype=np.uint64)
    for g, a in zip(slots, allows):
        pad = np.zeros(nw * 64, dtype=bool)
        pad[:n] = a.numpy()
        mask8[:, g] = np.packbits(pad, bitorder="little").view(np.uint64)
    mask8[n // 64, :] |= np.uint64((0xFFFFFFFFFFFFFFFF << (n % 64)) & 0xFFFFFFFFFFFFFFFF)
    mask8_d = torch.from_numpy(mask8.view(np.int64)).to(DEV)
    union = mask8_d[:, 0] | mask8_d[:, 2] | mask8_d[:, 7]
    tiles, n_live = K.filter_tiles(union.contiguous(), n)
    # every other query names its slot as 8 + slot: only the low three bits count
    qgroup = torch.tensor([slots[g] + (8 if i % 2 else 0) for i, g in enumerate(group_of)],
                          dtype=torch.int32, device=DEV)
    lists, _ = hip().topk_geometry(D, 16)
    n_rblk = 5
    cs = torch.full((nq, n_rblk * lists * 16), 123.0, device=DEV)
    ci = torch.full((nq, n_rblk * lists * 16), -7, dtype=torch.int32, device=DEV)
    gate = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.index_scan_filter_group(sh.rows, n, mask8_d, qgroup, tiles, n_live, q, 16, n_rblk, cs, ci,
                              gate=gate)
    torch.cuda.synchronize()
    assert bool((cs == 123.0).all()) and bool((ci == -7).all())     # closed gate: untouched
    gate.fill_(1)
    K.index_scan_filter_group(sh.rows, n, mask8_d, qgroup, tiles, n_live, q, 16, n_rblk, cs, ci,
                              gate=gate)
    out_s = torch.empty(nq, k, device=DEV)
    out_i = torch.empty(nq, k, dtype=torch.int32, device=DEV)
    hip().topk_merge(cs.data_ptr(), ci.data_ptr(), nq, cs.shape[1], 16, k, out_s.data_ptr(),
                     out_i.data_ptr(), 0, 0, stream_handle(sh.device), 0)
    torch.cuda.synchronize()
    assert int(out_i.max()) < n
    assert torch.equal(out_s, s0) and torch.equal(out_i, r0)
    # seed pass on == off
    mg = sh.make_mask_groups([a.to(DEV) for a in allows], group_of)
    try:
        sh.filter_seed = False
        s1, r1 = sh.search(q, k, allow=mg)
    finally:
        sh.filter_seed = type(sh).FILTER_SEED_DEFAULT
    assert torch.equal(s1, s0) and torch.equal(r1, r0)


def test_seed_pass_on_and_off_identical():
    D, k, nq = 1024, 32, 130
    sh = _shard(D, N_BIG)
    q = _queries(nq, D, seed=41)
    mixes = _mixes(N_BIG, k)
    try:
        for name in ("ones next to zero", "eight documents", "uniform 50% x 8",
                     "union of 3 live tiles"):
            allows = [a.to(DEV) for a in mixes[name][0]]
            mg = sh.make_mask_groups(allows, [(i * 3) % len(allows) for i in range(nq)])
            sh.filter_seed = True
            s1, r1 = sh.search(q, k, allow=mg)
            sh.filter_seed = False
            s0, r0 = sh.search(q, k, allow=mg)
            torch.cuda.synchronize()
            assert torch.equal(s0, s1) and torch.equal(r0, r1), name
    finally:
        sh.filter_seed = type(sh).FILTER_SEED_DEFAULT


def test_tombstones_under_grouped_masks():
    from codename_symbiont_amd.index.shard import HbmIndexShard

    D, n, k, nq = 384, N_SMALL, 10, 40
    sh = HbmIndexShard(D, n + 100)
    sh.fill_random(n, seed=61)
    q = _queries(nq, D, seed=62)
    rng = np.random.default_rng(63)
    allows = [torch.from_numpy(rng.random(n) < 0.5) for _ in range(3)]
    group_of = [i % 3 for i in range(nq)]
    mg = sh.make_mask_groups([a.to(DEV) for a in allows], group_of)
    s, r = sh.search(q, k, allow=mg)
    dead = torch.unique(r[:, :3].long().flatten())          # the best rows of every query
    sh.delete_rows(dead.tolist())
    with pytest.raises(ValueError, match="before a delete"):
        sh.search(q, k, allow=mg)
    with pytest.raises(ValueError, match="before a delete"):
        sh.make_mask_groups(mg.masks, group_of)
    alive = torch.ones(n, dtype=torch.bool)
    alive[dead.cpu()] = False
    # masks made now pass no dead row: the oracle under allow & alive, per group bit for bit
    mg2 = sh.make_mask_groups([a.to(DEV) for a in allows], group_of)
    s2, r2 = sh.search(q, k, allow=mg2)
    assert not bool(torch.isin(r2.long(), dead).any())
    ref_s, _ = R.grouped_filtered_topk_ref(sh.unit_rows()[:n], q, k,
                                           [(a & alive).to(DEV) for a in allows], group_of)
    _close(s2, ref_s, 2e-3, "after the delete")
    for g, a in enumerate(allows):
        idx = [i for i in range(nq) if group_of[i] == g]
        sg, rg = sh.search(q[idx], k, allow=a.to(DEV))
        _same(s2[idx], r2[idx], sg, rg, f"after the delete: group {g}")


def _bar(monkeypatch, *names):
    from codename_symbiont_amd.index.shard import HbmIndexShard

    for name in names:
        def barred(self, *a, _name=name, **kw):
            raise AssertionError(f"the search took {_name}")
        monkeypatch.setattr(HbmIndexShard, name, barred)


@pytest.mark.parametrize("pipeline", ["0", "1"])
def test_vector_store_filter_list(pipeline, monkeypatch):
    from codename_symbiont_amd.index.filter import Filter
    from codename_symbiont_amd.index.shard import Payload
    from codename_symbiont_amd.index.store import VectorStore

    monkeypatch.setenv("SYMB_SEARCH_PIPELINE", pipeline)
    D, k = 384, 10
    st = VectorStore(D, 4096, device="cuda")
    assert (st._streams is not None) == (pipeline == "1")
    sizes = {"doc-a": 5, "doc-b": 40, "doc-c": 300, "doc-d": 700}
    rng = np.random.default_rng(12)
    ids, pls = [], []
    for doc, m in sizes.items():
        for j in range(m):
            ids.append(f"{doc}/{j}")
            pls.append(Payload(doc, f"http://{doc}.example", f"s{j}", j, "m", 0))
    order = rng.permutation(len(ids))                  # documents interleaved over the rows
    ids, pls = [ids[i] for i in order], [pls[i] for i in order]
    st.upsert(ids, rng.standard_normal((len(ids), D)).astype(np.float32), pls)
    only = lambda doc: Filter(must={"original_document_id": doc})
    but = lambda doc: Filter(must_not={"original_document_id": doc})
    flts = [only("doc-a"), None, but("doc-d"), only("doc-c"), but("doc-c"), None, only("doc-a"),
            but("doc-d"), Filter(point_ids=["doc-b/1", "doc-d/2"]), only("doc-b"), but("doc-a")]
    q = rng.standard_normal((len(flts), D)).astype(np.float32)
    s, r = st.search(q, k, filter=flts)
    assert s.shape == (len(flts), k) and r.shape == (len(flts), k)
    for i, f in enumerate(flts):
        si, ri = st.search(q[i], k, filter=f)
        fin = np.isfinite(si[0])
        assert np.array_equal(np.isfinite(s[i]), fin) and (r[i][~fin] == -1).all(), i
        if f is not None:
            # the single-mask scan of this request alone: the same bits
            assert np.array_equal(s[i], si[0]), i
        else:
            # (an unfiltered search picks its route by the batch: the standing tolerance)
            assert np.allclose(s[i][fin], si[0][fin], rtol=0, atol=2e-3), i
        tie = np.zeros(k, bool)
        tie[1:] |= si[0][1:] == si[0][:-1]
        tie[:-1] |= si[0][:-1] == si[0][1:]
        assert ((r[i] == ri[0]) | tie | (f is None)).all(), i
    # the None entries are the plain search of those queries, bit for bit
    plain = [i for i, f in enumerate(flts) if f is None]
    sp, rp = st.search(q[plain], k)
    assert np.array_equal(s[plain], sp) and np.array_equal(r[plain], rp)
    assert int(np.isfinite(s[0]).sum()) == 5 and int(np.isfinite(s[8]).sum()) == 2
    assert {st.lookup(int(g))[0] for g in r[8][:2]} == {"doc-b/1", "doc-d/2"}
    # the route really taken: no filtered entry goes through a single-mask search or the matmul
    rest = [i for i, f in enumerate(flts) if f is not None]
    with monkeypatch.context() as m:
        _bar(m, "_search_masked", "_search_matmul")
        calls = _count_scans(m)
        s2, r2 = st.search(q[rest], k, filter=[flts[i] for i in rest])
        assert len(calls) == 2 and calls[0] == len(rest)      # seed pass + full pass, one chunk
    assert np.array_equal(s2, s[rest]) and np.array_equal(r2, r[rest])


def test_wrapper_validation_errors():
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import hip

    D, n, nq = 384, N_SMALL, 7
    sh = _shard(D, n)
    q = _queries(nq, D)
    nw = (n + 63) // 64
    mask8 = torch.zeros(nw, 8, dtype=torch.int64, device=DEV)
    qgroup = torch.zeros(nq, dtype=torch.int32, device=DEV)
    tiles, n_live = K.filter_tiles(mask8[:, 0].contiguous(), n)
    lists, _ = hip().topk_geometry(D, 16)
    cs = torch.empty(nq, 2 * lists * 16, device=DEV)
    ci = torch.empty(nq, 2 * lists * 16, dtype=torch.int32, device=DEV)

    def call(rows=sh.rows, n_valid=n, m8=mask8, qg=qgroup, tl=tiles, nl=n_live, qq=q, kmax=16,
             n_rblk=2, cs=cs, ci=ci, **kw):
        K.index_scan_filter_group(rows, n_valid, m8, qg, tl, nl, qq, kmax, n_rblk, cs, ci, **kw)

    call()                                              # the baseline is accepted
    torch.cuda.synchronize()
    with pytest.raises(TypeError):
        call(m8=mask8.to(torch.int32))
    with pytest.raises(TypeError):
        call(qg=qgroup.long())
    with pytest.raises(ValueError):
        call(m8=torch.zeros(nw, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        call(m8=mask8[:, 0].contiguous())               # the single-mask layout
    with pytest.raises(ValueError):
        call(m8=torch.zeros(8, nw, dtype=torch.int64, device=DEV).t())   # not contiguous
    with pytest.raises(ValueError):
        call(m8=mask8[:nw - 1])                         # does not cover n_valid
    with pytest.raises(ValueError):
        call(qg=qgroup[:nq - 1])
    with pytest.raises(ValueError):
        call(qg=torch.zeros(nq + 1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        call(qg=qgroup.cpu())
    with pytest.raises(ValueError):
        call(kmax=8)
    with pytest.raises(ValueError):
        call(stride=0)
    with pytest.raises(ValueError):
        call(n_rblk=3)                                  # candidate workspace too small
    with pytest.raises(ValueError):
        call(n_valid=sh.rows.shape[0] + 64)
    with pytest.raises(ValueError):
        call(rows=torch.zeros(n + 100, 256, dtype=torch.bfloat16, device=DEV),
             qq=_queries(nq, 256))
    with pytest.raises(ValueError):
        call(thr_init=torch.zeros(nq - 1, device=DEV))
    with pytest.raises(TypeError):
        call(gate=torch.zeros(1, dtype=torch.int64, device=DEV))
