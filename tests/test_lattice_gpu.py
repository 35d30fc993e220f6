"""Every search route of a GPU shard against the fp32 oracle, BIT FOR BIT, on lattice data.

tests/lattice.py makes rows and queries whose every dot product is exact in fp32 under any
summation order, so no route has a rounding excuse: the returned scores must equal the oracle's
top-k values exactly (``torch.equal`` inside ``lattice.check_exact``), the ids must be distinct,
in range, allowed under a mask, and each must score exactly what its slot says.  The data families
hold what random Gaussian rows never do: ties inside the top k and across the k-th place
(ternary rows, planted exact duplicates at tile and row-block edges) and score sets that are
negative throughout (orthant rows).  tests/test_lattice_cpu.py checks the data and the checker.

Each case builds one shard with ``append_unit``, asserts that the route it is named after is the
one that ran (the chunked matmul is spied on and must stay unused), and calls ``check_exact``.
Two sizes: a small ragged tier for the list scans, and 266,240 + 777 rows for the routes that
need ``_tile_sample_plan`` (the smallest shard with 64 sample groups at the default tile shift),
with the size gates lowered on the test's own shard instance.

Every case prints one ``LATTICE {...}`` line: route, family, overflow flag, mean candidates."""
import json

import pytest
import torch

import lattice as L
from codename_symbiont_amd.index.shard import TILE_ROWS, HbmIndexShard

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_BIG = 266_240 + 777
FAMILIES = ("dense", "ternary", "orthant", "dups")
EXTRA = ("ternary", "orthant", "dups")
_CACHE: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def matmul_calls(monkeypatch):
    """Calls of the chunked matmul (the fall-back of every route): a case asserts none."""
    calls = []
    real = HbmIndexShard._search_matmul

    def spy(self, *a, **kw):
        calls.append((self.dim, self.dtype))
        return real(self, *a, **kw)

    monkeypatch.setattr(HbmIndexShard, "_search_matmul", spy)
    return calls


def _data(family: str, n: int, D: int, nq: int):
    """(rows, queries, plan) of a family, cached.  ``dups`` is the dense family with 2, 9 and 70
    exact copies of the best rows of queries 0, 1 and 2 planted (``plan``: source -> copies).
    Where the shapes allow, the last four dense queries are exact copies of stored rows."""
    key = (family, n, D, nq)
    if key not in _CACHE:
        plan = {}
        if family == "dups":
            x0, q, _ = _data("dense", n, D, nq)
            best = L.oracle_topk(x0, q[:3], 1)[1][:, 0].tolist()
            x, plan = L.with_duplicates(x0, best, [2, 9, 70][:len(best)], seed=n + D)
        elif family == "orthant":
            x = L.orthant(n, D, seed=n + D + 1, device=DEV)
            q = L.orthant_queries(nq, D, seed=n + D + 2, device=DEV)
        else:
            gen = L.dense if family == "dense" else L.ternary
            x = gen(n, D, seed=n + D + 3, device=DEV)
            q = gen(nq, D, seed=n + D + 4, device=DEV)
            if n >= 4096 and nq >= 17:
                q[-4:] = x[torch.tensor([5, n // 3, n // 2, n - 2], device=DEV)]
        _CACHE[key] = (x, q, plan)
    return _CACHE[key]


def _shard(x, dtype="bf16", gates=True, **kw):
    """A shard holding exactly ``x``.  ``gates``: the row-count gates of the sampled routes
    lowered on this instance (as the older tests lower ``mq_min_nq``); no default changes."""
    n, D = x.shape
    sh = HbmIndexShard(D, n + TILE_ROWS, device=DEV, dtype=dtype, **kw)
    sh.append_unit(x)
    assert sh.visible == n
    if gates:
        sh.SEED_MIN_ROWS = 0
        sh.FP8_LARGE_K_MIN_ROWS = 0
    return sh


def _note(route, family, **kw):
    print("LATTICE " + json.dumps(dict(route=route, family=family, **kw)))


def _flags(pair):
    """(overflow flag, mean candidates per query) of a route's (cnt, ovf) record."""
    cnt, ovf = pair
    return int(ovf.item()), round(float(cnt.float().mean()), 1)


def _allowed(n: int, seed: int, plan=None) -> torch.Tensor:
    """About half the rows at random, two whole 64-row tiles dead, the last visible row allowed
    (so the last allowed row IS the last visible one); with a duplicates plan, the first source
    row allowed and one of its exact copies masked out (a tie across the mask)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.rand(n, generator=g, device=DEV) < 0.5
    a[2 * TILE_ROWS:3 * TILE_ROWS] = False
    last_full = n // TILE_ROWS - 1
    a[last_full * TILE_ROWS:(last_full + 1) * TILE_ROWS] = False
    a[n - 1] = True
    if plan:
        src = next(iter(plan))
        twin = [p for p in plan[src] if p != n - 1][0]
        a[src], a[twin] = True, False
    return a


# ------------------------------------------------------------------------------ list scans
def _small_cases():
    cases = []
    widths = [("bf16", D) for D in (384, 768, 1024)] + [("fp8", D) for D in (256, 384, 512, 768, 1024)]
    for dtype, D in widths:
        cases += [(dtype, D, 4133, 257, 10, "dense"), (dtype, D, 4133, 17, 20, "dense")]
    for dtype in ("bf16", "fp8"):
        for n in (3, 63, 64, 65):
            cases += [(dtype, 384, n, 1, 10, "dense"), (dtype, 384, n, 17, 32, "dense"),
                      (dtype, 384, n, 256, 5, "dense")]
        cases += [(dtype, 384, 4133, 256, 32, "dense"), (dtype, 1024, 65, 257, 16, "dense"),
                  (dtype, 384, 4133, 1, 10, "ternary")]
        for D in (384, 1024):
            for fam in EXTRA:
                cases += [(dtype, D, 4133, 257, 10, fam), (dtype, D, 4133, 17, 20, fam)]
    return cases


@pytest.mark.parametrize("dtype,D,n,nq,k,family", _small_cases())
def test_list_scan_is_bit_exact(dtype, D, n, nq, k, family, matmul_calls):
    """The bf16 / e4m3 list scan + merge (kmax 16 and 32) on ragged shards: fewer rows than k,
    one row short of / exactly / one past a tile, several row blocks with a ragged last one;
    1, 17, 256 and 257 queries (one block, a ragged one, a full one, one past it)."""
    x, q, _ = _data(family, n, D, nq)
    sh = _shard(x, dtype, gates=False)
    assert sh._seed_rows(n, k) == 0, "unseeded list scan"
    if n == 4133:
        # several row blocks of whole tiles, so no block size divides n: the last one is ragged
        assert n % TILE_ROWS and n > 2 * TILE_ROWS * sh.scan_min_tiles
    if dtype == "fp8":
        assert torch.equal(sh.unit_rows(), x), "the e4m3 image is lossless on lattice data"
    s, r = sh.search(q, k)
    torch.cuda.synchronize()
    assert not matmul_calls and r.dtype == torch.int32
    L.check_exact(s, r, x, q, k, what=f"list {dtype} D={D} n={n} nq={nq} k={k} {family}")
    if n < k:
        assert bool((r[:, n:] == -1).all()) and bool(torch.isinf(s[:, n:]).all())


@pytest.mark.parametrize("dtype,D,family", [("bf16", 384, f) for f in FAMILIES]
                         + [("fp8", 1024, f) for f in FAMILIES])
def test_seeded_list_scan_is_bit_exact(dtype, D, family, matmul_calls):
    """``scan_mq = False``: the list scan seeded with the k-th best of the first n / 64 rows (a
    threshold one ulp below it: a row that ties the seed must survive)."""
    nq, k = 300, 10
    x, q, _ = _data(family, N_BIG, D, nq)
    sh = _shard(x, dtype)
    sh.scan_mq = False
    assert sh._seed_rows(N_BIG, k) > 0 and not sh._mq_ok(nq, k, sh.rows, dtype)
    sh._mq_last = None
    s, r = sh.search(q, k)
    torch.cuda.synchronize()
    assert not matmul_calls and sh._mq_last is None
    L.check_exact(s, r, x, q, k, what=f"seeded list {dtype} D={D} {family}")


# ------------------------------------------------------------------------------ emitting scan
@pytest.mark.parametrize("D,nq,rsplit,family",
                         [(384, 300, True, "dense"), (384, 300, False, "dense"),
                          (384, 512, True, "dense"), (384, 1100, True, "dense"),
                          (768, 300, True, "dense"), (1024, 300, True, "dense")]
                         + [(384, 300, True, f) for f in EXTRA]
                         + [(384, 300, False, "ternary"), (384, 512, True, "dups")]
                         + [(768, 300, True, f) for f in EXTRA]
                         + [(1024, 300, True, "ternary")])
def test_emitting_scan_is_bit_exact(D, nq, rsplit, family, matmul_calls):
    """The 256 / 512-query emitting scan behind the in-place tile sample: its threshold is a
    sampled k-th best less a margin, so every row tied with the true k-th must be emitted and the
    select must pick k distinct ones."""
    k = 10
    x, q, _ = _data(family, N_BIG, D, nq)
    sh = _shard(x)
    sh.mq_min_nq, sh.mq_rsplit = 256, rsplit
    assert sh._seed_rows(N_BIG, k) and sh._mq_ok(nq, k, sh.rows, "bf16")
    assert sh._tile_sample_plan(N_BIG) is not None
    sh._mq_last = None
    s, r = sh.search(q, k)
    torch.cuda.synchronize()
    assert not matmul_calls and sh._mq_last is not None
    ovf, cnt = _flags(sh._mq_last)
    _note(f"emitting D={D} nq={nq} rsplit={int(rsplit)}", family, ovf=ovf, cand=cnt)
    if family != "orthant":
        assert ovf == 0, "the emitting scan's own result, not the gated list-scan fallback"
    L.check_exact(s, r, x, q, k, what=f"emitting D={D} nq={nq} rsplit={rsplit} {family}")


# ------------------------------------------------------------------------------ large k
@pytest.mark.parametrize("dtype,D,k,family",
                         [(dt, D, k, "dense") for dt, D in (("bf16", 384), ("bf16", 1024), ("fp8", 768))
                          for k in (17, 64, 128)]
                         + [(dt, D, 64, f) for dt, D in (("bf16", 384), ("bf16", 1024), ("fp8", 768))
                            for f in EXTRA]
                         + [("bf16", 384, 128, "ternary"), ("fp8", 384, 128, "ternary"),
                            ("fp8", 384, 100, "dups")])
def test_large_k_is_bit_exact(dtype, D, k, family, matmul_calls):
    """16 < k <= 128: bf16, the sampled threshold + emitting scan + radix select; fp8, the list
    scan (kmax 32) at k = 17 and the emitting e4m3 scan under the all-ones mask above 32."""
    nq = 300
    x, q, _ = _data(family, N_BIG, D, nq)
    sh = _shard(x, dtype)
    sh._mq_last = sh._filter_large_k_last = None
    s, r = sh.search(q, k)
    torch.cuda.synchronize()
    assert not matmul_calls
    if dtype == "bf16":
        assert sh._tile_sample_plan(N_BIG, sh.PRUNE_TILE_SHIFT) is not None
        assert sh._mq_last is not None and sh._filter_large_k_last is None
        last = sh._mq_last
    elif k <= 32:
        assert sh._filter_large_k_last is None and sh._mq_last is None
        last = None
    else:
        assert sh._filter_large_k_serves(k) and sh._filter_large_k_last is not None
        last = sh._filter_large_k_last
    if last is not None:
        ovf, cnt = _flags(last)
        _note(f"large-k {dtype} D={D} k={k}", family, ovf=ovf, cand=cnt)
        if family != "orthant":
            assert ovf == 0
    L.check_exact(s, r, x, q, k, what=f"large-k {dtype} D={D} k={k} {family}")


# ------------------------------------------------------------------------------ fp8 prefilter
@pytest.mark.parametrize("D,family", [(384, f) for f in FAMILIES] + [(768, f) for f in FAMILIES])
def test_prefilter_is_bit_exact(D, family, matmul_calls):
    """``prefilter="fp8"``: e4m3 is lossless on lattice data, so the e4m3 candidate scan ranks
    by the exact scores and the re-scored top k must be exact, not merely high-recall."""
    nq, k = 300, 10
    x, q, _ = _data(family, N_BIG, D, nq)
    sh = _shard(x, prefilter="fp8")
    assert sh.rows8 is not None and sh.prefilter == "fp8"
    s, r = sh.search(q, k)
    torch.cuda.synchronize()
    assert not matmul_calls
    L.check_exact(s, r, x, q, k, what=f"prefilter D={D} {family}")


# ------------------------------------------------------------------------------ pruned search
PRUNE_MODES = {
    # name: (D, SYMB_PRUNE_STREAM, SYMB_PRUNE_I8, SYMB_I8_SPLIT)
    "384-stream": (384, "1", "auto", "auto"),
    "384-lds": (384, "0", "auto", "auto"),
    "768-ring": (768, "1", "ring", "auto"),
    "768-stream": (768, "1", "stream", "auto"),
    "1024-stream": (1024, "1", "auto", "auto"),
    "384-split": (384, "1", "auto", "on"),
}


@pytest.mark.parametrize("mode,family,nq", [(m, "dense", 300) for m in PRUNE_MODES]
                         + [(m, f, 300) for m in ("384-stream", "768-ring") for f in EXTRA]
                         + [("384-lds", "ternary", 300), ("384-split", "dups", 300),
                            ("1024-stream", "dups", 300)]
                         # the smallest batch the route takes, and the 512-query forms
                         + [("384-stream", "dense", 16), ("384-stream", "dups", 512),
                            ("384-stream", "ternary", 1100), ("384-lds", "dups", 512),
                            ("768-ring", "dense", 512), ("384-split", "ternary", 512)])
def test_pruned_search_is_bit_exact(mode, family, nq, matmul_calls, monkeypatch):
    """``prune="i8"``: the int8 / split / MX-fp4 tiers only choose candidates; every returned
    score is a bf16 re-score, so the result must be exact whichever tier, route or fallback ran
    (the flags are recorded, not asserted: the int8 band's population on lattice data is not a
    contract).  Four dense queries are exact copies of stored rows (MX-fp4 tier candidates)."""
    D, stream, i8k, split = PRUNE_MODES[mode]
    monkeypatch.setenv("SYMB_PRUNE_STREAM", stream)
    monkeypatch.setenv("SYMB_PRUNE_I8", i8k)
    monkeypatch.setenv("SYMB_I8_SPLIT", split)
    k = 10
    x, q, _ = _data(family, N_BIG, D, nq)
    sh = _shard(x, prune="i8")
    assert sh.stream == (stream == "1") and sh.i8_ring == (mode == "768-ring")
    if split == "on":
        sh.calibrate_prune()
        assert sh._i8_heavy == 64
    elif family != "orthant":
        # (orthant rows share a mean direction: a 384-wide shard takes the split image by itself)
        assert sh._i8_heavy == 0
    assert sh._seed_rows(N_BIG, k) and nq >= sh.prune_min_nq
    sh._mq_last = sh._route_last = None
    s, r = sh.search(q, k)
    torch.cuda.synchronize()
    assert not matmul_calls
    assert sh._route_last is not None and sh._mq_last is not None, "the pruned search ran"
    ovf, cnt = _flags(sh._mq_last)
    mx4 = None if sh._mx4_last is None else int(sh._mx4_last.item()) == 0
    _note(f"pruned {mode} nq={nq}", family, ovf=ovf, cand=cnt, all_dense=int(sh._route_last.item()),
          mx4_tier=mx4, heavy=sh._i8_heavy)
    L.check_exact(s, r, x, q, k, what=f"pruned {mode} {family} nq={nq}")
    # the pipelined halves (search_begin on the rows visible now, search_end later) agree
    s2, r2 = sh.search_end(sh.search_begin(q, k))
    torch.cuda.synchronize()
    assert not matmul_calls
    L.check_exact(s2, r2, x, q, k, what=f"pruned {mode} {family} nq={nq} begin/end")


# ------------------------------------------------------------------------------ masks
def _spy(sh, name):
    calls = []
    real = getattr(sh, name)

    def wrapped(*a, **kw):
        calls.append(name)
        return real(*a, **kw)

    setattr(sh, name, wrapped)
    return calls


@pytest.mark.parametrize("dtype,D,n,family",
                         [("bf16", 384, 4133, "dups"), ("bf16", 1024, 4133, "dups"),
                          ("bf16", 384, N_BIG, "dups"), ("fp8", 384, 4133, "dups"),
                          ("fp8", 512, 4133, "dups"), ("fp8", 1024, N_BIG, "dups"),
                          ("bf16", 384, 4133, "orthant"), ("bf16", 768, N_BIG, "orthant"),
                          ("fp8", 384, 4133, "orthant"), ("fp8", 384, N_BIG, "orthant"),
                          ("bf16", 384, N_BIG, "ternary"), ("fp8", 1024, 4133, "ternary")])
def test_masked_list_scan_is_bit_exact(dtype, D, n, family, matmul_calls):
    """The masked list scan (seed pass over every 64th live tile, then the full pass from its
    k-th best less one ulp): the duplicates family masks out an exact copy of an allowed top row,
    the orthant family keeps every threshold below zero."""
    nq, k = 48, 10
    x, q, plan = _data(family, n, D, nq)
    sh = _shard(x, dtype, gates=False)
    allowed = _allowed(n, 5, plan)
    mask = sh.make_mask(allowed)
    assert mask.tiles is not None
    ran = _spy(sh, "_search_filtered")
    s, r = sh.search(q, k, allow=mask)
    torch.cuda.synchronize()
    assert ran and not matmul_calls
    L.check_exact(s, r, x, q, k, allowed, what=f"masked list {dtype} D={D} n={n} {family}")


@pytest.mark.parametrize("dtype,D,family",
                         [("bf16", 384, "dups"), ("bf16", 768, "dups"), ("fp8", 384, "dups"),
                          ("fp8", 1024, "dups"), ("bf16", 384, "orthant"), ("fp8", 384, "orthant"),
                          ("bf16", 1024, "ternary"), ("fp8", 768, "ternary")])
def test_masked_emitting_scan_is_bit_exact(dtype, D, family, matmul_calls):
    """k = 64 under a mask: the seed passes' k-th best finite candidate (less the margin on bf16,
    less one ulp on fp8), the masked emitting scan, the radix select."""
    nq, k = 48, 64
    x, q, plan = _data(family, N_BIG, D, nq)
    sh = _shard(x, dtype)
    allowed = _allowed(N_BIG, 6, plan)
    mask = sh.make_mask(allowed)
    assert mask.tiles is not None and sh._filter_large_k_serves(k)
    sh._filter_large_k_last = None
    s, r = sh.search(q, k, allow=mask)
    torch.cuda.synchronize()
    assert not matmul_calls and sh._filter_large_k_last is not None
    ovf, cnt = _flags(sh._filter_large_k_last)
    _note(f"masked emitting {dtype} D={D} k={k}", family, ovf=ovf, cand=cnt)
    if family != "orthant":
        assert ovf == 0
    L.check_exact(s, r, x, q, k, allowed, what=f"masked emitting {dtype} D={D} {family}")


@pytest.mark.parametrize("dtype,n,family",
                         [("bf16", 4133, "dups"), ("bf16", N_BIG, "dups"), ("fp8", 4133, "dups"),
                          ("fp8", N_BIG, "dups"), ("bf16", 4133, "orthant"), ("fp8", 4133, "orthant")])
def test_grouped_scan_is_bit_exact(dtype, n, family, matmul_calls):
    """Three masks over 48 queries in one grouped scan: each query exact under its own mask."""
    nq, k, D = 48, 10, 384
    x, q, plan = _data(family, n, D, nq)
    sh = _shard(x, dtype, gates=False)
    allows = [_allowed(n, 7, plan), _allowed(n, 8), _allowed(n, 9, plan)]
    group_of = [(i * 7) % 3 for i in range(nq)]
    groups = sh.make_mask_groups(allows, group_of)
    assert len(groups) == 3 and sh._group_scan_serves(k, groups)
    chunk, single = _spy(sh, "_search_group_chunk"), _spy(sh, "_search_masked")
    s, r = sh.search(q, k, allow=groups)
    torch.cuda.synchronize()
    assert len(chunk) == 1 and not single and not matmul_calls
    per_query = torch.stack(allows)[torch.tensor(group_of, device=DEV)]
    L.check_exact(s, r, x, q, k, per_query, what=f"grouped {dtype} n={n} {family}")


@pytest.mark.parametrize("dtype,n,prune,k,family",
                         [("bf16", 4133, None, 10, "dups"), ("bf16", N_BIG, "i8", 10, "dups"),
                          ("fp8", 4133, None, 10, "dups"), ("fp8", N_BIG, None, 10, "dups"),
                          ("bf16", N_BIG, None, 64, "dups"), ("fp8", N_BIG, None, 64, "dups"),
                          ("bf16", 4133, None, 10, "orthant"), ("bf16", N_BIG, "i8", 10, "orthant"),
                          ("fp8", N_BIG, None, 10, "orthant"), ("bf16", N_BIG, None, 64, "orthant")])
def test_tombstoned_then_compacted_shard_is_bit_exact(dtype, n, prune, k, family, matmul_calls):
    """Every query's top 3 rows deleted: both ``delete_route`` values return the exact top k of
    the live rows, and after ``compact()`` the unmasked routes do, over the renumbered rows.  A
    zeroed dead row scores exactly 0: below every top-k score of the duplicates family (the
    unmasked route's result stands), above every score of the orthant family (the "zero" route
    must see the dead ids and take its gated masked fallback)."""
    nq, D = 48, 384
    x, q, _ = _data(family, n, D, nq)
    sh = _shard(x, dtype, **({"prune": prune} if prune else {}))
    top3 = L.oracle_topk(x, q, 3)[1].flatten()
    live = torch.ones(n, dtype=torch.bool, device=DEV)
    live[top3] = False
    assert sh.delete_rows(top3) == int((~live).sum())
    for route in ("zero", "mask"):
        sh.delete_route = route
        s, r = sh.search(q, k)
        torch.cuda.synchronize()
        assert not matmul_calls
        hits = None if sh.last_dead_hits is None else int(sh.last_dead_hits.item())
        _note(f"tombstoned {dtype} n={n} k={k} route={route}", family, dead_hits=hits)
        if route == "zero":
            assert (hits > 0) == (family == "orthant")
        L.check_exact(s, r, x, q, k, live, what=f"tombstoned {dtype} n={n} k={k} {route} {family}")
    assert sh.compact() == int((~live).sum()) and sh.n_dead == 0 and sh.visible == int(live.sum())
    xl = x[live]
    s, r = sh.search(q, k)
    torch.cuda.synchronize()
    assert not matmul_calls
    L.check_exact(s, r, xl, q, k, what=f"compacted {dtype} n={n} k={k} {family}")
