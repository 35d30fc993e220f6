"""The masked e4m3 list scan (csrc/hip/fp8_filter_scan.h) and the filtered search of a GPU fp8
shard built on it, against ops/reference.filtered_topk_ref over the DECODED rows and queries (the
MFMA sums exact e4m3 products in fp32), against the unfiltered fp8 search, and against the fp8
list scan over the gathered rows.

Shapes are test_filter_gpu.py's: 64 * 37 + 19 rows (a partial last tile, few workgroups) and
20 011 rows (several workgroups, slices longer than the ring).  Tolerances are the suite's
standing ones for this kernel family (test_kernels_gpu.py::
test_index_scan_fp8_exact_on_decoded_rows): scores and returned rows' true scores atol 2e-3,
recall above 0.99 on the random masks; the conditions on WHICH rows may come back carry no
tolerance.  Same-kernel comparisons (masked against unmasked, masked against gathered) use
atol 1e-6, the suite's figure for same-kernel repeats: per row the MFMA chain is the same."""
import math

import numpy as np
import pytest
import torch

from codename_symbiont_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_SMALL = 64 * 37 + 19
N_BIG = 20_011
DIMS = (256, 384, 512, 768, 1024)
CASES = [(D, k, nq) for D in DIMS for k, nq in ((10, 1), (10, 300), (32, 130))]

_shards = {}


def _shard(D, n):
    """One random fp8 shard per (width, rows) for the whole module (never written after this),
    with its decoded rows."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    key = (D, n)
    if key not in _shards:
        sh = HbmIndexShard(D, n + 100, device=DEV, dtype="fp8")
        sh.fill_random(n, seed=5 + D + n)
        _shards[key] = (sh, sh.unit_rows()[:n])
    return _shards[key]


def _queries(nq, D, seed=11):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(nq, D, generator=g), dim=-1).bfloat16().to(DEV)


def _decoded(q):
    """The queries the fp8 scan scores: e4m3(FP8_SCALE * q), decoded."""
    from codename_symbiont_amd.ops import kernels as K

    return K.fp8_to_float(K.quant_fp8(q))


def _tiles_mask(n, tiles):
    a = torch.zeros(n, dtype=torch.bool)
    for t in tiles:
        a[t * 64:(t + 1) * 64] = True
    return a


def _masks(n, k):
    """name -> (bool [n] on the host, random?)."""
    nt = (n + 63) // 64
    rng = np.random.default_rng(n + k)
    rows = lambda idx: torch.zeros(n, dtype=torch.bool).index_fill_(0, torch.as_tensor(idx), True)
    per_tile = [t * 64 + (t * 7) % 64 for t in range(nt)]
    m = {
        "ones": (torch.ones(n, dtype=torch.bool), False),
        "zero": (torch.zeros(n, dtype=torch.bool), False),
        "one row": (rows([777 % n]), False),
        "k-1 rows": (rows(rng.choice(n, k - 1, replace=False)), False),
        "one bit per tile": (rows([r for r in per_tile if r < n]), False),
        "alternate tiles dead": (_tiles_mask(n, range(0, nt, 2)), False),
        "1 live tile": (_tiles_mask(n, [5]), False),
        "2 live tiles": (_tiles_mask(n, [5, nt - 2]), False),
        "3 live tiles": (_tiles_mask(n, [0, 9, 20]), False),
        "7 live tiles": (_tiles_mask(n, [1, 2, 3, 11, 17, 30, nt - 2]), False),
        "partial last tile only": (rows(list(range((nt - 1) * 64, n))), False),
        "uniform 50%": (torch.from_numpy(rng.random(n) < 0.5), True),
        "uniform 1%": (torch.from_numpy(rng.random(n) < 0.01), True),
    }
    return m


def _close(out, ref, atol, what):
    err = (out.float() - ref.float()).abs()
    bad = int((err > atol).sum())
    assert bad == 0, f"{what}: {bad} elems off, max err {float(err.max()):.4g}"


def _check_out(s, r, rows, qd, k, allow, what, random_mask=False):
    """(scores, rows) of one masked search against the reference over the decoded rows [n, D]
    and decoded queries; ``allow``: bool [n] on the host."""
    n = rows.shape[0]
    allow_d = allow.to(DEV)
    ref_s, ref_i = R.filtered_topk_ref(rows, qd, k, allow_d)
    torch.cuda.synchronize()
    assert s.shape == (qd.shape[0], k) and r.shape == (qd.shape[0], k), what
    assert s.dtype == torch.float32 and r.dtype == torch.int32, what
    fin = torch.isfinite(ref_s)
    n_allowed = int(allow.sum())
    assert int(fin[0].sum()) == min(k, n_allowed), what
    # the (-inf, -1) tail is exactly where the reference has it
    assert torch.equal(torch.isfinite(s), fin), what
    assert bool((s[~fin] == -math.inf).all()) and bool((r[~fin] == -1).all()), what
    rr = r.long()
    got = rr[fin]
    # hard conditions: allowed rows only, none at or past `visible`, none twice
    assert bool((got >= 0).all()) and bool((got < n).all()), what
    assert bool(allow_d[got].all()), f"{what}: a disallowed row came back"
    srt = torch.sort(torch.where(fin, rr, torch.arange(-k, 0, device=DEV).expand_as(rr)), 1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), f"{what}: a row came back twice"
    _close(s[fin], ref_s[fin], 2e-3, f"{what}: scores")
    true = R.row_scores_ref(rows, qd, rr.clamp_min(0))
    _close(s[fin], true[fin], 2e-3, f"{what}: returned rows' true scores")
    if n_allowed <= k:
        want = torch.nonzero(allow_d).flatten()
        have = torch.sort(rr[:, :n_allowed], 1).values
        assert torch.equal(have, want.expand_as(have)), f"{what}: not the allowed set"
    if random_mask:
        hit = ((rr[:, :, None] == ref_i[:, None, :]) & fin[:, :, None]).any(-1).sum()
        assert float(hit) / float(fin.sum()) > 0.99, what


def _check(sh, rows, q, qd, k, allow, what, random_mask=False, arg=None):
    """One filtered search through the shard against the reference; returns (scores, rows)."""
    s, r = sh.search(q, k, allow=allow.to(DEV) if arg is None else arg)
    _check_out(s, r, rows, qd, k, allow, what, random_mask)
    return s, r


def _same_rows(sh, q, s, r, ref_r, what):
    """Rows equal except inside runs of equal scores (``s``: the scores both searches agree on),
    as test_filter_gpu.py compares them.  Exact ties are common among sums of e4m3 products, and
    a run can go on past k, where no equal neighbour shows it.  So a LAST slot whose rows differ
    without an equal neighbour must be proved a tie: neither row is among the other side's rows,
    and the two rows, searched alone under a two-row mask (k = 2, the masked kernel, the same
    per-row MFMA chain), score the same bit for bit, which is the slot's score."""
    rr, gg = r.long(), ref_r.long()
    tie = torch.zeros_like(rr, dtype=torch.bool)
    tie[:, 1:] |= s[:, 1:] == s[:, :-1]
    tie[:, :-1] |= s[:, :-1] == s[:, 1:]
    diff = (rr != gg) & ~tie
    assert not bool(diff[:, :-1].any()), f"{what}: rows differ outside ties"
    for i in torch.nonzero(diff[:, -1]).flatten().tolist():
        a, b = int(rr[i, -1]), int(gg[i, -1])
        assert a >= 0 and b >= 0, f"{what}: query {i}, last slot {a} against {b}"
        assert b not in rr[i].tolist() and a not in gg[i].tolist(), f"{what}: query {i}"
        s2, r2 = sh.search(q[i:i + 1], 2, allow=[a, b])
        assert sorted(r2[0].tolist()) == sorted((a, b)), f"{what}: query {i}"
        assert float(s2[0, 0]) == float(s2[0, 1]) == float(s[i, -1]), \
            f"{what}: query {i}: last slot {a} against {b} is no tie"


def _raw_search(sh, n, words, q8, k, kmax, n_rblk, stride=1):
    """filter_tiles + index_scan_filter_fp8 + topk_merge on packed words; raw scores rescaled."""
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import hip, stream_handle

    nq = q8.shape[0]
    tiles, n_live = K.filter_tiles(words, n)
    cs = torch.empty(nq, n_rblk * 2 * kmax, device=DEV)
    ci = torch.empty(nq, n_rblk * 2 * kmax, dtype=torch.int32, device=DEV)
    K.index_scan_filter_fp8(sh.rows, n, words, tiles, n_live, q8, kmax, n_rblk, cs, ci,
                            stride=stride)
    out_s = torch.empty(nq, k, device=DEV)
    out_i = torch.empty(nq, k, dtype=torch.int32, device=DEV)
    hip().topk_merge(cs.data_ptr(), ci.data_ptr(), nq, cs.shape[1], kmax, k, out_s.data_ptr(),
                     out_i.data_ptr(), 0, 0, stream_handle(sh.device), 0)
    return out_s * (1.0 / (K.FP8_SCALE * K.FP8_SCALE)), out_i, tiles, n_live


def _words(allow):
    """bool [n] on the host -> packed int64 words on the device."""
    n = allow.numel()
    b = np.zeros((n + 63) // 64 * 8, dtype=np.uint8)
    p = np.packbits(allow.numpy(), bitorder="little")
    b[:p.size] = p
    return torch.from_numpy(b).to(DEV).view(torch.int64)


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,k,nq", CASES)
def test_filtered_fp8_search_masks(D, k, nq):
    q = _queries(nq, D)
    qd = _decoded(q)
    for n in (N_SMALL, N_BIG):
        sh, rows = _shard(D, n)
        for name, (allow, rnd) in _masks(n, k).items():
            _check(sh, rows, q, qd, k, allow, f"D={D} n={n} k={k} nq={nq} {name}", rnd)


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_slices_around_the_ring_depth(D):
    """0 .. NS + 2 live tiles spread over the shard, in one slice and in three, every entry and
    every second one: slices shorter than the ring, as long as it and longer (the prologue's
    NS list reads and the clamped re-loads), empty slices, and n_live = 0.  With a stride the
    kernel walks every stride-th entry of each workgroup's slice, so the reference's mask is
    the allowed rows of exactly those tiles."""
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import hip

    n, k, nq = N_SMALL, 10, 70
    nt = (n + 63) // 64
    sh, rows = _shard(D, n)
    q = _queries(nq, D, seed=51)
    q8 = K.quant_fp8(q)
    qd = K.fp8_to_float(q8)
    rng = np.random.default_rng(D)
    ns = hip().filter_fp8_ring_depth(D)        # the ring depth the kernel was built with
    assert 2 <= ns <= 8
    for m in range(0, ns + 3):
        live = sorted({int(round(t)) for t in np.linspace(0, nt - 1, m)}) if m else []
        assert len(live) == m
        allow = torch.zeros(n, dtype=torch.bool)
        for t in live:                        # a random half of each live tile, never empty
            lo, hi = t * 64, min(n, t * 64 + 64)
            allow[lo:hi] = torch.from_numpy(rng.random(hi - lo) < 0.5)
            allow[lo] = True
        words = _words(allow)
        for n_rblk in (1, 3):
            per = -(-m // n_rblk)
            for stride in (1, 2):
                walked = [t for rb in range(n_rblk) for t in live[rb * per:(rb + 1) * per][::stride]]
                want = allow & _tiles_mask(n, walked)
                for kmax in (16, 32):
                    what = f"D={D} live={m} n_rblk={n_rblk} stride={stride} kmax={kmax}"
                    s, r, _, n_live = _raw_search(sh, n, words, q8, k, kmax, n_rblk, stride)
                    assert int(n_live) == m, what
                    _check_out(s, r, rows, qd, k, want, what)


# 3 ------------------------------------------------------------------------------------------------
def test_bits_and_rows_past_visible():
    """Packed words with every bit past `visible` set give the bool mask's result, through the
    shard and through the raw kernel pair, with e4m3 copies of the queries sitting in the slab's
    rows past `visible` (a scan that ignored n_valid would return them at ~1.0)."""
    from codename_symbiont_amd.index.shard import HbmIndexShard
    from codename_symbiont_amd.ops import kernels as K

    D, n, k, nq = 384, N_SMALL, 10, 19
    sh = HbmIndexShard(D, n + 100, device=DEV, dtype="fp8")
    sh.fill_random(n, seed=3)
    rows = sh.unit_rows()[:n]
    q = _queries(nq, D)
    q8 = K.quant_fp8(q)
    qd = K.fp8_to_float(q8)
    sh.rows[n:n + nq].copy_(q8)                     # unpublished rows of the last tile and beyond
    allow = torch.from_numpy(np.random.default_rng(4).random(n) < 0.2)
    s0, r0 = _check(sh, rows, q, qd, k, allow, "bool")
    dirty = np.full((n + 63) // 64 * 8 + 24, 0xFF, dtype=np.uint8)
    packed = np.packbits(allow.numpy(), bitorder="little")
    dirty[:packed.size] = packed
    dirty[n // 8] |= (0xFF << (n % 8)) & 0xFF
    for what, arg in (("packed", dirty), ("device packed", torch.from_numpy(dirty).to(DEV))):
        s, r = _check(sh, rows, q, qd, k, allow, what, arg=arg)
        assert torch.equal(s, s0) and torch.equal(r, r0), what
        assert int(r.max()) < n, what
    # the kernels themselves on words whose bits past n are all set
    nw = (n + 63) // 64
    words = torch.from_numpy(dirty[:nw * 8].copy()).to(DEV).view(torch.int64)
    s, r, _, n_live = _raw_search(sh, n, words, q8, k, 16, 5)
    _check_out(s, r, rows, qd, k, allow, "raw kernels")
    assert int(n_live) == len({int(t) // 64 for t in torch.nonzero(allow).flatten()})
    assert int(r.max()) < n
    assert torch.equal(s, s0)
    _same_rows(sh, q, s0, r, r0, "raw kernels")


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,k", [(1024, 10), (384, 32)])
def test_all_ones_mask_equals_no_mask(D, k):
    """A filter must not change what a score means: under an all-ones mask the search returns
    the unmasked fp8 search's scores (e4m3 queries, the same per-row MFMA chain) and rows."""
    sh, _ = _shard(D, N_BIG)
    q = _queries(300, D, seed=61)
    s_all, r_all = sh.search(q, k)
    s, r = sh.search(q, k, allow=torch.ones(N_BIG, dtype=torch.bool, device=DEV))
    torch.cuda.synchronize()
    _close(s, s_all, 1e-6, f"D={D} k={k}: all-ones mask against no mask")
    _same_rows(sh, q, s_all, r, r_all, f"D={D} k={k}")


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,k,nq", [(384, 10, 300), (768, 10, 130), (1024, 32, 64), (256, 32, 70),
                                    (512, 10, 257)])
def test_filtered_equals_fp8_list_scan_over_gathered_rows(D, k, nq):
    from codename_symbiont_amd.ops import kernels as K

    sh, _ = _shard(D, N_BIG)
    q = _queries(nq, D, seed=31)
    q8 = K.quant_fp8(q)
    rng = np.random.default_rng(6)
    docs = torch.zeros(N_BIG, dtype=torch.bool)
    for s0 in rng.choice(N_BIG - 200, 12, replace=False):
        docs[s0:s0 + 200] = True
    kmax = 16 if k <= 16 else 32
    for what, allow in (("uniform 50%", torch.from_numpy(rng.random(N_BIG) < 0.5)), ("documents", docs)):
        idx = torch.nonzero(allow.to(DEV)).flatten()
        m = idx.numel()
        sub = torch.zeros((m + 63) // 64 * 64, D, dtype=torch.uint8, device=DEV)
        torch.index_select(sh.rows, 0, idx, out=sub[:m])
        gs, gi = sh._scan(m, q8, kmax, k, None, None, rows=sub, dtype="fp8")
        gs = gs * (1.0 / (K.FP8_SCALE * K.FP8_SCALE))
        gi = idx[gi.long()]
        for seed in (False, True):
            sh.filter_seed = seed
            try:
                s, r = sh.search(q, k, allow=allow.to(DEV))
            finally:
                sh.filter_seed = type(sh).FILTER_SEED_DEFAULT
            torch.cuda.synchronize()
            _close(s, gs, 1e-6, f"{what} seed={seed}")
            _same_rows(sh, q, gs, r, gi, f"{what} seed={seed}")


# 6 ------------------------------------------------------------------------------------------------
def test_planted_copies_allowed_found_disallowed_never():
    from codename_symbiont_amd.index.shard import HbmIndexShard
    from codename_symbiont_amd.ops import kernels as K

    D, n, k, nq = 384, N_BIG, 10, 40
    sh = HbmIndexShard(D, n + 100, device=DEV, dtype="fp8")
    sh.fill_random(n, seed=21)
    q = _queries(nq, D, seed=22)
    q8 = K.quant_fp8(q)
    bad = torch.arange(nq) + 100                       # disallowed copies, in live tiles 1 and 2
    good = (torch.arange(nq) + 50) * 64 + 5            # allowed copies, each alone in its tile
    sh.rows[bad.to(DEV)] = q8
    sh.rows[good.to(DEV)] = q8
    allow = torch.zeros(n, dtype=torch.bool)
    allow[:40 * 64] = torch.from_numpy(np.random.default_rng(5).random(40 * 64) < 0.1)
    allow[bad] = False
    allow[good] = True
    s_all, r_all = sh.search(q, k)
    s, r = _check(sh, sh.unit_rows()[:n], q, K.fp8_to_float(q8), k, allow, "planted")
    # (a copy scores |e4m3(q)|^2, 1 up to the rounding; a random row of this width below 0.4)
    assert bool((s_all[:, 0] > 0.9).all())
    assert bool(((r_all[:, :2].long() == bad.to(DEV)[:, None]).any(1)).all())
    assert torch.equal(r[:, 0].long(), good.to(DEV)) and bool((s[:, 0] > 0.9).all())
    assert not bool((r.long()[:, :, None] == bad.to(DEV)[None, None, :]).any())


# 7 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [384, 768])
def test_seed_pass_on_and_off_identical(D):
    k, nq = 10, 300
    sh, _ = _shard(D, N_BIG)
    q = _queries(nq, D, seed=41)
    masks = _masks(N_BIG, k)
    try:
        for name in ("ones", "alternate tiles dead", "uniform 1%", "3 live tiles"):
            allow = masks[name][0].to(DEV)
            mask = sh.make_mask(allow)
            sh.filter_seed = True
            s1, r1 = sh.search(q, k, allow=mask)
            sh.filter_seed = False
            s0, r0 = sh.search(q, k, allow=mask)
            torch.cuda.synchronize()
            assert torch.equal(s0, s1) and torch.equal(r0, r1), name
    finally:
        sh.filter_seed = type(sh).FILTER_SEED_DEFAULT


# 8 ------------------------------------------------------------------------------------------------
def test_row_mask_reused_across_an_append():
    from codename_symbiont_amd.index.shard import HbmIndexShard

    D, n, k, nq = 512, N_SMALL, 10, 30
    sh = HbmIndexShard(D, n + 100, device=DEV, dtype="fp8")
    sh.fill_random(n, seed=7)
    q = _queries(nq, D, seed=8)
    mask = sh.make_mask(torch.ones(n, dtype=torch.bool, device=DEV))
    assert mask.tiles is not None and mask.n_live is not None
    s0, r0 = sh.search(q, k, allow=mask)
    sh.append_unit(q)                                  # the queries themselves: unmasked top-1
    s1, r1 = sh.search(q, k, allow=mask)
    s_all, r_all = sh.search(q, k)
    torch.cuda.synchronize()
    assert torch.equal(r_all[:, 0].long(), torch.arange(n, n + nq, device=DEV))
    assert int(r1.max()) < n
    assert torch.equal(s0, s1) and torch.equal(r0, r1)
    # a mask made now sees them
    s2, r2 = sh.search(q, k, allow=torch.ones(n + nq, dtype=torch.bool, device=DEV))
    assert torch.equal(r2[:, 0].long(), torch.arange(n, n + nq, device=DEV))


# 9 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["0", "1"])
def test_vector_store_fp8_filter_plain_and_pipelined(pipeline, monkeypatch):
    from codename_symbiont_amd.index.filter import Filter
    from codename_symbiont_amd.index.shard import HbmIndexShard, Payload
    from codename_symbiont_amd.index.store import VectorStore

    monkeypatch.setenv("SYMB_SEARCH_PIPELINE", pipeline)
    D, k = 256, 10
    st = VectorStore(D, 4096, device="cuda", dtype="fp8")
    assert (st._streams is not None) == (pipeline == "1")
    took = []
    real = HbmIndexShard._search_filtered
    monkeypatch.setattr(HbmIndexShard, "_search_filtered",
                        lambda self, *a, **kw: (took.append(self.dtype), real(self, *a, **kw))[1])
    sizes = {"doc-a": 5, "doc-b": 40, "doc-c": 300}
    rng = np.random.default_rng(12)
    ids, pls = [], []
    for doc, m in sizes.items():
        for j in range(m):
            ids.append(f"{doc}/{j}")
            pls.append(Payload(doc, f"http://{doc}.example", f"s{j}", j, "m", 0))
    order = rng.permutation(len(ids))                  # documents interleaved over the rows
    ids, pls = [ids[i] for i in order], [pls[i] for i in order]
    st.upsert(ids, rng.standard_normal((len(ids), D)).astype(np.float32), pls)
    q = rng.standard_normal((9, D)).astype(np.float32)
    for doc, m in sizes.items():
        s, r = st.search(q, k, filter=Filter(must={"original_document_id": doc}))
        assert s.shape == (9, k) and r.shape == (9, k)
        for i in range(9):
            fin = np.isfinite(s[i])
            assert int(fin.sum()) == min(k, m) and (r[i][~fin] == -1).all()
            hits = [st.lookup(int(g)) for g in r[i][fin]]
            assert all(p.original_document_id == doc for _, p in hits)
            assert all(pid.startswith(doc + "/") for pid, _ in hits)
            assert len({pid for pid, _ in hits}) == min(k, m)
    s, r = st.search(q, k, filter=Filter(must_not={"original_document_id": ["doc-b", "doc-c"]}))
    assert all(st.lookup(int(g))[1].original_document_id == "doc-a" for g in r[np.isfinite(s)])
    assert int(np.isfinite(s).sum()) == 9 * 5
    assert took == ["fp8"] * 4                         # every search took the masked e4m3 scan


# 10 -----------------------------------------------------------------------------------------------
def test_wrapper_validation_and_routes(monkeypatch):
    from codename_symbiont_amd.index import shard as S
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops import _ext

    assert K.FILTER_FP8_DIMS == S.FILTER_FP8_DIMS == DIMS
    assert hasattr(_ext.hip(), "index_scan_filter_fp8")
    D, n, nq, kmax, n_rblk = 384, N_SMALL, 8, 16, 2
    sh, rows = _shard(D, n)
    q = _queries(nq, D)
    q8 = K.quant_fp8(q)
    words = _words(torch.ones(n, dtype=torch.bool))
    tiles, n_live = K.filter_tiles(words, n)
    cs = torch.empty(nq, n_rblk * 2 * kmax, device=DEV)
    ci = torch.empty(nq, n_rblk * 2 * kmax, dtype=torch.int32, device=DEV)
    launched = []
    real = _ext.hip().index_scan_filter_fp8
    ok = (sh.rows, n, words, tiles, n_live, q8, kmax, n_rblk, cs, ci)

    def bad(**kw):
        a = dict(zip(("rows", "n", "words", "tiles", "n_live", "q", "kmax", "n_rblk", "cs", "ci"), ok))
        a.update(kw)
        return tuple(a.values())

    class Spy:
        def __getattr__(self, name):
            if name == "index_scan_filter_fp8":
                return lambda *a, **kw: launched.append(1) or real(*a, **kw)
            return getattr(_ext.hip(), name)

    spy = Spy()
    monkeypatch.setattr(K, "hip", lambda: spy)
    wide = torch.zeros(n + 100, 320, dtype=torch.uint8, device=DEV)
    for what, args in (
            ("wrong width", bad(rows=wide, q=torch.zeros(nq, 320, dtype=torch.uint8, device=DEV))),
            ("query width", bad(q=torch.zeros(nq, 256, dtype=torch.uint8, device=DEV))),
            ("bf16 rows", bad(rows=torch.zeros(n + 100, D, dtype=torch.bfloat16, device=DEV))),
            ("bf16 queries", bad(q=q)),
            ("short mask", bad(words=words[:-1])),
            ("short tile list", bad(tiles=tiles[:-1])),
            ("short slab", bad(rows=sh.rows[:n])),
            ("small workspace", bad(cs=cs.flatten()[:-1])),
            ("kmax 8", bad(kmax=8)),
            ("stride 0", bad() + (None, 0))):
        with pytest.raises(ValueError):
            K.index_scan_filter_fp8(*args)
        assert not launched, what
    with pytest.raises(ValueError):
        K.index_scan_filter_fp8(*ok, thr_init=torch.zeros(nq - 1, device=DEV))
    assert not launched
    K.index_scan_filter_fp8(*ok)
    torch.cuda.synchronize()
    assert launched == [1]
    monkeypatch.undo()

    # routes: CPU fp8 shards and k > 32 keep the chunked matmul
    calls = []
    real_mm = S.HbmIndexShard._search_matmul
    monkeypatch.setattr(S.HbmIndexShard, "_search_matmul",
                        lambda self, *a, **kw: (calls.append(self.device.type), real_mm(self, *a, **kw))[1])
    cpu = S.HbmIndexShard(D, 600, device="cpu", dtype="fp8")
    cpu.fill_random(500, seed=1)
    allow = torch.from_numpy(np.random.default_rng(2).random(500) < 0.3)
    assert cpu.make_mask(allow).tiles is None
    s, r = cpu.search(q.cpu(), 5, allow=allow)
    assert calls == ["cpu"] and bool(allow[r.long().flatten()].all())
    allow = torch.from_numpy(np.random.default_rng(3).random(n) < 0.5)
    s, r = sh.search(q, 40, allow=allow.to(DEV))
    assert calls == ["cpu", "cuda"]
    # (the matmul scores float(q) . decode(x): the reference takes the queries as they are)
    _check_out(s, r, rows, q, 40, allow, "k = 40 fallback", True)
    s, r = sh.search(q, 32, allow=allow.to(DEV))
    assert calls == ["cpu", "cuda"]
