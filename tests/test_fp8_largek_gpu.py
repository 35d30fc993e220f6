"""The emitting e4m3 scan (csrc/hip/fp8_emit.h) and the searches built on it: top-k for
32 < k <= 128 on a GPU fp8 shard, unmasked, under a row mask or over tombstones, with no chunked
matmul from FP8_LARGE_K_MIN_ROWS visible rows on.

Shapes and masks are those of test_filter_fp8_gpu.py, for its reasons (restated here; that module
is not edited): 64 * 37 + 19 rows (a partial last tile, few workgroups, slices shorter than the
ring) and 20 011 rows (several workgroups, slices longer than the ring).  References are
ops/reference.filtered_topk_ref / row_scores_ref and the same fp32 product over the DECODED rows
and the DECODED e4m3 queries (the MFMA sums exact e4m3 products in fp32).

Kernel-level tests fix the set the kernel must emit from the fp32 reference alone: the threshold
of a query is the midpoint of the largest gap between consecutive sorted reference scores among
ranks [64, 192), asserted to be at least GAP_MIN first.  GAP_MIN = max(1e-4, 4 * LIST_SCAN_ERR),
where LIST_SCAN_ERR is the largest |raw / S^2 - fp32 reference| of the masked e4m3 LIST scan
(fp8_filter_scan.h, which this change does not touch; kmax 32, every candidate slot of 300
queries, an all-ones and a uniform 50 % mask) measured on an MI355X over these very shards, all
five widths, both sizes: 8.70e-6 at D = 256, falling with the width to 2.7e-6 at 1024
(LIST_SCAN_ERR below rounds the largest up).  4 x 8.8e-6 = 3.5e-5 is below 1e-4, so GAP_MIN stays
1e-4 and a threshold clears every score by 5e-5, 5.7 times the measured error.  No row's
membership is ambiguous; set
conditions carry no tolerance.  That the emitting scan scores a row bit for bit as the list scan
does (what lets the search take its threshold from the list scan with no margin) is test 1.
Search-level tolerances are test_filter_fp8_gpu.py::_check_out's (scores atol 2e-3, recall above
0.99 on the random masks, hard conditions without tolerance)."""
import math

import numpy as np
import pytest
import torch

from codename_symbiont_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_SMALL = 64 * 37 + 19
N_BIG = 20_011
N_GATE = (1 << 20) + 999
DIMS = (256, 384, 512, 768, 1024)
K_MASKS = 100               # the "k-1 rows" mask of the kernel-level tests
LIST_SCAN_ERR = 8.8e-6      # measured, see the module docstring
GAP_MIN = max(1e-4, 4 * LIST_SCAN_ERR)
SENT_N, SENT_I, SENT_S = -7, -9, -12345.0

_shards = {}
_refs = {}


def _shard(D, n):
    """One random fp8 shard per (width, rows) for the whole module (rows never written after
    this), with its decoded rows; the small-shard gate of the new route is off on it."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    key = (D, n)
    if key not in _shards:
        sh = HbmIndexShard(D, n + 100, device=DEV, dtype="fp8")
        sh.fill_random(n, seed=5 + D + n)
        sh.FP8_LARGE_K_MIN_ROWS = 0
        _shards[key] = (sh, sh.unit_rows()[:n])
    return _shards[key]


def _queries(nq, D, seed=11):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(nq, D, generator=g), dim=-1).bfloat16().to(DEV)


def _quant(q):
    """(e4m3 bytes the scans take, their decoded values the reference takes)."""
    from codename_symbiont_amd.ops import kernels as K

    q8 = K.quant_fp8(q)
    return q8, K.fp8_to_float(q8)


def _ref_scores(D, n, nq):
    """fp32 scores [nq, n] of the module's decoded queries on the shard's decoded rows: computed
    once per shape, shared, never written."""
    key = (D, n, nq)
    if key not in _refs:
        _refs[key] = _quant(_queries(nq, D))[1] @ _shard(D, n)[1].float().t()
    return _refs[key]


def _tiles_mask(n, tiles):
    a = torch.zeros(n, dtype=torch.bool)
    for t in tiles:
        a[t * 64:(t + 1) * 64] = True
    return a


def _masks(n, k):
    """name -> (bool [n] on the host, random?): the mask set of test_filter_fp8_gpu.py."""
    nt = (n + 63) // 64
    rng = np.random.default_rng(n + k)
    rows = lambda idx: torch.zeros(n, dtype=torch.bool).index_fill_(0, torch.as_tensor(idx), True)
    per_tile = [t * 64 + (t * 7) % 64 for t in range(nt)]
    return {
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


def _close(out, ref, atol, what):
    err = (out.float() - ref.float()).abs()
    bad = int((err > atol).sum())
    assert bad == 0, f"{what}: {bad} elems off, max err {float(err.max()):.4g}"


def _check_out(s, r, rows, qd, k, allow, what, random_mask=False):
    """(scores, rows) of one search against the reference over the decoded rows [n, D] and
    decoded queries; ``allow``: bool [n] on the host (test_filter_fp8_gpu.py::_check_out)."""
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


def _same(sh, q, s, r, ref_s, ref_r, what):
    """Two searches that must agree: scores bit for bit; rows equal except inside runs of equal
    scores (the emitting scan hands its slots out by atomics, and exact ties are common among
    sums of e4m3 products).  A run can go on past k, where no equal neighbour shows it, so a
    LAST slot whose rows differ without an equal neighbour must be proved a tie: the two rows,
    searched alone under a two-row mask (k = 2: the list scan, the same per-row MFMA chain),
    score the same bit for bit, which is the slot's score."""
    assert torch.equal(s, ref_s), f"{what}: scores differ"
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


def _bar_matmul(monkeypatch):
    """No search of the test may take the chunked matmul."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    def barred(self, *a, **kw):
        raise AssertionError("the search took the chunked matmul")

    monkeypatch.setattr(HbmIndexShard, "_search_matmul", barred)


def _count_matmul(monkeypatch):
    """-> list that collects the (queries, mask) of every chunked matmul."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    calls = []
    real = HbmIndexShard._search_matmul

    def spy(self, q_unit, k, *a, **kw):
        calls.append((q_unit, kw.get("mask")))
        return real(self, q_unit, k, *a, **kw)

    monkeypatch.setattr(HbmIndexShard, "_search_matmul", spy)
    return calls


def _gap_threshold(masked_sc, lo, hi, what):
    """Per query: the midpoint of the largest gap between consecutive sorted scores among ranks
    [lo, hi) of ``masked_sc`` [nq, n] (-inf = disallowed), in raw units; the gap is asserted
    first."""
    from codename_symbiont_amd.ops.kernels import FP8_SCALE

    top = torch.topk(masked_sc, hi, dim=1).values
    assert bool(torch.isfinite(top).all()), what
    gaps = top[:, lo:hi - 1] - top[:, lo + 1:hi]
    g, j = gaps.max(1)
    assert float(g.min()) >= GAP_MIN, f"{what}: reference gap {float(g.min()):.3g} below {GAP_MIN}"
    a = torch.gather(top, 1, (lo + j)[:, None])[:, 0]
    b = torch.gather(top, 1, (lo + j + 1)[:, None])[:, 0]
    return ((a + b) * 0.5 * (FP8_SCALE * FP8_SCALE)).contiguous()


def _emit(sh, n, allow, q8, thr, cap, n_rblk, gate=None, bufs=None, zero_cnt=True):
    """filter_tiles + index_scan_emit_fp8 through the wrappers -> (cand_s, cand_i [nq * cap + 64]
    and cand_n [nq + 64], each with a 64-entry sentinel guard at its end)."""
    from codename_symbiont_amd.ops import kernels as K

    nq = q8.shape[0]
    mask = sh.make_mask(allow.to(DEV))
    if bufs is None:
        bufs = (torch.full((nq * cap + 64,), SENT_S, device=DEV),
                torch.full((nq * cap + 64,), SENT_I, dtype=torch.int32, device=DEV),
                torch.full((nq + 64,), SENT_N, dtype=torch.int32, device=DEV))
    cs, ci, cn = bufs
    K.index_scan_emit_fp8(sh.rows, n, mask.words, mask.tiles, mask.n_live, q8, thr,
                          cs[:nq * cap], ci[:nq * cap], cn[:nq], cap, n_rblk, 1, gate, zero_cnt)
    torch.cuda.synchronize()
    return cs, ci, cn


def _emitted_matrix(ci, cn, nq, n, cap, what):
    """bool [nq, n]: row emitted for the query, and the valid-slot matrix [nq, cap]; asserts ids
    in range (below ``visible``) and no row twice."""
    cnt = cn[:nq].long()
    valid = torch.arange(cap, device=DEV)[None, :] < cnt[:, None]
    ids = ci[:nq * cap].view(nq, cap).long()
    assert bool(((ids >= 0) & (ids < n))[valid].all()), f"{what}: a row id outside [0, n_valid)"
    times = torch.zeros(nq, n, dtype=torch.int32, device=DEV)
    times.scatter_add_(1, ids.clamp(0, n - 1), valid.to(torch.int32))
    assert int(times.max()) <= 1, f"{what}: a row was emitted twice"
    return times > 0, valid


def _check_emitted(sh, n, allow, q8, sc, thr, n_rblk, what, cap=None):
    """One launch against the reference set {allowed rows with reference score above thr}."""
    from codename_symbiont_amd.ops.kernels import FP8_SCALE

    nq = q8.shape[0]
    allow_d = allow.to(DEV)
    msc = torch.where(allow_d[None, :], sc, torch.full_like(sc, -math.inf))
    want = msc * (FP8_SCALE * FP8_SCALE) > thr[:, None]
    cap = cap or max(512, int(want.sum(1).max()))
    cs, ci, cn = _emit(sh, n, allow, q8, thr, cap, n_rblk)
    assert torch.equal(cn[:nq].long(), want.sum(1)), f"{what}: cand_n"
    # queries past NQ in the padded block emitted nothing; nothing past the buffers' ends
    assert bool((cn[nq:] == SENT_N).all()), f"{what}: counters past NQ written"
    assert bool((cs[nq * cap:] == SENT_S).all()) and bool((ci[nq * cap:] == SENT_I).all()), what
    got, valid = _emitted_matrix(ci, cn, nq, n, cap, what)
    assert not bool((got & ~allow_d[None, :]).any()), f"{what}: a disallowed row"
    assert torch.equal(got, want), f"{what}: not the reference set"
    ids = ci[:nq * cap].view(nq, cap).long()
    true = torch.gather(sc, 1, ids.clamp(0, n - 1))
    raw = cs[:nq * cap].view(nq, cap) * (1.0 / (FP8_SCALE * FP8_SCALE))
    # (half the gap: the clearance the thresholds above rely on)
    _close(raw[valid], true[valid], GAP_MIN / 2, f"{what}: emitted scores")
    assert bool((cs[:nq * cap].view(nq, cap)[~valid] == SENT_S).all()), what
    assert bool((ci[:nq * cap].view(nq, cap)[~valid] == SENT_I).all()), what


def _thr_for(allow, sc, nq, what):
    """The gap threshold, or -inf for a mask with too few allowed rows to have ranks [64, 192)."""
    if int(allow.sum()) <= 256:
        return torch.full((nq,), -math.inf, device=DEV)
    msc = torch.where(allow.to(DEV)[None, :], sc, torch.full_like(sc, -math.inf))
    return _gap_threshold(msc, 64, 192, what)


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_same_row_same_score(D):
    """thr = -inf and cap >= n: the emitted (row, raw score) set of a query is the allowed rows,
    each once, and the raw scores of the query's top 32 rows are the list scan's, bit for bit."""
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import hip, stream_handle

    n, nq, cap, n_rblk, kmax = N_SMALL, 70, 2560, 3, 32
    sh, _ = _shard(D, n)
    q8, _ = _quant(_queries(nq, D, seed=21))
    thr = torch.full((nq,), -math.inf, device=DEV)
    for name in ("ones", "uniform 50%"):
        allow = _masks(n, K_MASKS)[name][0]
        n_allowed = int(allow.sum())
        cs, ci, cn = _emit(sh, n, allow, q8, thr, cap, n_rblk)
        assert bool((cn[:nq] == n_allowed).all()), f"D={D} {name}: cand_n"
        ids = ci[:nq * cap].view(nq, cap)[:, :n_allowed].long()
        order = torch.argsort(ids, 1)
        want = torch.nonzero(allow.to(DEV)).flatten()
        assert torch.equal(torch.gather(ids, 1, order), want.expand(nq, -1)), \
            f"D={D} {name}: not the allowed rows, each once"
        dense = torch.full((nq, n), math.nan, device=DEV)
        dense.scatter_(1, ids, cs[:nq * cap].view(nq, cap)[:, :n_allowed])
        # the list scan's top 32 of the same mask, raw
        mask = sh.make_mask(allow.to(DEV))
        ls = torch.empty(nq, n_rblk * 2 * kmax, device=DEV)
        li = torch.empty(nq, n_rblk * 2 * kmax, dtype=torch.int32, device=DEV)
        K.index_scan_filter_fp8(sh.rows, n, mask.words, mask.tiles, mask.n_live, q8, kmax, n_rblk,
                                ls, li)
        top_s = torch.empty(nq, kmax, device=DEV)
        top_i = torch.empty(nq, kmax, dtype=torch.int32, device=DEV)
        hip().topk_merge(ls.data_ptr(), li.data_ptr(), nq, ls.shape[1], kmax, kmax,
                         top_s.data_ptr(), top_i.data_ptr(), 0, 0, stream_handle(sh.device), 0)
        torch.cuda.synchronize()
        assert int(top_i.min()) >= 0
        assert torch.equal(torch.gather(dense, 1, top_i.long()), top_s), \
            f"D={D} {name}: a row scores differently in the two kernels"


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,nq", [(D, nq) for D in DIMS for nq in (1, 130, 300)])
def test_emitted_set_is_the_reference_set(D, nq):
    q8, _ = _quant(_queries(nq, D))
    for n, n_rblk in ((N_SMALL, 5), (N_BIG, 7)):
        sh, _ = _shard(D, n)
        sc = _ref_scores(D, n, nq)
        for name, (allow, _) in _masks(n, K_MASKS).items():
            what = f"D={D} nq={nq} n={n} {name}"
            _check_emitted(sh, n, allow, q8, sc, _thr_for(allow, sc, nq, what), n_rblk, what)


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_slices_around_the_ring_depth(D):
    """Masks whose live tiles number 1, NS - 1, NS, NS + 1 and 2 NS + 1 per workgroup, over 1, 2
    and 3 workgroups (the last slice one tile short where the shard has no more tiles): slices
    shorter than the ring, as long as it and longer -- the prologue's NS list reads, the clamped
    re-loads and the tail prefetches."""
    from codename_symbiont_amd.ops._ext import hip

    n, nq = N_SMALL, 70
    nt = (n + 63) // 64
    sh, _ = _shard(D, n)
    q8, _ = _quant(_queries(nq, D))
    sc = _ref_scores(D, n, nq)
    rng = np.random.default_rng(D)
    ns = hip().filter_fp8_ring_depth(D)
    assert 2 <= ns <= 8
    for per in sorted({1, ns - 1, ns, ns + 1, 2 * ns + 1}):
        for n_rblk in (1, 2, 3):
            m = min(per * n_rblk, nt)
            assert -(-m // n_rblk) == per
            live = sorted({int(round(t)) for t in np.linspace(0, nt - 1, m)})
            assert len(live) == m
            allow = torch.zeros(n, dtype=torch.bool)
            for t in live:                        # a random half of each live tile, never empty
                lo, hi = t * 64, min(n, t * 64 + 64)
                allow[lo:hi] = torch.from_numpy(rng.random(hi - lo) < 0.5)
                allow[lo] = True
            what = f"D={D} per={per} n_rblk={n_rblk}"
            _check_emitted(sh, n, allow, q8, sc, _thr_for(allow, sc, nq, what), n_rblk, what)


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,nq", [(256, 70), (768, 130), (1024, 20)])
def test_overflow_is_counted_never_written(D, nq):
    """cap = 64 under thr = -inf: every query overflows.  A slot written at or past cap would
    land in the next query's slots or in the guard, so every slot below cap must hold an allowed
    row with the score THIS query gives it (from a launch whose cap holds every row)."""
    n, cap, big = N_SMALL, 64, 2560
    sh, _ = _shard(D, n)
    q8, _ = _quant(_queries(nq, D, seed=31))
    thr = torch.full((nq,), -math.inf, device=DEV)
    for name in ("ones", "uniform 50%"):
        what = f"D={D} nq={nq} {name}"
        allow = _masks(n, K_MASKS)[name][0]
        allow_d, n_allowed = allow.to(DEV), int(allow.sum())
        fs, fi, fn = _emit(sh, n, allow, q8, thr, big, 5)
        dense = torch.full((nq, n), math.nan, device=DEV)
        dense.scatter_(1, fi[:nq * big].view(nq, big)[:, :n_allowed].long(),
                       fs[:nq * big].view(nq, big)[:, :n_allowed])
        bufs = _emit(sh, n, allow, q8, thr, cap, 5)
        for rep, zero_cnt in ((1, True), (2, False)):      # zero_cnt = False appends
            if rep == 2:
                bufs = _emit(sh, n, allow, q8, thr, cap, 5, bufs=bufs, zero_cnt=False)
            cs, ci, cn = bufs
            assert bool((cn[:nq] == rep * n_allowed).all()), f"{what}: cand_n is not the count"
            assert bool((cn[nq:] == SENT_N).all()), f"{what}: counters past NQ written"
            assert bool((cs[nq * cap:] == SENT_S).all()) and bool((ci[nq * cap:] == SENT_I).all()), \
                f"{what}: written past the buffers"
            ids = ci[:nq * cap].view(nq, cap).long()
            assert bool(((ids >= 0) & (ids < n)).all()), what
            assert bool(allow_d[ids].all()), f"{what}: a slot holds a disallowed row"
            srt = torch.sort(ids, 1).values
            assert bool((srt[:, 1:] != srt[:, :-1]).all()), f"{what}: a row twice"
            assert torch.equal(cs[:nq * cap].view(nq, cap), torch.gather(dense, 1, ids)), \
                f"{what}: a slot holds another query's score"


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_gate(D):
    n, nq, cap = N_SMALL, 40, 512
    sh, _ = _shard(D, n)
    q8, _ = _quant(_queries(nq, D))
    sc = _ref_scores(D, n, nq)
    allow = _masks(n, K_MASKS)["uniform 50%"][0]
    thr = _thr_for(allow, sc, nq, f"D={D}")
    cs0, ci0, cn0 = _emit(sh, n, allow, q8, thr, cap, 5)
    shut = torch.zeros(1, dtype=torch.int32, device=DEV)
    cs, ci, cn = _emit(sh, n, allow, q8, thr, cap, 5, gate=shut)
    assert bool((cn == SENT_N).all()) and bool((cs == SENT_S).all()) and bool((ci == SENT_I).all())
    cs, ci, cn = _emit(sh, n, allow, q8, thr, cap, 5, gate=shut + 1, bufs=(cs, ci, cn))
    assert torch.equal(cn, cn0)
    # (slots are handed out by atomics: compare each query's candidates as sorted sets)
    v = lambda t: t[:nq * cap].view(nq, cap)
    o0, o = torch.argsort(v(ci0).long(), 1), torch.argsort(v(ci).long(), 1)
    assert torch.equal(torch.gather(v(ci0), 1, o0), torch.gather(v(ci), 1, o))
    assert torch.equal(torch.gather(v(cs0), 1, o0), torch.gather(v(cs), 1, o))


# 6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,k,nq", [(D, k, nq) for D in DIMS
                                    for k, nq in ((33, 1), (100, 300), (128, 130))])
def test_search_large_k_masks_and_unmasked(D, k, nq, monkeypatch):
    _bar_matmul(monkeypatch)
    q = _queries(nq, D)
    _, qd = _quant(q)
    for n in (N_SMALL, N_BIG):
        sh, rows = _shard(D, n)
        for name, (allow, rnd) in _masks(n, k).items():
            what = f"D={D} n={n} k={k} nq={nq} {name}"
            s, r = sh.search(q, k, allow=allow.to(DEV))
            _check_out(s, r, rows, qd, k, allow, what, rnd)
            assert int(sh._filter_large_k_last[1]) == 0, what
        s, r = sh.search(q, k)
        _check_out(s, r, rows, qd, k, torch.ones(n, dtype=torch.bool), f"D={D} n={n} k={k} unmasked")
        assert int(sh._filter_large_k_last[1]) == 0


@pytest.mark.parametrize("D", DIMS)
def test_seed_on_equals_seed_off(D):
    """T from the seed pass against T = -inf, where the cap holds every row."""
    k, nq, n = 100, 130, N_SMALL
    sh, _ = _shard(D, n)
    q = _queries(nq, D, seed=41)
    assert sh.LARGE_K_CAP >= n
    for name in ("ones", "alternate tiles dead", "uniform 50%", "7 live tiles"):
        mask = sh.make_mask(_masks(n, k)[name][0].to(DEV))
        s1, r1 = sh._search_filtered_large_k(q, k, mask, None, seed=True)
        s0, r0 = sh._search_filtered_large_k(q, k, mask, None, seed=False)
        torch.cuda.synchronize()
        _same(sh, q, s1, r1, s0, r0, f"D={D} {name}")


@pytest.mark.parametrize("D", [384, 1024])
def test_unmasked_equals_all_ones_mask(D, monkeypatch):
    _bar_matmul(monkeypatch)
    k, nq, n = 100, 300, N_BIG
    sh, _ = _shard(D, n)
    q = _queries(nq, D, seed=61)
    s_all, r_all = sh.search(q, k)
    s, r = sh.search(q, k, allow=torch.ones(n, dtype=torch.bool, device=DEV))
    torch.cuda.synchronize()
    _same(sh, q, s, r, s_all, r_all, f"D={D}")
    # the internal mask is make_mask's, and is built once per number of visible rows
    assert torch.equal(sh._all_rows().bits, sh.make_mask(torch.ones(n, dtype=torch.bool)).bits)
    assert sh._all_rows() is sh._all_rows()


# 7 ------------------------------------------------------------------------------------------------
def test_overflow_falls_back_on_the_decoded_queries(monkeypatch):
    from codename_symbiont_amd.index.shard import HbmIndexShard

    D, n, k, nq = 384, N_BIG, 100, 20
    sh = HbmIndexShard(D, n + 100, device=DEV, dtype="fp8")
    sh.fill_random(n, seed=61)
    sh.FP8_LARGE_K_MIN_ROWS, sh.LARGE_K_CAP = 0, 64
    q = _queries(nq, D, seed=62)
    _, qd = _quant(q)
    rows = sh.unit_rows()[:n]
    allow = torch.from_numpy(np.random.default_rng(7).random(n) < 0.3)
    calls = _count_matmul(monkeypatch)
    s, r = sh.search(q, k, allow=allow.to(DEV))
    _check_out(s, r, rows, qd, k, allow, "overflow", True)
    cnt, ovf = sh._filter_large_k_last
    assert int(ovf) == 1 and int(cnt.max()) > 64
    assert len(calls) == 1 and calls[0][1] is not None
    assert calls[0][0].dtype == torch.float32 and torch.equal(calls[0][0], qd)
    # the unmasked search overflows the same way, under the all-ones mask
    s, r = sh.search(q, k)
    _check_out(s, r, rows, qd, k, torch.ones(n, dtype=torch.bool), "overflow, unmasked")
    assert len(calls) == 2 and calls[1][1] is sh._all_rows() and torch.equal(calls[1][0], qd)


# 8 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [256, 768])
def test_tombstones_large_k(D, monkeypatch):
    from codename_symbiont_amd.index.shard import HbmIndexShard

    n, k, nq = N_BIG, 100, 130
    sh = HbmIndexShard(D, n + 100, device=DEV, dtype="fp8")
    sh.fill_random(n, seed=71 + D)
    sh.FP8_LARGE_K_MIN_ROWS = 0
    assert sh.delete_route == "mask"                   # the fp8 default
    q = _queries(nq, D, seed=72)
    _, qd = _quant(q)
    rows = sh.unit_rows()[:n].clone()
    dead = torch.from_numpy(np.random.default_rng(8).random(n) < 0.1)
    dead[64 * 100:64 * 105] = True                     # a run of whole tiles
    best = R.filtered_topk_ref(rows, qd, 5, torch.ones(n, dtype=torch.bool, device=DEV))[1]
    dead[best.flatten().cpu()] = True                  # and every query's five best rows
    sh.delete_rows(torch.nonzero(dead).flatten())
    live = ~dead
    _bar_matmul(monkeypatch)
    for route in ("zero", "mask"):
        sh.delete_route = route
        s, r = sh.search(q, k)
        what = f"D={D} {route}"
        _check_out(s, r, rows, qd, k, live, what, True)
        assert not bool(dead.to(DEV)[r.long().clamp_min(0)].any()), f"{what}: a dead row"
        assert isinstance(sh.last_dead_hits, torch.Tensor) and sh.last_dead_hits.is_cuda
        assert int(sh.last_dead_hits) == 0, what       # a zeroed row scores 0, below the k-th
    monkeypatch.undo()
    # few live rows: fewer than k score above 0, so the unmasked route returns zeroed rows (all of
    # them pass its threshold and overflow the cap: the one matmul here is the ROUTE's), the
    # dead-id check hits and the gated masked search supplies the answer
    sh.delete_route = "zero"
    keep = torch.from_numpy(np.random.default_rng(9).choice(n, 60, replace=False))
    live2 = torch.zeros(n, dtype=torch.bool)
    live2[keep] = True
    live2 &= live
    sh.delete_rows(torch.nonzero(~live2 & live).flatten())
    calls = _count_matmul(monkeypatch)
    s, r = sh.search(q, k)
    _check_out(s, r, rows, qd, k, live2, f"D={D} zero, few live rows")
    assert int(sh.last_dead_hits) > 0
    assert len(calls) <= 1 and all(m is sh._all_rows() for _, m in calls)
    assert int(sh._filter_large_k_last[1]) == 0        # the fallback itself did not overflow


# 9 ------------------------------------------------------------------------------------------------
def test_the_default_gate(monkeypatch):
    """Untouched attributes: a shard of 2^20 + 999 rows takes the emitting scan at k = 100,
    unmasked, masked and after a delete; one of 20 011 rows keeps the chunked matmul."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    D, k, nq = 256, 100, 8
    q = _queries(nq, D, seed=81)
    _, qd = _quant(q)
    assert HbmIndexShard.FP8_LARGE_K_MIN_ROWS == HbmIndexShard.SEED_MIN_ROWS == 1 << 20

    def three_calls(sh, n, qref):
        rows = sh.unit_rows()[:n].clone()
        ones = torch.ones(n, dtype=torch.bool)
        half = torch.from_numpy(np.random.default_rng(n).random(n) < 0.5)
        out = [(sh.search(q, k), ones, "unmasked"),
               (sh.search(q, k, allow=half.to(DEV)), half, "uniform 50%")]
        gone = int(out[0][0][1][0, 0])                 # query 0's best row
        assert sh.delete_rows([gone]) == 1
        live = ones.clone()
        live[gone] = False
        out.append((sh.search(q, k), live, "after a delete"))
        for (s, r), allow, what in out:
            _check_out(s, r, rows, qref, k, allow, f"n={n} {what}", what == "uniform 50%")
        assert gone not in out[2][0][1][0].tolist()

    big = HbmIndexShard(D, N_GATE + 100, device=DEV, dtype="fp8")
    big.fill_random(N_GATE, seed=82)
    assert "FP8_LARGE_K_MIN_ROWS" not in big.__dict__ and big._filter_large_k_serves(k)
    _bar_matmul(monkeypatch)
    three_calls(big, N_GATE, qd)
    assert int(big._filter_large_k_last[1]) == 0
    monkeypatch.undo()
    del big
    small = HbmIndexShard(D, N_BIG + 100, device=DEV, dtype="fp8")
    small.fill_random(N_BIG, seed=83)
    assert not small._filter_large_k_serves(k)
    calls = _count_matmul(monkeypatch)
    # (the matmul scores float(q) . decode(x): the reference takes the queries as they are)
    three_calls(small, N_BIG, q)
    assert len(calls) == 3 and [m is None for _, m in calls] == [True, False, False]


# 10 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["0", "1"])
def test_vector_store_fp8_large_k_filter_and_delete(pipeline, monkeypatch):
    from codename_symbiont_amd.index.filter import Filter
    from codename_symbiont_amd.index.shard import Payload
    from codename_symbiont_amd.index.store import VectorStore

    monkeypatch.setenv("SYMB_SEARCH_PIPELINE", pipeline)
    _bar_matmul(monkeypatch)
    D, k = 256, 100
    sizes = {"doc-a": 5, "doc-b": 40, "doc-c": 300}
    st = VectorStore(D, N_GATE + 100, device="cuda", dtype="fp8")
    assert (st._streams is not None) == (pipeline == "1")
    st.shard.fill_random(N_GATE - sum(sizes.values()), seed=91)     # rows without payloads
    rng = np.random.default_rng(12)
    ids, pls = [], []
    for doc, m in sizes.items():
        for j in range(m):
            ids.append(f"{doc}/{j}")
            pls.append(Payload(doc, f"http://{doc}.example", f"s{j}", j, "m", 0))
    order = rng.permutation(len(ids))
    ids, pls = [ids[i] for i in order], [pls[i] for i in order]
    st.upsert(ids, rng.standard_normal((len(ids), D)).astype(np.float32), pls)
    assert st.shard.visible == N_GATE and "FP8_LARGE_K_MIN_ROWS" not in st.shard.__dict__
    q = rng.standard_normal((9, D)).astype(np.float32)
    gone = set()

    def look(doc, m):
        s, r = st.search(q, k, filter=Filter(must={"original_document_id": doc}))
        assert s.shape == (9, k) and r.shape == (9, k)
        for i in range(9):
            fin = np.isfinite(s[i])
            assert int(fin.sum()) == min(k, m) and (r[i][~fin] == -1).all()
            hits = [st.lookup(int(g)) for g in r[i][fin]]
            assert all(p.original_document_id == doc for _, p in hits)
            assert not any(pid in gone for pid, _ in hits)
            assert len({pid for pid, _ in hits}) == min(k, m)

    for doc, m in sizes.items():
        look(doc, m)
    gone = {f"doc-c/{j}" for j in range(0, 300, 3)}
    gone_rows = {st.shard.payloads.id_to_row[p] for p in gone}
    gone_rows |= {st.shard.payloads.id_to_row[f"doc-a/{j}"] for j in range(5)}
    assert st.delete(point_ids=sorted(gone)) == 100
    assert st.delete(filter=Filter(must={"original_document_id": "doc-a"})) == 5
    look("doc-c", 200)
    look("doc-b", 40)
    look("doc-a", 0)
    # an unfiltered search over the tombstones at this k returns live rows only
    s, r = st.search(q, k)
    fin = np.isfinite(s)
    assert int(fin.sum()) == 9 * k
    assert not any(int(g) in gone_rows for g in r[fin])
    assert int(st.shard._filter_large_k_last[1]) == 0


# 11 -----------------------------------------------------------------------------------------------
def test_wrapper_validation(monkeypatch):
    """Every refusal is a ValueError raised before any launch."""
    from codename_symbiont_amd.index import shard as S
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops import _ext

    assert S.FILTER_LARGE_K_FP8_DIMS == K.FILTER_FP8_DIMS == DIMS
    D, n, nq, cap = 384, N_SMALL, 20, 64
    sh, _ = _shard(D, n)
    q = _queries(nq, D)
    q8, _ = _quant(q)
    mask = sh.make_mask(torch.ones(n, dtype=torch.bool, device=DEV))
    thr = torch.full((nq,), math.inf, device=DEV)
    cs = torch.empty(nq, cap, device=DEV)
    ci = torch.empty(nq, cap, dtype=torch.int32, device=DEV)
    cn = torch.full((nq,), SENT_N, dtype=torch.int32, device=DEV)
    launched = []
    real = _ext.hip().index_scan_emit_fp8

    class Spy:
        def __getattr__(self, name):
            if name == "index_scan_emit_fp8":
                return lambda *a, **kw: launched.append(1) or real(*a, **kw)
            return getattr(_ext.hip(), name)

    spy = Spy()
    monkeypatch.setattr(K, "hip", lambda: spy)

    def call(**kw):
        a = dict(rows_u8=sh.rows, n_valid=n, mask_words=mask.words, tiles=mask.tiles,
                 n_live=mask.n_live, q_e4m3=q8, thr=thr, cand_s=cs, cand_i=ci, cand_n=cn, cap=cap,
                 n_rblk=5)
        a.update(kw)
        K.index_scan_emit_fp8(**a)

    wide = torch.zeros(n + 100, 320, dtype=torch.uint8, device=DEV)
    for what, kw in (
            ("width", dict(rows_u8=wide, q_e4m3=torch.zeros(nq, 320, dtype=torch.uint8, device=DEV))),
            ("query width", dict(q_e4m3=torch.zeros(nq, 256, dtype=torch.uint8, device=DEV))),
            ("bf16 rows", dict(rows_u8=torch.zeros(n + 100, D, dtype=torch.bfloat16, device=DEV))),
            ("bf16 queries", dict(q_e4m3=q)),
            ("short slab", dict(rows_u8=sh.rows[:n])),
            ("short mask", dict(mask_words=mask.words[:-1])),
            ("short tile list", dict(tiles=mask.tiles[:-1])),
            ("thr shorter than the batch", dict(thr=thr[:-1])),
            ("thr longer than the batch", dict(thr=torch.cat([thr, thr]))),
            ("thr f64", dict(thr=thr.double())),
            ("thr missing", dict(thr=None)),
            ("cand_n shorter than the batch", dict(cand_n=cn[:-1])),
            ("workspace", dict(cand_s=cs.flatten()[:-1])),
            ("workspace ids", dict(cand_i=ci.flatten()[:-1])),
            ("cap", dict(cap=0)),
            ("n_rblk", dict(n_rblk=0)),
            ("n_valid", dict(n_valid=-1))):
        with pytest.raises(ValueError):
            call(**kw)
        assert not launched, what
    torch.cuda.synchronize()
    assert bool((cn == SENT_N).all())
    call()                                             # thr = +inf: runs, emits nothing
    torch.cuda.synchronize()
    assert launched == [1] and not bool(cn.any())
