"""The split-phase pruned search with its short tail switched on (index/shard.py _pruned_begin /
_pruned_end, ``route_at_begin`` and ``prune_fused_finish``): the begin half enqueues the
candidate prefill and the bf16 scan of the routed blocks, the end half runs the gated stream
scans and one finishing launch (prune_finish.hip).  Both switches are off by default (no
measured gain on the headline); every other end-to-end search test runs the default path.

search_begin / search_end must return what search() returns and what the fp32 oracle says, on
shards whose last 32-row sub-tile is partly filled (the prefill runs) and whose fresh-row tail
holds a crowd of near-duplicates (the route lists its block: the bf16 scan runs), with rows
appended and rows tombstoned between the halves, with and without a CU reserve; the tier hint
still follows the tier the last finished search took; and search_end launches none of the
kernels that moved or were fused.

Scores are fp32 dot products of 384 bf16 products of unit vectors: two summation orders differ by
at most 384 * 2^-24 = 2.3e-5 and in practice by ~1e-6, so the oracle is met within 2e-5, as in
the other end-to-end search tests; an id may differ from the oracle's only where its own exact
score ties the oracle's at that rank.
"""
import math

import pytest
import torch

from codename_symbiont_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 384
CROWD = 3000   # > PRUNE_CAP * PRUNE_BLOCK_FRAC = 1024 rows no int8 bound separates, in the tail
ATOL = 2e-5


def _unit(x):
    return torch.nn.functional.normalize(x, dim=-1)


def _near(c, m, e, g):
    return _unit(c + e * torch.randn(m, D, device=DEV, generator=g) / math.sqrt(D))


def _shard(n, seed):
    """n - CROWD random rows, then the crowd (the fresh-row tail, which the route counts row by
    row); the sampled search's row-count gates lowered on the instance."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    g = torch.Generator(device=DEV).manual_seed(seed)
    sh = HbmIndexShard(D, n + 1024, prune="i8")
    c = _unit(torch.randn(D, device=DEV, generator=g))
    sh.append_f32(torch.randn(n - CROWD, D, device=DEV, generator=g))
    sh.append_f32(_near(c, CROWD, 0.1, g))
    sh.SEED_MIN_ROWS = 0
    sh.PRUNE_MIN_SHIFT = 0
    sh.prune_fused_finish = sh.route_at_begin = True
    assert sh.visible == n and n % 32 != 0
    return sh, c, g


def _check(s, r, rows, q, k, what):
    """(s, r) against the fp32 oracle over ``rows`` (f32 [n, D])."""
    torch.cuda.synchronize()
    s0, r0 = R.topk_ref(rows, q, k)
    err = float((s - s0).abs().max())
    assert err <= ATOL, f"{what}: scores off the oracle by {err:.3g}"
    tie = (R.row_scores_ref(rows, q, r) - s0).abs() <= ATOL
    bad = (r.long() != r0) & ~tie
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} ids differ from the oracle"
    srt = torch.sort(r.long(), dim=1).values
    assert not bool((srt[:, 1:] == srt[:, :-1]).any()), f"{what}: a row returned twice"


def _listed(sh):
    blk = sh._route_blk_last
    return int(blk[0].item()), int(blk[1].item())


class _Calls:
    """Counts the extension's launches by name while it is active (the bindings wrapped)."""

    NAMES = ("rescore_bf16", "topk_select_counted", "index_scan_mq", "prefill_candidates",
             "prune_finish", "index_scan_stream")

    def __init__(self, monkeypatch):
        from codename_symbiont_amd.ops._ext import hip

        self.n = {}
        self.on = False
        h = hip()
        for name in self.NAMES:
            monkeypatch.setattr(h, name, self._wrap(name, getattr(h, name)))

    def _wrap(self, name, fn):
        def call(*a, **kw):
            if self.on:
                key = name + ("_routed" if name == "index_scan_mq" and kw.get("blist") else "")
                self.n[key] = self.n.get(key, 0) + 1
            return fn(*a, **kw)
        return call

    def during(self, f):
        self.n, self.on = {}, True
        try:
            return f()
        finally:
            self.on = False


@pytest.mark.parametrize("n", [20_011, 70_013])
@pytest.mark.parametrize("reserve", [0, 64])
def test_split_search_matches_search_and_the_oracle(n, reserve, monkeypatch):
    k, nq = 10, 256
    sh, c, g = _shard(n, seed=n)
    sh.scan_reserve = reserve
    rows = sh.unit_rows().float()[:n]
    qs = {"near": _near(c, nq, 0.1, g).bfloat16(),
          "heldout": _unit(torch.randn(nq, D, device=DEV, generator=g)).bfloat16()}
    calls = _Calls(monkeypatch)

    plain = {}
    for kind, q in qs.items():
        plain[kind] = sh.search(q, k)
        _check(*plain[kind], rows, q, k, f"n={n} plain {kind}")
        if kind == "near":
            listed, n_rblk = _listed(sh)
            assert 1 <= listed < n_rblk, f"the route lists the crowd's block: {listed} of {n_rblk}"
    # (the last finished search took the int8 tier: the hint says int8)

    def split(kind, hint_mx4):
        what = f"n={n} reserve={reserve} {kind} hint_mx4={hint_mx4}"
        ctx = calls.during(lambda: sh.search_begin(qs[kind], k))
        assert "full" not in ctx and ctx["hint_mx4"] == hint_mx4, what
        assert ctx["wide"] == (hint_mx4 and reserve > 0), what
        begin = calls.n
        assert "cand" in ctx and begin.get("prefill_candidates") == 1, (what, begin)
        assert begin.get("index_scan_mq_routed") == 1, (what, begin)
        s, r = calls.during(lambda: sh.search_end(ctx))
        end = calls.n
        for name in ("rescore_bf16", "topk_select_counted", "index_scan_mq_routed",
                     "prefill_candidates"):
            assert name not in end, f"{what}: search_end launched {name}: {end}"
        assert end.get("prune_finish") == 1 and end.get("index_scan_stream") == 2, (what, end)
        _check(s, r, rows, qs[kind], k, what)
        assert torch.equal(s, plain[kind][0]), f"{what}: scores differ from search()"
        assert (int(sh._mx4_last.item()) == 0) == (kind == "near"), what
        if kind == "near":
            assert _listed(sh)[0] >= 1, what

    split("near", False)      # after an int8 search: the hint says int8; the fp4 tier runs
    split("near", True)       # ... and has flipped: the case the reserve is for
    split("heldout", True)    # a wrong hint: the int8 tier on the reserve's grid
    split("heldout", False)   # flipped back
    split("near", False)


@pytest.mark.parametrize("reserve", [0, 64])
def test_split_search_with_an_append_between_the_halves(reserve):
    """Rows appended after begin land in the partly filled sub-tile the prefill listed (and raise
    its shared int8 scale); the search returns the top-k of the rows begin saw."""
    n, k, nq = 20_011, 10, 256
    sh, c, g = _shard(n, seed=3)
    sh.scan_reserve = reserve
    rows = sh.unit_rows().float()[:n]
    q = torch.cat([sh.rows[n - 11:n].clone(), _near(c, nq - 11, 0.1, g).bfloat16()])
    sh.search(q, k)           # leaves the fp4 hint
    torch.cuda.synchronize()
    spike = torch.zeros(13, D, device=DEV)
    spike[torch.arange(13), torch.arange(13) * 5] = 1.0
    spike = _unit(spike + 0.01 * torch.randn(13, D, device=DEV, generator=g)).bfloat16()
    ctx = sh.search_begin(q, k)
    assert "full" not in ctx and ctx["n"] == n and ctx["hint_mx4"] and "cand" in ctx
    sh.append_unit(spike)     # rewrites sub-tile n >> 5 in place
    sh.append_unit(q[:40])    # ... and exact copies of queries, past n: not to be returned
    s, r = sh.search_end(ctx)
    _check(s, r, rows, q, k, f"append between the halves, reserve={reserve}")
    assert int(r.max()) < n
    assert int(sh._mx4_last.item()) == 0 and _listed(sh)[0] >= 1
    assert bool((r[:11, 0] == torch.arange(n - 11, n, device=DEV, dtype=torch.int32)).all())


@pytest.mark.parametrize("reserve", [0, 64])
def test_split_search_with_a_tombstone_between_the_halves(reserve):
    """Rows the begin half already listed as candidates of every query -- the partly filled
    sub-tile's rows (the prefill) -- and rows of the crowd's block, which the begin half's bf16
    scan has already read, are deleted before the end half.  The finish re-scores what the rows
    hold at the end (zeros), so no deleted row is returned and the result is the top-k over the
    physical rows as they are then.  (The deleted rows are in no query's top-k: the threshold T
    is taken at begin, so a delete of a top-k row between the halves may leave a routed block
    short of candidates -- before this change as after it -- and a caller orders such a delete
    against the search.)"""
    n, k, nq = 20_011, 10, 64    # (64 queries: their top-k rows leave most of the crowd free)
    sh, c, g = _shard(n, seed=4)
    sh.scan_reserve = reserve
    q = _near(c, nq, 0.1, g).bfloat16()
    s_before, r_before = sh.search(q, k)      # leaves the fp4 hint
    torch.cuda.synchronize()
    top = torch.unique(r_before.long().cpu())
    n_scan = n - n % 32
    free = lambda rows: rows[~torch.isin(rows, top)]   # noqa: E731
    pre = free(torch.arange(n_scan, n))
    crowd = free(torch.arange(n - CROWD, n_scan))[::7][:200]
    assert pre.numel() >= 1 and crowd.numel() == 200
    ctx = sh.search_begin(q, k)
    assert "full" not in ctx and ctx["hint_mx4"] and "cand" in ctx and "live" not in ctx
    dead = torch.cat([pre, crowd])
    assert sh.delete_rows(dead) == dead.numel()
    s, r = sh.search_end(ctx)
    rows = sh.unit_rows().float()[:n]          # (the deleted rows are zero rows now)
    assert float(rows[dead.to(DEV)].abs().max()) == 0.0
    _check(s, r, rows, q, k, f"tombstone between the halves, reserve={reserve}")
    assert torch.equal(s, s_before), "the deleted rows were in no top-k: the scores stay"
    assert not bool(torch.isin(r.long(), dead.to(DEV)).any()), "a deleted row was returned"
    assert int(sh._mx4_last.item()) == 0 and _listed(sh)[0] >= 1
    # the next search sees the tombstones from its begin on (search_end checks the live mask)
    ctx = sh.search_begin(q, k)
    assert "live" in ctx and "cand" in ctx
    s2, r2 = sh.search_end(ctx)
    _check(s2, r2, rows, q, k, "after the delete")
    assert not bool(torch.isin(r2.long(), dead.to(DEV)).any())
