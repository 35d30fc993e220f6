"""A test of the tests: the lattice data and the bit-exact checker (tests/lattice.py) on the fp32
oracle and the CPU shard alone.

tests/test_lattice_gpu.py asserts ``torch.equal`` between every HIP search route and the fp32
matmul oracle.  That is only sound, and only worth anything, if

* the data is what lattice.py says: exact in bf16 and e4m3, every fp32 score equal to the integer
  computation (generator properties);
* the data holds the ties the GPU tests are there for, and few enough rows near the k-th score
  that the emitting routes run their main path and not the overflow fallback (tie and cap
  conditions, at the GPU tests' row count);
* ``check_exact`` rejects every way a top-k can be subtly wrong and accepts any choice among
  genuinely tied rows (checker self-test).

The same harness then runs on ``HbmIndexShard(device="cpu")``, the matmul route."""
import math

import pytest
import torch

import lattice as L
from codename_symbiont_amd.index.shard import HbmIndexShard
from codename_symbiont_amd.ops import reference as R

N_GPU = 266_240 + 777       # the sampled tier's row count in tests/test_lattice_gpu.py
NQ_STAT = 128


# ------------------------------------------------------------------------------ generators
FAMILIES = {
    "dense": lambda n, D, seed: (L.dense(n, D, seed=seed), 7),
    "ternary": lambda n, D, seed: (L.ternary(n, D, seed=seed), L.ternary_exp(D)),
    "orthant": lambda n, D, seed: (L.orthant(n, D, seed=seed), 7),
}


def _queries(family, nq, D, seed):
    if family == "orthant":
        return L.orthant_queries(nq, D, seed=seed)
    return FAMILIES[family](nq, D, seed)[0]


@pytest.mark.parametrize("D", [384, 768, 1024])
@pytest.mark.parametrize("family", ["dense", "ternary", "orthant"])
def test_lattice_values_and_scores_are_exact(family, D):
    x, e = FAMILIES[family](3001, D, 1)
    q = _queries(family, 33, D, 2)
    for t in (x, q):
        assert t.dtype == torch.bfloat16
        m = L.to_ints(t, e)
        # the bf16 value IS m / 2^e, and it survives the shard's e4m3 image unchanged
        assert torch.equal(t.float(), m.float() * 2.0 ** -e)
        assert torch.equal(t.float().bfloat16(), t)
        img = (t.float() * 256.0).to(torch.float8_e4m3fn)
        assert torch.equal(img.float(), t.float() * 256.0)
        assert int(m.abs().max()) <= (1 if family == "ternary" else 7)
    si = L.int_scores(x, q, e, e)
    assert int(si.abs().max()) < 2 ** 24
    s = q.float() @ x.float().t()
    assert torch.equal(s.double(), si.double() * 2.0 ** (-2 * e))
    # ... in another summation order too (row by row, then reversed columns)
    s2 = (q.float().flip(1)[:, None, :] * x.float().flip(1)[None, :64, :]).sum(-1)
    assert torch.equal(s2, s[:, :64])
    # the oracle the GPU tests use returns exactly these values
    v, i = R.topk_ref(x, q, 10)
    vi = torch.topk(si, 10, dim=1).values
    assert torch.equal(v.double(), vi.double() * 2.0 ** (-2 * e))
    assert torch.equal(torch.gather(si, 1, i), vi)
    if family == "orthant":
        assert float(s.max()) < 0.0


def test_with_duplicates_plants_exact_copies_at_the_edges():
    n = 4133
    x = L.dense(n, 384, seed=3)
    y, plan = L.with_duplicates(x, [5, 1000, 4000], [2, 9, 70], seed=4)
    assert sorted(plan) == [5, 1000, 4000] and [len(plan[s]) for s in (5, 1000, 4000)] == [2, 9, 70]
    every = [p for pos in plan.values() for p in pos]
    assert len(set(every)) == len(every) and not set(every) & set(plan)
    for src, pos in plan.items():
        assert torch.equal(y[src], x[src])
        assert all(torch.equal(y[p], x[src]) for p in pos)
    changed = (y != x).any(1).nonzero().flatten().tolist()
    assert set(changed) <= set(every)
    assert n - 1 in plan[5], "the last visible row holds a copy"
    for pos in (plan[1000], plan[4000]):
        assert any(p % 64 == 0 for p in pos) and any(p % 64 == 63 for p in pos)
        assert min(pos) < n // 4 and max(pos) > 3 * n // 4, "copies in different row blocks"


# ------------------------------------------------------------------------------ ties and caps
@pytest.fixture(scope="module", params=["dense", "ternary", "orthant"])
def stats(request):
    """Per family at D = 384 and the GPU tests' n: for k = 10 and 100, per query, the rows tied
    at the k-th score, whether two of the top k tie, and the rows at or above
    k-th - MQ_THR_MARGIN (the emitting scans' band under an ideal threshold)."""
    family = request.param
    x, e = FAMILIES[family](N_GPU, 384, 11)
    q = _queries(family, NQ_STAT, 384, 12)
    s = q.float() @ x.float().t()
    out = {"family": family}
    for k in (10, 100):
        v = torch.topk(s, k, dim=1).values
        kth = v[:, k - 1:k]
        out[k] = {"ties_at_kth": (s == kth).sum(1),
                  "tie_inside": (v[:, 1:] == v[:, :-1]).any(1),
                  "band": (s >= kth - HbmIndexShard.MQ_THR_MARGIN).sum(1)}
    return out


def test_lattice_families_hold_the_ties_and_fit_the_caps(stats):
    fam = stats["family"]
    for k, cap in ((10, HbmIndexShard.MQ_CAP), (100, HbmIndexShard.LARGE_K_CAP)):
        st = stats[k]
        print(f"{fam} k={k}: ties at k-th mean {st['ties_at_kth'].float().mean():.2f}, "
              f"tie inside top k in {st['tie_inside'].float().mean():.2%} of queries, "
              f"band max {int(st['band'].max())} (cap {cap})")
        # the main path of the emitting routes, not their overflow fallback
        assert int(st["band"].max()) < cap // 4
        if fam == "dense":
            assert st["tie_inside"].float().mean().item() >= 0.10
        if fam == "ternary":
            # every query has a tie inside its top k.  At k = 100 every query also shares its
            # k-th score with another row (15 or more of them over a dozen query seeds); at
            # k = 10 two or three queries in a hundred have a k-th row alone at its score
            # (every 64-query set tried held one), so there it is asserted of the majority
            assert bool(st["tie_inside"].all())
            shared = st["ties_at_kth"] >= 2
            assert bool(shared.all()) if k == 100 else shared.float().mean().item() > 0.5


# ------------------------------------------------------------------------------ checker
@pytest.fixture(scope="module")
def correct():
    """A correct unmasked result on dense data (distinct scores around most slots)."""
    n, nq, k = 5000, 8, 10
    x = L.dense(n, 384, seed=21)
    q = L.dense(nq, 384, seed=22)
    s, i = L.oracle_topk(x, q, k)
    L.check_exact(s, i, x, q, k)
    return x, q, k, s, i


def _slot_where(x, q, s, i, cond):
    """First (query, slot) whose corruption ``cond(query, slot)`` changes something."""
    for a in range(i.shape[0]):
        for b in range(i.shape[1]):
            if cond(a, b):
                return a, b
    raise AssertionError("no slot fits the corruption")


def _score(x, q, a, row):
    return float(x[row].float() @ q[a].float())


def test_check_exact_rejects_every_corruption(correct):
    x, q, k, s, i = correct
    n = x.shape[0]

    def rejected(s2, i2, label, **kw):
        with pytest.raises(AssertionError, match=label):
            L.check_exact(s2, i2, x, q, k, **kw)

    # one id duplicated into a neighbouring slot
    i2 = i.clone()
    i2[3, 5] = i2[3, 4]
    rejected(s, i2, r"\(c\)")
    # one id replaced by id + 1, by id + 64 (a neighbouring row, the same row of the next tile)
    for off in (1, 64):
        a, b = _slot_where(x, q, s, i, lambda a, b: int(i[a, b]) + off < n
                           and int(i[a, b]) + off not in i[a].tolist()
                           and _score(x, q, a, int(i[a, b]) + off) != float(s[a, b]))
        i2 = i.clone()
        i2[a, b] += off
        rejected(s, i2, r"\(d\)")
    # the k-th row replaced by the (k+1)-th best, where that is no tie: score and id consistent
    s11, i11 = L.oracle_topk(x, q, k + 1)
    a = int(torch.nonzero(s11[:, k] != s11[:, k - 1])[0])
    s2, i2 = s.clone(), i.clone()
    s2[a, k - 1], i2[a, k - 1] = s11[a, k], i11[a, k]
    rejected(s2, i2, r"\(a\)")
    # one score nudged by one ulp, either way
    for to in (math.inf, -math.inf):
        s2 = s.clone()
        s2[2, 7] = torch.nextafter(s2[2, 7], torch.tensor(to))
        rejected(s2, i, r"\(a\)")
    # one slot blanked
    s2, i2 = s.clone(), i.clone()
    s2[5, k - 1], i2[5, k - 1] = -math.inf, -1
    rejected(s2, i2, r"\(a\)")
    # ... and an id left in a slot the oracle leaves empty (more slots than rows)
    s3, i3 = L.oracle_topk(x[:7], q, k)
    L.check_exact(s3, i3, x[:7], q, k)
    assert bool((i3[:, 7:] == -1).all()) and bool(torch.isinf(s3[:, 7:]).all())
    i4 = i3.clone()
    i4[0, 8] = 3
    with pytest.raises(AssertionError, match=r"\(b\)"):
        L.check_exact(s3, i4, x[:7], q, k)
    # two slots swapped out of order (scores and ids together)
    a, b = _slot_where(x, q, s, i, lambda a, b: b + 1 < k and float(s[a, b]) != float(s[a, b + 1]))
    s2, i2 = s.clone(), i.clone()
    s2[a, [b, b + 1]], i2[a, [b, b + 1]] = s[a, [b + 1, b]], i[a, [b + 1, b]]
    rejected(s2, i2, r"\(a\)")
    # ... ids alone swapped: every id is a right one, in the wrong slot
    i2 = i.clone()
    i2[a, [b, b + 1]] = i[a, [b + 1, b]]
    rejected(s, i2, r"\(d\)")
    # an id out of range
    i2 = i.clone()
    i2[1, 0] = n
    rejected(s, i2, r"\(b\)")
    # a NaN score is no score
    s2 = s.clone()
    s2[0, 0] = math.nan
    rejected(s2, i, r"\(a\)")


def test_check_exact_rejects_a_masked_out_twin_and_accepts_tied_swaps():
    n, nq, k = 5000, 8, 10
    x0 = L.dense(n, 384, seed=23)
    q = L.dense(nq, 384, seed=24)
    best = L.oracle_topk(x0, q, 1)[1][:, 0]
    kth = L.oracle_topk(x0, q, k)[1][:, k - 1]
    # two copies of query 0's best row, three of query 1's k-th best (a tie across the k-th place)
    x, plan = L.with_duplicates(x0, [int(best[0]), int(kth[1])], [2, 3], seed=25)
    s, i = L.oracle_topk(x, q, k)
    L.check_exact(s, i, x, q, k)
    twins = plan[int(best[0])]
    assert float(s[0, 0]) == float(s[0, 1]) == float(s[0, 2]) and set(i[0, :3].tolist()) == {
        int(best[0]), *twins}
    # a swap between genuinely tied rows is as correct as the oracle's order
    i2 = i.clone()
    i2[0, [0, 2]] = i[0, [2, 0]]
    L.check_exact(s, i2, x, q, k)
    # ... and so is a tied row from outside the oracle's top k in the k-th slot
    tied = [int(kth[1]), *plan[int(kth[1])]]
    assert float(s[1, k - 1]) == _score(x, q, 1, tied[0])
    outside = [r for r in tied if r not in i[1].tolist()]
    assert outside, "the planted tie straddles the k-th place"
    i2 = i.clone()
    i2[1, k - 1] = outside[0]
    L.check_exact(s, i2, x, q, k)
    # under a mask that drops one twin, the result may not return it -- its score is right
    allowed = torch.ones(n, dtype=torch.bool)
    allowed[twins[0]] = False
    sm, im = L.oracle_topk(x, q, k, allowed)
    L.check_exact(sm, im, x, q, k, allowed)
    assert twins[0] not in im[0].tolist() and float(sm[0, 0]) == float(sm[0, 1])
    i2 = im.clone()
    i2[0, 0] = twins[0]
    with pytest.raises(AssertionError, match=r"\(b\)"):
        L.check_exact(sm, i2, x, q, k, allowed)
    # the unmasked answer is wrong under the mask (query 0 has one tied row fewer)
    with pytest.raises(AssertionError):
        L.check_exact(s, i, x, q, k, allowed)
    # a mask per query: the same, with query 0 alone filtered
    per_q = torch.ones(nq, n, dtype=torch.bool)
    per_q[0, twins[0]] = False
    sg, ig = L.oracle_topk(x, q, k, per_q)
    L.check_exact(sg, ig, x, q, k, per_q)
    assert torch.equal(sg[0], sm[0]) and torch.equal(sg[1:], s[1:])
    with pytest.raises(AssertionError, match=r"\(b\)"):
        L.check_exact(sm, i2, x, q, k, per_q)


def test_check_exact_on_tie_heavy_data():
    """Ternary rows: every query's k-th score is shared, so the oracle's own choice is one of
    many; any tied row in the k-th slot passes, a row one score unit lower does not."""
    n, nq, k = 20000, 8, 10
    x, q = L.ternary(n, 384, seed=26), L.ternary(nq, 384, seed=27)
    s, i = L.oracle_topk(x, q, k)
    L.check_exact(s, i, x, q, k)
    full = q.float() @ x.float().t()
    for a in range(nq):
        tied = (full[a] == s[a, k - 1]).nonzero().flatten().tolist()
        other = [r for r in tied if r not in i[a].tolist()]
        if other:
            i2 = i.clone()
            i2[a, k - 1] = other[0]
            L.check_exact(s, i2, x, q, k)
        lower = int((full[a] == s[a, k - 1] - 2.0 ** -8).nonzero()[0])
        i2 = i.clone()
        i2[a, k - 1] = lower
        with pytest.raises(AssertionError, match=r"\(d\)"):
            L.check_exact(s, i2, x, q, k)


# ------------------------------------------------------------------------------ the CPU shard
@pytest.fixture(scope="module")
def cpu_case():
    n, nq, D = 4133, 17, 384
    x0 = L.dense(n, D, seed=31)
    q = L.dense(nq, D, seed=32)
    best = L.oracle_topk(x0, q, 1)[1][:, 0].tolist()
    x, plan = L.with_duplicates(x0, best[:3], [2, 9, 70], seed=33)
    return x, q, plan


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("k", [10, 100])
def test_cpu_shard_is_exact_on_lattice_data(cpu_case, dtype, k):
    x, q, plan = cpu_case
    n = x.shape[0]
    shard = HbmIndexShard(384, n + 64, device="cpu", dtype=dtype)
    shard.append_unit(x)
    assert torch.equal(shard.unit_rows(), x), "the stored image is lossless"
    s, r = shard.search(q, k)
    L.check_exact(s, r, x, q, k, what=f"cpu {dtype}")
    # allow=: about half the rows, two whole dead tiles, the last visible row allowed, and one
    # twin of query 0's best row masked out (a tie between an allowed and a masked-out row)
    allowed = torch.rand(n, generator=torch.Generator().manual_seed(34)) < 0.5
    allowed[128:192] = False
    allowed[-64 - n % 64:-(n % 64)] = False
    allowed[n - 1] = True
    src = next(iter(plan))
    allowed[src], allowed[plan[src][0]] = True, False
    s, r = shard.search(q, k, allow=allowed)
    L.check_exact(s, r, x, q, k, allowed, what=f"cpu {dtype} allow=")
    # tombstones: every query's top 3 rows go
    top3 = L.oracle_topk(x, q, 3)[1].flatten()
    shard.delete_rows(top3)
    live = torch.ones(n, dtype=torch.bool)
    live[top3] = False
    s, r = shard.search(q, k)
    L.check_exact(s, r, x, q, k, live, what=f"cpu {dtype} tombstoned")
    # fewer rows than k
    small = HbmIndexShard(384, 64, device="cpu", dtype=dtype)
    small.append_unit(x[:3])
    s, r = small.search(q, 5)
    L.check_exact(s, r, x[:3], q, 5, what=f"cpu {dtype} n < k")
