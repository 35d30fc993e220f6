"""Search under a row mask on CPU shards: mask packing, the masked chunked matmul against the
reference, the (-inf, -1) tail, and the Filter / PayloadStore semantics of VectorStore.search."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from codename_symbiont_amd.index.filter import Filter
from codename_symbiont_amd.index.shard import HbmIndexShard, Payload, RowMask
from codename_symbiont_amd.index.store import VectorStore
from codename_symbiont_amd.ops import reference as R

N, D, K = 3000, 32, 5


def _shard(n=N, dim=D, dtype="bf16", seed=3):
    sh = HbmIndexShard(dim, n + 200, device="cpu", dtype=dtype)
    sh.fill_random(n, seed=seed)
    return sh


def _queries(nq=7, dim=D, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(nq, dim, generator=g), dim=-1).bfloat16()


def _random_allow(n, share, seed):
    return torch.from_numpy(np.random.default_rng(seed).random(n) < share)


def test_make_mask_forms_agree_and_clear_past_visible():
    sh = _shard()
    allow = _random_allow(N, 0.3, 1)
    want = np.packbits(allow.numpy(), bitorder="little")
    m_bool = sh.make_mask(allow)
    m_np = sh.make_mask(allow.numpy())
    m_rows = sh.make_mask(torch.nonzero(allow).flatten().tolist())
    # packed input with every bit past `visible` SET: they must come out clear
    dirty = np.full((N + 63) // 64 * 8 + 16, 0xFF, dtype=np.uint8)
    dirty[:want.size] = want
    dirty[N // 8] |= (0xFF << (N % 8)) & 0xFF
    m_packed = sh.make_mask(dirty)
    m_bytes = sh.make_mask(dirty.tobytes())
    for m in (m_bool, m_np, m_rows, m_packed, m_bytes):
        assert isinstance(m, RowMask) and m.visible == N
        assert m.bits.dtype == torch.uint8 and m.bits.numel() % 8 == 0
        assert m.bits.numel() == (N + 63) // 64 * 8
        got = m.bits.numpy()
        assert np.array_equal(got[:want.size], want)
        assert not got[want.size:].any()
        assert m.count() == int(allow.sum())
    # a shorter bool mask disallows the rest; a longer one is refused; so is a row past visible
    short = sh.make_mask(torch.ones(100, dtype=torch.bool))
    assert short.count() == 100 and bool(short.bool_rows(90, 110)[:10].all())
    assert not short.bool_rows(90, 110)[10:].any()
    with pytest.raises(ValueError):
        sh.make_mask(torch.ones(N + 1, dtype=torch.bool))
    with pytest.raises(IndexError):
        sh.make_mask([0, N])
    assert sh.make_mask(m_bool) is m_bool


@pytest.mark.parametrize("share", [0.5, 0.01])
def test_masked_matmul_equals_reference_over_several_chunks(share):
    sh, q = _shard(), _queries()
    allow = _random_allow(N, share, 2)
    mask = sh.make_mask(allow)
    ref_s, ref_i = R.filtered_topk_ref(sh.unit_rows(), q, K, allow)
    # chunks of 1000 and of 999 rows (the second: chunk starts that are no multiple of 8)
    for chunk in (1000, 999):
        assert chunk < N
        s, r = sh._search_matmul(q, K, chunk=chunk, mask=mask)
        assert torch.equal(r.long(), ref_i), chunk
        torch.testing.assert_close(s, ref_s, atol=1e-6, rtol=0)
    s, r = sh.search(q, K, allow=allow)
    assert torch.equal(r.long(), ref_i)
    assert r.dtype == torch.int32 and s.dtype == torch.float32
    assert bool(allow[r.long().flatten()].all())


def test_fewer_than_k_allowed_rows_and_empty_mask():
    sh, q = _shard(), _queries()
    rows = [2999, 17, 1024]
    s, r = sh.search(q, K, allow=rows)
    assert torch.isfinite(s[:, :3]).all() and (s[:, 3:] == -float("inf")).all()
    assert (r[:, 3:] == -1).all()
    for i in range(q.shape[0]):
        assert sorted(r[i, :3].tolist()) == sorted(rows)
    assert (s[:, :2] >= s[:, 1:3]).all()
    s, r = sh.search(q, K, allow=torch.zeros(N, dtype=torch.bool))
    assert (s == -float("inf")).all() and (r == -1).all()
    assert s.shape == (q.shape[0], K) and r.shape == (q.shape[0], K)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_all_ones_mask_equals_unmasked_search(dtype):
    dim = D if dtype == "bf16" else 256            # (fp8 rows: 256 is the narrowest width)
    sh, q = _shard(n=700, dim=dim, dtype=dtype), _queries(dim=dim)
    s0, r0 = sh.search(q, K)
    s1, r1 = sh.search(q, K, allow=torch.ones(700, dtype=torch.bool))
    assert torch.equal(s0, s1) and torch.equal(r0, r1)
    ctx = sh.search_begin(q, K, allow=torch.ones(700, dtype=torch.bool))
    s2, r2 = sh.search_end(ctx)
    assert torch.equal(s0, s2) and torch.equal(r0, r2)


def test_row_mask_disallows_rows_appended_later():
    sh, q = _shard(), _queries()
    mask = sh.make_mask(torch.ones(N, dtype=torch.bool))
    sh.append_unit(q[:3])           # exact copies of three queries: unmasked top-1
    s, r = sh.search(q, K, allow=mask)
    assert int(r.max()) < N
    s_all, r_all = sh.search(q, K)
    assert r_all[:3, 0].tolist() == [N, N + 1, N + 2]


# ---------------------------------------------------------------------------- Filter semantics
DOCS = ("doc-a", "doc-b", "doc-c")
URLS = ("http://one.example/x", "http://two.example/y")
SD = 16


def _vec(i):
    g = np.random.default_rng(1000 + i)
    return g.standard_normal(SD).astype(np.float32)


def _store(n_points=30, bare=6):
    """Points p0..p{n-1}: document i % 3, url i % 2, model "m0" / "m1" by halves; then `bare`
    rows without point id or payload."""
    st = VectorStore(SD, 256, device="cpu")
    ids = [f"p{i}" for i in range(n_points)]
    pls = [Payload(DOCS[i % 3], URLS[i % 2], f"s{i}", i, "m0" if i < n_points // 2 else "m1", 0)
           for i in range(n_points)]
    st.upsert(ids, np.stack([_vec(i) for i in range(n_points)]), pls)
    if bare:
        st.shard.append_f32(torch.from_numpy(np.stack([_vec(500 + i) for i in range(bare)])))
    return st


def _hits(st, flt, k=64):
    q = np.stack([_vec(900), _vec(901)])
    s, r = st.search(q, k, filter=flt)
    assert s.shape == (2, k) and r.shape == (2, k)
    out = []
    for i in range(2):
        fin = np.isfinite(s[i])
        assert (r[i][fin] >= 0).all() and (r[i][~fin] == -1).all()
        assert not fin[int(fin.sum()):].any()          # finite slots first, then the tail
        assert len(set(r[i][fin].tolist())) == int(fin.sum())
        out.append(set(r[i][fin].tolist()))
    assert out[0] == out[1]
    return out[0]


def _check_indices(st):
    """Every built value index equals a fresh scan of the stored payloads."""
    ps = st.shard.payloads
    for field, idx in ps._by_value.items():
        want = {}
        for row, t in ps.fields.items():
            want.setdefault(ps._field_value(t, field), set()).add(row)
        assert idx == want, field


def _semantics(st, n_points, bare_rows):
    pts = set(range(n_points))
    doc = lambda d: {i for i in pts if i % 3 == d}
    url = lambda u: {i for i in pts if i % 2 == u}
    assert _hits(st, Filter(must={"original_document_id": "doc-a"})) == doc(0)
    assert _hits(st, Filter(must={"original_document_id": ["doc-a", "doc-c"]})) == doc(0) | doc(2)
    assert _hits(st, Filter(must={"original_document_id": "doc-b", "source_url": URLS[0]})) \
        == doc(1) & url(0)
    assert _hits(st, Filter(must={"original_document_id": "nope"})) == set()
    # must_not: rows without payload pass; must: they never match
    assert _hits(st, Filter(must_not={"original_document_id": "doc-a"})) \
        == (pts - doc(0)) | bare_rows
    assert _hits(st, Filter(must_not={"source_url": list(URLS)})) == bare_rows
    assert _hits(st, Filter(must={"model_name": "m0"}, must_not={"original_document_id": "doc-c"})) \
        == {i for i in pts if i < 15} - doc(2)
    want = {i for i in (1, 4, 7) if i in pts}
    assert _hits(st, Filter(point_ids=["p1", "p4", "p7", "missing"])) == want
    assert _hits(st, Filter(must={"original_document_id": "doc-b"}, point_ids=["p1", "p2", "p4"])) \
        == {i for i in (1, 4) if i in pts}
    _check_indices(st)


def test_filter_semantics_upkeep_and_truncate():
    st = _store()
    ps = st.shard.payloads
    q = np.stack([_vec(900)])
    s0, r0 = st.search(q, 5)                      # a search before any filter: no index is built
    assert ps._by_value == {}
    bare = set(range(30, 36))
    _semantics(st, 30, bare)
    assert set(ps._by_value) == {"original_document_id", "source_url", "model_name"}
    s1, r1 = st.search(q, 5)                      # ... and after: the plain search is unchanged
    assert np.array_equal(s0, s1) and np.array_equal(r0, r1)

    # fewer than k passing points: exactly that many finite slots
    s, r = st.search(q, 5, filter=Filter(point_ids=["p3", "p9"]))
    assert np.isfinite(s[0]).sum() == 2 and (r[0, 2:] == -1).all() and set(r[0, :2]) == {3, 9}

    # p0 (doc-a) upserted again under doc-b: it moves between the two filters (cached masks of
    # both were built above, so this checks the cache drop and the index upkeep)
    fa, fb = Filter(must={"original_document_id": "doc-a"}), Filter(must={"original_document_id": "doc-b"})
    assert 0 in _hits(st, fa) and 0 not in _hits(st, fb)
    assert len(st._masks) >= 2
    st.upsert(["p0"], _vec(0)[None], [Payload("doc-b", URLS[0], "s0", 0, "m0", 0)])
    assert len(st._masks) == 0
    assert 0 not in _hits(st, fa) and 0 in _hits(st, fb)
    _check_indices(st)
    # a new point lands in its document's filter
    st.upsert(["fresh"], _vec(77)[None], [Payload("doc-a", URLS[1], "sf", 0, "m1", 0)])
    assert 36 in _hits(st, fa)
    _check_indices(st)
    st.upsert(["p0"], _vec(0)[None], [Payload("doc-a", URLS[0], "s0", 0, "m0", 0)])

    # the mask cache is an LRU of bounded size
    for i in range(st.FILTER_CACHE_MAX + 3):
        st.search(q, 3, filter=Filter(point_ids=[f"p{i}"]))
    assert len(st._masks) == st.FILTER_CACHE_MAX

    # truncate: the rows (and their index entries) are gone; repeat the whole table
    st.shard.truncate(20)
    st._masks.clear()
    _check_indices(st)
    assert all(r < 20 for idx in ps._by_value.values() for rows in idx.values() for r in rows)
    _semantics(st, 20, set())


def test_filter_refuses_unknown_field_and_non_filter():
    with pytest.raises(ValueError):
        Filter(must={"sentence_text": "x"})
    st = _store(6, 0)
    with pytest.raises(TypeError):
        st.search(_vec(1)[None], 3, filter={"original_document_id": "doc-a"})
    assert Filter(must={"source_url": ["b", "a"]}) == Filter(must={"source_url": ("a", "b", "a")})


def test_filter_with_group_attached_raises():
    class Group:
        def __init__(self):
            self.shard = HbmIndexShard(SD, 64, device="cpu")
            self.shard.fill_random(8, seed=1)

        @property
        def count(self):
            return self.shard.count

        def search(self, q, k):
            return self.shard.search(q, k)

    st = VectorStore(SD, 64, device="cpu", group=Group())
    s, r = st.search(_vec(1)[None], 3)
    assert r.shape == (1, 3)
    with pytest.raises(ValueError, match="single-shard"):
        st.search(_vec(1)[None], 3, filter=Filter(must={"model_name": "m0"}))
