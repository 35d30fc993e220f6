"""The prefix tier of the MX-fp4 stream scan on the GPU (index_stream.hip scan_stream_kernel NKP_,
the image writers' prefix bounds, index_i8.hip mx4_prefix_select_kernel, index/shard.py): the scan
emits exactly the rows whose decoded PREFIX dot reaches the threshold, the bounds the kernels track
equal the reference, and a search takes the tier the rule names and returns what the bf16 scan
returns.  All at dim 384 on bf16 shards with pruning on.
"""
import math

import pytest
import torch

from codename_symbiont_amd.ops import reference as R
from test_prefix_tier_cpu import (near_duplicate_queries, remainder_row, small_shard_limit,
                                  tier_oracle)

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 384
DEEP = {3: 6, 2: 8}


def _unit(x):
    return torch.nn.functional.normalize(x.float(), dim=-1)


def _close(out, ref, atol, rtol=0.0, what=""):
    err = (out.float() - ref.float()).abs()
    bad = (err > atol + rtol * ref.float().abs()).sum().item()
    assert bad == 0, f"{what}: {bad} elems off, max err {err.max().item():.4g}"


def _emitted(ci, cnt, n):
    got = torch.zeros(ci.shape[0], n, dtype=torch.bool, device=DEV)
    for i in range(ci.shape[0]):
        got[i, ci[i, :int(cnt[i])].long()] = True
    return got


_SCAN = {}


def _scan_data():
    """One 200,077-row random shard, its decoded MX-fp4 image and the decoded images of the
    queries of each batch size (computed once for every case below)."""
    if _SCAN:
        return _SCAN
    from codename_symbiont_amd.index.shard import HbmIndexShard

    n = 200_000 + 77
    sh = HbmIndexShard(D, n + 4096, prune="i8")
    sh.fill_random(n, seed=5)
    assert sh.stream and sh.img_mx4 is not None and sh.prefix_on
    xt = R.stream_mx4_decode(sh.img_mx4[:(n + 31) // 32], n, D)
    qs = {}
    for nq in (200, 256, 600):
        g = torch.Generator(device="cpu").manual_seed(nq + D)
        q = _unit(torch.randn(nq, D, generator=g)).bfloat16().to(DEV)
        q4, qs4, _ = sh.mx4_query_image(q)
        qs[nq] = (q4, qs4, R.stream_mx4_query_decode(q4, qs4))
    _SCAN.update(sh=sh, n=n, xt=xt, qs=qs)
    return _SCAN


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("nkp", [2, 3])
def test_prefix_scan_emits_the_bound_set(nkp, wide):
    """The prefix form (thin and CU-granular, depth 3 and the deep depth, non-temporal): exactly
    the rows whose decoded dot over the first 64 nkp dims reaches the threshold, for 1, 2 and 3
    query blocks, a ragged row count (a partial last sub-tile) and skipped row blocks -- pins the
    partial record read and the scale dword's k-step bytes."""
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import stream_handle

    S = _scan_data()
    sh, n, p = S["sh"], S["n"], 64 * nkp
    st, img = stream_handle(sh.device), sh.img_mx4
    xp = S["xt"][:, :p].t().contiguous()
    for nq in (200, 256, 600):
        q4, qs4, qt = S["qs"][nq]
        est = qt[:, :p] @ xp
        t = est.topk(40, dim=1).values[:, -1].contiguous()
        _, rows_per_blk, n_rblk = sh._i8_geometry(n, nq, sh._n_cus())
        skip = torch.zeros(n_rblk, dtype=torch.int32, device=DEV)
        skip[1::3] = 1                                            # every third block skipped
        live = ~skip.bool().repeat_interleave(rows_per_blk)[:n]
        want = (est >= t[:, None]) & live[None, :]
        near = (est - t[:, None]).abs() <= 1e-5 * est.abs().clamp_min(1.0)
        for depth in (3, DEEP[nkp]):
            cap = 4096
            cs = torch.empty(nq, cap, device=DEV)
            ci = torch.empty(nq, cap, dtype=torch.int32, device=DEV)
            cnt = torch.empty(nq, dtype=torch.int32, device=DEV)
            K.index_scan_stream(img.data_ptr(), n, img.shape[0] * 32, rows_per_blk, n_rblk,
                                q4.data_ptr(), qs4.data_ptr(), nq, t.data_ptr(), cs.data_ptr(),
                                ci.data_ptr(), cnt.data_ptr(), cap, 1, st, skip=skip.data_ptr(),
                                dim=D, form=1, wide=wide, depth=depth, nt=1, prefix=nkp,
                                pbounds=sh.mx4_pbounds)
            torch.cuda.synchronize()
            assert int(cnt.max()) <= cap
            bad = (_emitted(ci, cnt, n) != want) & ~near
            what = f"nkp={nkp} wide={wide} depth={depth} nq={nq}"
            assert not bad.any(), f"{what}: {int(bad.sum())} rows differ"
            c0 = int(cnt[0])
            _close(cs[0, :c0], est[0, ci[0, :c0].long()], atol=1e-4, rtol=1e-5,
                   what=f"{what} emitted scores")


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("nkp", [2, 3])
def test_one_launch_runs_the_form_the_word_names(nkp, wide):
    """The fp4 tier's one launch (scan_stream_dual_kernel): form word 0 emits the prefix bound set
    at the prefix thresholds and counts a prefix run, any other value the whole-row bound set at
    the whole-row thresholds and counts none; a closed first gate runs neither."""
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import stream_handle

    S = _scan_data()
    sh, n, p, nq = S["sh"], S["n"], 64 * nkp, 200
    st, img = stream_handle(sh.device), sh.img_mx4
    q4, qs4, qt = S["qs"][nq]
    est = {0: qt[:, :p] @ S["xt"][:, :p].t(), 1: qt @ S["xt"].t()}
    thr = {w: e.topk(40, dim=1).values[:, -1].contiguous() for w, e in est.items()}
    _, rows_per_blk, n_rblk = sh._i8_geometry(n, nq, sh._n_cus())
    runs2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    for gate_open, word, want_runs in ((1, 0, 1), (1, 1, 1), (1, 5, 1), (0, 0, 1)):
        cap = 4096
        cs = torch.empty(nq, cap, device=DEV)
        ci = torch.empty(nq, cap, dtype=torch.int32, device=DEV)
        cnt = torch.empty(nq, dtype=torch.int32, device=DEV)
        gate = torch.tensor([0 if gate_open else 1], dtype=torch.int32, device=DEV)
        form = torch.tensor([word], dtype=torch.int32, device=DEV)
        K.index_scan_stream(img.data_ptr(), n, img.shape[0] * 32, rows_per_blk, n_rblk,
                            q4.data_ptr(), qs4.data_ptr(), nq, thr[1].data_ptr(), cs.data_ptr(),
                            ci.data_ptr(), cnt.data_ptr(), cap, 1, st, dim=D, form=1, wide=wide,
                            depth=DEEP[nkp], nt=1, prefix=nkp, pbounds=sh.mx4_pbounds,
                            thr_prefix=thr[0].data_ptr(), gate=gate.data_ptr(), gate_want=0,
                            gate2=form.data_ptr(), runs2=runs2.data_ptr())
        torch.cuda.synchronize()
        what = f"nkp={nkp} wide={wide} gate_open={gate_open} word={word}"
        assert int(runs2.item()) == want_runs, what
        if not gate_open:
            assert int(cnt.max()) == 0, what
            continue
        w = 0 if word == 0 else 1
        want = est[w] >= thr[w][:, None]
        near = (est[w] - thr[w][:, None]).abs() <= 1e-5 * est[w].abs().clamp_min(1.0)
        assert int(cnt.max()) <= cap
        bad = (_emitted(ci, cnt, n) != want) & ~near
        assert not bad.any(), f"{what}: {int(bad.sum())} rows differ"


@pytest.mark.parametrize("nkp", [2, 3])
def test_prefix_scan_centroid_test_is_exact(nkp):
    """Two near-duplicate query clusters with planted rows near each: the prefix scan with the
    centroid test emits exactly what it emits without it, with the rows' norm bound the shard
    hands the prefix scan: X_P = mx4_pbounds[1] (|(q~ - c~)_P| <= R_s, |x~_P| <= X_P; the bound
    tracked over 3 k-steps covers the 2 k-step prefix too)."""
    from codename_symbiont_amd.index.shard import HbmIndexShard
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import hip, stream_handle

    n, p = 150_000 + 33, 64 * nkp
    g = torch.Generator(device=DEV).manual_seed(81)
    sh = HbmIndexShard(D, n + 4096, prune="i8")
    sh.fill_random(n - 2000, seed=9)
    cs_ = _unit(torch.randn(2, D, device=DEV, generator=g))
    near = lambda c, m, e: _unit(c + e * torch.randn(m, D, device=DEV, generator=g) / math.sqrt(D))
    sh.append_f32(torch.cat([near(cs_[0], 1000, 0.3), near(cs_[1], 1000, 0.3)]))
    q = torch.cat([near(cs_[0], 128, 0.1), near(cs_[1], 100, 0.1)]).bfloat16()
    nq = q.shape[0]          # (228: a partial last set)
    h, st = hip(), stream_handle(sh.device)
    q4, qs4, _ = sh.mx4_query_image(q)
    n_sets = -(-nq // 32)
    c4 = torch.empty(n_sets, D // 2, dtype=torch.uint8, device=DEV)
    cqs = torch.empty(n_sets, qs4.shape[1], dtype=torch.int32, device=DEV)
    cR = torch.empty(n_sets, device=DEV)
    h.mx4_centroids(q4.data_ptr(), qs4.data_ptr(), nq, D, c4.data_ptr(), cqs.data_ptr(),
                    cR.data_ptr(), st)
    qt = R.stream_mx4_query_decode(q4, qs4)
    xt = R.stream_mx4_decode(sh.img_mx4[:(n + 31) // 32], n, D)
    est = qt[:, :p] @ xt[:, :p].t()
    t = (est.topk(30, dim=1).values[:, -1] - 0.02).contiguous()
    _, rows_per_blk, n_rblk = sh._i8_geometry(n, nq, sh._n_cus())
    got = []
    for cent in (False, True):
        cap = 8192
        cs = torch.empty(nq, cap, device=DEV)
        ci = torch.empty(nq, cap, dtype=torch.int32, device=DEV)
        cnt = torch.empty(nq, dtype=torch.int32, device=DEV)
        kw = sh._cent_args(dict(c4=c4, cqs=cqs, cR=cR), prefix=True) if cent else {}
        assert not cent or kw["bounds4"] == sh.mx4_pbounds.data_ptr()
        K.index_scan_stream(sh.img_mx4.data_ptr(), n, sh.img_mx4.shape[0] * 32, rows_per_blk,
                            n_rblk, q4.data_ptr(), qs4.data_ptr(), nq, t.data_ptr(), cs.data_ptr(),
                            ci.data_ptr(), cnt.data_ptr(), cap, 1, st, dim=D, form=1, nt=1,
                            depth=DEEP[nkp], prefix=nkp, pbounds=sh.mx4_pbounds, **kw)
        torch.cuda.synchronize()
        assert int(cnt.max()) <= cap
        got.append(_emitted(ci, cnt, n))
    assert torch.equal(got[0], got[1]), "the centroid test changed the emitted set"
    want = est >= t[:, None]
    near_t = (est - t[:, None]).abs() <= 1e-5
    assert not ((got[1] != want) & ~near_t).any()


@pytest.mark.parametrize("nkp", [2, 3])
def test_prefix_bounds_match_the_reference(nkp):
    """append_rows and quant_stream_mx4 raise mx4_pbounds to the reference's (E_P, X_P, XR), the
    query mode writes mP and qR from them, and a 2-float bounds buffer handed over without the new
    argument is not written past."""
    from codename_symbiont_amd.ops._ext import hip, stream_handle

    h, st = hip(), stream_handle()
    n, r0, cap = 1000 + 13, 37, 2048
    g = torch.Generator(device="cpu").manual_seed(3 + nkp)
    x = _unit(torch.randn(n, D, generator=g))
    x[5, 64 * nkp:] = 0                      # all its mass in the prefix
    x[6, :64 * nkp] = 0                      # ... in the remainder
    x[7] = 0
    x = _unit(x).bfloat16().to(DEV)
    pn = R.mx4_prefix_norms_ref(x, nkp)
    want = pn[:, [0, 1, 3]].amax(0)
    rec = h.stream_rec_bytes(D, 1)
    imgs = torch.zeros(3, cap // 32, rec, dtype=torch.uint8, device=DEV)
    img8 = torch.zeros(cap // 32, h.stream_rec_bytes(D, 0), dtype=torch.uint8, device=DEV)
    rows = torch.zeros(cap, D, dtype=torch.bfloat16, device=DEV)
    b8 = torch.zeros(2, device=DEV)
    b = torch.zeros(3, 4, device=DEV)
    b[:, 2:] = -7.0                          # (what lies past a 2-float bounds buffer)
    pb = torch.zeros(2, 3, device=DEV)
    h.append_rows(x.data_ptr(), n, D, rows.data_ptr(), r0, img8.data_ptr(), b8.data_ptr(),
                  imgs[0].data_ptr(), b[0].data_ptr(), st, pb4=pb[0].data_ptr(), nkp=nkp)
    h.quant_stream_mx4(rows.data_ptr(), r0, 0, n, D, imgs[1].data_ptr(), 0, 0, b[1].data_ptr(), 0,
                       st, pbounds=pb[1].data_ptr(), nkp=nkp)
    h.quant_stream_mx4(rows.data_ptr(), r0, 0, n, D, imgs[2].data_ptr(), 0, 0, b[2].data_ptr(), 0,
                       st)
    torch.cuda.synchronize()
    assert torch.equal(imgs[0], imgs[1]) and torch.equal(imgs[1], imgs[2])
    assert bool((b[:, 2:] == -7.0).all()), "written past a 2-float bounds buffer"
    assert torch.equal(b[0, :2], b[2, :2]) and torch.equal(b[1, :2], b[2, :2])
    print("pbounds", pb.tolist(), "reference", want.tolist())
    for i, what in enumerate(("append_rows", "quant_stream_mx4")):
        _close(pb[i], want, atol=0, rtol=1e-6, what=f"{what} prefix bounds")
    # queries: mP and qR beside m4
    nq = 77
    q4 = torch.empty(nq, D // 2, dtype=torch.uint8, device=DEV)
    qs4 = torch.empty(nq, 4, dtype=torch.int32, device=DEV)
    m4, mP, qR = (torch.full((nq,), -1.0, device=DEV) for _ in range(3))
    h.quant_stream_mx4(x.data_ptr(), 0, 0, nq, D, 0, q4.data_ptr(), qs4.data_ptr(),
                       b[1].data_ptr(), m4.data_ptr(), st, pbounds=pb[1].data_ptr(), nkp=nkp,
                       mP=mP.data_ptr(), qR=qR.data_ptr())
    torch.cuda.synchronize()
    _close(mP, pn[:nq, 2] * pb[1, 0] + pn[:nq, 0] * pb[1, 1] + 1e-5, atol=0, rtol=1e-6, what="mP")
    _close(qR, pn[:nq, 3], atol=1e-7, rtol=1e-6, what="qR")   # (qR = 0 exactly for row 5)
    nr = R.mx4_codes_ref(x[:nq])[3]
    _close(m4, nr[:, 2] * b[1, 0] + nr[:, 0] * b[1, 1] + 1e-5, atol=0, rtol=1e-6, what="m4")


_E2E = {}


def _e2e(kind):
    """(shard, queries, reference rows) of a routing case at ~150k rows: random rows, then
    (fp4: one remainder-only row) and 256 TorchEncoder near-duplicates as the fresh tail."""
    if kind in _E2E:
        return _E2E[kind]
    from codename_symbiont_amd.index.shard import HbmIndexShard

    if "dup" not in _E2E:
        _E2E["dup"] = near_duplicate_queries(256, 1).to(DEV)
    dup = _E2E["dup"]
    sh = HbmIndexShard(D, 160_000, prune="i8")
    sh.SEED_MIN_ROWS = 0        # (the sampled search's row-count gates, lowered on the instance)
    sh.PRUNE_MIN_SHIFT = 0
    small_shard_limit(sh)
    sh.fill_random(150_000 + 21, seed=4)
    if kind == "fp4":
        sh.append_unit(remainder_row().bfloat16().to(DEV))
    sh.append_unit(dup)
    if kind == "int8":
        g = torch.Generator(device="cpu").manual_seed(8)
        q = _unit(torch.randn(256, D, generator=g)).bfloat16().to(DEV)
    else:
        q = dup
    assert sh.prefix_on and sh._prefix_enqueued(True)
    _E2E[kind] = (sh, q)
    return _E2E[kind]


def _counters(sh):
    torch.cuda.synchronize()
    return (0 if sh._mx4_tot is None else int(sh._mx4_tot.item())), sh.prefix_runs


def _check_exact(sh, q, s, r, k, what):
    rows = sh.unit_rows().float()
    ts, _ = R.topk_ref(rows, q, k)
    _close(s, ts, atol=2e-5, what=f"{what} scores")
    _close(R.row_scores_ref(rows, q, r), ts, atol=2e-5, what=f"{what} rows")


@pytest.mark.parametrize("kind", ["prefix", "fp4", "int8"])
def test_search_takes_the_named_tier_and_is_exact(kind):
    """search() and the split-phase search on two streams take the tier the rule names (asserted
    through the device counters: a prefix-tier search raises the fp4-tier counter AND the prefix
    counter, a whole-row fp4 search only the former, an int8 search neither) and return what the
    bf16 scan returns; a ragged batch, and rows deleted before the search, included.  Without the
    qR XR term in thrP the "fp4" case would run the prefix scan (the counters differ) and the
    "prefix" case would put thrP near T, far above the prefix estimates of the true neighbours,
    and lose them.  (The "int8" case cannot tell: its fp4 tier is not viable with or without the
    term.)"""
    sh, q = _e2e(kind)
    k = 10
    name, _ = tier_oracle(sh, q, k)
    assert name == kind, name
    bump = {"prefix": (1, 1), "fp4": (1, 0), "int8": (0, 0)}[kind]

    def run(fn, what):
        c0 = _counters(sh)
        s, r = fn()
        c1 = _counters(sh)
        assert (c1[0] - c0[0], c1[1] - c0[1]) == bump, (what, c0, c1)
        # (the flag words: 0 = an fp4 tier ran; 0 = its prefix form)
        assert (int(sh._mx4_last.item()) == 0) == (kind != "int8")
        if kind != "int8":
            assert (int(sh._pfx_last.item()) == 0) == (kind == "prefix")
        return s, r

    s, r = run(lambda: sh.search(q, k), "search")
    _check_exact(sh, q, s, r, k, f"{kind} search")
    # a ragged batch
    s, r = run(lambda: sh.search(q[:203], k), "ragged")
    _check_exact(sh, q[:203], s, r, k, f"{kind} ragged search")
    # split-phase, the halves on two streams
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def split():
        s1.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s1):
            ctx = sh.search_begin(q, k)
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            out = sh.search_end(ctx)
        torch.cuda.current_stream().wait_stream(s2)
        return out

    s, r = run(split, "split")
    _check_exact(sh, q, s, r, k, f"{kind} split-phase search")
    # rows deleted by tombstone before the search: three of the near-duplicates, two bulk rows
    n = sh.visible
    sh.delete_rows([n - 1, n - 7, n - 100, 11, 70_000])
    s, r = sh.search(q, k)
    torch.cuda.synchronize()
    _check_exact(sh, q, s, r, k, f"{kind} search after deletes")
    dead = torch.tensor([n - 1, n - 7, n - 100, 11, 70_000], device=DEV, dtype=r.dtype)
    assert not bool(torch.isin(r, dead).any())
