"""The split (PCA fp16 + int8) pruning image at 768 on the GPU: the quantiser, the emitting scan
(index_i8.hip HK = 2 at D = 768: 13 k-steps, 2 query sets per wave) and the pruned search through
it, against the torch references; and the candidates of the partial last sub-tile, which a scan
launched without a gate used to erase."""
import pytest
import torch

from codename_symbiont_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
D, H = 768, 64


def _f(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def _close(out, ref, atol, rtol=0.0, what=""):
    err = (out.float() - ref.float()).abs()
    bad = (err > atol + rtol * ref.float().abs()).sum().item()
    assert bad == 0, f"{what}: {bad} elems off, max err {err.max().item():.4g}"


def _shard(n, dim=D, kind="anisotropic", seed=1, calibrate=True):
    from codename_symbiont_amd.index.shard import HbmIndexShard
    from codename_symbiont_amd.index.synth import CorpusGen, fill_corpus

    gen = CorpusGen(kind, dim, DEV)
    shard = HbmIndexShard(dim, n + 4096, prune="i8")
    fill_corpus(shard, gen, n, seed=seed)
    if calibrate:
        shard.calibrate_prune()
    return shard, gen


def test_quant_rows_split_768_matches_reference():
    """quant_rows_split at 768 (64 fp16 + 704 int8 per rotated row, 11 trailing dims per lane) ==
    the torch reference, rows raising (E_l, X_l, E_h, X_h) and queries getting sq and the margin."""
    from codename_symbiont_amd.ops._ext import hip, stream_handle

    n = 5003
    x = torch.nn.functional.normalize(_f(n, D, seed=81) * torch.linspace(3, 0.1, D, device=DEV),
                                      dim=-1)
    img = torch.empty(n, D + H, dtype=torch.int8, device=DEV)
    sx = torch.empty(n, device=DEV)
    b = torch.zeros(4, device=DEV)
    st = stream_handle(torch.device(DEV))
    hip().quant_rows_split(x.data_ptr(), n, D, img.data_ptr(), sx.data_ptr(), b.data_ptr(), 0, st)
    rimg, rsx, nr = R.quant_rows_split_ref(x, H)
    torch.cuda.synchronize()
    _close(sx, rsx, atol=0, rtol=1e-6, what="split scales")
    assert torch.equal(img[:, :2 * H], rimg[:, :2 * H])                  # fp16 part: bit-exact
    assert (img[:, 2 * H:].int() - rimg[:, 2 * H:].int()).abs().max() <= 1
    m = nr.amax(0)
    _close(b, torch.stack([m[0], m[1], m[3], m[4]]), atol=1e-6, rtol=1e-4, what="split bounds")
    q = torch.nn.functional.normalize(_f(300, D, seed=82), dim=-1)
    qi = torch.empty(300, D + H, dtype=torch.int8, device=DEV)
    sq = torch.empty(300, device=DEV)
    mg = torch.empty(300, device=DEV)
    hip().quant_rows_split(q.data_ptr(), 300, D, qi.data_ptr(), sq.data_ptr(), b.data_ptr(),
                           mg.data_ptr(), st)
    _, rsq, qn = R.quant_rows_split_ref(q, H)
    want = qn[:, 2] * b[0] + qn[:, 0] * b[1] + qn[:, 5] * b[2] + qn[:, 3] * b[3] + 1e-5
    torch.cuda.synchronize()
    _close(sq, rsq, atol=0, rtol=1e-6, what="split query scales")
    _close(mg, want, atol=1e-6, rtol=1e-4, what="split query margins")


def test_index_scan_i8_split_768_emits_the_bound_set():
    """The 768-wide split scan emits every row whose split estimate reaches the threshold and no
    other (rows within fp32 noise of it excepted), for both row-split forms (128 and 256 queries
    per workgroup; 64-row tiles in a 2-deep ring), over row blocks of many tiles with a ragged
    end; and none of a skipped block's rows."""
    from codename_symbiont_amd.ops._ext import hip, stream_handle

    n = 9 * 8192 + 77
    assert n % 64 != 0
    shard, gen = _shard(n)
    assert shard._i8_heavy == H and shard.rows_i8.shape[1] == D + H, shard.calib_share
    h, st = hip(), stream_handle(shard.device)
    cap = 4096
    forms = set()
    for nq in (256, 600):
        q = gen.unit(nq, seed=5).bfloat16()
        q8, sq, margin = shard.prune_query_image(q)
        est = shard.prune_estimate(q8, sq, 0, n)
        t = est.topk(40, dim=1).values[:, -1]
        thr = (t / sq).contiguous()
        want = est >= t[:, None]
        near = (est - t[:, None]).abs() <= 1e-5 * est.abs().clamp_min(1.0)
        for rs2 in (False, True):
            shard.i8_rsplit2 = rs2
            rsplit, rows_per_blk, n_rblk = shard._i8_geometry(n, nq, shard._n_cus())
            forms.add(rsplit)
            assert n_rblk >= 3 and rows_per_blk >= 5 * 64
            skip = torch.zeros(n_rblk, dtype=torch.int32, device=DEV)
            skip[1] = skip[n_rblk - 1] = 1
            for sk in (None, skip):
                cs = torch.empty(nq, cap, device=DEV)
                ci = torch.empty(nq, cap, dtype=torch.int32, device=DEV)
                cnt = torch.empty(nq, dtype=torch.int32, device=DEV)
                h.index_scan_i8(shard.rows_i8.data_ptr(), shard.sx_i8.data_ptr(), n,
                                shard.rows_i8.shape[0], rows_per_blk, n_rblk, q8.data_ptr(), nq,
                                thr.data_ptr(), cs.data_ptr(), ci.data_ptr(), cnt.data_ptr(), cap,
                                1, st, rsplit, skip=0 if sk is None else sk.data_ptr(), dim=D,
                                heavy=H, sq=sq.data_ptr())
                torch.cuda.synchronize()
                assert int(cnt.max()) <= cap
                got = torch.zeros_like(want)
                slot = torch.arange(cap, device=DEV)[None, :] < cnt[:, None]
                qi = torch.arange(nq, device=DEV)[:, None].expand(nq, cap)[slot]
                got[qi, ci[slot].long()] = True
                assert int(got.sum()) == int(cnt.sum()), "a row was emitted twice"
                w = want.clone()
                if sk is not None:
                    blk = torch.arange(n, device=DEV) // rows_per_blk
                    w &= (sk[blk] == 0)[None, :]
                    assert not got[:, sk[blk] != 0].any(), "rows of a skipped block were emitted"
                bad = (got != w) & ~near
                what = f"nq={nq} rsplit={rsplit} skip={sk is not None}"
                assert not bad.any(), f"{what}: {int(bad.sum())} rows differ"
                if sk is None:
                    assert (cnt >= 40 - near.sum(1)).all(), what
    assert forms == {1, 2}


def test_index_pruned_search_split_768_is_exact():
    """The pruned search on the anisotropic 768-d corpus through the split image: the exact bf16
    results (scores and rows) at 256 and 512 queries, no batch routed whole to the bf16 scan, no
    overflow, far fewer candidates than the plain int8 form emits -- and still the exact result
    when the image is re-calibrated between the search's halves."""
    from codename_symbiont_amd.index.shard import HbmIndexShard

    n, k = (1 << 20) + 333, 10
    shard, gen = _shard(n, seed=3)
    assert shard._i8_heavy == H, shard.calib_share
    shard.mq_stats = True
    q = gen.unit(512, seed=17).bfloat16()
    ts, ti = R.topk_ref(shard.unit_rows(), q, k)
    split_max = 0
    for nq in (256, 512):
        s1, r1 = shard.search(q[:nq], k)
        cnt, ovf = shard._mq_last
        dense = shard._route_last
        torch.cuda.synchronize()
        assert shard._pruned_last["heavy"] == H
        assert int(ovf.item()) == 0 and int(dense.item()) == 0, nq
        assert int(cnt.max()) <= HbmIndexShard.PRUNE_CAP
        _close(s1, ts[:nq], atol=2e-5, what=f"split768 pruned vs exact scores nq={nq}")
        _close(R.row_scores_ref(shard.unit_rows(), q[:nq], r1), ts[:nq], atol=2e-5,
               what=f"split768 pruned returned rows nq={nq}")
        if nq == 256:
            split_max = int(cnt.max())
    # re-calibrated between the halves (here: back to the plain image): the exact list scan
    ctx = shard._pruned_begin(q[:256], k, None)
    assert ctx is not None and ctx["heavy"] == H
    shard.i8_split = "off"
    shard.calibrate_prune()
    assert shard._i8_heavy == 0 and shard.rows_i8.shape[1] == D
    s3, r3 = shard._pruned_end(ctx)
    torch.cuda.synchronize()
    _close(s3, ts[:256], atol=2e-5, what="re-calibrated between the halves: scores")
    _close(R.row_scores_ref(shard.unit_rows(), q[:256], r3), ts[:256], atol=2e-5,
           what="re-calibrated between the halves: rows")
    # the plain int8 image of the same rows (same sample, same thresholds) emits far more
    shard.prune_route = False
    s2, r2 = shard.search(q[:256], k)
    cnt2, _ = shard._mq_last
    torch.cuda.synchronize()
    _close(s2, ts[:256], atol=2e-5, what="plain pruned vs exact scores")
    print("candidates max: split", split_max, "plain", int(cnt2.max()))
    assert split_max * 5 < int(cnt2.max()), (split_max, int(cnt2.max()))


@pytest.mark.parametrize("dim,kind,heavy", [(768, "anisotropic", 64), (768, "random", 0),
                                            (384, "anisotropic", 64)])
def test_partial_last_subtile_survives_a_scan_without_gate(dim, kind, heavy, monkeypatch):
    """Without the MX-fp4 tier the int8 / split scan is launched ungated.  The rows past the last
    whole 32-row sub-tile reach the candidates through prefill_candidates only, so the scan must
    not clear the counters: a query that IS one of those rows finds itself first, and every
    result equals the full bf16 scan's."""
    monkeypatch.setenv("SYMB_PRUNE_MX4", "0")
    n, k = 139_283, 10
    assert n % 32 == 19
    shard, gen = _shard(n, dim=dim, kind=kind, seed=7, calibrate=bool(heavy))
    assert not shard.mx4_on and shard._i8_heavy == heavy and shard.rows_i8 is not None
    shard.mq_stats = True
    q = torch.cat([shard.unit_rows()[n - 19:n].float(), gen.unit(45, seed=11)]).bfloat16()
    out = shard._search_pruned(q, k, None)
    assert out is not None
    s, r = out
    ts, ti = R.topk_ref(shard.unit_rows(), q, k)
    torch.cuda.synchronize()
    assert shard._pruned_last["heavy"] == heavy and int(shard._mq_last[1].item()) == 0
    assert r[:19, 0].tolist() == list(range(n - 19, n))
    _close(s, ts, atol=2e-5, what="scores")
    _close(R.row_scores_ref(shard.unit_rows(), q, r), ts, atol=2e-5, what="returned rows")
