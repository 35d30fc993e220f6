"""The split (PCA fp16 + int8) pruning image at 768: the bound, the choice of form and what the
shard allocates for it (CPU backend: the torch references are the kernels' oracles)."""
import pytest
import torch

from codename_symbiont_amd.index import shard as S
from codename_symbiont_amd.index.shard import HbmIndexShard
from codename_symbiont_amd.index.synth import CorpusGen

D = 768
H = 64   # leading fp16 components at 768 (13 k-steps of 64 bytes per row)


def test_split_widths_and_heavy_per_width():
    assert S.SPLIT_DIMS == (384, 768) and S.AUTO_SPLIT_DIMS == (384,)
    assert S.SPLIT_HEAVY[768] == H and S.SPLIT_HEAVY[384] == 64


def test_split_image_768_bound_holds_and_prunes_anisotropic_rows():
    """test_split_image_bound_holds_and_prunes_anisotropic_rows at 768: an explicit
    calibrate_prune() takes the split image on the anisotropic corpus, its bound holds for every
    (query, row) pair -- rows overwritten and appended after the calibration too -- and it leaves
    far fewer candidates above the true k-th score than the plain int8 bound."""
    n, k = 20000, 10
    g = CorpusGen("anisotropic", D, "cpu")
    sh = HbmIndexShard(D, n + 100, device="cpu", prune="i8")
    sh.append_f32(g.rows(n, seed=1))
    assert sh._i8_heavy == 0
    q = g.unit(48, seed=99).bfloat16()
    xb = sh.rows[:n].float()
    s = q.float() @ xb.t()
    T = s.topk(k, dim=1).values[:, -1:]
    q8, sq, m_plain = sh.prune_query_image(q)
    est = sh.prune_estimate(q8, sq)
    assert ((s - est).abs() <= m_plain[:, None]).all()
    c_plain = (est + m_plain[:, None] >= T).sum(1).float()

    sh.calibrate_prune()
    assert sh._i8_heavy == H and sh.calib_share > 0.6, (sh._i8_heavy, sh.calib_share)
    assert sh.rows_i8.shape[1] == D + H and sh.img_i8 is None
    rot = sh._i8_rot
    assert torch.allclose(rot @ rot.t(), torch.eye(D, dtype=torch.float64), atol=1e-10)
    sh.write_f32(7, g.rows(1, seed=3))
    sh.append_f32(g.rows(50, seed=4))
    assert sh._i8_heavy == H
    xb = sh.rows[:sh.count].float()
    s = q.float() @ xb.t()
    q8, sq, m = sh.prune_query_image(q)
    assert q8.shape == (48, D + H)
    est = sh.prune_estimate(q8, sq)
    assert ((s - est).abs() <= m[:, None]).all(), float(((s - est).abs() - m[:, None]).max())
    T = s.topk(k, dim=1).values[:, -1:]
    c_split = (est + m[:, None] >= T).sum(1).float()
    print("candidates/query plain", float(c_plain.mean()), "split", float(c_split.mean()),
          "margin plain", float(m_plain.mean()), "split", float(m.mean()), "share", sh.calib_share)
    assert (c_split >= k).all()
    assert float(c_split.mean()) * 8 < float(c_plain.mean()), (c_split.mean(), c_plain.mean())
    assert float(m.mean()) * 3 < float(m_plain.mean()), (m.mean(), m_plain.mean())


def test_isotropic_768_rows_keep_the_plain_image():
    r = HbmIndexShard(D, 5000, device="cpu", prune="i8")
    size = r._i8_store.numel()
    r.append_f32(torch.randn(5000, D, generator=torch.Generator().manual_seed(2)))
    r.calibrate_prune()
    assert r._i8_heavy == 0 and r.calib_share < 0.3, r.calib_share
    assert r.img_i8 is not None or r.rows_i8.shape[1] == D
    assert r._i8_store.numel() == size


def _plain_bytes(sh) -> int:
    """What a 768 shard's int8 store held before the split image existed at this width."""
    n_alloc = sh.sx_i8.shape[0]
    if sh.stream and not sh.i8_ring:
        return max(n_alloc * D, n_alloc // S.STREAM_SUB * sh._stream_rec(0))
    return n_alloc * D


@pytest.mark.parametrize("i8k", ["auto", "stream"])
def test_768_store_size_and_write_time_triggers(i8k, monkeypatch):
    """A 768 shard allocates the plain store until the split form is taken; under auto the
    write-time trigger never takes it at 768, SYMB_I8_SPLIT=on does, and i8_split = "off" plus a
    calibration returns to the plain view and size."""
    monkeypatch.setenv("SYMB_PRUNE_I8", i8k)
    monkeypatch.setattr(HbmIndexShard, "CALIB_MIN_ROWS", 2048)
    g = CorpusGen("anisotropic", D, "cpu")
    rows = g.rows(3000, seed=1)

    monkeypatch.setenv("SYMB_I8_SPLIT", "auto")
    a = HbmIndexShard(D, 4000, device="cpu", prune="i8")
    n_alloc = a.sx_i8.shape[0]
    assert a._i8_store.numel() == _plain_bytes(a)
    if i8k == "auto":
        assert a._i8_store.numel() == n_alloc * D
    else:
        assert a.img_i8 is not None and a._i8_store.numel() >= a.img_i8.numel()
    a.append_f32(rows[:1500])
    a.append_f32(rows[1500:])                      # past CALIB_MIN_ROWS
    assert a.count > HbmIndexShard.CALIB_MIN_ROWS
    assert a._i8_heavy == 0 and a._i8_store.numel() == _plain_bytes(a)

    monkeypatch.setenv("SYMB_I8_SPLIT", "on")
    b = HbmIndexShard(D, 4000, device="cpu", prune="i8")
    assert b._i8_heavy == 0 and b._i8_store.numel() == _plain_bytes(b)
    sx, bounds = b.sx_i8, b.i8_bounds
    b.append_f32(rows[:1500])
    b.append_f32(rows[1500:])
    assert b._i8_heavy == H and b.rows_i8.shape == (n_alloc, D + H)
    assert b._i8_store.numel() == n_alloc * (D + H)
    assert b.sx_i8 is sx and b.i8_bounds is bounds
    # the image is the reference's, in the shard's basis
    from codename_symbiont_amd.ops.reference import quant_rows_split_ref

    img, sc, _ = quant_rows_split_ref(b._rotate(b.rows[:b.count]), H)
    assert torch.equal(b.rows_i8[:b.count], img) and torch.allclose(b.sx_i8[:b.count], sc)

    b.i8_split = "off"
    b.calibrate_prune()
    assert b._i8_heavy == 0 and b._i8_store.numel() == _plain_bytes(b)
    assert (b.img_i8 is not None) if i8k == "stream" else b.rows_i8.shape == (n_alloc, D)
    assert b.sx_i8 is sx and b.i8_bounds is bounds
    # ... and the plain image bounds every pair again
    q = g.unit(16, seed=5).bfloat16()
    q8, sq, m = b.prune_query_image(q)
    s = q.float() @ b.rows[:b.count].float().t()
    assert ((s - b.prune_estimate(q8, sq)).abs() <= m[:, None]).all()


def test_384_store_and_heavy_are_unchanged(monkeypatch):
    monkeypatch.setenv("SYMB_I8_SPLIT", "auto")
    sh = HbmIndexShard(384, 3000, device="cpu", prune="i8")
    n_alloc = sh.sx_i8.shape[0]
    assert sh._i8_store.numel() == n_alloc * 448
    size = sh._i8_store.numel()
    sh.append_f32(CorpusGen("anisotropic", 384, "cpu").rows(2500, seed=1))
    sh.calibrate_prune()
    assert sh._i8_heavy == 64 and sh.rows_i8.shape == (n_alloc, 448)
    assert sh._i8_store.numel() == size
