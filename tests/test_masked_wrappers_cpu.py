"""The seven masked-scan wrappers share their checks (ops/kernels.py: _masked_scan_checks and the
two families' own): every one of them bounds the pointers its kernel dereferences -- ``n_valid``,
``n_live``, ``gate`` -- before it asks the extension for anything.  Host tensors, no extension."""
import pytest
import torch

from codename_symbiont_amd.ops import kernels as K

D, N, NQ, CAP, KMAX, N_RBLK = 384, 640, 5, 64, 16, 2
NW = N // 64


def _operands(fp8: bool, grouped: bool, emit: bool) -> dict:
    dt = torch.uint8 if fp8 else torch.bfloat16
    rows, q = ("rows_u8", "q_e4m3") if fp8 else ("rows", "q_unit")
    width = CAP if emit else N_RBLK * 8 * KMAX      # (8 lists: no bf16 geometry has more)
    a = {rows: torch.zeros(N, D, dtype=dt), "n_valid": N, q: torch.zeros(NQ, D, dtype=dt),
         "tiles": torch.zeros(NW, dtype=torch.int32), "n_live": torch.zeros(1, dtype=torch.int32),
         "cand_s": torch.zeros(NQ, width), "cand_i": torch.zeros(NQ, width, dtype=torch.int32),
         "n_rblk": N_RBLK}
    if grouped:
        a.update(mask8=torch.zeros(NW, 8, dtype=torch.int64),
                 qgroup=torch.zeros(NQ, dtype=torch.int32))
    else:
        a.update(mask_words=torch.zeros(NW, dtype=torch.int64))
    if emit:
        a.update(thr=torch.zeros(NQ), cand_n=torch.zeros(NQ, dtype=torch.int32), cap=CAP)
    else:
        a.update(kmax=KMAX)
    return a


# wrapper, fp8, grouped, emitting, further arguments
WRAPPERS = (
    ("index_scan_filter", False, False, False, {}),
    ("index_scan_filter_group", False, True, False, {}),
    ("index_scan_mq_filter", False, False, True, dict(sets=4, rsplit=2)),
    ("index_scan_filter_fp8", True, False, False, {}),
    ("index_scan_filter_group_fp8", True, True, False, {}),
    ("index_scan_emit_fp8", True, False, True, {}),
    ("index_scan_emit_group_fp8", True, True, True, {}),
)


@pytest.fixture
def host_only(monkeypatch):
    """``K.hip`` raises, and ``_chk`` passes host tensors (its other checks stay)."""
    def hip():
        raise AssertionError("the wrapper loaded the extension")

    def chk(t, dtype, name, ndim=None):
        if t.dtype != dtype:
            raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")
        if ndim is not None and t.dim() != ndim:
            raise ValueError(f"{name}: expected {ndim}-d, got {tuple(t.shape)}")

    monkeypatch.setattr(K, "hip", hip)
    monkeypatch.setattr(K, "_chk", chk)


@pytest.mark.parametrize("name,fp8,grouped,emit,more", WRAPPERS, ids=[w[0] for w in WRAPPERS])
def test_every_wrapper_bounds_what_its_kernel_dereferences(host_only, name, fp8, grouped, emit,
                                                           more):
    call = getattr(K, name)
    ok = {**_operands(fp8, grouped, emit), **more}
    for what, match, kw in (
            ("negative n_valid", "n_valid >= 0" if emit else "shorter than n_valid",
             dict(n_valid=-1)),
            ("empty n_live", "n_rblk >= 1" if emit else "shorter than n_valid",
             dict(n_live=torch.zeros(0, dtype=torch.int32))),
            ("empty gate", "one int32 flag", dict(gate=torch.zeros(0, dtype=torch.int32)))):
        # ValueError, and not the AssertionError of a wrapper that went on to the extension
        with pytest.raises(ValueError, match=f"^{name}: .*{match}"):
            call(**{**ok, **kw})
        assert what
    if fp8:     # with every check passed, the e4m3 wrappers go on to the extension
        with pytest.raises(AssertionError, match="loaded the extension"):
            call(**ok)
        with pytest.raises(AssertionError, match="loaded the extension"):
            call(**{**ok, "gate": torch.ones(1, dtype=torch.int32)})
