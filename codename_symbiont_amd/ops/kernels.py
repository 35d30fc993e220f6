"""Typed torch-tensor front-ends for the CDNA4 HIP kernels.

Each wrapper validates shapes/dtypes/devices on the host BEFORE launching (a malformed launch of a
hand-written kernel can fault the GPU), then calls the native launcher with raw pointers on the
current HIP stream.  Numerics of every op are pinned against the fp32 PyTorch oracles in
``codename_symbiont_amd.ops.reference`` by ``tests/test_kernels_gpu.py``.
"""
from __future__ import annotations

import torch

from ._ext import hip, stream_handle

EPI_BIAS, EPI_GELU, EPI_RES, EPI_RES_LN = 0, 1, 2, 3
LNF_FOLD, LNF_RESLN, LNF_STATS = 1, 2, 4    # deferred-LayerNorm epilogue modes (gemm.hip)
SUPPORTED_H = (384, 768, 1024)


def fold_ln(w: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    """Fold a LayerNorm that precedes a linear layer into it (the deferred LayerNorm, gemm.hip
    LNF_FOLD): LN(y) W^T + b = rstd (y W'^T - mean cs) + b' with W' = W o gamma (bf16 [N, K]),
    cs = rowsum(W') (f32 [N], from the rounded W'), b' = b + W beta (f32 [N])."""
    wf = w.float()
    wg = (wf * gamma.float()[None, :]).to(torch.bfloat16).contiguous()
    cs = wg.float().sum(1).contiguous()
    bf = (b.float() + wf @ beta.float()).contiguous()
    return wg, bf, cs


def gemm_ln(a, w, bias, epi, lnf, residual=None, gamma=None, beta=None, ln_eps=1e-12, cs=None,
            st_in=None, st_out=None, out=None):
    """Deferred-LayerNorm GEMM (gemm.hip symb_gemm_ln): st_in / st_out are float32 [M, N / 64, 2]
    row-statistics partials (chunk mean, squared deviations); see gemm_bf16_kernel's LNF modes."""
    _chk(a, torch.bfloat16, "a", 2)
    _chk(w, torch.bfloat16, "w", 2)
    _chk(bias, torch.float32, "bias", 1)
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or bias.numel() != N or K % 64 or N % 128:
        raise ValueError("gemm_ln: shapes")
    np_in = 0
    if lnf & (LNF_FOLD | LNF_RESLN):
        _chk(st_in, torch.float32, "st_in", 3)
        if st_in.shape[0] != M or st_in.shape[2] != 2:
            raise ValueError("st_in: [M, np, 2]")
        np_in = st_in.shape[1]
    if lnf & LNF_FOLD:
        _chk(cs, torch.float32, "cs", 1)
        if cs.numel() != N:
            raise ValueError("cs: [N]")
    if lnf & LNF_RESLN or epi == EPI_RES:
        _chk(residual, torch.bfloat16, "residual", 2)
        if residual.shape != (M, N):
            raise ValueError("residual: [M, N]")
    if lnf & LNF_STATS:
        _chk(st_out, torch.float32, "st_out", 3)
        if st_out.shape != (M, N // 64, 2):
            raise ValueError("st_out: [M, N / 64, 2]")
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    hip().gemm_ln(epi, lnf, _ptr(a), K, _ptr(w), K, _ptr(bias), _ptr(residual), N, _ptr(gamma),
                  _ptr(beta), float(ln_eps), _ptr(cs), _ptr(st_in), np_in, _ptr(st_out), _ptr(out),
                  N, M, N, K, stream_handle())
    return out


def _ptr(t: torch.Tensor | None) -> int:
    return 0 if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype: torch.dtype, name: str, ndim: int | None = None) -> None:
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name}: must be a device tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim}-d, got {tuple(t.shape)}")


def embed_ln(ids, pos, type_ids, wemb, pemb, temb, gamma, beta, eps, out=None):
    T = ids.numel()
    H = wemb.shape[1]
    if H not in SUPPORTED_H:
        raise ValueError(f"hidden {H} unsupported")
    for t, n in ((ids, "ids"), (pos, "pos")):
        _chk(t, torch.int32, n, 1)
    if type_ids is not None:
        _chk(type_ids, torch.int32, "type_ids", 1)
    for t, n in ((wemb, "wemb"), (pemb, "pemb"), (temb, "temb")):
        _chk(t, torch.bfloat16, n, 2)
    _chk(gamma, torch.float32, "gamma", 1)
    _chk(beta, torch.float32, "beta", 1)
    if out is None:
        out = torch.empty(T, H, dtype=torch.bfloat16, device=ids.device)
    hip().embed_ln(_ptr(ids), _ptr(pos), _ptr(type_ids), _ptr(wemb), _ptr(pemb), _ptr(temb),
                   _ptr(gamma), _ptr(beta), float(eps), _ptr(out), T, H, stream_handle())
    return out


def add_ln(x, res, gamma, beta, eps, out=None):
    _chk(x, torch.bfloat16, "x", 2)
    T, H = x.shape
    if H not in SUPPORTED_H:
        raise ValueError(f"hidden {H} unsupported")
    if res is not None:
        _chk(res, torch.bfloat16, "res", 2)
        assert res.shape == x.shape
    if out is None:
        out = torch.empty_like(x)
    hip().add_ln(_ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), float(eps), _ptr(out), T, H,
                 stream_handle())
    return out


def gemm(a, w, bias, epi=EPI_BIAS, residual=None, gamma=None, beta=None, eps=1e-12, out=None):
    """out = epi(a @ w.T + bias) with a:[M,K] bf16, w:[N,K] bf16, bias:[N] fp32."""
    _chk(a, torch.bfloat16, "a", 2)
    _chk(w, torch.bfloat16, "w", 2)
    _chk(bias, torch.float32, "bias", 1)
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise ValueError(f"K mismatch {K} vs {K2}")
    if K % 64:
        raise ValueError("K must be a multiple of 64")
    if epi == EPI_RES_LN:
        # 384-wide row-complete tiles, or any width <= 4096 on the small-M path's split-sum kernel
        if N != 384 and not (M <= hip().gemm_skinny_max_m() and N % 64 == 0 and N <= 4096):
            raise ValueError("fused LayerNorm epilogue needs N == 384 or M <= the small-M "
                             "limit (else EPI_RES + add_ln)")
    elif N % 128:
        raise ValueError("N must be a multiple of 128")
    if epi in (EPI_RES, EPI_RES_LN):
        _chk(residual, torch.bfloat16, "residual", 2)
        assert residual.shape == (M, N)
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    hip().gemm(epi, _ptr(a), K, _ptr(w), K, _ptr(bias), _ptr(residual), N, _ptr(gamma),
               _ptr(beta), float(eps), _ptr(out), N, M, N, K, stream_handle())
    return out


def mlp_fused(x, w1, b1, w2, b2, gamma, beta, eps=1e-12, out=None):
    """out = LayerNorm(GELU(x @ w1.T + b1) @ w2.T + b2 + x) in one launch (mlp_fused.hip;
    x: [M, 384] bf16, w1: [1536, 384], w2: [384, 1536] bf16; the intermediate is rounded to bf16
    as the two-GEMM path stores it)."""
    _chk(x, torch.bfloat16, "x", 2)
    _chk(w1, torch.bfloat16, "w1", 2)
    _chk(w2, torch.bfloat16, "w2", 2)
    M, H = x.shape
    FF = w1.shape[0]
    if (H, FF) != (384, 1536) or w1.shape != (FF, H) or w2.shape != (H, FF):
        raise ValueError("mlp_fused takes H = 384, FF = 1536")
    for t, n in ((b1, FF), (b2, H), (gamma, H), (beta, H)):
        _chk(t, torch.float32, "vector", 1)
        if t.shape[0] != n:
            raise ValueError("mlp_fused: vector length")
    if out is None:
        out = torch.empty(M, H, dtype=torch.bfloat16, device=x.device)
    if out.shape != (M, H) or not out.is_contiguous() or out.data_ptr() == x.data_ptr():
        raise ValueError("mlp_fused: bad output")
    hip().mlp_fused(_ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(gamma), _ptr(beta),
                    float(eps), _ptr(out), M, H, FF, stream_handle())
    return out


def attention(qkv, cu_seqlens, max_len, n_heads, head_dim, out=None):
    """Varlen attention over packed [T, 3H] QKV rows -> [T, H]."""
    _chk(qkv, torch.bfloat16, "qkv", 2)
    _chk(cu_seqlens, torch.int32, "cu_seqlens", 1)
    T, H3 = qkv.shape
    H = n_heads * head_dim
    if H3 != 3 * H or head_dim not in (32, 64):
        raise ValueError("bad attention geometry")
    B = cu_seqlens.numel() - 1
    if out is None:
        out = torch.empty(T, H, dtype=torch.bfloat16, device=qkv.device)
    hip().attention(_ptr(qkv), H3, _ptr(cu_seqlens), B, int(max_len), n_heads, head_dim,
                    _ptr(out), H, stream_handle())
    return out


def qkv_attention(x, wqkv, bqkv, cu_seqlens, max_len, n_heads, head_dim, out=None):
    """The QKV projection fused into varlen attention (attention.hip qkv_attn_kernel): x [T, H]
    bf16, wqkv [3H, H] bf16, bqkv [3H] f32 -> [T, H].  head_dim 32 / 12 heads, sentences of at
    most 128 tokens (the kernel raises otherwise)."""
    _chk(x, torch.bfloat16, "x", 2)
    _chk(wqkv, torch.bfloat16, "wqkv", 2)
    _chk(bqkv, torch.float32, "bqkv", 1)
    _chk(cu_seqlens, torch.int32, "cu_seqlens", 1)
    T, H = x.shape
    if wqkv.shape != (3 * H, H) or bqkv.numel() != 3 * H or H != n_heads * head_dim:
        raise ValueError("bad qkv_attention geometry")
    B = cu_seqlens.numel() - 1
    if out is None:
        out = torch.empty(T, H, dtype=torch.bfloat16, device=x.device)
    hip().qkv_attention(_ptr(x), _ptr(wqkv), _ptr(bqkv), _ptr(cu_seqlens), B, int(max_len),
                        n_heads, head_dim, _ptr(out), stream_handle())
    return out


def pool(hidden, cu_seqlens, mode="mean", normalize=False, want_normed_bf16=True):
    """Returns (pooled_f32 [B,H], unit_bf16 [B,H] or None)."""
    _chk(hidden, torch.bfloat16, "hidden", 2)
    _chk(cu_seqlens, torch.int32, "cu_seqlens", 1)
    T, H = hidden.shape
    B = cu_seqlens.numel() - 1
    out = torch.empty(B, H, dtype=torch.float32, device=hidden.device)
    normed = torch.empty(B, H, dtype=torch.bfloat16, device=hidden.device) if want_normed_bf16 else None
    hip().pool(_ptr(hidden), _ptr(cu_seqlens), B, H, 0 if mode == "mean" else 1,
               1 if normalize else 0, _ptr(out), _ptr(normed), stream_handle())
    return out, normed


def l2norm_cast(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Unit-normalise f32 rows into bf16 rows (out may be a row-slice of an index slab)."""
    _chk(x, torch.float32, "x", 2)
    n, D = x.shape
    if D % 4:
        raise ValueError("D must be a multiple of 4")
    if out is None:
        out = torch.empty(n, D, dtype=torch.bfloat16, device=x.device)
    if out.dtype != torch.bfloat16 or out.shape[0] < n or out.shape[1] != D or out.stride(1) != 1:
        raise ValueError("bad l2norm_cast output")
    hip().l2norm_cast(_ptr(x), _ptr(out), n, D, out.stride(0), stream_handle())
    return out


FP8_SCALE = 256.0  # global index/query scale: unit vectors -> |S x_i| <= 256 < 448 (e4m3 max)


def quant_fp8(x: torch.Tensor, out: torch.Tensor | None = None, scale: float = FP8_SCALE,
              normalize: bool = False) -> torch.Tensor:
    """Rows (f32 or bf16) -> OCP e4m3 bytes of scale * x (optionally unit-normalised first).
    ``out`` is a uint8 [n, D] tensor (may be a row-slice of an fp8 index slab)."""
    if x.dtype not in (torch.float32, torch.bfloat16) or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("quant_fp8 expects a row-major f32/bf16 matrix")
    if not x.is_cuda:
        raise ValueError("quant_fp8 runs on the GPU")
    n, D = x.shape
    if D % 8 or D > 1024:
        raise ValueError("D must be a multiple of 8 and <= 1024")
    if out is None:
        out = torch.empty(n, D, dtype=torch.uint8, device=x.device)
    if out.dtype != torch.uint8 or out.shape[0] < n or out.shape[1] != D or out.stride(1) != 1:
        raise ValueError("bad quant_fp8 output")
    hip().quant_fp8(_ptr(x), x.dtype == torch.float32, x.stride(0), _ptr(out), out.stride(0), n, D,
                    float(scale), bool(normalize), stream_handle())
    return out


def fp8_to_float(b: torch.Tensor, scale: float = FP8_SCALE) -> torch.Tensor:
    """Reference decode of e4m3 bytes (torch float8_e4m3fn == gfx950's OCP format)."""
    return b.view(torch.float8_e4m3fn).float() / scale


FILTER_DIMS = (384, 768, 1024)   # row widths of the masked scan (index_filter.hip)


def filter_tiles(mask_words: torch.Tensor, n_valid: int):
    """Packed row mask (int64 words, bit r % 64 of word r // 64 = row r allowed) -> (tiles int32
    [max(n_words, 1)], n_live int32 [1]): the ascending 64-row tiles that hold an allowed row
    below ``n_valid`` and their count, both left on the device (nothing is read back)."""
    _chk(mask_words, torch.int64, "mask_words", 1)
    n_words = mask_words.numel()
    n_valid = int(n_valid)
    if n_valid < 0 or (n_valid + 63) // 64 > n_words:
        raise ValueError(f"filter_tiles: {n_words} mask words do not cover {n_valid} rows")
    dev = mask_words.device
    tiles = torch.empty(max(n_words, 1), dtype=torch.int32, device=dev)
    n_live = torch.empty(1, dtype=torch.int32, device=dev)
    blk_cnt = torch.empty(256, dtype=torch.int32, device=dev)
    hip().filter_tiles(_ptr(mask_words), n_words, n_valid, _ptr(blk_cnt), _ptr(tiles),
                       _ptr(n_live), stream_handle(dev))
    return tiles, n_live


MASK_GROUPS = 8   # masks one grouped scan carries: mask words per tile (index_*_group*.hip)
FILTER_LARGE_K_DIMS = (384, 768, 1024)   # ... of the masked emitting scan (index_mq_filter.hip)
# (sets, rsplit) forms it is built for, per width
_MQ_FILTER_FORMS = {384: ((4, 1), (4, 2)), 768: ((2, 1),), 1024: ((1, 1),)}
FILTER_FP8_DIMS = (256, 384, 512, 768, 1024)   # ... of the e4m3 forms (index_filter_fp8.hip, ...)


def _masked_scan_checks(name, dtype, dims, rows, n_valid, mask, qgroup, tiles, n_live, q, cand_s,
                        cand_i, gate, scalars):
    """What the seven masked scans check alike; returns (D, NQ).  ``dtype``: the rows' and the
    queries' (uint8: e4m3 bytes); ``mask`` / ``qgroup``: mask words and None, or mask8 and the
    queries' groups; ``scalars``: the family's refusal of its scalar arguments, or None where
    they are in range.  Every pointer the kernels dereference is bounded here: the slab, the
    mask and the tile list cover ``n_valid``, ``n_live`` and ``gate`` hold an element."""
    fp8 = dtype == torch.uint8
    if fp8 and (rows.dtype != torch.uint8 or q.dtype != torch.uint8):
        # (a bf16 slab of the same width would be read as twice as many e4m3 rows)
        raise ValueError(f"{name}: rows and queries are e4m3 bytes (uint8), got "
                         f"{rows.dtype} / {q.dtype}")
    _chk(rows, dtype, "rows_u8" if fp8 else "rows", 2)
    _chk(q, dtype, "q_e4m3" if fp8 else "q_unit", 2)
    if qgroup is None:
        _chk(mask, torch.int64, "mask_words", 1)
    else:
        _chk(mask, torch.int64, "mask8", 2)
        _chk(qgroup, torch.int32, "qgroup", 1)
    _chk(tiles, torch.int32, "tiles", 1)
    _chk(n_live, torch.int32, "n_live", 1)
    _chk(cand_s, torch.float32, "cand_s")
    _chk(cand_i, torch.int32, "cand_i")
    D, NQ = rows.shape[1], q.shape[0]
    if D not in dims or q.shape[1] != D:
        raise ValueError(f"{name}: rows must be {dims} wide, queries alike")
    if scalars is not None:
        raise ValueError(f"{name}: {scalars}")
    what = "mask"
    if qgroup is not None:
        what = "mask8"
        if mask.shape[1] != MASK_GROUPS or not mask.is_contiguous():
            raise ValueError(f"{name}: mask8 must be contiguous [n_words, {MASK_GROUPS}]")
        if qgroup.numel() != NQ:
            raise ValueError(f"{name}: qgroup must hold one group per query")
    n_tiles = (n_valid + 63) // 64
    # every tile the list can name lies inside the row slab and has its mask word(s)
    if (n_valid < 0 or n_live.numel() < 1 or n_tiles * 64 > rows.shape[0]
            or n_tiles > mask.shape[0] or n_tiles > tiles.numel()):
        raise ValueError(f"{name}: rows / {what} / tile list shorter than n_valid")
    if gate is not None:
        _chk(gate, torch.int32, "gate", 1)
        if gate.numel() < 1:
            raise ValueError(f"{name}: gate is one int32 flag")
    return D, NQ


def _list_scan_checks(name, dtype, dims, rows, n_valid, mask, qgroup, tiles, n_live, q, kmax,
                      n_rblk, cand_s, cand_i, thr_init, stride, gate):
    """The checks of a masked list scan; returns (D, NQ).  Only the bf16 scans' workspace size
    asks the extension for anything (``topk_geometry``), after every other check of the
    operands; an e4m3 scan keeps 2 lists at every width."""
    ok = kmax in (16, 32) and stride >= 1 and n_rblk >= 1
    D, NQ = _masked_scan_checks(name, dtype, dims, rows, n_valid, mask, qgroup, tiles, n_live, q,
                                cand_s, cand_i, gate,
                                None if ok else "kmax in (16, 32), stride >= 1, n_rblk >= 1")
    if thr_init is not None:
        _chk(thr_init, torch.float32, "thr_init", 1)
        if thr_init.numel() < NQ:
            raise ValueError(f"{name}: thr_init shorter than the batch")
    lists = 2 if dtype == torch.uint8 else hip().topk_geometry(D, kmax)[0]
    need = NQ * n_rblk * lists * kmax
    if cand_s.numel() < need or cand_i.numel() < need:
        raise ValueError(f"{name}: candidate workspace too small")
    return D, NQ


def _emit_scan_checks(name, dtype, dims, rows, n_valid, mask, qgroup, tiles, n_live, q, thr,
                      cand_s, cand_i, cand_n, cap, n_rblk, gate, thr_exact):
    """The checks of a masked emitting scan; returns (D, NQ).  ``thr_exact``: ``thr`` holds NQ
    thresholds, no more (the e4m3 scans; the bf16 scan takes a longer ``thr``)."""
    ok = n_rblk >= 1 and cap >= 1 and n_valid >= 0 and n_live.numel() >= 1
    D, NQ = _masked_scan_checks(name, dtype, dims, rows, n_valid, mask, qgroup, tiles, n_live, q,
                                cand_s, cand_i, gate,
                                None if ok else "n_rblk >= 1, cap >= 1, n_valid >= 0")
    if thr is None or thr.dtype != torch.float32:
        raise ValueError(f"{name}: thr is a float32 tensor, one threshold per query")
    _chk(thr, torch.float32, "thr", 1)
    _chk(cand_n, torch.int32, "cand_n", 1)
    if thr.numel() != NQ if thr_exact else thr.numel() < NQ:
        raise ValueError(f"{name}: one threshold per query" if thr_exact
                         else f"{name}: thr shorter than the batch")
    if cand_n.numel() < NQ:
        raise ValueError(f"{name}: cand_n shorter than the batch")
    if cand_s.numel() < NQ * cap or cand_i.numel() < NQ * cap:
        raise ValueError(f"{name}: candidate workspace too small")
    return D, NQ


def index_scan_filter(rows: torch.Tensor, n_valid: int, mask_words: torch.Tensor,
                      tiles: torch.Tensor, n_live: torch.Tensor, q_unit: torch.Tensor, kmax: int,
                      n_rblk: int, cand_s: torch.Tensor, cand_i: torch.Tensor,
                      thr_init: torch.Tensor | None = None, stride: int = 1, xcd: int = 1,
                      gate: torch.Tensor | None = None) -> None:
    """The masked list scan: candidates [NQ][n_rblk][lists][kmax] (``topk_geometry``) of the
    allowed rows below ``n_valid``, for ``topk_merge``.  ``tiles`` / ``n_live`` are
    ``filter_tiles(mask_words, n_valid)``; ``stride`` walks every stride-th live tile of each
    workgroup's slice only (a seed pass).  ``gate`` (int32 device flag): the scan runs only if
    it is non-zero, and leaves the candidates untouched otherwise."""
    n_valid, n_rblk, stride = int(n_valid), int(n_rblk), int(stride)
    D, NQ = _list_scan_checks("index_scan_filter", torch.bfloat16, FILTER_DIMS, rows, n_valid,
                              mask_words, None, tiles, n_live, q_unit, kmax, n_rblk, cand_s,
                              cand_i, thr_init, stride, gate)
    hip().index_scan_filter(_ptr(rows), n_valid, D, _ptr(tiles), _ptr(n_live), _ptr(mask_words),
                            stride, n_rblk, _ptr(q_unit), NQ, kmax, _ptr(cand_s), _ptr(cand_i),
                            stream_handle(rows.device), _ptr(thr_init), xcd, _ptr(gate))


def index_scan_filter_group(rows: torch.Tensor, n_valid: int, mask8: torch.Tensor,
                            qgroup: torch.Tensor, tiles: torch.Tensor, n_live: torch.Tensor,
                            q_unit: torch.Tensor, kmax: int, n_rblk: int, cand_s: torch.Tensor,
                            cand_i: torch.Tensor, thr_init: torch.Tensor | None = None,
                            stride: int = 1, xcd: int = 1,
                            gate: torch.Tensor | None = None) -> None:
    """``index_scan_filter`` under a mask per query: ``mask8`` int64 [n_words, 8] holds, for
    each 64-row tile, the mask word of each of up to 8 groups (unused slots 0), and ``qgroup``
    int32 [NQ] names each query's group (its low three bits are used).  ``tiles`` / ``n_live``
    are ``filter_tiles`` of the OR of the eight slots.  Query q's candidates are those of
    ``index_scan_filter`` under slot ``qgroup[q]``'s words, scored bit for bit alike."""
    n_valid, n_rblk, stride = int(n_valid), int(n_rblk), int(stride)
    D, NQ = _list_scan_checks("index_scan_filter_group", torch.bfloat16, FILTER_DIMS, rows,
                              n_valid, mask8, qgroup, tiles, n_live, q_unit, kmax, n_rblk, cand_s,
                              cand_i, thr_init, stride, gate)
    hip().index_scan_filter_group(_ptr(rows), n_valid, D, _ptr(tiles), _ptr(n_live), _ptr(mask8),
                                  _ptr(qgroup), stride, n_rblk, _ptr(q_unit), NQ, kmax,
                                  _ptr(cand_s), _ptr(cand_i), stream_handle(rows.device),
                                  _ptr(thr_init), xcd, _ptr(gate))


def index_scan_mq_filter(rows: torch.Tensor, n_valid: int, mask_words: torch.Tensor,
                         tiles: torch.Tensor, n_live: torch.Tensor, q_unit: torch.Tensor,
                         thr: torch.Tensor, cand_s: torch.Tensor, cand_i: torch.Tensor,
                         cand_n: torch.Tensor, cap: int, n_rblk: int, sets: int, rsplit: int,
                         xcd: int = 1, gate: torch.Tensor | None = None,
                         zero_cnt: bool = True) -> None:
    """The masked emitting scan: every allowed row below ``n_valid`` scoring above ``thr[q]`` is
    appended to query q's candidates, ``cand_s`` / ``cand_i`` [NQ, cap] (score, physical row), and
    counted in ``cand_n`` [NQ] -- which may exceed ``cap``; nothing is written at or past it
    (``topk_select_counted`` raises its overflow flag then).  ``tiles`` / ``n_live`` are
    ``filter_tiles(mask_words, n_valid)``.  ``sets`` / ``rsplit``: the kernel form (16-query sets
    per wave, waves sharing a query group; 8 / rsplit * 16 * sets queries per workgroup); the
    grid is ``n_rblk`` row slots per query block, sharing the live tiles evenly.  ``zero_cnt``
    False appends to ``cand_n``.  ``gate`` (int32 device flag): scan and zeroing run only if it
    is non-zero, and leave every buffer untouched otherwise."""
    n_valid, n_rblk, cap = int(n_valid), int(n_rblk), int(cap)
    D, NQ = _emit_scan_checks("index_scan_mq_filter", torch.bfloat16, FILTER_LARGE_K_DIMS, rows,
                              n_valid, mask_words, None, tiles, n_live, q_unit, thr, cand_s,
                              cand_i, cand_n, cap, n_rblk, gate, thr_exact=False)
    if (int(sets), int(rsplit)) not in _MQ_FILTER_FORMS[D]:
        raise ValueError(f"index_scan_mq_filter: (sets, rsplit) at D = {D} is one of "
                         f"{_MQ_FILTER_FORMS[D]}")
    hip().index_scan_mq_filter(_ptr(rows), n_valid, _ptr(tiles), _ptr(n_live), _ptr(mask_words),
                               n_rblk, _ptr(q_unit), NQ, _ptr(thr), _ptr(cand_s), _ptr(cand_i),
                               _ptr(cand_n), cap, xcd, stream_handle(rows.device), int(sets),
                               int(rsplit), _ptr(gate), bool(zero_cnt), D)


def index_scan_filter_fp8(rows_u8: torch.Tensor, n_valid: int, mask_words: torch.Tensor,
                          tiles: torch.Tensor, n_live: torch.Tensor, q_e4m3: torch.Tensor,
                          kmax: int, n_rblk: int, cand_s: torch.Tensor, cand_i: torch.Tensor,
                          thr_init: torch.Tensor | None = None, stride: int = 1,
                          xcd: int = 1, gate: torch.Tensor | None = None) -> None:
    """The masked list scan over e4m3 rows (``quant_fp8`` bytes at FP8_SCALE) for e4m3 queries:
    candidates [NQ][n_rblk][2][kmax] of the allowed rows below ``n_valid``, for ``topk_merge``.
    Scores are raw accumulators (FP8_SCALE**2 * cosine) and ``thr_init`` is in the same units.
    ``tiles`` / ``n_live`` / ``stride`` / ``gate`` as in ``index_scan_filter``."""
    n_valid, n_rblk, stride = int(n_valid), int(n_rblk), int(stride)
    D, NQ = _list_scan_checks("index_scan_filter_fp8", torch.uint8, FILTER_FP8_DIMS, rows_u8,
                              n_valid, mask_words, None, tiles, n_live, q_e4m3, kmax, n_rblk,
                              cand_s, cand_i, thr_init, stride, gate)
    hip().index_scan_filter_fp8(_ptr(rows_u8), n_valid, D, _ptr(tiles), _ptr(n_live),
                                _ptr(mask_words), stride, n_rblk, _ptr(q_e4m3), NQ, kmax,
                                _ptr(cand_s), _ptr(cand_i), stream_handle(rows_u8.device),
                                _ptr(thr_init), xcd, _ptr(gate))


def index_scan_filter_group_fp8(rows_u8: torch.Tensor, n_valid: int, mask8: torch.Tensor,
                                qgroup: torch.Tensor, tiles: torch.Tensor, n_live: torch.Tensor,
                                q_e4m3: torch.Tensor, kmax: int, n_rblk: int,
                                cand_s: torch.Tensor, cand_i: torch.Tensor,
                                thr_init: torch.Tensor | None = None, stride: int = 1,
                                xcd: int = 1, gate: torch.Tensor | None = None) -> None:
    """``index_scan_filter_fp8`` under a mask per query (index_filter_group_fp8.hip): ``mask8``
    int64 [n_words, 8] and ``qgroup`` int32 [NQ] as in ``index_scan_filter_group``, ``tiles`` /
    ``n_live`` ``filter_tiles`` of the OR of the eight slots.  Query q's candidates
    [NQ][n_rblk][2][kmax] are those of ``index_scan_filter_fp8`` under slot ``qgroup[q]``'s
    words, raw accumulators scored bit for bit alike; ``thr_init`` in the same units."""
    n_valid, n_rblk, stride = int(n_valid), int(n_rblk), int(stride)
    D, NQ = _list_scan_checks("index_scan_filter_group_fp8", torch.uint8, FILTER_FP8_DIMS,
                              rows_u8, n_valid, mask8, qgroup, tiles, n_live, q_e4m3, kmax,
                              n_rblk, cand_s, cand_i, thr_init, stride, gate)
    hip().index_scan_filter_group_fp8(_ptr(rows_u8), n_valid, D, _ptr(tiles), _ptr(n_live),
                                      _ptr(mask8), _ptr(qgroup), stride, n_rblk, _ptr(q_e4m3), NQ,
                                      kmax, _ptr(cand_s), _ptr(cand_i),
                                      stream_handle(rows_u8.device), _ptr(thr_init), xcd,
                                      _ptr(gate))


def index_scan_emit_fp8(rows_u8: torch.Tensor, n_valid: int, mask_words: torch.Tensor,
                        tiles: torch.Tensor, n_live: torch.Tensor, q_e4m3: torch.Tensor,
                        thr: torch.Tensor, cand_s: torch.Tensor, cand_i: torch.Tensor,
                        cand_n: torch.Tensor, cap: int, n_rblk: int, xcd: int = 1,
                        gate: torch.Tensor | None = None, zero_cnt: bool = True) -> None:
    """The masked emitting scan over e4m3 rows (index_emit_fp8.hip): every allowed row below
    ``n_valid`` whose raw score (FP8_SCALE**2 * cosine, the list scan's own accumulator) lies
    above ``thr[q]`` is appended to query q's candidates, ``cand_s`` / ``cand_i`` [NQ, cap], and
    counted in ``cand_n`` [NQ] -- which may exceed ``cap``; nothing is written at or past it
    (``topk_select_counted`` raises its overflow flag then).  ``tiles`` / ``n_live`` are
    ``filter_tiles(mask_words, n_valid)``; the grid is ``n_rblk`` row slots per block of 256
    queries, sharing the live tiles evenly.  ``zero_cnt`` False appends to ``cand_n``.  ``gate``
    (int32 device flag): scan and zeroing run only if it is non-zero, and leave every buffer
    untouched otherwise."""
    n_valid, n_rblk, cap = int(n_valid), int(n_rblk), int(cap)
    D, NQ = _emit_scan_checks("index_scan_emit_fp8", torch.uint8, FILTER_FP8_DIMS, rows_u8,
                              n_valid, mask_words, None, tiles, n_live, q_e4m3, thr, cand_s,
                              cand_i, cand_n, cap, n_rblk, gate, thr_exact=True)
    hip().index_scan_emit_fp8(_ptr(rows_u8), n_valid, D, _ptr(tiles), _ptr(n_live),
                              _ptr(mask_words), n_rblk, _ptr(q_e4m3), NQ, _ptr(thr),
                              _ptr(cand_s), _ptr(cand_i), _ptr(cand_n), cap,
                              stream_handle(rows_u8.device), xcd, _ptr(gate), bool(zero_cnt))


def index_scan_emit_group_fp8(rows_u8: torch.Tensor, n_valid: int, mask8: torch.Tensor,
                              qgroup: torch.Tensor, tiles: torch.Tensor, n_live: torch.Tensor,
                              q_e4m3: torch.Tensor, thr: torch.Tensor, cand_s: torch.Tensor,
                              cand_i: torch.Tensor, cand_n: torch.Tensor, cap: int, n_rblk: int,
                              xcd: int = 1, gate: torch.Tensor | None = None,
                              zero_cnt: bool = True) -> None:
    """``index_scan_emit_fp8`` under a mask per query (index_emit_group_fp8.hip): ``mask8`` int64
    [n_words, 8] and ``qgroup`` int32 [NQ] as in ``index_scan_filter_group_fp8``, ``tiles`` /
    ``n_live`` ``filter_tiles`` of the OR of the eight slots.  Query q's candidates are those of
    ``index_scan_emit_fp8`` under slot ``qgroup[q]``'s words: every row that slot allows below
    ``n_valid`` whose raw score, bit for bit the list scans', lies above ``thr[q]``.
    ``cand_s`` / ``cand_i`` [NQ, cap], ``cand_n`` [NQ] (may exceed ``cap``; nothing is written at
    or past it), ``zero_cnt`` and ``gate`` as there."""
    n_valid, n_rblk, cap = int(n_valid), int(n_rblk), int(cap)
    D, NQ = _emit_scan_checks("index_scan_emit_group_fp8", torch.uint8, FILTER_FP8_DIMS, rows_u8,
                              n_valid, mask8, qgroup, tiles, n_live, q_e4m3, thr, cand_s, cand_i,
                              cand_n, cap, n_rblk, gate, thr_exact=True)
    hip().index_scan_emit_group_fp8(_ptr(rows_u8), n_valid, D, _ptr(tiles), _ptr(n_live),
                                    _ptr(mask8), _ptr(qgroup), n_rblk, _ptr(q_e4m3), NQ,
                                    _ptr(thr), _ptr(cand_s), _ptr(cand_i), _ptr(cand_n), cap,
                                    stream_handle(rows_u8.device), xcd, _ptr(gate),
                                    bool(zero_cnt))


def tombstone_rows(rows_list: torch.Tensor, n_valid: int, dead_words: torch.Tensor,
                   slab: torch.Tensor, slab2: torch.Tensor | None = None) -> None:
    """Tombstone the listed rows (index_delete.hip): zeros over each row of ``slab`` (and of
    ``slab2``, e.g. a shard's e4m3 prefilter image) and the row's bit set in ``dead_words`` (int64,
    bit r % 64 of word r // 64, as a RowMask packs).  ``rows_list``: distinct int32 rows on the
    device; entries outside [0, n_valid) are skipped.  Slabs are [>= n_valid, D] of 1- or 2-byte
    elements, D a multiple of 8."""
    _chk(rows_list, torch.int32, "rows_list", 1)
    _chk(dead_words, torch.int64, "dead_words", 1)
    n_valid = int(n_valid)
    D = slab.shape[-1]
    for name, t in (("slab", slab), ("slab2", slab2)):
        if t is None:
            continue
        if t.element_size() not in (1, 2):
            raise TypeError(f"tombstone_rows: {name} must hold 1- or 2-byte elements, got {t.dtype}")
        _chk(t, t.dtype, name, 2)
        # the list cannot name a row past the slab: every row below n_valid lies inside it
        if t.shape[1] != D or D % 8 or t.shape[0] < n_valid or t.device != rows_list.device:
            raise ValueError(f"tombstone_rows: {name} {tuple(t.shape)} does not hold {n_valid} "
                             f"rows of width {D} (a multiple of 8) on {rows_list.device}")
    if n_valid < 0 or (n_valid + 63) // 64 > dead_words.numel():
        raise ValueError(f"tombstone_rows: {dead_words.numel()} bitmap words do not cover "
                         f"{n_valid} rows")
    if dead_words.device != rows_list.device:
        raise ValueError("tombstone_rows: bitmap and row list on different devices")
    hip().tombstone_rows(_ptr(rows_list), rows_list.numel(), n_valid, _ptr(slab),
                         slab.element_size(), _ptr(slab2),
                         0 if slab2 is None else slab2.element_size(), D, _ptr(dead_words),
                         stream_handle(rows_list.device))


def results_dead(ids: torch.Tensor, dead_words: torch.Tensor, hits: torch.Tensor) -> None:
    """``hits[0]`` += the number of entries of ``ids`` (int32, a search's [NQ, k] rows) that are
    >= 0 and set in the ``dead_words`` bitmap (int64); the caller zeroes ``hits`` (int32 [1]).
    ``-1`` ids and ids past the bitmap count nothing.  Nothing is read back."""
    _chk(ids, torch.int32, "ids")
    _chk(dead_words, torch.int64, "dead_words", 1)
    _chk(hits, torch.int32, "hits", 1)
    if hits.numel() < 1:
        raise ValueError("results_dead: hits must hold one int32")
    if ids.device != dead_words.device or ids.device != hits.device:
        raise ValueError("results_dead: ids, bitmap and flag on different devices")
    hip().results_dead(_ptr(ids), ids.numel(), _ptr(dead_words), dead_words.numel(), _ptr(hits),
                       stream_handle(ids.device))


def compact_rows(dead_words: torch.Tensor, tile_dst: torch.Tensor, t0: int, t1: int, n_valid: int,
                 slab: torch.Tensor, stage: torch.Tensor | None = None,
                 slab2: torch.Tensor | None = None, stage2: torch.Tensor | None = None,
                 n_rows: int = 0) -> None:
    """Move the live rows of source tiles [t0, t1) (64 rows each) of one compaction window
    (index_compact.hip; the windows come from index.shard.compact_plan).  ``dead_words``: the
    tombstone bitmap (int64, bit r % 64 of word r // 64); ``tile_dst``: int32 [>= n_tiles + 1],
    tile_dst[t] = the new row of tile t's first live row; rows at or past ``n_valid`` are not live.

    ``stage`` None = a direct window: the rows go to ``slab[tile_dst[t] + rank]`` (the plan
    guarantees every destination lies below the window).  Otherwise a staged window: they are
    gathered into ``stage[tile_dst[t] - tile_dst[t0] + rank]`` and the caller copies
    ``stage[:n_rows]`` to ``slab[tile_dst[t0]:tile_dst[t1]]`` behind this call; ``n_rows`` is that
    row count from the host's plan and must fit the staging buffer.  ``slab2`` / ``stage2``: a
    second slab moved the same way in the same launch (a shard's e4m3 prefilter image).  Slabs are
    [>= n_valid, D] of 1- or 2-byte elements, D a multiple of 8."""
    _chk(dead_words, torch.int64, "dead_words", 1)
    _chk(tile_dst, torch.int32, "tile_dst", 1)
    t0, t1, n_valid, n_rows = int(t0), int(t1), int(n_valid), int(n_rows)
    dev, D = slab.device, slab.shape[-1]
    n_tiles = (n_valid + 63) // 64
    if n_valid <= 0 or not 0 <= t0 < t1 <= n_tiles:
        raise ValueError(f"compact_rows: window [{t0}, {t1}) outside the {n_tiles} tiles of "
                         f"{n_valid} rows")
    if dead_words.numel() < n_tiles or tile_dst.numel() < n_tiles + 1:
        raise ValueError(f"compact_rows: {dead_words.numel()} bitmap words / {tile_dst.numel()} "
                         f"tile offsets do not cover {n_tiles} tiles")
    if dead_words.device != dev or tile_dst.device != dev:
        raise ValueError("compact_rows: bitmap, tile offsets and slab on different devices")
    if (stage is None) != (stage2 is None) and slab2 is not None:
        raise ValueError("compact_rows: both slabs are staged or neither")
    if slab2 is None and stage2 is not None:
        raise ValueError("compact_rows: stage2 without slab2")
    for name, t, need in (("slab", slab, n_valid), ("slab2", slab2, n_valid),
                          ("stage", stage, n_rows), ("stage2", stage2, n_rows)):
        if t is None:
            continue
        if t.element_size() not in (1, 2):
            raise TypeError(f"compact_rows: {name} must hold 1- or 2-byte elements, got {t.dtype}")
        _chk(t, t.dtype, name, 2)
        if t.shape[1] != D or D % 8 or t.shape[0] < need or t.device != dev:
            raise ValueError(f"compact_rows: {name} {tuple(t.shape)} does not hold {need} rows "
                             f"of width {D} (a multiple of 8) on {dev}")
        if t.data_ptr() % 16:
            raise ValueError(f"compact_rows: {name} is not 16-byte aligned")
    for s, g, name in ((slab, stage, "stage"), (slab2, stage2, "stage2")):
        if g is not None and g.dtype != s.dtype:
            raise TypeError(f"compact_rows: {name} is {g.dtype}, its slab {s.dtype}")
    if stage is not None and n_rows < 0:
        raise ValueError("compact_rows: n_rows < 0")
    cap = 0 if stage is None else stage.shape[0]
    if stage2 is not None:
        cap = min(cap, stage2.shape[0])
    hip().compact_rows(_ptr(dead_words), _ptr(tile_dst), t0, t1, n_valid, _ptr(slab),
                       slab.element_size(), _ptr(stage), _ptr(slab2),
                       0 if slab2 is None else slab2.element_size(), _ptr(stage2), D, n_rows, cap,
                       stream_handle(dev))


def scan_stream_nt_ok(dim: int, form: int, depth: int = 0) -> bool:
    """Does the stream scan (index_stream.hip) have a non-temporal row stream for this form?
    Only where every sub-tile is read by exactly one wave, once: MX-fp4 (form 1) at width 384,
    at the kernel's default depth (0, or 3 by its number)."""
    return int(form) == 1 and int(dim) == 384 and int(depth) in (0, 3)


# the prefix scan's depths (index_stream.hip symb_stream_prefix_depth): 3 (or 0, the default) and
# the deep one that keeps the whole-row form's bytes in flight per wave
SCAN_PREFIX_DEEP = {3: 6, 2: 8}


def scan_stream_prefix_ok(dim: int, form: int, depth: int, prefix: int) -> bool:
    """Does the stream scan have a prefix form (scan_stream_kernel NKP_) reading ``prefix``
    k-steps?  Only MX-fp4 (form 1) at width 384, prefix 2 or 3, at depth 0 / 3 or the deep depth."""
    return (int(form) == 1 and int(dim) == 384 and int(prefix) in SCAN_PREFIX_DEEP
            and int(depth) in (0, 3, SCAN_PREFIX_DEEP[int(prefix)]))


def index_scan_stream(*args, nt: int = 0, prefix: int = 0, pbounds=None, thr_prefix: int = 0,
                      **kw) -> None:
    """``_hip.index_scan_stream`` with the ``nt`` and ``prefix`` arguments checked first: the
    non-temporal row stream is refused, before the extension is touched, for every form that has
    none (the int8 image, widths 768 / 1024, depths 4 / 5 -- scan_stream_nt_ok), and so is the
    prefix form (``prefix`` = 2 or 3 k-steps read per record; scan_stream_prefix_ok), which is
    non-temporal always.  A prefix scan's thresholds are only meaningful with the prefix bounds
    of the image it reads: ``pbounds`` (the shard's 3-float tensor) must be given with a nonzero
    ``prefix``.  ``thr_prefix`` (a pointer to the prefix thresholds): the fp4 tier in one launch
    that picks its form on the device from the word ``gate2`` (0: the prefix form at its deep
    depth, else the whole-row form with ``thr``); ``pbounds`` then goes to the kernel as the
    prefix form's row bound, otherwise it is not passed on.  Every other argument is passed
    through as the binding takes it (raw pointers, the stream handle)."""
    nt, prefix = int(nt), int(prefix)
    if nt not in (0, 1):
        raise ValueError(f"index_scan_stream: nt must be 0 or 1, got {nt}")
    dim, form, depth = kw.get("dim", 384), kw.get("form", 0), kw.get("depth", 0)
    if prefix:
        if not scan_stream_prefix_ok(dim, form, depth, prefix):
            raise ValueError(f"index_scan_stream: no prefix form for dim {dim}, form {form}, "
                             f"depth {depth}, prefix {prefix} (MX-fp4 at 384, prefix 2 or 3, "
                             f"depth 0 / 3 or {SCAN_PREFIX_DEEP})")
        if pbounds is None:
            raise ValueError("index_scan_stream: a prefix scan needs the image's prefix bounds")
        if not nt:
            raise ValueError("index_scan_stream: the prefix form is non-temporal (nt=1)")
        if thr_prefix:
            if int(depth) != SCAN_PREFIX_DEEP[prefix] or not kw.get("gate2"):
                raise ValueError("index_scan_stream: the one-launch fp4 tier runs its prefix form "
                                 f"at depth {SCAN_PREFIX_DEEP[prefix]} and needs the form word "
                                 "(gate2)")
            kw["thr_prefix"], kw["pbounds"] = int(thr_prefix), pbounds.data_ptr()
    elif thr_prefix:
        raise ValueError("index_scan_stream: thr_prefix without a prefix length")
    elif nt and not scan_stream_nt_ok(dim, form, depth):
        raise ValueError(f"index_scan_stream: no non-temporal form for dim {dim}, form {form}, "
                         f"depth {depth} (MX-fp4 at 384, default depth only)")
    if prefix:
        kw["prefix"] = prefix
    hip().index_scan_stream(*args, nt=nt, **kw)


def prune_finish(rows: torch.Tensor, q_unit: torch.Tensor, cand_i: torch.Tensor,
                 cand_n: torch.Tensor, cand_s: torch.Tensor, k: int, out_s: torch.Tensor,
                 out_i: torch.Tensor, ovf: torch.Tensor, tier: torch.Tensor | None = None,
                 host_word: int = 0) -> None:
    """The pruned search's finish in one launch (prune_finish.hip): every query's first
    ``min(cand_n[q], cap)`` candidates ``cand_i[q]`` (int32 [NQ, cap], rows of ``rows``) are
    re-scored exactly against the bf16 ``rows`` into ``cand_s`` (f32 [NQ, cap]) and their top
    ``k`` (<= 16) goes to ``out_s`` / ``out_i`` ([NQ, k]; missing slots (-inf, -1)).  A count above
    cap raises ``ovf[0]`` (int32, never cleared here).  ``tier`` (int32 [1] on the device) and
    ``host_word`` (the device address of a pinned host int32, ``_hip.host_device_ptr``): the
    kernel copies the one to the other; both or neither."""
    _chk(rows, torch.bfloat16, "rows", 2)
    _chk(q_unit, torch.bfloat16, "q_unit", 2)
    _chk(cand_i, torch.int32, "cand_i", 2)
    _chk(cand_s, torch.float32, "cand_s", 2)
    _chk(cand_n, torch.int32, "cand_n", 1)
    _chk(out_s, torch.float32, "out_s", 2)
    _chk(out_i, torch.int32, "out_i", 2)
    _chk(ovf, torch.int32, "ovf", 1)
    NQ, D = q_unit.shape
    cap, k = cand_i.shape[1], int(k)
    if D not in SUPPORTED_H or rows.shape[1] != D or rows.shape[0] < 1:
        raise ValueError(f"prune_finish: rows {tuple(rows.shape)} / queries {tuple(q_unit.shape)}: "
                         f"width must be one of {SUPPORTED_H}")
    if not 0 < k <= 16:
        raise ValueError(f"prune_finish: k = {k} outside 1 .. 16")
    if (cand_i.shape != (NQ, cap) or cand_s.shape != (NQ, cap) or cap < 1 or cand_n.numel() < NQ
            or out_s.shape != (NQ, k) or out_i.shape != (NQ, k) or ovf.numel() < 1):
        raise ValueError("prune_finish: candidate / output buffers do not match "
                         f"[{NQ}, cap] / [{NQ}, {k}]")
    dev = rows.device
    for name, t in (("q_unit", q_unit), ("cand_i", cand_i), ("cand_n", cand_n), ("cand_s", cand_s),
                    ("out_s", out_s), ("out_i", out_i), ("ovf", ovf), ("tier", tier)):
        if t is not None and t.device != dev:
            raise ValueError(f"prune_finish: {name} on {t.device}, rows on {dev}")
    if (tier is None) != (not host_word):
        raise ValueError("prune_finish: tier and host_word come together")
    if tier is not None:
        _chk(tier, torch.int32, "tier", 1)
    hip().prune_finish(_ptr(rows), rows.shape[0], _ptr(q_unit), NQ, D, _ptr(cand_i), _ptr(cand_n),
                       cap, _ptr(cand_s), 16, k, _ptr(out_s), _ptr(out_i), _ptr(ovf),
                       stream_handle(dev), tier=_ptr(tier), host_word=int(host_word))
