"""Plain-PyTorch fp32 oracles for every HIP kernel (and the CPU execution backend).

These are deliberately written as the straightforward textbook math of the reference pipeline:
BERT embeddings + LayerNorm, per-layer self-attention / GELU-FFN with post-LN residuals, and the
masked mean pool of services/preprocessing_service/src/embedding_generator.rs:201-207
(sum(h * mask) / (sum(mask) + 1e-9)).  They operate on the same packed (varlen) layout as the
HIP kernels so tests compare like with like.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def embed_ln_ref(ids, pos, type_ids, wemb, pemb, temb, gamma, beta, eps):
    x = wemb.float()[ids.long()] + pemb.float()[pos.long()]
    tt = type_ids.long() if type_ids is not None else torch.zeros_like(ids, dtype=torch.long)
    x = x + temb.float()[tt]
    return F.layer_norm(x, (x.shape[-1],), gamma.float(), beta.float(), eps)


def add_ln_ref(x, res, gamma, beta, eps):
    y = x.float() + (res.float() if res is not None else 0.0)
    return F.layer_norm(y, (y.shape[-1],), gamma.float(), beta.float(), eps)


def gemm_ref(a, w, bias, epi=0, residual=None, gamma=None, beta=None, eps=1e-12):
    y = a.float() @ w.float().t() + bias.float()
    if epi == 1:
        y = F.gelu(y)  # erf form, as BERT
    elif epi == 2:
        y = y + residual.float()
    elif epi == 3:
        y = F.layer_norm(y + residual.float(), (y.shape[-1],), gamma.float(), beta.float(), eps)
    return y


def ln_chunk_stats_ref(y: torch.Tensor, chunk: int = 64) -> torch.Tensor:
    """Per-row partial statistics of y [M, N] over `chunk`-column chunks: [M, N / chunk, 2] of
    (chunk mean, sum of squared deviations from it) in fp32 -- the deferred LayerNorm's LNF_STATS
    output (gemm.hip)."""
    yc = y.float().view(y.shape[0], -1, chunk)
    m = yc.mean(-1)
    return torch.stack([m, ((yc - m[..., None]) ** 2).sum(-1)], -1)


def attention_ref(qkv, cu_seqlens, n_heads, head_dim):
    """Varlen bidirectional attention over packed [T, 3H] rows -> [T, H] (fp32)."""
    H = n_heads * head_dim
    qkv = qkv.float()
    out = torch.empty(qkv.shape[0], H, dtype=torch.float32, device=qkv.device)
    cu = cu_seqlens.tolist()
    for b in range(len(cu) - 1):
        s, e = cu[b], cu[b + 1]
        if e <= s:
            continue
        blk = qkv[s:e]
        q = blk[:, :H].view(-1, n_heads, head_dim).transpose(0, 1)
        k = blk[:, H:2 * H].view(-1, n_heads, head_dim).transpose(0, 1)
        v = blk[:, 2 * H:].view(-1, n_heads, head_dim).transpose(0, 1)
        p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(head_dim), dim=-1)
        out[s:e] = (p @ v).transpose(0, 1).reshape(e - s, H)
    return out


def pool_ref(hidden, cu_seqlens, mode="mean", normalize=False):
    h = hidden.float()
    cu = cu_seqlens.tolist()
    outs = []
    for b in range(len(cu) - 1):
        s, e = cu[b], cu[b + 1]
        if mode == "cls":
            v = h[s] if e > s else torch.zeros(h.shape[1], device=h.device)
        else:
            v = h[s:e].sum(0) / (float(e - s) + 1e-9)
        outs.append(v)
    out = torch.stack(outs) if outs else torch.zeros(0, h.shape[1], device=h.device)
    if normalize:
        out = F.normalize(out, dim=-1)
    return out


def encoder_ref(params: dict, cfg, ids, pos, type_ids, cu_seqlens):
    """Full fp32 encoder forward on packed tokens -> last hidden state [T, H]."""
    H, nh = cfg.hidden, cfg.heads
    hd = H // nh
    h = embed_ln_ref(ids, pos, type_ids, params["wemb"], params["pemb"], params["temb"],
                     params["eln_g"], params["eln_b"], cfg.ln_eps)
    for L in params["layers"]:
        qkv = h @ L["wqkv"].float().t() + L["bqkv"].float()
        ctx = attention_ref(qkv, cu_seqlens, nh, hd)
        a = ctx @ L["wo"].float().t() + L["bo"].float()
        h2 = F.layer_norm(a + h, (H,), L["ln1_g"].float(), L["ln1_b"].float(), cfg.ln_eps)
        f = F.gelu(h2 @ L["wi"].float().t() + L["bi"].float())
        o = f @ L["wo2"].float().t() + L["bo2"].float()
        h = F.layer_norm(o + h2, (H,), L["ln2_g"].float(), L["ln2_b"].float(), cfg.ln_eps)
    return h


def topk_ref(index_rows: torch.Tensor, queries: torch.Tensor, k: int):
    """Exact cosine top-k of unit rows (fp32 math on the same bf16 data), over row chunks so
    no fp32 score block reaches 256 MiB (a single [NQ, n] GEMM output past 2 GiB came back with
    its tail unwritten on the GPU stack: benchmarks/diag/gemm_2g.py)."""
    qf = queries.float()
    n = index_rows.shape[0]
    k = min(k, n)
    chunk = max(4096, (1 << 26) // max(1, qf.shape[0]))
    if n <= chunk:
        return torch.topk(qf @ index_rows.float().t(), k, dim=1)
    vs, ix = [], []
    for s in range(0, n, chunk):
        v, i = torch.topk(qf @ index_rows[s:s + chunk].float().t(), min(k, n - s), dim=1)
        vs.append(v)
        ix.append(i + s)
    v, j = torch.topk(torch.cat(vs, 1), k, dim=1)
    return v, torch.gather(torch.cat(ix, 1), 1, j)


def filtered_topk_ref(index_rows: torch.Tensor, queries: torch.Tensor, k: int,
                      allow_bool: torch.Tensor):
    """Exact cosine top-k over the rows ``allow_bool`` [n] marks (fp32 math on the same bf16
    data, in row chunks as ``topk_ref``): disallowed scores go to -inf before the selection.
    Always [NQ, k]; slots past the allowed rows are (-inf, -1)."""
    qf = queries.float()
    n, NQ = index_rows.shape[0], qf.shape[0]
    allow = torch.as_tensor(allow_bool, dtype=torch.bool, device=index_rows.device)
    if allow.numel() != n:
        raise ValueError(f"filtered_topk_ref: {allow.numel()} mask entries for {n} rows")
    chunk = max(4096, (1 << 26) // max(1, NQ))
    vs = [torch.full((NQ, k), -math.inf, device=index_rows.device)]
    ix = [torch.full((NQ, k), -1, dtype=torch.int64, device=index_rows.device)]
    for s in range(0, n, chunk):
        sc = qf @ index_rows[s:s + chunk].float().t()
        sc.masked_fill_(~allow[s:s + chunk][None, :], -math.inf)
        v, i = torch.topk(sc, min(k, sc.shape[1]), dim=1)
        vs.append(v)
        ix.append(i + s)
    v, j = torch.topk(torch.cat(vs, 1), k, dim=1)
    i = torch.gather(torch.cat(ix, 1), 1, j)
    return v, torch.where(torch.isfinite(v), i, torch.full_like(i, -1))


def grouped_filtered_topk_ref(index_rows: torch.Tensor, queries: torch.Tensor, k: int, allows,
                              group_of):
    """``filtered_topk_ref`` under a mask per query: ``allows`` is a sequence of bool [n] masks
    (or a bool [G, n] tensor) and ``group_of`` [NQ] names each query's mask.  Query i's result
    is the exact top-k over the rows ``allows[group_of[i]]`` marks.  Always [NQ, k]; slots past
    a query's allowed rows are (-inf, -1)."""
    dev = index_rows.device
    qf = queries.float()
    n, NQ = index_rows.shape[0], qf.shape[0]
    allow = torch.stack([torch.as_tensor(a, dtype=torch.bool, device=dev) for a in allows]) \
        if not isinstance(allows, torch.Tensor) else allows.to(dev, torch.bool)
    if allow.dim() != 2 or allow.shape[1] != n:
        raise ValueError(f"grouped_filtered_topk_ref: masks {tuple(allow.shape)} for {n} rows")
    g = torch.as_tensor(group_of, dtype=torch.int64, device=dev).flatten()
    if g.numel() != NQ:
        raise ValueError(f"grouped_filtered_topk_ref: {g.numel()} groups for {NQ} queries")
    if NQ and (int(g.min()) < 0 or int(g.max()) >= allow.shape[0]):
        raise IndexError("grouped_filtered_topk_ref: group outside the masks")
    chunk = max(4096, (1 << 26) // max(1, NQ))
    vs = [torch.full((NQ, k), -math.inf, device=dev)]
    ix = [torch.full((NQ, k), -1, dtype=torch.int64, device=dev)]
    for s in range(0, n, chunk):
        sc = qf @ index_rows[s:s + chunk].float().t()
        sc.masked_fill_(~allow[:, s:s + chunk][g], -math.inf)
        v, i = torch.topk(sc, min(k, sc.shape[1]), dim=1)
        vs.append(v)
        ix.append(i + s)
    v, j = torch.topk(torch.cat(vs, 1), k, dim=1)
    i = torch.gather(torch.cat(ix, 1), 1, j)
    return v, torch.where(torch.isfinite(v), i, torch.full_like(i, -1))


def row_scores_ref(index_rows: torch.Tensor, queries: torch.Tensor, r: torch.Tensor):
    """Exact fp32 scores of the rows r [NQ, k] a search returned (no full score matrix)."""
    if r.numel() and int(r.min()) < 0:
        raise ValueError("row_scores_ref: negative row id")
    return (index_rows[r.long()].float() * queries.float()[:, None, :]).sum(-1)


def quant_rows_i8_ref(x: torch.Tensor):
    """Per-row int8 image of bf16 rows (index_i8.hip quant_rows_i8): scale = max|x| / 127,
    x8 = round-half-even(x / scale) clamped to +-127; returns (x8, scale, |x - x~|, |x~|)."""
    xf = x.float()
    amax = xf.abs().amax(dim=1)
    sc = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q = torch.round(xf / sc[:, None]).clamp_(-127, 127)
    xt = q * sc[:, None]
    return q.to(torch.int8), sc, (xf - xt).norm(dim=1), xt.norm(dim=1)


SPLIT_HEAVY = 64   # leading (rotated) dims the split int8 image keeps as fp16


def quant_rows_split_ref(xr: torch.Tensor, heavy: int = SPLIT_HEAVY):
    """Split image of ROTATED fp32 rows (index_i8.hip quant_rows_split): the leading ``heavy``
    dims as fp16 (bytes 0 .. 2 heavy of each image row), the rest as int8 with scale
    max |x_l| / 127.  Returns (img int8 [n, D + heavy], scale, norms) with norms = the 6 per-row
    norms (|x_l - x~_l|, |x~_l|, |x_l|, |x_h - x^_h|, |x^_h|, |x_h|) the bound is built from."""
    xf = xr.float()
    xh, xl = xf[:, :heavy], xf[:, heavy:]
    amax = xl.abs().amax(dim=1)
    sc = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    q = torch.round(xl * (1.0 / sc)[:, None]).clamp_(-127, 127)
    xt = q * sc[:, None]
    hh = xh.half()
    img = torch.cat([hh.view(torch.int8).reshape(xf.shape[0], 2 * heavy), q.to(torch.int8)], 1)
    hf = hh.float()
    norms = torch.stack([(xl - xt).norm(dim=1), xt.norm(dim=1), xl.norm(dim=1),
                         (xh - hf).norm(dim=1), hf.norm(dim=1), xh.norm(dim=1)], 1)
    return img, sc, norms


def split_estimate_ref(q_img: torch.Tensor, sq: torch.Tensor, x_img: torch.Tensor,
                       sx: torch.Tensor, heavy: int = SPLIT_HEAVY) -> torch.Tensor:
    """The split scan's estimate of every (query, row) score, q^_h . x^_h + sq sx (q8_l . x8_l)
    (index_scan_i8_kernel HK = 2, as acc_f + acc_i * sq * sx)."""
    def parts(img):
        h = img[:, :2 * heavy].contiguous().view(torch.float16).float()
        return h, img[:, 2 * heavy:].float()
    qh, ql = parts(q_img)
    xh, xl = parts(x_img)
    return qh @ xh.t() + (ql @ xl.t()) * sq[:, None] * sx[None, :]


E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mx4_codes_ref(x: torch.Tensor):
    """MX-fp4 quantisation of rows (D a multiple of 32): per 32-dim block the scale
    2^ceil(log2(max|x| / 6)) (exponent e, e8m0 byte e + 127), each element the nearest e2m1 value of
    x / s.  Returns (nibble bytes uint8 [n, D / 2] (element 2j in the low nibble of byte j),
    exponents int [n, D / 32], decoded x~ f32 [n, D], norms [n, 3] = (|x - x~|, |x~|, |x|))."""
    xf = x.float()
    n, d = xf.shape
    nb = d // 32
    blk = xf.view(n, nb, 32)
    amax = blk.abs().amax(-1)
    _, k = torch.frexp(amax / 6.0)
    e = k.clone()
    e = torch.where(amax <= 6.0 * torch.ldexp(torch.ones_like(amax), k - 1), k - 1, e)
    e = torch.where(amax > 6.0 * torch.ldexp(torch.ones_like(amax), e), e + 1, e)
    e = torch.where(amax > 0, e, torch.full_like(e, -127)).clamp_(min=-127)
    a = blk.abs() * torch.ldexp(torch.ones_like(amax), -e)[..., None]
    q = torch.where(a < 2.0, torch.round(a * 2.0) * 0.5,
                    torch.where(a < 4.0, torch.round(a), torch.where(a < 5.0, 4.0, 6.0)))
    grid = torch.tensor(E2M1, dtype=torch.float32, device=xf.device)
    code = (q[..., None] == grid).float().argmax(-1)
    code = code | torch.where((blk < 0) & (code != 0), 8, 0)
    xt = torch.where(blk < 0, -q, q) * torch.ldexp(torch.ones_like(amax), e)[..., None]
    codes = code.view(n, d).to(torch.int32)
    img = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)
    xt = xt.view(n, d)
    norms = torch.stack([(xf - xt).norm(dim=1), xt.norm(dim=1), xf.norm(dim=1)], 1)
    return img, e, xt, norms


def mx4_prefix_norms_ref(x: torch.Tensor, nkp: int) -> torch.Tensor:
    """The prefix tier's norms of rows (or queries), split at dim 64 nkp (P = the first nkp
    k-steps of the MX-fp4 scan, R = the rest): [n, 4] = (|x_P - x~_P|, |x~_P|, |x_P|, |x_R|), x~
    the MX-fp4 image.  Rows raise the bounds (E_P, X_P, XR) to the maxima of columns 0, 1, 3;
    a query's margin is mP = |q_P| E_P + |q_P - q~_P| X_P + 1e-5 and its qR column 3."""
    p = 64 * int(nkp)
    if not 0 < p <= x.shape[1]:
        raise ValueError(f"mx4_prefix_norms_ref: nkp {nkp} for width {x.shape[1]}")
    xf = x.float()
    xt = mx4_codes_ref(x)[2]
    return torch.stack([(xf[:, :p] - xt[:, :p]).norm(dim=1), xt[:, :p].norm(dim=1),
                        xf[:, :p].norm(dim=1), xf[:, p:].norm(dim=1)], 1)


def prefix_tier_choice_ref(T, m4, m8, mP, qR, XR, probe_s, probe_p, rate, tail_s, tail_p, limit,
                           band=1.0):
    """The first tier the pruned search takes (index_i8.hip mx4_select_kernel, then
    mx4_prefix_select_kernel), as a torch composition: "prefix", "fp4" or "int8".
    T / m4 / m8 / mP / qR: [NQ] (k-th score bound, fp4 margin, int8 margin, prefix margin, |q_R|);
    probe_s / probe_p: [NQ, n] exact scores and exact partial scores (first dims) of the probe rows,
    each standing for ``rate`` corpus rows; tail_s / tail_p: the same of the tail rows; limit: the
    candidates per query a tier may add; band: the share of mP between a row's prefix estimate and
    its exact partial score that the count allows (1 = the worst case).
    Returns (name, thr4, thrP)."""
    T, m4, m8 = T.float(), m4.float(), m8.float()
    hi = (T - m8)[:, None]

    def count(lo, ps, ts, pp=None, tp=None):
        a = ((ps if pp is None else pp) >= lo[:, None]) & (ps < hi)
        b = ((ts if tp is None else tp) >= lo[:, None]) & (ts < hi)
        return a.sum(1).float() * float(rate) + b.sum(1).float()

    thr4 = T - m4
    fp4 = bool((count(T - 2.0 * m4, probe_s, tail_s) <= limit).all())
    thrP = T - mP.float() - qR.float() * float(XR)
    pfx = bool((torch.isfinite(thrP) & (thrP > 0)).all()) and bool(
        (count(thrP - float(band) * mP.float(), probe_s, tail_s, probe_p, tail_p) <= limit).all())
    return ("prefix" if fp4 and pfx else "fp4" if fp4 else "int8"), thr4, thrP


# ---- the stream images (index_stream.hip): 32-row sub-tiles, fragment-major ----------------
def _stream_frags(rowbytes: torch.Tensor) -> torch.Tensor:
    """Row-major image bytes [n, RB] (RB = 32 NKS) -> fragment-major [n_sub, NKS * 1024]: k-step
    ks, lane l = 32 hh + rr holds row rr's bytes 32 ks + 16 hh .. + 16 at 1024 ks + 16 l."""
    n, rb = rowbytes.shape
    n_sub = (n + 31) // 32
    pad = torch.zeros(n_sub * 32, rb, dtype=torch.uint8, device=rowbytes.device)
    pad[:n] = rowbytes.view(torch.uint8)
    nks = rb // 32
    return pad.view(n_sub, 32, nks, 2, 16).permute(0, 2, 3, 1, 4).reshape(n_sub, nks * 1024)


def _stream_rows(frags: torch.Tensor, n: int, rb: int) -> torch.Tensor:
    """Inverse of _stream_frags: row-major bytes [n, rb]."""
    n_sub = frags.shape[0]
    nks = rb // 32
    return frags.reshape(n_sub, nks, 2, 32, 16).permute(0, 3, 1, 2, 4).reshape(n_sub * 32, rb)[:n]


def stream_i8_tile_codes_ref(x: torch.Tensor):
    """int8 codes of rows with ONE scale per 32-row sub-tile (index_stream.hip i8_stream_tile):
    s = max |x| / 127 over the tile's rows (rows past n count as zeros; an all-zero tile: 1),
    x8 = round(x * (1 / s)).  Returns (x8 int8 [n, D], per-row scale f32 [n] (the tile's),
    |x - x~| [n], |x~| [n])."""
    xf = x.float()
    n, d = xf.shape
    n_sub = (n + 31) // 32
    pad = torch.zeros(n_sub * 32, d, dtype=torch.float32, device=xf.device)
    pad[:n] = xf
    amax = pad.view(n_sub, 32 * d).abs().amax(1)
    s = torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))
    sr = s.repeat_interleave(32)[:n]
    inv = 1.0 / sr
    x8 = torch.round(xf * inv[:, None]).clamp_(-127, 127)
    xt = x8 * sr[:, None]
    return x8.to(torch.int8), sr, (xf - xt).norm(dim=1), xt.norm(dim=1)


def stream_i8_ref(x: torch.Tensor):
    """int8 stream image of bf16 rows (quant_stream_i8): records uint8 [n_sub, 16 + D * 32] (the
    sub-tile's scale as f32 at byte 0 of a 16-byte header, then the fragments), plus (|x - x~|,
    |x~|) per row."""
    q8, sr, err, xtn = stream_i8_tile_codes_ref(x)
    frags = _stream_frags(q8.view(torch.uint8))
    n_sub = frags.shape[0]
    hdr = torch.zeros(n_sub, 4, dtype=torch.float32, device=x.device)
    hdr[:, 0] = sr[::32]
    return torch.cat([hdr.view(torch.uint8), frags], 1), err, xtn


def stream_i8_decode(rec: torch.Tensor, n: int, d: int):
    """(x8 int8 [n, d], per-row scale f32 [n] -- its sub-tile's) of an int8 stream image."""
    hdr = rec[:, :16].contiguous().view(torch.float32)[:, 0].repeat_interleave(32)[:n]
    x8 = _stream_rows(rec[:, 16:], n, d).contiguous().view(torch.int8)
    return x8, hdr


def stream_mx4_ref(x: torch.Tensor):
    """MX-fp4 stream image of bf16 rows (quant_stream_mx4, rows): records uint8 [n_sub, D * 16 +
    NSC * 256] (fragments, then dword j of lane l = 32 hh + rr: the e8m0 bytes of k-steps 4j ..
    4j + 3 of row rr, block 2 ks + hh), plus norms [n, 3]."""
    img, e, _, norms = mx4_codes_ref(x)
    n, d = x.shape
    nks = d // 64
    nsc = (nks + 3) // 4
    frags = _stream_frags(img)
    n_sub = frags.shape[0]
    sc = torch.zeros(n_sub * 32, nsc, 2, 4, dtype=torch.uint8, device=x.device)  # [row][j][hh][b]
    for b in range(d // 32):
        ks, hh = b // 2, b % 2
        sc[:n, ks // 4, hh, ks % 4] = (e[:, b] + 127).to(torch.uint8)
    # -> [n_sub][j][lane = 32 hh + rr][byte]
    sc = sc.view(n_sub, 32, nsc, 2, 4).permute(0, 2, 3, 1, 4).reshape(n_sub, nsc * 256)
    return torch.cat([frags, sc], 1), norms


def stream_mx4_query_ref(x: torch.Tensor):
    """The MX-fp4 query image (quant_stream_mx4, queries): nibbles [n, D / 2] row-major and the
    scale record int32 [n, 2 NSC] (dword hh NSC + j, byte b = block 2 (4 j + b) + hh), plus the
    decoded x~ and norms."""
    img, e, xt, norms = mx4_codes_ref(x)
    n, d = x.shape
    nks = d // 64
    nsc = (nks + 3) // 4
    qs = torch.zeros(n, 2, nsc, 4, dtype=torch.uint8, device=x.device)
    for b in range(d // 32):
        ks, hh = b // 2, b % 2
        qs[:, hh, ks // 4, ks % 4] = (e[:, b] + 127).to(torch.uint8)
    return img, qs.view(n, 2 * nsc * 4).view(torch.int32), xt, norms


def mx4_decode_codes(img: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """Decoded f32 rows from nibble bytes [n, D / 2] and exponents [n, D / 32]."""
    n = img.shape[0]
    d = img.shape[1] * 2
    b = img.to(torch.int32)
    codes = torch.stack([b & 15, b >> 4], -1).view(n, d)
    grid = torch.tensor(E2M1, dtype=torch.float32, device=img.device)
    v = grid[codes & 7] * torch.where(codes & 8 != 0, -1.0, 1.0)
    return (v.view(n, d // 32, 32) * torch.ldexp(torch.ones_like(e, dtype=torch.float32),
                                                  e.to(torch.int32))[..., None]).view(n, d)


def stream_mx4_query_decode(q4: torch.Tensor, qs: torch.Tensor) -> torch.Tensor:
    """Decoded f32 queries of a stream MX-fp4 query image (stream_mx4_query_ref's layout)."""
    n, d = q4.shape[0], q4.shape[1] * 2
    nsc = (d // 64 + 3) // 4
    b = qs.contiguous().view(torch.uint8).view(n, 2, nsc, 4)
    e = torch.stack([b[:, blk % 2, (blk // 2) // 4, (blk // 2) % 4].to(torch.int32) - 127
                     for blk in range(d // 32)], 1)
    return mx4_decode_codes(q4, e)


def stream_mx4_decode(rec: torch.Tensor, n: int, d: int) -> torch.Tensor:
    """Decoded f32 rows [n, d] of an MX-fp4 stream image."""
    nks = d // 64
    nsc = (nks + 3) // 4
    n_sub = rec.shape[0]
    img = _stream_rows(rec[:, :nks * 1024], n, d // 2)
    sc = rec[:, nks * 1024:].reshape(n_sub, nsc, 2, 32, 4).permute(0, 3, 1, 2, 4).reshape(n_sub * 32, nsc, 2, 4)[:n]
    e = torch.stack([sc[:, (b // 2) // 4, b % 2, (b // 2) % 4].to(torch.int32) - 127
                     for b in range(d // 32)], 1)
    return mx4_decode_codes(img, e)


def quant_rows_mx4_ref(x: torch.Tensor):
    """MX-fp4 image of 384-wide rows (index_i8.hip quant_rows_mx4): per 32-dim block the scale
    2^ceil(log2(max|x| / 6)) (e8m0 byte e + 127), each element the nearest e2m1 value of x / s,
    element 2j in the low nibble of byte j; block-scale bytes in a 16-byte record per row, dword g
    = blocks g, 4 + g, 8 + g.  Returns (img uint8 [n, 192], scales uint8 [n, 16], decoded x~ f32
    [n, 384], norms [n, 3] = (|x - x~|, |x~|, |x|))."""
    xf = x.float()
    n, d = xf.shape
    assert d == 384
    blk = xf.view(n, 12, 32)
    amax = blk.abs().amax(-1)
    _, k = torch.frexp(amax / 6.0)
    e = k.clone()
    e = torch.where(amax <= 6.0 * torch.ldexp(torch.ones_like(amax), k - 1), k - 1, e)
    e = torch.where(amax > 6.0 * torch.ldexp(torch.ones_like(amax), e), e + 1, e)
    e = torch.where(amax > 0, e, torch.full_like(e, -127)).clamp_(min=-127)
    a = blk.abs() * torch.ldexp(torch.ones_like(amax), -e)[..., None]
    q = torch.where(a < 2.0, torch.round(a * 2.0) * 0.5,
                    torch.where(a < 4.0, torch.round(a), torch.where(a < 5.0, 4.0, 6.0)))
    grid = torch.tensor(E2M1, dtype=torch.float32, device=xf.device)
    code = (q[..., None] == grid).float().argmax(-1)
    code = code | torch.where((blk < 0) & (code != 0), 8, 0)
    xt = torch.where(blk < 0, -q, q) * torch.ldexp(torch.ones_like(amax), e)[..., None]
    codes = code.view(n, d).to(torch.int32)
    img = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)
    sc = torch.zeros(n, 16, dtype=torch.uint8, device=xf.device)
    for b in range(12):
        sc[:, 4 * (b & 3) + (b >> 2)] = (e[:, b] + 127).to(torch.uint8)
    xt = xt.view(n, d)
    norms = torch.stack([(xf - xt).norm(dim=1), xt.norm(dim=1), xf.norm(dim=1)], 1)
    return img, sc, xt, norms


def mx4_decode_ref(img: torch.Tensor, sc: torch.Tensor) -> torch.Tensor:
    """Decoded f32 rows of an MX-fp4 image (quant_rows_mx4_ref's layout)."""
    n = img.shape[0]
    b = img.to(torch.int32)
    codes = torch.stack([b & 15, b >> 4], -1).view(n, 384)
    grid = torch.tensor(E2M1, dtype=torch.float32, device=img.device)
    v = grid[codes & 7] * torch.where(codes & 8 != 0, -1.0, 1.0)
    e = torch.stack([sc[:, 4 * (blk & 3) + (blk >> 2)].to(torch.int32) - 127
                     for blk in range(12)], 1)
    return (v.view(n, 12, 32) * torch.ldexp(torch.ones(n, 12, device=img.device), e)[..., None]).view(n, 384)
