"""Teacher-forced probe for the fp8 encoder layer's HAND-OFFS (``EncoderRuntime::fp8_layer``).

Shared by test_fp8_probe_cpu.py (a test of this probe, CPU only) and test_encoder_fp8_gpu.py.

An end-to-end comparison of the fp8 encoder with the fp32 oracle drowns in a layer's worth of e4m3
noise (encoder_probe.fp8_emulated_forward: 0.20-0.32 pooled, above the planted effects).  After a
forward, though, the workspace still holds nearly every hand-off of the LAST layer, so each step
of that layer can be recomputed in float64 from the step's own OBSERVED inputs and compared with
its observed output: the only noise left is one rounding (bf16 or e4m3), not a layer's worth.
Running the 1-, 2- and 3-layer encoder makes every layer the last one once.

* quantiser rules, written once: ``quant_weight_fp8`` per output channel (models/encoder.py),
  ``quant_tokens`` per token (quant_rows_fp8_kernel and add_ln's fused output), ``mx_quant`` /
  ``mx_decode`` per 32 columns (attention's and FFN1's MX epilogues);
* ``emulate_layer``: the CPU model of fp8_layer, every hand-off under the checker's names;
* ``check_layer``: {step: statistic}; statistic = max over token rows of |out_r - ref_r|_2 /
  |ref_r|_2 with ref in float64 from the observed inputs, plus the element-wise measures the
  per-kernel tests use for the three e4m3-output steps;
* ``workspace_views``: the hand-offs sliced out of a HipEncoder's workspace;
* ``PLANTED``: fp8 wiring bugs planted into the emulation (test code only), each naming the
  step(s) that must reject it.

Steps (class = the rounding of the observed output):

    qkv     ws qkv           dec(a8_in, sa_in) dec(Wqkv)^T + bqkv          bf16 (k = 1), e4m3 (k >= 2)
    ctx     dec(ctx8, ctxs)  attention(observed qkv)                       e4m3
    h2      ws h2            LN1(bf16(dec ctx dec(Wo)^T + bo + h_in))      bf16
    a8      dec(a8, sa)      observed h2 (per-token rule)                  e4m3
    ff      dec(ff8, ffs)    GELU(dec a8 dec(Wi)^T + bi)                   e4m3
    tmp     ws tmp           dec ff dec(Wo2)^T + bo2 + observed h2         bf16
    h       ws h             LN2(observed tmp)                             bf16
    pooled  forward output   pool_ref(observed h)                          test_pool's tolerances

For k >= 2 the checker's a8_in is the per-token rule applied to the bf16 h_in (the (k-1)-layer
encoder's output), while the runtime quantised the fp32 LayerNorm value: a few bytes round the
other way, so that qkv step sits in the e4m3 class.  The emulation does the same.

Thresholds.  Everything is measured on the CPU with lively_params(seed = 3) of the 3-layer probe
config and the probe batches short_mix, long_mix, q1 (e5-large: short_mix); nothing comes from the
HIP output.  Per model and class: F = the largest statistic of the two legitimate emulations
(fp32 GEMMs and LayerNorms; float64 with the K axis reversed) over the batches and k = 1..3,
P = the smallest statistic of the PLANTED entries, each at its own step, tau with
3 F <= tau <= P / 2 (test_fp8_probe_cpu.py recomputes F and P and asserts the rule).

    bf16 steps     F        P (entry, batch, k, step)                      tau
    minilm-l6    0.0021   0.195 (bo dropped, q1, 2, h2)                   0.02
    bge-base     0.0020   0.193 (ctx exponents one block off, q1, 3, h2)  0.02
    e5-large     0.0019   0.213 (bo dropped, short_mix, 2, h2)            0.02

    e4m3 steps     F        P (entry, batch, k, step)                      tau
    minilm-l6    0.0333   0.277 (bi dropped, q1, 2, ff)                   0.11
    bge-base     0.0315   0.245 (stale sa in FFN1, q1, 3, ff)             0.11
    e5-large     0.0294   0.292 (bi dropped, short_mix, 2, ff)            0.11

The planted entries run on every layer of q1 and on the middle layer (h_quantized and
quantize_out both set) of the two large batches.  The e4m3 class's F is the k >= 2 qkv step's
(0.018-0.033, the bytes of a8_in that round the other way); the three e4m3-output steps sit at
0.027-0.032, the bf16 steps at 0.0017-0.0021 whatever the model.  An entry that only permutes the
attention output's exponents does nothing where a row has one exponent throughout (MiniLM's q1,
third layer): Planted.acts says where it acted, and test_fp8_probe_cpu.py asserts that every
entry acts on short_mix's middle layer of every model.

Element-wise measures.  ctx / ff keep the per-kernel tests' acceptance numbers (exponent share
0.99 / 0.995, elements inside the bound: all / 0.999), sa its rtol 2^-8 -- bf16's unit roundoff,
the exact bound on |amax(bf16(y)) - amax(y)| / amax(bf16(y)), which the emulation reaches within
2 % (0.0039).  The a8 byte agreement keeps 0.995 but counts a byte as agreeing when the per-token
rule can produce it from SOME value that rounds to the observed bf16 h2 (bytes_consistent): the
kernel quantises the fp32 LayerNorm value, and plain equality with e4m3(h2 / scale) is 0.973-0.980
for a correct emulation and for the MI355X alike, so test_add_ln_fused_fp8_quant's 0.995 (taken
against the fp32 value, which no hand-off holds) is out of reach for any correct runtime there.

The HIP encoder's measured statistics (MI355X; test_fp8_layer_handoffs prints each), the largest
over the model's batches; exponent / element / byte shares are the smallest:

    model      k   qkv     ctx     h2      a8      ff      tmp     h       ctx_exp ff_exp  ff_elem a8_bytes sa
    minilm-l6  1  0.0018  0.0305  0.0021  0.0306  0.0298  0.0019  0.0020   0.9996  1.0000  1.0000  1.0000  0.00382
    minilm-l6  2  0.0281  0.0310  0.0021  0.0293  0.0292  0.0020  0.0020   0.9996  1.0000  1.0000  1.0000  0.00363
    minilm-l6  3  0.0269  0.0309  0.0020  0.0306  0.0293  0.0019  0.0020   0.9995  1.0000  1.0000  1.0000  0.00374
    bge-base   1  0.0018  0.0290  0.0019  0.0295  0.0285  0.0019  0.0019   0.9982  1.0000  1.0000  1.0000  0.00382
    bge-base   2  0.0246  0.0289  0.0019  0.0294  0.0288  0.0019  0.0019   0.9996  1.0000  1.0000  1.0000  0.00385
    bge-base   3  0.0264  0.0294  0.0023  0.0297  0.0287  0.0018  0.0018   0.9996  1.0000  1.0000  1.0000  0.00383
    e5-large   1  0.0017  0.0288  0.0019  0.0292  0.0281  0.0018  0.0018   0.9991  1.0000  1.0000  1.0000  0.00351
    e5-large   2  0.0234  0.0287  0.0019  0.0289  0.0281  0.0018  0.0018   0.9997  1.0000  1.0000  1.0000  0.00379
    e5-large   3  0.0237  0.0288  0.0019  0.0284  0.0281  0.0018  0.0018   1.0000  1.0000  1.0000  1.0000  0.00370

i.e. every step sits on the CPU emulation's floor, a factor 9 (bf16) and 3.5 (e4m3) under tau and
under tau / 2 throughout; ctx_elem is 1 and the pooled output equals pool_ref(observed h) to
0.0000 / 0.08 of test_pool's tolerances (f32 / unit) everywhere; plain a8 byte equality is
0.9746-0.9787.  These figures need the e4m3 matrices AS THE ENCODER QUANTISED THEM on the device
(test_encoder_fp8_gpu._layer_weights): with the host's image, which differs in 1-3 bytes in 10^4
(exact rounding ties), the bf16 steps read 0.0023-0.0042 and ff_elem 0.993-0.9986.
"""
from __future__ import annotations

import dataclasses
import functools
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

import encoder_probe as EP
from codename_symbiont_amd.models.encoder import quant_weight_fp8
from codename_symbiont_amd.ops import reference as R

MODELS = ("minilm-l6", "bge-base", "e5-large")
BATCHES = ("short_mix", "long_mix", "q1")
LAYERS = 3
E4M3 = torch.float8_e4m3fn
STEPS = ("qkv", "ctx", "h2", "a8", "ff", "tmp", "h", "pooled")
E4M3_STEPS = ("ctx", "a8", "ff")


def batches_for(model: str) -> tuple:
    return ("short_mix",) if model == "e5-large" else BATCHES


def cases():
    for m in MODELS:
        for n in batches_for(m):
            yield m, n


# --------------------------------------------------------------------------------- quantisers
def _bf16(x):
    return x.to(torch.bfloat16)


def quant_tokens(x: torch.Tensor):
    """Per-token e4m3 image of x [T, K]: (bytes uint8 [T, K], scale f32 [T]) with
    scale = max(amax, 1e-12) / 448 and bytes = e4m3(x * (448 / amax)), in fp32 as the kernels do."""
    x = x.float()
    amax = x.abs().amax(dim=1).clamp_min(1e-12)
    q = (x * (448.0 / amax)[:, None]).to(E4M3)
    return q.view(torch.uint8), amax / 448.0


def dequant_tokens(q8: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return q8.view(E4M3).double() * scale.double()[:, None]


def mx_quant(x, block=32):
    """Host MX fp8 quantiser: E8M0 exponent e per 32 consecutive columns (smallest e with
    amax * 2^-e < 448), e4m3 bytes of x * 2^-e.  Returns (bytes uint8 [M,K], exps int [M,K/32])."""
    M, K = x.shape
    xb = x.float().view(M, K // block, block)
    amax = xb.abs().amax(-1)
    _, ex = torch.frexp(amax / 448.0)
    ex = torch.where(amax > 0, ex.clamp(-127, 127), torch.full_like(ex, -127))
    q = (xb * torch.pow(2.0, -ex.float())[..., None]).to(torch.float8_e4m3fn)
    return q.view(M, K).view(torch.uint8), ex


def mx_decode(q8, ex, block=32):
    M, K = q8.shape
    v = q8.view(torch.float8_e4m3fn).float().view(M, K // block, block)
    return (v * torch.pow(2.0, ex.float())[..., None]).view(M, K)


def layer_weights(L: dict) -> dict:
    """What the fp8 encoder holds for one layer, from the layer's parameters: the four matrices
    rounded to bf16 and quantised per output channel (``wqkv`` -> e4m3 bytes, ``sw_qkv`` -> f32
    scales, ...), biases and LayerNorm parameters in fp32."""
    W = {}
    for k, s in (("wqkv", "sw_qkv"), ("wo", "sw_o"), ("wi", "sw_i"), ("wo2", "sw_o2")):
        W[k], W[s] = quant_weight_fp8(_bf16(L[k]))
    for k in ("bqkv", "bo", "bi", "bo2", "ln1_g", "ln1_b", "ln2_g", "ln2_b"):
        W[k] = L[k].float()
    return W


def attention(qkv, cu_seqlens, n_heads, head_dim, dtype=torch.float64):
    """ops.reference.attention_ref in ``dtype`` (the reference itself computes in fp32)."""
    if dtype == torch.float32:
        return R.attention_ref(qkv, cu_seqlens, n_heads, head_dim)
    H = n_heads * head_dim
    qkv = qkv.to(dtype)
    out = torch.zeros(qkv.shape[0], H, dtype=dtype)
    cu = cu_seqlens.tolist()
    for b in range(len(cu) - 1):
        s, e = cu[b], cu[b + 1]
        if e <= s:
            continue
        sp = lambda x: x.reshape(e - s, n_heads, head_dim).transpose(0, 1)  # noqa: E731
        q, k, v = sp(qkv[s:e, :H]), sp(qkv[s:e, H:2 * H]), sp(qkv[s:e, 2 * H:])
        p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(head_dim), dim=-1)
        out[s:e] = (p @ v).transpose(0, 1).reshape(e - s, H)
    return out


# --------------------------------------------------------------------------------- the emulation
VARIANTS = ("f32", "f64_reversed")


def emulate_layer(W: dict, cfg, batch, h_in, a8_in=None, *, variant="f32", bug=None, stale=None):
    """The CPU model of ``EncoderRuntime::fp8_layer`` -> every hand-off under the checker's names.

    W        layer_weights() of the layer
    h_in     the layer's bf16 input [T, H]
    a8_in    (bytes, scales): the image of h_in the QKV GEMM reads; None = quant_rows_fp8 of h_in
             (h_quantized false).  The returned ``a8_out`` / ``sa_out`` is ln2's fused image of
             the fp32 LayerNorm value, the next layer's a8_in when quantize_out is set.
    variant  "f32": GEMMs accumulate in fp32, LayerNorm in fp32 (what the kernels do, in another
             order); "f64_reversed": float64 with the K axis reversed, LayerNorm in float64 -- both
             legitimate, they differ in which way borderline bf16 / e4m3 roundings fall.
    bug      a PLANTED key (test code only); ``stale`` = the previous layer's hand-offs, what the
             workspace still holds where a planted bug reads the wrong region.
    The out-projection result is rounded to bf16 before ln1, as the runtime's tmp buffer does."""
    H, FF, nh = cfg.hidden, cfg.ffn, cfg.heads
    T = h_in.shape[0]
    dt = torch.float32 if variant == "f32" else torch.float64
    e4 = lambda b: b.view(E4M3).to(dt)  # noqa: E731

    def mm(a, w):            # [T, K] x [N, K]^T
        a, w = a.to(dt), w.to(dt)
        if variant != "f32":
            a, w = a.flip(1), w.flip(1)
        return a @ w.t()

    def ln(x, g, b):
        return F.layer_norm(x.to(dt), (H,), g.to(dt), b.to(dt), cfg.ln_eps)

    h_in = _bf16(h_in)
    a8i, sai = quant_tokens(h_in) if a8_in is None else a8_in
    out = {"a8_in": a8i, "sa_in": sai}
    # QKV
    xa, xs = (stale["a8"], stale["sa"]) if bug == "qkv_stale_a8" else (a8i, sai)
    acc = mm(e4(xa), e4(W["wqkv"]))
    if bug != "qkv_no_sa":
        acc = acc * xs.to(dt)[:, None]
    qkv = _bf16(acc * W["sw_qkv"].to(dt) + W["bqkv"].to(dt))
    out["qkv"] = qkv
    # attention -> MX fp8
    ctx8, ctxs = mx_quant(attention(qkv, batch.cu_seqlens, nh, H // nh, dt).float())
    out["ctx8"], out["ctxs"] = ctx8, ctxs
    # out-projection (block-scaled A) + residual -> bf16 tmp -> ln1 + fused quant
    ex = ctxs
    if bug == "ctx_exp_block_off":
        # hd 64: a head's second block takes its first block's exponent; hd 32: the block before
        ex = ctxs.roll(1, dims=1) if H // nh == 32 else ctxs[:, 0::2].repeat_interleave(2, dim=1)
    elif bug == "ctx_exp_from_ffs":
        ex = stale["ffs"].reshape(-1)[:T * (H // 32)].view(T, H // 32)
    elif bug == "ctx_exp_ignored":
        ex = torch.zeros_like(ctxs)
    elif bug == "ctx_exp_stride_ff":
        flat = ctxs.reshape(-1)
        idx = torch.arange(T)[:, None] * (FF // 32) + torch.arange(H // 32)[None, :]
        ex = flat[idx % flat.numel()]
    out["ctxs_read"] = ex       # (what the out-projection read: says whether a planted bug acted)
    res = h_in.to(dt)
    if bug == "oproj_res_dropped":
        res = torch.zeros_like(res)
    elif bug == "oproj_res_h2":
        res = stale["h2"].to(dt)
    sw_o = W["sw_qkv"][:H] if bug == "sw_qkv_for_sw_o" else W["sw_o"]
    bo = torch.zeros(H) if bug == "bo_dropped" else W["bo"]
    t1 = _bf16(mm(mx_decode(ctx8, ex), e4(W["wo"])) * sw_o.to(dt) + bo.to(dt) + res)
    swap = bug == "ln_swapped"
    y1 = ln(t1, W["ln2_g" if swap else "ln1_g"], W["ln2_b" if swap else "ln1_b"])
    out["h2"] = h2 = _bf16(y1)
    a8, sa = quant_tokens(y1)
    if bug == "a8_stride":
        # written with row stride max(H, FF), read (and sliced) with row stride H
        buf = torch.zeros(T, max(H, FF), dtype=torch.uint8)
        buf[:, :H] = a8
        a8 = buf.reshape(-1)[:T * H].view(T, H).clone()
    out["a8"], out["sa"] = a8, sa
    # FFN1 -> GELU -> MX fp8
    sx = sai if bug == "ffn1_stale_sa" else sa
    bi = torch.zeros(FF) if bug == "bi_dropped" else W["bi"]
    pre = mm(e4(a8), e4(W["wi"])) * sx.to(dt)[:, None] * W["sw_i"].to(dt) + bi.to(dt)
    late_gelu = bug == "gelu_after_mx"
    act = pre if (bug == "no_gelu" or late_gelu) else F.gelu(pre)
    ff8, ffs = mx_quant(act.float())
    out["ff8"], out["ffs"] = ff8, ffs
    # FFN2 (block-scaled A) + residual -> bf16 tmp -> ln2 (+ fused quant)
    f = mx_decode(ff8, torch.zeros_like(ffs) if bug == "ff_exp_ignored" else ffs)
    if late_gelu:
        f = F.gelu(f)
    res = h_in if bug == "ffn2_res_h" else h2
    sw_o2 = W["sw_o"] if bug == "sw_o_for_sw_o2" else W["sw_o2"]
    bo2 = torch.zeros(H) if bug == "bo2_dropped" else W["bo2"]
    out["tmp"] = tmp = _bf16(mm(f, e4(W["wo2"])) * sw_o2.to(dt) + bo2.to(dt) + res.to(dt))
    y2 = ln(tmp, W["ln1_g" if swap else "ln2_g"], W["ln1_b" if swap else "ln2_b"])
    out["h"] = _bf16(y2)
    out["a8_out"], out["sa_out"] = quant_tokens(y2)
    return out


# --------------------------------------------------------------------------------- the checker
def row_err(out: torch.Tensor, ref: torch.Tensor) -> float:
    """max over rows of |out_r - ref_r|_2 / |ref_r|_2 (float64)."""
    out, ref = out.double(), ref.double()
    return float(((out - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).max())


def bytes_consistent(a8: torch.Tensor, sa: torch.Tensor, h2: torch.Tensor) -> float:
    """Share of the bytes of a per-token image (a8, sa) that the per-token rule can produce from
    the observed bf16 ``h2``.  The kernel quantises the fp32 LayerNorm value y, of which h2 is
    the bf16 rounding: |y - h2| <= half a bf16 ulp of h2.  That interval is 16 times narrower than
    an e4m3 step, so it pins the byte to one code, or to two neighbours where it straddles a
    rounding boundary; a byte agrees when it is the code of one end of the interval under the
    observed scale.  (Plain equality with e4m3(h2 / scale) cannot reach the per-kernel test's
    0.995, which compares with y itself: a relative 2^-9 perturbation moves 2-3 % of the values
    across an e4m3 boundary 2^-4 apart -- 0.973-0.980 for a correct emulation, reported as
    ``a8_bytes_exact``.)"""
    h = h2.float()
    mag = h.abs()
    _, e = torch.frexp(mag)
    half = torch.where(mag > 0, torch.ldexp(torch.ones_like(mag), e - 9), torch.zeros_like(mag))
    inv = (1.0 / sa.float())[:, None]
    lo = ((mag - half).clamp_min(0.0) * inv).to(E4M3).float()
    hi = ((mag + half) * inv).to(E4M3).float()
    got = a8.view(E4M3).float()
    sign_ok = (got == 0) | (torch.sign(got) == torch.sign(h))
    return float((sign_ok & ((got.abs() == lo) | (got.abs() == hi))).double().mean())


def check_layer(ho: dict, W: dict, cfg, batch, h_in, pooled=None, unit=None) -> dict:
    """{step: statistic} for one layer's observed hand-offs ``ho`` (emulate_layer's names; a8_in /
    sa_in included) against float64 recomputations from each step's own observed inputs, never
    from the previous step's reference.  For the e4m3-output steps also the element-wise
    measures of the per-kernel tests: ``ctx_exp`` / ``ff_exp`` (share of exponents on the MX
    rule), ``ctx_elem`` / ``ff_elem`` (share of elements inside the kernel test's bound),
    ``a8_bytes`` (byte agreement with the per-token rule) and ``sa`` (largest relative error).
    ``pooled`` / ``unit``: the forward's outputs; their statistics are the largest error in units
    of test_pool's tolerance (<= 1 passes)."""
    H, nh = cfg.hidden, cfg.heads
    d = torch.float64
    decw = lambda w, s: W[w].view(E4M3).to(d) * W[s].to(d)[:, None]  # noqa: E731

    def ln(x, g, b):
        return F.layer_norm(x.to(d), (H,), W[g].to(d), W[b].to(d), cfg.ln_eps)

    st = {}
    # qkv
    ref = dequant_tokens(ho["a8_in"], ho["sa_in"]) @ decw("wqkv", "sw_qkv").t() + W["bqkv"].to(d)
    st["qkv"] = row_err(ho["qkv"], ref)
    # ctx (test_attention_mx8_output's measures)
    ref = attention(ho["qkv"], batch.cu_seqlens, nh, H // nh, d)
    ctx = mx_decode(ho["ctx8"], ho["ctxs"]).to(d)
    st["ctx"] = row_err(ctx, ref)
    _, ref_ex = mx_quant(ref)
    st["ctx_exp"] = float((ho["ctxs"] == ref_ex).double().mean())
    blk = torch.pow(2.0, ho["ctxs"].double()).repeat_interleave(32, dim=1)
    st["ctx_elem"] = float(((ctx - ref).abs() <= ref.abs() * 0.07 + blk * 2.0 ** -8 + 2e-2)
                           .double().mean())
    # h2
    t1 = _bf16(ctx @ decw("wo", "sw_o").t() + W["bo"].to(d) + h_in.to(d))
    st["h2"] = row_err(ho["h2"], ln(t1, "ln1_g", "ln1_b"))
    # a8 (test_add_ln_fused_fp8_quant's measures)
    a = dequant_tokens(ho["a8"], ho["sa"])
    st["a8"] = row_err(a, ho["h2"])
    ref8, ref_sa = quant_tokens(ho["h2"])
    st["a8_bytes_exact"] = float((ho["a8"] == ref8).double().mean())
    st["a8_bytes"] = bytes_consistent(ho["a8"], ho["sa"], ho["h2"])
    st["sa"] = float(((ho["sa"].double() - ref_sa.double()).abs() / ref_sa.double()).max())
    # ff (test_gemm_fp8_mx_gelu_output's measures)
    ref = F.gelu(a @ decw("wi", "sw_i").t() + W["bi"].to(d))
    ff = mx_decode(ho["ff8"], ho["ffs"]).to(d)
    st["ff"] = row_err(ff, ref)
    _, ref_ex = mx_quant(ref)
    st["ff_exp"] = float((ho["ffs"] == ref_ex).double().mean())
    blk = torch.pow(2.0, ho["ffs"].double()).repeat_interleave(32, dim=1)
    st["ff_elem"] = float(((ff - ref).abs() <= ref.abs() * 0.0625 + blk * 2.0 ** -9 + 1e-3)
                          .double().mean())
    # tmp, h
    ref = ff @ decw("wo2", "sw_o2").t() + W["bo2"].to(d) + ho["h2"].to(d)
    st["tmp"] = row_err(ho["tmp"], ref)
    st["h"] = row_err(ho["h"], ln(ho["tmp"], "ln2_g", "ln2_b"))
    # pooled (test_pool's tolerances)
    if pooled is not None:
        ref = R.pool_ref(ho["h"], batch.cu_seqlens, cfg.pooling, cfg.normalize).to(d)
        st["pooled"] = float(((pooled.to(d) - ref).abs() / (1e-3 + 1e-3 * ref.abs())).max())
        if unit is not None:
            st["unit"] = float(((unit.to(d) - F.normalize(ref, dim=-1)).abs() / 1e-2).max())
    return st


# The acceptance numbers of the per-kernel tests (test_attention_mx8_output,
# test_add_ln_fused_fp8_quant, test_gemm_fp8_mx_gelu_output); sa: one bf16 rounding of the row
# maximum (2^-9) with a factor 2 on top.
CTX_EXP_MIN, FF_EXP_MIN, FF_ELEM_MIN, A8_BYTES_MIN, SA_RTOL = 0.99, 0.995, 0.999, 0.995, 2.0 ** -8

TAU_BF16 = {"minilm-l6": 0.02, "bge-base": 0.02, "e5-large": 0.02}
TAU_E4M3 = {"minilm-l6": 0.11, "bge-base": 0.11, "e5-large": 0.11}


def step_class(step: str, k: int) -> str:
    return "e4m3" if step in E4M3_STEPS or (step == "qkv" and k >= 2) else "bf16"


def tau(model: str, step: str, k: int) -> float:
    return (TAU_E4M3 if step_class(step, k) == "e4m3" else TAU_BF16)[model]


def failing_steps(st: dict, model: str, k: int) -> list:
    """The steps of check_layer's result that miss: the statistic above the class's tau, or one of
    the step's element-wise measures under the per-kernel test's acceptance number."""
    bad = [s for s in STEPS[:-1] if not st[s] <= tau(model, s, k)]
    extra = {"ctx": st["ctx_exp"] > CTX_EXP_MIN and st["ctx_elem"] == 1.0,
             "a8": st["a8_bytes"] > A8_BYTES_MIN and st["sa"] <= SA_RTOL,
             "ff": st["ff_exp"] > FF_EXP_MIN and st["ff_elem"] > FF_ELEM_MIN}
    bad += [s for s, ok in extra.items() if not ok and s not in bad]
    if "pooled" in st and not (st["pooled"] <= 1.0 and st.get("unit", 0.0) <= 1.0):
        bad.append("pooled")
    return sorted(bad, key=STEPS.index)


# --------------------------------------------------------------------------------- workspace
def workspace_views(enc, T: int, ws=None) -> dict:
    """The last layer's hand-offs sliced out of an fp8 HipEncoder's workspace after a forward of T
    tokens (``ws``: another 8-buffer workspace of the same encoder, a captured graph's), by the
    layout documented above fp8_layer in csrc/hip/bindings.cpp:

        ws[0] h  ws[1] h2  ws[2] qkv  ws[5] tmp      bf16 rows, T of them
        ws[3]    first T*H bytes: the attention output's e4m3 bytes
        ws[4]    bytes [0, T*FF): FFN1's e4m3 output, then T*FF/32 E8M0 exponents of it, then
                 T*H/32 E8M0 exponents of the attention output
        ws[6]    a8 as [T, H] bytes with row stride H      ws[7] sa, T floats

    Exponents come back unbiased (byte - 127), as mx_decode takes them.  Device tensors are
    touched through .cpu() copies of the slices only."""
    ws = enc._ws if ws is None else ws
    H, FF = enc.cfg.hidden, enc.cfg.ffn

    def raw(t, nbytes):       # the first nbytes of a buffer, as uint8 on the host
        flat = t.reshape(-1)
        n = -(-nbytes // flat.element_size())
        return flat[:n].cpu().view(torch.uint8)[:nbytes]

    out = {"h": ws[0][:T].cpu(), "h2": ws[1][:T].cpu(), "qkv": ws[2][:T].cpu(),
           "tmp": ws[5][:T].cpu()}
    out["ctx8"] = raw(ws[3], T * H).view(T, H)
    n_ff, n_ffs, n_ctxs = T * FF, T * (FF // 32), T * (H // 32)
    ffb = raw(ws[4], n_ff + n_ffs + n_ctxs)
    out["ff8"] = ffb[:n_ff].view(T, FF)
    out["ffs"] = ffb[n_ff:n_ff + n_ffs].view(T, FF // 32).int() - 127
    out["ctxs"] = ffb[n_ff + n_ffs:].view(T, H // 32).int() - 127
    out["a8"] = raw(ws[6], T * H).view(T, H)
    out["sa"] = ws[7][:T].cpu()
    return out


# --------------------------------------------------------------------------------- planted bugs
@dataclass(frozen=True)
class Planted:
    """An fp8 wiring bug planted into emulate_layer.  ``steps``: the steps of check_layer that
    must reject it (and, the checks being teacher-forced, the only ones that do); ``min_k``: the
    first layer it can act on (2 where it reads what the previous layer left in the workspace).
    An entry that only moves the attention output's exponents acts where the exponents it reads
    differ from the right ones (``acts``): a 23-token sentence's third layer, say, has one exponent
    for the whole row, and the miswired runtime computes the very same numbers there."""
    name: str
    bug: str
    steps: tuple
    min_k: int = 1

    def acts(self, ho: dict) -> bool:
        """Whether the bug changed anything in the planted layer's hand-offs ``ho``."""
        if not self.bug.startswith("ctx_exp_"):
            return True
        return float((ho["ctxs_read"] != ho["ctxs"]).double().mean()) >= 0.05


PLANTED = [
    Planted("QKV reads a stale a8/sa (the previous layer's ln1 image of h2: h_quantized wrongly "
            "true or quantize_out wrongly false)", "qkv_stale_a8", ("qkv",), 2),
    Planted("sa not applied in QKV", "qkv_no_sa", ("qkv",)),
    Planted("stale sa in FFN1 (the scales of h, not of h2)", "ffn1_stale_sa", ("ff",)),
    Planted("ctx exponents read one block off", "ctx_exp_block_off", ("h2",)),
    Planted("ctx exponents read from the FFN exponent region", "ctx_exp_from_ffs", ("h2",), 2),
    Planted("ctx exponents ignored", "ctx_exp_ignored", ("h2",)),
    Planted("FFN exponents ignored", "ff_exp_ignored", ("tmp",)),
    Planted("the [T, H/32] exponent row stride mistaken for FF/32", "ctx_exp_stride_ff", ("h2",)),
    Planted("out-projection residual dropped", "oproj_res_dropped", ("h2",)),
    Planted("out-projection residual taken from h2", "oproj_res_h2", ("h2",), 2),
    Planted("FFN2 residual taken from h instead of h2", "ffn2_res_h", ("tmp",)),
    Planted("sw_qkv[:H] used for sw_o", "sw_qkv_for_sw_o", ("h2",)),
    Planted("sw_o used for sw_o2", "sw_o_for_sw_o2", ("tmp",)),
    Planted("ln1 and ln2 parameters swapped", "ln_swapped", ("h2", "h")),
    Planted("bo dropped", "bo_dropped", ("h2",)),
    Planted("bi dropped", "bi_dropped", ("ff",)),
    Planted("bo2 dropped", "bo2_dropped", ("tmp",)),
    Planted("FFN1 without GELU", "no_gelu", ("ff",)),
    # (the pre-activation is stored, the consumer applies GELU to what it decodes: both ends show)
    Planted("GELU applied after the MX quantisation", "gelu_after_mx", ("ff", "tmp")),
    Planted("a8 written with row stride max(H, FF) while read with stride H", "a8_stride", ("a8",)),
]


# --------------------------------------------------------------------------------- shared cases
@functools.lru_cache(maxsize=None)
def probe(model: str):
    """(3-layer probe config, lively parameters with bf16 matrices, per-layer fp8 weights), built
    once per model and read-only."""
    cfg = dataclasses.replace(EP.probe_cfg(model), layers=LAYERS)
    params = EP.round_weights_bf16(EP.lively_params(cfg, seed=EP.PARAM_SEED))
    return cfg, params, [layer_weights(L) for L in params["layers"]]


@functools.lru_cache(maxsize=None)
def batch_for(model: str, name: str):
    cfg = probe(model)[0]
    return EP.make_batch(cfg, EP.get_batch(cfg, name))


def embed(params, cfg, b) -> torch.Tensor:
    return _bf16(R.embed_ln_ref(b.ids, b.pos, b.type_ids, params["wemb"], params["pemb"],
                                params["temb"], params["eln_g"], params["eln_b"], cfg.ln_eps))


@functools.lru_cache(maxsize=None)
def chain(model: str, name: str, variant: str = "f32") -> list:
    """The emulated 3-layer fp8 encoder on one probe batch: [(h_in, hand-offs)] per layer, each
    layer reading the image the one before left (quant_rows for the first)."""
    cfg, params, Ws = probe(model)
    b = batch_for(model, name)
    out, h, a8 = [], embed(params, cfg, b), None
    with torch.no_grad():
        for W in Ws:
            ho = emulate_layer(W, cfg, b, h, a8, variant=variant)
            out.append((h, ho))
            h, a8 = ho["h"], (ho["a8_out"], ho["sa_out"])
    return out


def checker_inputs(ho: dict, h_in: torch.Tensor, k: int) -> dict:
    """The hand-offs as the GPU test sees them for layer k: from the second layer on, a8_in /
    sa_in is not observable and is recreated by the per-token rule from the bf16 h_in."""
    ho = dict(ho)
    if k >= 2:
        ho["a8_in"], ho["sa_in"] = quant_tokens(h_in)
    return ho


@functools.lru_cache(maxsize=None)
def emulated_stats(model: str, name: str, k: int, variant: str = "f32", entry: Planted | None = None):
    """check_layer's result for layer k of the emulated encoder, optionally with a planted bug in
    that layer (then with ``acted``: Planted.acts), computed once and shared (read-only)."""
    cfg, params, Ws = probe(model)
    b = batch_for(model, name)
    ch = chain(model, name, variant)
    h_in, ho = ch[k - 1]
    with torch.no_grad():
        if entry is not None:
            a8 = None if k == 1 else (ch[k - 2][1]["a8_out"], ch[k - 2][1]["sa_out"])
            ho = emulate_layer(Ws[k - 1], cfg, b, h_in, a8, variant=variant, bug=entry.bug,
                               stale=ch[k - 2][1] if k >= 2 else None)
        pooled = R.pool_ref(ho["h"], b.cu_seqlens, cfg.pooling, cfg.normalize)
        st = check_layer(checker_inputs(ho, h_in, k), Ws[k - 1], cfg, b, h_in, pooled,
                         F.normalize(pooled, dim=-1).to(torch.bfloat16))
    if entry is not None:
        st["acted"] = entry.acts(ho)
    return st


def planted_ks(name: str) -> tuple:
    """The layers the planted entries are tried on: every one on the 23-token batch, the middle
    one (h_quantized and quantize_out both set) on the two large batches."""
    return (1, 2, 3) if name == "q1" else (2,)
