"""Probe for the encoder's WIRING (shared by test_encoder_probe_cpu.py and the GPU wiring tests).

The per-kernel tests are dense; what they cannot see is whether ``EncoderRuntime::forward`` wires
the kernels into the right network.  On ``random_params`` (weights N(0, 0.02), LayerNorms at
(1, 0)) the residual stream dominates: pooled outputs of different sentences are near parallel and
a cosine bound of 0.999 passes swapped LayerNorm parameters, a wrong softmax scale, a dropped
bias...  This module provides

* ``lively_params``: weights under which every sublayer matters,
* ``probe_cfg`` / ``probe_batches``: cut-down real configs and hand-built batches, one per route
  through ``EncoderRuntime::forward``,
* ``rel_err``: error relative to the spread BETWEEN rows (sentences or tokens),
* ``bf16_emulated_forward``: the legitimate noise floor (the fp32 oracle with bf16 hand-offs),
* ``PLANTED``: wiring bugs planted into the oracle (test code only, applied to copies),
* ``TAU_POOLED`` / ``TAU_TOKEN``: one threshold per model and level with 3 F <= tau <= P / 2.

Thresholds.  Everything below is measured on the CPU with the fp32 oracle, lively_params(seed=3)
and the probe batches; nothing comes from the HIP output.  Per model, over all its probe batches:
F = the largest rel_err of ``bf16_emulated_forward``, P = the smallest rel_err of the PLANTED
entries the level has to catch, tau chosen with 3 F <= tau <= P / 2.

    pooled         F       P (entry, batch)                        tau
    minilm-l6    0.0270  0.190 (softmax scale, eps_small)          0.09
    bge-base     0.0216  0.234 (softmax scale, q1)                 0.09
    mpnet-multi  0.0208  0.203 (softmax scale, q4)                 0.08
    e5-large     0.0227  0.220 (softmax scale, eps_small)          0.09

    token-level    F       P (entry, batch)                        tau
    minilm-l6    0.1085  2.82 (last token row unwritten, limit)    0.33
    bge-base     0.0363  1.93 (last token row unwritten, eps)      0.11
    mpnet-multi  0.0428  2.45 (last token row unwritten, short_mix) 0.13
    e5-large     0.0416  2.27 (last token row unwritten, limit)    0.13

A bug has to be caught at ONE level.  Every PLANTED entry but one clears 2 tau at the pooled level
on every batch it applies to (and the pool bug can show nowhere else); "last token row of the
batch never written" is averaged away by pooling (0.004 pooled) and is the token level's to
catch, so the token level's P is that entry's.  The token-level taus are therefore the tightest
the rule allows, 3 F rounded up; the token-level F is a maximum over several hundred rows with a
heavy tail (MiniLM: 0.03-0.07 on ten batches, 0.11 on the one-sentence batch).  The smallest
token-level effect of any other entry is 0.21-0.29 (softmax scale), i.e. above tau for the three
wide models too.

Different-sentence cosine of the pooled oracle output (the largest over sentence pairs): <= 0.958
on every real-eps batch of every model (bge-base <= 0.88), <= 0.977 on the eps = 0.5 batches,
where every normalised row shrinks by sqrt(1.5) against the same beta.  Mean max-probability of
the layer-0 softmax over a 128-token sentence: 0.39-0.43 for the four models (uniform would be
0.008, saturated 1).  The fp32 oracle takes 0.01-0.09 s per batch.

The HIP encoder's measured rel_err (MI355X; test_encoder_wiring_matches_oracle prints each), the
largest over the route's batches, pooled / token-level:

    route       minilm-l6        bge-base         mpnet-multi      e5-large
    default     0.0257 / 0.1172  0.0255 / 0.0361  0.0225 / 0.0466  0.0234 / 0.0483
    unfused     0.0230 / 0.0357  -                -                -
    own_tiles   -                0.0255 / 0.0239  -                0.0226 / 0.0284
    hipblaslt   -                0.0191 / 0.0236  0.0198 / 0.0259  0.0195 / 0.0254
    deferred    -                0.0217 / 0.0232  -                0.0236 / 0.0260
    graph       0.0247 / 0.0357  0.0193 / 0.0253  -                -

i.e. every route sits on the CPU-emulated bf16 floor F, a factor 3.5-3.8 (pooled) and 2.7-3
(token-level) under tau.
"""
from __future__ import annotations

import copy
import dataclasses
import functools
import math
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

from codename_symbiont_amd.models import get_config
from codename_symbiont_amd.models.encoder import PackedBatch, pack_token_ids
from codename_symbiont_amd.models.weights import random_params
from codename_symbiont_amd.ops import reference as R

MODELS = ("minilm-l6", "bge-base", "mpnet-multi", "e5-large")
PROBE_VOCAB = 4096
WORDS_PER_SENTENCE = 3
EPS_PROBE = 0.5          # the eps route's LayerNorm eps: ignoring it changes rows by ~sqrt(1.5)


# --------------------------------------------------------------------------------- configs
def probe_cfg(model: str, **over):
    """The real config with the vocabulary cut to 4096 rows and the three wide models cut to 4
    layers (layer 0 runs the plain QKV of the deferred forward, layers >= 1 the folded one; every
    layer runs the same code otherwise).  MiniLM keeps its 6.  Position table, offset, eps,
    type_vocab, pooling and heads stay real."""
    cfg = get_config(model)
    layers = cfg.layers if cfg.hidden == 384 else 4
    return dataclasses.replace(cfg, vocab_size=PROBE_VOCAB, layers=layers, **over)


# --------------------------------------------------------------------------------- weights
def lively_params(cfg, seed: int = 0) -> dict:
    """``random_params`` (N(0, 0.02) matrices, biases N(0, 0.01), LayerNorms (1, 0)) rescaled so
    that every sublayer's output is comparable to its residual input:

    * embeddings (word / position / type) x 50: std 1, so position and type rows matter as much
      as the word row;
    * every projection [N, K] x 50 / sqrt(K): unit gain (std 1 / sqrt(K));
    * the Q and K rows of wqkv x 2 on top: logits q.k / sqrt(d) of std ~4 -- a sharp but not
      saturated softmax (measured mean max-probability over heads and tokens of a 128-token
      sentence in layer 0: 0.39-0.43; sharper logits raise the bf16 floor as fast as the planted
      softmax-scale effect, a larger out-projection gain raises the token-level floor past 1);
    * biases x 30 (std 0.3);
    * every LayerNorm, the embedding one included: gamma = 1 + 0.3 N(0, 1), beta = 0.2 N(0, 1).

    Different-sentence cosine of the pooled oracle output stays <= DIFF_COS_MAX for every model
    on the probe batches (checked in test_encoder_probe_cpu.py; the batches help: make_batch
    gives each sentence a few words of its own)."""
    p = random_params(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)

    def ln(H):
        return (1.0 + 0.3 * torch.randn(H, generator=g), 0.2 * torch.randn(H, generator=g))

    for k in ("wemb", "pemb", "temb"):
        p[k] = p[k] * 50.0
    p["eln_g"], p["eln_b"] = ln(cfg.hidden)
    H = cfg.hidden
    for L in p["layers"]:
        for k in ("wqkv", "wo", "wi", "wo2"):
            L[k] = L[k] * (50.0 / math.sqrt(L[k].shape[1]))
        L["wqkv"][:2 * H] *= 2.0
        for k in ("bqkv", "bo", "bi", "bo2"):
            L[k] = L[k] * 30.0
        L["ln1_g"], L["ln1_b"] = ln(H)
        L["ln2_g"], L["ln2_b"] = ln(H)
    return p


# --------------------------------------------------------------------------------- batches
@dataclass(frozen=True)
class ProbeBatch:
    name: str
    route: str                 # the route through EncoderRuntime::forward this batch forces
    lens: tuple                # sentence lengths of one forward call
    type_ids: bool = False
    eps: float | None = None   # replace cfg.ln_eps (the eps route)
    over_limit: bool = False   # one token past the position table: must raise ValueError
    companion: str | None = None   # a one-sentence batch has no spread between sentences of its
    #                                own: its pooled row is measured among this batch's rows


def _limit(cfg) -> int:
    return cfg.max_position - cfg.position_offset


def probe_batches(cfg) -> list[ProbeBatch]:
    """Hand-built batches (<= ~1500 tokens), each naming the route it forces."""
    lim = _limit(cfg)
    out = [
        ProbeBatch("short_mix", "T > 256, max_len <= 128: MiniLM fused QKV+attention and fused "
                   "FFN; wide models hipBLASLt + add_ln; one 128-key attention tile",
                   (1, 2, 3, 63, 0, 64, 65, 127, 128, 17)),
        ProbeBatch("long_mix", "T > 256 with sentences of 129 and 200: the QKV GEMM + attention "
                   "pair and 64-key tiles", (129, 5, 200, 1, 64, 33)),
        ProbeBatch("t255", "T = 255 <= gemm_skinny_max_m(): every GEMM on the small-M path",
                   (100, 1, 90, 64)),
        ProbeBatch("t256", "T = 256 == gemm_skinny_max_m()", (100, 1, 91, 64)),
        ProbeBatch("t257", "T = 257: the first T on the tiled / fused route", (100, 1, 92, 64)),
        ProbeBatch("q1", "T <= 64, B = 1 (one 64-row block of the small-M path)", (23,),
                   companion="q4"),
        ProbeBatch("q4", "T <= 64, B = 4", (7, 1, 31, 20)),
        ProbeBatch("limit", "one sentence of max_position - position_offset tokens (its last "
                   "token reads the position table's last row)", (1, lim, 2, 40, 64, 17)),
        ProbeBatch("eps", "ln_eps = 0.5 in the config: every LayerNorm-bearing kernel must "
                   "honour eps (T > 256)", (40, 64, 1, 90, 128, 2), eps=EPS_PROBE),
        ProbeBatch("eps_small", "ln_eps = 0.5 on the small-M path (T <= 256)", (40, 1, 64, 2, 33, 17, 50),
                   eps=EPS_PROBE),
    ]
    if cfg.type_vocab >= 2:
        out.append(ProbeBatch("types", "type_ids: zeros then ones inside each sentence "
                              "(T > 256)", (2, 64, 1, 97, 128, 30), type_ids=True))
    return out


def get_batch(cfg, name: str) -> ProbeBatch:
    if name == "over_limit":
        return ProbeBatch("over_limit", "one token past the position table", (3, _limit(cfg) + 1),
                          over_limit=True)
    return next(b for b in probe_batches(cfg) if b.name == name)


def batch_cfg(cfg, pb: ProbeBatch):
    return cfg if pb.eps is None else dataclasses.replace(cfg, ln_eps=pb.eps)


def make_batch(cfg, pb: ProbeBatch, seed: int = 0) -> PackedBatch:
    rng = np.random.default_rng(seed + len(pb.lens) * 7919 + sum(pb.lens))
    # each sentence draws from its own pool of WORDS_PER_SENTENCE words: random words from the
    # whole vocabulary average out under mean pooling (every sentence then pools to the same
    # vector), a few repeated words give each sentence content of its own; positions still make
    # every token row different
    toks = []
    for n in pb.lens:
        words = rng.integers(5, cfg.vocab_size, size=WORDS_PER_SENTENCE).astype(np.int32)
        toks.append(words[rng.integers(0, WORDS_PER_SENTENCE, size=int(n))])
    b = pack_token_ids(toks, cfg)
    if pb.type_ids:
        tt = np.concatenate([(np.arange(n) >= n // 2).astype(np.int32) for n in pb.lens])
        b.type_ids = torch.from_numpy(tt)
    return b


# --------------------------------------------------------------------------------- measures
def rel_err(out: torch.Tensor, ref: torch.Tensor, among: torch.Tensor | None = None) -> torch.Tensor:
    """Per-row error relative to the spread between rows: |out_r - ref_r| / |ref_r - mean_r(ref)|.
    Rows are sentences for a pooled [B, H] output and tokens for a [T, H] hidden state (centred
    on the token mean).  ``among``: further reference rows that only take part in the mean (a
    one-sentence batch's companion: a single row has no spread of its own).  An all-zero
    reference row (a zero-length sentence's pooled output) has a spread like any other: its
    distance from the mean row."""
    out, ref = out.double(), ref.double()
    rows = ref if among is None else torch.cat([ref, among.double()])
    assert rows.shape[0] > 1, "rel_err needs more than one reference row"
    spread = (ref - rows.mean(0, keepdim=True)).norm(dim=1)
    return (out - ref).norm(dim=1) / spread.clamp_min(1e-30)


def diff_sentence_cos(pooled: torch.Tensor) -> float:
    """Largest cosine between the pooled outputs of two different non-empty sentences."""
    x = pooled.double()
    x = x[x.norm(dim=1) > 0]
    if x.shape[0] < 2:
        return -1.0
    c = F.normalize(x, dim=1) @ F.normalize(x, dim=1).t()
    c.fill_diagonal_(-1.0)
    return float(c.max())


# --------------------------------------------------------------------------------- the oracle
def _bf16(x):
    return x.to(torch.bfloat16).float()


def _ident(x):
    return x


def oracle_forward(params, cfg, b: PackedBatch, rnd=_ident, hooks: dict | None = None):
    """The fp32 oracle (ops/reference.py's operations, in encoder_ref's order) -> (hidden [T, H],
    pooled [B, H]).  With rnd = identity and no hooks it IS encoder_ref + pool_ref (asserted in
    test_encoder_probe_cpu.py); ``rnd`` is applied wherever the HIP runtime stores bf16, and
    ``hooks`` are the planted bugs' entry points."""
    hooks = hooks or {}
    H, nh = cfg.hidden, cfg.heads
    hd = H // nh
    attn = hooks.get("attention", R.attention_ref)
    act = hooks.get("act", F.gelu)
    skip = hooks.get("skip", ())     # {(layer, "attn" | "ffn")}: the sublayer's output dropped
    h = rnd(R.embed_ln_ref(b.ids, b.pos, b.type_ids, params["wemb"], params["pemb"],
                           params["temb"], params["eln_g"], params["eln_b"], cfg.ln_eps))
    for li, L in enumerate(params["layers"]):
        qkv = rnd(h @ L["wqkv"].float().t() + L["bqkv"].float())
        ctx = rnd(attn(qkv, b.cu_seqlens, nh, hd))
        a = ctx @ L["wo"].float().t() + L["bo"].float()
        if (li, "attn") in skip:
            a = torch.zeros_like(a)
        h2 = rnd(F.layer_norm(a + h, (H,), L["ln1_g"].float(), L["ln1_b"].float(), cfg.ln_eps))
        f = rnd(act(h2 @ L["wi"].float().t() + L["bi"].float()))
        o = f @ L["wo2"].float().t() + L["bo2"].float()
        if (li, "ffn") in skip:
            o = torch.zeros_like(o)
        h = rnd(F.layer_norm(o + h2, (H,), L["ln2_g"].float(), L["ln2_b"].float(), cfg.ln_eps))
    if "hidden" in hooks:
        h = hooks["hidden"](h)
    pool = hooks.get("pool", R.pool_ref)
    return h, pool(h, b.cu_seqlens, cfg.pooling, cfg.normalize)


def round_weights_bf16(params: dict) -> dict:
    mats = {"wemb", "pemb", "temb", "wqkv", "wo", "wi", "wo2"}
    out = {k: (_bf16(v) if k in mats else v) for k, v in params.items() if k != "layers"}
    out["layers"] = [{k: (_bf16(v) if k in mats else v) for k, v in L.items()}
                     for L in params["layers"]]
    return out


def bf16_emulated_forward(params, cfg, b: PackedBatch):
    """The oracle with the matrices rounded to bf16 and every tensor the HIP runtime stores in
    bf16 rounded at that point (embed-LN out, qkv, ctx, h2, ff, h); fp32 everywhere else.  The
    legitimate noise floor of a correct bf16 encoder."""
    return oracle_forward(round_weights_bf16(params), cfg, b, rnd=_bf16)


def _e4m3(x, dim):
    """Round to e4m3 with one scale per slice along ``dim`` (max |x| -> 448), as
    quant_weight_fp8 does per output channel and the runtime per token."""
    s = x.abs().amax(dim=dim, keepdim=True).clamp_min(1e-12) / 448.0
    return (x / s).to(torch.float8_e4m3fn).float() * s


def fp8_emulated_forward(params, cfg, b: PackedBatch):
    """e4m3 emulation of the fp8 encoder: the four projection matrices rounded per output
    channel, the activation entering each projection rounded per token, bf16 hand-offs as in
    bf16_emulated_forward.  (The runtime's block-scaled MX hand-offs for ctx and ff are finer
    than per-token, so this is a floor from the coarser side.)"""
    p = round_weights_bf16(params)
    for L in p["layers"]:
        for k in ("wqkv", "wo", "wi", "wo2"):
            L[k] = _e4m3(L[k], 1)
    H, nh = cfg.hidden, cfg.heads
    q = lambda x: _e4m3(x, 1)  # noqa: E731
    h = _bf16(R.embed_ln_ref(b.ids, b.pos, b.type_ids, p["wemb"], p["pemb"], p["temb"],
                             p["eln_g"], p["eln_b"], cfg.ln_eps))
    for L in p["layers"]:
        qkv = _bf16(q(h) @ L["wqkv"].t() + L["bqkv"].float())
        ctx = R.attention_ref(qkv, b.cu_seqlens, nh, H // nh)
        a = q(ctx) @ L["wo"].t() + L["bo"].float()
        h2 = _bf16(F.layer_norm(_bf16(a + h), (H,), L["ln1_g"].float(), L["ln1_b"].float(),
                                cfg.ln_eps))
        f = F.gelu(q(h2) @ L["wi"].t() + L["bi"].float())
        o = q(f) @ L["wo2"].t() + L["bo2"].float()
        h = _bf16(F.layer_norm(_bf16(o + h2), (H,), L["ln2_g"].float(), L["ln2_b"].float(),
                               cfg.ln_eps))
    return h, R.pool_ref(h, b.cu_seqlens, cfg.pooling, cfg.normalize)


# --------------------------------------------------------------------------------- planted bugs
@dataclass(frozen=True)
class Planted:
    """A wiring bug planted into the oracle.  ``apply(params, cfg, batch)`` works on copies and
    returns (params, cfg, batch, hooks); ``applies(cfg, pb, batch)`` says whether the bug can act
    on that model and batch at all."""
    name: str
    apply: object
    applies: object = field(default=lambda cfg, pb, b: True)


def _cp(params):
    return copy.deepcopy(params)


def _swap_ln(p, cfg, b):
    p = _cp(p)
    for L in p["layers"]:
        L["ln1_g"], L["ln2_g"] = L["ln2_g"], L["ln1_g"]
        L["ln1_b"], L["ln2_b"] = L["ln2_b"], L["ln1_b"]
    return p, cfg, b, {}


def _other_scale(p, cfg, b):
    # softmax scaled for the OTHER head_dim (32 <-> 64): 1/8 for 1/sqrt(32), or the reverse
    hd = cfg.head_dim
    other = 64 if hd == 32 else 32
    s = math.sqrt(hd) / math.sqrt(other)
    p = _cp(p)
    for L in p["layers"]:
        L["wqkv"][:cfg.hidden] *= s
        L["bqkv"][:cfg.hidden] *= s
    return p, cfg, b, {}


def _real_eps(p, cfg, b):
    # the eps route's ln_eps = 0.5 ignored: the kernel's usual constant instead
    return p, dataclasses.replace(cfg, ln_eps=1e-12), b, {}


def _leak_attention(qkv, cu_seqlens, n_heads, head_dim):
    """attention_ref where each sentence also attends to the first key of the next sentence."""
    H = n_heads * head_dim
    qkv = qkv.float()
    out = torch.zeros(qkv.shape[0], H)
    cu = cu_seqlens.tolist()
    T = qkv.shape[0]
    for i in range(len(cu) - 1):
        s, e = cu[i], cu[i + 1]
        if e <= s:
            continue
        ke = min(e + 1, T)
        sp = lambda x, n: x.view(n, n_heads, head_dim).transpose(0, 1)  # noqa: E731
        q = sp(qkv[s:e, :H], e - s)
        k = sp(qkv[s:ke, H:2 * H], ke - s)
        v = sp(qkv[s:ke, 2 * H:], ke - s)
        p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(head_dim), dim=-1)
        out[s:e] = (p @ v).transpose(0, 1).reshape(e - s, H)
    return out


def _leak(p, cfg, b):
    return p, cfg, b, {"attention": _leak_attention}


def _merged_attention(qkv, cu_seqlens, n_heads, head_dim):
    cu = cu_seqlens.tolist()
    merged = cu[0:-1:2] + [cu[-1]]
    return R.attention_ref(qkv, torch.tensor(merged, dtype=torch.int32), n_heads, head_dim)


def _merge(p, cfg, b):
    return p, cfg, b, {"attention": _merged_attention}


def _drop_last_ffn2_bias(p, cfg, b):
    p = _cp(p)
    p["layers"][-1]["bo2"] = torch.zeros_like(p["layers"][-1]["bo2"])
    return p, cfg, b, {}


def _last_row_unwritten(p, cfg, b):
    def hidden(h):
        h = h.clone()
        h[-1] = 0.0
        return h
    return p, cfg, b, {"hidden": hidden}


def _ffn_cols_lost(p, cfg, b):
    p = _cp(p)
    p["layers"][2]["wo2"][:, -128:] = 0.0
    return p, cfg, b, {}


def _head_dropped(p, cfg, b):
    p = _cp(p)
    hd = cfg.head_dim
    p["layers"][3]["wo"][:, 5 * hd:6 * hd] = 0.0
    return p, cfg, b, {}


def _pool_skips_last(p, cfg, b):
    def pool(h, cu_seqlens, mode, normalize):
        cu = cu_seqlens.tolist()
        outs = []
        for i in range(len(cu) - 1):
            s, e = cu[i], cu[i + 1]
            if mode == "cls":
                v = h[s] if e > s else torch.zeros(h.shape[1])
            else:
                v = h[s:e - 1].sum(0) / (float(e - s) + 1e-9) if e > s else torch.zeros(h.shape[1])
            outs.append(v)
        out = torch.stack(outs)
        return F.normalize(out, dim=-1) if normalize else out
    return p, cfg, b, {"pool": pool}


def _pos_zero(p, cfg, b):
    b = dataclasses.replace(b, pos=torch.full_like(b.pos, cfg.position_offset))
    return p, cfg, b, {}


def _pos_offset_wrong(p, cfg, b):
    # the offset of the other family: +2 on a BERT table, -2 on an XLM-R one
    d = -2 if cfg.position_offset else 2
    return p, cfg, dataclasses.replace(b, pos=b.pos + d), {}


def _relu(p, cfg, b):
    return p, cfg, b, {"act": F.relu}


def _drop_attn(p, cfg, b):
    return p, cfg, b, {"skip": {(1, "attn")}}


def _drop_ffn(p, cfg, b):
    return p, cfg, b, {"skip": {(2, "ffn")}}


def _types_ignored(p, cfg, b):
    return p, cfg, dataclasses.replace(b, type_ids=None), {}


def _bf16_hand_offs(p, cfg, b):
    raise AssertionError("the legitimate entry: run bf16_emulated_forward instead")


_multi = lambda cfg, pb, b: b.num_seqs > 1                                    # noqa: E731
_not_limit = lambda cfg, pb, b: b.max_len + 2 <= _limit(cfg)                  # noqa: E731

# The ten cases of the first table (the first is the LEGITIMATE one: it must be accepted) and the
# further wiring bugs.  Every other entry must be rejected wherever it applies.
LEGITIMATE = "bf16 rounding at every hand-off"
PLANTED = [
    Planted(LEGITIMATE, _bf16_hand_offs),
    Planted("ln1 / ln2 parameters swapped, every layer", _swap_ln),
    Planted("softmax scaled for the other head_dim", _other_scale,
            lambda cfg, pb, b: b.max_len > 1),
    Planted("the wrong LayerNorm eps", _real_eps, lambda cfg, pb, b: pb.eps is not None),
    Planted("each sentence attends to one key of the next sentence", _leak, _multi),
    Planted("last layer's FFN2 bias dropped", _drop_last_ffn2_bias),
    Planted("last token row of the batch never written", _last_row_unwritten),
    Planted("last 128 FFN columns lost in layer 2", _ffn_cols_lost),
    Planted("one head dropped in layer 3", _head_dropped),
    Planted("pool skips each sentence's last token", _pool_skips_last,   # (needs a short sentence)
            lambda cfg, pb, b: cfg.pooling == "mean" and 1 in pb.lens),
    Planted("positions all zero", _pos_zero, lambda cfg, pb, b: b.max_len > 1),
    Planted("position offset wrong by 2", _pos_offset_wrong, _not_limit),
    Planted("attention merged across sentence pairs", _merge, _multi),
    Planted("relu for gelu", _relu),
    Planted("layer 1's attention dropped", _drop_attn),
    Planted("layer 2's FFN dropped", _drop_ffn),
    Planted("type_ids ignored", _types_ignored, lambda cfg, pb, b: pb.type_ids),
]


def run_planted(entry: Planted, params, cfg, b: PackedBatch):
    p, c, bb, hooks = entry.apply(params, cfg, b)
    return oracle_forward(p, c, bb, hooks=hooks)


# --------------------------------------------------------------------------------- thresholds
DIFF_COS_MAX = 0.96        # real-eps batches
DIFF_COS_MAX_EPS = 0.98    # the eps = 0.5 batches
TAU_POOLED = {"minilm-l6": 0.09, "bge-base": 0.09, "mpnet-multi": 0.08, "e5-large": 0.09}
TAU_TOKEN = {"minilm-l6": 0.33, "bge-base": 0.11, "mpnet-multi": 0.13, "e5-large": 0.13}


def accepted(model: str, err_pooled: float, err_token: float | None) -> bool:
    """The verdict both test files use: within tau at every level that was compared."""
    ok = err_pooled <= TAU_POOLED[model]
    if err_token is not None:
        ok = ok and err_token <= TAU_TOKEN[model]
    return ok


# --------------------------------------------------------------------------------- shared cases
PARAM_SEED = 3


@functools.lru_cache(maxsize=None)
def params_for(model: str) -> dict:
    """lively_params of the probe config, computed once per process (read-only: copy to alter)."""
    return lively_params(probe_cfg(model), seed=PARAM_SEED)


@dataclass(frozen=True)
class Case:
    model: str
    pb: ProbeBatch
    cfg: object
    params: dict
    batch: PackedBatch
    hidden: torch.Tensor        # fp32 oracle, [T, H]
    pooled: torch.Tensor        # fp32 oracle, [B, H]
    among: torch.Tensor | None  # the companion batch's pooled oracle rows (one-sentence batches)

    def errs(self, hidden, pooled):
        """(pooled rel_err, token-level rel_err or None) of an output against this case's oracle."""
        ep = float(rel_err(pooled.float().cpu(), self.pooled, self.among).max())
        et = None if hidden is None else float(rel_err(hidden.float().cpu(), self.hidden).max())
        return ep, et


@functools.lru_cache(maxsize=None)
def case(model: str, name: str) -> Case:
    """The fp32 oracle's output for one model and probe batch, computed once and shared."""
    cfg0 = probe_cfg(model)
    pb = get_batch(cfg0, name)
    cfg = batch_cfg(cfg0, pb)
    params = params_for(model)
    b = make_batch(cfg, pb)
    with torch.no_grad():
        h, o = oracle_forward(params, cfg, b)
    among = case(model, pb.companion).pooled if pb.companion else None
    return Case(model, pb, cfg, params, b, h, o, among)
