"""A test of the tests: the fp8 hand-off probe (tests/fp8_probe.py) on its CPU emulation alone.

For every model and probe batch the GPU tests use: both legitimate emulations of a CORRECT
fp8_layer pass every step of check_layer, every planted fp8 wiring bug is rejected at the step(s)
it names and nowhere else, the threshold table of the probe's docstring holds
(3 F <= tau <= P / 2 per model and class), and workspace_views slices a workspace packed by the
documented layout back bit-identically.
"""
import types

import pytest
import torch

import fp8_probe as P
from codename_symbiont_amd.ops import reference as R

CASES = list(P.cases())


def _line(st):
    return " ".join(f"{s}={st[s]:.4f}" for s in P.STEPS[:-1])


@pytest.mark.parametrize("model,name", CASES)
def test_probe_accepts_both_legitimate_emulations(model, name):
    for k in (1, 2, 3):
        for v in P.VARIANTS:
            st = P.emulated_stats(model, name, k, v)
            print(f"{model} {name} k={k} {v}: {_line(st)} ctx_exp={st['ctx_exp']:.4f} "
                  f"a8_bytes={st['a8_bytes']:.4f} (exact {st['a8_bytes_exact']:.4f}) "
                  f"sa={st['sa']:.5f} ff_exp={st['ff_exp']:.4f} ff_elem={st['ff_elem']:.4f}")
            assert P.failing_steps(st, model, k) == [], (k, v, st)
            assert st["ctx_elem"] == 1.0 and st["pooled"] <= 1.0 and st["unit"] <= 1.0
    # the two emulations are different computations: some borderline rounding falls the other way
    a, b = P.chain(model, name, "f32")[-1][1], P.chain(model, name, "f64_reversed")[-1][1]
    if name != "q1":
        assert not torch.equal(a["h"], b["h"])


@pytest.mark.parametrize("model,name", CASES)
def test_probe_rejects_every_planted_bug_at_its_step(model, name):
    for k in P.planted_ks(name):
        for e in P.PLANTED:
            if k < e.min_k:
                continue
            st = P.emulated_stats(model, name, k, "f32", e)
            if not st["acted"]:
                continue
            bad = P.failing_steps(st, model, k)
            print(f"{model} {name} k={k} {e.bug:20s} -> {bad}  {_line(st)}")
            assert bad == sorted(e.steps, key=P.STEPS.index), (e.name, k, bad, st)
            for s in e.steps:
                assert st[s] >= 2 * P.tau(model, s, k), (e.name, s, st[s])


def test_every_planted_bug_acts_on_every_model():
    """No entry is dropped silently: each acts on short_mix's middle layer of every model, and the
    list covers what the issue names."""
    assert len(P.PLANTED) == 20 and len({e.bug for e in P.PLANTED}) == 20
    for m in P.MODELS:
        for e in P.PLANTED:
            assert P.emulated_stats(m, "short_mix", 2, "f32", e)["acted"], (m, e.name)
    for m, n in CASES:        # and the first-layer class of the qkv step is planted on too
        if n == "q1":
            e = next(e for e in P.PLANTED if e.bug == "qkv_no_sa")
            assert P.step_class("qkv", 1) == "bf16" and P.emulated_stats(m, n, 1, "f32", e)["acted"]


@pytest.mark.parametrize("model", P.MODELS)
def test_threshold_table_holds(model):
    """F and P recomputed: 3 F <= tau <= P / 2 for both classes."""
    F = {"bf16": 0.0, "e4m3": 0.0}
    Pm = {"bf16": (float("inf"), None), "e4m3": (float("inf"), None)}
    for n in P.batches_for(model):
        for k in (1, 2, 3):
            for v in P.VARIANTS:
                st = P.emulated_stats(model, n, k, v)
                for s in P.STEPS[:-1]:
                    c = P.step_class(s, k)
                    F[c] = max(F[c], st[s])
        for k in P.planted_ks(n):
            for e in P.PLANTED:
                if k < e.min_k:
                    continue
                st = P.emulated_stats(model, n, k, "f32", e)
                if not st["acted"]:
                    continue
                for s in e.steps:
                    c = P.step_class(s, k)
                    if st[s] < Pm[c][0]:
                        Pm[c] = (st[s], (e.bug, n, k, s))
    for c, t in (("bf16", P.TAU_BF16[model]), ("e4m3", P.TAU_E4M3[model])):
        print(f"{model} {c}: F={F[c]:.4f} P={Pm[c][0]:.4f} {Pm[c][1]} tau={t}")
        assert 3 * F[c] <= t <= Pm[c][0] / 2, (c, F[c], Pm[c], t)


def test_attention_in_float64_is_the_reference():
    cfg = P.probe("bge-base")[0]
    b = P.batch_for("bge-base", "short_mix")
    qkv = torch.randn(b.num_tokens, 3 * cfg.hidden, generator=torch.Generator().manual_seed(1))
    ref = R.attention_ref(qkv, b.cu_seqlens, cfg.heads, cfg.head_dim)
    got = P.attention(qkv, b.cu_seqlens, cfg.heads, cfg.head_dim)
    empty = [i for i, n in enumerate(P.EP.get_batch(cfg, "short_mix").lens) if n == 0]
    assert empty and got.dtype == torch.float64
    assert torch.allclose(got.float(), ref, atol=1e-5, rtol=1e-5)


def test_quantisers_round_trip():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(37, 256, generator=g) * torch.logspace(-3, 3, 37)[:, None]
    x[5] = 0.0
    q, s = P.quant_tokens(x)
    d = P.dequant_tokens(q, s)
    assert torch.isfinite(d).all() and (d[5] == 0).all()
    # e4m3: 3 mantissa bits, 2^-4 relative; subnormals of the row scale below 2^-6 * scale
    assert ((d - x.double()).abs() <= x.double().abs() * 2.0 ** -4 + s.double()[:, None] * 2.0 ** -10).all()
    assert float(P.quant_tokens(d)[0].ne(q).double().mean()) == 0.0
    q, ex = P.mx_quant(x)
    d = P.mx_decode(q, ex)
    blk = torch.pow(2.0, ex.float()).repeat_interleave(32, dim=1)
    assert ((d - x).abs() <= x.abs() * 2.0 ** -4 + blk * 2.0 ** -10).all()
    assert (ex[5] == -127).all() and (q.view(torch.float8_e4m3fn).float().abs() <= 448).all()
    # the rule: the smallest exponent that keeps the block maximum under 448
    amax = x.view(37, 8, 32).abs().amax(-1)
    live = amax > 0
    assert (amax * torch.pow(2.0, -ex.float()) < 448)[live].all()
    assert (amax * torch.pow(2.0, -(ex.float() - 1)) >= 448)[live].all()


def test_bytes_consistent_counts_what_the_rule_can_produce():
    g = torch.Generator().manual_seed(3)
    y = torch.randn(64, 384, generator=g) * 1.7
    a8, sa = P.quant_tokens(y)                 # the kernel's image: of the fp32 value
    h2 = y.to(torch.bfloat16)                  # what the checker observes
    exact = float((P.quant_tokens(h2)[0] == a8).double().mean())
    assert P.bytes_consistent(a8, sa, h2) == 1.0 and 0.95 < exact < 0.995
    rolled = a8.roll(1, dims=1)                # a misplaced image is not consistent
    assert P.bytes_consistent(rolled, sa, h2) < 0.2
    flipped = a8 ^ 0x80                        # nor one with the signs lost
    assert P.bytes_consistent(flipped, sa, h2) < 0.2
    off = a8.clone()
    off[:, ::2] += 1                           # nor one a code off in every other byte
    assert P.bytes_consistent(off, sa, h2) < 0.6


@pytest.mark.parametrize("model", ["minilm-l6", "e5-large"])
def test_workspace_views_follow_the_documented_layout(model):
    """emulate_layer's hand-offs packed into byte buffers by the layout above fp8_layer (with the
    capacity and the row padding a real workspace has) come back bit-identical."""
    cfg = P.probe(model)[0]
    H, FF = cfg.hidden, cfg.ffn
    _, ho = P.chain(model, "short_mix")[1]
    T, cap = ho["h"].shape[0], 600
    g = torch.Generator().manual_seed(4)

    def junk(n, dtype):      # a workspace is never zeroed
        return torch.randint(0, 255, (n,), generator=g, dtype=torch.uint8).view(dtype)

    def rows(x, width):      # T rows at the head of a [cap, width] bf16 buffer
        buf = junk(cap * width * 2, torch.bfloat16).view(cap, width)
        buf[:T] = x
        return buf

    ctx = junk(cap * H * 2, torch.uint8)
    ctx[:T * H] = ho["ctx8"].reshape(-1)
    ff = junk(cap * FF * 2, torch.uint8)
    ff[:T * FF] = ho["ff8"].reshape(-1)
    o = T * FF
    ff[o:o + T * (FF // 32)] = (ho["ffs"] + 127).to(torch.uint8).reshape(-1)
    o += T * (FF // 32)
    ff[o:o + T * (H // 32)] = (ho["ctxs"] + 127).to(torch.uint8).reshape(-1)
    a8 = junk(cap * max(H, FF), torch.uint8)
    a8[:T * H] = ho["a8"].reshape(-1)
    sa = torch.rand(cap, generator=g)
    sa[:T] = ho["sa"]
    ws = [rows(ho["h"], H), rows(ho["h2"], H), rows(ho["qkv"], 3 * H),
          ctx.view(torch.bfloat16).view(cap, H), ff.view(torch.bfloat16).view(cap, FF),
          rows(ho["tmp"], H), a8.view(cap, max(H, FF)), sa, torch.zeros(4)]
    enc = types.SimpleNamespace(_ws=ws, cfg=cfg)
    got = P.workspace_views(enc, T)
    assert set(got) == {"h", "h2", "qkv", "tmp", "ctx8", "ctxs", "ff8", "ffs", "a8", "sa"}
    for k, v in got.items():
        assert v.shape == ho[k].shape and v.dtype == ho[k].dtype, k
        assert torch.equal(v, ho[k]), k
    # the views are copies of the hand-offs, in the order the checker reads them
    st = P.check_layer({**got, "a8_in": ho["a8_in"], "sa_in": ho["sa_in"]}, P.probe(model)[2][1],
                       cfg, P.batch_for(model, "short_mix"), P.chain(model, "short_mix")[1][0])
    assert st["h2"] <= P.TAU_BF16[model] and st["ff"] <= P.TAU_E4M3[model]
