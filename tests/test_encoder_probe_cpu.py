"""A test of the tests: the encoder probe (tests/encoder_probe.py) on the fp32 oracle alone.

For every model and probe batch: the bf16 emulation of a CORRECT encoder is accepted by the
thresholds the GPU wiring tests use, every planted wiring bug that can act on the batch is rejected
by at least one of them, and the pooled outputs of different sentences are not near parallel.
This pins the suite's discriminating power: a tolerance loosened later (tau x 10, say) fails here.

Margins: on the machine the thresholds were set on, 3 F <= tau <= P / 2 (encoder_probe's table).
F and P move a little with the BLAS's summation order, so this file pins the rule with some of
that margin spent: F <= tau / 2 and P >= 1.5 tau.
"""
import pytest
import torch

import encoder_probe as P
from codename_symbiont_amd.models.encoder import TorchEncoder

BATCHES = ("short_mix", "long_mix", "t255", "t256", "t257", "q1", "q4", "limit", "eps", "eps_small",
           "types")
BUGS = [e for e in P.PLANTED if e.name != P.LEGITIMATE]


def _cases():
    for m in P.MODELS:
        names = [pb.name for pb in P.probe_batches(P.probe_cfg(m))]
        assert set(names) <= set(BATCHES)
        for n in names:
            yield m, n


def test_every_probe_batch_is_listed():
    for m in P.MODELS:
        have = {pb.name for pb in P.probe_batches(P.probe_cfg(m))}
        want = set(BATCHES) - ({"types"} if P.probe_cfg(m).type_vocab < 2 else set())
        assert have == want, (m, have ^ want)


def test_probe_oracle_is_the_torch_encoder():
    """oracle_forward without hooks or rounding IS TorchEncoder (encoder_ref + pool_ref)."""
    for m, n in [("minilm-l6", "types"), ("mpnet-multi", "short_mix")]:
        c = P.case(m, n)
        enc = TorchEncoder(c.cfg, params=c.params)
        pooled, _ = enc.forward_packed(c.batch)
        assert torch.equal(pooled, c.pooled) and torch.equal(enc.last_hidden(), c.hidden)


def test_probe_config_keeps_the_real_architecture():
    from codename_symbiont_amd.models import get_config

    for m in P.MODELS:
        real, cfg = get_config(m), P.probe_cfg(m)
        assert cfg.vocab_size == 4096 and cfg.layers == (6 if m == "minilm-l6" else 4)
        for f in ("hidden", "heads", "ffn", "max_position", "position_offset", "ln_eps",
                  "type_vocab", "pooling", "normalize", "pad_token_id"):
            assert getattr(cfg, f) == getattr(real, f), (m, f)
        for pb in P.probe_batches(cfg):
            assert sum(pb.lens) <= 1500


@pytest.mark.parametrize("model,name", list(_cases()))
def test_probe_accepts_bf16_and_rejects_planted_bugs(model, name):
    c = P.case(model, name)
    tp, tt = P.TAU_POOLED[model], P.TAU_TOKEN[model]
    with torch.no_grad():
        eh, eo = P.bf16_emulated_forward(c.params, c.cfg, c.batch)
    fp, ft = c.errs(eh, eo)
    print(f"{model} {name}: T={c.batch.num_tokens} floor pooled={fp:.4f} token={ft:.4f}")
    assert P.accepted(model, fp, ft), (fp, ft)
    assert fp <= tp / 2 and ft <= tt / 2, f"noise floor too close to tau: {fp:.4f} {ft:.4f}"
    if c.batch.num_seqs > 1:
        cos = P.diff_sentence_cos(c.pooled)
        print(f"    different-sentence cosine {cos:.3f}")
        assert cos <= (P.DIFF_COS_MAX if c.pb.eps is None else P.DIFF_COS_MAX_EPS), cos
    for e in BUGS:
        if not e.applies(c.cfg, c.pb, c.batch):
            continue
        with torch.no_grad():
            ph, po = P.run_planted(e, c.params, c.cfg, c.batch)
        ep, et = c.errs(ph, po)
        print(f"    {e.name:55s} pooled={ep:.4f} token={et:.4f}")
        assert not P.accepted(model, ep, et), f"planted bug passes: {e.name} ({ep:.4f}, {et:.4f})"
        assert max(ep / tp, et / tt) >= 1.5, f"planted bug too close to tau: {e.name}"
        if c.cfg.pooling == "mean" and "never written" not in e.name:
            # the pooled output alone (all the deferred route can compare) catches it too
            assert ep > tp, f"planted bug passes the pooled threshold: {e.name} ({ep:.4f})"


def test_every_planted_bug_is_exercised():
    """No entry of PLANTED is skipped silently: each applies to some batch of EVERY model it can
    exist in (type_ids need type_vocab 2, the pool bug mean pooling)."""
    assert len(P.PLANTED) == 17 and P.PLANTED[0].name == P.LEGITIMATE
    for m in P.MODELS:
        cfg0 = P.probe_cfg(m)
        hit = {e.name: 0 for e in BUGS}
        for pb in P.probe_batches(cfg0):
            cfg = P.batch_cfg(cfg0, pb)
            b = P.make_batch(cfg, pb)
            for e in BUGS:
                hit[e.name] += bool(e.applies(cfg, pb, b))
        never = {n for n, k in hit.items() if k == 0}
        allowed = set()
        if cfg0.type_vocab < 2:
            allowed.add("type_ids ignored")
        if cfg0.pooling != "mean":
            allowed.add("pool skips each sentence's last token")
        assert never == allowed, (m, never)
    # and across the models every entry acts somewhere
    assert all(any(e.applies(P.batch_cfg(P.probe_cfg(m), pb), pb,
                             P.make_batch(P.batch_cfg(P.probe_cfg(m), pb), pb))
                   for m in P.MODELS for pb in P.probe_batches(P.probe_cfg(m))) for e in BUGS)


def test_rel_err_measures_against_the_spread_between_rows():
    ref = torch.tensor([[10.0, 0.0], [10.0, 2.0]])            # spread: 1 per row around (10, 1)
    out = ref + torch.tensor([[0.0, 0.5], [0.0, 0.0]])
    assert torch.allclose(P.rel_err(out, ref), torch.tensor([0.5, 0.0], dtype=torch.float64))
    one = P.rel_err(out[:1], ref[:1], among=ref[1:])          # a single row among its companions
    assert torch.allclose(one, torch.tensor([0.5], dtype=torch.float64))
    with pytest.raises(AssertionError):
        P.rel_err(out[:1], ref[:1])


def test_over_limit_batch_is_one_token_past_the_table():
    for m in P.MODELS:
        cfg = P.probe_cfg(m)
        assert max(P.get_batch(cfg, "limit").lens) == cfg.max_position - cfg.position_offset == 512
        b = P.make_batch(cfg, P.get_batch(cfg, "limit"))
        assert int(b.pos.max()) == cfg.max_position - 1
        assert max(P.get_batch(cfg, "over_limit").lens) == 513


@pytest.mark.parametrize("model", ["minilm-l6", "bge-base"])
def test_fp8_floor_sits_above_the_planted_effects(model):
    """Why test_encoder_fp8_close_to_fp32_oracle keeps its cosine check alone: the e4m3 emulation
    of a CORRECT fp8 encoder already misses the pooled threshold (tau <= P / 2) on lively
    parameters, so a spread-relative bound could not tell it from a miswired one."""
    c = P.case(model, "short_mix")
    with torch.no_grad():
        h, o = P.fp8_emulated_forward(c.params, c.cfg, c.batch)
    ep, et = c.errs(h, o)
    print(f"{model}: fp8 floor pooled={ep:.4f} token={et:.4f}")
    assert ep > 2 * P.TAU_POOLED[model]
