"""prune_finish_kernel (prune_finish.hip): the pruned search's re-score + top-k + tier word in one
launch, against the composition it replaces -- rescore_bf16 then topk_select_counted on the same
buffers.

Lattice rows and queries (tests/lattice.py): every score is exact in fp32 whatever the summation
order, exact copies of each query's source row are planted and listed first among its
candidates, so the best score is tied four ways -- across the k-th place at k = 1 -- and the
counts 0, 1, k - 1, k, k + 1, cap and cap + 1 are mixed within one batch.  cap = 64 keeps every
list in the kernel's LDS; cap = 4096 sends the long lists through global memory (and through the
select's floor pass), the short ones of the same batch through LDS.
"""
import pytest
import torch

import lattice as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_ROWS = 8192
NQ_MAX = 256
N_SRC = 8          # planted sources; query q is a copy of source q % N_SRC
COPIES = 3         # copies per source: 4 identical rows
GUARD = 64
_DATA = {}


def _data(D):
    """(rows bf16 [N_ROWS, D], queries bf16 [NQ_MAX, D], candidate order int32 [NQ_MAX, N_ROWS],
    exact scores f32 [NQ_MAX, N_ROWS]): each query's order lists its source and the copies first
    (shuffled among themselves), then every other row in a seeded random order."""
    if D in _DATA:
        return _DATA[D]
    x = L.dense(N_ROWS, D, seed=D, device=DEV)
    sources = [17 + 1000 * j for j in range(N_SRC)]
    x, plan = L.with_duplicates(x, sources, COPIES, seed=D)
    q = torch.stack([x[sources[i % N_SRC]] for i in range(NQ_MAX)]).contiguous()
    g = torch.Generator(device="cpu").manual_seed(D + 1)
    order = torch.empty(NQ_MAX, N_ROWS, dtype=torch.int32)
    for i in range(NQ_MAX):
        src = sources[i % N_SRC]
        first = torch.tensor([src] + plan[src])
        first = first[torch.randperm(first.numel(), generator=g)]
        rest = torch.randperm(N_ROWS, generator=g)
        keep = torch.ones(N_ROWS, dtype=torch.bool)
        keep[first] = False
        order[i] = torch.cat([first, rest[keep[rest]]]).int()
    exact = q.float() @ x.float().t()
    _DATA[D] = (x.contiguous(), q, order.to(DEV), exact)
    return _DATA[D]


def _counts(nq, k, cap, shift):
    pat = [0, 1, k - 1, k, k + 1, cap, cap + 1]
    return torch.tensor([pat[(i + shift) % len(pat)] for i in range(nq)], dtype=torch.int32,
                        device=DEV)


def _guarded(nq, k, dtype, fill):
    buf = torch.full((2 * GUARD + nq * k,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + nq * k].view(nq, k)


@pytest.mark.parametrize("cap", [64, 4096])
@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("nq", [1, 33, 256])
@pytest.mark.parametrize("D", [384, 768, 1024])
def test_prune_finish_matches_rescore_then_select(D, nq, k, cap):
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import hip, stream_handle

    h, st = hip(), stream_handle()
    x, q_all, order, exact = _data(D)
    q = q_all[:nq].contiguous()
    ci = order[:nq, :cap].contiguous()
    # (every count of the pattern is met: a batch of one query is run once per count)
    for shift in range(-(-7 // nq)):
        what = f"D={D} nq={nq} k={k} cap={cap} shift={shift}"
        cnt = _counts(nq, k, cap, shift)
        # the composition: rescore_bf16 -> topk_select_counted
        cs0 = torch.full((nq, cap), float("nan"), device=DEV)
        s0 = torch.full((nq, k), -3.0, device=DEV)
        i0 = torch.full((nq, k), -3, dtype=torch.int32, device=DEV)
        ovf0 = torch.zeros(1, dtype=torch.int32, device=DEV)
        h.rescore_bf16(x.data_ptr(), q.data_ptr(), nq, D, ci.data_ptr(), cnt.data_ptr(), cap,
                       cs0.data_ptr(), st)
        h.topk_select_counted(cs0.data_ptr(), ci.data_ptr(), cnt.data_ptr(), cap, nq, 16, k,
                              s0.data_ptr(), i0.data_ptr(), ovf0.data_ptr(), st, reset_ovf=False)
        # the fused kernel: NaN where nothing may be read before it is written, guards around
        # the outputs, the tier word into the middle of a pinned buffer
        cs = torch.full((nq, cap), float("nan"), device=DEV)
        sbuf, s = _guarded(nq, k, torch.float32, -5.0)
        ibuf, i = _guarded(nq, k, torch.int32, -5)
        ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
        word = torch.full((4,), -9, dtype=torch.int32).pin_memory()
        base = h.host_device_ptr(word.data_ptr())
        assert base, "pinned host memory has no device address"
        tier = torch.tensor([7 + shift], dtype=torch.int32, device=DEV)
        K.prune_finish(x, q, ci, cnt, cs, k, s, i, ovf, tier=tier, host_word=base + 4)
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        assert word.tolist() == [-9, 7 + shift, -9, -9], f"{what}: tier word {word.tolist()}"
        torch.cuda.synchronize()
        # scores bit for bit, candidate scores too (NaN past each count: nothing else written)
        assert torch.equal(s, s0), f"{what}: top-k scores differ from rescore + select"
        assert torch.equal(cs.view(torch.int32), cs0.view(torch.int32)), f"{what}: cand_s differs"
        n_used = torch.minimum(cnt, torch.tensor(cap, device=DEV)).long()
        used = torch.arange(cap, device=DEV)[None, :] < n_used[:, None]
        assert bool(torch.isnan(cs[~used]).all()) and not bool(torch.isnan(cs[used]).any()), what
        assert int(ovf.item()) == int(ovf0.item()) == int(bool((cnt > cap).any())), what
        # ... and what the lattice says they are: the top k of the first min(count, cap) entries
        sc = torch.gather(exact[:nq], 1, ci.long())
        sc = torch.where(used, sc, torch.full_like(sc, float("-inf")))
        ref = torch.topk(sc, min(k, cap), dim=1).values
        assert torch.equal(s[:, :ref.shape[1]], ref), f"{what}: not the top k of the first cap"
        # ids: equal outside runs of equal scores; every id carries its slot's score, is listed
        # among the query's used candidates and appears once
        tied = torch.zeros_like(s, dtype=torch.bool)
        if k > 1:
            eq = s[:, 1:] == s[:, :-1]
            tied[:, 1:] |= eq
            tied[:, :-1] |= eq
        tied[:, k - 1] = True   # (the k-th place may tie with the first entry left out)
        assert not bool(((i != i0) & ~tied).any()), f"{what}: ids differ outside ties"
        have = i >= 0
        assert torch.equal(have, s > float("-inf")), what
        assert bool((i[~have] == -1).all()), f"{what}: a missing slot is not (-inf, -1)"
        got = torch.gather(exact[:nq], 1, i.clamp(min=0).long())
        assert torch.equal(got[have], s[have]), f"{what}: an id does not carry its score"
        pos_of = torch.full((nq, N_ROWS), cap, dtype=torch.long, device=DEV)
        pos_of.scatter_(1, ci.long(), torch.arange(cap, device=DEV).expand(nq, cap).contiguous())
        pos = torch.gather(pos_of, 1, i.clamp(min=0).long())
        assert bool((pos[have] < n_used[:, None].expand(nq, k)[have]).all()), \
            f"{what}: an id outside the query's candidates"
        srt = torch.sort(torch.where(have, i, -1 - torch.arange(k, device=DEV, dtype=torch.int32)
                                     .expand(nq, k)), dim=1).values
        assert not bool((srt[:, 1:] == srt[:, :-1]).any()), f"{what}: an id returned twice"
        # guards
        for buf, fill in ((sbuf, -5.0), (ibuf, -5)):
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all()), \
                f"{what}: a write outside the outputs"


def test_prune_finish_without_a_tier_pair_writes_no_word():
    from codename_symbiont_amd.ops import kernels as K
    from codename_symbiont_amd.ops._ext import hip

    D, nq, k, cap = 384, 33, 10, 64
    x, q_all, order, _ = _data(D)
    q, ci = q_all[:nq].contiguous(), order[:nq, :cap].contiguous()
    cnt = _counts(nq, k, cap, 0)
    cs = torch.full((nq, cap), float("nan"), device=DEV)
    s = torch.empty(nq, k, device=DEV)
    i = torch.empty(nq, k, dtype=torch.int32, device=DEV)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    word = torch.full((4,), -9, dtype=torch.int32).pin_memory()
    assert hip().host_device_ptr(word.data_ptr())
    K.prune_finish(x, q, ci, cnt, cs, k, s, i, ovf)
    torch.cuda.synchronize()
    assert word.tolist() == [-9] * 4
    tier = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="tier and host_word"):
        K.prune_finish(x, q, ci, cnt, cs, k, s, i, ovf, tier=tier)
    with pytest.raises(ValueError, match="k = 17"):
        K.prune_finish(x, q, ci, cnt, cs, 17, torch.empty(nq, 17, device=DEV),
                       torch.empty(nq, 17, dtype=torch.int32, device=DEV), ovf)
