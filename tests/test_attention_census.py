"""The test of the test: tests/attention_census.py against a plain-torch emulator of tiled online-softmax attention with injectable
faults.  Runs without a GPU.

Why the census exists.  The random-input checks of tests/test_llm_kernels_gpu.py (randn Q / K / V, 600 - 700 keys, allclose with
rtol = atol = 2e-2) let every one of these through - measured on the CPU with that test's shapes, bf16 inputs, fp32 reference:

    context (len, plen)   fault                                   max error   under rtol = atol = 2e-2
    700, 0                last key dropped                        0.008       passes
    700, 0                first key dropped                       0.012       passes
    700, 0                key 63 counted twice                    0.013       passes
    700, 0                last FOUR keys dropped                  0.017       passes
    650, 611              last key (the newest token) dropped     0.012       passes
    650, 611              last four keys dropped                  0.020       passes
    620, 611              last key dropped                        0.018       passes
    620, 611              first own key dropped                   0.015       passes
    620, 611              key 63 counted twice                    0.016       passes

(the softmax is diffuse and max |out| is ~0.22 at 700 keys: one key contributes less than the tolerance).  Here every such fault, and
the merge faults that need no wrong key at all, must be REJECTED by at least one of the three census patterns, at a short and at a
long context, while the unfaulted emulator - outputs rounded to bf16 / fp16, P optionally rounded - must pass all three."""
import math

import pytest
import torch

import attention_census as AC

FAULTS = ["drop_newest", "drop_first_own", "double_at_64", "causal_plus_1", "causal_minus_1", "own_index_from_1", "wrong_kv_head",
          "rescale_omitted", "empty_chunk_weight_1"]
H, HKV, D = 8, 2, 128
# (keys in the context, prefix keys, emulator tile): the short one fits one 64-key chunk of the kernels, whose four lane groups are
# four online-softmax partials of their own - hence the 16-key tile
CONTEXTS = {"short": (64, 20, 16), "long": (700, 611, 64)}


def emulate(q, k_own, v_own, k_pre, v_pre, slot, pslot, plen, n, scale, dtype, round_p=False, fault=None, tile=64):
    """Attention of q [R, H, D] (row r sees keys 0 .. n[r]-1 of [prefix slot | own slot]) the way the kernels do it: fp32 scores from
    the stored inputs, one un-normalised partial (max, sum, acc) per tile of keys, partials merged with exp(m_c - M), one empty
    trailing tile whose partial holds stale workspace, output rounded to the storage type.  `fault` breaks one thing."""
    R = q.shape[0]
    n = torch.as_tensor(n).long()
    L = int(n.max()) + 1                                     # one key beyond the longest row (what an off-by-one mask would admit)
    rep = H // HKV
    kvh = torch.arange(H) % HKV if fault == "wrong_kv_head" else torch.arange(H) // rep
    o0 = 1 if fault == "own_index_from_1" else 0
    K = torch.cat([k_pre[pslot, :, :plen], k_own[slot, :, o0:o0 + L - plen]], 1).float()[kvh]      # [H, L, D]
    V = torch.cat([v_pre[pslot, :, :plen], v_own[slot, :, o0:o0 + L - plen]], 1).float()[kvh]
    n_eff = n + (1 if fault == "causal_plus_1" else -1 if fault == "causal_minus_1" else 0)
    t = torch.arange(L)
    mult = (t[None, :] < n_eff[:, None]).float()                                                       # [R, L] times a key is counted
    rows = torch.arange(R)
    if fault == "drop_newest":
        mult[rows, n - 1] = 0
    if fault == "drop_first_own":
        mult[:, plen] = 0
    if fault == "double_at_64":
        mult[:, 63] *= 2
    s = torch.einsum("rhd,hld->rhl", q.float(), K) * scale                                              # fp32
    nt = -(-L // tile) + 1                                                                              # + the empty trailing tile
    ms, ls, accs = [], [], []
    for c in range(nt):
        sl = slice(c * tile, min(L, (c + 1) * tile))
        if sl.start >= L:
            ms.append(torch.full((R, H), -math.inf)); ls.append(torch.full((R, H), 1.0)); accs.append(torch.full((R, H, D), 3.0))
            continue
        w = mult[:, None, sl].expand(R, H, -1)
        sc = s[:, :, sl].masked_fill(w == 0, -math.inf)
        m = sc.max(-1).values
        p = torch.where(w > 0, torch.exp(sc - torch.where(m.isinf(), torch.zeros_like(m), m)[..., None]), torch.zeros_like(sc)) * w
        ls.append(p.sum(-1))
        if round_p:
            p = p.to(dtype).float()
        accs.append(torch.einsum("rhl,hld->rhd", p, V[:, sl]))
        ms.append(m)
    m, l, acc = torch.stack(ms, -1), torch.stack(ls, -1), torch.stack(accs, -2)                        # [R, H, nt], [R, H, nt, D]
    M = m.max(-1).values
    wgt = torch.where(m.isinf(), torch.zeros_like(m), torch.exp(m - M[..., None]))
    if fault == "empty_chunk_weight_1":
        wgt[..., -1] = 1.0
    if fault == "rescale_omitted":                          # the first tile that is not the row's maximum keeps its own scale
        order = (m < M[..., None]) & ~m.isinf()
        first = order.float().argmax(-1)
        hit = order.any(-1)
        ix = hit.nonzero()
        wgt[ix[:, 0], ix[:, 1], first[hit]] = 1.0
    out = (wgt[..., None] * acc).sum(-2) / (wgt * l).sum(-1)[..., None]
    return out.to(dtype)


def _pools(k_ctx, v_ctx, plen, dtype):
    """[3 slots] own and prefix pools around the context, the own slot with room behind its last key (poisoned V)"""
    L = k_ctx.shape[1]
    g = torch.Generator().manual_seed(7)
    mk = lambda t: torch.randn(3, HKV, t, D, generator=g).to(dtype)
    k_own, v_own, k_pre, v_pre = mk(L - plen + 8), mk(L - plen + 8), mk(plen + 8), mk(plen + 8)
    AC.put_context(k_ctx, v_ctx, plen, k_own, v_own, 1, k_pre, v_pre, 2)
    return k_own, v_own, k_pre, v_pre


def _cases(ctx, dtype):
    """the three patterns on one context: (name, q, pools, n, v_max); every row length plen+1 .. L.  The pools hold two more keys of
    the same sequence behind the longest row, so that a mask that admits one key too many reads real data."""
    L, plen, _ = CONTEXTS[ctx]
    scale = AC.f32(D ** -0.5)
    n = torch.arange(plen + 1, L + 1)
    kc, vc = AC.census_context(HKV, L + 2, D, dtype, seed=1)
    kn, vn = AC.needle_context(HKV, L + 2, D, dtype, seed=3)
    R = n.numel()
    # needles: the newest key, the first own key, the last prefix key, key 0, and a sweep
    hh = torch.arange(H)[None, :]
    cyc = (torch.arange(R)[:, None] + hh) % 5
    sweep = (torch.arange(R)[:, None] * H + hh) * 7 % n[:, None]
    tg = torch.where(cyc == 0, n[:, None] - 1, torch.where(cyc == 1, torch.full_like(sweep, plen), torch.where(
        cyc == 2, torch.full_like(sweep, plen - 1), torch.where(cyc == 3, torch.zeros_like(sweep), sweep))))
    signs = torch.where(torch.arange(R) % 2 == 0, 1.0, -1.0)
    return [("uniform", AC.q_uniform(R, H, D, dtype), _pools(kc, vc, plen, dtype), n, 1.0),
            ("ramp", AC.q_ramp(n, signs, H, D, dtype, scale), _pools(kc, vc, plen, dtype), n, 1.0),
            ("needle", AC.q_needle(kn, tg, H), _pools(kn, vn, plen, dtype), n, float(vn.float().abs().max()))]


def _check(ctx, dtype, round_p, fault):
    """names of the patterns that reject the emulator's output"""
    L, plen, tile = CONTEXTS[ctx]
    rejected = []
    for name, q, pools, n, v_max in _cases(ctx, dtype):
        k, v = AC.context_of(*pools, 1, 2, plen, L)
        ref = AC.reference(q, k, v, n)
        got = emulate(q, *pools, 1, 2, plen, n, AC.f32(D ** -0.5), dtype, round_p=round_p, fault=fault, tile=tile)
        try:
            AC.assert_census(got, ref, dtype, 1 if round_p else 0, v_max=v_max, what=f"{ctx} {name} {fault}")
        except AssertionError:
            rejected.append(name)
    return rejected


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("round_p", [False, True], ids=["p_fp32", "p_rounded"])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_the_unfaulted_emulator_passes_every_pattern(ctx, round_p, dtype):
    assert _check(ctx, dtype, round_p, None) == []


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_is_rejected_short_and_long(fault, ctx, dtype):
    L, plen, _ = CONTEXTS[ctx]
    assert (L <= 64) if ctx == "short" else (L >= 640)
    for round_p in (False, True):
        assert _check(ctx, dtype, round_p, fault), f"{fault} slipped through every pattern ({ctx}, P rounded: {round_p})"


def test_each_pattern_catches_what_it_is_for():
    """which pattern sees which fault (bf16, long context): wrong keys are the uniform census's, the merge faults the ramp's and the
    needle's, the GQA head map the needle's alone (the census V is the same in every KV head)"""
    seen = {f: set(_check("long", torch.bfloat16, False, f)) for f in FAULTS}
    for f in ("drop_newest", "drop_first_own", "double_at_64", "causal_plus_1", "causal_minus_1", "empty_chunk_weight_1"):
        assert "uniform" in seen[f], (f, seen[f])
    assert "uniform" not in seen["rescale_omitted"] and {"ramp", "needle"} <= seen["rescale_omitted"]
    assert seen["wrong_kv_head"] == {"needle"}
    assert "needle" in seen["own_index_from_1"]


def test_census_expected_counts_keys_per_dim():
    for Dm, du in ((128, None), (64, 40)):
        for n in (1, 2, 39, 40, 41, 127, 128, 129, 700):
            v = AC.census_v(n, Dm, torch.float64, d_used=du)
            assert torch.equal(AC.census_expected(torch.tensor(n), Dm, du), v.sum(0) / n)
    e = AC.census_expected(torch.tensor([700, 699]), 128)
    assert abs(e[0].sum().item() - 1) < 1e-12 and (e[0] - e[1]).abs().max().item() / e[0].max().item() > 0.16      # one key = 16 % of an entry


def test_uniform_reference_is_the_census_and_the_needle_is_its_key():
    dt = torch.bfloat16
    k, v = AC.census_context(HKV, 300, D, dt, seed=5)
    n = torch.arange(1, 301)
    ref = AC.reference(AC.q_uniform(300, H, D, dt), k, v, n)
    assert (ref - AC.census_expected(n, D)[:, None, :]).abs().max().item() < 1e-12
    kn, vn = AC.needle_context(HKV, 700, D, dt, seed=6)
    tg = AC.needle_sweep_targets(700, H)
    assert sorted(set(tg.flatten().tolist())) == list(range(700)) and bool((tg[:, 0] != tg[:, 1]).all())
    ref = AC.reference(AC.q_needle(kn, tg, H), kn, vn, torch.full((tg.shape[0],), 700))
    kvh = (torch.arange(H) // (H // HKV))[None].expand_as(tg)
    assert (ref - vn[kvh, tg].double()).abs().max().item() < 1e-4           # >= 0.9999993 of the mass on the needle
    # the ramp spans RAMP_SPAN in score from a row's first key to its last, up or down
    q = AC.q_ramp(torch.tensor([700, 700]), torch.tensor([1.0, -1.0]), H, D, dt, AC.f32(D ** -0.5))
    s = q[:, 0, 0].double()[:, None] * k[0, :, 0].double()[None, :300] * AC.f32(D ** -0.5)
    assert s[0, -1] > s[0, 0] and s[1, -1] < s[1, 0]


def test_reference_reads_prefix_then_own_with_gqa_and_scale():
    dt = torch.float16
    kn, vn = AC.needle_context(HKV, 90, D, dt, seed=8)
    k_own, v_own, k_pre, v_pre = _pools(kn, vn, 36, dt)
    k, v = AC.context_of(k_own, v_own, k_pre, v_pre, 1, 2, 36, 90)
    assert torch.equal(k, kn) and torch.equal(v, vn) and bool((v_own[1, :, 54:] == AC.POISON).all())
    q = torch.randn(4, H, D, generator=torch.Generator().manual_seed(9)).to(dt)
    n = torch.tensor([37, 50, 89, 90])
    ref = AC.reference(q, k, v, n, scale=0.05)
    for r in range(4):
        for h in range(H):
            p = ((kn[h // 4, :n[r]].double() @ q[r, h].double()) * AC.f32(0.05)).softmax(0)
            assert (ref[r, h] - p @ vn[h // 4, :n[r]].double()).abs().max().item() < 1e-12
    pr = AC.reference_probs(q, k, n, scale=0.05)
    assert pr.shape == (H, 4, 90) and not pr[:, 0, 37:].any() and (pr.sum(-1) - 1).abs().max().item() < 1e-12
    assert AC.flash_counts(3, 5, True).tolist() == [6, 7, 8] and AC.flash_counts(3, 5, False).tolist() == [8, 8, 8]


def test_checker_bound_and_verdicts():
    ref = torch.tensor([[[0.5, 0.0, 2.0]]], dtype=torch.float64)
    for dt, hu in ((torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
        ok = ref + torch.tensor([2 * hu * 0.5, 1e-5, -2 * hu * 2.0]) * 0.99
        AC.assert_census(ok, ref, dt, 0)
        with pytest.raises(AssertionError):
            AC.assert_census(ref + torch.tensor([2 * hu * 0.5 + 2e-5, 0, 0]), ref, dt, 0)
        AC.assert_census(ref + torch.tensor([2 * hu * 0.5 + 2e-5, 0, 0]), ref, dt, 1)           # one P rounding doubles the relative term
        with pytest.raises(AssertionError):
            AC.assert_census(ref + torch.tensor([0, 3e-5, 0]), ref, dt, 1)
        with pytest.raises(AssertionError, match="1 of 3"):
            AC.assert_census(torch.tensor([[[0.5, math.nan, 2.0]]]), ref, dt, 1)
        # terms64 (sum of p |V|, for signed V that cancels) widens the P-rounding term alone
        small, terms = torch.tensor([[[0.01]]], dtype=torch.float64), torch.tensor([[[1.0]]], dtype=torch.float64)
        AC.assert_census(small + hu, small, dt, 1, terms64=terms)
        for kw in ({"p_roundings": 0, "terms64": terms}, {"p_roundings": 1}):
            with pytest.raises(AssertionError):
                AC.assert_census(small + hu, small, dt, **kw)
