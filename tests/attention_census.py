"""Structured inputs, an fp64 reference and a rounding-sized checker for the attention kernels (plain torch, any device, no GPU needed to import).

Random Q / K / V make a diffuse softmax: at 700 keys one key carries ~1/700 of an output that is itself ~0.2 large, far below any
bf16-sized tolerance (the table in tests/test_attention_census.py).  The inputs here are built so that ONE missing, doubled, misplaced
or mis-masked key moves the output by a large factor, and the expected value is known from the operation itself:

  uniform census   q = 0: every admitted key weighs exactly 1/n; with the one-hot census V (V[t, t % D] = 1) output dim d is
                   count{t < n : t % D == d} / n.  A dropped or doubled key moves one entry by >= 16 % at 700 keys, by 100 % below 129.
  needle           K, V random, q = beta * K[kv head, t*]: key t* holds all but ~1e-6 of the mass, the output is V[t*] to rounding; a
                   kernel that skips t*, or reads the V row of another key, is off by O(1).
  ramp             q = (q0, 0, ...) against K[t, 0] = t / 512: the score rises (q0 > 0) or falls (q0 < 0) linearly by ~8 over the row's
                   keys, so the running maximum moves in every tile, or never - the rescale and the merge of partials, which the other
                   two do not exercise.  V is the census V.

A context is the LOGICAL key sequence [Hkv, L, D]; the entries read it as [prefix slot: keys 0..plen) ++ [own slot: key t at index
t - plen (+ own_off)], see context_of()."""
import math

import torch

HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # relative half-ulp of the two storage types (8 / 11 significant bits)
NEEDLE_BETA = 3.0
RAMP_DEN = 512.0            # K[t, 0] = t / RAMP_DEN: <= 1.4 at 704 keys, small against |K[t*]|^2 = D in the needle's own score
RAMP_SPAN = 8.0             # score difference between the first and the last key of a ramp row
POISON = 96.0               # V beyond the last logical key: a kernel that reads past the end shows it at once


def f32(x: float) -> float:
    """x as the kernel receives it through a C float argument"""
    return torch.tensor(float(x), dtype=torch.float32).item()


def census_v(T, D, dtype, device="cpu", d_used=None):
    """[T, D] one-hot census: V[t, t % d_used] = 1 (exact in bf16 and fp16); dims >= d_used stay zero (the padded-head layout)."""
    du = D if d_used is None else d_used
    v = torch.zeros(T, D, dtype=dtype, device=device)
    t = torch.arange(T, device=device)
    v[t, t % du] = 1
    return v


def census_expected(n, D, d_used=None):
    """fp64 [..., D]: what attention with equal weights over keys 0 .. n-1 of the census V gives: count{t < n : t % d_used == d} / n."""
    du = D if d_used is None else d_used
    n = torch.as_tensor(n).long()
    d = torch.arange(D, device=n.device)
    cnt = torch.div(n[..., None] - d + du - 1, du, rounding_mode="floor").clamp(min=0)
    cnt = torch.where(d < du, cnt, torch.zeros_like(cnt))
    return cnt.double() / n[..., None].double()


def _randn(shape, dtype, device, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(device=device, dtype=dtype)


def census_context(Hkv, L, D, dtype, device="cpu", seed=0, d_used=None):
    """K, V [Hkv, L, D] for the uniform census and the ramp: V = census; K[t, 0] = t / 512 (the ramp reads only this dim), the other
    dims random (the uniform census has q = 0 and must not care)."""
    du = D if d_used is None else d_used
    k = _randn((Hkv, L, D), dtype, device, seed)
    k[:, :, 0] = (torch.arange(L, device=device, dtype=torch.float32) / RAMP_DEN).to(dtype)
    k[:, :, du:] = 0
    v = census_v(L, D, dtype, device, d_used)[None].expand(Hkv, L, D).contiguous()
    return k, v


def needle_context(Hkv, L, D, dtype, device="cpu", seed=0, d_used=None):
    """K, V [Hkv, L, D] random (every KV head and every key its own rows)."""
    du = D if d_used is None else d_used
    k, v = _randn((Hkv, L, D), dtype, device, seed), _randn((Hkv, L, D), dtype, device, seed + 1)
    k[:, :, du:] = 0
    v[:, :, du:] = 0
    return k, v


def q_uniform(R, H, D, dtype, device="cpu"):
    return torch.zeros(R, H, D, dtype=dtype, device=device)


def q_ramp(n, signs, H, D, dtype, scale, device="cpu"):
    """[R, H, D]: q[r, :, 0] = signs[r] * q0(n[r]) with q0 chosen so that the score moves by RAMP_SPAN over the row's n[r] keys (capped
    for very short rows; whatever the rounded q is, the reference uses the same one)."""
    n = torch.as_tensor(n, device=device).double()
    q0 = (RAMP_SPAN * RAMP_DEN / (n * scale)).clamp(max=8192.0) * torch.as_tensor(signs, device=device).double()
    q = torch.zeros(n.numel(), H, D, dtype=torch.float64, device=device)
    q[:, :, 0] = q0[:, None]
    return q.to(dtype)


def q_needle(k_ctx, targets, H, beta=NEEDLE_BETA):
    """[R, H, D]: q[r, h] = beta * K[kv head of h, targets[r, h]], rounded to the storage type."""
    Hkv = k_ctx.shape[0]
    kvh = (torch.arange(H, device=k_ctx.device) // (H // Hkv))[None].expand_as(targets)
    return (beta * k_ctx[kvh, targets.long()].float()).to(k_ctx.dtype)


def needle_sweep_targets(L, H, device="cpu"):
    """[ceil(L / H), H]: every key 0 .. L-1 is the needle of some (row, head); heads that share a KV head get different needles."""
    R = -(-L // H)
    return (torch.arange(R * H, device=device) % L).view(R, H)


def context_of(k_own, v_own, k_pre, v_pre, slot, pslot, plen, L, own_off=0):
    """The logical K, V [Hkv, L, D] that a row (slot, len <= L, pslot, plen) reads from the pools [n_slots, Hkv, t, D]."""
    k = torch.cat([k_pre[pslot, :, :plen], k_own[slot, :, own_off:own_off + L - plen]], 1)
    v = torch.cat([v_pre[pslot, :, :plen], v_own[slot, :, own_off:own_off + L - plen]], 1)
    assert k.shape[1] == L, "pools too short for this context"
    return k, v


def put_context(k_ctx, v_ctx, plen, k_own, v_own, slot, k_pre, v_pre, pslot, own_off=0):
    """Write a logical context into the pools the way the entries read it; V behind the last key is poisoned."""
    L = k_ctx.shape[1]
    if plen:
        k_pre[pslot, :, :plen], v_pre[pslot, :, :plen] = k_ctx[:, :plen], v_ctx[:, :plen]
        v_pre[pslot, :, plen:] = POISON
    k_own[slot, :, own_off:own_off + L - plen], v_own[slot, :, own_off:own_off + L - plen] = k_ctx[:, plen:], v_ctx[:, plen:]
    v_own[slot, :, own_off + L - plen:] = POISON


def reference(q, k_ctx, v_ctx, n, scale=None, abs_v=False):
    """fp64 attention of q [R, H, D] over keys 0 .. n[r]-1 of the logical context [Hkv, L, D] (GQA: head h reads KV head h // (H / Hkv)).
    A causal prefill is the same thing with n[i] = pos0 + i + 1, a non-causal one with n = pos0 + Tq.  Returns [R, H, D] fp64.
    abs_v: sum_t p_t |V_t| instead (the size of the terms of the sum, for assert_census's P-rounding term)."""
    R, H, D = q.shape
    Hkv, L, _ = k_ctx.shape
    scale = f32(D ** -0.5 if scale is None else scale)
    n = torch.as_tensor(n, device=q.device).long()
    assert int(n.min()) >= 1 and int(n.max()) <= L
    rep = H // Hkv
    K = k_ctx.double().repeat_interleave(rep, 0)
    V = v_ctx.double().repeat_interleave(rep, 0)
    V = V.abs() if abs_v else V
    s = torch.einsum("rhd,hld->rhl", q.double(), K) * scale
    s = s.masked_fill((torch.arange(L, device=q.device)[None, :] >= n[:, None])[:, None, :], -math.inf)
    return torch.einsum("rhl,hld->rhd", s.softmax(-1), V)


def reference_probs(q, k_ctx, n, scale=None):
    """fp64 [H, R, L]: the softmax map itself (zeros behind each row's n keys)."""
    R, H, D = q.shape
    Hkv, L, _ = k_ctx.shape
    scale = f32(D ** -0.5 if scale is None else scale)
    n = torch.as_tensor(n, device=q.device).long()
    s = torch.einsum("rhd,hld->hrl", q.double(), k_ctx.double().repeat_interleave(H // Hkv, 0)) * scale
    s = s.masked_fill((torch.arange(L, device=q.device)[None, :] >= n[:, None])[None], -math.inf)
    return s.softmax(-1)


def flash_counts(Tq, pos0, causal, device="cpu"):
    """keys seen by the Tq query rows of a prefill sequence that starts at position pos0"""
    i = torch.arange(Tq, device=device)
    return pos0 + i + 1 if causal else torch.full((Tq,), pos0 + Tq, device=device)


def assert_census(got, ref64, dtype, p_roundings, v_max=1.0, what="", terms64=None):
    """Every (row, head, dim) of `got` within (1 + p_roundings) * 2 * halfulp(dtype) * |ref| + 1e-5 * max|V| of the fp64 reference.
    halfulp = 2^-8 (bf16) / 2^-11 (fp16) is the relative error of ONE rounding to the storage type.  2 * halfulp: the output rounding,
    and one ulp in all when the kernel's fp32 value sits a hair on the other side of a rounding boundary from the exact one.
    p_roundings = 1 where the kernel rounds P to the storage type before P V (every term of the numerator moves by <= half an ulp,
    the fp32 denominator does not), 0 where P stays in fp32; 1e-5 * max|V| covers fp32 accumulation and __expf.  These are derived
    bounds, not measurements of any kernel.
    terms64 (widens the P-rounding term only): reference(..., abs_v=True) = sum_t p_t |V_t|.  Rounding every p_t once moves the numerator
    by up to halfulp * sum_t p_t |V_t|, and that is |ref| only while the terms have one sign: always for the census V, and for a
    random V while the needle holds all the mass.  Where it does not - 40-dim heads: two keys share a row 0.66 / 0.33 - the V rows
    cancel and |ref| falls far below the terms, so a kernel that rounds P exactly as allowed misses a bound written on |ref|.  The
    needle checks of the P-rounding kernels pass it; with a concentrated needle it changes nothing."""
    got64 = got.double().reshape(ref64.shape)
    p_term = ref64.abs() if terms64 is None else torch.maximum(terms64.reshape(ref64.shape), ref64.abs())
    tol = 2 * HALF_ULP[dtype] * (ref64.abs() + p_roundings * p_term) + 1e-5 * float(v_max)
    err = (got64 - ref64).abs()
    bad = ~(err <= tol)                                     # NaN / inf count as wrong
    if bool(bad.any()):
        idx = bad.nonzero()
        lines = [f"{tuple(i.tolist())}: got {got64[tuple(i)].item():.6g} want {ref64[tuple(i)].item():.6g}" for i in idx[:8]]
        first = sorted(set(idx[:, 0].tolist()))
        raise AssertionError(f"{what}: {idx.shape[0]} of {bad.numel()} entries outside the census bound, in {len(first)} rows "
                             f"(first rows {first[:12]}); worst |err| / tol = {(err / tol)[bad].nan_to_num(posinf=1e30).max().item():.3g}\n  "
                             + "\n  ".join(lines))
