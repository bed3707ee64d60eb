"""Exact-integer census of the GEMM forms: operands, references and checkers (no tests here; tests/test_gemm_census.py is the test
of these helpers on the CPU, tests/test_gemm_census_gpu.py applies them to the kernels).

The idea.  x holds integers in [-R, R], w integers in [-R, R] times 2^-s.  Every product and every partial sum of a dot product is
then an integer times 2^-s below 2^24 in magnitude: exactly representable in fp32, so an fp32 accumulator holds the TRUE sum whatever
the order of the additions - wave splits of K, stream-K cuts, split-K slabs, the order inside the matrix core.  The epilogue then
rounds known values at known points, and the output of a correct kernel equals the fp64 reference, rounded where the kernel rounds,
bit for bit.  A dropped or doubled k-step, a partial rounded too early, truncation for round-to-nearest-even, a row taken from the
neighbouring tile all change bits (tests/test_gemm_census.py shows it on an emulator with those faults)."""
import math

import torch

SENTINEL = -1024.0                       # pre-fill of every output buffer: exact in bf16 / fp16, far outside any census output
GUARD = 4096                             # elements of sentinel on either side of an output
EPIS = ("none", "bias", "bias_resid", "resid", "resid_ss", "swiglu", "quick_gelu", "gelu")
EXACT_EPIS = ("none", "bias", "bias_resid", "resid", "resid_ss")
QUICK_GELU_ALPHA = float(torch.tensor(1.702, dtype=torch.float32))       # the kernels' constant is the fp32 one


def scale_exp(K, R=15):
    """s with outputs of x @ w^T (x, w * 2^s uniform integers in [-R, R]: variance R (R + 1) / 3 each) at a standard deviation of
    about 2: fp16 neither overflows nor goes subnormal, and most outputs need more bits than the storage type has."""
    return math.ceil(math.log2(R * (R + 1) / 3 * math.sqrt(K) / 2))


def _strided(t, pad, fill=3.0):
    """t as the leading columns of a buffer `pad` columns wider (the gap holds a value that would show in any product)"""
    if not pad:
        return t
    big = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=t.device)
    big[:, : t.shape[1]] = t
    return big[:, : t.shape[1]]


def operands(M, N, K, dt, seed, R=15, device="cpu", x_pad=0, w_pad=0):
    """x [M, K] of integers in [-R, R], w [N, K] of integers in [-R, R] times 2^-s, and s.  x_pad / w_pad > 0: that operand is a
    column slice of a buffer so many columns wider (strided rows)."""
    assert K * R * R < 2 ** 24, (K, R)                       # every partial sum of a dot product is an integer below 2^24 (times 2^-s)
    s = scale_exp(K, R)
    g = torch.Generator(device=device).manual_seed(seed)
    xi = torch.randint(-R, R + 1, (M, K), generator=g, device=device, dtype=torch.int32)
    wi = torch.randint(-R, R + 1, (N, K), generator=g, device=device, dtype=torch.int32)
    x64, w64 = xi.double(), wi.double() * 2.0 ** -s
    x, w = x64.to(dt), w64.to(dt)
    assert torch.equal(x.double(), x64) and torch.equal(w.double(), w64), "operands do not survive the cast to the storage type"
    return _strided(x, x_pad), _strided(w, w_pad), s


def counting(M, N, K, dt, device="cpu"):
    """All-ones operands: every output is K exactly (K has at most 8 significant bits, so K is a bf16 and an fp16 value) - a failure
    reads as 'this output summed K - 32 terms'."""
    assert K > 0 and K // (K & -K) < 256 and K < 65504, K
    return torch.ones(M, K, dtype=dt, device=device), torch.ones(N, K, dtype=dt, device=device)


def side_inputs(M, N, dt, seed, device="cpu", resid_pad=0):
    """bias [N] and resid [M, N]: integers in [-31, 31] times 2^-2"""
    g = torch.Generator(device=device).manual_seed(seed)
    bias = (torch.randint(-31, 32, (N,), generator=g, device=device, dtype=torch.int32).double() / 4).to(dt)
    resid = (torch.randint(-31, 32, (M, N), generator=g, device=device, dtype=torch.int32).double() / 4).to(dt)
    return bias, _strided(resid, resid_pad)


def product(x, w):
    """the exact product in fp64"""
    return x.double() @ w.double().t()


def reference(x, w, epi, bias, resid, dt, acc=None, want_pre=False):
    """_gemm_ref of tests/test_llm_kernels_gpu.py in fp64 with .to(dt) at the same rounding points; returns a tensor of dtype dt.
    epi: "none" r(acc) | "bias" r(acc + b) | "bias_resid" r(r(acc + b) + res) | "resid" / "resid_ss" r(r(acc) + res) (skinny_gemm with
    a residual, linear_resid_ss) | "swiglu" r(r(silu(g)) u), g, u = r(acc) of the gate / up halves of w's rows |
    "quick_gelu" / "gelu" of y = r(acc + b).  want_pre: also the pre-activation y (fp64) of the two GELUs."""
    acc = product(x, w) if acc is None else acc
    r = lambda t: t.to(dt).double()
    pre = None
    if epi == "none":
        out = r(acc)
    elif epi == "swiglu":
        F = acc.shape[1] // 2
        g, u = r(acc[:, :F]), r(acc[:, F:])
        out = r(r(g / (1 + torch.exp(-g))) * u)
    elif epi in ("resid", "resid_ss"):
        out = r(r(acc) + resid.double())
    else:
        y = pre = r(acc + bias.double())
        if epi == "bias":
            out = y
        elif epi == "quick_gelu":
            out = r(y / (1 + torch.exp(-QUICK_GELU_ALPHA * y)))
        elif epi == "gelu":
            out = r(0.5 * y * (1 + torch.erf(y * math.sqrt(0.5))))
        elif epi == "bias_resid":
            out = r(y + resid.double())
        else:
            raise ValueError(epi)
    out = out.to(dt)
    return (out, pre) if want_pre else out


def slab_reference(x, w, bounds):
    """fp32 [S, M, N]: slab i is the exact product over K elements bounds[i] .. bounds[i + 1] (each is exactly an fp32 value)"""
    out = torch.stack([product(x[:, a:b], w[:, a:b]) for a, b in zip(bounds[:-1], bounds[1:])])
    f = out.float()
    assert torch.equal(f.double(), out)
    return f


def ss_reference(h):
    """fp64 [M, N / 16]: sums of squares of each run of 16 values of h's rows"""
    M, N = h.shape
    return (h.double() ** 2).view(M, N // 16, 16).sum(-1)


def _blocks(bad):
    ix = bad.nonzero()
    return sorted({(int(m) // 32, int(n) // 32) for m, n in ix.tolist()[:100000]})


def assert_exact(got, ref, what=""):
    """got == ref entry for entry ([M, N], one dtype).  On failure: how many entries are wrong, the first ten (m, n, got, ref) and the
    32 x 32 blocks that hold a wrong entry - one tile, one wave, one row band or one column quad."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if torch.equal(got, ref):
        return
    g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    bad = (g2 != r2) | g2.isnan()
    ix = bad.nonzero()[:10].tolist()
    first = [(m, n, float(g2[m, n]), float(r2[m, n])) for m, n in ix]
    blocks = _blocks(bad)
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} entries differ; first (m, n, got, ref): {first}; "
                         f"32 x 32 blocks (m // 32, n // 32) with a wrong entry: {blocks[:40]}{' ...' if len(blocks) > 40 else ''}")


def _ordinal(t):
    """position of each value on the line of representable values of a 16-bit float type (+-0 -> 0)"""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def ulp_of(ref, dt):
    """spacing of dt's representable values at |ref| (fp64)"""
    mant, emin = (7, -126) if dt == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(ref.double().abs())
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), (e - 1).clamp(min=emin) - mant)


def assert_ulps(got, ref, max_ulps, max_share, what="", slack=None):
    """The activation epilogues (__expf / erff: equality is impossible): no entry of got more than max_ulps representable values from
    ref, and at most max_share of the entries differ at all.  slack (fp64, per entry): an absolute allowance on top - the entry then
    passes if |got - ref| <= max_ulps ulp(ref) + slack (the GELU's fp32 cancellation in 1 + erf).
    Where the caps of the callers come from.  SwiGLU rounds twice, r(silu(g)) and r(. u): each rounding can land one representable
    value from the reference's, so 2; quick-GELU and bias + act round once, so 1.  The share: with |g| <= 12 the relative error of
    __expf is a few 2^-21 against a half-ulp of 2^-12 (fp16; 2^-9 for bf16), so only a value within 2^-21 / 2^-12 = 2^-9 of a rounding
    boundary can flip - at worst about 2^-8 of the entries for the two roundings, 0.4 %; the cap is 1 %, the fp32 stand-in on the CPU
    shows <= 0.02 %.  GELU: 2 ulp(ref) for the rounding and erff, plus 2^-21 |y| for 1 + erf(y / sqrt 2) at negative y, where fp32
    leaves 1 + erf an absolute error of a few fp32 ulps of 1 (2^-23), times 0.5 |y|."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    assert not bool(got.isnan().any()), f"{what}: NaN in the output"
    dist = (_ordinal(got) - _ordinal(ref)).abs()
    if slack is None:
        bad = dist > max_ulps
    else:
        bad = (got.double() - ref.double()).abs() > max_ulps * ulp_of(ref, ref.dtype) + slack
    share = float((dist != 0).float().mean())
    if bool(bad.any()) or share > max_share:
        g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
        b2 = bad.reshape(-1, got.shape[-1]) if bool(bad.any()) else (dist != 0).reshape(-1, got.shape[-1])
        first = [(m, n, float(g2[m, n]), float(r2[m, n])) for m, n in b2.nonzero()[:10].tolist()]
        raise AssertionError(f"{what}: {int(bad.sum())} entries beyond {max_ulps} representable values (largest distance {int(dist.max())}), "
                             f"{share:.4%} of entries differ (cap {max_share:.2%}); first (m, n, got, ref): {first}; "
                             f"32 x 32 blocks: {_blocks(b2)[:40]}")
    return int(dist.max()), share


def guarded(M, N, dt, device, ldy=None, lead=0):
    """A sentinel-filled buffer [GUARD | lead | M rows of ldy | GUARD] and the [M, N] view of it that starts `lead` elements behind
    the front guard with row stride ldy: (buffer, view)."""
    ldy = N if ldy is None else ldy
    buf = torch.full((2 * GUARD + lead + M * ldy,), SENTINEL, dtype=dt, device=device)
    view = buf[GUARD + lead: GUARD + lead + M * ldy].view(M, ldy)[:, :N]
    return buf, view


def assert_guards(buf, view, what=""):
    """every element of buf outside the view still holds the sentinel: both guards, the lead and the gap columns of each row"""
    M, N = view.shape
    ldy = view.stride(0)
    start = view.storage_offset() - buf.storage_offset()
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    body = mask[start: start + M * ldy].view(M, ldy)
    body[:, :N] = False
    touched = mask & (buf != SENTINEL)
    assert not bool(touched.any()), f"{what}: {int(touched.sum())} elements outside the output were written, first at offset " \
                                    f"{int(touched.nonzero()[0])} (output starts at {start}, row stride {ldy}, N {N})"
