"""The test of the test: tests/gemm_census.py against a plain-torch emulator of a tiled stream-K GEMM with injectable faults.
Runs without a GPU.

Why the census exists.  The random-input checks (tests/test_llm_kernels_gpu.py, tests/test_gemm_guard_gpu.py: randn operands, largest
absolute error <= 2^-7 max|ref| + 1e-3, the tightest bound of the suite) accept a kernel with any of these faults - asserted below on
the emulator, bf16 and fp16, at K = 384 and K = 13824 (OLD_BOUND_ACCEPTS):

    partial_rounded   one stream-K partial rounded to the storage type before it is added
    truncate          truncation instead of round-to-nearest-even at the output
    ties_away         ties rounded away from zero (randn operands meet no tie at all)
    resid_early       the residual added before the first rounding instead of after it

A dropped 32-deep k-step (fault 1) is NOT among them on the emulator: at K = 13824 its largest error on randn operands is 3.3 % of
max|ref| (0.34 against 10.25), beyond 2^-7 and the 2e-2 of the weight-streaming tests and at the edge of the 3e-2 of the guard test -
those bounds see it only through the one largest entry of the one tile it hits, the census through every entry of that tile.

The census (integer operands times a power of two, equality with the fp64 reference) must reject every one of the ten faults at both
depths, while the unfaulted emulator - K cut into 128-deep units handed to workgroups in stream-K order, each wave's slice walked in
batches of 8 x 32, every fp32 sum taken in a SHUFFLED order, one rounding at the end - passes for every shuffle seed."""
import math

import pytest
import torch

import gemm_census as GC

FAULTS = ["drop_kstep", "double_kstep", "partial_twice", "partial_rounded", "truncate", "ties_away", "rows_from_previous_tile",
          "last_quad_unwritten", "swiglu_neighbour_pair", "resid_early"]
OLD_BOUND_ACCEPTS = ["partial_rounded", "truncate", "ties_away", "resid_early"]      # under 2^-7 max|ref| + 1e-3, both depths, both types
DTYPES = [torch.bfloat16, torch.float16]
BM = BN = 32
M_, N_ = 70, 76             # 3 x 3 tiles: a ragged last row tile of 6 rows, N % 8 == 4 (a last column quad), 12 columns in the last tile
F_ = 40                     # SwiGLU: 2 F = 80 rows of w
WG, WAVES = 7, 4            # "workgroups" of the stream-K cut; waves that split a segment's K


def _from_ordinal(o, dt):
    """inverse of gemm_census._ordinal"""
    bits = torch.where(o < 0, (-o) | 0x8000, o)
    return torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(dt)


def _round_to(t64, dt, mode):
    """fp64 -> dt: 'rne' (the type's own conversion), 'truncate' (towards zero), 'ties_away'"""
    near = t64.to(dt)
    if mode == "rne":
        return near
    o, sg = GC._ordinal(near), torch.sign(t64).to(torch.int32)
    lo_o = torch.where(near.double().abs() > t64.abs(), o - sg, o)        # the representable neighbour towards zero (t64 itself if exact)
    lo = _from_ordinal(lo_o, dt)
    if mode == "truncate":
        return lo
    hi = _from_ordinal(lo_o + sg, dt)
    tie = (lo.double() != t64) & ((t64 - lo.double()).abs() == (hi.double() - t64).abs())
    return torch.where(tie, hi, near)


def emulate(x, w, dt, epi="none", bias=None, resid=None, seed=0, fault=None):
    """x [M, K] @ w [Nw, K]^T the way the kernels do it, in fp32: BM x BN tiles, K in 128-deep units dealt to WG workgroups as
    contiguous unit ranges over (tile, unit) in stream-K order; inside a segment WAVES waves split the 32-deep k-steps and walk them in
    batches of 8 with a ragged tail; k-steps, wave sums and stream-K partials are each added in an order shuffled by `seed`; the
    epilogue rounds once per rounding point.  Returns ([M, N_out] of dtype dt pre-filled with the sentinel, tiles that were cut)."""
    rng = torch.Generator().manual_seed(seed)
    perm = lambda n: torch.randperm(n, generator=rng).tolist()
    M, K = x.shape
    Nw = w.shape[0]
    xf, wf = x.float(), w.float()
    Mt, Nt, UP = -(-M // BM), -(-Nw // BN), K // 128
    tiles = [(tm, tn) for tn in range(Nt) for tm in range(Mt)]
    U = len(tiles) * UP
    bounds = [i * U // WG for i in range(WG + 1)]
    parts = {t: [] for t in range(len(tiles))}                                  # tile -> [(unit0, unit1)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        u = a
        while u < b:
            t = u // UP
            e = min(b, (t + 1) * UP)
            parts[t].append((u - t * UP, e - t * UP))
            u = e
    cut = [t for t, p in parts.items() if len(p) > 1]
    victim = cut[len(cut) // 2] if cut else len(tiles) // 2                     # the tile that takes the K faults
    acc = torch.zeros(M, Nw, dtype=torch.float32)
    for t, (tm, tn) in enumerate(tiles):
        rows = slice(tm * BM, min(M, (tm + 1) * BM))
        cols = slice(tn * BN, min(Nw, (tn + 1) * BN))
        xr = xf[rows]
        if fault == "rows_from_previous_tile" and tm == Mt - 1 and tm > 0:
            xr = xf[(tm - 1) * BM: (tm - 1) * BM + (rows.stop - rows.start)]
        partials = []
        for pi, (u0, u1) in enumerate(parts[t]):
            steps = list(range(u0 * 4, u1 * 4))                                 # 32-deep k-steps of this segment
            per = -(-len(steps) // WAVES)
            wave_sums = []
            for wv in range(WAVES):
                mine = steps[wv * per: (wv + 1) * per]
                if not mine:
                    continue
                batches = [mine[i: i + 8] for i in range(0, len(mine), 8)]      # the last one is the ragged tail
                if t == victim and pi == 0 and wv == 0:
                    if fault == "drop_kstep":
                        batches[-1] = batches[-1][:-1]
                    if fault == "double_kstep":
                        batches[-1] = batches[-1] + batches[-1][-1:]
                order = [k for b_ in batches for k in b_]
                s_ = torch.zeros(xr.shape[0], cols.stop - cols.start, dtype=torch.float32)
                for j in perm(len(order)):
                    k = order[j]
                    s_ = s_ + xr[:, k * 32: (k + 1) * 32] @ wf[cols, k * 32: (k + 1) * 32].t()
                wave_sums.append(s_)
            p_ = torch.zeros_like(wave_sums[0])
            for j in perm(len(wave_sums)):
                p_ = p_ + wave_sums[j]
            partials.append(p_)
        if t == victim and fault == "partial_twice":
            partials.append(partials[-1])
        if t == victim and fault == "partial_rounded":
            partials[-1] = partials[-1].to(dt).float()
        tot = torch.zeros_like(partials[0])
        for j in perm(len(partials)):
            tot = tot + partials[j]
        acc[rows, cols] = tot
    mode = {"truncate": "truncate", "ties_away": "ties_away"}.get(fault, "rne")
    r = lambda t32: _round_to(t32.double(), dt, mode).float()
    if epi == "swiglu":
        F = Nw // 2
        g, u = r(acc[:, :F]), r(acc[:, F:])
        if fault == "swiglu_neighbour_pair":
            u = torch.roll(u, -1, 1)
        val = r(r(g / (1 + torch.exp(-g))) * u)
    elif epi == "resid":
        val = r(acc + resid.float()) if fault == "resid_early" else r(r(acc) + resid.float())
    elif epi == "none":
        val = r(acc)
    else:
        y = r(acc + bias.float())
        val = {"bias": lambda: y, "quick_gelu": lambda: r(y / (1 + torch.exp(-torch.tensor(1.702, dtype=torch.float32) * y))),
               "gelu": lambda: r(0.5 * y * (1 + torch.erf(y * torch.tensor(math.sqrt(0.5), dtype=torch.float32))))}[epi]()
    out = torch.full(val.shape, GC.SENTINEL, dtype=dt)
    out[:] = val.to(dt)
    if fault == "last_quad_unwritten":
        out[M // 2, -4:] = GC.SENTINEL
    return out, cut


def _epi_of(fault):
    return "swiglu" if fault == "swiglu_neighbour_pair" else "resid" if fault == "resid_early" else "none"


def _case(K, dt, epi, pattern):
    """operands of one emulator run: the integer census or the randn operands of the old tests"""
    Nw = 2 * F_ if epi == "swiglu" else N_
    if pattern == "census":
        x, w, _ = GC.operands(M_, Nw, K, dt, seed=K)
        bias, resid = GC.side_inputs(M_, Nw, dt, seed=K + 1)
    else:
        g = torch.Generator().manual_seed(K)
        x, w = torch.randn(M_, K, generator=g).to(dt), (torch.randn(Nw, K, generator=g) * 0.02).to(dt)
        bias, resid = torch.randn(Nw, generator=g).to(dt), torch.randn(M_, Nw, generator=g).to(dt)
    return x, w, bias, resid


def _census_rejects(fault, K, dt, seed=0):
    epi = _epi_of(fault)
    x, w, bias, resid = _case(K, dt, epi, "census")
    got, _ = emulate(x, w, dt, epi, bias, resid, seed=seed, fault=fault)
    ref = GC.reference(x, w, epi, bias, resid, dt)
    try:
        if epi == "swiglu":
            GC.assert_ulps(got, ref, 2, 0.01, f"{fault} K={K}")
        else:
            GC.assert_exact(got, ref, f"{fault} K={K}")
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", [128, 384, 1280, 2816, 13824])
def test_the_unfaulted_emulator_is_exact_for_every_shuffle(K, dt):
    for epi in ("none", "resid", "bias"):
        x, w, bias, resid = _case(K, dt, epi, "census")
        ref = GC.reference(x, w, epi, bias, resid, dt)
        for seed in range(2 if K > 2816 else 4):
            got, cut = emulate(x, w, dt, epi, bias, resid, seed=seed)
            assert cut or K == 128                                   # a stream-K cut falls inside a tile
            GC.assert_exact(got, ref, f"clean {epi} K={K} seed={seed}")
    rounded = (GC.product(x, w).to(dt).double() != GC.product(x, w)).float().mean().item()
    assert rounded > 0.01                                            # the output rounding is exercised (bf16: most entries)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", [384, 13824])
@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_is_rejected_by_the_census(fault, K, dt):
    msg = _census_rejects(fault, K, dt)
    assert msg is not None, f"{fault} slipped through the census at K = {K}"
    assert "32 x 32 blocks" in msg


def _old_errors(fault, K, dt):
    """(largest error, max|ref|) of the faulted emulator on randn operands against the fp32 reference of the old tests"""
    epi = _epi_of(fault)
    x, w, bias, resid = _case(K, dt, epi, "randn")
    got, _ = emulate(x, w, dt, epi, bias, resid, fault=fault)
    acc = x.float() @ w.float().t()
    r = lambda t: t.to(dt).float()
    if epi == "swiglu":
        g, u = r(acc[:, :F_]), r(acc[:, F_:])
        ref = r(r(g / (1 + torch.exp(-g))) * u)
    elif epi == "resid":
        ref = r(r(acc) + resid.float())
    else:
        ref = r(acc)
    return (got.float() - ref).abs().max().item(), ref.abs().max().item()


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", [384, 13824])
def test_the_old_randn_bound_accepts_what_the_census_rejects(K, dt):
    """The written reason for this file: each of OLD_BOUND_ACCEPTS passes the tightest bound of the random-input tests."""
    for fault in OLD_BOUND_ACCEPTS:
        err, top = _old_errors(fault, K, dt)
        assert err <= 2 ** -7 * top + 1e-3, (fault, err, top)
        assert _census_rejects(fault, K, dt) is not None
    err, top = _old_errors(None, K, dt)                                     # and the bound is not vacuous: the clean emulator is far inside
    assert err <= 2 ** -8 * top + 1e-3


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_activation_stand_ins_stay_inside_their_caps(dt):
    """fp32 exp / erf (what the kernels' epilogues compute with) against the fp64 reference: SwiGLU within 2 representable values,
    quick-GELU within 1, at most 1 % of entries different; GELU within 2 ulp(ref) + 2^-21 |y|."""
    for K in (384, 2816):
        x, w, bias, resid = _case(K, dt, "swiglu", "census")
        got, _ = emulate(x, w, dt, "swiglu")
        d, share = GC.assert_ulps(got, GC.reference(x, w, "swiglu", None, None, dt), 2, 0.01, "swiglu stand-in")
        assert d <= 2 and share <= 0.01
        x, w, bias, resid = _case(K, dt, "none", "census")
        got, _ = emulate(x, w, dt, "quick_gelu", bias)
        GC.assert_ulps(got, GC.reference(x, w, "quick_gelu", bias, None, dt), 1, 0.01, "quick-GELU stand-in")
        got, _ = emulate(x, w, dt, "gelu", bias)
        ref, y = GC.reference(x, w, "gelu", bias, None, dt, want_pre=True)
        GC.assert_ulps(got, ref, 2, 1.0, "GELU stand-in", slack=2.0 ** -21 * y.abs())      # (no cap on the share: the negative tail differs by design)


def test_operands_and_counting_are_what_they_say():
    for dt in DTYPES:
        for K in (128, 4096, 13824):
            x, w, s = GC.operands(5, 7, K, dt, seed=1)
            assert s == GC.scale_exp(K) and x.dtype == dt and float(x.abs().max()) <= 15
            wi = w.double() * 2.0 ** s
            assert torch.equal(wi, wi.round()) and float(wi.abs().max()) <= 15
            p = GC.product(x, w)
            assert float(p.abs().max()) * 2.0 ** s < 2 ** 24 / 5 and torch.equal(p.float().double(), p)
            assert 0.5 < float(GC.product(*GC.operands(64, 64, K, dt, seed=2)[:2]).std()) < 4
        xs, ws, _ = GC.operands(3, 4, 256, dt, seed=3, x_pad=64, w_pad=8)
        x0, w0, _ = GC.operands(3, 4, 256, dt, seed=3)
        assert xs.stride(0) == 320 and ws.stride(0) == 264 and torch.equal(xs, x0) and torch.equal(ws, w0)
        a, b = GC.counting(3, 5, 13824, dt)
        assert torch.equal(GC.reference(a, b, "none", None, None, dt), torch.full((3, 5), 13824.0, dtype=dt))
    with pytest.raises(AssertionError):
        GC.counting(1, 1, 13824 + 32, torch.bfloat16)                       # 433 * 32: nine significant bits
    with pytest.raises(AssertionError):
        GC.operands(1, 1, 2 ** 17, torch.bfloat16, seed=0)                  # K R^2 >= 2^24


def test_reference_rounds_where_the_kernels_round():
    dt = torch.bfloat16
    x, w = torch.tensor([[1.0]], dtype=dt), torch.tensor([[1.00390625 * 2]], dtype=torch.float64)
    acc = torch.tensor([[257.0 / 128]], dtype=torch.float64)                # 2.0078125: a bf16 tie between 2.0 and 2.015625 -> even: 2.0
    res = torch.tensor([[0.0078125]], dtype=dt)
    assert float(GC.reference(x, w, "none", None, None, dt, acc=acc)) == 2.0
    assert float(GC.reference(x, w, "resid", None, res, dt, acc=acc)) == 2.0            # r(r(acc) + res) = r(2.0078125) = 2.0 ...
    assert float(GC.reference(x, w, "bias", res[0], None, dt, acc=acc)) == 2.015625     # ... r(acc + b) = r(2.015625)
    assert float(GC.reference(x, w, "bias_resid", res[0], res, dt, acc=acc)) == 2.03125  # r(2.015625 + 0.0078125): tie -> even
    sl = GC.slab_reference(*GC.operands(3, 4, 512, dt, seed=4)[:2], [0, 128, 512])
    assert sl.shape == (2, 3, 4) and torch.equal(sl.sum(0).double(), GC.product(*GC.operands(3, 4, 512, dt, seed=4)[:2]))
    h = torch.arange(32, dtype=torch.float32).view(1, 32).to(dt)
    assert GC.ss_reference(h).tolist() == [[sum(i * i for i in range(16)), sum(i * i for i in range(16, 32))]]


def test_checkers_and_their_messages():
    dt = torch.bfloat16
    ref = torch.zeros(70, 76, dtype=dt)
    got = ref.clone()
    GC.assert_exact(got, ref)
    got[40, 70] = 1.0
    got[41, 3] = float("nan")
    with pytest.raises(AssertionError, match=r"2 of 5320 entries differ.*\(40, 70, 1\.0, 0\.0\).*\[\(1, 0\), \(1, 2\)\]"):
        GC.assert_exact(got, ref, "t")
    one = torch.ones(4, 8, dtype=dt)
    up1, up3 = one + 2.0 ** -7, one + 3 * 2.0 ** -7
    assert GC.assert_ulps(up1, one, 1, 1.0)[0] == 1
    with pytest.raises(AssertionError, match="largest distance 3"):
        GC.assert_ulps(up3, one, 2, 1.0)
    with pytest.raises(AssertionError, match="of entries differ"):
        GC.assert_ulps(up1, one, 1, 0.5)
    GC.assert_ulps(up3, one, 2, 1.0, slack=torch.full((4, 8), 2.0 ** -7, dtype=torch.float64))
    assert GC.assert_ulps(torch.tensor([[-(2.0 ** -133)]], dtype=dt), torch.tensor([[2.0 ** -133]], dtype=dt), 2, 1.0)[0] == 2   # across zero
    assert float(GC.ulp_of(torch.tensor(1.5), dt)) == 2.0 ** -7 and float(GC.ulp_of(torch.tensor(1.5), torch.float16)) == 2.0 ** -10
    buf, view = GC.guarded(3, 12, dt, "cpu", ldy=16, lead=4)
    assert view.shape == (3, 12) and view.stride(0) == 16 and view.storage_offset() == GC.GUARD + 4
    view.fill_(1.0)
    GC.assert_guards(buf, view)
    buf[GC.GUARD + 4 + 16 + 13] = 0.0                                       # a gap column of row 1
    with pytest.raises(AssertionError, match="1 elements outside"):
        GC.assert_guards(buf, view)
    for mode, want in (("rne", 2.0), ("truncate", 2.0), ("ties_away", 2.015625)):
        assert float(_round_to(torch.tensor(257.0 / 128, dtype=torch.float64), dt, mode)) == want
    assert float(_round_to(torch.tensor(2.0149, dtype=torch.float64), dt, "truncate")) == 2.0
    assert float(_round_to(torch.tensor(-2.0149, dtype=torch.float64), dt, "truncate")) == -2.0
    assert float(_round_to(torch.tensor(-3.0, dtype=torch.float64), dt, "ties_away")) == -3.0
