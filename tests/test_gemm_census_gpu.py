"""Exact-integer census of every dense contraction of llava_align_amd.ops (tests/gemm_census.py): the persistent stream-K MFMA GEMM
- 16 macro tiles x 3 schedules, the split-K slab mode, 5 epilogues - and the weight-streaming family (skinny_gemm in its 4-wave,
8-wave, 17 - 64-row and "wide" forms and as slabs, swiglu_linear, linear_resid_ss, linear_normed, swiglu_linear_normed and their 8-bit
twins).  Operands are small integers times a power of two, so every fp32 partial sum is exact whatever the summation order, and the
plain, bias, bias + residual, residual and slab forms must equal the fp64 reference - rounded where the kernel rounds - BIT FOR BIT, in
bf16 and fp16.  The three activation epilogues (__expf / erff) are held to a distance in representable values instead (caps below).

Which branch a shape reaches is asserted from the shape (tile counts, data-parallel rounds, the staged / unstaged epilogue, the
weight-streaming form), never read from the binary.  Every output lies in a sentinel-filled buffer with 4096 guard elements on
either side; strided outputs also check the gap columns of each row.

Caps of the activation epilogues (conditions, not measurements; derivation: the `assert_ulps` docstring of tests/gemm_census.py)
and, in brackets, the largest figures any launch of this file showed on the MI355X (printed when the module ends under `pytest -s`):
    SwiGLU       <= 2 representable values (two roundings), <= 1 % of entries differ     [MFMA GEMM: 2, 0.027 %; weight streaming: 1, 0.19 %]
    quick-GELU   <= 1 representable value,                  <= 1 % of entries differ     [1, 0.036 %]
    GELU         |got - ref| <= 2 ulp(ref) + 2^-21 |y|      (y the pre-activation: fp32 cancellation in 1 + erf for negative y; no cap on
                 the share: with y down to -15 a fifth of the entries lie in that tail and differ)     [20.5 % of entries differ; the largest |got - ref| / bound is printed with the other figures when the module ends]"""
import pytest
import torch

import gemm_census as GC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# macro tile id (1-based, as in ops.gemm_config) -> (BM, BN, WM, WN): the `switch` of vdd_gemm in csrc/vdd_gemm.hip
TILES = {1: (256, 256, 2, 4), 2: (128, 256, 2, 4), 3: (256, 128, 4, 2), 4: (192, 256, 2, 4), 5: (256, 192, 4, 2), 6: (192, 192, 2, 3),
         7: (192, 128, 2, 4), 8: (64, 256, 2, 4), 9: (128, 128, 2, 4), 10: (128, 128, 2, 2), 11: (192, 128, 2, 2), 12: (64, 128, 2, 2),
         13: (64, 128, 2, 4), 14: (32, 128, 1, 4), 15: (32, 128, 1, 2), 16: (96, 128, 1, 4)}
NO_SWIGLU = (5, 6, 7, 9, 13, 14, 16)          # the candidate skips of test_gemm_epilogues: no gate / up pair inside a wave, or 192 columns
SCHEDS = (0, 1, 2)                            # hybrid, data-parallel only, stream-K only
LAYOUT_IDS = (1, 2, 7, 8, 12, 14)             # both classes of the wave tile: 64 columns (staged epilogue possible) and 32
M_SUBSET = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64]
STATS = {}


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def dt(request):
    return request.param


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cache():
    yield
    _CACHE.clear()
    for k, v in sorted(STATS.items()):
        print(f"gemm census, largest seen: {k}: {v[0]}, share of entries that differ {v[1]:.4%}")


def ops():
    from llava_align_amd import ops as O
    return O


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def P():
    return max(8, n_cu() & ~7)


def wave_tn(tid):
    BM, BN, WM, WN = TILES[tid]
    return BN // WN


def plan(M, ncols, K, tid, sched):
    """The host-side schedule of launch_cfg, restated: tile counts and whole-tile rounds before the stream-K part."""
    BM, BN, _, _ = TILES[tid]
    Mt, Nt = -(-M // BM), -(-ncols // BN)
    T, p = Mt * Nt, P()
    full, rem = divmod(T, p)
    dp = -(-T // p) if sched == 1 else 0 if sched == 2 else (full if rem == 0 else max(full - 1, 0))
    return dict(Mt=Mt, Nt=Nt, T=T, UP=K // 128, dp_rounds=dp, sk_tiles=T - min(T, dp * p),
                GM=Mt if Mt < 8 else (4 if (Mt >= 32 and Nt >= 80) else 8))


def stage_out(out):
    return out.stride(0) % 8 == 0 and out.data_ptr() % 16 == 0


_CACHE = {}


def cached(key, make):
    """one set of operands and references per shape, shared by every candidate and test that uses the shape (a few live at a time)"""
    if key not in _CACHE:
        if len(_CACHE) >= 6:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = make()
    return _CACHE[key]


def epi_code(epi):
    O = ops()
    return {"none": O.EPI_NONE, "bias": O.EPI_BIAS, "bias_resid": O.EPI_BIAS_RESID, "swiglu": O.EPI_SWIGLU, "quick_gelu": O.EPI_BIAS_QUICK_GELU,
            "gelu": O.EPI_BIAS_GELU}[epi]


def note(name, d, share):
    old = STATS.get(name, (0, 0.0))
    STATS[name] = (max(old[0], d), max(old[1], share))


def gemm_case(M, N, K, dt, epis, seed=1, x_pad=0, w_pad=0, resid_pad=0, pattern="census"):
    """operands and the reference of each epilogue in `epis` for an [M, K] x [N, K] product (SwiGLU: its own [2 N', K] weight with
    N' = N rounded up to 128 features)"""
    def make():
        c = {}
        if pattern == "counting":
            x, w = GC.counting(M, N, K, dt, device=DEV)
        else:
            x, w, _ = GC.operands(M, N, K, dt, seed, device=DEV, x_pad=x_pad, w_pad=w_pad)
        bias, resid = GC.side_inputs(M, N, dt, seed + 1, device=DEV, resid_pad=resid_pad)
        acc = GC.product(x, w)
        c.update(x=x, w=w, bias=bias, resid=resid)
        for e in epis:
            if e == "swiglu":
                F = -(-N // 128) * 128
                _, wg, _ = GC.operands(1, 2 * F, K, dt, seed + 2, device=DEV, w_pad=w_pad)
                c["w_swiglu"], c["F"] = wg, F
                c["ref_swiglu"] = GC.reference(x, wg, "swiglu", None, None, dt)
            elif e == "gelu":
                c["ref_gelu"], c["pre_gelu"] = GC.reference(x, w, e, bias, resid, dt, acc=acc, want_pre=True)
            else:
                c["ref_" + e] = GC.reference(x, w, e, bias, resid, dt, acc=acc)
        return c
    return cached((M, N, K, dt, tuple(epis), seed, x_pad, w_pad, resid_pad, pattern), make)


def run_gemm(c, epi, config, out_spec=None, what=""):
    """one launch of vdd_gemm into a guarded, sentinel-filled output (out_spec: (ldy, lead)), checked against the case's reference"""
    O = ops()
    x = c["x"]
    w = c["w_swiglu"] if epi == "swiglu" else c["w"]
    M, N = x.shape[0], (c["F"] if epi == "swiglu" else c["w"].shape[0])
    ldy, lead = out_spec or (N, 0)
    buf, out = GC.guarded(M, N, x.dtype, DEV, ldy=ldy, lead=lead)
    bias = c["bias"] if epi in ("bias", "bias_resid", "quick_gelu", "gelu") else None
    resid = c["resid"] if epi == "bias_resid" else None
    O.gemm(x, w, bias=bias, resid=resid, epi=epi_code(epi), out=out, config=config)
    ref = c["ref_" + epi]
    if epi in GC.EXACT_EPIS:
        GC.assert_exact(out, ref, what)
    elif epi == "gelu":
        slack = 2.0 ** -21 * c["pre_gelu"].abs()
        _, share = GC.assert_ulps(out, ref, 2, 1.0, what, slack=slack)
        note("gelu (|got - ref| as a fraction of its bound)", float(((out.double() - ref.double()).abs() / (2 * GC.ulp_of(ref, ref.dtype) + slack)).max()), share)
    else:
        note(epi + " (MFMA GEMM)", *GC.assert_ulps(out, ref, 2 if epi == "swiglu" else 1, 0.01, what))
    GC.assert_guards(buf, out, what)
    return out


# ------------------------------------------------------------------------------------------------ a. MFMA GEMM: all 48 candidates

@pytest.mark.parametrize("tid", list(TILES))
def test_gemm_one_tile_row_stream_k_cuts_inside_a_tile(tid, dt):
    """M = BM - 1, N = 3 BN + 4, K = 384: one ragged row tile, four column tiles (the last of 4 columns), three K units per tile and
    more workgroups than tiles - the stream-K ranges cut inside every tile.  The premise of the census is confirmed here first: the
    matrix core adds exactly representable products without loss (all three schedules, random integers and the counting pattern)."""
    O = ops()
    BM, BN, _, _ = TILES[tid]
    M, N, K = BM - 1, 3 * BN + 4, 384
    for sched in SCHEDS:
        p = plan(M, N, K, tid, sched)
        assert p["Mt"] == 1 and p["Nt"] == 4 and p["UP"] == 3 and p["T"] < P() and N % 8 == 4
        assert (p["dp_rounds"], p["sk_tiles"]) == ((1, 0) if sched == 1 else (0, 4))
        for pattern in ("census", "counting"):
            c = gemm_case(M, N, K, dt, ("none",), pattern=pattern)
            run_gemm(c, "none", O.gemm_config(tid, sched), what=f"tile {tid} sched {sched} {pattern} {M}x{N}x{K}")


def _partial_round_shape(tid):
    BM, BN, _, _ = TILES[tid]
    Nt = -(-(P() + 37) // 5)
    return 4 * BM + 1, (Nt - 1) * BN + 12, 256


@pytest.mark.parametrize("tid", list(TILES))
def test_gemm_partial_last_round_every_epilogue(tid, dt):
    """Five row tiles, the last of ONE row, N = 4 (mod 8), at least P + 37 and fewer than 2 P tiles: the data-parallel schedule ends in
    a partial round, the hybrid and stream-K schedules cut 128-deep units of ~300 tiles over P workgroups.  Every candidate: plain,
    bias and bias + residual epilogues bit for bit; quick-GELU, GELU and (where the tile pairs gate / up) SwiGLU inside their caps."""
    O = ops()
    BM, BN, _, _ = TILES[tid]
    M, N, K = _partial_round_shape(tid)
    epis = ("none", "bias", "bias_resid", "quick_gelu", "gelu") + (() if tid in NO_SWIGLU else ("swiglu",))
    c = gemm_case(M, N, K, dt, ("none", "bias", "bias_resid", "quick_gelu", "gelu", "swiglu"))
    for sched in SCHEDS:
        p = plan(M, N, K, tid, sched)
        assert p["Mt"] == 5 and M % BM == 1 and N % 8 == 4 and P() + 37 <= p["T"] < 2 * P()
        assert p["dp_rounds"] == (2 if sched == 1 else 0) and (sched != 1 or p["T"] % P() != 0)
        for epi in epis:
            run_gemm(c, epi, O.gemm_config(tid, sched), what=f"tile {tid} sched {sched} {epi} {M}x{N}x{K}")


@pytest.mark.parametrize("tid", list(TILES))
def test_gemm_hybrid_data_parallel_rounds_then_stream_k(tid, dt):
    """At least 2 P + 37 tiles (five row tiles, the last of one row, N = 4 (mod 8), K = 256): the hybrid schedule runs a whole-tile
    round and then stream-K over the remaining P + 38 .. tiles.  Tiles 1 and 14 also at 34 x 86 tiles - groups of FOUR row tiles, the
    last group ragged: 1058 x 11008 for the 32 x 128 tile; for the 256 x 256 tile 8500 rows of a plain product 21772 wide and of the
    SwiGLU product of 11008 features (the 8500 x 11008 x 256 shape of test_gemm_epilogues).  Every tile id runs at these shapes - none
    only at the smaller ones."""
    O = ops()
    BM, BN, _, _ = TILES[tid]
    Nt = -(-(2 * P() + 37) // 5)
    shapes = [(4 * BM + 1, (Nt - 1) * BN + 12, 256, "none")]
    if tid == 14:
        shapes.append((1058, 11008, 256, "none"))
    if tid == 1:
        shapes += [(8500, 85 * 256 + 12, 256, "none"), (8500, 11008, 256, "swiglu")]
    for M, N, K, epi in shapes:
        c = gemm_case(M, N, K, dt, (epi,))
        for sched in SCHEDS:
            p = plan(M, 2 * N if epi == "swiglu" else N, K, tid, sched)
            assert p["T"] >= 2 * P() + 37
            if sched == 0:
                assert p["dp_rounds"] >= 1 and p["sk_tiles"] >= P()            # whole-tile rounds AND a stream-K remainder
            if len(shapes) > 1 and (M, N, K, epi) != shapes[0]:
                assert (p["Mt"], p["Nt"], p["GM"]) == (34, 86, 4) and p["Mt"] % 4 != 0 and M % BM != 0
            else:
                assert p["Mt"] == 5 and M % BM == 1 and N % 8 == 4
            run_gemm(c, epi, O.gemm_config(tid, sched), what=f"tile {tid} sched {sched} {epi} {M}x{N}x{K}")


@pytest.mark.parametrize("tid", list(TILES))
def test_gemm_k_pipeline(tid, dt):
    """K = 128, 256, 1152, 11008 (1, 2, 9, 86 units of 128) at 96 x 512: fewer K tiles than the 5 - 8 LDS buffers of the streaming tiles,
    exactly as many, and a long pipeline; every schedule."""
    O = ops()
    for K in (128, 256, 1152, 11008):
        c = gemm_case(96, 512, K, dt, ("none",), seed=3)
        for sched in SCHEDS:
            assert plan(96, 512, K, tid, sched)["UP"] == K // 128
            run_gemm(c, "none", O.gemm_config(tid, sched), what=f"tile {tid} sched {sched} 96x512x{K}")
    c = gemm_case(96, 512, 11008, dt, ("none",), pattern="counting")
    run_gemm(c, "none", O.gemm_config(tid, 0), what=f"tile {tid} counting 96x512x11008")


def test_gemm_tuned_choice_and_batch_invariant_mode(dt):
    """config=None (whatever the tuner measured or has on file) and the one-form batch-invariant mode give the same bits."""
    O = ops()
    for M, N, K in ((96, 512, 1152), (255, 772, 384), _partial_round_shape(8)):
        c = gemm_case(M, N, K, dt, ("none", "bias", "bias_resid", "quick_gelu", "gelu", "swiglu") if K == 256 else ("none",), seed=1 if K != 1152 else 3)
        run_gemm(c, "none", None, what=f"tuned {M}x{N}x{K}")
        with O.batch_invariant():
            run_gemm(c, "none", None, what=f"batch-invariant {M}x{N}x{K}")
            if K == 256:
                run_gemm(c, "bias_resid", None, what=f"batch-invariant bias+resid {M}x{N}x{K}")


# ------------------------------------------------------------------------------------------------ b. layouts that never ran before

@pytest.mark.parametrize("tid", LAYOUT_IDS)
def test_gemm_output_and_operand_layouts(tid, dt):
    """Two row tiles (the second of one row), K = 256, each epilogue, hybrid and data-parallel schedules:
      unstaged_ldy     N = 4 (mod 8), a contiguous output: ldy % 8 = 4, so the epilogue stores 8-byte quads from the accumulator layout
      staged_half      N = 4 (mod 8) into a 16-byte aligned view with ldy % 8 == 0: whole rows leave through LDS (64-column wave tiles),
                       the last four columns of a row as a half chunk
      unstaged_align   N = 0 (mod 8) into a view that starts 4 elements into an aligned buffer: unstaged by alignment alone
      strided          w a row slice of [N, K + 64], resid a column slice of a wider buffer, x a column slice (staged where possible)
    SwiGLU (F = 256 features): out a view with ldy = F + 4 (unstaged), F + 8 (staged) and F + 8 from 4 elements in (unstaged)."""
    O = ops()
    BM, BN, _, _ = TILES[tid]
    M, K = BM + 1, 256
    can_stage = wave_tn(tid) % 64 == 0
    seen = set()
    plain = ("none", "bias", "bias_resid", "quick_gelu", "gelu")
    for name, N, ldy_extra, lead, pads in (("unstaged_ldy", 2 * BN + 4, 0, 0, (0, 0, 0)), ("staged_half", 2 * BN + 4, 4, 0, (0, 0, 0)),
                                           ("unstaged_align", 2 * BN + 8, 8, 4, (0, 0, 0)), ("strided", 2 * BN + 8, 16, 0, (64, 64, 8))):
        c = gemm_case(M, N, K, dt, plain, seed=5, x_pad=pads[0], w_pad=pads[1], resid_pad=pads[2])
        if name == "strided":
            assert c["x"].stride(0) == K + 64 and c["w"].stride(0) == K + 64 and c["resid"].stride(0) == N + 8
        for sched in (0, 1):
            for epi in plain:
                out = run_gemm(c, epi, O.gemm_config(tid, sched), out_spec=(N + ldy_extra, lead), what=f"tile {tid} sched {sched} {name} {epi}")
                assert stage_out(out) == (name in ("staged_half", "strided"))
                seen.add(("staged" if (can_stage and stage_out(out)) else "unstaged", "half" if N % 8 == 4 else "whole"))
    assert plan(M, 2 * BN + 4, K, tid, 0)["Mt"] == 2
    assert seen == ({("staged", "half"), ("staged", "whole"), ("unstaged", "half"), ("unstaged", "whole")} if can_stage
                    else {("unstaged", "half"), ("unstaged", "whole")})
    if tid in NO_SWIGLU:
        return
    F = 256
    c = gemm_case(M, F, K, dt, ("swiglu",), seed=6, w_pad=64)
    assert c["F"] == F and wave_tn(tid) == 64
    seen = set()
    for ldy, lead in ((F + 4, 0), (F + 8, 0), (F + 8, 4)):
        for sched in (0, 1):
            out = run_gemm(c, "swiglu", O.gemm_config(tid, sched), out_spec=(ldy, lead), what=f"tile {tid} sched {sched} swiglu ldy {ldy} lead {lead}")
            seen.add(stage_out(out))
    assert seen == {True, False}


def test_gemm_refuses_layouts_out_of_contract_before_any_launch(dt):
    """ldy, ldr % 4, ldx, ldw % 8 and N % 4 are the contract of vdd_gemm: anything else is VDD_ERR_INVALID_ARG at the entry."""
    O = ops()
    c = gemm_case(33, 136, 256, dt, ("none",), seed=7)
    x, w = c["x"], c["w"]
    for kw in (dict(out=GC.guarded(33, 136, dt, DEV, ldy=138)[1]), dict(x=GC._strided(x, 4)), dict(w=GC._strided(w, 4)),
               dict(resid=GC._strided(c["resid"], 2), bias=c["bias"], epi=O.EPI_BIAS_RESID)):
        args = dict(x=x, w=w, config=O.gemm_config(12, 0))
        args.update(kw)
        with pytest.raises(ValueError, match="invalid argument"):
            O.gemm(args.pop("x"), args.pop("w"), **args)


# ------------------------------------------------------------------------------------------------ c. the weight-streaming family

def skinny_form(M, N, K, slabs=False):
    """the kernel vdd_skinny_gemm launches (its dispatch in csrc/vdd_llm_kernels.hip), from the shape"""
    blocks = -(-N // 16)
    if M > 16 and not slabs and K % 256 == 0 and N > 8192:
        return "wide"
    if M <= 16 and not slabs and N <= 8192 and K % 256 == 0 and (blocks <= n_cu() or blocks % n_cu() == 0):
        return "8-wave"
    return "4-wave" if M <= 16 else "4-wave x2" if M <= 32 else "4-wave x4"


def skinny_ks(M):
    return ([128, 384] if M <= 16 else []) + [256, 512, 1280, 2816, 4096]


def skinny_case(N, K, dt):
    """64 rows of x (contiguous and as a column slice), w [N, K], resid, and the references of all 64 rows: a launch of M rows must
    return the first M of them"""
    def make():
        x, w, _ = GC.operands(64, N, K, dt, seed=11, device=DEV)
        _, resid = GC.side_inputs(64, N, dt, seed=12, device=DEV)
        acc = GC.product(x, w)
        return dict(x=x, xs=GC._strided(x, 64), w=w, resid=resid, acc=acc, none=GC.reference(x, w, "none", None, None, dt, acc=acc),
                    resid_ref=GC.reference(x, w, "resid", None, resid, dt, acc=acc))
    return cached(("skinny", N, K, dt), make)


@pytest.mark.parametrize("N", [37, 1000, 1001, 4096, 8208])
def test_skinny_gemm_every_row_count(N, dt):
    """EVERY M from 1 to 64 at every N (the full sweep is well under a second per N), K = 128, 384 (up to 16 rows), 256, 512, 1280, 2816,
    4096 (1280 / 8 and 2816 / 8: ragged last batches of the 8-wave kernels, 2816 / 4 of the 4-wave ones): plain, with a residual into a
    strided output from a strided x, and (rows of M_SUBSET) a strided output alone and a residual alone; as split-K slabs (n_split 2 and
    4, every M) every slab equals the product of its own K part exactly and so does their sum.  Counting pattern: 16, 24 and 64 rows and
    the slab mode.  N = 37, 1001: odd; 1000, 8208: no multiple of 32."""
    O = ops()
    forms = set()
    for K in (128, 384, 256, 512, 1280, 2816, 4096):
        c = skinny_case(N, K, dt)
        slabs = {ns: GC.slab_reference(c["x"], c["w"], [i * K // ns for i in range(ns + 1)]) for ns in (2, 4) if K % (128 * ns) == 0}
        for M in range(1, 17 if K % 256 else 65):
            assert K in skinny_ks(M)
            forms.add(skinny_form(M, N, K))
            what = f"skinny_gemm {M}x{N}x{K} ({skinny_form(M, N, K)})"
            buf, out = GC.guarded(M, N, dt, DEV)
            O.skinny_gemm(c["x"][:M], c["w"], out=out)
            GC.assert_exact(out, c["none"][:M], what)
            GC.assert_guards(buf, out, what)
            buf, out = GC.guarded(M, N, dt, DEV, ldy=N + 3, lead=1)
            O.skinny_gemm(c["xs"][:M], c["w"], resid=c["resid"][:M], out=out)
            GC.assert_exact(out, c["resid_ref"][:M], what + " + resid, strided x and out")
            GC.assert_guards(buf, out, what + " + resid, strided x and out")
            if M in M_SUBSET:                                          # the two options on their own
                buf, out = GC.guarded(M, N, dt, DEV, ldy=N + 5, lead=3)
                O.skinny_gemm(c["x"][:M], c["w"], out=out)
                GC.assert_exact(out, c["none"][:M], what + ", strided out")
                GC.assert_guards(buf, out, what + ", strided out")
                buf, out = GC.guarded(M, N, dt, DEV)
                O.skinny_gemm(c["x"][:M], c["w"], resid=c["resid"][:M], out=out)
                GC.assert_exact(out, c["resid_ref"][:M], what + " + resid")
                GC.assert_guards(buf, out, what + " + resid")
            for ns in slabs:
                sl = O.skinny_gemm(c["x"][:M], c["w"], n_split=ns, slabs=True)
                GC.assert_exact(sl.view(ns * M, N), slabs[ns][:, :M].reshape(ns * M, N), what + f" slabs {ns}")
                assert torch.equal(sl.sum(0).double(), c["acc"][:M]), what + f" slab sum {ns}"
    want = {"4-wave", "wide"} if N > 8192 else {"4-wave", "4-wave x2", "4-wave x4", "8-wave"}
    assert forms == want, (forms, want)                               # odd / ragged N reached the 4-wave, 8-wave and wide kernels
    x1, w1 = GC.counting(64, N, 2816, dt, device=DEV)
    for M in (16, 24, 64):
        GC.assert_exact(O.skinny_gemm(x1[:M], w1), torch.full((M, N), 2816.0, dtype=dt, device=DEV), f"skinny_gemm counting {M}x{N}x2816")
    x1, w1 = GC.counting(64, N, 4096, dt, device=DEV)
    for M, ns in ((16, 2), (24, 4), (64, 2)):
        GC.assert_exact(O.skinny_gemm(x1[:M], w1, n_split=ns, slabs=True).view(ns * M, N),
                        torch.full((ns * M, N), 4096.0 / ns, device=DEV), f"skinny_gemm slabs counting {M}x{N}x4096 / {ns}")


@pytest.mark.parametrize("F", [516, 520, 1000, 4104])
def test_swiglu_linear_weight_streaming_form(F, dt):
    """The fused gate / up weight-streaming kernels (8 features per block up to 16 rows, 16 features from 17): F % 8 != 0 and
    F % 16 != 0, rows of M_SUBSET, the depths of skinny_gemm; SwiGLU cap: 2 representable values, 1 % of entries."""
    O = ops()
    O.FORCE_FORM["swiglu"] = "skinny"
    try:
        for K in (128, 384, 256, 512, 1280, 2816, 4096):
            x, w, _ = GC.operands(64, 2 * F, K, dt, seed=13, device=DEV)
            ref = GC.reference(x, w, "swiglu", None, None, dt)
            for M in [m for m in M_SUBSET if m <= 16 or K % 256 == 0]:
                buf, out = GC.guarded(M, F, dt, DEV)
                O.swiglu_linear(GC._strided(x, 64)[:M] if M % 2 else x[:M], w, out=out)
                note("swiglu (weight streaming)", *GC.assert_ulps(out, ref[:M], 2, 0.01, f"swiglu_linear {M}x{F}x{K}"))
                GC.assert_guards(buf, out, f"swiglu_linear {M}x{F}x{K}")
    finally:
        O.FORCE_FORM.pop("swiglu")


@pytest.mark.parametrize("N", [256, 4096, 5120])
def test_linear_resid_ss(N, dt):
    """h = r(r(x w^T) + resid) bit for bit (also into a strided output, and from 8-bit codes of the same weight); ss[m, j] is the fp32
    sum of the squares of 16 exactly known values - only the order of 16 fp32 additions is free: rtol 2^-22."""
    O = ops()
    for K in (128, 384, 256, 512, 1280, 2816, 4096):
        c = skinny_case(N, K, dt)
        codes, scale, w16 = O.quantize_w8(c["w"])
        assert torch.equal(w16, c["w"])                                # |int| <= 15 times a power of two: e4m3 codes reproduce w
        for M in range(1, 17):
            what = f"linear_resid_ss {M}x{N}x{K}"
            ss_ref = GC.ss_reference(c["resid_ref"][:M])
            for w8 in (None, (codes, scale)):
                buf, out = GC.guarded(M, N, dt, DEV, ldy=N + (8 if M % 2 else 0))
                n0 = O.w8_launches()
                h, ss = O.linear_resid_ss(c["xs"][:M] if M % 3 == 0 else c["x"][:M], c["w"], c["resid"][:M], out=out, w8=w8)
                assert O.w8_launches() - n0 == (1 if (w8 is not None and K % 256 == 0) else 0)
                GC.assert_exact(h, c["resid_ref"][:M], what + (" w8" if w8 else ""))
                GC.assert_guards(buf, out, what)
                assert ss.shape == (M, N // 16) and bool(((ss.double() - ss_ref).abs() <= 2.0 ** -22 * ss_ref).all()), what


@pytest.mark.parametrize("K", [256, 1280, 4096, 5120, 8192])
def test_linear_normed_and_swiglu_linear_normed(K, dt):
    """Normalise-on-load made exact by construction: ss partials of K / (4 nss) each (mean square 0.25, eps 0: rstd = 2 to an ulp),
    integer h (|h| <= 7) and ln_w in {0.5, 1, 2}: r(r(h rstd) ln_w) = 2 h ln_w exactly even if rstd is an ulp off.  The projection is
    then an integer GEMM: equality for linear_normed (with and without bias), the SwiGLU cap for swiglu_linear_normed; the same from
    8-bit codes.  Rows: 1, 2, 3, 4, 5, 8, 9, 14, 16 up to what the LDS image of the normalised rows holds (ops.norm_fused_rows: 16 rows up to
    K = 4096, 14 at K = 5120 - so 16 is left out there - and 8 at K = 8192, the cap on K - so 9, 14 and 16 are left out); the largest row
    count of each K is in the list, so the LDS boundary itself runs."""
    O = ops()
    g = torch.Generator(device=DEV).manual_seed(K)
    h = torch.randint(-7, 8, (16, K), generator=g, device=DEV, dtype=torch.int32).to(dt)
    ln = torch.tensor([0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 3, (K,), generator=g, device=DEV)].to(dt)
    xn = (2 * h.double() * ln.double()).to(dt)
    assert torch.equal(xn.double(), 2 * h.double() * ln.double()) and K * 28 * 15 < 2 ** 24
    nss = K // 16
    ss = torch.full((16, nss), K / (4.0 * nss), dtype=torch.float32, device=DEV)
    hs = GC._strided(h, 64)
    for N, F in ((1000, 516), (4096, 1000)):
        _, w, _ = GC.operands(1, N, K, dt, seed=14, device=DEV)
        _, wg, _ = GC.operands(1, 2 * F, K, dt, seed=15, device=DEV)
        bias, _ = GC.side_inputs(1, N, dt, seed=16, device=DEV)
        ref = GC.reference(xn, w, "none", None, None, dt)
        ref_b = GC.reference(xn, w, "resid", None, bias[None].expand(16, N), dt)            # bias_act behind the projection: r(r(acc) + b)
        ref_g = GC.reference(xn, wg, "swiglu", None, None, dt)
        q, qg = O.quantize_w8(w), O.quantize_w8(wg)
        assert torch.equal(q[2], w) and torch.equal(qg[2], wg)
        rows = [m for m in (1, 2, 3, 4, 5, 8, 9, 14, 16) if m <= O.norm_fused_rows(K)]
        assert rows[-1] == O.norm_fused_rows(K) == {5120: 14, 8192: 8}.get(K, 16)
        for M in rows:
            hm = hs[:M] if M % 2 else h[:M]
            for w8, w8g in ((None, None), (q[:2], qg[:2])):
                what = f"{M}x{N}x{K}" + (" w8" if w8 else "")
                n0 = O.w8_launches()
                buf, out = GC.guarded(M, N, dt, DEV, ldy=N + 2)
                O.linear_normed(hm, ss[:M], ln, 0.0, w, out=out, w8=w8)
                GC.assert_exact(out, ref[:M], "linear_normed " + what)
                GC.assert_guards(buf, out, "linear_normed " + what)
                GC.assert_exact(O.linear_normed(hm, ss[:M], ln, 0.0, w, bias=bias, w8=w8), ref_b[:M], "linear_normed + bias " + what)
                buf, out = GC.guarded(M, F, dt, DEV)
                O.swiglu_linear_normed(hm, ss[:M], ln, 0.0, wg, out=out, w8=w8g)
                note("swiglu (weight streaming)", *GC.assert_ulps(out, ref_g[:M], 2, 0.01, "swiglu_linear_normed " + what))
                GC.assert_guards(buf, out, "swiglu_linear_normed " + what)
                assert O.w8_launches() - n0 == (3 if w8 else 0)


def test_counting_pattern_in_the_fused_weight_streaming_forms(dt):
    """All-ones operands through swiglu_linear (up to 16 rows, and 17 - 64), linear_resid_ss, linear_normed and swiglu_linear_normed: an
    output that summed fewer or more than K terms reads as such.  The SwiGLU forms keep gate = up = 128 (K = 128 of ones, or K = 256 of
    halves / quarters), so silu(128) 128 = 16384 is an fp16 value."""
    O = ops()
    F, N = 520, 1000
    O.FORCE_FORM["swiglu"] = "skinny"
    try:
        for M, K, wv in ((16, 128, 1.0), (24, 256, 0.5), (64, 256, 0.5)):
            x1, w1 = GC.counting(M, 2 * F, K, dt, device=DEV)
            w1 = w1 * wv
            ref = GC.reference(x1, w1, "swiglu", None, None, dt)
            assert bool((ref == 16384).all())
            GC.assert_ulps(O.swiglu_linear(x1, w1), ref, 2, 0.01, f"swiglu_linear counting {M}x{F}x{K}")
    finally:
        O.FORCE_FORM.pop("swiglu")
    for K in (384, 2816):                                                       # the 4-wave and the 8-wave form
        x1, w1 = GC.counting(16, N, K, dt, device=DEV)
        _, resid = GC.side_inputs(16, N, dt, seed=21, device=DEV)
        h, ss = O.linear_resid_ss(x1, w1, resid)
        GC.assert_exact(h, (K + resid.double()).to(dt), f"linear_resid_ss counting 16x{N}x{K}")
    for M, K in ((8, 256), (16, 4096), (8, 8192)):
        nss = K // 16
        h1, ln1 = torch.ones(M, K, dtype=dt, device=DEV), torch.ones(K, dtype=dt, device=DEV)
        ss = torch.full((M, nss), K / (4.0 * nss), dtype=torch.float32, device=DEV)              # rstd = 2: the normalised operand is 2
        GC.assert_exact(O.linear_normed(h1, ss, ln1, 0.0, torch.ones(N, K, dtype=dt, device=DEV)), torch.full((M, N), 2.0 * K, dtype=dt, device=DEV),
                        f"linear_normed counting {M}x{N}x{K}")
        wq = torch.full((2 * F, K), 64.0 / K, dtype=dt, device=DEV)                               # gate = up = 2 K (64 / K) = 128
        ref = GC.reference(2 * h1, wq, "swiglu", None, None, dt)
        assert bool((ref == 16384).all())
        GC.assert_ulps(O.swiglu_linear_normed(h1, ss, ln1, 0.0, wq), ref, 2, 0.01, f"swiglu_linear_normed counting {M}x{F}x{K}")


# ------------------------------------------------------------------------------------------------ d. the dispatching entries

@pytest.mark.parametrize("M,N,K", [(12, 4096, 4096), (40, 5120, 5120), (64, 4096, 2816), (200, 4096, 1024)])
def test_every_eligible_form_of_linear_gives_the_same_bits(M, N, K, dt):
    """ops.linear (weight streaming | MFMA GEMM) and ops.linear_to_norm (+ split-K slabs, compared behind the RMSNorm that adds them:
    resid_out = r(resid + r(product))): every form on request through FORCE_FORM, each equal to the exact reference - hence to each other."""
    O = ops()
    x, w, _ = GC.operands(M, N, K, dt, seed=17, device=DEV)
    bias, res = GC.side_inputs(M, N, dt, seed=18, device=DEV)
    ref = GC.reference(x, w, "none", None, None, dt)
    ref_bias_gemm = GC.reference(x, w, "bias", bias, None, dt)
    ref_bias_skinny = GC.reference(x, w, "resid", None, bias[None].expand(M, N), dt)
    ref_res = GC.reference(x, w, "resid", None, res, dt)
    lnw = torch.ones(N, dtype=dt, device=DEV)
    forms = ["gemm"] + (["skinny"] if O._skinny_serves(M, K) else [])
    assert ("skinny" in forms) == (M <= 64)
    for form in forms:
        O.FORCE_FORM["linear"] = form
        try:
            GC.assert_exact(O.linear(x, w), ref, f"linear as {form} {M}x{N}x{K}")
            GC.assert_exact(O.linear(x, w, bias=bias), ref_bias_gemm if form == "gemm" else ref_bias_skinny, f"linear + bias as {form} {M}x{N}x{K}")
        finally:
            O.FORCE_FORM.pop("linear")
    s_ = O.slab_splits(M, N, K) if (M <= 256 and N <= 8192 and K % 256 == 0) else 0
    assert s_ >= 4                                                       # all four shapes have the slab form
    for form in forms + ["slabs"]:
        O.FORCE_FORM["to_norm"] = form
        try:
            o_ = O.linear_to_norm(x, w)
        finally:
            O.FORCE_FORM.pop("to_norm")
        assert (o_.dim() == 3) == (form == "slabs")
        ro = torch.full_like(res, GC.SENTINEL)
        O.rmsnorm(res, lnw, 1e-5, delta=o_, resid_out=ro)
        GC.assert_exact(ro, ref_res, f"linear_to_norm as {form} {M}x{N}x{K} behind rmsnorm")


@pytest.mark.parametrize("N", [260, 4096])
def test_gemm_slabs_are_the_exact_k_parts(N, dt):
    """Schedule 3 (64 x 256 tiles, one (tile, K part) per workgroup, no fix-up): S = 1, 2, 5, K / 128 parts at K = 1024 and 2816; every slab
    is the exact product over its own K units (part p: units p UP / S .. (p + 1) UP / S) and the slabs sum to the exact product."""
    O = ops()
    for K in (1024, 2816):
        x, w, _ = GC.operands(200, N, K, dt, seed=19, device=DEV)
        UP = K // 128
        for M in (1, 63, 64, 65, 200):
            for S in (1, 2, 5, UP):
                what = f"gemm_slabs {M}x{N}x{K} S={S}"
                buf = torch.full((2 * GC.GUARD + S * M * N,), GC.SENTINEL, dtype=torch.float32, device=DEV)
                out = buf[GC.GUARD: GC.GUARD + S * M * N].view(S, M, N)
                sl = O.gemm_slabs(x[:M], w, S, out=out)
                want = GC.slab_reference(x[:M], w, [p * UP // S * 128 for p in range(S + 1)])
                GC.assert_exact(sl.view(S * M, N), want.view(S * M, N), what)
                assert torch.equal(sl.sum(0).double(), GC.product(x[:M], w)), what
                assert bool((buf[: GC.GUARD] == GC.SENTINEL).all()) and bool((buf[GC.GUARD + S * M * N:] == GC.SENTINEL).all()), what
    x1, w1 = GC.counting(65, N, 1024, dt, device=DEV)
    GC.assert_exact(O.gemm_slabs(x1, w1, 5).view(5 * 65, N), torch.tensor([128.0, 256, 128, 256, 256], device=DEV).repeat_interleave(65)[:, None].expand(5 * 65, N).contiguous(), "gemm_slabs counting")
