"""vdd_gemm_w8 - the MFMA GEMM's W-stream tiles reading e4m3 codes - against its 16-bit twin, vdd_gemm with the same config on the
dequantised weight w16: BIT IDENTITY (the codes widen exactly to the twin's MFMA fragments, schedule, work list, fix-up and epilogue are
the twin's code, and the power-of-two row scale commutes with every fp32 addition), so there is no tolerance to choose.  Weights as in
tests/test_w8_kernels_gpu.py: a row of all 254 finite codes, a zero row, rows 64 x and 1 / 64 x their neighbours' scale - a wrong row's
scale changes bits.  x = randn * 0.5 with a padded row stride.

Shapes are the smallest that reach each branch of the schedule, asserted from the shape with `plan()` of tests/test_gemm_census_gpu.py:
    one_row_tile     M = BM - 1, N = 3 BN + 4, K = 384: a ragged row tile, a last column tile of 4 columns, stream-K cuts inside every tile
    partial_round    `_partial_round_shape` (K = 256): the data-parallel schedule ends in a partial round
    rounds_then_sk   at least 2 P + 37 tiles: the hybrid schedule runs whole-tile rounds, then a stream-K remainder
A twin comparison cannot see a fault both kernels share, so the exact-integer census of tests/gemm_census.py runs on the 8-bit GEMM too
(its operands quantise without loss - asserted here): plain, bias and slabs against the fp64 reference, K-tile counts below, at and far
above the number of LDS buffers of the 8-bit form."""
import pytest
import torch

import gemm_census as GC
from test_gemm_census_gpu import NO_SWIGLU, P, SCHEDS, TILES, _partial_round_shape, plan, stage_out, wave_tn
from test_w8_kernels_gpu import _bits, _rows, _weight

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SERVED = (7, 8, 9, 10, 11, 12, 13, 14, 15, 16)        # the tile ids with three or more K-tile buffers (ops.W8_GEMM_TILES)


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def dt(request):
    return request.param


def ops():
    from llava_align_amd import ops as O
    return O


def _rounds_then_sk_shape(tid):
    BM, BN, _, _ = TILES[tid]
    Nt = -(-(2 * P() + 37) // 5)
    return 4 * BM + 1, (Nt - 1) * BN + 12, 256


def _bias(N, dtype):
    return (torch.randn(N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(N)) * 0.5).to(dtype)


def _twin(x, w16, q, epi, cfg, N, bias=None, ldy_extra=0, what=""):
    """one launch on codes and one on w16 into guarded sentinel buffers: the same bits, one 8-bit launch counted, guards intact"""
    O = ops()
    M = x.shape[0]
    outs = []
    for w8 in (q, None):
        buf, out = GC.guarded(M, N, x.dtype, DEV, ldy=N + ldy_extra)
        n0 = O.w8_launches()
        O.gemm(x, w16, bias=bias, epi=epi, out=out, config=cfg, w8=w8)
        assert O.w8_launches() == n0 + (1 if w8 is not None else 0), what
        GC.assert_guards(buf, out, what)
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), what
    return outs[0]


def test_served_tiles_are_the_w_stream_tiles():
    assert tuple(ops().W8_GEMM_TILES) == SERVED and ops().W8_GEMM_MAX_M == 256


@pytest.mark.parametrize("tid", SERVED)
def test_w8_gemm_is_the_16bit_gemm_on_w16(tid, dt):
    O = ops()
    BM, BN, _, _ = TILES[tid]
    classes = (("one_row_tile", (BM - 1, 3 * BN + 4, 384)), ("partial_round", _partial_round_shape(tid)), ("rounds_then_sk", _rounds_then_sk_shape(tid)))
    seen = set()
    for ci, (name, (M, N, K)) in enumerate(classes):
        w16, codes, scale = _weight(N, K, dt)
        assert len(set(scale.tolist())) >= 3                      # rows with different scales: a neighbour's scale would show
        x = _rows(M, K, dt, 17 * M + K)
        assert x.stride(0) == K + 64
        bias = _bias(N, dt)
        F = -(-N // 128) * 128
        swiglu = tid not in NO_SWIGLU and ci < 2
        if swiglu:
            wg16, gcodes, gscale = _weight(2 * F, K, dt)
        for sched in SCHEDS:
            p = plan(M, N, K, tid, sched)
            if name == "one_row_tile":
                assert p["Mt"] == 1 and p["Nt"] == 4 and p["UP"] == 3 and p["T"] < P() and N % 8 == 4
                assert (p["dp_rounds"], p["sk_tiles"]) == ((1, 0) if sched == 1 else (0, 4))
            elif name == "partial_round":
                assert p["Mt"] == 5 and M % BM == 1 and N % 8 == 4 and P() + 37 <= p["T"] < 2 * P()
                assert p["dp_rounds"] == (2 if sched == 1 else 0) and (sched != 1 or p["T"] % P() != 0)
            else:
                assert p["T"] >= 2 * P() + 37 and p["Mt"] == 5
                if sched == 0:
                    assert p["dp_rounds"] >= 1 and p["sk_tiles"] >= P()
            cfg = O.gemm_config(tid, sched)
            what = f"tile {tid} sched {sched} {name} {M}x{N}x{K}"
            # N = 4 (mod 8): a contiguous output is unstaged (8-byte quads from the accumulators), ldy = N + 4 is staged (rows through LDS)
            for ldy_extra in (0, 4):
                out = _twin(x, w16, (codes, scale), O.EPI_NONE, cfg, N, ldy_extra=ldy_extra, what=what + f" none ldy+{ldy_extra}")
                assert stage_out(out) == (ldy_extra == 4)
                seen.add("staged" if (stage_out(out) and wave_tn(tid) % 64 == 0) else "unstaged")
            if ci < 2:
                _twin(x, w16, (codes, scale), O.EPI_BIAS, cfg, N, bias=bias, ldy_extra=4 * (sched & 1), what=what + " bias")
            if swiglu:
                _twin(x, wg16, (gcodes, gscale), O.EPI_SWIGLU, cfg, F, ldy_extra=8 * (sched & 1) + 4 * (sched >> 1), what=what + " swiglu")
    assert seen == ({"staged", "unstaged"} if wave_tn(tid) % 64 == 0 else {"unstaged"})


@pytest.mark.parametrize("M", [17, 64])
def test_w8_slabs_are_the_16bit_slabs_on_w16(M, dt):
    O = ops()
    N, K = 4096 + 4, 4096
    w16, codes, scale = _weight(N, K, dt)
    x = _rows(M, K, dt, 3 * M)
    S = O.slab_splits(M, N, K)
    assert S >= 4
    for s_ in (S, 3):
        n0 = O.w8_launches()
        a = O.gemm_slabs(x, w16, s_, w8=(codes, scale))
        assert O.w8_launches() == n0 + 1
        b = O.gemm_slabs(x, w16, s_)
        assert O.w8_launches() == n0 + 1
        assert a.dtype == torch.float32 and torch.equal(_bits(a), _bits(b)), (M, s_)


def _census_operands(M, N, K, dtype, pattern):
    O = ops()
    if pattern == "counting":
        x, w = GC.counting(M, N, K, dtype, device=DEV)
    else:
        x, w, _ = GC.operands(M, N, K, dtype, seed=1, device=DEV)
    codes, scale, w16 = O.quantize_w8(w)
    # the premise: the census weights (integers up to 15 times a power of two) are e4m3 values times a power of two - quantising loses nothing
    assert torch.equal(w16, w), (M, N, K, pattern)
    return x, w, (codes, scale)


@pytest.mark.parametrize("tid", SERVED)
def test_w8_gemm_census_plain_and_bias(tid, dt):
    """M = BM - 1, N = 3 BN + 4, K = 384 under every schedule, random integers and the counting pattern; then 96 x 512 at K = 128, 256, 1152
    and 11008: 2, 4, 18 and 172 K-tiles against the 3 - 8 LDS buffers of the 8-bit form."""
    O = ops()
    BM, BN, _, _ = TILES[tid]
    M, N, K = BM - 1, 3 * BN + 4, 384
    for pattern in ("census", "counting"):
        x, w, q = _census_operands(M, N, K, dt, pattern)
        bias, _ = GC.side_inputs(M, N, dt, 2, device=DEV)
        acc = GC.product(x, w)
        for sched in SCHEDS:
            for epi, code, b in (("none", O.EPI_NONE, None), ("bias", O.EPI_BIAS, bias)):
                what = f"w8 tile {tid} sched {sched} {pattern} {epi} {M}x{N}x{K}"
                buf, out = GC.guarded(M, N, dt, DEV)
                n0 = O.w8_launches()
                O.gemm(x, w, bias=b, epi=code, out=out, config=O.gemm_config(tid, sched), w8=q)
                assert O.w8_launches() == n0 + 1, what
                GC.assert_exact(out, GC.reference(x, w, epi, bias, None, dt, acc=acc), what)
                GC.assert_guards(buf, out, what)
    for K in (128, 256, 1152, 11008):
        x, w, q = _census_operands(96, 512, K, dt, "census")
        ref = GC.reference(x, w, "none", None, None, dt)
        for sched in SCHEDS:
            what = f"w8 tile {tid} sched {sched} 96x512x{K}"
            buf, out = GC.guarded(96, 512, dt, DEV)
            n0 = O.w8_launches()
            O.gemm(x, w, out=out, config=O.gemm_config(tid, sched), w8=q)
            assert O.w8_launches() == n0 + 1, what
            GC.assert_exact(out, ref, what)
            GC.assert_guards(buf, out, what)
    x, w, q = _census_operands(96, 512, 11008, dt, "counting")
    GC.assert_exact(O.gemm(x, w, config=O.gemm_config(tid, 0), w8=q), torch.full((96, 512), 11008.0, dtype=dt, device=DEV), f"w8 tile {tid} counting")


def test_w8_slab_census(dt):
    """Every slab of the 8-bit slab mode is the exact product over its own K units; the counting pattern names a dropped k-step."""
    O = ops()
    N = 260
    for K in (1024, 2816):
        x, w, q = _census_operands(65, N, K, dt, "census")
        UP = K // 128
        for M in (17, 64, 65):
            for S in (1, 5, UP):
                what = f"w8 gemm_slabs {M}x{N}x{K} S={S}"
                buf = torch.full((2 * GC.GUARD + S * M * N,), GC.SENTINEL, dtype=torch.float32, device=DEV)
                out = buf[GC.GUARD: GC.GUARD + S * M * N].view(S, M, N)
                n0 = O.w8_launches()
                sl = O.gemm_slabs(x[:M], w, S, out=out, w8=q)
                assert O.w8_launches() == n0 + 1, what
                want = GC.slab_reference(x[:M], w, [p * UP // S * 128 for p in range(S + 1)])
                GC.assert_exact(sl.view(S * M, N), want.view(S * M, N), what)
                assert bool((buf[: GC.GUARD] == GC.SENTINEL).all()) and bool((buf[GC.GUARD + S * M * N:] == GC.SENTINEL).all()), what
    x1, w1, q1 = _census_operands(65, N, 1024, dt, "counting")
    GC.assert_exact(O.gemm_slabs(x1, w1, 5, w8=q1).view(5 * 65, N),
                    torch.tensor([128.0, 256, 128, 256, 256], device=DEV).repeat_interleave(65)[:, None].expand(5 * 65, N).contiguous(), "w8 slabs counting")


def test_w8_gemm_refusals_launch_nothing_and_the_wrapper_falls_back():
    from llava_align_amd import _lib
    O = ops()
    lib = O._lib_ready()
    dtype, dtc = torch.bfloat16, _lib.VDD_BF16
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    M, N = 33, 136

    def raw(x, codes, scale, out, bias, K, epi, cfg):
        ws = O._gemm_workspace(x.device, M, N)
        rc = lib.vdd_gemm_w8(x.data_ptr(), codes.data_ptr(), scale.data_ptr(), out.data_ptr(), bias.data_ptr() if bias is not None else None,
                             M, N, K, x.stride(0), out.stride(0), epi, cfg, ws.data_ptr(), ws.numel(), dtc, st)
        torch.cuda.synchronize()
        return rc

    bias = _bias(N, dtype)
    for name, K, epi, cfg in (("tile id 1", 256, O.EPI_NONE, O.gemm_config(1, 0)), ("GELU epilogue", 256, O.EPI_BIAS_GELU, O.gemm_config(12, 0)),
                              ("K % 128", 320, O.EPI_NONE, O.gemm_config(12, 0))):
        w16, codes, scale = _weight(N, K, dtype)
        x = _rows(M, K, dtype, K)
        out = torch.full((M, N), 7.0, device=DEV, dtype=dtype)
        assert raw(x, codes, scale, out, bias if epi != O.EPI_NONE else None, K, epi, cfg) == -2, name
        assert bool((out == 7.0).all()), name                                      # VDD_ERR_UNSUPPORTED: nothing launched
        if K % 128 != 0:
            continue                                                               # (ops.gemm itself takes K % 128 only)
        n0 = O.w8_launches()
        kw = dict(bias=bias, epi=epi) if epi != O.EPI_NONE else {}
        a = O.gemm(x, w16, config=cfg, w8=(codes, scale), **kw)
        assert O.w8_launches() == n0, name                                         # the wrapper ran the 16-bit GEMM ...
        assert torch.equal(_bits(a), _bits(O.gemm(x, w16, config=cfg, **kw))), name      # ... the same bits
    # the served neighbour of the three: launches
    w16, codes, scale = _weight(N, 256, dtype)
    out = torch.full((M, N), 7.0, device=DEV, dtype=dtype)
    assert raw(_rows(M, 256, dtype, 256), codes, scale, out, None, 256, O.EPI_NONE, O.gemm_config(12, 0)) == 0 and not bool((out == 7.0).all())


@pytest.mark.parametrize("M", [17, 33, 64, 96])
def test_wrappers_take_the_8bit_forms_and_return_the_16bit_bits(monkeypatch, M, dt):
    """linear / linear_to_norm (product and slabs) / swiglu_linear with w8= and the new forms forced, against the same functions forced
    to their 16-bit forms with the same tile and schedule pinned under both tuning keys; with the switch off no 8-bit kernel runs."""
    O = ops()
    N, K, F = 1024, 1024, 256
    dtc = O._MODEL_DT[dt]
    cfg = O.gemm_config(12 if M <= 64 else 10, 0)                                 # both pair gate / up
    pinned = {}
    for n_, epi in ((N, O.EPI_NONE), (N, O.EPI_BIAS), (F, O.EPI_SWIGLU)):
        pinned[O._gemm_key(M, n_, K, epi, dtc)] = cfg
        pinned[O._gemm_key_w8(M, n_, K, epi, dtc)] = cfg
    monkeypatch.setattr(O, "_gemm_choice", pinned)
    monkeypatch.setattr(O, "_form_choice", {})
    w16, codes, scale = _weight(N, K, dt)
    wg16, gcodes, gscale = _weight(2 * F, K, dt)
    x = _rows(M, K, dt, 5 * M)
    bias = _bias(N, dt)
    assert O.slab_splits(M, N, K) >= 4
    calls = {"linear": lambda: O.linear(x, w16, w8=(codes, scale)), "linear+bias": lambda: O.linear(x, w16, bias=bias, w8=(codes, scale)),
             "to_norm": lambda: O.linear_to_norm(x, w16, w8=(codes, scale)), "swiglu": lambda: O.swiglu_linear(x, wg16, w8=(gcodes, gscale))}
    for form8, form16 in (("gemm8", "gemm"), ("slabs8", "slabs")):
        for name, fn in calls.items():
            if form8 == "slabs8" and name != "to_norm":
                continue
            monkeypatch.setattr(O, "FORCE_FORM", {k: form8 for k in ("linear8", "to_norm8", "swiglu8")})
            n0 = O.w8_launches()
            a = fn()
            assert O.w8_launches() == n0 + 1, (name, form8)
            assert a.dim() == (3 if form8 == "slabs8" else 2)
            monkeypatch.setattr(O, "FORCE_FORM", {k: form16 for k in ("linear8", "to_norm8", "swiglu8")})
            b = fn()
            assert O.w8_launches() == n0 + 1, (name, form16)
            assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (name, form8, M)
            monkeypatch.setattr(O, "FORCE_FORM", {**{k: form8 for k in ("linear8", "to_norm8", "swiglu8")}, **{k: form16 for k in ("linear", "to_norm", "swiglu")}})
            with O.w8_decode(False):
                c = fn()
            assert O.w8_launches() == n0 + 1, (name, "switch off")
            assert torch.equal(_bits(a), _bits(c)), (name, "switch off", M)
