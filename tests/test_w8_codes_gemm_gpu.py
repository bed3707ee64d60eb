"""vdd_gemm_codes - the MFMA GEMM for a weight that exists as e4m3 codes ONLY - against its 16-bit twin, vdd_gemm with the same config on
the dequantised weight: BIT IDENTITY, as for vdd_gemm_w8 (tests/test_w8_gemm_gpu.py, whose shapes, weights and helpers these tests
share).  New ground: the compute-bound tiles (ids 1 - 4 and 6: two K-tile buffers, 64-byte W rows; 192 x 256 without the third W image
of its twin; 256 x 256, 192 x 256 and 192 x 192 read 8 bytes of codes per k-step), any M for the W-stream tiles, and the refusals - tile
id 5 (256 x 192) has no 8-bit form.  A twin comparison cannot see a fault both kernels share, so the exact-integer census of
tests/gemm_census.py runs on the new tiles too."""
import pytest
import torch

import gemm_census as GC
from test_gemm_census_gpu import NO_SWIGLU, P, SCHEDS, TILES, _partial_round_shape, plan, stage_out, wave_tn
from test_w8_gemm_gpu import _bias, _census_operands, _rounds_then_sk_shape
from test_w8_kernels_gpu import _bits, _rows, _weight

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEFT_OUT = (5,)                                           # 256 x 192: 12 code images over 8 waves


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def dt(request):
    return request.param


def ops():
    from llava_align_amd import ops as O
    return O


def new_tiles():
    O = ops()
    return tuple(t for t in O.W8_CODES_TILES if t not in O.W8_GEMM_TILES)


NEW = (1, 2, 3, 4, 6)                                     # what new_tiles() must return (parametrisation happens at import, without the library)


def _twin(x, w16, q, epi, cfg, N, bias=None, ldy_extra=0, what=""):
    """one launch on the codes-only weight and one on w16 into guarded sentinel buffers: the same bits, one 8-bit launch counted, guards intact"""
    O = ops()
    M = x.shape[0]
    outs = []
    for w in (O.CodesWeight(q[0], q[1], x.dtype), w16):
        buf, out = GC.guarded(M, N, x.dtype, DEV, ldy=N + ldy_extra)
        n0 = O.w8_launches()
        O.gemm(x, w, bias=bias, epi=epi, out=out, config=cfg)
        assert O.w8_launches() == n0 + (1 if w is not w16 else 0), what
        GC.assert_guards(buf, out, what)
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), what
    return outs[0]


def test_served_tiles_are_every_tile_but_256x192():
    O = ops()
    assert tuple(O.W8_CODES_TILES) == tuple(t for t in sorted(TILES) if t not in LEFT_OUT)
    assert new_tiles() == NEW and set(O.W8_GEMM_TILES) < set(O.W8_CODES_TILES)
    for t in (1, 2, 4):                                   # the prefill and the 1,536-row decode batch
        assert t in O.W8_CODES_TILES


@pytest.mark.parametrize("tid", NEW)
def test_codes_gemm_is_the_16bit_gemm_on_w16(tid, dt):
    O = ops()
    BM, BN, _, _ = TILES[tid]
    classes = (("one_row_tile", (BM - 1, 3 * BN + 4, 384)), ("partial_round", _partial_round_shape(tid)), ("rounds_then_sk", _rounds_then_sk_shape(tid)))
    seen = set()
    for ci, (name, (M, N, K)) in enumerate(classes):
        w16, codes, scale = _weight(N, K, dt)
        assert len(set(scale.tolist())) >= 3
        x = _rows(M, K, dt, 17 * M + K)
        bias = _bias(N, dt)
        F = -(-N // 128) * 128
        swiglu = tid not in NO_SWIGLU and ci < 2
        if swiglu:
            wg16, gcodes, gscale = _weight(2 * F, K, dt)
        for sched in SCHEDS:
            p = plan(M, N, K, tid, sched)
            if name == "one_row_tile":
                assert p["Mt"] == 1 and p["Nt"] == 4 and p["UP"] == 3 and p["T"] < P() and N % 8 == 4
            elif name == "partial_round":
                assert p["Mt"] == 5 and M % BM == 1 and N % 8 == 4 and P() + 37 <= p["T"] < 2 * P()
            else:
                assert p["T"] >= 2 * P() + 37 and p["Mt"] == 5
            cfg = O.gemm_config(tid, sched)
            what = f"tile {tid} sched {sched} {name} {M}x{N}x{K}"
            for ldy_extra in (0, 4):
                out = _twin(x, w16, (codes, scale), O.EPI_NONE, cfg, N, ldy_extra=ldy_extra, what=what + f" none ldy+{ldy_extra}")
                assert stage_out(out) == (ldy_extra == 4)
                seen.add("staged" if (stage_out(out) and wave_tn(tid) % 64 == 0) else "unstaged")
            if ci < 2:
                _twin(x, w16, (codes, scale), O.EPI_BIAS, cfg, N, bias=bias, ldy_extra=4 * (sched & 1), what=what + " bias")
            if swiglu:
                _twin(x, wg16, (gcodes, gscale), O.EPI_SWIGLU, cfg, F, ldy_extra=8 * (sched & 1) + 4 * (sched >> 1), what=what + " swiglu")
    assert seen == ({"staged", "unstaged"} if wave_tn(tid) % 64 == 0 else {"unstaged"})


@pytest.mark.parametrize("tid", NEW)
def test_codes_gemm_k_edges(tid, dt):
    """K = 128 (two K-tiles: the pipeline's prologue and tail alone), K = 256 (the first K at which tile t + 2 is staged behind the barrier;
    where the 192 x 256 twin first stages its third W image, which the 8-bit form does not have) and K = 11008 (172 K-tiles).  Tile 4 is the
    one whose pipeline differs from its twin's; the other new tiles run the same cases (they read codes with another LDS layout)."""
    O = ops()
    BM, BN, _, _ = TILES[tid]
    M, N = BM + 1, BN + 4
    for K in (128, 256, 11008):
        w16, codes, scale = _weight(N, max(K, 256), dt)
        w16, codes = w16[:, :K].contiguous(), codes[:, :K].contiguous()          # (whole 64-element groups: the storage order holds)
        x = _rows(M, K, dt, 3 * M + K)
        for sched in SCHEDS:
            _twin(x, w16, (codes, scale), O.EPI_NONE, O.gemm_config(tid, sched), N, ldy_extra=4 * (sched & 1), what=f"tile {tid} sched {sched} K={K}")


@pytest.mark.parametrize("tid", NEW)
def test_codes_gemm_census_plain_and_bias(tid, dt):
    O = ops()
    BM, BN, _, _ = TILES[tid]
    M, N, K = BM - 1, 3 * BN + 4, 384
    for pattern in ("census", "counting"):
        x, w, q = _census_operands(M, N, K, dt, pattern)
        cw = O.CodesWeight(q[0], q[1], dt)
        bias, _ = GC.side_inputs(M, N, dt, 2, device=DEV)
        acc = GC.product(x, w)
        for sched in SCHEDS:
            for epi, code, b in (("none", O.EPI_NONE, None), ("bias", O.EPI_BIAS, bias)):
                what = f"codes tile {tid} sched {sched} {pattern} {epi} {M}x{N}x{K}"
                buf, out = GC.guarded(M, N, dt, DEV)
                n0 = O.w8_launches()
                O.gemm(x, cw, bias=b, epi=code, out=out, config=O.gemm_config(tid, sched))
                assert O.w8_launches() == n0 + 1, what
                GC.assert_exact(out, GC.reference(x, w, epi, bias, None, dt, acc=acc), what)
                GC.assert_guards(buf, out, what)
    for K in (128, 256, 1152, 11008):
        x, w, q = _census_operands(96, 512, K, dt, "census")
        cw = O.CodesWeight(q[0], q[1], dt)
        ref = GC.reference(x, w, "none", None, None, dt)
        for sched in SCHEDS:
            what = f"codes tile {tid} sched {sched} 96x512x{K}"
            buf, out = GC.guarded(96, 512, dt, DEV)
            O.gemm(x, cw, out=out, config=O.gemm_config(tid, sched))
            GC.assert_exact(out, ref, what)
            GC.assert_guards(buf, out, what)
    x, w, q = _census_operands(96, 512, 11008, dt, "counting")
    GC.assert_exact(O.gemm(x, O.CodesWeight(q[0], q[1], dt), config=O.gemm_config(tid, 0)), torch.full((96, 512), 11008.0, dtype=dt, device=DEV),
                    f"codes tile {tid} counting")


@pytest.mark.parametrize("tid", [7, 12])
@pytest.mark.parametrize("M", [257, 1025])
def test_w_stream_tiles_above_256_rows(tid, M, dt):
    """vdd_gemm_codes launches the W-stream instantiations at any M (vdd_gemm_w8's wrapper stops tuning them at 256 rows)."""
    O = ops()
    N, K = 3 * TILES[tid][1] + 4, 384
    w16, codes, scale = _weight(N, K, dt)
    x = _rows(M, K, dt, 7 * M)
    for sched in SCHEDS:
        _twin(x, w16, (codes, scale), O.EPI_NONE, O.gemm_config(tid, sched), N, ldy_extra=4 * (sched & 1), what=f"tile {tid} M={M} sched {sched}")


def test_codes_gemm_refusals_launch_nothing():
    from llava_align_amd import _lib
    O = ops()
    lib = O._lib_ready()
    dtype, dtc = torch.bfloat16, _lib.VDD_BF16
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    M, N = 33, 136

    def raw(x, codes, scale, out, bias, K, epi, cfg):
        ws = O._gemm_workspace(x.device, M, N)
        rc = lib.vdd_gemm_codes(x.data_ptr(), codes.data_ptr(), scale.data_ptr(), out.data_ptr(), bias.data_ptr() if bias is not None else None,
                                M, N, K, x.stride(0), out.stride(0), epi, cfg, ws.data_ptr(), ws.numel(), dtc, st)
        torch.cuda.synchronize()
        return rc

    bias = _bias(N, dtype)
    # (what is refused, K, epilogue, config) and its served neighbour (K, epilogue, config)
    cases = (("GELU epilogue", 256, O.EPI_BIAS_GELU, O.gemm_config(1, 0), (256, O.EPI_BIAS, O.gemm_config(1, 0))),
             ("K % 128", 320, O.EPI_NONE, O.gemm_config(2, 0), (256, O.EPI_NONE, O.gemm_config(2, 0))),
             ("a residual", 256, O.EPI_BIAS_RESID, O.gemm_config(4, 0), (256, O.EPI_BIAS, O.gemm_config(4, 0))),
             ("tile id 5", 256, O.EPI_NONE, O.gemm_config(5, 0), (256, O.EPI_NONE, O.gemm_config(6, 0))),
             ("tile id 5, data-parallel", 256, O.EPI_BIAS, O.gemm_config(5, 1), (256, O.EPI_BIAS, O.gemm_config(3, 1))))
    for name, K, epi, cfg, (K1, epi1, cfg1) in cases:
        w16, codes, scale = _weight(N, K, dtype)
        x = _rows(M, K, dtype, K)
        out = torch.full((M, N), 7.0, device=DEV, dtype=dtype)
        assert raw(x, codes, scale, out, bias if epi != O.EPI_NONE else None, K, epi, cfg) == -2, name
        assert bool((out == 7.0).all()), name                                      # VDD_ERR_UNSUPPORTED: nothing launched, nothing written
        w16, codes, scale = _weight(N, K1, dtype)
        assert raw(_rows(M, K1, dtype, K1), codes, scale, out, bias if epi1 != O.EPI_NONE else None, K1, epi1, cfg1) == 0, name
        assert not bool((out == 7.0).all()), name                                  # the served neighbour launches
    # the wrapper has no 16-bit weight to fall back to: it raises, naming the shape
    w16, codes, scale = _weight(N, 256, dtype)
    cw, x = O.CodesWeight(codes, scale, dtype), _rows(M, 256, dtype, 256)
    n0 = O.w8_launches()
    with pytest.raises(ValueError, match="N=136"):
        O.gemm(x, cw, config=O.gemm_config(5, 0))
    with pytest.raises(ValueError):
        O.gemm(x, cw, bias=bias, resid=torch.zeros(M, N, device=DEV, dtype=dtype), epi=O.EPI_BIAS_RESID)
    with O.w8_decode(False):
        with pytest.raises(RuntimeError):
            O.gemm(x, cw, config=O.gemm_config(1, 0))
    assert O.w8_launches() == n0
