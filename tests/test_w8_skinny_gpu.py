"""vdd_skinny_gemm_w8 / vdd_skinny_swiglu_w8 - the plain weight-streaming kernels reading e4m3 codes - against their 16-bit twins
(vdd_skinny_gemm without residual and slabs, vdd_skinny_swiglu) on the dequantised weight w16: BIT IDENTITY, as for the norm-fused forms
(tests/test_w8_kernels_gpu.py, whose weights are used here: a row of all 254 finite codes, a zero row, rows 64 x and 1 / 64 x their
neighbours' scale; x = randn * 0.5 with a padded row stride).  fp16 runs the same unrestricted weights (row 0 dequantises down to 2^-19).

One case per dispatch branch of the 16-bit entry:
    M = 1, 9, 16     N = 48 (3 column blocks: eight waves per block) and N = 5120 (320 blocks - neither one round of the CUs nor whole
                     rounds: four waves per block); K = 256 / 512 (a wave slice of ONE k-step over eight waves, the remainder batch alone),
                     2816 (eight waves: 11 k-steps per wave - odd, every second wave starts in the middle of a 64-element code group) and
                     4096 (both register stages in flight)
    M = 17, 32       N = 48, K = 512 and 4096: two MFMA row tiles
    M = 33, 64       N = 48, K = 512 and 4096: four row tiles (stages of four k-steps)
    M = 17, 40, 64   N = 8208 (> 8192: the 32-column blocks, MT = 2 / 3 / 4; 8208 = 256 * 32 + 16: the last block owns ONE column tile),
                     K = 256 (remainder batch alone for MT = 2 / 3, one stage for MT = 4), 1024 and 2816 (stages + remainder)
    M = 33           N = 48, K = 11008: 86 k-steps per wave = 21 stages + a remainder of two
SwiGLU: M = 2, 16 (8 features per block) and 17, 40, 64 (16 features per block), F = 40 (a ragged last block in either form) and 128,
K = 256, 512 and 2816 (the up-to-16-row kernel's k-step-by-k-step tail).
A twin comparison cannot see a fault both kernels share, so the exact-integer census of tests/gemm_census.py runs on the 8-bit entries too."""
import pytest
import torch

import gemm_census as GC
from test_w8_kernels_gpu import _bits, _rows, _weight

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNSUPPORTED = -2


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def dt(request):
    return request.param


def ops():
    from llava_align_amd import ops as O
    return O


def _twin(fn, M, N, dtype, ldy_extra, what):
    """fn(out, w8 on?) on codes and on w16 into guarded sentinel buffers: the same bits, one 8-bit launch counted, guards intact"""
    O = ops()
    outs = []
    for on in (True, False):
        buf, out = GC.guarded(M, N, dtype, DEV, ldy=N + ldy_extra)
        n0 = O.w8_launches()
        fn(out, on)
        assert O.w8_launches() == n0 + (1 if on else 0), what
        GC.assert_guards(buf, out, what)
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), what
    assert not bool((outs[0] == GC.SENTINEL).any()), what
    return outs[0]


GEMM_CASES = ([(M, 48, K) for M in (1, 9, 16) for K in (256, 512, 2816, 4096)] + [(M, 5120, K) for M in (1, 9, 16) for K in (256, 512)]
              + [(M, 48, K) for M in (17, 32, 33, 64) for K in (512, 4096)]
              + [(M, 8208, K) for M in (17, 40, 64) for K in (256, 1024, 2816)] + [(33, 48, 11008)])


def test_skinny_gemm_w8_is_the_16bit_kernel_on_w16(dt):
    O = ops()
    for M, N, K in GEMM_CASES:
        w16, codes, scale = _weight(N, K, dt)
        assert len(set(scale.tolist())) >= 3                      # rows with different scales: a neighbour's scale would show
        x = _rows(M, K, dt, 19 * M + K)
        assert x.stride(0) == K + 64
        for ldy_extra in (0, 8):
            _twin(lambda out, on: O.skinny_gemm(x, w16, out=out, w8=(codes, scale) if on else None), M, N, dt, ldy_extra,
                  f"skinny_gemm {M}x{N}x{K} ldy+{ldy_extra}")


def test_dispatch_branches_are_the_ones_the_cases_name():
    """eight_wave_blocks of csrc/vdd_llm_kernels.hip restated: N = 48 takes the eight-wave blocks and N = 5120 the four-wave ones on this chip"""
    n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
    blocks = lambda N: -(-N // 16)
    assert blocks(48) <= n_cu
    assert blocks(5120) > n_cu and blocks(5120) % n_cu != 0


@pytest.mark.parametrize("F", [40, 128])
def test_skinny_swiglu_w8_is_the_16bit_kernel_on_w16(F, dt):
    O = ops()
    for K in (256, 512, 2816):
        w16, codes, scale = _weight(2 * F, K, dt)
        for M in (2, 16, 17, 40, 64):
            x = _rows(M, K, dt, 23 * M + K)
            _twin(lambda out, on: O._skinny_swiglu(x, w16, out, w8=(codes, scale) if on else None), M, F, dt, 0, f"skinny_swiglu {M}x{F}x{K}")


def _census_operands(M, N, K, dtype, pattern):
    O = ops()
    if pattern == "counting":
        x, w = GC.counting(M, N, K, dtype, device=DEV)
    else:
        x, w, _ = GC.operands(M, N, K, dtype, seed=2, device=DEV, x_pad=64)
    codes, scale, w16 = O.quantize_w8(w)
    assert torch.equal(w16, w), (M, N, K, pattern)                # the census weights quantise without loss
    return x, w, (codes, scale)


@pytest.mark.parametrize("M,N,K", [(9, 48, 2816), (40, 48, 1024), (40, 8208, 768)], ids=["up_to_16_rows", "narrow", "wide"])
def test_skinny_gemm_w8_census(M, N, K, dt):
    """Exact integers: the output is the fp64 product rounded once, whatever the order of the fp32 additions; the counting pattern reads
    as 'this output summed K - 32 terms'."""
    O = ops()
    for pattern in ("census", "counting"):
        x, w, q = _census_operands(M, N, K, dt, pattern)
        what = f"skinny_gemm w8 {pattern} {M}x{N}x{K}"
        buf, out = GC.guarded(M, N, dt, DEV)
        n0 = O.w8_launches()
        O.skinny_gemm(x, w, out=out, w8=q)
        assert O.w8_launches() == n0 + 1, what
        GC.assert_exact(out, GC.reference(x, w, "none", None, None, dt), what)
        GC.assert_guards(buf, out, what)


@pytest.mark.parametrize("M", [12, 40])
def test_skinny_swiglu_w8_census(M, dt):
    """gate and up are exact integers before the activation; the caps are those of every SwiGLU epilogue (tests/gemm_census.py,
    assert_ulps: two roundings -> 2 representable values, at most 1 % of the entries off at all)."""
    O = ops()
    F, K = 40, 768
    for pattern in ("census", "counting"):
        x, w, q = _census_operands(M, 2 * F, K, dt, pattern)
        what = f"skinny_swiglu w8 {pattern} {M}x{F}x{K}"
        buf, out = GC.guarded(M, F, dt, DEV)
        n0 = O.w8_launches()
        O._skinny_swiglu(x, w, out, w8=q)
        assert O.w8_launches() == n0 + 1, what
        GC.assert_ulps(out, GC.reference(x, w, "swiglu", None, None, dt), 2, 0.01, what)
        GC.assert_guards(buf, out, what)


def test_refusals_launch_nothing_and_the_wrapper_falls_back():
    from llava_align_amd import _lib
    O = ops()
    lib = O._lib_ready()
    dtype, dtc = torch.bfloat16, _lib.VDD_BF16
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    for name, M, K in (("M = 65", 65, 512), ("K = 320", 12, 320), ("K = 320 above 16 rows", 40, 320), ("K % 256", 12, 384)):
        N = F = 48
        w16, codes, scale = _weight(2 * F, K, dtype)
        x = _rows(M, K, dtype, K)
        out = torch.full((M, N), 7.0, device=DEV, dtype=dtype)
        rc = lib.vdd_skinny_gemm_w8(x.data_ptr(), codes.data_ptr(), scale.data_ptr(), out.data_ptr(), M, N, K, x.stride(0), out.stride(0), dtc, st)
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and bool((out == 7.0).all()), name
        rc = lib.vdd_skinny_swiglu_w8(x.data_ptr(), codes.data_ptr(), scale.data_ptr(), out.data_ptr(), M, F, K, x.stride(0), dtc, st)
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and bool((out == 7.0).all()), name
    # the served neighbour: launches
    w16, codes, scale = _weight(48, 512, dtype)
    x = _rows(64, 512, dtype, 1)
    out = torch.full((64, 48), 7.0, device=DEV, dtype=dtype)
    rc = lib.vdd_skinny_gemm_w8(x.data_ptr(), codes.data_ptr(), scale.data_ptr(), out.data_ptr(), 64, 48, 512, x.stride(0), out.stride(0), dtc, st)
    torch.cuda.synchronize()
    assert rc == 0 and not bool((out == 7.0).any())
    # the wrappers run the 16-bit twin on w16 for what the 8-bit entries do not serve: K % 256 != 0, a residual, slabs - the same bits, no 8-bit launch
    for M in (12, 24):
        K = 384
        w16, codes, scale = _weight(48, K, dtype)
        wg16, gcodes, gscale = _weight(96, K, dtype)
        x = _rows(M, K, dtype, M)
        r = (torch.randn(M, 48, device=DEV, generator=torch.Generator(device=DEV).manual_seed(M)) * 0.5).to(dtype)
        calls = {"K % 256": lambda q: O.skinny_gemm(x, w16, w8=q), "residual": lambda q: O.skinny_gemm(x, w16, resid=r, w8=q),
                 "slabs": lambda q: O.skinny_gemm(x, w16, n_split=3, slabs=True, w8=q)}
        if M <= 16:                                                                # (the 16-bit SwiGLU kernel above 16 rows takes K % 256 only)
            calls["swiglu K % 256"] = lambda q: O._skinny_swiglu(x, wg16, w8=(gcodes, gscale) if q else None)
        for name, fn in calls.items():
            n0 = O.w8_launches()
            a = fn((codes, scale))
            assert O.w8_launches() == n0, (name, M)
            assert torch.equal(_bits(a), _bits(fn(None))), (name, M)
    # a residual at a K the 8-bit entry serves is 16-bit too
    w16, codes, scale = _weight(48, 512, dtype)
    x = _rows(12, 512, dtype, 3)
    r = (torch.randn(12, 48, device=DEV) * 0.5).to(dtype)
    n0 = O.w8_launches()
    a = O.skinny_gemm(x, w16, resid=r, w8=(codes, scale))
    assert O.w8_launches() == n0 and torch.equal(_bits(a), _bits(O.skinny_gemm(x, w16, resid=r)))


def test_above_64_rows_the_wrappers_offer_no_skinny8(monkeypatch):
    """65 rows with "skinny8" forced: not eligible, so the projection runs the GEMM (on codes or on w16, whichever it measures) - with one
    data-parallel tile pinned under both tuning keys, the bits of the switch off."""
    from llava_align_amd import _lib
    O = ops()
    dtype, dtc = torch.bfloat16, _lib.VDD_BF16
    M, N, K = 65, 1024, 1024
    cfg = O.gemm_config(10, 1)
    monkeypatch.setattr(O, "_gemm_choice", {O._gemm_key(M, N, K, O.EPI_NONE, dtc): cfg, O._gemm_key_w8(M, N, K, O.EPI_NONE, dtc): cfg})
    monkeypatch.setattr(O, "_form_choice", {})
    monkeypatch.setattr(O, "_load_persisted", lambda device: None)
    monkeypatch.setattr(O, "_persist", {"loaded": None, "path": None, "section": None})
    monkeypatch.setattr(O, "FORCE_FORM", {"linear8": "skinny8", "linear": "skinny"})
    w16, codes, scale = _weight(N, K, dtype)
    x = _rows(M, K, dtype, 65)
    a = O.linear(x, w16, w8=(codes, scale))
    assert O._form_choice[O._form_key("linear8", M, N, K, dtc)] in ("gemm", "gemm8")
    with O.w8_decode(False):
        b = O.linear(x, w16, w8=(codes, scale))
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("M", [12, 24, 48])
def test_wrappers_take_skinny8_and_return_the_bits_of_skinny(monkeypatch, M, dt):
    """linear (with and without bias) / linear_to_norm / swiglu_linear with w8= and "skinny8" forced for the three 8-bit kinds: one 8-bit
    launch each and the bits of "skinny"; with the switch off no 8-bit kernel runs."""
    O = ops()
    N, K, F = 1024, 1024, 256
    monkeypatch.setattr(O, "_form_choice", {})
    w16, codes, scale = _weight(N, K, dt)
    wg16, gcodes, gscale = _weight(2 * F, K, dt)
    x = _rows(M, K, dt, 5 * M)
    bias = (torch.randn(N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(N)) * 0.5).to(dt)
    calls = {"linear": lambda: O.linear(x, w16, w8=(codes, scale)), "linear+bias": lambda: O.linear(x, w16, bias=bias, w8=(codes, scale)),
             "to_norm": lambda: O.linear_to_norm(x, w16, w8=(codes, scale)), "swiglu": lambda: O.swiglu_linear(x, wg16, w8=(gcodes, gscale))}
    kinds8, kinds16 = ("linear8", "to_norm8", "swiglu8"), ("linear", "to_norm", "swiglu")
    for name, fn in calls.items():
        monkeypatch.setattr(O, "FORCE_FORM", {k: "skinny8" for k in kinds8})
        n0 = O.w8_launches()
        a = fn()
        assert O.w8_launches() == n0 + 1, name
        monkeypatch.setattr(O, "FORCE_FORM", {k: "skinny" for k in kinds8})
        b = fn()
        assert O.w8_launches() == n0 + 1, name
        assert a.dim() == 2 and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (name, M)
        monkeypatch.setattr(O, "FORCE_FORM", {**{k: "skinny8" for k in kinds8}, **{k: "skinny" for k in kinds16}})
        with O.w8_decode(False):
            c = fn()
        assert O.w8_launches() == n0 + 1, (name, "switch off")
        assert torch.equal(_bits(a), _bits(c)), (name, "switch off", M)
    assert not O._form_choice                                                      # forced forms measure nothing


@pytest.mark.parametrize("M", [2, 10, 16])
def test_linear_keep_bits_stays_inside_the_16bit_form(monkeypatch, M, dt):
    """linear(w8=, keep_bits=True) - layer 0's qkv of the few-row step - returns the bits of the call without codes whichever form that
    call takes: one 8-bit launch where it is "skinny" (the twin, forced under "linear8t"), none where it is the GEMM, and a forced
    "linear8" form is not consulted."""
    O = ops()
    N, K = 1024, 1024
    monkeypatch.setattr(O, "_form_choice", {})
    w16, codes, scale = _weight(N, K, dt)
    x = _rows(M, K, dt, 7 * M)
    for form16, launches in (("skinny", 1), ("gemm", 0)):
        monkeypatch.setattr(O, "FORCE_FORM", {"linear": form16, "linear8t": "skinny8", "linear8": "gemm8" if form16 == "skinny" else "skinny8"})
        n0 = O.w8_launches()
        a = O.linear(x, w16, w8=(codes, scale), keep_bits=True)
        assert O.w8_launches() == n0 + launches, form16
        b = O.linear(x, w16)
        assert O.w8_launches() == n0 + launches and torch.equal(_bits(a), _bits(b)), (form16, M)
