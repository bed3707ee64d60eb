"""The three 8-bit-weight projections (vdd_skinny_gemm_normed_w8 / vdd_skinny_swiglu_normed_w8 / vdd_skinny_gemm_resid_ss_w8) against their
16-bit twins on the dequantised weight w16: BIT IDENTITY (torch.equal on the raw 16-bit patterns of Y / act, on the raw fp32 bits of ss_out) -
the codes widen exactly to the twin's MFMA fragments, the MFMAs and the order of the fp32 sums are the twin's, and the power-of-two row scale
commutes with every fp32 addition, so there is no tolerance to choose.

Shapes: the smallest that reach every code path.  M in {1, 2, 3, 5, 8, 9, 16}: the RMAX buckets 2 / 4 / 8 / 16 of the normalise-once prologue
and both of its block plans (4 waves while two copies of the normalised rows fit in LDS, 8 waves beyond).  K in {256, 512, 4096, 5120, 8192},
the normed forms only where M * 2K fits their 142 KiB of LDS (the twins' own limit: 8 rows at 8192, 14 at 5120); 5120 over 8 waves is the ragged
slice (640 = 2 stages + 128).  K = 11008 and 13824 for the d-wide form: 11008 over 8 waves is 43 k-steps per wave - odd, so every second wave
starts in the middle of a 64-element code group - plus a 3-k-step remainder; K = 256 over 8 waves is the one-k-step slice.  N in {16, 40, 1000,
4096}: column tails; N = 5120 is added for the d-wide form because only a column-block count that neither fits one round of the CUs nor
divides into whole rounds takes its 4-wave plan.  F in {8, 20, 512}.  X / H have a row stride larger than K.
Weights: N(0, 0.02) rows; row 0 holds all 254 finite codes, row 1 is zero, rows 2 / 3 / 5 have scales 2^6 and 2^-6 away from their neighbours'.

fp16: codes that dequantise below 2^-14 reach the 16-bit twin's MFMA as fp16 SUBNORMALS, while the 8-bit kernel's fragments hold the (normal)
code values and the scale comes in afterwards, so the equality also says that the matrix core takes subnormal fp16 inputs exactly.  It does: on
unrestricted weights 0 of 82,896 output elements differed when this was first measured on the MI355X, so the fp16 tests run the same
unrestricted weights as the bf16 ones (row 0 alone reaches 2^-19) and assert the same bit identity - no weaker fp16 form is kept."""
import ctypes as C

import pytest
import torch

from llava_align_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MS = (1, 2, 3, 5, 8, 9, 16)
LDS_CAP = 142 * 1024
EPS = 1e-5
_cache = {}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _weight(N, K, dtype):
    """(w16, codes, scale) of an [N, K] test weight (built once per shape and left unchanged)."""
    key = (N, K, dtype)
    if key not in _cache:
        g = torch.Generator(device=DEV).manual_seed(1000 * N + K)
        w = torch.randn(N, K, device=DEV, generator=g) * 0.02
        lut = ops._e4m3_values().to(DEV)
        finite = lut[torch.isfinite(lut)]
        w[0, :254] = finite * 2.0 ** -10                      # every finite code (largest 448: the row's exponent is -10)
        w[0, 254:] = 0.0
        w[0, 255] = 448.0 * 2.0 ** -10
        if N > 1:
            w[1] = 0.0
        if N > 5:
            w[2] *= 64.0
            w[5] *= 1.0 / 64.0
        codes, scale, w16 = ops.quantize_w8(w.to(dtype))
        _cache[key] = (w16, codes, scale)
    return _cache[key]


def _rows(M, K, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    full = (torch.randn(M, K + 64, device=DEV, generator=g) * 0.5).to(dtype)
    return full[:, :K]                                         # row stride K + 64


def _ss(h):
    K = h.shape[1]
    return (h.float() ** 2).reshape(h.shape[0], K // 16, 16).sum(-1).contiguous()        # nss = K / 16 partial sums per row


def _both(fn):
    """fn() with the 8-bit path, then with the switch off (the 16-bit twin on w16); checks that the first really launched 8-bit."""
    n0 = ops.w8_launches()
    a = fn()
    assert ops.w8_launches() == n0 + 1
    with ops.w8_decode(False):
        b = fn()
    assert ops.w8_launches() == n0 + 1
    return a, b


def _normed_case(M, N, K, dtype):
    w16, codes, scale = _weight(N, K, dtype)
    h = _rows(M, K, dtype, 7 * M + K)
    lnw = (1.0 + 0.02 * torch.randn(K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(K))).to(dtype)
    return _both(lambda: ops.linear_normed(h, _ss(h), lnw, EPS, w16, w8=(codes, scale)))


def _swiglu_case(M, F, K, dtype):
    w16, codes, scale = _weight(2 * F, K, dtype)
    h = _rows(M, K, dtype, 11 * M + K)
    lnw = (1.0 + 0.02 * torch.randn(K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(K + 1))).to(dtype)
    return _both(lambda: ops.swiglu_linear_normed(h, _ss(h), lnw, EPS, w16, w8=(codes, scale)))


def _resid_case(M, N, K, dtype):
    w16, codes, scale = _weight(N, K, dtype)
    x = _rows(M, K, dtype, 13 * M + K)
    r = (torch.randn(M, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(M + N)) * 0.5).to(dtype)
    (y8, s8), (y16, s16) = _both(lambda: ops.linear_resid_ss(x, w16, r, w8=(codes, scale)))
    return (y8, s8), (y16, s16)


NORMED_K = (256, 512, 4096, 5120, 8192)
RESID_K = NORMED_K + (11008, 13824)
NS = (16, 40, 1000, 4096)
FS = (8, 20, 512)


def _fits(M, K):
    return M * 2 * K <= LDS_CAP


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", NORMED_K)
def test_normed_w8_is_the_16bit_kernel_on_w16(dtype, K):
    n = 0
    for N in NS:
        for M in MS:
            if not _fits(M, K):
                continue
            y8, y16 = _normed_case(M, N, K, dtype)
            assert torch.equal(_bits(y8), _bits(y16)), (M, N, K)
            n += 1
    assert n >= 4 * 5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", NORMED_K)
def test_swiglu_normed_w8_is_the_16bit_kernel_on_w16(dtype, K):
    for F in FS:
        for M in MS:
            if not _fits(M, K):
                continue
            a8, a16 = _swiglu_case(M, F, K, dtype)
            assert torch.equal(_bits(a8), _bits(a16)), (M, F, K)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", RESID_K)
def test_resid_ss_w8_is_the_16bit_kernel_on_w16(dtype, K):
    for N in NS + (5120,):
        for M in MS:
            (y8, s8), (y16, s16) = _resid_case(M, N, K, dtype)
            assert torch.equal(_bits(y8), _bits(y16)) and torch.equal(_bits(s8), _bits(s16)), (M, N, K)


def test_unsupported_shapes_return_unsupported_and_the_wrapper_falls_back():
    lib = ops._lib_ready()
    dt = _lib.VDD_BF16
    dtype = torch.bfloat16
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    # K % 256 != 0 (the 16-bit d-wide twin takes K % 128)
    M, N, K = 3, 40, 384
    w16, codes, scale = _weight(N, K, dtype)
    x = _rows(M, K, dtype, 5)
    r = (torch.randn(M, N, device=DEV) * 0.5).to(dtype)
    y = torch.full((M, N), 7.0, device=DEV, dtype=dtype)
    ss = torch.zeros(M, 3, device=DEV)
    rc = lib.vdd_skinny_gemm_resid_ss_w8(x.data_ptr(), codes.data_ptr(), scale.data_ptr(), r.data_ptr(), y.data_ptr(), ss.data_ptr(), M, N, K,
                                         x.stride(0), r.stride(0), y.stride(0), dt, st)
    torch.cuda.synchronize()
    assert rc == -2 and bool((y == 7.0).all())                                 # VDD_ERR_UNSUPPORTED, nothing launched
    n0 = ops.w8_launches()
    y8, s8 = ops.linear_resid_ss(x, w16, r, w8=(codes, scale))
    assert ops.w8_launches() == n0                                             # the wrapper ran the 16-bit twin ...
    with ops.w8_decode(False):
        y16, s16 = ops.linear_resid_ss(x, w16, r, w8=(codes, scale))
    assert torch.equal(_bits(y8), _bits(y16)) and torch.equal(_bits(s8), _bits(s16))      # ... the same bits
    # more than 16 rows, and the normed forms beyond their LDS image
    K = 512
    w16, codes, scale = _weight(40, K, dtype)
    h = _rows(16, K, dtype, 6)
    lnw = torch.ones(K, device=DEV, dtype=dtype)
    out = torch.zeros(17, 40, device=DEV, dtype=dtype)
    ssn = _ss(h)
    rc = lib.vdd_skinny_gemm_normed_w8(h.data_ptr(), ssn.data_ptr(), ssn.shape[1], lnw.data_ptr(), C.c_float(EPS), codes.data_ptr(), scale.data_ptr(),
                                       out.data_ptr(), 17, 40, K, h.stride(0), out.stride(0), dt, st)
    assert rc == -2
    w16, codes, scale = _weight(16, 8192, dtype)
    h = _rows(9, 8192, dtype, 8)
    ssn = _ss(h)
    lnw = torch.ones(8192, device=DEV, dtype=dtype)
    out = torch.zeros(9, 8, device=DEV, dtype=dtype)
    rc = lib.vdd_skinny_swiglu_normed_w8(h.data_ptr(), ssn.data_ptr(), ssn.shape[1], lnw.data_ptr(), C.c_float(EPS), codes.data_ptr(), scale.data_ptr(),
                                         out.data_ptr(), 9, 8, 8192, h.stride(0), dt, st)
    assert rc == -2                                                            # 9 x 16 KiB of normalised rows do not fit
