"""ops.quantize_w8 (host, load time): e4m3fn codes + one power-of-two fp32 scale per output row, and the dequantised 16-bit weight w16 that
the whole engine runs.  CPU only.  Every bound here is derived from the format - e4m3 has 3 mantissa bits (relative spacing 2^-3, so RNE
errs by at most 2^-4 of the value) and a subnormal spacing of 2^-9 (RNE errs by at most 2^-10) - none is tuned.

One point where the rows fixed for this test meet the quantiser's own fp16 rule: the row scaled by 1e-3 has its largest magnitude near 2^-14,
so the unconstrained exponent would be about -22; for fp16 the quantiser keeps e >= -15 (the smallest code, 2^-9, must land on an fp16 value,
2^-24).  The "largest code in [224, 448]" property therefore holds for every non-zero row whose unconstrained exponent is >= -15 - all rows in
bf16, all but that one in fp16 - and for the clamped row the test asserts e == -15 and a largest code <= 448 instead."""
import pytest
import torch

from llava_align_amd import ops

K = 256
LUT = ops._e4m3_values()
FINITE = [c for c in range(256) if (c & 0x7F) != 0x7F]


def _rows(dtype):
    g = torch.Generator().manual_seed(11)
    w = torch.randn(12, K, generator=g) * 0.02
    w[1] = 0.0                                                    # a zero row
    w[2] *= 1e-3                                                  # a tiny row
    w[3] *= 50.0                                                  # a large row
    # a row whose quantisation hits every finite code: the 254 finite e4m3 values themselves (largest 448: e = 0 before scaling), times 2^-10
    allc = LUT[torch.tensor(FINITE)]
    w[4] = torch.cat([allc, torch.tensor([448.0, -448.0])]) * 2.0 ** -10
    return w.to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_quantize_w8_rows(dtype):
    w = _rows(dtype)
    codes, scale, w16 = ops.quantize_w8(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    assert w16.dtype == dtype and w16.shape == w.shape
    m, e = torch.frexp(scale)
    assert bool((m == 0.5).all())                                 # exact powers of two
    e = e - 1
    nat = ops.w8_unpack(codes)
    assert not bool(((nat & 0x7F) == 0x7F).any())                 # no NaN codes
    assert e[1].item() == 0 and not bool(nat[1].any())            # the zero row: e = 0, all codes +0
    val = LUT[nat.long()]                                         # fp32 value of every code
    a = w.float().abs().amax(dim=1)
    m_a, e_a = torch.frexp(a)
    e_free = torch.where(m_a <= 0.875, e_a - 9, e_a - 8)          # smallest e with a 2^-e <= 448, before the fp16 floor
    for n in range(w.shape[0]):
        if n == 1:
            continue
        top = val[n].abs().max().item()
        if dtype == torch.float16 and e_free[n].item() < -15:
            assert e[n].item() == -15 and top <= 448.0
        else:
            assert e[n].item() == e_free[n].item() and 224.0 <= top <= 448.0, (n, top)
    if dtype == torch.float16:
        assert int(e.min()) >= -15 and e[2].item() == -15
    else:
        assert e[2].item() < -15
    assert set(nat[4].tolist()) == set(FINITE)                    # every finite code occurs
    # w16 == code * scale exactly, in fp32 and after the round trip through the storage type
    prod = val * scale[:, None]
    assert torch.equal(w16.float(), prod) and torch.equal(prod.to(dtype).float(), prod)
    assert torch.equal(ops.w8_dequantize(codes, scale, dtype), w16)
    # quantising the quantised weight changes nothing
    c2, s2, w2 = ops.quantize_w8(w16)
    assert torch.equal(w2, w16) and torch.equal(ops.w8_dequantize(c2, s2, dtype), w16)
    # the error, per element: a = |W|, e the row's exponent
    wf = w.float()
    x = wf.abs() / scale[:, None]
    err = (w16.float() - wf).abs()
    normal = x >= 2.0 ** -6
    assert bool((err[normal] <= 2.0 ** -4 * wf.abs()[normal]).all())
    assert bool((err[~normal] <= (2.0 ** -10 * scale[:, None]).expand_as(err)[~normal]).all())
    if hasattr(torch, "float8_e4m3fn"):                           # the same codes as torch's own RNE cast
        assert torch.equal((wf / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), nat)


def test_every_finite_code_is_a_value_of_both_storage_types():
    v = LUT[torch.tensor(FINITE)]
    assert len(FINITE) == 254 and bool(torch.isfinite(v).all())
    for dtype in (torch.bfloat16, torch.float16):
        assert torch.equal(v.to(dtype).float(), v)
        assert torch.equal((v * 2.0 ** -15).to(dtype).float(), v * 2.0 ** -15)      # at the fp16 floor of the exponent as well


def test_w8_pack_is_the_documented_order_and_unpack_inverts_it():
    x = torch.arange(3 * 192, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(3, 192)
    p = ops.w8_pack(x)
    assert torch.equal(ops.w8_unpack(p), x) and torch.equal(ops.w8_pack(ops.w8_unpack(x)), x)
    k = torch.arange(192)
    byte = (k // 64) * 64 + ((k % 32) // 8) * 16 + ((k % 64) // 32) * 8 + k % 8      # include/vdd_hip.h, "8-bit weight rows"
    assert sorted(byte.tolist()) == list(range(192))
    assert torch.equal(p[:, byte], x)
    # lane group g's 16 bytes of a 64-group: its 8 elements of k-step 2b, then its 8 of k-step 2b + 1
    assert p[0, 16:32].tolist() == x[0, 8:16].tolist() + x[0, 40:48].tolist()
    with pytest.raises(ValueError):
        ops.w8_pack(torch.zeros(2, 96, dtype=torch.uint8))


def test_quantize_w8_rejects_what_it_cannot_represent():
    w = torch.zeros(2, 64, dtype=torch.bfloat16)
    for bad in (float("inf"), float("-inf"), float("nan")):
        w2 = w.clone()
        w2[1, 3] = bad
        with pytest.raises(ValueError):
            ops.quantize_w8(w2)
    with pytest.raises(ValueError):
        ops.quantize_w8(torch.zeros(2, 64))                       # fp32: not a model dtype
    with pytest.raises(ValueError):
        ops.quantize_w8(torch.zeros(64, dtype=torch.bfloat16))


def test_switch_counter_and_key_slot():
    assert ops.W8_DECODE is True and isinstance(ops.w8_launches(), int)
    with ops.w8_decode(False):
        assert ops.W8_DECODE is False
        with ops.w8_decode(True):
            assert ops.W8_DECODE is True
        assert ops.W8_DECODE is False
    assert ops.W8_DECODE is True
    # the fused-versus-plain choice of the 8-bit layer lives under its own key (8 in the fourth slot) and never reads the 16-bit one
    saved = dict(ops._form_choice)
    try:
        ops._form_choice.clear()
        dt = ops._MODEL_DT[torch.bfloat16]
        ops._form_choice[("layer", 12, 4096, 0, dt)] = "plain"
        assert not ops.norm_fused_pays(12, 4096) and not ops.norm_fused_pays(12, 4096, w8=True)      # (no 8-bit record: the generic fallback, 8 rows)
        assert ops.norm_fused_pays(4, 4096, w8=True)
        ops._form_choice[("layer", 12, 4096, 8, dt)] = "fused"
        assert ops.norm_fused_pays(12, 4096, w8=True) and not ops.norm_fused_pays(12, 4096)
        ops.gemm_choices_import(ops.form_choices_export())                                           # the key survives the cache file's text form
        assert ops._form_choice[("layer", 12, 4096, 8, dt)] == "fused"
    finally:
        ops._form_choice.clear()
        ops._form_choice.update(saved)


def test_load_4bit_raises_and_default_engine_weights_have_no_codes():
    from llava_align_amd.engine import LlavaWeights, VddLlavaEngine, preset
    with pytest.raises(NotImplementedError):
        VddLlavaEngine("tiny", device="cpu", load_4bit=True)
    cfg = preset("tiny")
    w = LlavaWeights(cfg, "cpu", torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    lm = cfg.lm
    for i in range(lm.n_layers):
        for n, shape in (("wqkv", (3 * lm.d, lm.d)), ("wo", (lm.d, lm.d)), ("wgu", (2 * lm.ffn, lm.d)), ("wd", (lm.d, lm.ffn))):
            w.t[f"l{i}.{n}"] = (torch.randn(*shape, generator=g) * 0.02).to(torch.bfloat16)
    w.t["lm_head"] = (torch.randn(lm.vocab + 3, lm.d, generator=g) * 0.02).to(torch.bfloat16)       # rows not a multiple of 8: padded codes
    w.t["embed"] = w.t["lm_head"].clone()
    before = {k: v.clone() for k, v in w.t.items()}
    assert not any(k.endswith(".w8") for k in w.t)
    w.quantize_lm_w8()
    for name in [f"l{i}.{n}" for i in range(lm.n_layers) for n in LlavaWeights.W8_NAMES] + ["lm_head"]:
        codes, scale = w.w8(name)
        rows = (before[name].shape[0] + 7) // 8 * 8
        assert codes.shape == (rows, before[name].shape[1]) and scale.shape == (rows,)
        assert w.t[name].shape == before[name].shape
        assert torch.equal(ops.w8_dequantize(codes, scale, torch.bfloat16)[:before[name].shape[0]], w.t[name])
        assert not bool(ops.w8_unpack(codes)[before[name].shape[0]:].any())                         # the padding rows are zero codes
    assert torch.equal(w.t["embed"], before["embed"]) and w.w8("embed") is None
    again = {k: v for k, v in w.t.items()}
    w.quantize_lm_w8()
    assert all(w.t[k] is again[k] for k in again)                                                    # a second call changes nothing
