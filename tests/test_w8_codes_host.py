"""Codes-only weights (load_8bit with w8_only) without a GPU: what LlavaWeights.quantize_lm_w8(keep_w16=False) leaves behind and what it
weighs, the ops.CodesWeight handle, which forms the wrappers consider for it (the library calls never reached: `_pick_form` is
stubbed and records its candidates), the tuning-key family, the 8-byte LDS read of the large tiles restated, and the rule for the two
committed choices files (stated here too: their `choices` are untouched, their stamps follow the kernel sources)."""
import json
import os

import pytest
import torch

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llava-align_amd")


def _tiny_weights(dtype=torch.bfloat16, vocab_extra=3):
    """`tiny` language-model weights on the CPU with a vocabulary that is not a multiple of 8 rows."""
    from llava_align_amd.engine import LlavaWeights, preset
    cfg = preset("tiny")
    w = LlavaWeights(cfg, "cpu", dtype)
    g = torch.Generator().manual_seed(5)
    lm = cfg.lm
    for i in range(lm.n_layers):
        for n, shape in (("wqkv", (3 * lm.d, lm.d)), ("wo", (lm.d, lm.d)), ("wgu", (2 * lm.ffn, lm.d)), ("wd", (lm.d, lm.ffn))):
            w.t[f"l{i}.{n}"] = (torch.randn(*shape, generator=g) * 0.02).to(dtype)
        w.t[f"l{i}.ln1"], w.t[f"l{i}.ln2"] = torch.ones(lm.d, dtype=dtype), torch.ones(lm.d, dtype=dtype)
    w.t["lm_head"] = (torch.randn(lm.vocab + vocab_extra, lm.d, generator=g) * 0.02).to(dtype)
    w.t["embed"], w.t["norm"] = w.t["lm_head"].clone(), torch.ones(lm.d, dtype=dtype)
    return w


def _names(w):
    from llava_align_amd.engine import LlavaWeights
    return [f"l{i}.{n}" for i in range(w.cfg.lm.n_layers) for n in LlavaWeights.W8_NAMES] + ["lm_head"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_quantize_lm_w8_codes_only(dtype):
    from llava_align_amd import ops
    w = _tiny_weights(dtype)
    before = {k: v.clone() for k, v in w.t.items()}
    base, stream16 = w.nbytes(), w.lm_stream_bytes()
    w.quantize_lm_w8(keep_w16=False)
    elems = rows = pad = 0
    for name in _names(w):
        cw = w.t[name]
        assert isinstance(cw, ops.CodesWeight) and not torch.is_tensor(cw), name           # no quantised name holds a 16-bit tensor
        N, K = before[name].shape
        Np = (N + 7) // 8 * 8
        assert tuple(cw.shape) == (Np, K) and cw.dtype == dtype and cw.device == torch.device("cpu")
        codes, scale = w.w8(name)
        assert codes is cw.codes and scale is cw.scale                                       # w8(name) returns the pair
        assert name + ".w8" not in w.t and name + ".w8s" not in w.t
        qc, qs, w16 = ops.quantize_w8(torch.nn.functional.pad(before[name], (0, 0, 0, Np - N)))
        assert torch.equal(codes, qc) and torch.equal(scale, qs)
        assert torch.equal(cw.dequantize(), w16)                                             # dequantize() is the w16 of quantize_w8
        elems, rows, pad = elems + N * K, rows + N, pad + (Np - N) * (K + 4)
    assert pad == 5 * (w.cfg.lm.d + 4)                                                       # 1003 rows -> 1008
    # one byte per quantised element less, four bytes per quantised row more, plus lm_head's padding rows (codes + scales): exact
    assert w.nbytes() == base - elems + 4 * rows + pad
    assert w.lm_stream_bytes() == stream16 - 2 * elems + elems + pad - 5 * 4                 # one byte per code, padding included
    for k in ("embed", "norm", "l0.ln1"):
        assert w.t[k] is not None and torch.equal(w.t[k], before[k]) and w.w8(k) is None     # everything else stays 16-bit
    again = dict(w.t)
    w.quantize_lm_w8(keep_w16=False)
    w.quantize_lm_w8()                                                                       # (nor does the w16-keeping call bring tensors back)
    assert set(w.t) == set(again) and all(w.t[k] is again[k] for k in again)                # a second call changes nothing


def test_codes_only_after_w16_kept_and_odd_depths():
    from llava_align_amd import ops
    a, b = _tiny_weights(), _tiny_weights()
    a.quantize_lm_w8()
    kept = {n: a.w8(n) for n in _names(a)}
    a.quantize_lm_w8(keep_w16=False)                  # drops the w16 tensors, keeps the codes it has
    b.quantize_lm_w8(keep_w16=False)
    for n in _names(a):
        assert a.t[n].codes is kept[n][0] and torch.equal(a.t[n].codes, b.t[n].codes) and torch.equal(a.t[n].scale, b.t[n].scale)
    assert a.nbytes() == b.nbytes() and not any(k.endswith((".w8", ".w8s")) for k in a.t)
    # K % 128 != 0: no kernel on codes takes the weight, so it stays a 16-bit tensor, unquantised
    c = _tiny_weights()
    c.t["l1.wd"] = torch.ones(256, 576, dtype=torch.bfloat16) * 0.3
    c.quantize_lm_w8(keep_w16=False)
    assert torch.is_tensor(c.t["l1.wd"]) and bool((c.t["l1.wd"] == 0.3).all()) and c.w8("l1.wd") is None
    assert isinstance(c.t["l1.wo"], ops.CodesWeight)


def test_codes_weight_handle_checks_its_parts():
    from llava_align_amd import ops
    codes, scale = torch.zeros(8, 128, dtype=torch.uint8), torch.ones(8)
    cw = ops.CodesWeight(codes, scale, torch.float16)
    assert tuple(cw.shape) == (8, 128) and cw.shape[0] == 8 and cw.numel() == 1024 and cw.nbytes() == 1024 + 32 and cw.dim() == 2
    cp = cw.clone()
    assert cp.codes is not codes and cp.scale is scale and torch.equal(cp.codes, codes)
    for bad in ((codes.to(torch.int8), scale), (codes, scale.double()), (codes, torch.ones(4)), (torch.zeros(8, 256, dtype=torch.uint8)[:, ::2], scale),
                (torch.zeros(8, 96, dtype=torch.uint8), scale)):
        with pytest.raises(ValueError):
            ops.CodesWeight(bad[0], bad[1], torch.float16)
    with pytest.raises(ValueError):
        ops.CodesWeight(codes, scale, torch.float32)


def test_w8_only_needs_load_8bit():
    from llava_align_amd.engine import VddLlavaEngine
    with pytest.raises(ValueError, match="load_8bit"):
        VddLlavaEngine("tiny", device="cpu", w8_only=True)
    import argparse
    from llava_align_amd import driver_common as D
    a = argparse.Namespace(load_8bit=True, w8_only=True)
    assert D.load_kw(a) == dict(load_8bit=True, w8_only=True) and D.load_kw(argparse.Namespace(load_8bit=True)) == dict(load_8bit=True)
    assert D.load_kw(argparse.Namespace()) == {}


class _Stop(Exception):
    pass


def _candidates(monkeypatch, call):
    """The (kind, candidate names) a wrapper hands to `_pick_form` - stubbed, so no library call is reached."""
    from llava_align_amd import ops
    seen = {}

    def pick(kind, M, N, K, x, w, cands, consumer=None):
        seen.update(kind=kind, names=set(cands), consumer=consumer)
        raise _Stop()
    monkeypatch.setattr(ops, "_pick_form", pick)
    with pytest.raises(_Stop):
        call()
    return seen["kind"], seen["names"]


def test_candidates_of_a_codes_weight_are_codes_forms_only(monkeypatch):
    from llava_align_amd import ops
    dt = torch.bfloat16
    cw = lambda N, K: ops.CodesWeight(torch.zeros(N, K, dtype=torch.uint8), torch.ones(N), dt)
    x = lambda M, K: torch.zeros(M, K, dtype=dt)
    all8 = {"gemm8", "slabs8", "skinny8"}
    # linear: the GEMM on codes at every M; the weight-streaming kernels on codes up to 64 rows where K % 256 == 0
    assert _candidates(monkeypatch, lambda: ops.linear(x(12, 512), cw(256, 512))) == ("linearc", {"gemm8", "skinny8"})
    assert _candidates(monkeypatch, lambda: ops.linear(x(12, 512), cw(256, 512), keep_bits=True)) == ("linearc", {"gemm8", "skinny8"})
    assert _candidates(monkeypatch, lambda: ops.linear(x(64, 512), cw(256, 512)))[1] == {"gemm8", "skinny8"}
    assert _candidates(monkeypatch, lambda: ops.linear(x(65, 512), cw(256, 512)))[1] == {"gemm8"}
    assert _candidates(monkeypatch, lambda: ops.linear(x(5000, 512), cw(256, 512)))[1] == {"gemm8"}              # any M
    assert _candidates(monkeypatch, lambda: ops.linear(x(12, 384), cw(256, 384)))[1] == {"gemm8"}                # K % 256 != 0 drops "skinny8", keeps "gemm8"
    assert _candidates(monkeypatch, lambda: ops.linear(x(12, 512), cw(254, 512)))[1] == {"skinny8"}              # N % 4 != 0: no GEMM
    # swiglu_linear: the SwiGLU epilogue, or the plain GEMM on codes + silu_mul for an odd feature count - both "gemm8"
    assert _candidates(monkeypatch, lambda: ops.swiglu_linear(x(12, 512), cw(512, 512))) == ("swigluc", {"gemm8", "skinny8"})
    assert _candidates(monkeypatch, lambda: ops.swiglu_linear(x(200, 512), cw(2 * 88, 512)))[1] == {"gemm8"}
    assert _candidates(monkeypatch, lambda: ops.swiglu_linear(x(200, 384), cw(512, 384)))[1] == {"gemm8"}
    # linear_to_norm: + the slabs on codes where slab_splits serves the shape
    assert ops.slab_splits(24, 1024, 1024) >= 4
    assert _candidates(monkeypatch, lambda: ops.linear_to_norm(x(24, 1024), cw(1024, 1024))) == ("to_normc", all8)
    assert _candidates(monkeypatch, lambda: ops.linear_to_norm(x(300, 1024), cw(1024, 1024)))[1] == {"gemm8"}
    assert _candidates(monkeypatch, lambda: ops.linear_to_norm(x(24, 384), cw(1024, 384)))[1] == {"gemm8"}
    for names in (all8,):
        assert all(n.endswith("8") for n in names)
    # batch-invariant mode leaves "gemm8" alone
    with ops.batch_invariant():
        assert _candidates(monkeypatch, lambda: ops.linear(x(12, 512), cw(256, 512)))[1] == {"gemm8"}
        assert _candidates(monkeypatch, lambda: ops.swiglu_linear(x(12, 512), cw(512, 512)))[1] == {"gemm8"}
        assert _candidates(monkeypatch, lambda: ops.linear_to_norm(x(24, 1024), cw(1024, 1024)))[1] == {"gemm8"}


def test_pick_codes_form_rules(monkeypatch):
    from llava_align_amd import _lib, ops
    monkeypatch.setattr(ops, "GEMM_AUTOTUNE", False)
    monkeypatch.setattr(ops, "_form_choice", {})
    monkeypatch.setattr(ops, "FORCE_FORM", {})
    x = torch.zeros(12, 512, dtype=torch.bfloat16)
    cw = ops.CodesWeight(torch.zeros(256, 512, dtype=torch.uint8), torch.ones(256), torch.bfloat16)
    f = lambda *a: None
    cands = {"gemm8": f, "slabs8": f, "skinny8": f}
    assert ops._pick_form("to_normc", 12, 256, 512, x, cw, dict(cands)) == "skinny8"        # the tuner off: the shape-generic fallback
    assert ops._pick_form("to_normc", 24, 256, 512, x, cw, dict(cands)) == "gemm8"
    assert ops._pick_form("to_normc", 24, 256, 512, x, cw, {"skinny8": f}) == "skinny8"     # one eligible form: that one
    ops._form_choice[ops._form_key("to_norm8", 24, 256, 512, _lib.VDD_BF16)] = "slabs8"           # a load_8bit=True choice: another kind, not read
    assert ops._pick_form("to_normc", 24, 256, 512, x, cw, dict(cands)) == "gemm8"
    ops._form_choice[ops._form_key("to_normc", 24, 256, 512, _lib.VDD_BF16)] = "slabs8"
    assert ops._pick_form("to_normc", 24, 256, 512, x, cw, dict(cands)) == "slabs8"
    monkeypatch.setattr(ops, "FORCE_FORM", {"to_normc": "skinny8"})
    assert ops._pick_form("to_normc", 24, 256, 512, x, cw, dict(cands)) == "skinny8"
    with ops.batch_invariant():
        assert ops._pick_form("to_normc", 24, 256, 512, x, cw, dict(cands)) == "gemm8"      # one summation order: forced or measured forms do not count
    with pytest.raises(ValueError, match="M=24 N=256 K=512"):
        ops._pick_form("to_normc", 24, 256, 512, x, cw, {})                                # nothing serves the call: the shape is named


def test_w8_decode_off_raises_for_a_codes_weight():
    from llava_align_amd import ops
    dt = torch.bfloat16
    cw = ops.CodesWeight(torch.zeros(512, 512, dtype=torch.uint8), torch.ones(512), dt)
    x, ss, ln = torch.zeros(12, 512, dtype=dt), torch.zeros(12, 32), torch.ones(512, dtype=dt)
    calls = [lambda: ops.gemm(x, cw), lambda: ops.linear(x, cw), lambda: ops.linear_to_norm(x, cw), lambda: ops.swiglu_linear(x, cw),
             lambda: ops.skinny_gemm(x, cw), lambda: ops.gemm_slabs(x, cw, 2), lambda: ops.linear_resid_ss(x, cw, x),
             lambda: ops.linear_normed(x, ss, ln, 1e-5, cw), lambda: ops.swiglu_linear_normed(x, ss, ln, 1e-5, cw)]
    n0 = ops.w8_launches()
    with ops.w8_decode(False):
        for i, call in enumerate(calls):
            with pytest.raises(RuntimeError, match="codes-only"):
                call()
    assert ops.w8_launches() == n0 and ops.W8_DECODE is True


def test_fused_layer_answers_plain_where_a_launch_on_codes_would_be_refused():
    from llava_align_amd import ops
    saved = dict(ops._form_choice)
    try:
        ops._form_choice.clear()
        dt = ops._MODEL_DT[torch.bfloat16]
        assert ops.norm_fused_pays(4, 4096, w8=True, codes_only_ks=(4096, 4096, 11008))           # every depth a multiple of 256: the generic rule
        assert not ops.norm_fused_pays(4, 4096, w8=True, codes_only_ks=(4096, 4096, 11008 + 128))   # one fused launch would be refused: plain
        ops._form_choice[("layer", 12, 4096, 8, dt)] = "fused"                                     # the load_8bit=True record is not this mode's
        assert not ops.norm_fused_pays(12, 4096, w8=True, codes_only_ks=(4096, 4096, 11008))
        ops._form_choice[("layer", 12, 4096, 16, dt)] = "fused"
        assert ops.norm_fused_pays(12, 4096, w8=True, codes_only_ks=(4096, 4096, 11008)) and not ops.norm_fused_pays(12, 4096)
        with ops.w8_decode(False):
            assert not ops.norm_fused_pays(4, 4096, w8=False, codes_only_ks=(4096, 4096, 11008))
    finally:
        ops._form_choice.clear()
        ops._form_choice.update(saved)


def test_codes_keys_are_a_family_of_their_own():
    from llava_align_amd import _lib, ops
    gemm = json.load(open(os.path.join(PKG, "gemm_choices_mi355x.json")))["choices"]
    form = json.load(open(os.path.join(PKG, "form_choices_mi355x.json")))["choices"]
    dts = {int(k.split(",")[5]) for k in gemm}
    kinds = ["linearc", "to_normc", "swigluc"]
    assert [k + ops.CODES_KIND_SUFFIX for k in ("linear", "to_norm", "swiglu")] == kinds
    assert not {k.split(",")[1] for k in form} & set(kinds)
    assert [(c, s) for (c, s) in ops.GEMM_CANDIDATES if c in ops.W8_CODES_TILES] == [(c, s) for c in range(1, 17) if c != 5 for s in (0, 1, 2)]
    assert tuple(ops.W8_GEMM_TILES) == tuple(range(7, 17)) and ops.W8_GEMM_MAX_M == 256        # (unchanged)
    for dt in (_lib.VDD_BF16, _lib.VDD_F16):
        for M in (2, 36, 256, 1536, 5000):
            for N, K, epi in ((12288, 4096, 0), (11008, 4096, 4), (4096, 11008, 0), (32000, 4096, 0)):
                kc, k8, k16 = ops._gemm_key_codes(M, N, K, epi, dt), ops._gemm_key_w8(M, N, K, epi, dt), ops._gemm_key(M, N, K, epi, dt)
                assert kc[:-1] == k16[:-1] and kc[-1] == dt + 16 and len({kc, k8, k16}) == 3 and kc[-1] not in dts
                assert ",".join(map(str, kc)) not in gemm
                before = dict(ops._gemm_choice)
                try:
                    ops._gemm_choice.clear()
                    ops.gemm_choices_import(json.loads(json.dumps({",".join(map(str, kc)): 17})))      # survives the cache file's text form
                    assert ops._gemm_choice == {kc: 17}
                finally:
                    ops._gemm_choice.clear()
                    ops._gemm_choice.update(before)


def test_committed_choices_are_untouched_and_stamped_to_the_sources():
    """The rule of tests/test_w8_gemm.py, for a reader of this file: a kernel change that leaves the 16-bit instantiations instruction for
    instruction what they were re-stamps the two files and leaves their `choices` as measured; codes-only choices are never committed."""
    from llava_align_amd import ops
    from test_w8_gemm import FORM_CHOICES_SHA, GEMM_CHOICES_SHA, _digest
    g = json.load(open(os.path.join(PKG, "gemm_choices_mi355x.json")))
    f = json.load(open(os.path.join(PKG, "form_choices_mi355x.json")))
    assert _digest(g["choices"]) == GEMM_CHOICES_SHA and _digest(f["choices"]) == FORM_CHOICES_SHA
    assert g["gemm_source_sha"] == ops.gemm_source_fingerprint() and f["kernel_source_sha"] == ops.kernel_source_fingerprint()


def test_eight_byte_code_reads_restated():
    """The 8-bit form of the 256 x 256, 192 x 256 and 192 x 192 tiles reads 8 bytes of codes per k-step (csrc/vdd_gemm.hip, W8_READ8): lane
    (r, h) at k-step kk reads row * 64 + ((h ^ ((r >> 2) & 3)) * 16 ^ ((kk & 1) << 5)) + 8 (kk >> 1) of the K-tile image that
    tests/test_w8_gemm.py restates.  On a row packed by ops.w8_pack those 8 bytes must be elements 16 kk + 8 h .. + 7 of the K-tile: what
    the 16-byte read of the other tiles yields in two halves, and what the 16-bit fragment holds."""
    from llava_align_amd import ops
    rows = 32
    k = torch.arange(64, dtype=torch.int64)
    codes = (k[None, :] + 64 * torch.arange(rows)[:, None]) % 251
    packed = ops.w8_pack(codes.to(torch.uint8)).to(torch.int64)
    lds = torch.full((rows * 64,), -1, dtype=torch.int64)
    for img in range(rows // 16):
        for lane in range(64):
            row = img * 16 + (lane >> 2)
            c = (lane & 3) ^ ((row >> 2) & 3)
            lds[img * 1024 + lane * 16: img * 1024 + lane * 16 + 16] = packed[row, c * 16: c * 16 + 16]
    for kk in range(4):
        for h in (0, 1):
            for r in range(rows):
                addr = ((r * 64 + ((h ^ ((r >> 2) & 3)) * 16)) ^ ((kk & 1) << 5)) + (kk >> 1) * 8
                assert lds[addr: addr + 8].tolist() == codes[r, 16 * kk + 8 * h: 16 * kk + 8 * h + 8].tolist(), (kk, h, r)
                assert r * 64 <= addr and addr + 8 <= (r + 1) * 64                            # inside the row's 64 bytes
