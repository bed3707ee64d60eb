"""The 8-bit weight-streaming entries' host side, without a GPU: both C entries are declared, bound and exported; the ops wrappers take `w8=`
and reject a pair that does not belong to the weight; and the keys under which the batch-invariant mode keeps its choices on codes - form
kinds of its own, GEMM keys that carry the mode flag - meet no entry of the two in-tree choice files and survive the cache file's text form."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llava-align_amd")

ENTRIES = {"vdd_skinny_gemm_w8": (11, ["X", "W8", "w_scale", "Y", "M", "N", "K", "ldx", "ldy"]),
           "vdd_skinny_swiglu_w8": (10, ["X", "W8_gate_up", "w_scale", "act", "M", "F", "K", "ldx"])}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entries_are_declared_bound_and_exported(name):
    from llava_align_amd import _lib, ops
    n_params, names = ENTRIES[name]
    hdr = open(os.path.join(ROOT, "include", "vdd_hip.h")).read()
    m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
    assert m, f"include/vdd_hip.h does not declare {name}"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == n_params and params[-2] == "int dtype" and params[-1] == "void* hip_stream"
    assert [p.split()[-1].lstrip("*") for p in params[:-2]] == names
    sig = ops._SIGS[name]
    assert len(sig) == n_params
    for p, c in zip(params, sig):
        want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int
        assert c is want, (p, c)
    assert hasattr(ctypes.CDLL(_lib.lib_path()), name)
    assert "#define VDD_ABI_VERSION 3" in hdr and _lib.ABI_VERSION == 3
    # beside the other 8-bit entries, under "8-bit weight rows"
    assert hdr.index("8-bit weight rows (load_8bit)") < hdr.index("int %s(" % name) < hdr.index("int vdd_gemm_w8(")


def test_wrappers_accept_w8_and_reject_a_malformed_pair():
    from llava_align_amd import ops
    for fn in (ops.skinny_gemm, ops._skinny_swiglu):
        assert inspect.signature(fn).parameters["w8"].default is None, fn.__name__
    x = torch.zeros(17, 256, dtype=torch.bfloat16)
    w = torch.zeros(256, 256, dtype=torch.bfloat16)
    bad = [(torch.zeros(256, 256, dtype=torch.int8), torch.ones(256)),             # codes are uint8
           (torch.zeros(128, 256, dtype=torch.uint8), torch.ones(128)),            # another weight's pair
           (torch.zeros(256, 256, dtype=torch.uint8), torch.ones(256, dtype=torch.float64)),
           (torch.zeros(256, 512, dtype=torch.uint8)[:, ::2], torch.ones(256))]    # rows not contiguous
    for pair in bad:
        for fn in (ops.skinny_gemm, ops._skinny_swiglu):
            with pytest.raises(ValueError, match="w8 = "):
                fn(x, w, w8=pair)
    # an odd feature count takes no GEMM on codes, and the pair is still checked
    with pytest.raises(ValueError, match="w8 = "):
        ops.swiglu_linear(x, torch.zeros(80, 256, dtype=torch.bfloat16), w8=bad[1])


def test_which_8bit_forms_are_candidates():
    """The shape rules of the two helpers, restated: the GEMM on codes up to W8_GEMM_MAX_M rows in either mode, the weight-streaming
    kernels on codes where the 16-bit ones serve and K % 256 == 0 - never in batch-invariant mode."""
    from llava_align_amd import ops
    w = torch.zeros(256, 512, dtype=torch.bfloat16)
    q = (torch.zeros(256, 512, dtype=torch.uint8), torch.ones(256))
    w384 = torch.zeros(256, 384, dtype=torch.bfloat16)
    q384 = (torch.zeros(256, 384, dtype=torch.uint8), torch.ones(256))
    assert ops._w8_skinny_args(w, q, 12, 512) is not None and ops._w8_skinny_args(w, q, 64, 512) is not None
    assert ops._w8_skinny_args(w, q, 65, 512) is None and ops._w8_skinny_args(w384, q384, 12, 384) is None
    assert ops._w8_form_args(w, q, 256, 512, 256) is not None and ops._w8_form_args(w, q, 257, 512, 256) is None
    with ops.w8_decode(False):
        assert ops._w8_skinny_args(w, q, 12, 512) is None and ops._w8_form_args(w, q, 24, 512, 256) is None
    with ops.batch_invariant():
        assert ops._w8_skinny_args(w, q, 12, 512) is None
        assert ops._w8_form_args(w, q, 24, 512, 256) is not None
    assert ops._w8_skinny_args(w, None, 12, 512) is None


def test_invariant_mode_picks_between_gemm_and_gemm8_only(monkeypatch):
    """`_pick_form` in batch-invariant mode, the tuner off (no measurement possible): without codes the GEMM at once; with codes the 16-bit
    rule unless the mode's own kind is forced or holds a choice; "skinny8" / "slabs8" / a tuned-mode choice are never taken."""
    from llava_align_amd import _lib, ops
    monkeypatch.setattr(ops, "GEMM_AUTOTUNE", False)
    monkeypatch.setattr(ops, "_form_choice", {})
    monkeypatch.setattr(ops, "FORCE_FORM", {})
    x = torch.zeros(24, 512, dtype=torch.bfloat16)
    w = torch.zeros(256, 512, dtype=torch.bfloat16)
    f = lambda *a: None
    cands = {"skinny": f, "gemm": f, "slabs": f, "gemm8": f, "slabs8": f, "skinny8": f}
    dt = _lib.VDD_BF16
    with ops.batch_invariant():
        assert ops._pick_form("to_norm", 24, 256, 512, x, w, {"skinny": f, "gemm": f, "slabs": f}) == "gemm"
        assert ops._pick_form("to_norm8", 24, 256, 512, x, w, dict(cands)) == "gemm"
        ops._form_choice[ops._form_key("to_norm8", 24, 256, 512, dt)] = "skinny8"          # a tuned-mode choice: not read
        assert ops._pick_form("to_norm8", 24, 256, 512, x, w, dict(cands)) == "gemm"
        ops._form_choice[ops._form_key("to_norm8" + ops.INVARIANT_KIND_SUFFIX, 24, 256, 512, dt)] = "gemm8"
        assert ops._pick_form("to_norm8", 24, 256, 512, x, w, dict(cands)) == "gemm8"
        ops._form_choice.clear()
        for forced in ("skinny8", "slabs8", "skinny"):
            monkeypatch.setattr(ops, "FORCE_FORM", {"to_norm8": forced, "to_norm8" + ops.INVARIANT_KIND_SUFFIX: forced})
            assert ops._pick_form("to_norm8", 24, 256, 512, x, w, dict(cands)) == "gemm"
        monkeypatch.setattr(ops, "FORCE_FORM", {"to_norm8" + ops.INVARIANT_KIND_SUFFIX: "gemm8"})
        assert ops._pick_form("to_norm8", 24, 256, 512, x, w, dict(cands)) == "gemm8"
    assert ops._pick_form("to_norm8", 24, 256, 512, x, w, dict(cands)) == "gemm"           # tuned mode, tuner off, 24 rows: the fallback


def test_invariant_keys_are_disjoint_from_the_committed_choices_and_survive_the_cache_file():
    from llava_align_amd import _lib, ops
    gemm = json.load(open(os.path.join(PKG, "gemm_choices_mi355x.json")))["choices"]
    form = json.load(open(os.path.join(PKG, "form_choices_mi355x.json")))["choices"]
    assert gemm and form
    kinds_i = [k + ops.INVARIANT_KIND_SUFFIX for k in ("linear8", "to_norm8", "swiglu8")]
    assert kinds_i == ["linear8i", "to_norm8i", "swiglu8i"]
    assert not {k.split(",")[1] for k in form} & (set(kinds_i) | {"linear8", "to_norm8", "swiglu8", "linear8t"})
    assert "skinny8" not in form.values()
    dts = {int(k.split(",")[5]) for k in gemm}
    for dt in (_lib.VDD_BF16, _lib.VDD_F16):
        for M in (2, 12, 24, 36, 64, 128, 256):
            for N, K, epi in ((12288, 4096, 0), (4096, 4096, 0), (11008, 4096, 4), (4096, 11008, 0), (32000, 4096, 0)):
                tuned = ops._gemm_key_w8(M, N, K, epi, dt)
                with ops.batch_invariant():
                    k8 = ops._gemm_key_w8(M, N, K, epi, dt)
                    k16 = ops._gemm_key(M, N, K, epi, dt)
                # the mode flag separates the key from the tuned-mode key on codes, the storage-type slot from every 16-bit key
                assert k8[4] is True and tuned[4] is False and k8[:4] == tuned[:4] and k8[-1] == tuned[-1] == dt + 8
                assert k8 != k16 and k8[-1] not in dts and ",".join(map(str, k8)) not in gemm
                fkeys = [ops._form_key(kind, M, N, K, dt) for kind in kinds_i]
                assert all("form," + ",".join(map(str, fk)) not in form for fk in fkeys)
                # ... and the keys survive the cache file's text form
                before_g, before_f = dict(ops._gemm_choice), dict(ops._form_choice)
                try:
                    ops._gemm_choice.clear()
                    ops._form_choice.clear()
                    ops.gemm_choices_import(json.loads(json.dumps({",".join(map(str, k8)): 24, **{"form," + ",".join(map(str, fk)): "gemm8" for fk in fkeys}})))
                    assert ops._gemm_choice == {k8: 24}
                    assert ops._form_choice == {fk: "gemm8" for fk in fkeys}
                    assert ops.gemm_choices_export() == {",".join(map(str, k8)): 24, **{"form," + ",".join(map(str, fk)): "gemm8" for fk in fkeys}}
                finally:
                    ops._gemm_choice.clear()
                    ops._gemm_choice.update(before_g)
                    ops._form_choice.clear()
                    ops._form_choice.update(before_f)


def test_rowsw8_stages_restated_feed_the_16bit_fragments_and_read_every_code_once():
    """RowsW8 of csrc/vdd_llm_kernels.hip restated for the wave slices the new entries use - four waves (slices start on a group of 64)
    with stages of U = 2, 4, 8 k-steps plus the remainder batch's single k-steps, and eight waves with an odd slice (K / 256 odd: every
    second wave starts in the middle of a group) - on a row packed by ops.w8_pack: k-step t of lane group g must hold elements
    kbeg + 32 t + 8 g .. + 7 of the row, what Rows16 loads there, and the slice's bytes are each read exactly once."""
    from llava_align_amd import ops

    def ld(p, odd, kk, U):                               # RowsW8::ld: U k-steps of 8 bytes for one lane
        q = p + kk
        if not odd:
            out = []
            for j in range(U // 2):
                out += [(q + 64 * j, 8), (q + 64 * j + 8, 8)]
            return out
        out = [(q + 8, 8)]
        for j in range(1, U // 2):
            out += [(q + 64 * j, 8), (q + 64 * j + 8, 8)]
        return out + [(q + 64 * (U // 2), 8)]

    def ld1(p, odd, k):                                       # RowsW8::ld1
        t = (k >> 5) + odd
        return (p + (t >> 1) * 64 + (t & 1) * 8, 8)

    for K, NW, U in ((256, 4, 2), (256, 4, 4), (768, 4, 4), (2816, 4, 2), (2816, 4, 4), (2816, 4, 8), (11008, 4, 4), (2816, 8, 8), (11008, 8, 8)):
        elems = torch.arange(K, dtype=torch.int64)
        packed = ops.w8_pack((elems % 251).to(torch.uint8)[None, :])[0].to(torch.int64)
        kq = K // NW
        read = torch.zeros(K, dtype=torch.int32)
        for wave in range(NW):
            kbeg = wave * kq
            for g in range(4):
                p, odd = (kbeg & ~63) + g * 16, (kbeg >> 5) & 1
                nit = kq // (32 * U)
                steps = []                                     # (byte offset, length) of k-step t = index
                for it in range(nit):
                    steps += ld(p, odd, it * 32 * U, U)
                for k in range(nit * 32 * U, kq, 32):
                    steps.append(ld1(p, odd, k))
                assert len(steps) == kq // 32, (K, NW, U)
                for t, (off, n) in enumerate(steps):
                    k0 = kbeg + 32 * t + 8 * g
                    assert packed[off: off + n].tolist() == (elems[k0: k0 + 8] % 251).tolist(), (K, NW, U, wave, g, t)
                    read[off: off + n] += 1
        assert bool((read == 1).all()), (K, NW, U)
