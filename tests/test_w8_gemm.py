"""The 8-bit GEMM's host side, without a GPU: the C entry is declared, bound and exported; the ops wrappers take `w8=` and reject a pair
that does not belong to the weight; the 8-bit tuning and form keys can never meet a 16-bit entry of the two in-tree choice files; and
those files' measured choices are what they were."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llava-align_amd")


def test_entry_is_declared_bound_and_exported():
    from llava_align_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "vdd_hip.h")).read()
    m = re.search(r"int vdd_gemm_w8\(([^;]*)\);", hdr)
    assert m, "include/vdd_hip.h does not declare vdd_gemm_w8"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 16 and params[-2] == "int dtype" and params[-1] == "void* hip_stream"
    assert [p.split()[-1].lstrip("*") for p in params[:5]] == ["X", "W8", "w_scale", "Y", "bias"]
    sig = ops._SIGS["vdd_gemm_w8"]
    assert len(sig) == 16
    for p, c in zip(params, sig):
        want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int
        assert c is want, (p, c)
    lib = ctypes.CDLL(_lib.lib_path())
    assert hasattr(lib, "vdd_gemm_w8")
    assert "ABI_VERSION 3" in hdr.replace("VDD_ABI_VERSION", "ABI_VERSION") or _lib.ABI_VERSION == 3


def test_wrappers_accept_w8_and_reject_a_malformed_pair():
    from llava_align_amd import ops
    for fn in (ops.gemm, ops.gemm_slabs, ops.linear, ops.linear_to_norm, ops.swiglu_linear):
        assert inspect.signature(fn).parameters["w8"].default is None, fn.__name__
    assert ops.W8_DECODE
    x = torch.zeros(17, 256, dtype=torch.bfloat16)
    w = torch.zeros(256, 256, dtype=torch.bfloat16)
    bad = [(torch.zeros(256, 256, dtype=torch.int8), torch.ones(256)),             # codes are uint8
           (torch.zeros(128, 256, dtype=torch.uint8), torch.ones(128)),            # another weight's pair
           (torch.zeros(256, 256, dtype=torch.uint8), torch.ones(256, dtype=torch.float64)),
           (torch.zeros(256, 512, dtype=torch.uint8)[:, ::2], torch.ones(256))]    # rows not contiguous
    for pair in bad:
        for fn in (ops.gemm, ops.linear, ops.linear_to_norm, ops.swiglu_linear):
            with pytest.raises(ValueError, match="w8 = "):
                fn(x, w, w8=pair)


def test_8bit_keys_are_disjoint_from_the_committed_choices():
    from llava_align_amd import _lib, ops
    gemm = json.load(open(os.path.join(PKG, "gemm_choices_mi355x.json")))["choices"]
    form = json.load(open(os.path.join(PKG, "form_choices_mi355x.json")))["choices"]
    assert gemm and form
    dts = {int(k.split(",")[5]) for k in gemm}
    assert dts <= {_lib.VDD_BF16, _lib.VDD_F16}
    kinds = {k.split(",")[1] for k in form}
    assert not kinds & {"linear8", "to_norm8", "swiglu8"}
    for dt in (_lib.VDD_BF16, _lib.VDD_F16):
        for M in (17, 24, 36, 64, 128, 256):
            for N, K, epi in ((12288, 4096, 0), (4096, 4096, 0), (11008, 4096, 4), (4096, 11008, 0), (32000, 4096, 0), (15360, 5120, 1)):
                k8 = ops._gemm_key_w8(M, N, K, epi, dt)
                assert k8[-1] not in dts and k8[:-1] == ops._gemm_key(M, N, K, epi, dt)[:-1]
                assert ",".join(map(str, k8)) not in gemm
                # ... and the key survives the cache file's text form
                before = dict(ops._gemm_choice)
                try:
                    ops._gemm_choice.clear()
                    ops.gemm_choices_import({",".join(map(str, k8)): 29})
                    assert ops._gemm_choice == {k8: 29}
                finally:
                    ops._gemm_choice.clear()
                    ops._gemm_choice.update(before)
                for kind in ("linear8", "to_norm8", "swiglu8"):
                    assert "form," + ",".join(map(str, ops._form_key(kind, M, N, K, dt))) not in form
    assert [(c, s) for (c, s) in ops.GEMM_CANDIDATES if c in ops.W8_GEMM_TILES] == [(c, s) for c in range(7, 17) for s in (0, 1, 2)]


# sha256 (first 16 hex digits) of json.dumps(choices, sort_keys=True, separators=(",", ":")) of the two files as they were measured
GEMM_CHOICES_SHA = "dc6d75b4d56da61e"
FORM_CHOICES_SHA = "6a8ac310cf55f80e"


def _digest(choices):
    import hashlib
    return hashlib.sha256(json.dumps(choices, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:16]


def test_committed_choices_are_unchanged_apart_from_the_source_hash():
    """The measured choices of both files are re-stamped to the new kernel source, not re-measured: their `choices` hash to the digest
    taken before vdd_gemm_w8 existed, and the stamps are the current sources' fingerprints."""
    from llava_align_amd import ops
    g = json.load(open(os.path.join(PKG, "gemm_choices_mi355x.json")))
    f = json.load(open(os.path.join(PKG, "form_choices_mi355x.json")))
    assert _digest(g["choices"]) == GEMM_CHOICES_SHA
    assert _digest(f["choices"]) == FORM_CHOICES_SHA
    assert g["gemm_source_sha"] == ops.gemm_source_fingerprint()
    assert f["kernel_source_sha"] == ops.kernel_source_fingerprint()


def test_code_image_restated_keeps_the_mfma_slot_map_and_has_no_bank_conflict():
    """The K-tile image of codes in LDS, restated from csrc/vdd_gemm.hip (W8 form): LDS-DMA lane l of a 1-KiB image writes byte 16 l (row
    l >> 2, physical chunk l & 3) and fetches the logical chunk (l & 3) ^ ((row >> 2) & 3) of that row's 64 bytes; lane (r, h) reads 16
    bytes at row * 64 + ((h ^ ((r >> 2) & 3)) * 16 ^ ((kk & 1) << 5)) at k-steps 0 and 1.  On a row packed by ops.w8_pack that read must
    hold element 16 kk + 8 h + j of the K-tile in byte j (k-step kk) and element 16 (kk + 2) + 8 h + j in byte 8 + j; and the 16 lanes
    of a ds_read_b128 group (16 consecutive rows, one half) must cover 16 distinct 16-byte bank slots of the 256-byte bank window."""
    from llava_align_amd import ops
    rows = 32
    k = torch.arange(64, dtype=torch.int64)
    codes = (k[None, :] + 64 * torch.arange(rows)[:, None]) % 251              # element k of row n: a value that names (n, k)
    packed = ops.w8_pack(codes.to(torch.uint8)).to(torch.int64)
    lds = torch.full((rows * 64,), -1, dtype=torch.int64)
    for img in range(rows // 16):
        for lane in range(64):
            row = img * 16 + (lane >> 2)
            c = (lane & 3) ^ ((row >> 2) & 3)
            lds[img * 1024 + lane * 16: img * 1024 + lane * 16 + 16] = packed[row, c * 16: c * 16 + 16]
    assert int(lds.min()) >= 0
    for kk in (0, 1):
        for h in (0, 1):
            for base in (0, 16):
                slots = set()
                for r in range(base, base + 16):
                    addr = (r * 64 + ((h ^ ((r >> 2) & 3)) * 16)) ^ ((kk & 1) << 5)
                    got = lds[addr: addr + 16]
                    assert got[:8].tolist() == codes[r, 16 * kk + 8 * h: 16 * kk + 8 * h + 8].tolist(), (kk, h, r)
                    assert got[8:].tolist() == codes[r, 16 * (kk + 2) + 8 * h: 16 * (kk + 2) + 8 * h + 8].tolist(), (kk, h, r)
                    slots.add((addr % 256) // 16)
                assert len(slots) == 16, (kk, h, base)
