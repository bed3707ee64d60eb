"""load_8bit at 17 - 256 rows: the seven-launch decode layer and its head with the MFMA GEMM reading e4m3 codes (ops.W8_DECODE on) against
the same step on the dequantised 16-bit weights (switch off) over ONE quantised model - bit-identical in every score of every step.  Both legs
are pinned to the GEMM's data-parallel schedule, whose bits do not depend on the macro tile (every output element is accumulated over K in one
fixed order: the GEMM_BATCH_INVARIANT comment in ops.py), so the two tuners may pick different tiles; the projection forms are forced to the
GEMM.  One unpinned run is held to the fp32 reference of its own w16 weights with the tolerance of tests/test_w8_engine_gpu.py."""
import pytest
import torch

from test_engine_shapes_gpu import _compare, _prompts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W7B = dict(d=4096, n_heads=32, n_kv_heads=32, head_dim=128, ffn=11008, vocab=32000)
_engines = {}


def _engine(key, dtype=torch.bfloat16):
    from llava_align_amd.engine import LlavaConfig, LlavaWeights, LMConfig, VddLlavaEngine, VisionConfig, preset
    if (key, dtype) not in _engines:
        if key == "tiny":
            cfg = preset("tiny")
            w = LlavaWeights.random(cfg, DEV, seed=5, std=0.02, lm_head_gain=4.0, dtype=dtype)
        else:
            cfg = LlavaConfig(LMConfig(n_layers=2, max_pos=1024, **W7B), VisionConfig(layers=3), "w8-gemm-test")
            w = LlavaWeights.random(cfg, DEV, seed=5, std=0.02, lm_head_gain=2.0, dtype=dtype)
        _engines[(key, dtype)] = VddLlavaEngine(cfg, weights=w, device=DEV, use_graph=True, load_8bit=True)
    return _engines[(key, dtype)]


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _engines.clear()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _pin(monkeypatch, ops):
    """data-parallel schedule only, fresh choice tables that neither read nor write a persisted file, every projection on the GEMM"""
    monkeypatch.setattr(ops, "GEMM_CANDIDATES", [(c, 1) for c in range(1, 17)])
    monkeypatch.setattr(ops, "_gemm_choice", {})
    monkeypatch.setattr(ops, "_form_choice", {})
    monkeypatch.setattr(ops, "_load_persisted", lambda device: None)
    monkeypatch.setattr(ops, "_persist", {"loaded": None, "path": None, "section": None})
    monkeypatch.setattr(ops, "FORCE_FORM", {"linear": "gemm", "to_norm": "gemm", "swiglu": "gemm",
                                            "linear8": "gemm8", "to_norm8": "gemm8", "swiglu8": "gemm8"})


CASES = [("tiny", torch.bfloat16, 2), ("tiny", torch.bfloat16, 3), ("tiny", torch.float16, 2), ("tiny", torch.float16, 3),
         ("7b", torch.bfloat16, 2), ("7b", torch.bfloat16, 3)]


@pytest.mark.parametrize("key,dtype,nb", CASES, ids=[f"{k}-{str(d)[6:]}-12x{b}" for k, d, b in CASES])
def test_switch_on_equals_switch_off_above_16_rows(monkeypatch, key, dtype, nb):
    from llava_align_amd import ops
    _pin(monkeypatch, ops)
    eng = _engine(key, dtype)
    lm, image = eng.cfg.lm, eng.cfg.vision.image
    assert eng.w.w8("l0.wqkv") is not None and eng.w.w8("l1.wd") is not None and eng.w.w8("lm_head") is not None
    ids, imgs = _prompts(12, 1, lm.vocab, seed=41 + nb, image=image)
    kw = dict(images=imgs, use_dd_unk=True, use_dd=nb == 3, cd_alpha=1.0, cd_beta=0.1, temperature=0.7, max_new_tokens=4, cd_greedy=True,
              output_scores=True)
    n0 = ops.w8_launches()
    a = eng.generate(ids, **kw)
    n1 = ops.w8_launches()
    assert a.stats["n_rows"] == 12 * nb and a.stats["graph"]
    assert n1 >= n0 + 4 * lm.n_layers + 1                       # qkv, o, gate/up, down of every layer and the head (a captured launch counts once)
    # every tuned shape (bucket 0 is the untuned default of the prefill's thousands of rows, the same launch in both legs) took schedule 1
    assert all((cfg >> 4) & 3 == 1 for k, cfg in ops._gemm_choice.items() if k[0] != 0) and any(k[-1] > 8 for k in ops._gemm_choice)
    with ops.w8_decode(False):
        b = eng.generate(ids, **kw)
    assert ops.w8_launches() == n1 and b.stats["graph"]
    assert len(a.scores) == len(b.scores) == 4
    for step, (sa, sb) in enumerate(zip(a.scores, b.scores)):
        assert torch.equal(_bits(sa), _bits(sb)), step
    assert torch.equal(a.tokens, b.tokens)


def test_load_8bit_engine_at_36_rows_matches_the_fp32_reference_of_its_own_weights():
    import copy

    from llava_align_amd import ops
    from ref_llava import RefLlava
    eng = _engine("7b")
    w16 = copy.copy(eng.w)
    w16.t = {k: v for k, v in eng.w.t.items() if not k.endswith((".w8", ".w8s"))}
    ref = RefLlava(w16, device=DEV)
    ids, imgs = _prompts(12, 1, 32000, seed=29)
    n0 = ops.w8_launches()
    # _compare holds every finite score of every step of every question to the tolerance; `checked` counts the steps whose reference margin
    # (top-1 over top-2 by more than twice the tolerance) also made the picked TOKEN comparable - how many there are depends on the random
    # prompts, so the floor only says that the token comparison was not vacuous
    out, checked = _compare(eng, ref, ids, imgs, dict(use_dd_unk=True, use_dd=True), dict(temperature=0.5), n_new=4, questions=range(12), tol=0.5)
    assert out.stats["n_rows"] == 36 and out.stats["graph"] and checked >= 1
    assert ops.w8_launches() >= n0                               # (the tuner takes the codes only where it measured them faster)
