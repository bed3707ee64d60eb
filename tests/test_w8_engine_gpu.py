"""load_8bit through the engine: the few-row decode step streaming e4m3 codes against the same step streaming the dequantised 16-bit weights
(ops.W8_DECODE on / off over ONE quantised model) is bit-identical in every score of every step; the quantised engine against the fp32
reference built from its own w16 weights passes the tolerances of test_engine_shapes_gpu.py (it is just an engine with other weights); and the
public surface (VddLlavaEngine / checkpoint.load_llava `load_8bit`, `load_4bit`)."""
import pytest
import torch

from test_engine_shapes_gpu import _compare, _prompts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W7B = dict(d=4096, n_heads=32, n_kv_heads=32, head_dim=128, ffn=11008, vocab=32000)
W13B = dict(d=5120, n_heads=40, n_kv_heads=40, head_dim=128, ffn=13824, vocab=32000)
_engines = {}


def _engine(key, dtype=torch.bfloat16):
    """One load_8bit engine per shape for the whole module (2 decoder layers at the real widths, as test_engine_shapes_gpu.py builds them)."""
    from llava_align_amd.engine import LlavaConfig, LlavaWeights, LMConfig, VddLlavaEngine, VisionConfig, preset
    if (key, dtype) not in _engines:
        if key == "tiny":
            cfg = preset("tiny")
            w = LlavaWeights.random(cfg, DEV, seed=5, std=0.02, lm_head_gain=4.0, dtype=dtype)
        else:
            cfg = LlavaConfig(LMConfig(n_layers=2, max_pos=1024, **(W7B if key == "7b" else W13B)), VisionConfig(layers=3), "w8-test")
            w = LlavaWeights.random(cfg, DEV, seed=5, std=0.02, lm_head_gain=2.0, dtype=dtype)
        _engines[(key, dtype)] = VddLlavaEngine(cfg, weights=w, device=DEV, use_graph=True, load_8bit=True)
    return _engines[(key, dtype)]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


CASES = [("tiny", torch.bfloat16, 1, 2), ("tiny", torch.bfloat16, 8, 2), ("tiny", torch.bfloat16, 3, 3),
         ("tiny", torch.float16, 1, 2), ("tiny", torch.float16, 8, 2), ("tiny", torch.float16, 3, 3),
         ("7b", torch.bfloat16, 1, 2), ("7b", torch.bfloat16, 5, 2), ("13b", torch.bfloat16, 1, 3)]


@pytest.mark.parametrize("key,dtype,n_q,nb", CASES, ids=[f"{k}-{str(d)[6:]}-{q}x{b}" for k, d, q, b in CASES])
def test_switch_on_equals_switch_off(monkeypatch, key, dtype, n_q, nb):
    from llava_align_amd import ops
    monkeypatch.setattr(ops, "FORCE_LAYER_FORM", "fused")
    eng = _engine(key, dtype)
    lm, image = eng.cfg.lm, eng.cfg.vision.image
    assert eng.w.w8("l0.wqkv") is not None and eng.w.w8("l1.wd") is not None and eng.w.w8("lm_head") is not None
    ids, imgs = _prompts(n_q, 1, lm.vocab, seed=31 + n_q, image=image)
    kw = dict(images=imgs, use_dd_unk=True, use_dd=nb == 3, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, max_new_tokens=5, cd_greedy=True,
              output_scores=True)
    n0 = ops.w8_launches()
    a = eng.generate(ids, **kw)
    n1 = ops.w8_launches()
    assert a.stats["n_rows"] == n_q * nb and a.stats["graph"]
    assert n1 > n0                                             # the 8-bit kernels really ran (a captured launch counts once)
    with ops.w8_decode(False):
        b = eng.generate(ids, **kw)
    assert ops.w8_launches() == n1 and b.stats["graph"]        # ... and with the switch off none did
    assert len(a.scores) == len(b.scores) == 5
    for step, (sa, sb) in enumerate(zip(a.scores, b.scores)):
        assert torch.equal(_bits(sa), _bits(sb)), step
    assert torch.equal(a.tokens, b.tokens)


def test_load_8bit_engine_matches_the_fp32_reference_of_its_own_weights():
    from ref_llava import RefLlava
    eng = _engine("7b")
    import copy
    w16 = copy.copy(eng.w)
    w16.t = {k: v for k, v in eng.w.t.items() if not k.endswith((".w8", ".w8s"))}
    ref = RefLlava(w16, device=DEV)                            # fp32 model of w16
    ids, imgs = _prompts(6, 1, 32000, seed=23)
    out, checked = _compare(eng, ref, ids, imgs, dict(use_dd_unk=True), dict(temperature=0.5), n_new=4, questions=range(6), tol=0.5)
    assert out.stats["n_rows"] == 12 and checked >= 6


def test_surface(tmp_path):
    from llava_align_amd import checkpoint as K
    from llava_align_amd.engine import LlavaWeights, VddLlavaEngine
    from tiny_checkpoint import write_checkpoint
    info = write_checkpoint(str(tmp_path))
    with pytest.raises(NotImplementedError):
        K.load_llava(info["ckpt"], DEV, load_4bit=True)
    with pytest.raises(NotImplementedError):
        VddLlavaEngine("tiny", device=DEV, load_4bit=True)
    eng_a, tok, _proc = K.load_llava(info["ckpt"], DEV, load_8bit=True)
    cfg, sd = K.config_from_dir(info["ckpt"]), K.load_state_dict(info["ckpt"])
    eng_b = VddLlavaEngine(cfg, weights=LlavaWeights.from_state_dict(cfg, sd, DEV, dtype=torch.float16), device=DEV, load_8bit=True)
    eng_c = VddLlavaEngine(cfg, weights=LlavaWeights.from_state_dict(cfg, sd, DEV, dtype=torch.float16), device=DEV)
    assert any(k.endswith(".w8") for k in eng_a.w.t) and any(k.endswith(".w8") for k in eng_b.w.t)
    assert not any(k.endswith((".w8", ".w8s")) for k in eng_c.w.t)             # load_8bit=False: no codes anywhere
    ids, imgs = _prompts(2, 1, cfg.lm.vocab, seed=9, image=cfg.vision.image)
    kw = dict(images=imgs, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, max_new_tokens=6, cd_greedy=True)
    assert torch.equal(eng_a.generate(ids, **kw).tokens, eng_b.generate(ids, **kw).tokens)
