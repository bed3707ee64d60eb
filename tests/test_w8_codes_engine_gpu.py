"""load_8bit with w8_only through the engine: the quantised language-model weights exist as e4m3 codes only (ops.CodesWeight), and prefill,
decode, batch-invariant mode and generate_list run on the kernels that read codes.

A `w8_only` engine and a `load_8bit=True` engine over the same seed hold the same model (w16 = code * scale), and wherever the summation
order is fixed they must return the same BITS: in batch-invariant mode (every projection is the GEMM's data-parallel schedule, whose bits do
not depend on the tile) and in tuned mode with one form, tile and schedule pinned for every projection of both engines.  Step 0 of a
generate() call comes from the prefill, so the equalities pin the prefill GEMMs on codes as well.  Left to its own measured forms the
`w8_only` engine is just an engine with other weights: it meets the fp32 reference of its dequantised weights under the tolerance the
`load_8bit` test uses."""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch

from test_engine_shapes_gpu import _compare, _prompts
from test_w8_engine_gpu import CASES, W7B, W13B, _bits
from test_w8_engine_gpu import _engine as _w16_kept_engine          # the load_8bit=True engines: same seeds, same shapes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("linear", "to_norm", "swiglu")
_engines = {}


def _engine(key, dtype=torch.bfloat16):
    """One w8_only engine per shape for the whole module, over the weights test_w8_engine_gpu._engine draws (seed 5)."""
    from llava_align_amd.engine import LlavaConfig, LlavaWeights, LMConfig, VddLlavaEngine, VisionConfig, preset
    if (key, dtype) not in _engines:
        if key == "tiny":
            cfg = preset("tiny")
            w = LlavaWeights.random(cfg, DEV, seed=5, std=0.02, lm_head_gain=4.0, dtype=dtype)
        else:
            cfg = LlavaConfig(LMConfig(n_layers=2, max_pos=1024, **(W7B if key == "7b" else W13B)), VisionConfig(layers=3), "w8-test")
            w = LlavaWeights.random(cfg, DEV, seed=5, std=0.02, lm_head_gain=2.0, dtype=dtype)
        _engines[(key, dtype)] = VddLlavaEngine(cfg, weights=w, device=DEV, use_graph=True, load_8bit=True, w8_only=True)
    return _engines[(key, dtype)]


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _engines.clear()


class _Pinned(dict):
    """A GEMM choice table that answers every key of the given families with one config."""

    def __init__(self, cfg, families):
        super().__init__()
        self.cfg, self.families = cfg, families

    def get(self, key, default=None):
        return self.cfg if self.families(key) else super().get(key, default)


def _quiet_tables(monkeypatch, ops, gemm_choice, force=()):
    monkeypatch.setattr(ops, "_gemm_choice", gemm_choice)
    monkeypatch.setattr(ops, "_form_choice", {})
    monkeypatch.setattr(ops, "_load_persisted", lambda device: None)
    monkeypatch.setattr(ops, "_persist", {"loaded": None, "path": None, "section": None})
    monkeypatch.setattr(ops, "FORCE_FORM", dict(force))


def _lm_names(eng):
    from llava_align_amd.engine import LlavaWeights
    return [f"l{i}.{n}" for i in range(eng.cfg.lm.n_layers) for n in LlavaWeights.W8_NAMES] + ["lm_head"]


def _same(a, b, n_steps):
    assert len(a.scores) == len(b.scores) == n_steps
    for step, (sa, sb) in enumerate(zip(a.scores, b.scores)):
        assert torch.equal(_bits(sa), _bits(sb)), step
    assert torch.equal(a.tokens, b.tokens)


@pytest.mark.parametrize("key,dtype,n_q,nb", CASES, ids=[f"{k}-{str(d)[6:]}-{q}x{b}" for k, d, q, b in CASES])
def test_batch_invariant_bits_equal_the_load_8bit_engine(monkeypatch, key, dtype, n_q, nb):
    """The tuner is off (a timing run per shape is not what this test is about) and the GEMM on codes is pinned to another compute-bound tile
    per case: in this mode the bits may not depend on it."""
    from llava_align_amd import ops
    tile = (1, 2, 3, 4)[CASES.index((key, dtype, n_q, nb)) % 4]
    _quiet_tables(monkeypatch, ops, _Pinned(ops.gemm_config(tile, 1), lambda k: k[-1] > 16))
    monkeypatch.setattr(ops, "GEMM_AUTOTUNE", False)
    eng, twin = _engine(key, dtype), _w16_kept_engine(key, dtype)
    assert eng.w8_only and all(isinstance(eng.w.t[n], ops.CodesWeight) for n in _lm_names(eng))
    for n in ("l0.wqkv", "l1.wd", "lm_head"):                                      # the same model: the same codes
        assert torch.equal(eng.w.t[n].codes, twin.w.w8(n)[0]) and torch.equal(eng.w.t[n].scale, twin.w.w8(n)[1])
    lm, image = eng.cfg.lm, eng.cfg.vision.image
    ids, imgs = _prompts(n_q, 1, lm.vocab, seed=31 + n_q, image=image)
    kw = dict(images=imgs, use_dd_unk=True, use_dd=nb == 3, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, max_new_tokens=5, cd_greedy=True,
              output_scores=True)
    with ops.batch_invariant():
        n0 = ops.w8_launches()
        a = eng.generate(ids, **kw)
        assert ops.w8_launches() >= n0 + 4 * lm.n_layers + 1                       # every projection of the model launched on codes
        b = twin.generate(ids, **kw)
    assert a.stats["n_rows"] == n_q * nb
    _same(a, b, 5)


def test_tuned_mode_matches_the_fp32_reference_and_pinned_forms_give_the_twins_bits(monkeypatch):
    from llava_align_amd import ops
    from ref_llava import RefLlava
    eng, twin = _engine("7b"), _w16_kept_engine("7b")
    _quiet_tables(monkeypatch, ops, {})                                            # measured forms and tiles, under tables of the test's own
    w16 = copy.copy(eng.w)
    w16.t = {k: (v.dequantize() if isinstance(v, ops.CodesWeight) else v) for k, v in eng.w.t.items()}
    ref = RefLlava(w16, device=DEV)                                                # fp32 model of the dequantised weights
    ids, imgs = _prompts(6, 1, 32000, seed=23)
    out, checked = _compare(eng, ref, ids, imgs, dict(use_dd_unk=True), dict(temperature=0.5), n_new=4, questions=range(6), tol=0.5)
    assert out.stats["n_rows"] == 12 and checked >= 6
    families = {k[-1] for k in ops._gemm_choice}
    assert families & {17, 18} and not families & {9, 10}                          # tuned under the codes keys, none of load_8bit=True's written
    kinds = {k[0] for k in ops._form_choice}
    assert kinds & {n + ops.CODES_KIND_SUFFIX for n in KINDS} and not kinds & {n + "8" for n in KINDS}
    del ref, w16
    # one form per projection on both engines - the GEMM, 128 x 128 tiles on four waves (an id both 8-bit entries serve), hybrid schedule
    cfg = ops.gemm_config(10, 0)
    force = {**{n: "gemm" for n in KINDS}, **{n + "8": "gemm8" for n in KINDS}, **{n + ops.CODES_KIND_SUFFIX: "gemm8" for n in KINDS}}
    _quiet_tables(monkeypatch, ops, _Pinned(cfg, lambda k: k[2] in (4096, 11008)), force)          # (K of the language model's projections, every key family)
    monkeypatch.setattr(ops, "GEMM_AUTOTUNE", False)
    monkeypatch.setattr(ops, "FORCE_LAYER_FORM", "plain")
    kw = dict(images=imgs[:3], use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, max_new_tokens=4, cd_greedy=True, output_scores=True)
    _same(eng.generate(ids[:3], **kw), twin.generate(ids[:3], **kw), 4)


def test_generate_list_tokens_equal_the_load_8bit_engine(monkeypatch):
    from llava_align_amd import ops
    _quiet_tables(monkeypatch, ops, {})
    monkeypatch.setattr(ops, "GEMM_AUTOTUNE", False)
    eng, twin = _engine("tiny"), _w16_kept_engine("tiny")
    lm, image = eng.cfg.lm, eng.cfg.vision.image
    ids, imgs = _prompts(6, 1, lm.vocab, seed=77, image=image)
    kw = dict(use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, cd_greedy=True, max_new_tokens=8, eos_token_id=[2], pad_token_id=0)
    with ops.batch_invariant():
        n0 = ops.w8_launches()
        a = eng.generate_list(ids, imgs, in_flight=3, sync_every=2, admit_min=1, **kw)
        assert ops.w8_launches() > n0
        b = twin.generate_list(ids, imgs, in_flight=3, sync_every=2, admit_min=1, **kw)
    assert a.stats["questions"] == 6 and a.stats["in_flight"] == 3
    assert torch.equal(a.tokens, b.tokens)


def test_memory_and_prefill_on_codes(monkeypatch):
    from llava_align_amd import ops
    _quiet_tables(monkeypatch, ops, {})
    monkeypatch.setattr(ops, "GEMM_AUTOTUNE", False)
    eng, twin = _engine("7b"), _w16_kept_engine("7b")
    for n in _lm_names(eng):
        assert not torch.is_tensor(eng.w.t[n]) and isinstance(eng.w.t[n], ops.CodesWeight), n      # no 16-bit LM projection anywhere
    assert isinstance(eng.lm.lm_head, ops.CodesWeight)                                              # nor a padded 16-bit head
    assert not any(k.endswith((".w8", ".w8s")) for k in eng.w.t)

    def lm_bytes(e):
        held = [e.w.t.get(k) for n in _lm_names(e) for k in (n, n + ".w8", n + ".w8s")]
        return sum(v.nbytes() if isinstance(v, ops.CodesWeight) else v.numel() * v.element_size() for v in held if v is not None)
    assert 2.9 < lm_bytes(twin) / lm_bytes(eng) < 3.0                                               # codes + w16 against codes alone
    seen = {}
    real = type(eng.lm).prefill

    def prefill(self, *a, **k):
        n0 = ops.w8_launches()
        out = real(self, *a, **k)
        seen["prefill"] = ops.w8_launches() - n0
        return out
    monkeypatch.setattr(type(eng.lm), "prefill", prefill)
    ids, imgs = _prompts(2, 1, 32000, seed=3)
    eng.generate(ids, images=imgs, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, max_new_tokens=2, cd_greedy=True)
    assert seen["prefill"] >= 4 * eng.cfg.lm.n_layers                                               # the prefill's projections launched on codes
    with ops.w8_decode(False):
        with pytest.raises(RuntimeError, match="codes-only"):
            eng.generate(ids, images=imgs, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, max_new_tokens=2, cd_greedy=True)
    with pytest.raises(ValueError, match="load_8bit"):
        type(eng)("tiny", device=DEV, w8_only=True)


def _env():
    env = dict(os.environ, VDD_FORCE_DEVICE="0", VDD_DIST_BACKEND="gloo", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def test_surface(tmp_path):
    from llava_align_amd import checkpoint as K
    from llava_align_amd import ops
    from llava_align_amd.engine import LlavaWeights, VddLlavaEngine
    from tiny_checkpoint import write_checkpoint
    info = write_checkpoint(str(tmp_path))
    with pytest.raises(ValueError, match="load_8bit"):
        K.load_llava(info["ckpt"], DEV, w8_only=True)
    eng_a, tok, _proc = K.load_llava(info["ckpt"], DEV, load_8bit=True, w8_only=True)
    cfg, sd = K.config_from_dir(info["ckpt"]), K.load_state_dict(info["ckpt"])
    eng_b = VddLlavaEngine(cfg, weights=LlavaWeights.from_state_dict(cfg, sd, DEV, dtype=torch.float16), device=DEV, load_8bit=True, w8_only=True)
    assert all(isinstance(e.w.t["l0.wgu"], ops.CodesWeight) and isinstance(e.w.t["lm_head"], ops.CodesWeight) for e in (eng_a, eng_b))
    ids, imgs = _prompts(2, 1, cfg.lm.vocab, seed=9, image=cfg.vision.image)
    kw = dict(images=imgs, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, max_new_tokens=6, cd_greedy=True)
    assert torch.equal(eng_a.generate(ids, **kw).tokens, eng_b.generate(ids, **kw).tokens)


def test_driver_with_w8_only_writes_the_answers_of_load_8bit_alone(tmp_path):
    """One driver command line, each run a fresh child process (tests/test_cli.py): --load-8bit --w8-only against --load-8bit alone in a
    cd_greedy run, which selects batch-invariant mode - every field of every answer, the logit scores included."""
    from tiny_checkpoint import write_checkpoint
    info = write_checkpoint(str(tmp_path))
    common = ["--model-path", info["ckpt"], "--question-file", info["questions"], "--image-folder", info["images"], "--use_dd_unk", "--cd_alpha", "1",
              "--cd_beta", "0.1", "--temperature", "0.5", "--cd_greedy", "--max_new_tokens", "6", "--batch", "6", "--load-8bit"]
    files = []
    for name, extra in (("w16_kept", []), ("w8_only", ["--w8-only"])):
        out = str(tmp_path / "out" / f"{name}.jsonl")
        p = subprocess.run([sys.executable, "-m", "llava_align_amd.pope_driver", *common, *extra, "--answers-file", out], capture_output=True, text=True,
                           env=_env(), timeout=900, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        assert json.loads(p.stdout[p.stdout.index("{"):])["batch_invariant"] is True
        files.append([json.loads(l) for l in open(out)])
    assert len(files[0]) == info["n_questions"] and files[0] == files[1]
