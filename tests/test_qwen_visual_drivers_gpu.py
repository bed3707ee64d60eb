"""The native Qwen-VL tower behind the drivers and the adapter: a QWenLMHeadModel-shaped double (tests/hf_doubles.build_qwen) whose
`transformer.visual` is swapped for a module carrying tiny-config weights under visual.py's names (forward = tests/ref_qwen_visual.py),
so that `QwenVisualWeights.from_hf(model)` reads it as it reads a real checkpoint's tower."""
import json
from types import SimpleNamespace

import pytest
import torch

import hf_doubles
import ref_qwen_visual
from qwen_visual_weights import WEIGHT_SEED, qwen_visual_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def decode(ids):
    return " ".join(f"w{int(t)}" for t in ids)


class RefVisual(torch.nn.Module):
    """visual.py's parameter names (state_dict) and its forward (the restatement) - what QwenVisualWeights.from_hf reads."""

    def __init__(self, cfg, sd, dtype):
        super().__init__()
        self.cfg, self.dtype = cfg, dtype
        self.sd = {k: v.to(DEV, dtype) for k, v in sd.items()}
        self.conv1 = SimpleNamespace(weight=self.sd["conv1.weight"])

    def state_dict(self, *a, **k):
        return dict(self.sd)

    def forward(self, images):
        return ref_qwen_visual.forward(self.sd, self.cfg, images.to(DEV), dtype=self.dtype)


class TowerAsVisual(torch.nn.Module):
    """`transformer.visual` that returns the native tower's rows (the rows the native path gets, handed over the HF way)."""

    def __init__(self, tower):
        super().__init__()
        self.tower = tower

    def forward(self, images):
        return self.tower(images)


def qwen_with_tiny_tower():
    from llava_align_amd.qwen_visual import tiny_qwen_visual_config
    cfg = tiny_qwen_visual_config()
    model = hf_doubles.build_qwen(DEV, torch.bfloat16)
    assert model.config.hidden_size == cfg.output_dim
    model.transformer.visual = RefVisual(cfg, qwen_visual_state_dict(cfg, WEIGHT_SEED), torch.bfloat16)
    model.img_rows = cfg.n_queries
    model.config.visual.update(image_size=cfg.image, patch_size=cfg.patch, width=cfg.width, layers=cfg.layers, heads=cfg.heads,
                               mlp_ratio=(cfg.mlp + 0.5) / cfg.width, n_queries=cfg.n_queries, output_dim=cfg.output_dim)
    return cfg, model


def tokenizer_of(model):
    V, st = model.config.vocab_size, model.config.visual["image_start_id"]

    def tokenize(text):                                   # '<img>path</img>' -> <img> + img_rows slots + </img>, as the Qwen tokenizer expands it
        out = []
        for i, part in enumerate(text.replace("</img>", "<img>").split("<img>")):
            out += [st] + [st + 2] * model.img_rows + [st + 1] if i % 2 else hf_doubles.word_ids(part, V - 40)
        return out
    return tokenize


class Counting:
    def __init__(self, tower):
        self.tower, self.calls = tower, []

    def __call__(self, images):
        self.calls.append(int(images.shape[0]))
        return self.tower(images)


def test_run_qwen_pope_on_the_native_tower(tmp_path):
    from llava_align_amd.checkpoint import qwen_embed_prompt
    from llava_align_amd.engine import VddLlavaEngine
    from llava_align_amd.hf_adapter import lm_config_from_hf, lm_weights_from_hf
    from llava_align_amd.qwen_driver import SAMPLING_PROMPT, run_qwen_pope
    from llava_align_amd.qwen_visual import QwenVisualTower, QwenVisualWeights
    cfg, model = qwen_with_tiny_tower()
    lm = lm_config_from_hf(model)
    eng = VddLlavaEngine(lm, weights=lm_weights_from_hf(model, lm), device=DEV)
    eod = model.generation_config.eos_token_id
    tokenize = tokenizer_of(model)
    tower = QwenVisualTower(QwenVisualWeights.from_hf(model))
    images = {f"im{i}.jpg": torch.randn(3, cfg.image, cfg.image, generator=torch.Generator().manual_seed(40 + i)) for i in range(3)}
    qs = [{"question_id": i, "image": f"im{i // 3}.jpg", "text": f"Is there a thing{i} in the image?", "label": ("yes", "no")[i % 2]} for i in range(9)]
    kw = dict(eos_token_id=eod, pad_token_id=eod, max_new_tokens=4, temperature=0.5, cd_alpha=1.0, cd_beta=0.1, use_dd_unk=True, cd_greedy=True,
              batch_questions=6, batch_invariant=True, image_path=lambda f: "/imgs/" + f)

    counted = Counting(tower)
    embed = qwen_embed_prompt(model, tokenize, DEV, tower=counted)
    assert callable(embed.encode_batch)
    torch.manual_seed(3)
    run_qwen_pope(eng, qs, embed, decode, lambda n: images[n], answers_path=str(tmp_path / "native.jsonl"), **kw)
    # per batch (6 + 3 questions): the distinct clean images in one call, the per-question `noise` copies in one call, the zero image once
    assert counted.calls == [2, 6, 1, 1, 3, 1]
    native = [json.loads(l) for l in open(tmp_path / "native.jsonl")]
    assert list(native[0]) == ["question_id", "prompt", "text", "naive", "noise", "none", "zero", "unk", "model_id", "image", "metadata"]

    # the same tower's rows handed over through the model's own `transformer.visual` (the path without encode_batch): the same file
    ref_visual = model.transformer.visual
    model.transformer.visual = TowerAsVisual(tower)
    try:
        plain = qwen_embed_prompt(model, tokenize, DEV)
        assert not hasattr(plain, "encode_batch")
        torch.manual_seed(3)
        run_qwen_pope(eng, qs, plain, decode, lambda n: images[n], answers_path=str(tmp_path / "rows.jsonl"), **kw)
    finally:
        model.transformer.visual = ref_visual
    assert [json.loads(l) for l in open(tmp_path / "rows.jsonl")] == native

    # --use_cd: the noised copies (fresh noise per question) of a batch in ONE tower call
    counted = Counting(tower)
    embed = qwen_embed_prompt(model, tokenize, DEV, tower=counted)
    s = run_qwen_pope(eng, qs[:3], embed, decode, lambda n: images[n], priors=(), prompt_format=SAMPLING_PROMPT, use_cd=True, noise_step=500,
                      seed=5, **dict(kw, batch_invariant=None))
    assert sorted(counted.calls) == [1, 3] and len(s["answers"]) == 3


def test_mme_qwen_inputs_encode_a_batch_once(tmp_path):
    """mme_driver's Qwen path: a batch's distinct image paths go through the tower in one call before the prompts are built (the files
    are read with the model's own `visual.image_transform`)."""
    from llava_align_amd.checkpoint import qwen_embed_prompt
    from llava_align_amd.mme_driver import qwen_mme_inputs
    from llava_align_amd.qwen_visual import QwenVisualTower, QwenVisualWeights
    cfg, model = qwen_with_tiny_tower()
    paths = []
    for i in range(2):
        p = tmp_path / f"p{i}.pt"
        torch.save(torch.randn(3, cfg.image, cfg.image, generator=torch.Generator().manual_seed(i)), p)
        paths.append(str(p))
    model.transformer.visual.image_transform = lambda img: img          # (a stand-in: the "file" is the tensor)
    import PIL.Image
    orig = PIL.Image.open
    PIL.Image.open = lambda p: SimpleNamespace(convert=lambda mode: torch.load(p))
    try:
        counted = Counting(QwenVisualTower(QwenVisualWeights.from_hf(model)))
        embed = qwen_embed_prompt(model, tokenizer_of(model), DEV, tower=counted)
        build = qwen_mme_inputs(embed, lambda f: f)
        lines = [{"image": paths[i % 2], "text": f"q{i}"} for i in range(5)]
        build.prepare(lines)
        assert counted.calls == [2]
        b = build(lines[3], "main")
        assert counted.calls == [2]                                      # rows found kept
        e = b["inputs_embeds"]
        rows = counted.tower(torch.stack([torch.load(p) for p in paths]).to(DEV))[1]     # the same 2-image call as prepare()
        assert torch.equal(e[1:1 + cfg.n_queries], rows.to(e.dtype)) and b["embeds_prefix"] == (paths[1], cfg.n_queries + 2)
    finally:
        PIL.Image.open = orig


def test_attach_qwen_engine_native_visual():
    from llava_align_amd.hf_adapter import attach_qwen_engine, detach_engine
    cfg, model = qwen_with_tiny_tower()
    eng = attach_qwen_engine(model, native_visual=True)
    counted = Counting(model._vdd_tower)
    model._vdd_tower = counted
    V, eod = model.config.vocab_size, model.generation_config.eos_token_id
    ids = torch.tensor([model.image_prompt(hf_doubles.word_ids("Is there a cat in the picture? Answer:", V - 40))], device=DEV)
    img = torch.randn(1, 3, cfg.image, cfg.image, generator=torch.Generator().manual_seed(4)).to(DEV)
    got = model.generate(input_ids=ids, attention_mask=torch.ones_like(ids), do_sample=True, max_new_tokens=4, min_new_tokens=1, pad_token_id=eod,
                         eos_token_id=eod, temperature=1.0, images=img, cd_alpha=1.0, cd_beta=0.1, return_dict_in_generate=True, cd_greedy=True)
    assert counted.calls == [1]
    e = model.transformer.wte(ids)[0].clone()
    e[1:1 + cfg.n_queries] = counted.tower(img)[0].to(e.dtype)
    direct = eng.generate(None, inputs_embeds=[e], max_new_tokens=4, min_new_tokens=1, eos_token_id=eod, pad_token_id=eod, temperature=1.0,
                          cd_alpha=1.0, cd_beta=0.1, cd_greedy=True)
    assert torch.equal(got["tokens"].cpu(), direct.tokens.cpu())
    detach_engine(model)
    assert "_vdd_tower" not in model.__dict__
