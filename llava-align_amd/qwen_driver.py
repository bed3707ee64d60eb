"""Qwen-VL POPE / open-ended drivers over the native engine: the batched replacement of the reference's per-question loops
experiments/eval/calibrate/qwen_calibrate.py:90-168 (POPE answers + four content-free priors) and
experiments/eval/sampling/qwenvl_sampling.py:48-115 (answers only).

Per question qwen_calibrate.py runs FIVE `model.generate(input_ids, attention_mask, images=..., do_sample=True, max_new_tokens=20,
min_new_tokens=1, pad = eos = tokenizer.eod_id, temperature, top_p, top_k, ...)` calls at B = 1:
  main    '<img>{path}</img>{q} Answer:' with the image tensor, images_cd = add_diffusion_noise(image, noise_step) under --use_cd,
          use_dd / use_dd_unk, cd_alpha, cd_beta (:113-136)                                  -> `text`, `naive` (step-0 top-10 label dict)
  none    '{q} Answer:', plain sampling (:36-37, :142)                                           -> `none`
  unk     'None {q} Answer:', plain (:38-39, :143)                                               -> `unk`
  noise   the main prompt with images = add_diffusion_noise(image, 999), plain (:145-146)        -> `noise`
  zero    the main prompt with images = zeros_like(image), plain (:148-149)                      -> `zero`
Only the step-0 scores of the four prior passes are used (:66-68), so they decode ONE token here.  Each pass is one engine call
over a whole batch of questions.

`embed_prompt(text, image) -> [T, d]` is the
caller's front-end (checkpoint.qwen_embed_prompt: the model's own ViT + resampler, or with --native-visual the package's
qwen_visual.QwenVisualTower, whose `encode_batch` runs a batch's distinct images - and under --use_cd its per-question noised copies - in
one tower call) - token embeddings with the 256 slots between <img> and </img> filled from `image` (a [3, S, S] tensor: what the
reference passes as `images=`, modeling_qwen.py:565-566) or, for prompts without an image span, image = None.  It may return
`(embeddings, n_shared)`, n_shared = the leading rows every prompt about the same image tensor starts with ('<img>' + the slots).
"""
from __future__ import annotations

import json
from typing import Callable, List, Optional, Sequence

import torch

from . import calibrate as C
from . import shard
from .driver_common import (ShardedRun, add_common_args, load_kw, mode_kw, add_script_args, answer_text, chunk_of, distinct, eos_set, finish_distributed, load_distinct_images,
                            plain_kw, pope_scores_for, read_questions, setting_kw, sweep_result, sweep_settings, to_all_rows, write_jsonl)
from .engine import VddLlavaEngine

POPE_PROMPT = "<img>{}</img>{} Answer:"                       # qwen_calibrate.py:41, :97
SAMPLING_PROMPT = "Question: <img>{}</img> {} Answer:"        # qwenvl_sampling.py:54
PRIORS = ("none", "unk", "noise", "zero")                     # the order of qwen_calibrate.py:142-149 (file keys :160-164)
CALIBRATE_NAMES = ("naive", "none", "unk", "none_unk", "noise", "zero", "none_noise", "none_unk_noise", "all")


def _unwrap(e):
    return (e[0], int(e[1])) if isinstance(e, tuple) else (e, None)


def _embeds(embed_prompt, texts, images, keys):
    """-> (list of [T, d], embeds_prefix list or None).  keys[i]: what identifies images[i] (rows with one key share the image span's K/V).
    An embed_prompt with `encode_batch` (checkpoint.qwen_embed_prompt over the native tower) gets the call's distinct images in ONE tower
    call first; the prompts then find their rows kept."""
    hook = getattr(embed_prompt, "encode_batch", None)
    if hook is not None:
        hook(list({id(im): im for im in images if im is not None}.values()))
    out, pre = [], []
    for t, im, k in zip(texts, images, keys):
        e, n = _unwrap(embed_prompt(t, im))
        out.append(e)
        pre.append((k, n) if (n is not None and k is not None) else None)
    return out, (pre if all(p_ is not None for p_ in pre) else None)


def run_qwen_pope(engine: VddLlavaEngine, questions: Sequence[dict], embed_prompt: Callable[[str, Optional[torch.Tensor]], torch.Tensor],
                  decode: Callable[[List[int]], str], load_image: Callable[[str], torch.Tensor], image_path: Callable[[str], str] = lambda f: f,
                  answers_path: Optional[str] = None, model_id: str = "qwen-vl", batch_questions: int = 128, eos_token_id=151643,
                  pad_token_id: Optional[int] = 151643, max_new_tokens: int = 20, min_new_tokens: Optional[int] = 1, use_cd: bool = False,
                  noise_step: int = 500, priors: Sequence[str] = PRIORS, prompt_format: str = POPE_PROMPT, rank: Optional[int] = None,
                  world: Optional[int] = None, batch_invariant: Optional[bool] = None, invariant_shared_prefix: bool = False, sweep: Optional[Sequence[dict]] = None, paged_kv: bool = False, group_images: bool = False,
                  **generate_kw) -> dict:
    """questions: POPE json lines (question_id, image, text[, label]).  load_image(name) -> the [3, S, S] tensor the model's own
    `visual.image_transform` makes of the file (qwen_calibrate.py:100-101).  generate_kw: temperature, top_p, top_k, use_dd, use_dd_unk,
    cd_alpha, cd_beta, seed, cd_greedy ... - the reference's generate kwargs (:113-136; defaults there: temperature 0.2, cd_alpha 1,
    cd_beta 0.1).  priors: which content-free passes to run (all four as the reference; () = answers only, the call shape of
    qwenvl_sampling.py with prompt_format = SAMPLING_PROMPT).
    rank / world (default: the initialised torch.distributed group): every rank decodes its chunk of whole images (shard.ShardPlan), ONE
    collective gathers the results, rank 0 writes the file; every rank returns the full result.  batch_invariant: as in
    pope_driver.run_pope.  The JSONL carries the reference's fields (:155-166): question_id, prompt, text, naive, noise, none, zero, unk,
    model_id, image, metadata.  Returns {"answers": [...], "scores": {...}}.
    sweep (answers-only runs, priors = (): qwenvl_sampling.py:147-185 walks the question file once per sampling setting): a list of
    {"tag", "temperature", "top_p", "top_k"[, "answers_path"]} decodes every setting from ONE prefill per batch (engine.generate(reuse_prefill=True);
    not with --use_cd, whose noise is drawn per call, and not for open-ended lists, which go through generate_list per setting).
    Returns {"runs": {tag: result}}.
    paged_kv: the open-ended list call (generate_list) keeps its own KV in pages that follow the tokens really generated.
    group_images: that call attends a shared (declared) prefix once per group of rows (generate_list(group_images=True)).  A deterministic
    decode runs in batch-invariant mode, which has no groups without its shared-prefix form: there it needs invariant_shared_prefix=True
    (--invariant-shared-prefix) as well, or the engine raises ValueError."""
    from .vcd_add_noise import add_diffusion_noise
    priors = tuple(priors)
    if any(p_ not in PRIORS for p_ in priors):
        raise ValueError(f"priors must be among {PRIORS}")
    run = ShardedRun(questions, rank, world, generate_kw, batch_invariant, invariant_shared_prefix)
    mine, generate_kw = run.mine, run.generate_kw
    decode_token = lambda t: decode([t])
    prior_kw = dict(max_new_tokens=1, n_top=10, min_new_tokens=min_new_tokens, eos_token_id=eos_token_id, pad_token_id=pad_token_id, **plain_kw(generate_kw))
    prompts = {}
    if sweep is not None and priors:
        raise ValueError("sweep: answers-only runs (priors=())")
    settings = sweep_settings(sweep)
    all_rows = [run.rows(engine.device, max_new_tokens, pad_token_id, n_sets=1 + len(priors)) for _ in settings]
    # answers only, no EOS floor (qwenvl_sampling.py:89-103: open-ended answers, max_new_tokens 1024): the whole shard as ONE list, batch_questions
    # in flight, waiting questions admitted into the slots of finished ones (engine.generate_list)
    list_kw = ("temperature", "top_p", "top_k", "use_dd", "use_dd_unk", "cd_alpha", "cd_beta", "seed", "cd_greedy", "sync_every", "admit_min")
    as_list = (not priors and not min_new_tokens and eos_token_id is not None and pad_token_id is not None and bool(mine)
               and engine.cfg.lm.head_dim == 128 and all(k in list_kw for k in generate_kw))
    if sweep is not None and as_list:
        raise ValueError("sweep: open-ended lists (no EOS floor) decode one setting per call")
    list_stats = {}

    def gen(texts_, images_, keys_, **kw):
        emb, pre = _embeds(embed_prompt, texts_, images_, keys_)
        if pre is not None:
            kw["embeds_prefix"] = pre
        return engine.generate(None, inputs_embeds=emb, **kw)

    def text_only(qs, fmt):
        """POPE repeats its question texts over the images, and a text-only prompt's step-0 label dict depends on the text alone: every
        distinct prompt runs once"""
        ts = [fmt.format(q["text"]) for q in qs]
        pick, where = distinct(ts)
        return to_all_rows(gen([ts[i] for i in pick], [None] * len(pick), [None] * len(pick), **prior_kw), where)
    with run.mode():
        for idx, qs in ([(mine, [questions[i] for i in mine])] if as_list else run.batches(batch_questions)):
            imgs = load_distinct_images([q["image"] for q in qs], load_image, engine.device)
            texts = [prompt_format.format(image_path(q["image"]), q["text"]) for q in qs]
            prompts.update(zip(idx, texts))
            kw = dict(generate_kw)
            if use_cd:            # fresh noise per QUESTION, as the reference draws it inside its loop (:103-106); no sharing between them
                kw["images_cd"] = _embeds(embed_prompt, texts, [add_diffusion_noise(im, noise_step) for im in imgs], [None] * len(qs))[0]
            emb, pre = _embeds(embed_prompt, texts, imgs, [("clean", q["image"]) for q in qs])
            if as_list:
                out = engine.generate_list(None, inputs_embeds=emb, embeds_prefix=pre, in_flight=batch_questions, max_new_tokens=max_new_tokens, n_top=10,
                                           eos_token_id=eos_token_id, pad_token_id=pad_token_id, paged_kv=paged_kv, group_images=group_images, **kw)
                all_rows[0].add(idx, out.tokens, [(out.top_tok, out.top_prob)])
                list_stats = out.stats
                continue
            if pre is not None:
                kw["embeds_prefix"] = pre
            # a sweep's settings: the same embedding tensors, decoded again from the first one's kept prefill
            for j, s_ in enumerate(settings):
                o = engine.generate(None, inputs_embeds=emb, max_new_tokens=max_new_tokens, min_new_tokens=min_new_tokens, n_top=10, eos_token_id=eos_token_id,
                                    pad_token_id=pad_token_id, reuse_prefill=len(settings) > 1 and not use_cd, **setting_kw(kw, s_))
                if j:
                    all_rows[j].add(idx, o.tokens, [(o.top_tok, o.top_prob)])
                else:
                    main = o
            tops = [(main.top_tok, main.top_prob)]
            for name in priors:
                if name == "none":
                    tops.append(text_only(qs, "{} Answer:"))
                elif name == "unk":
                    tops.append(text_only(qs, "None {} Answer:"))
                elif name == "noise":
                    o = gen(texts, [add_diffusion_noise(im, 999) for im in imgs], [None] * len(qs), **prior_kw)
                    tops.append((o.top_tok, o.top_prob))
                else:             # one zero image per tensor shape: the span's rows replace the path bytes, so EVERY question shares them
                    zero = {}
                    zs = [zero.setdefault(tuple(im.shape), torch.zeros_like(im)) for im in imgs]
                    o = gen(texts, zs, [("zero", tuple(im.shape)) for im in imgs], **prior_kw)
                    tops.append((o.top_tok, o.top_prob))
            all_rows[0].add(idx, main.tokens, tops)
            engine.clear_image_cache()
    eos = eos_set(eos_token_id)

    def finish(rows, answers_path):
        got = run.gather(rows)
        dicts = [[C.label_dict_from_top(t, p_, decode_token) for t, p_ in got["tops"][s_]] for s_ in range(1 + len(priors))]
        answers = []
        for i, q in enumerate(questions):
            a = {"question_id": q["question_id"], "prompt": prompts.get(i, prompt_format.format(image_path(q["image"]), q["text"])),
                 "text": answer_text(decode, got["tokens"][i], eos)}
            if priors:
                a["naive"] = dicts[0][i]
                for name in ("noise", "none", "zero", "unk"):      # the file's key order (:160-164)
                    if name in priors:
                        a[name] = dicts[1 + priors.index(name)][i]
            a.update(model_id=model_id, image=q["image"], metadata={})
            answers.append(a)
        if answers_path is not None and run.rank == 0:
            write_jsonl(answers_path, answers)
        names = [n_ for n_ in (CALIBRATE_NAMES if priors else ()) if set(C.calibrate_sources(n_)) <= set(("naive",) + priors)]
        return {"answers": answers, "scores": pope_scores_for(questions, answers, ["string_match"] + names), "rank": run.rank, "world": run.world,
                "batch_invariant": run.invariant, "stats": list_stats}
    return sweep_result(sweep, settings, lambda j, s_: finish(all_rows[j], answers_path if sweep is None else s_.get("answers_path")),
                        batch_invariant=run.invariant)


def _parser():
    import argparse
    ap = argparse.ArgumentParser()
    add_common_args(ap, image_folder="", seed=42, dtype="bfloat16",
                    help={"temperature": "default 0.2 (qwen_calibrate.py:182); --sampling runs at 1.0 as qwenvl_sampling.py:147 sets it"})
    add_script_args(ap)
    ap.add_argument("--model-path", default="Qwen/Qwen-VL-Chat")
    ap.add_argument("--use_dd", action="store_true")
    ap.add_argument("--use_dd_unk", action="store_true")
    ap.add_argument("--sampling", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--paged-kv", action="store_true", default=argparse.SUPPRESS, help="open-ended lists: paged own-KV pool (engine.generate_list(paged_kv=True))")
    ap.add_argument("--group-images", action="store_true", default=argparse.SUPPRESS, help="open-ended lists: a shared prefix is attended once per group of rows (engine.generate_list(group_images=True)); a deterministic "
                    "run (batch-invariant mode) also needs --invariant-shared-prefix, else the call raises")
    ap.add_argument("--native-visual", action="store_true", help="the ViT + resampler on the package's kernels (qwen_visual) instead of the model's module")
    return ap


def main(argv=None):
    """python -m llava_align_amd.qwen_driver --model-path DIR --question-file Q.json --image-folder IMGS --answers-file OUT.jsonl
    [--use_dd --use_dd_unk --use_cd --noise_step 500 --cd_alpha 1 --cd_beta 0.1 --temperature 0.2 --top_p P --top_k K --seed 42]
    [--sampling [--no-sweep]]: the arguments of experiments/eval/calibrate/qwen_calibrate.py:170-195; with --sampling the answers-only runs of
    experiments/eval/sampling/qwenvl_sampling.py:117-185 ('setting' in the answers file name replaced by default / temp_T / top_p_P / top_k_K;
    max_new_tokens 20 for POPE question files, 1024 otherwise).  The Qwen-VL directory is loaded through transformers (trust_remote_code: the
    caller's environment must provide what modeling_qwen.py imports); its ViT + resampler fill the image slots, the language model runs
    natively.  Under torchrun: one rank per GPU, whole images per rank, one gather."""
    import os
    import numpy as np
    a = _parser().parse_args(argv)
    from . import checkpoint as K
    rank, world, device = shard.init_from_env()
    eng, tok, model, embed_prompt = K.load_qwen(a.model_path, device, dtype=getattr(torch, a.dtype), native_visual=a.native_visual, **load_kw(a))
    questions = chunk_of(read_questions(a.question_file), a)

    def load_image(name):                                      # qwen_calibrate.py:100-101
        from PIL import Image
        return model.transformer.visual.image_transform(Image.open(os.path.join(a.image_folder, name)).convert("RGB"))
    runs = [(None, a.temperature if a.temperature is not None else 0.2, a.top_p, a.top_k)]
    if a.sampling:                                             # qwenvl_sampling.py:147-185: temperature 1.0, no top-p / top-k whatever the CLI says
        runs = [("default", 1.0, None, None)]
        if not (a.no_sweep or a.use_cd):
            runs += [(f"temp_{t}", float(t), None, None) for t in np.round(np.arange(0.05, 1.05, 0.05), 2)]
            runs += [(f"top_p_{p_}", 1.0, float(p_), None) for p_ in np.round(np.arange(0, 1.05, 0.05), 2)]
            runs += [(f"top_k_{k}", 1.0, None, k) for k in (1, 2, 5, 10, 20, 50, 100, 200, 500)]
    pope = "POPE" in a.question_file
    common = dict(image_path=lambda f: os.path.join(a.image_folder, f), model_id="qwen-vl" if "Chat" not in a.model_path else "qwen-vl-chat",
                  batch_questions=a.batch, eos_token_id=tok.eod_id, pad_token_id=tok.eod_id, use_cd=a.use_cd, noise_step=a.noise_step, rank=rank, world=world,
                  use_dd=a.use_dd, use_dd_unk=a.use_dd_unk, cd_alpha=a.cd_alpha, cd_beta=a.cd_beta, seed=a.seed, paged_kv=getattr(a, "paged_kv", False), group_images=getattr(a, "group_images", False), **mode_kw(a))
    if a.sampling and pope and len(runs) > 1:
        # the POPE sampling sweep (answers of <= 20 tokens): every setting from ONE pass over the question file, a batch's prefill shared by its settings
        sweep = [dict(tag=tag, temperature=temp, top_p=top_p, top_k=top_k, answers_path=os.path.expanduser(a.answers_file).replace("setting", tag))
                 for tag, temp, top_p, top_k in runs]
        res = run_qwen_pope(eng, questions, embed_prompt, lambda ids: tok.decode(ids, skip_special_tokens=True), load_image, priors=(), prompt_format=SAMPLING_PROMPT,
                            max_new_tokens=20, min_new_tokens=1, sweep=sweep, **common)
        if rank == 0:
            for s_ in sweep:
                print(json.dumps({"run": s_["tag"], "answers_file": s_["answers_path"], "n_answers": len(res["runs"][s_["tag"]]["answers"]),
                                  "scores": res["runs"][s_["tag"]]["scores"]}), flush=True)
        runs = []
    for tag, temp, top_p, top_k in runs:
        path = os.path.expanduser(a.answers_file)
        path = path.replace("setting", tag) if tag else path
        kw = dict(max_new_tokens=20, min_new_tokens=1) if (pope or not a.sampling) else dict(max_new_tokens=1024, min_new_tokens=None)
        res = run_qwen_pope(eng, questions, embed_prompt, lambda ids: tok.decode(ids, skip_special_tokens=True), load_image, answers_path=path,
                            priors=() if a.sampling else PRIORS, prompt_format=SAMPLING_PROMPT if a.sampling else POPE_PROMPT,
                            temperature=temp, top_p=top_p, top_k=top_k, **common, **kw)
        if rank == 0:
            nan = {k: v["nan_rows"] for k, v in res["scores"].items() if isinstance(v, dict) and v.get("nan_rows")}
            print(json.dumps({"run": tag or "calibrate", "answers_file": path, "n_answers": len(res["answers"]), "scores": res["scores"],
                              "rows_whose_calibrated_vector_is_nan": nan}), flush=True)
    finish_distributed(world)


if __name__ == "__main__":
    main()
