"""generate_list(group_images=True) against the default list call: what attending an image prefix once per image buys on
a list with several questions per image, and what singleton groups cost on a list of distinct images.

    python tools/list_group_images_probe.py [--in-flight 90] [--questions 360] [--reps 5] [--max-new-tokens 256] [--layers N]
                                            [--out profiles/list_group_images.jsonl]
        LLaVA-1.5-7B shapes, bf16, use_dd_unk (2 branches), sampled (tuned forms), answer lengths geometric from a random EOS set.
        list "six_per_image": --questions questions, six per image; list "distinct": the same number with every image distinct.
        Legs per list: group_images off / on, each with and without paged_kv.  Every leg runs once untimed (pools, captured steps, form
        choices), then --reps timed rounds in which the four legs ALTERNATE (off, on, off+paged, on+paged, off, ...).  Per leg: tokens/s
        (answer tokens over the wall time of the call, which ends in a device synchronise) as the median over the rounds, every
        round's value, the spread (max - min) of the off leg, peak HBM of the leg's first call on empty caches, in_flight actually
        used, peak groups / rows in groups.  One JSON line per list, appended to --out.
No GPU: the script fails (there is nothing to measure on a CPU)."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from llava_align_amd.engine import LlavaConfig, LlavaWeights, LMConfig, VddLlavaEngine, preset

ap = argparse.ArgumentParser()
ap.add_argument("--in-flight", type=int, default=90)
ap.add_argument("--questions", type=int, default=360)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--max-new-tokens", type=int, default=256)
ap.add_argument("--eos-ids", type=int, default=500)
ap.add_argument("--layers", type=int, default=0, help="decoder layers (0: the preset's 32)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_group_images.jsonl"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("list_group_images_probe: no GPU - nothing to measure")
dev = torch.device("cuda:0")
if a.layers:
    base = preset("llava-1.5-7b")
    cfg = LlavaConfig(LMConfig(**{**base.lm.__dict__, "n_layers": a.layers}), base.vision, "list-group-images-probe")
    eng = VddLlavaEngine(cfg, weights=LlavaWeights.random(cfg, dev, seed=0, lm_head_gain=4.0), device=dev)
else:
    eng = VddLlavaEngine("llava-1.5-7b", device=dev, seed=0, use_graph=True, lm_head_gain=4.0)
eos = sorted(set(np.random.default_rng(5).integers(3, 32000, size=a.eos_ids).tolist()))
kw = dict(use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=1.0, max_new_tokens=a.max_new_tokens, eos_token_id=eos, pad_token_id=0, seed=11,
          sync_every=8, in_flight=a.in_flight)
LEGS = [("off", dict()), ("on", dict(group_images=True)), ("off_paged", dict(paged_kv=True)), ("on_paged", dict(group_images=True, paged_kv=True))]
keep = ("in_flight", "admissions", "steps", "tail_shrinks", "mean_live_rows", "answer_tokens", "n_groups", "shared_rows", "prefix_chunks_per_item",
        "items_capacity", "kv_pages", "kv_pages_peak", "preemptions")


def run(ids, imgs, extra):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = eng.generate_list(ids, imgs, **kw, **extra)
    torch.cuda.synchronize()
    return o, time.perf_counter() - t0


for name, per_img in (("six_per_image", 6), ("distinct", 1)):
    ids, imgs = bench.pope_prompts(a.questions // per_img, per_img=per_img, seed=778)
    by_id = {}
    imgs = [by_id.setdefault(id(im), im.to(dev).to(eng.dtype)) for im in imgs]          # the SAME tensor for the questions about one image
    rec = {"list": name, "questions": len(ids), "per_image": per_img, "in_flight_asked": a.in_flight, "max_new_tokens": a.max_new_tokens,
           "layers": eng.cfg.lm.n_layers, "reps": a.reps, "legs": {}}
    for leg, extra in LEGS:                                                              # untimed: peak HBM on empty caches, warm state
        eng._kvs.clear(); eng._graphs.clear(); eng._kv = None
        gc.collect(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        o, _ = run(ids, imgs, extra)
        rec["legs"][leg] = {"hbm_peak_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1), "tokens_per_s_all": [],
                            **{k: v for k, v in o.stats.items() if k in keep}}
    for _ in range(a.reps):
        for leg, extra in LEGS:
            o, dt = run(ids, imgs, extra)             # (the engine keeps four captured steps: a leg re-captures its steps, every leg alike)
            rec["legs"][leg]["tokens_per_s_all"].append(round(o.stats["answer_tokens"] / dt, 1))
    for leg, r in rec["legs"].items():
        r["tokens_per_s"] = statistics.median(r["tokens_per_s_all"])
    off = rec["legs"]["off"]["tokens_per_s_all"]
    rec["off_spread"] = round(max(off) - min(off), 1)
    rec["on_over_off"] = round(rec["legs"]["on"]["tokens_per_s"] / rec["legs"]["off"]["tokens_per_s"], 3)
    rec["on_paged_over_off_paged"] = round(rec["legs"]["on_paged"]["tokens_per_s"] / rec["legs"]["off_paged"]["tokens_per_s"], 3)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
