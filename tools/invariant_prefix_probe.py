"""Batch-invariant mode: what the shared-prefix form (ops.INVARIANT_SHARED_PREFIX) costs and buys per decode step.

    python tools/invariant_prefix_probe.py [--questions 768,48,1] [--layers N] [--out profiles/invariant_shared_prefix.jsonl] [--parent DIR]
        LLaVA-1.5-7B language-model shapes (32 layers), bf16, use_dd_unk (2 branches), 6 questions per image; batches of 768 questions
        (1,536 rows), 48 and 1.  ms per captured decode step from the engine's HIP events (VddLlavaEngine.call_timing), median of 5
        ALTERNATING runs per leg, in one process:
            tuned        the tuned forms (sampled decode: what a run outside the mode takes)
            per_row      the mode as it is by default, flag off (cd_greedy) - the reference leg: its spread (max - min) is in the record
            shared_C     the mode with the flag on at C = 1, 2, 4, 8, 16 chunks per work item of the prefix pass
        Every timed call follows an untimed one of the same leg: the engine keeps four captured steps and the pools of three forms do not
        fit side by side at 768 questions, so a leg's step may have to be captured again, and a capture must not land in a timed decode.
        Per leg also `prefill_s` (the fragment images are new work in the mode) and the peak HBM of one call made on empty caches.
        One JSON line per batch.  --parent DIR: the per-row leg once more from the tree in DIR (a build of the parent commit), in a
        process of its own in the same visit - `per_row_parent_ms`; the flag-off mode must cost what it cost before this form existed.
    python tools/invariant_prefix_probe.py --leg per_row --questions 48 --root DIR
        one leg alone, from the package in DIR (what --parent runs): one JSON line {questions, ms_all}.
No GPU: the script fails (there is nothing to measure on a CPU)."""
import gc
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = sys.argv[1:]
PKG_ROOT = os.path.abspath(ARGS[ARGS.index("--root") + 1]) if "--root" in ARGS else ROOT
sys.path.insert(0, PKG_ROOT)
import torch

from bench import pope_prompts
from llava_align_amd import ops
from llava_align_amd.engine import LlavaConfig, LlavaWeights, LMConfig, VddLlavaEngine, VisionConfig

DEV = "cuda:0"
SHAPE = dict(d=4096, n_heads=32, n_kv_heads=32, head_dim=128, ffn=11008, vocab=32000, n_layers=32)
SIZES = (1, 2, 4, 8, 16)
NEW, REPS = 10, 5


def engine(layers):
    kw = dict(SHAPE)
    if layers:
        kw["n_layers"] = layers
    cfg = LlavaConfig(LMConfig(max_pos=1024, **kw), VisionConfig(layers=1), "invariant-prefix-probe")
    return VddLlavaEngine(cfg, weights=LlavaWeights.random(cfg, DEV, seed=0, lm_head_gain=4.0), device=DEV, max_questions=768)


def mode_of(leg):
    """(context manager, generate keywords) of a leg"""
    if leg == "tuned":
        return ops.batch_invariant(False), dict(seed=1)
    if leg == "per_row":
        return ops.batch_invariant(), dict(cd_greedy=True)
    return ops.batch_invariant(shared_prefix=True), dict(cd_greedy=True)


def call(eng, leg, ids, kw):
    """one generate() of the leg -> (ms per decode step, prefill seconds, stats)"""
    cm, extra = mode_of(leg)
    old = getattr(ops, "INVARIANT_PREFIX_CHUNKS", None)
    try:
        if leg.startswith("shared_"):
            ops.INVARIANT_PREFIX_CHUNKS = int(leg.split("_")[1])          # the constant under test: one value per leg, never per call
        with cm:
            eng.call_log = []
            out = eng.generate(ids, **kw, **extra)
            t = eng.call_timing(eng.call_log[-1])
            eng.call_log = None
    finally:
        if old is not None:
            ops.INVARIANT_PREFIX_CHUNKS = old
    return t["decode_ms"] / max(t["decode_steps"], 1), t["prefill_ms"] / 1e3, out.stats


def peak_gb(eng, leg, ids, kw):
    """peak HBM of one call of the leg on empty caches (pools, captured steps)"""
    eng._kvs.clear(); eng._graphs.clear(); eng._kv = None; eng._prefill_cache = None
    gc.collect(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    call(eng, leg, ids, kw)
    torch.cuda.synchronize()
    return round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("invariant_prefix_probe: no GPU - nothing can be measured here")
    layers = int(ARGS[ARGS.index("--layers") + 1]) if "--layers" in ARGS else 0
    out = ARGS[ARGS.index("--out") + 1] if "--out" in ARGS else None
    parent = ARGS[ARGS.index("--parent") + 1] if "--parent" in ARGS else None
    batches = [int(v) for v in ARGS[ARGS.index("--questions") + 1].split(",")] if "--questions" in ARGS else [768, 48, 1]
    only = ARGS[ARGS.index("--leg") + 1] if "--leg" in ARGS else None
    legs = [only] if only else ["tuned", "per_row"] + [f"shared_{c}" for c in SIZES]
    eng = engine(layers)
    lm = eng.cfg.lm
    for Q in batches:
        ids, imgs = pope_prompts(max(1, Q // 6), per_img=min(6, Q), seed=5, vocab=lm.vocab, image=eng.cfg.vision.image)
        kw = dict(images=imgs, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, max_new_tokens=NEW)
        ms = {leg: [] for leg in legs}
        pre = {leg: [] for leg in legs}
        stats = {}
        for rep in range(REPS):                                          # alternating legs; warm call, then the timed one
            for leg in legs:
                call(eng, leg, ids, kw)
                t, p, stats[leg] = call(eng, leg, ids, kw)
                ms[leg].append(t); pre[leg].append(p)
                print(f"questions {Q} rep {rep} {leg}: {t:.3f} ms / step, prefill {p:.2f} s", file=sys.stderr, flush=True)
        if only:
            emit(dict(leg=only, questions=Q, ms_all=[round(v, 4) for v in ms[only]], ms=round(statistics.median(ms[only]), 4)), out)
            continue
        med = {leg: statistics.median(v) for leg, v in ms.items()}
        rec = dict(shape="7b", layers=lm.n_layers, dtype="bf16", questions=Q, rows=2 * Q, questions_per_image=min(6, Q), new_tokens=NEW, reps=REPS,
                   step_ms={leg: round(v, 4) for leg, v in med.items()}, step_ms_all={leg: [round(x, 4) for x in v] for leg, v in ms.items()},
                   per_row_spread_ms=round(max(ms["per_row"]) - min(ms["per_row"]), 4),
                   prefill_s={leg: round(statistics.median(v), 4) for leg, v in pre.items()},
                   n_groups={leg: s.get("n_groups") for leg, s in stats.items()}, shared_rows={leg: s.get("shared_rows") for leg, s in stats.items()},
                   peak_hbm_gb={leg: peak_gb(eng, leg, ids, kw) for leg in ("tuned", "per_row", "shared_2")})
        rec["shared_over_per_row"] = {leg: round(med[leg] / med["per_row"], 4) for leg in legs if leg.startswith("shared_")}
        rec["shared_over_tuned"] = {leg: round(med[leg] / med["tuned"], 4) for leg in legs if leg.startswith("shared_")}
        rec["per_row_over_tuned"] = round(med["per_row"] / med["tuned"], 4)
        if parent:
            # the flag-off leg from a build of the parent commit, same visit, a process of its own (it ends before the next batch starts)
            eng._kvs.clear(); eng._graphs.clear(); eng._kv = None; eng._prefill_cache = None          # this process keeps its weights only
            gc.collect(); torch.cuda.empty_cache()
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "per_row", "--questions", str(Q), "--root", parent]
                               + (["--layers", str(layers)] if layers else []), capture_output=True, text=True, timeout=900)
            got = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not got:
                raise SystemExit(f"parent leg failed ({r.returncode}):\n{r.stderr[-2000:]}")
            rec["per_row_parent_ms"], rec["per_row_parent_ms_all"] = got[-1]["ms"], got[-1]["ms_all"]
            rec["per_row_equals_parent_within_spread"] = bool(abs(got[-1]["ms"] - med["per_row"]) <= max(rec["per_row_spread_ms"], max(got[-1]["ms_all"]) - min(got[-1]["ms_all"])))
        emit(rec, out)


if __name__ == "__main__":
    main()
