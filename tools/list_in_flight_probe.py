"""generate_list on the 360-question LLaVA-Bench-shaped list of bench.py (`llava_bench_eos.list_of_360`) at several `in_flight` values: the
own-KV pools grow with it (3 x in_flight slots of suffix + max_new_tokens), the tokens per decode step too.  Record: profiles/r06_list_in_flight.jsonl
--paged-kv: every point in BOTH own-KV forms, alternating (unpaged, paged, unpaged, paged ...: --reps rounds), one JSON line per run.
--preset / --max-new-tokens: the 13B shapes at 1,024 new tokens, where full-length slots do not fit 90 questions in flight.
Record: profiles/list_paged_kv.jsonl"""
import argparse, sys, os, json, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bench
from llava_align_amd.engine import VddLlavaEngine
ap = argparse.ArgumentParser()
ap.add_argument("in_flight", type=int, nargs="*", default=[90, 135, 160])
ap.add_argument("--paged-kv", action="store_true")
ap.add_argument("--reps", type=int, default=1)
ap.add_argument("--preset", default="llava-1.5-7b")
ap.add_argument("--max-new-tokens", type=int, default=512)
ap.add_argument("--questions", type=int, default=360)
a = ap.parse_args()
dev = torch.device("cuda:0")
eng = VddLlavaEngine(a.preset, device=dev, seed=0, use_graph=True, lm_head_gain=4.0)
ids4, imgs4 = bench.pope_prompts(a.questions, per_img=1, seed=778)
imgs4 = [im.to(dev).to(eng.dtype) for im in imgs4]
eos = sorted(set(np.random.default_rng(5).integers(3, 32000, size=250).tolist()))
kw = dict(use_dd=True, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=1.0, top_p=0.9, max_new_tokens=a.max_new_tokens, eos_token_id=eos, pad_token_id=0, seed=11, sync_every=8)
keep = ("in_flight", "admissions", "steps", "tail_shrinks", "admit_gpu_s", "mean_live_rows", "answer_tokens", "paged_kv", "kv_pages", "kv_pages_peak", "preemptions", "own_kv_bytes")
for n_q in a.in_flight:
    for rep in range(a.reps):
        for paged in ((False, True) if a.paged_kv else (False,)):
            eng._kvs.clear(); eng._graphs.clear(); eng._kv = None
            torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            eng.generate_list(ids4, imgs4, in_flight=n_q, paged_kv=paged, **kw)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            o = eng.generate_list(ids4, imgs4, in_flight=n_q, paged_kv=paged, **kw)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            print(json.dumps({"preset": a.preset, "max_new_tokens": a.max_new_tokens, "in_flight_asked": n_q, "rep": rep, "seconds": round(dt, 2),
                              "tokens_per_s": round(o.stats["answer_tokens"] / dt, 1), "hbm_peak_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1),
                              "mean_answer_tokens": round(o.stats["answer_tokens"] / len(ids4), 1),
                              **{k: v for k, v in o.stats.items() if k in keep}}), flush=True)
