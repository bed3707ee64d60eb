"""load_8bit: what the decode step costs with 8-bit weight codes against 16-bit weights.

    python tools/w8_step_probe.py [7b] [13b] [--layers N] [--out profiles/w8_decode_step.jsonl]
        LLaVA-1.5-7B / 13B language-model shapes, bf16, rows 2, 3, 6, 12, 16 (the norm-fused few-row step) and 24, 36, 64, 128, 256 (the
        seven-launch layer, where the GEMM's W-stream tiles read the codes): ms per captured decode step from the
        engine's HIP events (VddLlavaEngine.call_timing).  The two legs ALTERNATE in one process: "w16" is an unquantised engine with
        ops.W8_DECODE off - the path of a build without this feature - and "w8" a load_8bit engine over the same random weights.  One JSON
        line per (shape, rows, mode) with the per-leg medians, the spread of the repeated 16-bit runs (`w16_spread_ms` = max - min) and
        whether the 8-bit step is slower than its 16-bit leg by more than that (`w8_slower_beyond_spread`), the layer form each leg took, the
        projection forms the 8-bit leg measured and the bytes a step streams.  Two modes per row count: "tuned" (sampled decode, every form
        measured) and "invariant" (`ops.batch_invariant()`, cd_greedy - what the drivers select for every deterministic decode: the GEMM's
        data-parallel schedule on w16 or, where measured faster, on the codes).  `--modes tuned|invariant` and `--rows 2,24,...` restrict.
    python tools/w8_step_probe.py --proj [7b] [13b] [--out profiles/w8_decode_step.jsonl]
        the projections of one layer alone at 24, 36, 64, 128, 256 rows - `to_norm` (o, down), `linear` (qkv, lm_head), `swiglu` (gate/up) -
        through the ops wrappers, 16-bit (w8=None) against 8-bit (w8=codes), each in the form its tuner measured; cold weights by rotation
        through copies as ops._time_thunks does; the legs alternate and the 16-bit leg is repeated, so its spread is in the record.  Up to
        64 rows the record also holds the weight-streaming kernels alone, forced: "skinny" on w16 against "skinny8" on the codes
        (`skinny_us`, `skinny8_us`).
    python tools/w8_step_probe.py --trace 7b
        one leg-w8 and one leg-w16 decode at 2 rows, nothing else: the workload for a kernel trace taken in a run of its own,
            timeout 600 rocprofv3 --kernel-trace --stats -d profiles/w8_trace -o w8 -- python tools/w8_step_probe.py --trace 7b
        whose kernel stats go to profiles/w8_kernel_stats.csv.
No GPU: the script fails (there is nothing to measure on a CPU)."""
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from bench import pope_prompts
from llava_align_amd import ops
from llava_align_amd.engine import LlavaConfig, LlavaWeights, LMConfig, VddLlavaEngine, VisionConfig

DEV = "cuda:0"
SHAPES = {"7b": dict(d=4096, n_heads=32, n_kv_heads=32, head_dim=128, ffn=11008, vocab=32000, n_layers=32),
          "13b": dict(d=5120, n_heads=40, n_kv_heads=40, head_dim=128, ffn=13824, vocab=32000, n_layers=40)}
ROWS = {2: (1, 2), 3: (1, 3), 6: (3, 2), 12: (6, 2), 16: (8, 2),          # rows -> (questions, branches)
        24: (12, 2), 36: (12, 3), 64: (32, 2), 128: (64, 2), 256: (128, 2)}
PROJ_ROWS = (24, 36, 64, 128, 256)
NEW, REPS = 48, 5


def engines(name, layers):
    kw = dict(SHAPES[name])
    if layers:
        kw["n_layers"] = layers
    cfg = LlavaConfig(LMConfig(max_pos=1024, **kw), VisionConfig(layers=1), f"w8-probe-{name}")
    w16 = LlavaWeights.random(cfg, DEV, seed=0, lm_head_gain=4.0)
    w8 = LlavaWeights(cfg, DEV, w16.dtype)
    w8.t = dict(w16.t)                                            # the same tensors; quantize_lm_w8 replaces the quantised entries only
    return (VddLlavaEngine(cfg, weights=w16, device=DEV, max_questions=128), VddLlavaEngine(cfg, weights=w8, device=DEV, load_8bit=True, max_questions=128))


def step_ms(eng, ids, kw, w8):
    with ops.w8_decode(w8):
        eng.call_log = []
        eng.generate(ids, **kw)
        t = eng.call_timing(eng.call_log[-1])
        eng.call_log = None
    return t["decode_ms"] / t["decode_steps"]


def stream_bytes(eng, w8, rows=2):
    """Weight bytes one step reads: 16-bit everywhere, or codes + scales with EVERY projection on codes; the forms the tuner really took
    are in the record."""
    n = 0
    for k, t in eng.w.t.items():
        if k.endswith((".w8", ".w8s")) or not ((k.startswith("l") and k[1].isdigit()) or k in ("norm", "lm_head")):
            continue
        coded = w8 and eng.w.w8(k) is not None
        n += t.numel() * (1 if coded else 2) + (t.shape[0] * 4 if coded else 0)
    return n


@contextlib.contextmanager
def _forced(forms):
    """ops.FORCE_FORM = forms for the duration"""
    old = dict(ops.FORCE_FORM)
    ops.FORCE_FORM.clear()
    ops.FORCE_FORM.update(forms)
    try:
        yield
    finally:
        ops.FORCE_FORM.clear()
        ops.FORCE_FORM.update(old)


def _time_rot(fn, n_rot, iters=16):
    """ms per call of fn(i) over `iters` calls on rotating weight copies (cold weights), after two untimed calls (tuning happens there)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(0), fn(1 % n_rot)
    e0.record()
    for i in range(iters):
        fn((i + 2) % n_rot)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def proj_leg(name, out):
    """One layer's projections alone, 16-bit against 8-bit, per row count: one JSON line each."""
    sh = SHAPES[name]
    d, ffn, V = sh["d"], sh["ffn"], sh["vocab"]
    dtype = torch.bfloat16
    projs = (("to_norm", "wo", d, d), ("to_norm", "wd", d, ffn), ("linear", "wqkv", 3 * d, d), ("linear", "lm_head", V, d), ("swiglu", "wgu", 2 * ffn, d))
    g = torch.Generator(device=DEV).manual_seed(0)
    for kind, wname, N, K in projs:
        w = (torch.randn(N, K, device=DEV, generator=g) * 0.02).to(dtype)
        codes, scale, w16 = ops.quantize_w8(w)
        n_rot = int(min(24, max(2, -(-640 * 2 ** 20 // (w16.numel() * 2)))))
        w16s, qs = [w16] + [w16.clone() for _ in range(n_rot - 1)], [(codes, scale)] + [(codes.clone(), scale) for _ in range(n_rot - 1)]
        fn = {"to_norm": ops.linear_to_norm, "linear": ops.linear, "swiglu": ops.swiglu_linear}[kind]
        for rows in PROJ_ROWS:
            x = (torch.randn(rows, K, device=DEV, generator=g) * 0.5).to(dtype)
            t16, t8 = [], []
            for _ in range(REPS):
                t16.append(_time_rot(lambda i: fn(x, w16s[i]), n_rot))
                t8.append(_time_rot(lambda i: fn(x, w16s[i], w8=qs[i]), n_rot))
            dt = ops._MODEL_DT[dtype]
            rec = dict(leg="proj", shape=name, kind=kind, weight=wname, rows=rows, N=N, K=K, dtype="bf16", reps=REPS,
                       w16_us=round(statistics.median(t16) * 1e3, 2), w8_us=round(statistics.median(t8) * 1e3, 2),
                       w16_us_all=[round(v * 1e3, 2) for v in t16], w8_us_all=[round(v * 1e3, 2) for v in t8],
                       w16_form=ops._form_choice.get(ops._form_key(kind, rows, N, K, dt)), w8_form=ops._form_choice.get(ops._form_key(kind + "8", rows, N, K, dt)),
                       w16_mb=round(N * K * 2 / 1e6, 1), w8_mb=round((N * K + N * 4) / 1e6, 1))
            rec["speedup"] = round(rec["w16_us"] / rec["w8_us"], 3)
            if ops._skinny_serves(rows, K) and K % 256 == 0:      # the weight-streaming kernels alone: "skinny" on w16 against "skinny8" on the codes
                s16, s8 = [], []
                for _ in range(REPS):
                    with _forced({k: "skinny" for k in (kind, kind + "8")}):
                        s16.append(_time_rot(lambda i: fn(x, w16s[i]), n_rot))
                    with _forced({kind + "8": "skinny8"}):
                        s8.append(_time_rot(lambda i: fn(x, w16s[i], w8=qs[i]), n_rot))
                rec.update(skinny_us=round(statistics.median(s16) * 1e3, 2), skinny8_us=round(statistics.median(s8) * 1e3, 2),
                           skinny_us_all=[round(v * 1e3, 2) for v in s16], skinny8_us_all=[round(v * 1e3, 2) for v in s8])
                rec["skinny8_speedup"] = round(rec["skinny_us"] / rec["skinny8_us"], 3)
            rec["w16_tb_s"], rec["w8_tb_s"] = round(rec["w16_mb"] / rec["w16_us"], 2), round(rec["w8_mb"] / rec["w8_us"], 2)      # MB / us = TB / s
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
                with open(out, "a") as f:
                    f.write(line + "\n")
        del w, w16, codes, w16s, qs
        torch.cuda.empty_cache()


def main():
    args = sys.argv[1:]
    layers = int(args[args.index("--layers") + 1]) if "--layers" in args else 0
    out = args[args.index("--out") + 1] if "--out" in args else None
    names = [a for a in args if a in SHAPES] or list(SHAPES)
    modes = args[args.index("--modes") + 1].split(",") if "--modes" in args else ["tuned", "invariant"]
    only_rows = {int(v) for v in args[args.index("--rows") + 1].split(",")} if "--rows" in args else set(ROWS)
    if not torch.cuda.is_available():
        raise SystemExit("w8_step_probe: no GPU - nothing can be measured here")
    if "--proj" in args:
        for name in names:
            proj_leg(name, out)
        return
    for name in names:
        e16, e8 = engines(name, layers)
        lm = e16.cfg.lm
        for rows, (Q, nb) in ROWS.items():
            if rows not in only_rows:
                continue
            ids, imgs = pope_prompts(Q, per_img=1, seed=5, vocab=lm.vocab, image=e16.cfg.vision.image)
            kw = dict(images=imgs, use_dd_unk=True, use_dd=nb == 3, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, max_new_tokens=NEW, seed=1)
            if "--trace" in args:
                if rows == 2:
                    for _ in range(2):
                        step_ms(e8, ids, kw, True), step_ms(e16, ids, kw, False)
                    torch.cuda.synchronize()
                continue
            for mode in modes:
                inv = mode == "invariant"
                mkw = dict(kw, cd_greedy=True) if inv else kw         # the mode is what the drivers select for deterministic decodes
                with ops.batch_invariant(inv):
                    for _ in range(2):                                # warm-up: forms measured, steps captured
                        step_ms(e16, ids, mkw, False), step_ms(e8, ids, mkw, True)
                    t16, t8 = [], []
                    for _ in range(REPS):                             # alternating legs
                        t16.append(step_ms(e16, ids, mkw, False))
                        t8.append(step_ms(e8, ids, mkw, True))
                dt = ops._MODEL_DT[e16.dtype]
                bucket = ops._form_key("linear8", rows, 0, 0, dt)[1]
                kinds8 = tuple(k + (ops.INVARIANT_KIND_SUFFIX if inv else "") for k in ("linear8", "to_norm8", "swiglu8"))
                rec = dict(shape=name, layers=lm.n_layers, dtype="bf16", mode=mode, rows=rows, questions=Q, new_tokens=NEW, reps=REPS,
                           w16_ms=round(statistics.median(t16), 4), w8_ms=round(statistics.median(t8), 4),
                           w16_ms_all=[round(v, 4) for v in t16], w8_ms_all=[round(v, 4) for v in t8],
                           w16_layer_form=None if inv else ops._form_choice.get(("layer", rows, lm.d, 0, dt)),
                           w8_layer_form=None if inv else ops._form_choice.get(("layer", rows, lm.d, 8, dt)),
                           w16_stream_gb=round(stream_bytes(e16, False, rows) / 1e9, 3), w8_stream_gb=round(stream_bytes(e8, True, rows) / 1e9, 3),
                           w8_forms={",".join(map(str, k)): v for k, v in ops._form_choice.items() if k[0] in kinds8 and k[1] == bucket})
                rec["speedup"] = round(rec["w16_ms"] / rec["w8_ms"], 3)
                rec["w16_spread_ms"] = round(max(t16) - min(t16), 4)
                rec["w8_slower_beyond_spread"] = bool(rec["w8_ms"] - rec["w16_ms"] > rec["w16_spread_ms"])
                if Q == 1:
                    rec["w16_tok_s"], rec["w8_tok_s"] = round(1e3 / rec["w16_ms"], 1), round(1e3 / rec["w8_ms"], 1)
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
                    with open(out, "a") as f:
                        f.write(line + "\n")
        del e16, e8
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
