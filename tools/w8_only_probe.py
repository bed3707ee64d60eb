"""load_8bit with w8_only: what keeping the quantised weights as codes ONLY costs or buys against load_8bit=True (codes + w16) and against
16-bit weights ("Codes-only weights").  LLaVA-1.5-7B language-model shapes, 32 layers, bf16.

    python tools/w8_only_probe.py [--out profiles/w8_only.jsonl] [--layers N] [--steps memory,tiles,rows2,rows36,rows256,rows1536]
        One visit.  Every step is a fresh child process of this script under its own `timeout`; the chain stops at the first step that fails
        or runs out of time, and what the earlier steps wrote stays in the file.  Steps, one JSON line per record:
          memory     torch.cuda.memory_allocated() after engine construction, one child per mode: 16-bit, load_8bit=True, w8_only=True
          tiles      tiles 1 (256 x 256) and 4 (192 x 256) alone, hybrid schedule, at M = 1,536 and at prefill size (M = 20,480) on the shapes of
                     qkv, o, gate/up (SwiGLU epilogue) and down: vdd_gemm_codes on the codes against vdd_gemm on w16, cold weights by
                     rotation through copies, the legs alternating, 5 runs each
          rowsN      prefill + first token (`prefill_ms`) and the captured decode step (`step_ms`) at N rows (2, 36, 256, 1,536), three
                     engines over the same random weights alternating in one process: "w16" (unquantised, ops.W8_DECODE off), "w8"
                     (load_8bit=True - what the parent commit runs) and "w8_only"; medians of 5, the 16-bit leg's max - min as the spread,
                     and `w8_only_slower_beyond_spread` against either leg (at 1,536 rows one engine at a time - the KV pools of three do not fit
                     one device - so the legs follow each other there: `legs_alternate` false)
No GPU: the script fails (there is nothing to measure on a CPU)."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
SHAPE = dict(d=4096, n_heads=32, n_kv_heads=32, head_dim=128, ffn=11008, vocab=32000)
ROWS = {2: (1, 2), 36: (12, 3), 256: (128, 2), 1536: (768, 2)}           # rows -> (questions, branches)
STEP_TIMEOUT = {"memory": 300, "tiles": 420, "rows2": 420, "rows36": 420, "rows256": 600, "rows1536": 900}       # seconds per child
NEW, REPS = 24, 5


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def build(mode, layers, max_questions=64):
    import torch
    from llava_align_amd.engine import LlavaConfig, LlavaWeights, LMConfig, VddLlavaEngine, VisionConfig
    cfg = LlavaConfig(LMConfig(max_pos=1024, n_layers=layers, **SHAPE), VisionConfig(layers=1), "w8-only-probe")
    w = LlavaWeights.random(cfg, DEV, seed=0, lm_head_gain=4.0, dtype=torch.bfloat16)
    kw = {"w16": {}, "w8": dict(load_8bit=True), "w8_only": dict(load_8bit=True, w8_only=True)}[mode]
    return VddLlavaEngine(cfg, weights=w, device=DEV, max_questions=max_questions, **kw)


def child_memory(mode, layers, out):
    import torch
    eng = build(mode, layers)
    torch.cuda.synchronize()
    emit(dict(step="memory", mode=mode, layers=layers, dtype="bf16", allocated_gb=round(torch.cuda.memory_allocated() / 1e9, 3),
              weights_gb=round(eng.w.nbytes() / 1e9, 3), lm_stream_gb=round(eng.w.lm_stream_bytes() / 1e9, 3)), out)


def child_tiles(out):
    import torch
    from llava_align_amd import ops
    d, ffn = SHAPE["d"], SHAPE["ffn"]
    g = torch.Generator(device=DEV).manual_seed(0)
    for wname, N, K, epi in (("wqkv", 3 * d, d, ops.EPI_NONE), ("wo", d, d, ops.EPI_NONE), ("wgu", 2 * ffn, d, ops.EPI_SWIGLU), ("wd", d, ffn, ops.EPI_NONE)):
        w = (torch.randn(N, K, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
        codes, scale, w16 = ops.quantize_w8(w)
        n_rot = int(min(24, max(2, -(-640 * 2 ** 20 // (w16.numel() * 2)))))
        w16s = [w16] + [w16.clone() for _ in range(n_rot - 1)]
        cws = [ops.CodesWeight(codes, scale, torch.bfloat16)] + [ops.CodesWeight(codes.clone(), scale, torch.bfloat16) for _ in range(n_rot - 1)]
        for M in (1536, 20480):
            x = (torch.randn(M, K, device=DEV, generator=g) * 0.5).to(torch.bfloat16)
            for tile in (1, 4):
                cfg = ops.gemm_config(tile, 0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

                def us(ws, iters=12):
                    ops.gemm(x, ws[0], epi=epi, config=cfg), ops.gemm(x, ws[1 % n_rot], epi=epi, config=cfg)
                    e0.record()
                    for i in range(iters):
                        ops.gemm(x, ws[(i + 2) % n_rot], epi=epi, config=cfg)
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) / iters * 1e3
                t16, tc = [], []
                for _ in range(REPS):
                    t16.append(us(w16s)), tc.append(us(cws))
                flop = 2.0 * M * N * K
                rec = dict(step="tiles", weight=wname, M=M, N=N, K=K, epilogue="swiglu" if epi == ops.EPI_SWIGLU else "none", tile=tile, schedule=0,
                           dtype="bf16", reps=REPS, w16_us=round(statistics.median(t16), 1), codes_us=round(statistics.median(tc), 1),
                           w16_us_all=[round(v, 1) for v in t16], codes_us_all=[round(v, 1) for v in tc], w16_spread_us=round(max(t16) - min(t16), 1))
                rec.update(w16_pflops=round(flop / rec["w16_us"] / 1e9, 3), codes_pflops=round(flop / rec["codes_us"] / 1e9, 3),
                           codes_slower_beyond_spread=bool(rec["codes_us"] - rec["w16_us"] > rec["w16_spread_us"]))
                emit(rec, out)
        del w, w16, codes, w16s, cws
        torch.cuda.empty_cache()


def child_rows(rows, layers, out):
    import torch
    from bench import pope_prompts
    from llava_align_amd import ops
    Q, nb = ROWS[rows]
    modes = ("w16", "w8", "w8_only")
    alternate = rows < 1536           # at 1,536 rows one engine's KV pools take half the device: one engine at a time, the legs one after the other
    engs = {m: build(m, layers, max_questions=max(64, Q)) for m in modes} if alternate else {}
    first = engs["w16"] if alternate else build("w16", layers, max_questions=max(64, Q))
    lm = first.cfg.lm
    # (1,536 rows: six questions per image, the benchmark's batch - 768 image prefixes of their own would need 246 GB of prefix KV at 32 layers)
    ids, imgs = pope_prompts(Q // 6 if rows >= 1536 else Q, per_img=6 if rows >= 1536 else 1, seed=5, vocab=lm.vocab, image=first.cfg.vision.image)
    kw = dict(images=imgs, use_dd_unk=True, use_dd=nb == 3, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, max_new_tokens=NEW, seed=1)

    def run(eng, mode):
        with ops.w8_decode(mode != "w16"):
            eng.call_log = []
            eng.generate(ids, **kw)
            t = eng.call_timing(eng.call_log[-1])
            eng.call_log = None
        return t["prefill_ms"], t["decode_ms"] / t["decode_steps"]
    ts = {m: [] for m in modes}
    if alternate:
        for _ in range(2):                                        # warm-up: forms and tiles measured, steps captured
            for m in modes:
                run(engs[m], m)
        for _ in range(REPS):                                     # alternating legs
            for m in modes:
                ts[m].append(run(engs[m], m))
    else:
        for m in modes:
            eng = first if m == "w16" else build(m, layers, max_questions=max(64, Q))
            first = None
            for _ in range(2):
                run(eng, m)
            for _ in range(REPS):
                ts[m].append(run(eng, m))
            del eng
            torch.cuda.empty_cache()
    rec = dict(step="rows", rows=rows, questions=Q, layers=lm.n_layers, dtype="bf16", mode="tuned", new_tokens=NEW, reps=REPS, legs_alternate=alternate)
    for m in modes:
        rec[m + "_prefill_ms"] = round(statistics.median(v[0] for v in ts[m]), 3)
        rec[m + "_step_ms"] = round(statistics.median(v[1] for v in ts[m]), 4)
        rec[m + "_step_ms_all"] = [round(v[1], 4) for v in ts[m]]
        rec[m + "_prefill_ms_all"] = [round(v[0], 3) for v in ts[m]]
    for what in ("step_ms", "prefill_ms"):
        i = 1 if what == "step_ms" else 0
        spread = max(v[i] for v in ts["w16"]) - min(v[i] for v in ts["w16"])
        rec["w16_spread_" + what] = round(spread, 4)
        rec["w8_only_slower_beyond_spread_" + what] = {leg: bool(rec["w8_only_" + what] - rec[leg + "_" + what] > spread) for leg in ("w16", "w8")}
    dt = ops._MODEL_DT[torch.bfloat16]
    bucket = ops._form_key("linearc", rows, 0, 0, dt)[1]
    rec["w8_only_forms"] = {",".join(map(str, k)): v for k, v in ops._form_choice.items() if k[0].endswith(ops.CODES_KIND_SUFFIX) and k[1] == bucket}
    rec["w8_only_layer_form"] = ops._form_choice.get(("layer", rows, lm.d, 16, dt))
    emit(rec, out)


def main():
    args = sys.argv[1:]
    out = args[args.index("--out") + 1] if "--out" in args else None
    layers = int(args[args.index("--layers") + 1]) if "--layers" in args else 32
    if "--child" in args:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("w8_only_probe: no GPU - nothing can be measured here")
        what = args[args.index("--child") + 1]
        if what.startswith("memory:"):
            child_memory(what.split(":")[1], layers, out)
        elif what == "tiles":
            child_tiles(out)
        else:
            child_rows(int(what[4:]), layers, out)
        return
    steps = args[args.index("--steps") + 1].split(",") if "--steps" in args else list(STEP_TIMEOUT)
    for step in steps:
        for child in ([f"memory:{m}" for m in ("w16", "w8", "w8_only")] if step == "memory" else [step]):
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--child", child, "--layers", str(layers)]
            rc = subprocess.run(cmd + (["--out", out] if out else []), cwd=ROOT).returncode
            if rc != 0:
                raise SystemExit(f"w8_only_probe: step {child} ended with status {rc}; the steps after it were not run")


if __name__ == "__main__":
    main()
