"""Speed of the native Qwen-VL vision tower (llava_align_amd.qwen_visual) at the full Qwen-VL-7B shape, bf16, 448 px: images/s at
1, 8 and 32 images per call; the eager restatement (tests/ref_qwen_visual.py in bf16: bmm + softmax in the dtype, as visual.py
computes) at batch 1, the way checkpoint.py used to call the HF module one image at a time; TFLOP per image from the shapes (heads
unpadded = the model's work, padded to 128 = what the kernels execute) and the achieved PF/s.  Seeded random weights (no checkpoint).

    python tools/qwen_visual_speed.py [--out profiles/qwen_visual_speed.jsonl] [--trace-only]

--trace-only: one warm-up, then ONE 32-image call and nothing else - the run to put under
`rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/qwen_visual_speed.py --trace-only` for per-kernel times."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def flops_per_image(cfg, padded: bool) -> float:
    """2 x MACs of the forward of one image."""
    T, W, E, NQ = cfg.n_tokens, cfg.width, cfg.output_dim, cfg.n_queries
    hd = 128 if padded else cfg.head_dim
    A = cfg.heads * hd
    per_layer = 2 * T * W * 3 * A + 2 * T * A * W + 2 * 2 * T * W * cfg.mlp + 2 * 2 * T * T * A
    pool = 2 * T * W * E + 2 * 2 * T * E * E + 2 * 2 * NQ * T * E + 2 * NQ * E * E * 2
    patch = 2 * T * (cfg.k_patch if padded else 3 * cfg.patch ** 2) * W
    return cfg.layers * per_layer + pool + patch        # (the queries' projection is done once per tower, not per image)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen_visual_speed.jsonl"))
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    from llava_align_amd.qwen_visual import QwenVisualConfig, QwenVisualTower, QwenVisualWeights
    from qwen_visual_weights import qwen_visual_images, qwen_visual_state_dict
    import ref_qwen_visual
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    cfg = QwenVisualConfig()
    sd = {k: v.to(torch.bfloat16) for k, v in qwen_visual_state_dict(cfg, 7, device=dev).items()}
    tower = QwenVisualTower(QwenVisualWeights.from_state_dict(cfg, sd, dev, torch.bfloat16))
    imgs = qwen_visual_images(cfg, 8, 32, device=dev)
    tower(imgs)                                                   # warm-up: code objects, GEMM choices, buffers at 32 images
    if a.trace_only:
        torch.cuda.synchronize()
        tower(imgs)
        torch.cuda.synchronize()
        print("traced one 32-image call")
        return
    f_pad, f_unpad = flops_per_image(cfg, True), flops_per_image(cfg, False)
    recs = []
    for n, iters in ((1, 20), (8, 6), (32, 4)):
        x = imgs[:n].contiguous()
        tower(x)
        s = timed(lambda: tower(x), iters)
        recs.append({"what": "native_tower", "dtype": "bf16", "images_per_call": n, "s_per_call": s, "images_per_s": n / s,
                     "ms_per_image": 1e3 * s / n, "pflops_unpadded": f_unpad * n / s / 1e15, "pflops_executed_padded": f_pad * n / s / 1e15})
    x1 = imgs[:1].contiguous()
    ref_qwen_visual.forward(sd, cfg, x1, dtype=torch.bfloat16)
    s = timed(lambda: ref_qwen_visual.forward(sd, cfg, x1, dtype=torch.bfloat16), 5)
    recs.append({"what": "eager_restatement", "dtype": "bf16", "images_per_call": 1, "s_per_call": s, "images_per_s": 1 / s, "ms_per_image": 1e3 * s,
                 "pflops_unpadded": f_unpad / s / 1e15})
    recs.append({"what": "flops_per_image", "tflop_unpadded": f_unpad / 1e12, "tflop_padded_heads": f_pad / 1e12,
                 "speedup_native32_vs_eager1": recs[2]["images_per_s"] / recs[-1]["images_per_s"],
                 "speedup_native1_vs_eager1": recs[0]["images_per_s"] / recs[-1]["images_per_s"],
                 "device": torch.cuda.get_device_name(0), "torch": torch.__version__})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
