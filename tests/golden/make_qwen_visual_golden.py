"""Build-container-only: runs the REAL Qwen-VL vision tower of the reference (read-only import by file path, nothing copied) on seeded
weights / inputs and commits its OUTPUTS as tests/golden/qwen_visual.npz.

    python tests/golden/make_qwen_visual_golden.py

What is executed unmodified: experiments/Qwen_VL/visual.py VisionTransformer.forward (conv1, get_abs_pos, ln_pre, TransformerBlock of
VisualAttentionBlock / VisualAttention, the Resampler with its nn.MultiheadAttention, ln_post, proj), in fp32 on the CPU.

Import stubs (runtime only): an inert `torchvision` / `torchvision.transforms` (Compose, Resize, ToTensor, Normalize, InterpolationMode)
- torchvision is not installed, and visual.py needs it for its preprocessing only (visual.py:19-20, :354-361), which the tower's
forward never calls.  Weights and inputs come from tests/qwen_visual_weights.py (numpy RandomState: regenerated identically wherever
the tests run).  The tiny config keeps the real head width (1664 / 16 = 104) with 2 layers, an 8 x 8 grid, 16 queries, output 256."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
REF = os.path.join(os.environ.get("VDD_REFERENCE_ROOT", "/root/reference"), "experiments/Qwen_VL/visual.py")


def load_visual():
    class _Inert:
        def __init__(self, *a, **k):
            pass

        def __call__(self, x):
            raise RuntimeError("preprocessing is not part of the fixture")
    tv = types.ModuleType("torchvision")
    tt = types.ModuleType("torchvision.transforms")
    for n in ("Compose", "Resize", "ToTensor", "Normalize"):
        setattr(tt, n, _Inert)
    tt.InterpolationMode = types.SimpleNamespace(BICUBIC="bicubic")
    tv.transforms = tt
    stubs = {}
    for n, m in (("torchvision", tv), ("torchvision.transforms", tt)):
        stubs[n] = sys.modules.get(n)
        sys.modules[n] = m
    try:
        spec = importlib.util.spec_from_file_location("ref_qwen_visual_module", REF)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, old in stubs.items():
            if old is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = old
    return mod


def mlp_ratio(cfg):
    """A ratio for which int(width * ratio) == cfg.mlp (visual.py:264)."""
    r = (cfg.mlp + 0.5) / cfg.width
    assert int(cfg.width * r) == cfg.mlp
    return r


@torch.no_grad()
def run_reference(vis_mod, cfg, sd, imgs):
    torch.manual_seed(0)                                  # (random init, overwritten by load_state_dict)
    m = vis_mod.VisionTransformer(image_size=cfg.image, patch_size=cfg.patch, width=cfg.width, layers=cfg.layers, heads=cfg.heads,
                                  mlp_ratio=mlp_ratio(cfg), n_queries=cfg.n_queries, output_dim=cfg.output_dim)
    m.load_state_dict(sd, strict=True)
    m.eval()
    keep = {}
    h1 = m.ln_pre.register_forward_hook(lambda mod, i, o: keep.__setitem__("ln_pre", o))
    h2 = m.transformer.register_forward_hook(lambda mod, i, o: keep.__setitem__("pre_pool", o.permute(1, 0, 2)))   # LND -> NLD
    out = m(imgs)
    h1.remove(); h2.remove()
    return out, keep


def main():
    from llava_align_amd.qwen_visual import tiny_qwen_visual_config
    from qwen_visual_weights import IMAGE_SEED, N_IMAGES, ROWS, WEIGHT_SEED, qwen_visual_images, qwen_visual_state_dict
    cfg = tiny_qwen_visual_config()
    sd = qwen_visual_state_dict(cfg, WEIGHT_SEED)
    imgs = qwen_visual_images(cfg, IMAGE_SEED, N_IMAGES)
    out, keep = run_reference(load_visual(), cfg, sd, imgs)
    res = {"out": out.numpy()}
    for name in ("ln_pre", "pre_pool"):
        h = keep[name][0]
        res[f"{name}_rows"] = h[list(ROWS)].numpy()
        res[f"{name}_rowsum"] = h.sum(-1).numpy()
        res[f"{name}_rowabs"] = h.abs().sum(-1).numpy()
    print({k: v.shape for k, v in res.items()}, "|out|", float(out.abs().mean()))
    path = os.path.join(HERE, "qwen_visual.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
