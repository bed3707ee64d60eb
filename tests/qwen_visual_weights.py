"""Seeded Qwen-VL vision-tower weights under experiments/Qwen_VL/visual.py's parameter names (test infrastructure).

The golden fixture (tests/golden/qwen_visual.npz, made by tests/golden/make_qwen_visual_golden.py from the REAL VisionTransformer)
stores outputs only; the weights and inputs are regenerated here from `numpy.random.RandomState` (a frozen stream: the same numbers
under every numpy version, on the build container and on the GPU box).  Every tensor is pre-rounded to bf16 (returned as fp32), so
the reference's fp32 run, tests/ref_qwen_visual.py and the bf16 / fp16 kernels all see the same parameter values.  Linear weights
are scaled by fan-in, so activations stay O(1) through the full 48 layers.

Names: conv1, positional_embedding, ln_pre (visual.py:363-373), transformer.resblocks.{i}.{ln_1, ln_2, attn.in_proj, attn.out_proj,
mlp.c_fc, mlp.c_proj} (:173-175, :266-274), attn_pool.{query, pos_embed, kv_proj, ln_q, ln_kv, attn.in_proj_weight / _bias,
attn.out_proj} (:107-127), ln_post, proj (:389-390)."""
import numpy as np
import torch


def _bf16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float()


def qwen_visual_state_dict(cfg, seed: int, std: float = 0.05, device=None):
    """cfg: llava_align_amd.qwen_visual.QwenVisualConfig.  device=None: numpy RandomState (the fixture's stream); a torch device: the same
    layout drawn by a seeded torch generator on that device (the full-size tower's 1.8 B parameters, where the CPU stream is too slow)."""
    if device is None:
        rs = np.random.RandomState(seed)
        draw = lambda s, sc: _bf16(rs.standard_normal(s) * sc)
    else:
        g = torch.Generator(device=device).manual_seed(seed)
        draw = lambda s, sc: (torch.randn(*s, generator=g, device=device) * sc).to(torch.bfloat16).float()
    rnd = lambda *s, sc=std: draw(s, sc)
    lin = lambda o, i: draw((o, i), 0.7 / np.sqrt(i))
    one = lambda n: 1.0 + draw((n,), 0.05)
    W, E, P = cfg.width, cfg.output_dim, cfg.patch
    sd = {}
    sd["conv1.weight"] = draw((W, 3, P, P), 0.7 / np.sqrt(3 * P * P))
    sd["positional_embedding"] = rnd(256, W, sc=0.5)                       # hard-coded 256 rows (visual.py:367), resized to the grid
    sd["ln_pre.weight"], sd["ln_pre.bias"] = one(W), rnd(W)
    for i in range(cfg.layers):
        p = f"transformer.resblocks.{i}."
        sd[p + "ln_1.weight"], sd[p + "ln_1.bias"] = one(W), rnd(W)
        sd[p + "attn.in_proj.weight"], sd[p + "attn.in_proj.bias"] = lin(3 * W, W), rnd(3 * W)
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = lin(W, W), rnd(W)
        sd[p + "ln_2.weight"], sd[p + "ln_2.bias"] = one(W), rnd(W)
        sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = lin(cfg.mlp, W), rnd(cfg.mlp)
        sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = lin(W, cfg.mlp), rnd(W)
    a = "attn_pool."
    sd[a + "query"] = rnd(cfg.n_queries, E, sc=0.5)
    sd[a + "pos_embed"] = rnd(cfg.n_queries, E, sc=0.5)
    sd[a + "kv_proj.weight"] = lin(E, W)
    sd[a + "attn.in_proj_weight"], sd[a + "attn.in_proj_bias"] = lin(3 * E, E), rnd(3 * E)
    sd[a + "attn.out_proj.weight"], sd[a + "attn.out_proj.bias"] = lin(E, E), rnd(E)
    sd[a + "ln_q.weight"], sd[a + "ln_q.bias"] = one(E), rnd(E)
    sd[a + "ln_kv.weight"], sd[a + "ln_kv.bias"] = one(E), rnd(E)
    sd["ln_post.weight"], sd["ln_post.bias"] = one(E), rnd(E)
    sd["proj"] = lin(E, E)                                                 # used as x @ proj: [in, out]
    return sd


def qwen_visual_images(cfg, seed: int, n: int, device=None):
    """Seeded images [n, 3, S, S] (bf16-representable fp32), about what visual.image_transform's Normalize produces."""
    if device is None:
        return _bf16(np.random.RandomState(seed).standard_normal((n, 3, cfg.image, cfg.image)))
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(n, 3, cfg.image, cfg.image, generator=g, device=device).to(torch.bfloat16).float()


# The fixture's case: the tiny config (tests need only it: the full-size tower is checked against the restatement on the GPU).
WEIGHT_SEED, IMAGE_SEED, N_IMAGES = 31, 32, 3
ROWS = (0, 1, 2, 3, 4, 5, 6, 7, -1)      # hidden-state rows stored in full for image 0; all rows as sums
