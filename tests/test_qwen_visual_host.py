"""Host side of the native Qwen-VL vision tower (no GPU): tests/ref_qwen_visual.py is pinned to outputs of the reference's own
VisionTransformer (tests/golden/qwen_visual.npz, made by tests/golden/make_qwen_visual_golden.py), the config reads the checkpoint's
`config.visual`, and the load-time weight layouts (blocked, head-padded q | k | v; resized position tables; transposed proj) reproduce
the reference's per-head projections when applied with plain matmuls."""
import os

import numpy as np
import pytest
import torch

import ref_qwen_visual
from qwen_visual_weights import IMAGE_SEED, N_IMAGES, ROWS, WEIGHT_SEED, qwen_visual_images, qwen_visual_state_dict
from llava_align_amd.qwen_visual import PAD_D, QwenVisualConfig, QwenVisualWeights, tiny_qwen_visual_config

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "qwen_visual.npz"))

# config.json "visual" of Qwen-VL / Qwen-VL-Chat (7B)
QWEN_VL_7B_VISUAL = {"heads": 16, "image_size": 448, "image_start_id": 151857, "layers": 48, "mlp_ratio": 4.9231, "output_dim": 4096,
                     "patch_size": 14, "width": 1664}


def close(got, want, tol=1e-4):
    want = torch.from_numpy(np.asarray(want))
    scale = max(1.0, float(want.abs().max()))
    err = float((got.float() - want).abs().max())
    assert err <= tol * scale, (err, scale)


@pytest.fixture(scope="module")
def tiny():
    cfg = tiny_qwen_visual_config()
    return cfg, qwen_visual_state_dict(cfg, WEIGHT_SEED), qwen_visual_images(cfg, IMAGE_SEED, N_IMAGES)


def test_ref_qwen_visual_matches_the_reference_module(tiny):
    cfg, sd, imgs = tiny
    keep = {}
    out = ref_qwen_visual.forward(sd, cfg, imgs, keep=keep)
    close(out, GOLD["out"])
    for name in ("ln_pre", "pre_pool"):
        h = keep[name][0]
        close(h[list(ROWS)], GOLD[f"{name}_rows"])
        close(h.sum(-1), GOLD[f"{name}_rowsum"], tol=1e-4 * 8)
        close(h.abs().sum(-1), GOLD[f"{name}_rowabs"])


def test_fixture_exercises_the_resized_tables(tiny):
    """Both position tables are resized in the fixture's config (256 rows -> 8 x 8; 16 query positions -> 8 x 8 keys), and the outputs
    depend on the image."""
    cfg, sd, imgs = tiny
    assert cfg.n_tokens == 64 and sd["positional_embedding"].shape[0] == 256 and cfg.n_queries == 16
    assert cfg.width // cfg.heads == 104 and cfg.heads_out == 2
    out = torch.from_numpy(GOLD["out"])
    assert float((out[0] - out[1]).abs().max()) > 0.1


def test_config_from_hf_qwen_vl_7b():
    c = QwenVisualConfig.from_hf(QWEN_VL_7B_VISUAL)
    assert (c.image, c.patch, c.width, c.layers, c.heads, c.head_dim, c.mlp) == (448, 14, 1664, 48, 16, 104, 8192)
    assert (c.n_queries, c.output_dim, c.heads_out, c.grid, c.n_tokens, c.k_patch) == (256, 4096, 32, 32, 1024, 640)
    assert c == QwenVisualConfig()                       # the defaults are Qwen-VL-7B's tower
    assert QwenVisualConfig.from_hf(type("V", (), QWEN_VL_7B_VISUAL)()) == c     # attribute-style configs too


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_weight_layouts_reproduce_the_per_head_projections(tiny, dtype):
    cfg, sd, imgs = tiny
    pref = {"transformer.visual." + k: v for k, v in sd.items()}          # the HF model's names carry the prefix
    w = QwenVisualWeights.from_state_dict(cfg, pref, "cpu", dtype)
    t, W, H, hd, E = w.t, cfg.width, cfg.heads, cfg.head_dim, cfg.output_dim
    assert all(v.dtype == dtype for v in t.values())
    torch.manual_seed(0)
    x = torch.randn(5, W, dtype=torch.float64)
    for i in range(cfg.layers):
        p = f"transformer.resblocks.{i}.attn."
        ref = torch.nn.functional.linear(x, sd[p + "in_proj.weight"].to(dtype).double(), sd[p + "in_proj.bias"].to(dtype).double())
        ref = ref.view(5, H, 3, hd)                                          # visual.py:194-204: per head [q_h | k_h | v_h]
        got = (x @ t[f"blk{i}.wqkv"].double().t() + t[f"blk{i}.bqkv"].double()).view(5, 3, H, PAD_D)
        for j in range(3):
            torch.testing.assert_close(got[:, j, :, :hd], ref[:, :, j], rtol=1e-12, atol=1e-12)      # (fp64: only the summation order differs)
            assert torch.count_nonzero(got[:, j, :, hd:]) == 0
        assert torch.count_nonzero(t[f"blk{i}.wqkv"].view(3, H, PAD_D, W)[:, :, hd:]) == 0
        assert torch.count_nonzero(t[f"blk{i}.bqkv"].view(3, H, PAD_D)[:, :, hd:]) == 0
        # out projection: padded context columns meet zero weights; the real ones the reference's columns
        ctx = torch.randn(5, H, hd, dtype=torch.float64)
        pad = torch.zeros(5, H, PAD_D, dtype=torch.float64)
        pad[:, :, :hd] = ctx
        pad[:, :, hd:] = 1e3                                                 # anything in the padding must not leak
        wo = t[f"blk{i}.wo"].double()
        assert torch.count_nonzero(wo.view(W, H, PAD_D)[:, :, hd:]) == 0
        torch.testing.assert_close(pad.view(5, -1) @ wo.t(), ctx.view(5, -1) @ sd[p + "out_proj.weight"].to(dtype).double().t(), rtol=1e-12, atol=1e-9)
    # patch GEMM operand = conv1 (zero-padded from 588 to 640 columns)
    assert t["patch"].shape == (W, 640) and torch.count_nonzero(t["patch"][:, 588:]) == 0
    assert torch.equal(t["patch"][:, :588], sd["conv1.weight"].to(dtype).reshape(W, -1))
    # position tables: the reference's get_abs_pos of the dtype parameter (fp32 bicubic, cast back)
    assert torch.equal(t["pos"], ref_qwen_visual.get_abs_pos(sd["positional_embedding"].to(dtype), cfg.n_tokens))
    assert torch.equal(t["pool.kpos"], ref_qwen_visual.get_abs_pos(sd["attn_pool.pos_embed"].to(dtype), cfg.n_tokens))
    assert t["pos"].shape == (cfg.n_tokens, W) and t["pool.kpos"].shape == (cfg.n_tokens, E)
    # resampler q / k / v blocks of nn.MultiheadAttention's packed in-projection, proj transposed into an [N, K] operand
    wi = sd["attn_pool.attn.in_proj_weight"].to(dtype)
    assert torch.equal(torch.cat([t["pool.wq"], t["pool.wk"], t["pool.wv"]]), wi)
    assert torch.equal(t["proj_t"], sd["proj"].to(dtype).t())
    y = torch.randn(3, E, dtype=torch.float64)
    torch.testing.assert_close(y @ t["proj_t"].double().t(), y @ sd["proj"].to(dtype).double())


def test_weights_refuse_other_dtypes(tiny):
    cfg, sd, _ = tiny
    with pytest.raises(ValueError):
        QwenVisualWeights.from_state_dict(cfg, sd, "cpu", torch.float32)
