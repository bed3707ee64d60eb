"""Qwen-VL vision front-end (BASELINE config #4 and the Qwen POPE / calibrate / sampling drivers) on the package's kernels:

    image -> ViT-bigG/14 (conv1 patch embed, + bicubic-resized position table, ln_pre, 48 pre-LN blocks with 16 heads of 104)
          -> perceiver resampler (kv_proj, ln_kv, 256 learned queries cross-attending each image's 1024 tokens, 32 heads of 128)
          -> ln_post -> proj  =  [n, 256, 4096] rows for the 256 slots between <img> and </img>
    (experiments/Qwen_VL/visual.py:95-151 Resampler, :154-256 VisualAttention / VisualAttentionBlock, :332-414 VisionTransformer).

Every op of the forward is a kernel of this package (GEMMs with fused bias / GELU / residual epilogues, LayerNorm and LayerNorm with
position tables, non-causal flash attention, the ViT glue kernels); torch only holds buffers and does slice / broadcast copies.
The 104-wide ViT heads run on the 128-wide attention kernel: the per-head interleaved in-projection ([q_h | k_h | v_h] per head,
visual.py:194-204) is permuted to the blocked q | k | v layout vit_qkv_split reads and zero-padded per head to 128 in its rows and
bias and in the out-projection's columns, once at load, so the padded dimensions are exactly zero (scale stays 104^-0.5).
Everything that does not depend on the image is derived once: the resized position tables (get_abs_pos, visual.py:23-39, in fp32
then cast, as the reference does on every forward) and the resampler's projected queries Wq (ln_q(query) + pos_embed) + bq.
The tiktoken tokenizer and the torchvision preprocessing (`visual.image_transform`) stay with the caller.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict

import torch

from . import ops

PAD_D = 128                       # head width the attention kernel runs the ViT's heads at
CHUNK = 32                        # images per tower pass (about 45 MB of activations per image at 448 px, bf16)


@dataclass
class QwenVisualConfig:
    image: int = 448
    patch: int = 14
    width: int = 1664
    layers: int = 48
    heads: int = 16
    head_dim: int = 104
    mlp: int = 8192
    n_queries: int = 256
    output_dim: int = 4096
    eps: float = 1e-6

    @property
    def grid(self) -> int:
        return self.image // self.patch

    @property
    def n_tokens(self) -> int:
        return self.grid ** 2

    @property
    def heads_out(self) -> int:
        return self.output_dim // 128          # Resampler(num_heads=output_dim // 128), visual.py:382-388

    @property
    def k_patch(self) -> int:
        return (3 * self.patch * self.patch + 127) // 128 * 128

    @staticmethod
    def from_hf(visual) -> "QwenVisualConfig":
        """`config.visual` of a Qwen-VL checkpoint (a dict: image_size, patch_size, width, layers, heads, mlp_ratio[, n_queries, output_dim])
        -> the tower's shapes; mlp = int(width * mlp_ratio) as VisualAttentionBlock computes it (visual.py:264)."""
        g = (lambda k, d=None: visual.get(k, d)) if isinstance(visual, dict) else (lambda k, d=None: getattr(visual, k, d))
        width, heads = int(g("width")), int(g("heads"))
        return QwenVisualConfig(image=int(g("image_size")), patch=int(g("patch_size")), width=width, layers=int(g("layers")), heads=heads,
                                head_dim=width // heads, mlp=int(width * float(g("mlp_ratio", 4.0))), n_queries=int(g("n_queries", 256)),
                                output_dim=int(g("output_dim", 512)))


def tiny_qwen_visual_config() -> QwenVisualConfig:
    """Test size with the real structure: 104-wide heads (1664 / 16: the smallest width with 104-wide heads the GEMM's K % 128 allows),
    an 8 x 8 grid (the 256-row position table is resized 16 -> 8), 16 queries of 2 heads of 128 (the key table is resized 4 -> 8)."""
    return QwenVisualConfig(image=112, patch=14, width=1664, layers=2, heads=16, head_dim=104, mlp=1024, n_queries=16, output_dim=256)


def get_abs_pos(abs_pos: torch.Tensor, tgt_len: int) -> torch.Tensor:
    """visual.py:23-39: the [L, C] table bicubic-resized to sqrt(tgt_len)^2 rows, in fp32, cast back to the table's dtype."""
    src, tgt = int(math.sqrt(abs_pos.shape[0])), int(math.sqrt(tgt_len))
    if src == tgt:
        return abs_pos
    return torch.nn.functional.interpolate(abs_pos.float().reshape(1, src, src, -1).permute(0, 3, 1, 2), size=(tgt, tgt), mode="bicubic",
                                           align_corners=False).permute(0, 2, 3, 1).flatten(0, 2).to(dtype=abs_pos.dtype)


class QwenVisualWeights:
    """Tensors of one 16-bit dtype under visual.py's parameter names (without the `transformer.visual.` prefix) plus the derived GEMM
    operands: `patch` [width, k_patch], `pos` [T, width], `blk{i}.wqkv / bqkv / wo` (blocked, head-padded), `pool.wq / wk / wv / bq / bk / bv`,
    `pool.kpos` [T, E], `proj_t` [E, E] (the reference computes x @ proj, visual.py:412)."""

    def __init__(self, cfg: QwenVisualConfig, device, dtype=torch.bfloat16):
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype
        self.t: Dict[str, torch.Tensor] = {}

    @staticmethod
    def from_state_dict(cfg: QwenVisualConfig, sd: Dict[str, torch.Tensor], device, dtype=torch.bfloat16) -> "QwenVisualWeights":
        if dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("the tower's kernels take bf16 or fp16 weights")
        w = QwenVisualWeights(cfg, device, dtype)
        pre = "transformer.visual."
        for k, t in sd.items():
            w.t[k[len(pre):] if k.startswith(pre) else k] = t.detach().to(device=device, dtype=dtype).contiguous()
        t, W, H, hd, E = w.t, cfg.width, cfg.heads, cfg.head_dim, cfg.output_dim
        if H * hd != W or hd > PAD_D:
            raise ValueError(f"heads x head_dim must be the width with head_dim <= {PAD_D} (got {H} x {hd} vs {W})")
        pw = t["conv1.weight"].reshape(W, -1)
        t["patch"] = torch.nn.functional.pad(pw, (0, cfg.k_patch - pw.shape[1])).contiguous()
        t["pos"] = get_abs_pos(t["positional_embedding"].cpu(), cfg.n_tokens).to(device).contiguous()
        for i in range(cfg.layers):
            p = f"transformer.resblocks.{i}.attn."
            wq = torch.zeros(3, H, PAD_D, W, dtype=dtype, device=device)
            wq[:, :, :hd] = t[p + "in_proj.weight"].view(H, 3, hd, W).transpose(0, 1)       # per-head [q|k|v] -> blocked q|k|v
            bq = torch.zeros(3, H, PAD_D, dtype=dtype, device=device)
            bq[:, :, :hd] = t[p + "in_proj.bias"].view(H, 3, hd).transpose(0, 1)
            wo = torch.zeros(W, H, PAD_D, dtype=dtype, device=device)
            wo[:, :, :hd] = t[p + "out_proj.weight"].view(W, H, hd)
            t[f"blk{i}.wqkv"], t[f"blk{i}.bqkv"], t[f"blk{i}.wo"] = wq.view(3 * H * PAD_D, W), bq.view(-1), wo.view(W, H * PAD_D)
        a = "attn_pool."
        for j, name in enumerate("qkv"):
            t[f"pool.w{name}"] = t[a + "attn.in_proj_weight"][j * E:(j + 1) * E].contiguous()
            t[f"pool.b{name}"] = t[a + "attn.in_proj_bias"][j * E:(j + 1) * E].contiguous()
        t["pool.kpos"] = get_abs_pos(t[a + "pos_embed"].cpu(), cfg.n_tokens).to(device).contiguous()
        t["proj_t"] = t["proj"].t().contiguous()
        return w

    @staticmethod
    def from_hf(model) -> "QwenVisualWeights":
        """The weights of a loaded QWenLMHeadModel's `transformer.visual`, in its dtype and on its device."""
        vis = model.transformer.visual
        cfg = QwenVisualConfig.from_hf(model.config.visual)
        return QwenVisualWeights.from_state_dict(cfg, vis.state_dict(), vis.conv1.weight.device, vis.conv1.weight.dtype)


class QwenVisualTower:
    """`tower(images [n, 3, S, S]) -> [n, n_queries, output_dim]` in the weights' dtype: `transformer.visual(images)` on package kernels, the
    images in chunks of CHUNK, the K / V caches and activation buffers kept between calls."""

    def __init__(self, weights: QwenVisualWeights, chunk: int = CHUNK):
        self.w, self.cfg, self.device, self.chunk = weights, weights.cfg, weights.device, int(chunk)
        self._bufs: Dict[str, torch.Tensor] = {}
        self._cache: Dict[str, tuple] = {}
        cfg, t = self.cfg, weights.t
        if cfg.n_tokens < cfg.n_queries:
            raise ValueError("the cross-attention descriptor assumes at least as many image tokens as queries")
        with torch.no_grad():      # the queries are the same for every image: Wq (ln_q(query) + pos_embed) + bq, once (visual.py:143-149)
            a = "attn_pool."
            qn = ops.layernorm(t[a + "query"], t[a + "ln_q.weight"], t[a + "ln_q.bias"], cfg.eps)
            self.q = ops.gemm(ops.add(qn, t[a + "pos_embed"]), t["pool.wq"], bias=t["pool.bq"], epi=ops.EPI_BIAS)

    def _buf(self, name, rows, cols):
        b = self._bufs.get(name)
        if b is None or b.shape[0] < rows or b.shape[1] != cols:
            b = self._bufs[name] = torch.empty(rows, cols, dtype=self.w.dtype, device=self.device)
        return b[:rows]

    def _kv(self, key, n, H, T, D):
        c = self._cache.get(key)
        if c is None or c[0].shape[0] < n or c[0].shape[2] < T:
            mk = lambda: torch.zeros(n, H, T, D, dtype=self.w.dtype, device=self.device)
            c = self._cache[key] = (mk(), mk())
        return c

    def _queries(self, n):
        """The precomputed queries repeated for n images ([n * NQ, E]); filled once per buffer size."""
        NQ = self.cfg.n_queries
        b = self._bufs.get("q_rep")
        if b is None or b.shape[0] < n * NQ:
            b = self._bufs["q_rep"] = self.q.repeat(n, 1)
        return b[: n * NQ]

    @torch.no_grad()
    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        c = self.cfg
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != c.image or images.shape[3] != c.image:
            raise ValueError(f"images must be [n, 3, {c.image}, {c.image}] (got {tuple(images.shape)})")
        x = images.to(self.device)
        if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            x = x.float()
        n = x.shape[0]
        out = torch.empty(n, c.n_queries, c.output_dim, dtype=self.w.dtype, device=self.device)
        for c0 in range(0, n, self.chunk):
            m = min(self.chunk, n - c0)
            self._forward(x[c0:c0 + m].contiguous(), out[c0:c0 + m].view(m * c.n_queries, c.output_dim))
        return out

    def _forward(self, x, out):
        c, t = self.cfg, self.w.t
        m, T, H, E, NQ, Ho = x.shape[0], c.n_tokens, c.heads, c.output_dim, c.n_queries, c.heads_out
        R = m * T
        patches = ops.vit_im2col(x, c.patch, c.k_patch, out=self._buf("patches", R, c.k_patch), dtype=self.w.dtype)
        emb = ops.gemm(patches, t["patch"], out=self._buf("emb", R, c.width))                                  # conv1, no bias
        h = ops.layernorm_pos(emb, t["ln_pre.weight"], t["ln_pre.bias"], c.eps, pos_in=t["pos"], out=self._buf("h0", R, c.width))
        h2 = self._buf("h1", R, c.width)
        kc, vc = self._kv("vit", m, H, T, PAD_D)
        seqs = torch.tensor([[i * T, T, 0, i, 0, 0] for i in range(m)], dtype=torch.int32, device=self.device)
        a_, qkv_ = self._buf("ln", R, c.width), self._buf("qkv", R, 3 * H * PAD_D)
        q_, att_, f_ = self._buf("q", R, H * PAD_D), self._buf("att", R, H * PAD_D), self._buf("mlp", R, c.mlp)
        for i in range(c.layers):                                             # VisualAttentionBlock.forward, visual.py:300-312
            p = f"transformer.resblocks.{i}."
            a = ops.layernorm(h, t[p + "ln_1.weight"], t[p + "ln_1.bias"], c.eps, out=a_)
            qkv = ops.gemm(a, t[f"blk{i}.wqkv"], bias=t[f"blk{i}.bqkv"], epi=ops.EPI_BIAS, out=qkv_)
            q = ops.vit_qkv_split(qkv, kc, vc, m, T, H, PAD_D, q_out=q_)
            att = ops.flash_attention(q, kc, vc, seqs, m, T, H, H, PAD_D, causal=False, scale=c.head_dim ** -0.5, out=att_)
            ops.gemm(att, t[f"blk{i}.wo"], bias=t[p + "attn.out_proj.bias"], resid=h, epi=ops.EPI_BIAS_RESID, out=h2)
            h, h2 = h2, h
            a = ops.layernorm(h, t[p + "ln_2.weight"], t[p + "ln_2.bias"], c.eps, out=a_)
            f = ops.gemm(a, t[p + "mlp.c_fc.weight"], bias=t[p + "mlp.c_fc.bias"], epi=ops.EPI_BIAS_GELU, out=f_)
            ops.gemm(f, t[p + "mlp.c_proj.weight"], bias=t[p + "mlp.c_proj.bias"], resid=h, epi=ops.EPI_BIAS_RESID, out=h2)
            h, h2 = h2, h
        # Resampler.forward (visual.py:137-151): keys are ln_kv(kv_proj(x)) + pos, values ln_kv(kv_proj(x)); the K and V projections
        # write the two halves of one [R, 2E] buffer (the GEMM's output row stride), which vit_qkv_split(kv_only) scatters to the caches
        a = "attn_pool."
        kv = ops.gemm(h, t[a + "kv_proj.weight"], out=self._buf("kv_in", R, E))
        y, y2 = ops.layernorm_pos(kv, t[a + "ln_kv.weight"], t[a + "ln_kv.bias"], c.eps, pos_out=t["pool.kpos"],
                                  out=self._buf("kv_ln", R, E), out2=self._buf("kv_ln_pos", R, E))
        kvb = self._buf("kv", R, 2 * E)
        ops.gemm(y2, t["pool.wk"], bias=t["pool.bk"], epi=ops.EPI_BIAS, out=kvb[:, :E])
        ops.gemm(y, t["pool.wv"], bias=t["pool.bv"], epi=ops.EPI_BIAS, out=kvb[:, E:])
        kx, vx = self._kv("pool", m, Ho, T, 128)
        ops.vit_qkv_split(kvb, kx, vx, m, T, Ho, 128, kv_only=True)
        seq_x = torch.tensor([[i * NQ, NQ, T - NQ, i, 0, 0] for i in range(m)], dtype=torch.int32, device=self.device)
        ax = ops.flash_attention(self._queries(m), kx, vx, seq_x, m, NQ, Ho, Ho, 128, causal=False, out=self._buf("ax", m * NQ, E))
        o = ops.gemm(ax, t[a + "attn.out_proj.weight"], bias=t[a + "attn.out_proj.bias"], epi=ops.EPI_BIAS, out=self._buf("o", m * NQ, E))
        o = ops.layernorm(o, t["ln_post.weight"], t["ln_post.bias"], c.eps, out=self._buf("o_ln", m * NQ, E))
        ops.gemm(o, t["proj_t"], out=out)                                                                          # x @ proj, visual.py:412
        return out


__all__ = ["QwenVisualConfig", "QwenVisualWeights", "QwenVisualTower", "tiny_qwen_visual_config", "get_abs_pos", "CHUNK", "PAD_D"]
