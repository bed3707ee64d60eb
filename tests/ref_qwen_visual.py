"""Plain-PyTorch restatement of the Qwen-VL vision tower as experiments/Qwen_VL/visual.py computes it (test infrastructure only;
PINNED to outputs of the reference's own VisionTransformer by tests/test_qwen_visual_host.py / tests/golden/make_qwen_visual_golden.py).

Structured like the reference so that it rounds where the reference rounds when run in a 16-bit dtype (the "eager in the storage
type" yardstick of the GPU tests): conv1 -> + get_abs_pos(positional_embedding) -> ln_pre -> blocks (ln_1, per-head interleaved
in_proj split, q / sqrt(hd), bmm, softmax in the tensor's dtype, bmm, out_proj, residual; ln_2, c_fc, GELU, c_proj, residual) ->
Resampler (kv_proj, ln_kv, queries ln_q(query) + pos_embed, keys x + get_abs_pos(pos_embed), values x; nn.MultiheadAttention's
need_weights path: q * hd^-0.5, bmm, softmax, bmm, out_proj) -> ln_post -> @ proj (visual.py:95-151, :178-256, :298-312, :392-414)."""
import math

import torch
import torch.nn.functional as F


def get_abs_pos(abs_pos, tgt_len):
    src, tgt = int(math.sqrt(abs_pos.shape[0])), int(math.sqrt(tgt_len))
    if src == tgt:
        return abs_pos
    return F.interpolate(abs_pos.float().reshape(1, src, src, -1).permute(0, 3, 1, 2), size=(tgt, tgt), mode="bicubic",
                         align_corners=False).permute(0, 2, 3, 1).flatten(0, 2).to(dtype=abs_pos.dtype)


def _mha(q, k, v, H):
    """[B, Tq, E] x [B, Tk, E] -> [B, Tq, E] as F.multi_head_attention_forward's need_weights path computes it (after the projections)."""
    B, Tq, E = q.shape
    D = E // H
    sp = lambda t: t.reshape(B, -1, H, D).transpose(1, 2).reshape(B * H, -1, D)
    p = torch.bmm(sp(q) * math.sqrt(1.0 / D), sp(k).transpose(-2, -1)).softmax(dim=-1)
    return torch.bmm(p, sp(v)).view(B, H, Tq, D).transpose(1, 2).reshape(B, Tq, E)


@torch.no_grad()
def forward(sd, cfg, images, dtype=torch.float32, keep=None):
    """sd: visual.py's names (fp32 or any dtype; cast to `dtype`), images [n, 3, S, S] -> [n, n_queries, output_dim] in `dtype`.
    keep: a dict that receives `ln_pre` [n, T, W] and `pre_pool` [n, T, W] (the hidden state going into attn_pool)."""
    dev = images.device
    w = lambda k: sd[k].to(device=dev, dtype=dtype)
    W, H, hd, E = cfg.width, cfg.heads, cfg.width // cfg.heads, cfg.output_dim
    x = F.conv2d(images.to(dtype), w("conv1.weight"), stride=cfg.patch)
    x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
    n, T, _ = x.shape
    x = x + get_abs_pos(w("positional_embedding"), T)
    x = F.layer_norm(x, (W,), w("ln_pre.weight"), w("ln_pre.bias"), cfg.eps)
    if keep is not None:
        keep["ln_pre"] = x
    for i in range(cfg.layers):
        p = f"transformer.resblocks.{i}."
        a = F.layer_norm(x, (W,), w(p + "ln_1.weight"), w(p + "ln_1.bias"), cfg.eps)
        qkv = F.linear(a, w(p + "attn.in_proj.weight"), w(p + "attn.in_proj.bias")).view(n, T, H, 3 * hd)
        q, k, v = qkv.split(hd, dim=-1)
        q, k, v = (t.permute(0, 2, 1, 3).reshape(n * H, T, hd) for t in (q, k, v))
        prob = torch.bmm(q / math.sqrt(hd), k.transpose(-2, -1)).softmax(dim=-1)
        ctx = torch.bmm(prob, v).view(n, H, T, hd).permute(0, 2, 1, 3).reshape(n, T, W)
        x = x + F.linear(ctx, w(p + "attn.out_proj.weight"), w(p + "attn.out_proj.bias"))
        a = F.layer_norm(x, (W,), w(p + "ln_2.weight"), w(p + "ln_2.bias"), cfg.eps)
        x = x + F.linear(F.gelu(F.linear(a, w(p + "mlp.c_fc.weight"), w(p + "mlp.c_fc.bias"))), w(p + "mlp.c_proj.weight"), w(p + "mlp.c_proj.bias"))
    if keep is not None:
        keep["pre_pool"] = x
    a = "attn_pool."
    kpos = get_abs_pos(w(a + "pos_embed"), T)
    kv = F.layer_norm(F.linear(x, w(a + "kv_proj.weight")), (E,), w(a + "ln_kv.weight"), w(a + "ln_kv.bias"), cfg.eps)
    qin = F.layer_norm(w(a + "query"), (E,), w(a + "ln_q.weight"), w(a + "ln_q.bias"), cfg.eps) + w(a + "pos_embed")
    wi, bi = w(a + "attn.in_proj_weight"), w(a + "attn.in_proj_bias")
    q = F.linear(qin, wi[:E], bi[:E]).unsqueeze(0).expand(n, -1, -1)
    k = F.linear(kv + kpos, wi[E:2 * E], bi[E:2 * E])
    v = F.linear(kv, wi[2 * E:], bi[2 * E:])
    o = F.linear(_mha(q, k, v, E // 128), w(a + "attn.out_proj.weight"), w(a + "attn.out_proj.bias"))
    o = F.layer_norm(o, (E,), w("ln_post.weight"), w("ln_post.bias"), cfg.eps)
    return o @ w("proj")
