"""Wrapper level of tests/poison.py: every public wrapper of the package that allocates its own output or workspace runs once at ONE small
ragged shape (the smallest ragged shape of its own test) with its allocations filled with 0.0, NaN and +3.0e4, in both storage types,
and the WHOLE returned tensors must be the same bits under the three: output bytes a kernel never wrote show up as well as input bytes
it should not have read.

CASES is the coverage table: "module:function" (as poison.allocating_functions names the allocating functions) -> a builder that makes
the inputs - outside the poisoned block - and returns the thunk that calls the wrapper.  tests/test_poison_host.py checks on the host
that every allocating function of the package is in CASES, in ENGINE_COVERED (functions of engine.py, run by
tests/test_poisoned_engine_gpu.py) or in its own list of exceptions.  No wrapper of the table documents an unspecified part of its
output, so every comparison is over whole tensors.  An unpoisoned warm-up call comes first: it fixes the measured forms and GEMM
schedules (ops._pick_form, the tuner), which change the fp32 summation order."""
import pytest
import torch

from poison import PATTERNS, poisoned_alloc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128

# functions of engine.py that allocate: all of them run under tests/test_poisoned_engine_gpu.py (pools, ViT K/V and graph input, the
# repacked own pools of the `retire` mode, the prefill's residual streams, the runner's score rows, the packed prompt embeddings)
ENGINE_COVERED = ("engine:VisionTower._kv_cache", "engine:VisionTower.__call__", "engine:KVCache.__init__", "engine:KVCache.repack_own",
                  "engine:LanguageModel.prefill", "engine:_DecodeRunner.__init__", "engine:VddLlavaEngine._pack")


def _ops():
    from llava_align_amd import ops
    return ops


def _rn(dt, *shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(dt)


def i32(x):
    return torch.as_tensor(x, dtype=torch.int32, device=DEV).contiguous()


def _rope_table(max_pos, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous().to(DEV)


# ------------------------------------------------------------------ element-wise and norm kernels
def _rmsnorm(dt):
    O = _ops()
    x, dl, w = _rn(dt, 7, 4096, seed=1), _rn(dt, 7, 4096, seed=2), _rn(dt, 4096, seed=3) * 0.1 + 1
    slabs = _rn(torch.float32, 4, 7, 4096, seed=4, scale=0.5)
    return lambda: (O.rmsnorm(x, w, 1e-5, delta=dl), O.rmsnorm(x, w, 1e-5), O.rmsnorm(x, w, 1e-5, delta=slabs))


def _silu_mul(dt):
    O = _ops()
    gu = _rn(dt, 5, 2 * 11008, seed=5)
    return lambda: O.silu_mul(gu)


def _embed(dt):
    O = _ops()
    table, ids = _rn(dt, 1000, 4096, seed=6), torch.tensor([0, 999, 5, 5, 17], device=DEV)
    return lambda: O.embed(ids, table)


def _layernorm(dt):
    O = _ops()
    x, w, b = _rn(dt, 9, 1024, seed=31), _rn(dt, 1024, seed=32) * 0.1 + 1, _rn(dt, 1024, seed=33) * 0.1
    return lambda: O.layernorm(x, w, b, 1e-5)


def _layernorm_pos(dt):
    O = _ops()
    T, d = 64, 1664
    M = 2 * T + 37                                         # the tables wrap, M is no multiple of anything
    x, pin, pout = _rn(dt, M, d, seed=34, scale=2.0), _rn(dt, T, d, seed=35), _rn(dt, T, d, seed=36)
    w, b = _rn(dt, d, seed=37) * 0.1 + 1, _rn(dt, d, seed=38) * 0.1
    return lambda: (*O.layernorm_pos(x, w, b, 1e-6, pos_in=pin, pos_out=pout), O.layernorm_pos(x, w, b, 1e-6, pos_in=pin))


def _bias_act(dt):
    O = _ops()
    z, bias = _rn(dt, 7, 4096, seed=34), _rn(dt, 4096, seed=35)
    return lambda: (O.bias_act(z, bias, O.ACT_QUICK_GELU), O.bias_act(z, bias, O.ACT_GELU), O.bias_act(z, None, O.ACT_NONE))


def _add(dt):
    O = _ops()
    a, b = _rn(dt, 7, 520, seed=39), _rn(dt, 7, 520, seed=40)                 # (the kernel takes whole 8-element vectors)
    return lambda: O.add(a, b)


def _vit_im2col(dt):
    O = _ops()
    img = _rn(torch.float32, 3, 3, 56, 56, seed=41)
    return lambda: O.vit_im2col(img, 14, 640, dtype=dt)                   # 588 patch columns, 52 zero-padded ones


def _vit_assemble(dt):
    O = _ops()
    n, T, w = 3, 17, 128
    emb, cls, pos = _rn(dt, n * (T - 1), w, seed=71), _rn(dt, w, seed=72), _rn(dt, T, w, seed=73)
    return lambda: O.vit_assemble(emb, cls, pos, n, T)


def _vit_qkv_split(dt):
    O = _ops()
    n, T, H, Dv = 3, 17, 2, 64
    qkv = _rn(dt, n * T, 3 * H * Dv, seed=74)
    kc, vc = torch.zeros(n + 1, H, T + 3, Dv, dtype=dt, device=DEV), torch.zeros(n + 1, H, T + 3, Dv, dtype=dt, device=DEV)
    return lambda: (O.vit_qkv_split(qkv, kc, vc, n, T, H, Dv), kc, vc)


# ------------------------------------------------------------------ projections
def _skinny_gemm(dt):
    """rows 17 and 50 of the streaming forms, N no multiple of 32, plain / residual; split-K slabs at 5 rows"""
    O = _ops()
    ins = [(_rn(dt, M, K, seed=81), _rn(dt, N, K, seed=82, scale=0.02), _rn(dt, M, N, seed=83)) for M, N, K in ((17, 1000, 256), (50, 40, 512))]
    x5, w5 = _rn(dt, 5, 256, seed=7), _rn(dt, 1000, 256, seed=8, scale=0.02)

    def run():
        out = []
        for x, w, r in ins:
            out += [O.skinny_gemm(x, w), O.skinny_gemm(x, w, resid=r)]
        return out + [O.skinny_gemm(x5, w5, n_split=2, slabs=True)]
    return run


def _gemm_slabs(dt):
    O = _ops()
    x, w = _rn(dt, 33, 512, seed=91), _rn(dt, 520, 512, seed=92, scale=0.02)
    return lambda: O.gemm_slabs(x, w, 2)


def _fused_norm_inputs(dt):
    O = _ops()
    M, d = 5, 256
    x, resid = _rn(dt, M, d, seed=70), _rn(dt, M, d, seed=71)
    wo, ln = _rn(dt, d, d, seed=72, scale=0.02), (1 + 0.1 * _rn(dt, d, seed=73).float()).to(dt)
    h, ss = O.linear_resid_ss(x, wo, resid)
    return O, x, resid, wo, ln, h, ss


def _linear_resid_ss(dt):
    O, x, resid, wo, _, _, _ = _fused_norm_inputs(dt)
    return lambda: O.linear_resid_ss(x, wo, resid)


def _linear_normed(dt):
    O, _, _, _, ln, h, ss = _fused_norm_inputs(dt)
    w3, w1, bias = _rn(dt, 3 * 256, 256, seed=74, scale=0.02), _rn(dt, 1000, 256, seed=75, scale=0.02), _rn(dt, 1000, seed=76)
    return lambda: (O.linear_normed(h, ss, ln, 1e-5, w3), O.linear_normed(h, ss, ln, 1e-5, w1, bias=bias))


def _swiglu_linear_normed(dt):
    O, _, _, _, ln, h, ss = _fused_norm_inputs(dt)
    wgu = _rn(dt, 2 * 512, 256, seed=77, scale=0.02)
    return lambda: O.swiglu_linear_normed(h, ss, ln, 1e-5, wgu)


def _gemm(dt):
    """M = 66 (one row tile and two rows of the next), N of three ragged column tiles: the tuned choice and a stream-K-only schedule (its
    partial tiles go through ops._gemm_ws, which is zeroed, not poisoned), plain / bias + residual / SwiGLU epilogues"""
    O = _ops()
    M, N, K = 66, 520, 256
    x, w, w2 = _rn(dt, M, K, seed=51), _rn(dt, N, K, seed=52, scale=0.02), _rn(dt, 2 * 512, K, seed=55, scale=0.03)
    w3, bias, resid = _rn(dt, 512, K, seed=58, scale=0.03), _rn(dt, 512, seed=56), _rn(dt, M, 512, seed=57)
    return lambda: (O.gemm(x, w), O.gemm(x, w, config=1 + 32), O.gemm(x, w3, bias=bias, resid=resid, epi=O.EPI_BIAS_RESID),
                    O.gemm(x, w2, epi=O.EPI_SWIGLU))


def _skinny_swiglu(dt):
    """ops._skinny_swiglu through its public entry swiglu_linear, the weight-streaming form forced: rows 17 and 50, F = 520"""
    O = _ops()
    w = _rn(dt, 2 * 520, 256, seed=85) * 0.05
    xs = [_rn(dt, M, 256, seed=84) for M in (17, 50)]

    def run():
        O.FORCE_FORM["swiglu"] = "skinny"
        try:
            return [O.swiglu_linear(x, w) for x in xs]
        finally:
            O.FORCE_FORM.pop("swiglu")
    return run


# ------------------------------------------------------------------ KV writes and decode attention
def _rope_kv_write(dt):
    O = _ops()
    M, H, Hkv, T, S = 6, 8, 4, 32, 5
    qkv = _rn(dt, M, (H + 2 * Hkv) * D, seed=4)
    pos, slot = i32([0, 3, 31, 7, 7, 12]), i32([0, 1, 2, 3, 4, 0])
    kc, vc, cs = torch.zeros(S, Hkv, T, D, dtype=dt, device=DEV), torch.zeros(S, Hkv, T, D, dtype=dt, device=DEV), _rope_table(64)
    return lambda: (O.rope_kv_write(qkv, pos, slot, cs, kc, vc, H, Hkv, D), kc, vc)


def _rope_kv_write_paged(dt):
    from llava_align_amd.paged_kv import PAGE
    from test_paged_kv_kernels_gpu import _shuffled_table
    O = _ops()
    H, Hkv, T, S = 32, 8, 64, 6
    cpos_l, slot_l = [0, 15, 16, 17, 63, 31, 5], [0, 1, 2, 3, 4, 5, 1]
    qkv = _rn(dt, len(cpos_l), (H + 2 * Hkv) * D, seed=4)
    pos, cpos, slot, cs = i32([40 + c for c in cpos_l]), i32(cpos_l), i32(slot_l), _rope_table(128)
    n_pages = S * (T // PAGE) + 7
    table = _shuffled_table(S, [T // PAGE] * S, T // PAGE + 2, n_pages, seed=1)
    pk, pv = torch.zeros(n_pages, Hkv, PAGE, D, dtype=dt, device=DEV), torch.zeros(n_pages, Hkv, PAGE, D, dtype=dt, device=DEV)
    return lambda: (O.rope_kv_write_paged(qkv, pos, slot, cs, pk, pv, table, H, Hkv, D, cpos=cpos), pk, pv)


def _decode_case(dt):
    """own slots only, a prefix in another slot, lengths of 1 ... 700 keys (none but one a multiple of 64)"""
    H, Hkv, T, S = 8, 4, 700, 6
    kc, vc = _rn(dt, S, Hkv, T, D, seed=11), _rn(dt, S, Hkv, T, D, seed=12)
    rows = i32([[0, 1, 0, 0], [1, 4, 0, 0], [2, 37, 0, 0], [3, 700, 0, 0], [4, 650, 5, 611], [3, 620, 5, 611], [1, 5, 2, 4]])
    q = _rn(dt, rows.shape[0], H * D, seed=13)
    return H, Hkv, kc, vc, rows, q


def _decode_attention(dt):
    O = _ops()
    H, Hkv, kc, vc, rows, q = _decode_case(dt)
    return lambda: O.decode_attention(q, kc, vc, rows, H, Hkv, D)            # (the wrapper makes its own split-KV workspace: ops._attn_ws is emptied first)


def _attention_workspace(dt):
    """the workspace the engine allocates per runner: returned unwritten by design, so what is compared is the attention that uses it"""
    O = _ops()
    H, Hkv, kc, vc, rows, q = _decode_case(dt)
    return lambda: O.decode_attention(q, kc, vc, rows, H, Hkv, D, workspace=O.attention_workspace(rows.shape[0], H, D, 1400, DEV), max_len=1400)


def _decode_attention_paged(dt):
    from llava_align_amd.paged_kv import PAGE
    from test_paged_kv_kernels_gpu import _paged_copy, _shuffled_table
    O = _ops()
    H, Hkv, T_own, T_pre = 32, 8, 304, 640
    own_lens, prefix_lens = [1, 15, 17, 65, 300], [0, 35, 611]
    S = len(own_lens)
    kc, vc = _rn(dt, S, Hkv, T_own, D, seed=11), _rn(dt, S, Hkv, T_own, D, seed=12)
    kp, vp = _rn(dt, 3, Hkv, T_pre, D, seed=13), _rn(dt, 3, Hkv, T_pre, D, seed=14)
    rows = i32([[s, pl + n, ps, pl] for ps, pl in enumerate(prefix_lens) for s, n in enumerate(own_lens)])
    q = _rn(dt, rows.shape[0], H * D, seed=15)
    held = [-(-n // PAGE) for n in own_lens]                               # a slot holds exactly the pages its own keys need
    n_pages = sum(held) + 9
    table = _shuffled_table(S, held, T_own // PAGE, n_pages, seed=2)
    pk, pv = _paged_copy(kc, table, n_pages), _paged_copy(vc, table, n_pages)          # pages nobody holds: NaN
    max_len = T_pre + T_own
    return lambda: O.decode_attention_paged(q, pk, pv, table, rows, H, Hkv, D, kp, vp, max_len, O.attention_workspace(rows.shape[0], H, D, max_len, DEV))


def _decode_attention_fused(dt):
    O = _ops()
    H, Hkv, T, S, TP = 8, 2, 720, 5, 640
    cs = _rope_table(800)
    kc, vc = _rn(dt, S, Hkv, T, D, seed=31), _rn(dt, S, Hkv, T, D, seed=32)
    kp, vp = _rn(dt, 2, Hkv, TP, D, seed=33), _rn(dt, 2, Hkv, TP, D, seed=34)
    rows = i32([[0, 1, 0, 0], [1, 2, 0, 0], [2, 66, 0, 0], [3, 700, 0, 0], [4, 650, 1, 611]])       # len counts the new token
    qkv = _rn(dt, rows.shape[0], (H + 2 * Hkv) * D, seed=35)
    pos, cpos, slot = (rows[:, 1] - 1).contiguous(), (rows[:, 1] - 1 - rows[:, 3]).contiguous(), rows[:, 0].contiguous()
    return lambda: [O.decode_attention_fused(qkv, pos, cpos, slot, cs, kc, vc, rows, H, Hkv, D, k_prefix=kp, v_prefix=vp, n_split=ns) for ns in (1, 4)]


def _grouped_case(dt, seed=0):
    """tests/test_grouped_list_attention_gpu.py's scene: groups of 6, 17 (two slices) and 1 rows behind prefixes of 611, 100 and 64 keys,
    six rows in no group, own ranges of 1 .. 40 keys"""
    from test_grouped_list_attention_gpu import R, T_PRE, _case
    return R, T_PRE, _case(dt, 8, 2, 64, None, seed)


def _decode_attention_grouped(dt):
    O = _ops()
    R, T_PRE, (q, ko, vo, kp, vp, frag, rows) = _grouped_case(dt)
    groups, members, items, n = O.list_prefix_work(rows, [True] * R, None, 2, 65535)
    args = (i32(rows), i32(groups), i32(members), i32(items), n)
    return lambda: O.decode_attention_grouped(q, ko, vo, kp, vp, *args, 8, 2, D, T_PRE, 64, prefix_frag=frag, chunks_per_item=2)


def _invariant_case(dt):
    O = _ops()
    R, T_PRE, c = _grouped_case(dt, seed=1)
    rows = c[-1]
    mode = [int(r[3] > 0) for r in rows]
    for r in (7, 11, 22):                       # rows behind a prefix that is not canonical: per row, from the row-major pool
        mode[r] = 0
    return O, R, T_PRE, c, mode, O.list_prefix_work(rows, [True] * R, mode, 2, 65535)


def _decode_attention_shared_invariant(dt):
    O, R, T_PRE, (q, ko, vo, kp, vp, frag, rows), mode, (groups, members, items, n) = _invariant_case(dt)
    args = (i32(rows), i32(mode), i32(groups), i32(members), i32(items), n)
    return lambda: O.decode_attention_shared_invariant(q, ko, vo, kp, vp, *args, 8, 2, D, T_PRE, 64, T_PRE + 64, frag, chunks_per_item=2)


def _decode_attention_grouped_list(dt):
    from test_grouped_list_attention_gpu import _ListTables
    O = _ops()
    R, T_PRE, (q, ko, vo, kp, vp, frag, rows) = _grouped_case(dt)
    groups, members, items, n = O.list_prefix_work(rows, [True] * R, None, 2, 65535)
    tb = _ListTables(4 * n + 3)
    tb.load(rows, groups, members, items)
    return lambda: O.decode_attention_grouped_list(q, ko, vo, kp, vp, tb.rows, tb.groups, tb.group_rows, tb.items, tb.n, tb.cap, 8, 2, D, T_PRE, 64,
                                                   frag, chunks_per_item=2)


def _decode_attention_shared_invariant_list(dt):
    from test_grouped_list_attention_gpu import _ListTables
    O, R, T_PRE, (q, ko, vo, kp, vp, frag, rows), mode, (groups, members, items, n) = _invariant_case(dt)
    tb = _ListTables(5 * n)
    tb.load(rows, groups, members, items, mode)
    return lambda: O.decode_attention_shared_invariant_list(q, ko, vo, kp, vp, tb.rows, tb.mode, tb.groups, tb.group_rows, tb.items, tb.n, tb.cap,
                                                            8, 2, D, T_PRE, 64, T_PRE + 64, frag, chunks_per_item=2)


# ------------------------------------------------------------------ prefill attention
def _flash_attention(dt):
    """packed ragged sequences: several 128-row query blocks, a single row, sequences continuing a prefix held in another slot"""
    O = _ops()
    H, Hkv, T, S = 8, 2, 700, 4
    kc, vc = _rn(dt, S, Hkv, T, D, seed=21), _rn(dt, S, Hkv, T, D, seed=22)
    seqs = [(0, 300, 0, 0, 0, 0), (300, 1, 0, 1, 0, 0), (301, 65, 0, 2, 0, 0), (366, 30, 611, 3, 0, 611), (396, 130, 36, 1, 2, 36)]
    q, sd = _rn(dt, sum(s[1] for s in seqs), H * D, seed=23), i32(seqs)
    q3, sd3 = q[:366].contiguous(), i32(seqs[:3])                        # the first three sequences alone, every key visible
    return lambda: (O.flash_attention(q, kc, vc, sd, len(seqs), 300, H, Hkv, D, causal=True),
                    O.flash_attention(q3, kc, vc, sd3, 3, 300, H, Hkv, D, causal=False))


def _flash_attention_packed(dt):
    O = _ops()
    H, Hkv = 8, 4
    kp, vp = _rn(dt, 3, Hkv, 640, D, seed=61), _rn(dt, 3, Hkv, 640, D, seed=62)
    ko, vo = _rn(dt, 16, Hkv, 64, D, seed=63), _rn(dt, 16, Hkv, 64, D, seed=64)
    rows, r = [], 0
    for i, (tq, ps, pl) in enumerate([(25, 0, 611), (19, 0, 611), (28, 0, 611), (32, 0, 611), (1, 0, 611), (22, 0, 611), (24, 1, 36), (20, 1, 36),
                                      (27, 1, 36), (30, 2, 100), (17, 2, 100), (9, 0, 0)]):
        rows.append([r, tq, pl, i, ps, pl]); r += tq
    q, sd, packs = _rn(dt, r, H * D, seed=65), i32(rows), O.flash_packs(rows)
    pk = i32(packs)
    return lambda: O.flash_attention_packed(q, ko, vo, sd, pk, len(packs), H, Hkv, D, k_prefix=kp, v_prefix=vp)


def _attention_probs(dt):
    O = _ops()
    H, Hkv, plen, Ts = 8, 4, 37, 21
    kp, ko = _rn(dt, 3, Hkv, 64, D, seed=101), _rn(dt, 5, Hkv, 32, D, seed=102)
    q = _rn(dt, plen + Ts + 4, H * D, seed=103)
    return lambda: (O.attention_probs(q, ko, (2, plen + Ts, 0, 4, 1, plen), H, Hkv, D, k_prefix=kp), O.attention_probs(q, ko, (0, 9, 0, 3, 0, 0), H, Hkv, D, k_prefix=kp))


# ------------------------------------------------------------------ the other modules
def _contrast_sample(dt):
    """V = 4099 (no multiple of the 8-element chunk) with scores and the top-10; V = 100003 without scores: the row does not fit the LDS
    and goes through a workspace the wrapper allocates"""
    from llava_align_amd.sampling import WarpSpec, contrast_sample
    ins = []
    for B, V, seed in ((3, 4099, 7), (2, 100003, 8)):
        v = _rn(dt, B, V, seed=seed, scale=4.0)
        v[torch.arange(B), torch.arange(B) * 1031 + 5] = 25.0
        ins.append((v, (v.float() + _rn(torch.float32, B, V, seed=seed + 10, scale=1.5)).to(dt)))

    def run():
        out = []
        for (v, c), scores in zip(ins, (True, False)):
            r = contrast_sample(v, c, alpha=1.0, beta=0.1, warp=WarpSpec(temperature=0.7, top_p=0.9), return_scores=scores, pick_argmax=True,
                                n_top=10, seed=3, offset=0)
            out += [r.tokens, r.top_prob, r.top_tok, r.status] + ([r.scores] if scores else [])
        return out
    return run


def _add_diffusion_noise(dt):
    from llava_align_amd.vcd_add_noise import add_diffusion_noise
    img = _rn(dt, 3, 37, 37, seed=9)
    return lambda: add_diffusion_noise(img, 500, seed=(11, 2))


def _qwen_visual_tower(dt):
    """three images through chunks of two: the second chunk runs in the front rows of buffers sized for the first"""
    from llava_align_amd import qwen_visual as Q
    from qwen_visual_weights import IMAGE_SEED, WEIGHT_SEED, qwen_visual_images, qwen_visual_state_dict
    cfg = Q.tiny_qwen_visual_config()
    w = Q.QwenVisualWeights.from_state_dict(cfg, qwen_visual_state_dict(cfg, WEIGHT_SEED), torch.device(DEV), dt)
    imgs = qwen_visual_images(cfg, IMAGE_SEED, 3).to(DEV)
    return lambda: Q.QwenVisualTower(w, chunk=2)(imgs)


CASES = {
    "ops:rmsnorm": _rmsnorm, "ops:silu_mul": _silu_mul, "ops:embed": _embed, "ops:layernorm": _layernorm, "ops:layernorm_pos": _layernorm_pos,
    "ops:bias_act": _bias_act, "ops:add": _add, "ops:vit_im2col": _vit_im2col, "ops:vit_assemble": _vit_assemble, "ops:vit_qkv_split": _vit_qkv_split,
    "ops:skinny_gemm": _skinny_gemm, "ops:gemm_slabs": _gemm_slabs, "ops:linear_resid_ss": _linear_resid_ss, "ops:linear_normed": _linear_normed,
    "ops:swiglu_linear_normed": _swiglu_linear_normed, "ops:gemm": _gemm, "ops:_skinny_swiglu": _skinny_swiglu,
    "ops:rope_kv_write": _rope_kv_write, "ops:rope_kv_write_paged": _rope_kv_write_paged, "ops:decode_attention": _decode_attention,
    "ops:attention_workspace": _attention_workspace, "ops:decode_attention_paged": _decode_attention_paged,
    "ops:decode_attention_fused": _decode_attention_fused, "ops:decode_attention_grouped": _decode_attention_grouped,
    "ops:decode_attention_shared_invariant": _decode_attention_shared_invariant, "ops:decode_attention_grouped_list": _decode_attention_grouped_list,
    "ops:decode_attention_shared_invariant_list": _decode_attention_shared_invariant_list, "ops:flash_attention": _flash_attention,
    "ops:flash_attention_packed": _flash_attention_packed, "ops:attention_probs": _attention_probs,
    "sampling:contrast_sample": _contrast_sample, "vcd_add_noise:add_diffusion_noise": _add_diffusion_noise,
    "qwen_visual:QwenVisualTower._buf": _qwen_visual_tower, "qwen_visual:QwenVisualTower.__call__": _qwen_visual_tower,
}


def _bits(result):
    ts = [result] if torch.is_tensor(result) else list(result)
    iv = {2: torch.int16, 4: torch.int32, 8: torch.int64}
    return [t.contiguous().view(iv[t.element_size()]).clone() if t.is_floating_point() else t.clone() for t in ts]


def _function_lines(name):
    """(module name, first line, last line) of the function a CASES key names"""
    import importlib
    import inspect
    mod, qual = name.split(":")
    obj = importlib.import_module("llava_align_amd." + mod)
    for part in qual.split("."):
        obj = getattr(obj, part)
    src, first = inspect.getsourcelines(obj)
    return "llava_align_amd." + mod, first, first + len(src) - 1


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "qwen_visual:QwenVisualTower._buf"))       # (one thunk serves both of the tower's functions)
def test_wrapper_output_does_not_depend_on_what_its_allocations_hold(name, dt):
    O = _ops()
    sites = [_function_lines(n) for n in CASES if CASES[n] is CASES[name]]
    CASES[name](dt)()                                       # warm-up: measured forms and schedules are fixed from here on
    got = {}
    for pattern in sorted(PATTERNS):
        thunk = CASES[name](dt)                             # fresh inputs (some wrappers write their caches), made outside the block
        O._attn_ws.clear()                                  # the wrappers' shared split-KV workspace: allocated again, under the pattern
        with poisoned_alloc(pattern) as census:
            out = thunk()
            torch.cuda.synchronize()
        for site in sites:
            assert census.bytes_in(*site) > 0, f"{name} allocated nothing under the pattern: {census.sites}"
        got[pattern] = _bits(out)
    for pattern in ("nan", "big"):
        assert len(got[pattern]) == len(got["zero"])
        for i, (a, b) in enumerate(zip(got["zero"], got[pattern])):
            assert a.shape == b.shape and torch.equal(a, b), f"{name}: returned tensor {i} differs between zero and {pattern} in {int((a != b).sum())} elements"
