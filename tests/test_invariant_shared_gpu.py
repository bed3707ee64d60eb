"""The shared-prefix form of the batch-invariant mode (ops.INVARIANT_SHARED_PREFIX, vdd_decode_attention_shared_invariant).

The contract: the attention output of (row, head) is a function of q[row, head], the K / V of the row's context keys in key order, the
row's len and its prefix length - not of M, the row's place, the other rows or groups, a group's size / index / order, slot numbers,
the max_* bounds, n_items or the workspace.  So ONE target row is computed alone and then as a member of many differently built
launches, and every copy must come out bit for bit the same (torch.equal).  Rows of the per-row kind must equal ops.decode_attention
bit for bit; the census of tests/test_attention_census_gpu.py checks that every key is counted once; the engine, the driver and
generate_list are checked end to end."""

import numpy as np
import pytest
import torch

import attention_census as AC
import test_attention_census_gpu as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
T_PRE, OWN_T = 704, 320
PLENS = [1, 36, 63, 64, 65, 611, 640]
OWNS = [1, 64, 65, 257, 300]
LAYOUTS = [(8, 8), (8, 2)]
W7B = dict(d=4096, n_heads=32, n_kv_heads=32, head_dim=128, ffn=11008, vocab=32000)


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def dt(request):
    return request.param


@pytest.fixture(params=LAYOUTS, ids=[f"H{h}kv{k}" for h, k in LAYOUTS])
def layout(request):
    return request.param


def ops():
    from llava_align_amd import ops as O
    return O


i32 = TC.i32
r64 = lambda v: (int(v) + 63) // 64 * 64


def item_sizes():
    """INVARIANT_PREFIX_CHUNKS and two other fixed item sizes"""
    c = ops().INVARIANT_PREFIX_CHUNKS
    return [c] + [s for s in (1, 4, 2, 8) if s != c][:2]


# ------------------------------------------------------------------------------------------------ 1. row invariance

def _pools(Hkv, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV, dtype)
    p = dict(kp=rnd(6, Hkv, T_PRE, D), vp=rnd(6, Hkv, T_PRE, D), ko=rnd(9, Hkv, OWN_T, D), vo=rnd(9, Hkv, OWN_T, D),
             tk=rnd(Hkv, 640, D), tv=rnd(Hkv, 640, D))
    for a in ("ko", "vo"):
        p[a][7] = p[a][0]                       # the target's own keys live in own slots 0 and 7
    return p


FILL_PLEN = {2: 200, 3: 611, 5: 64}            # the other prefixes of the pool (slots 1 and 4 hold the target's)


def _scene(plen, own, target_groups_first, per_row_rows, seed):
    """-> rows, mode, groups, group_rows, indices of the target's copies.  The target (own slot 0 or 7, prefix slot 1 or 4, `plen` + `own`
    keys) is a group of one, and first / last / at index 16 (a slice edge) of groups of 2, 15, 16, 17 and 33 rows whose other members
    are other questions about the same prefix; three groups on other prefixes come before or after them; the rows are shuffled."""
    rows, mode, groups, members, targets = [], [], [], [], []

    def group(size, pslot, pl, at=None, tslot=0):
        off = len(members)
        for r in range(size):
            i = len(rows)
            if r == at:
                rows.append([tslot, pl + own, pslot, pl]); targets.append(i)
            else:
                rows.append([1 + i % 6, pl + 1 + (i * 37) % 300, pslot, pl])
            mode.append(1); members.append(i)
        groups.append([off, size, pslot, pl])

    def others():
        group(3, 2, FILL_PLEN[2]); group(20, 3, FILL_PLEN[3]); group(1, 5, FILL_PLEN[5])

    def with_target():
        for size, pslot, at, tslot in ((1, 1, 0, 0), (2, 4, 0, 7), (2, 1, 1, 0), (15, 1, 14, 0), (16, 4, 0, 0), (16, 1, 15, 7), (17, 1, 16, 0),
                                       (17, 4, 0, 0), (33, 1, 16, 7), (33, 4, 32, 0), (33, 1, 0, 0)):
            group(size, pslot, plen, at, tslot)
    if target_groups_first:
        with_target(); others()
    else:
        others(); with_target()
    if per_row_rows:
        for r in ([8, 150, 2, 100], [8, 77, 0, 0], [2, 641, 3, 611], [8, 300, 0, 0]):
            rows.append(r); mode.append(0)
    perm = torch.randperm(len(rows), generator=torch.Generator().manual_seed(seed)).tolist()
    inv = {old: new for new, old in enumerate(perm)}
    return [rows[o] for o in perm], [mode[o] for o in perm], groups, [inv[m] for m in members], [inv[t] for t in targets]


def test_a_row_is_the_same_in_every_launch(dt, layout):
    O = ops()
    H, Hkv = layout
    P = _pools(Hkv, dt, seed=7)
    g = torch.Generator().manual_seed(8)
    q_t = torch.randn(H * D, generator=g).to(DEV, dt)
    q_fill = torch.randn(256, H * D, generator=g).to(DEV, dt)
    nan_ws = lambda n_rows, keys, times=1: torch.full((times * O.attention_workspace(n_rows, H, D, keys, DEV).numel(),), float("nan"),
                                                      dtype=torch.float32, device=DEV)
    for plen in PLENS:
        for s in (1, 4):
            P["kp"][s, :, :plen], P["vp"][s, :, :plen] = P["tk"][:, :plen], P["tv"][:, :plen]
        pf = torch.full((6, Hkv, 2 * T_PRE, D), float("nan"), dtype=dt, device=DEV)         # blocks behind a prefix stay NaN: never read
        O.prefix_fragments(P["kp"], P["vp"], pf, i32([0, plen, FILL_PLEN[2], FILL_PLEN[3], plen, FILL_PLEN[5]]))
        for own in OWNS:
            scenes = [_scene(plen, own, False, True, 100 + own), _scene(plen, own, True, False, 200 + own)]
            for cpi in item_sizes():
                def run(rows, mode, groups, grp_rows, mp, mo, mr, ws):
                    M = len(rows)
                    q = q_fill[:M].clone()
                    items = O.prefix_work_items(groups, cpi)
                    return q, lambda qq: O.decode_attention_shared_invariant(qq, P["ko"], P["vo"], P["kp"], P["vp"], i32(rows), i32(mode), i32(groups),
                                                                             i32(grp_rows), i32(items), len(items), H, Hkv, D, mp, mo, mr, pf,
                                                                             workspace=ws, chunks_per_item=cpi)
                # alone: M = 1, a group of one, the tightest bounds and workspace
                _, f = run([[0, plen + own, 1, plen]], [1], [[0, 1, 1, plen]], [0], plen, own, 0, nan_ws(1, r64(plen) + r64(own)))
                alone = f(q_t[None].clone())
                assert bool(torch.isfinite(alone.float()).all())
                # groups on other prefixes first (the target's are groups 3 ...), per-row rows in the call, the pools' capacities as bounds, twice the workspace
                rows, mode, groups, grp_rows, tg = scenes[0]
                q, f = run(rows, mode, groups, grp_rows, T_PRE, OWN_T, T_PRE + OWN_T, nan_ws(len(rows), T_PRE + OWN_T, 2))
                q[tg] = q_t
                big = f(q)
                assert torch.equal(big[tg], alone.expand(len(tg), -1)), (plen, own, cpi, "among other groups and per-row rows")
                # the target's groups first (group 0 ...), no per-row rows, another shuffle, the module's own workspace
                rows, mode, groups, grp_rows, tg = scenes[1]
                q, f = run(rows, mode, groups, grp_rows, 640, 300, 0, None)
                q[tg] = q_t
                assert torch.equal(f(q)[tg], alone.expand(len(tg), -1)), (plen, own, cpi, "as the first groups")
                assert bool(torch.isfinite(big.float()).all())


# ------------------------------------------------------------------------------------------------ 2. per-row rows

def test_per_row_rows_are_decode_attention_bit_for_bit(dt, layout):
    """Rows of kind 0 - behind a prefix slot (wherever the cut lies) or without one - against ops.decode_attention on the same pools."""
    O = ops()
    H, Hkv = layout
    P = _pools(Hkv, dt, seed=17)
    pf = torch.full((6, Hkv, 2 * T_PRE, D), float("nan"), dtype=dt, device=DEV)
    O.prefix_fragments(P["kp"], P["vp"], pf, i32([0, 611, FILL_PLEN[2], FILL_PLEN[3], 611, FILL_PLEN[5]]))
    rows, mode, groups, grp_rows, _ = _scene(611, 65, False, False, 3)
    extra = [[8, n, ps, pl] for n, ps, pl in ((1, 0, 0), (63, 0, 0), (64, 0, 0), (65, 0, 0), (300, 0, 0), (37, 2, 36), (101, 2, 36), (64, 5, 63), (65, 5, 64),
                                              (129, 5, 65), (612, 3, 611), (911, 3, 611), (640, 1, 611), (700, 4, 640), (960, 4, 640), (2, 2, 1))]
    at = list(range(0, len(rows), len(rows) // len(extra)))[:len(extra)]
    for i, r in zip(reversed(at), reversed(extra)):                 # spread over the call
        rows.insert(i, r); mode.insert(i, 0)
        grp_rows = [m + 1 if m >= i else m for m in grp_rows]
    M = len(rows)
    q = torch.randn(M, H * D, generator=torch.Generator().manual_seed(5)).to(DEV, dt)
    rt = i32(rows)
    want = O.decode_attention(q, P["ko"], P["vo"], rt, H, Hkv, D, k_prefix=P["kp"], v_prefix=P["vp"], max_len=T_PRE + OWN_T)
    per_row = (i32(mode) == 0).nonzero().flatten()
    assert per_row.numel() == len(extra)
    for cpi in item_sizes():
        items = O.prefix_work_items(groups, cpi)
        got = O.decode_attention_shared_invariant(q, P["ko"], P["vo"], P["kp"], P["vp"], rt, i32(mode), i32(groups), i32(grp_rows), i32(items), len(items),
                                                  H, Hkv, D, 640, OWN_T, T_PRE + OWN_T, pf, chunks_per_item=cpi)
        assert torch.equal(got[per_row], want[per_row]), cpi
        assert not torch.equal(got, want)                            # (the shared rows take another arithmetic: P rounded for the MFMA)
    # a call of per-row rows only: no group, no item, no prefix pass
    only = rt[per_row].contiguous()
    z = i32([[0, 0, 0, 0]])
    got = O.decode_attention_shared_invariant(q[per_row].contiguous(), P["ko"], P["vo"], P["kp"], P["vp"], only, i32([0] * len(extra)), z, i32([0]), z, 0,
                                              H, Hkv, D, 0, 0, T_PRE + OWN_T, None)
    assert torch.equal(got, want[per_row])


# ------------------------------------------------------------------------------------------------ 3. census

def test_shared_invariant_census(dt, layout):
    """The grouped census of tests/test_attention_census_gpu.py on the new entry: groups of 1 / 15 / 16 / 17 / 33 rows on prefixes of
    1 ... 640 keys, every (group size, prefix length) pair, 1 / 2 / 4 / 16 chunks per item, own ranges of 1 ... 256 and 1 ... 300 keys
    (both through the own chunks + combine here).  Shared rows: the prefix pass rounds P to the storage type (p_roundings = 1); the two
    rows without a prefix are of the per-row kind (0).  Census launch: uniform / rising / falling rows; needle launch: the last prefix
    key, the first own key, the newest key and a walk over the context take turns over (row, head)."""
    O = ops()
    H, Hkv = layout
    scale = AC.f32(D ** -0.5)
    LB = TC.T_PRE + TC.OWN_T
    kc, vc = AC.census_context(Hkv, LB, D, dt, DEV, seed=31)
    needles = [AC.needle_context(Hkv, LB, D, dt, DEV, seed=40 + 2 * j) for j in range(6)]
    v_max = max(float(v.float().abs().max()) for _, v in needles)
    k_needles = torch.stack([k for k, _ in needles])
    k_cfg = 0
    for rot in range(len(TC.PLENS)):
        plens = [TC.PLENS[(rot + j) % len(TC.PLENS)] for j in range(5)]
        pool_sets, frags = {}, {}
        for name in ("census", "needle"):
            pools = TC.empty_pools(6, TC.OWN_T, 6, TC.T_PRE, Hkv, dt)
            for j in range(6):
                kk, vv = (kc, vc) if name == "census" else needles[j]
                pl = plens[j] if j < 5 else 0
                AC.put_context(kk[:, :pl + 300], vv[:, :pl + 300], pl, pools[0], pools[1], j, pools[2], pools[3], j + 1 if j < 5 else 0)
            pf = torch.full((6, Hkv, 2 * TC.T_PRE, D), float("nan"), dtype=dt, device=DEV)
            O.prefix_fragments(pools[2], pools[3], pf, i32([0] + plens))
            pool_sets[name], frags[name] = pools, pf
        for cpi in (1, 2, 4, 16):
            for max_own, modulo in ((256, 256), (TC.OWN_T, 300)):
                rows, groups, grp_rows = TC._group_rows(plens, k_cfg, modulo)
                M = len(rows)
                rt = i32(rows)
                n, pl_r = rt[:, 1].long(), rt[:, 3].long()
                pre = pl_r > 0
                items = O.prefix_work_items(groups, cpi)
                ridx = torch.arange(M, device=DEV)
                for name in ("census", "needle"):
                    pools = pool_sets[name]
                    if name == "census":
                        sign = torch.tensor([0.0, 1.0, -1.0], device=DEV)[(ridx + k_cfg) % 3]
                        q = AC.q_ramp(n, sign, H, D, dt, scale, DEV)
                    else:
                        walk = (ridx * 37 + k_cfg * 11) % n
                        tg = TC.cyc_targets(n, H, [(pl_r - 1).clamp(min=0), pl_r, n - 1, walk])
                        kvh = (torch.arange(H, device=DEV) // (H // Hkv))[None].expand(M, H)
                        q = (AC.NEEDLE_BETA * k_needles[rt[:, 0].long()[:, None].expand(M, H), kvh, tg].float()).to(dt)
                    got = O.decode_attention_shared_invariant(q.view(M, H * D), pools[0], pools[1], pools[2], pools[3], rt, pre.to(torch.int32).contiguous(),
                                                              i32(groups), i32(grp_rows), i32(items), len(items), H, Hkv, D, max(plens), max_own, max_own,
                                                              frags[name], chunks_per_item=cpi).view(M, H, D)
                    ref = torch.empty(M, H, D, dtype=torch.float64, device=DEV)
                    terms = torch.empty_like(ref) if name == "needle" else None
                    for j in range(6):
                        sel = (rt[:, 0] == j).nonzero().flatten()
                        pl = plens[j] if j < 5 else 0
                        k, v = AC.context_of(*pools, j, j + 1 if j < 5 else 0, pl, pl + 300)
                        ref[sel] = AC.reference(q[sel], k, v, n[sel])
                        if terms is not None:
                            terms[sel] = AC.reference(q[sel], k, v, n[sel], abs_v=True)
                    tag = f"shared-invariant {name} plens {plens} cpi {cpi} max_own {max_own} cfg {k_cfg}: (slot, len, pslot, plen) of the rows "
                    AC.assert_census(got[pre], ref[pre], dt, 1, v_max=v_max if name == "needle" else 1.0, terms64=None if terms is None else terms[pre],
                                     what=tag + str([r for r in rows if r[3]]))
                    AC.assert_census(got[~pre], ref[~pre], dt, 0, v_max=v_max if name == "needle" else 1.0, what=tag + str([r for r in rows if not r[3]]))
                k_cfg += 1


# ------------------------------------------------------------------------------------------------ 4. refusals

def test_refusals_return_invalid_arg_and_launch_nothing():
    from llava_align_amd import _lib
    O = ops()
    lib = O._lib_ready()
    H, Hkv, M = 8, 2, 3
    dt_ = torch.bfloat16
    ko, vo = torch.zeros(2, Hkv, 64, D, dtype=dt_, device=DEV), torch.zeros(2, Hkv, 64, D, dtype=dt_, device=DEV)
    kp, vp = torch.zeros(2, Hkv, 64, D, dtype=dt_, device=DEV), torch.zeros(2, Hkv, 64, D, dtype=dt_, device=DEV)
    pf = torch.zeros(2, Hkv, 128, D, dtype=dt_, device=DEV)
    q = torch.zeros(M, H * D, dtype=dt_, device=DEV)
    rows, mode = i32([[0, 40, 1, 30]] * M), i32([1] * M)
    groups, grp_rows, items = i32([[0, M, 1, 30]]), i32([0, 1, 2]), i32([[0, 0, 0, 0]])
    out = torch.full((M, H * D), 7.0, dtype=dt_, device=DEV)
    ws = torch.full((O.attention_workspace(M, H, D, 128, DEV).numel(),), 5.0, dtype=torch.float32, device=DEV)

    def call(**over):
        a = dict(q=q.data_ptr(), kc=ko.data_ptr(), vc=vo.data_ptr(), kp=kp.data_ptr(), vp=vp.data_ptr(), pf=pf.data_ptr(), rows=rows.data_ptr(),
                 mode=mode.data_ptr(), groups=groups.data_ptr(), grp=grp_rows.data_ptr(), items=items.data_ptr(), n_items=1, out=out.data_ptr(),
                 ws=ws.data_ptr(), M=M, H=H, Hkv=Hkv, D=D, ss=ko.stride(0), t=64, ps=kp.stride(0), pt=64, mp=30, mo=10, mr=0, cpi=1)
        a.update(over)
        return lib.vdd_decode_attention_shared_invariant(a["q"], a["kc"], a["vc"], a["kp"], a["vp"], a["pf"], a["rows"], a["mode"], a["groups"], a["grp"],
                                                         a["items"], a["n_items"], a["out"], a["ws"], a["M"], a["H"], a["Hkv"], a["D"], a["ss"], a["t"],
                                                         a["ps"], a["pt"], a["mp"], a["mo"], a["mr"], a["cpi"], D ** -0.5, _lib.VDD_BF16, None)
    bad = [dict(D=64), dict(cpi=0), dict(cpi=-1), dict(pf=None), dict(pt=100)]
    bad += [{k: None} for k in ("q", "kc", "vc", "kp", "vp", "rows", "mode", "groups", "grp", "items", "out", "ws")]
    for over in bad:
        assert call(**over) == -1, over
    torch.cuda.synchronize()
    # status only, nothing launched: neither the output nor the workspace was touched by the refused calls
    refused_out, refused_ws = out.clone(), ws.clone()
    assert call() == 0                                              # the same arguments, all valid, do run
    torch.cuda.synchronize()
    assert bool((refused_out == 7.0).all()) and not bool((out == 7.0).any())
    assert bool((refused_ws == 5.0).all())
    assert call(M=0, q=None) == 0                                   # an empty call is done before anything is looked at


# ------------------------------------------------------------------------------------------------ 5. engine (7B widths, 2 layers)

@pytest.fixture(scope="module")
def eng7():
    from test_engine_shapes_gpu import _engine
    return _engine(W7B, n_layers=2, vit_layers=2)


def _questions():
    """2 images x 6 questions; the SAME six question texts about both images, so that in the batch of 12 the `unk` rows with equal ids
    share all but their last position (engine._plan) and a question alone has nothing to share: the image-free rows' cut moves."""
    from test_engine_shapes_gpu import _prompts
    ids, imgs = _prompts(2, 6, 32000, seed=71)
    texts = [r[r.tolist().index(-200) + 1:] for r in ids[:6]]
    return [torch.cat([r[: r.tolist().index(-200) + 1], texts[i % 6]]) for i, r in enumerate(ids)], imgs


def _gen(eng, ids, imgs, sel, **kw):
    return eng.generate([ids[i] for i in sel], images=[imgs[i] for i in sel], cd_alpha=1.0, cd_beta=0.1, cd_greedy=True, output_scores=True,
                        max_new_tokens=8, use_dd_unk=True, temperature=0.2, **kw)


def _same(a, b, qa, qb):
    return torch.equal(a.tokens[qa], b.tokens[qb]) and all(torch.equal(sa[qa].view(torch.int16), sb[qb].view(torch.int16))
                                                           for sa, sb in zip(a.scores, b.scores))


def test_engine_decodes_a_question_the_same_alone_in_a_batch_and_shuffled(eng7):
    O = ops()
    eng = eng7
    ids, imgs = _questions()
    order = np.random.default_rng(3).permutation(12).tolist()
    with O.batch_invariant(shared_prefix=True):
        full = _gen(eng, ids, imgs, range(12))
        shuffled = _gen(eng, ids, imgs, order)
        alone = _gen(eng, ids, imgs, [4])
        lone_image = _gen(eng, ids, imgs, [4, 6, 7, 8, 9])          # question 4's image has no other user
    with O.batch_invariant():
        per_row = _gen(eng, ids, imgs, range(12))
    # the `unk` rows of the batch share their repeated texts (their cut lies one token before the end), alone they are cut behind <unk>
    assert full.stats["prefill_tokens"] < 2 * 611 + 12 * 30 + 6 * 70 and alone.stats["prefill_tokens"] >= 611 + 36
    for out, n_img in ((full, 2), (shuffled, 2), (alone, 1), (lone_image, 2)):
        assert out.stats["n_groups"] == n_img and out.stats["shared_rows"] == out.stats["decode_rows"] // 2 > 0
    assert all(_same(full, shuffled, q, order.index(q)) for q in range(12))
    assert _same(full, alone, 4, 0) and _same(full, lone_image, 4, 0)
    assert all(_same(full, lone_image, q, 1 + j) for j, q in enumerate((6, 7, 8, 9)))
    assert len({tuple(full.tokens[q].tolist()) for q in range(12)}) > 4
    # with the flag off: today's mode, nothing grouped
    assert per_row.stats["n_groups"] == 0 and per_row.stats["shared_rows"] == 0
    # against the per-row mode (the bound tuned against invariant is held to, test_batch_invariant_gpu.py): the first tokens agree
    assert (full.tokens[:, 0] == per_row.tokens[:, 0]).float().mean().item() >= 0.9


# ------------------------------------------------------------------------------------------------ 6. against the per-row mode, 7. generate_list

@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def tiny(request):
    from llava_align_amd.engine import LlavaWeights, VddLlavaEngine, preset
    cfg = preset("tiny")
    w = LlavaWeights.random(cfg, DEV, seed=3, std=0.06, dtype=request.param)
    return VddLlavaEngine(cfg, weights=w, device=DEV, t_max=256, use_graph=False)


def test_shared_form_agrees_with_the_per_row_form_to_rounding(tiny):
    """Same checks, same bounds as test_engine_gpu.test_prefix_sharing_is_transparent (scores within 0.2: the MFMA pass rounds P to the
    storage type, x6 contrast gain; a token may differ only on a near-tie) and the first tokens of at least 0.9 of the questions."""
    from test_engine_gpu import prompts
    O = ops()
    ids, imgs = prompts(n_img=2, per_img=6, seed=5)
    kw = dict(images=imgs, cd_alpha=1.0, cd_beta=0.1, temperature=0.5, max_new_tokens=5, cd_greedy=True, output_scores=True, use_dd=True, use_dd_unk=True)
    with O.batch_invariant(shared_prefix=True):
        a = tiny.generate(ids, **kw)
    with O.batch_invariant():
        b = tiny.generate(ids, **kw)
    assert a.stats["n_groups"] == 2 and a.stats["shared_rows"] == 12 and b.stats["n_groups"] == 0
    tol, agree = 0.2, 0
    for q in range(len(ids)):
        for step, (sa, sb) in enumerate(zip(a.scores, b.scores)):
            fin = torch.isfinite(sa[q]) & torch.isfinite(sb[q])
            assert (sa[q][fin].float() - sb[q][fin].float()).abs().max().item() <= tol, (q, step)
            top2 = torch.topk(sa[q].float(), 2).values
            if (top2[0] - top2[1]).item() > 2 * tol:
                assert a.tokens[q, step] == b.tokens[q, step], (q, step)
            if a.tokens[q, step] != b.tokens[q, step]:
                break
            agree += 1
    assert agree >= 4 * len(ids)
    assert (a.tokens[:, 0] == b.tokens[:, 0]).float().mean().item() >= 0.9
    assert (a.tokens[:, 1] == b.tokens[:, 1]).float().mean().item() >= 0.9       # (column 0 is sampled from the prefill: the first DECODED token too)


def test_generate_list_refuses_the_flag(tiny):
    from test_engine_gpu import prompts
    O = ops()
    ids, imgs = prompts(n_img=1, per_img=2, seed=5)
    kw = dict(in_flight=2, max_new_tokens=3, eos_token_id=2, pad_token_id=0, cd_greedy=True, temperature=0.5)
    with O.batch_invariant(shared_prefix=True):
        with pytest.raises(ValueError, match="INVARIANT_SHARED_PREFIX"):
            tiny.generate_list(ids, imgs, **kw)
    with O.batch_invariant():                                       # flag off: as ever
        assert tiny.generate_list(ids, imgs, **kw).tokens.shape[0] == 2
    old = O.INVARIANT_SHARED_PREFIX
    try:
        O.INVARIANT_SHARED_PREFIX = True                            # outside the mode the flag means nothing
        assert tiny.generate_list(ids, imgs, **kw).tokens.shape[0] == 2
    finally:
        O.INVARIANT_SHARED_PREFIX = old


# ------------------------------------------------------------------------------------------------ 8. the driver

def test_run_pope_with_the_option_writes_the_same_answers_at_two_batch_sizes(eng7, tmp_path):
    from llava_align_amd.pope_driver import run_pope
    from test_engine_shapes_gpu import _prompts
    eng = eng7
    ids, imgs = _prompts(3, 6, 32000, seed=5, image=336)
    images = {f"im{i}.jpg": imgs[6 * i] for i in range(3)}
    by_text = {f"q{i}": ids[i].tolist() for i in range(18)}
    qs = [{"question_id": i, "image": f"im{i // 6}.jpg", "text": f"q{i}", "label": ("yes", "no")[i % 2]} for i in range(18)]
    enc = lambda text, with_image: by_text[text] if with_image else [t for t in by_text[text] if t != -200]
    dec = lambda t: " ".join(map(str, t))
    kw = dict(unk_token_id=0, pad_token_id=0, eos_token_id=None, max_new_tokens=8, stop_str=None, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1,
              temperature=0.5, cd_greedy=True, invariant_shared_prefix=True)
    shared_rows, generate = [], eng.generate

    def spy(*a, **k):
        out = generate(*a, **k)
        shared_rows.append(out.stats["shared_rows"])
        return out
    eng.generate = spy
    try:
        a = run_pope(eng, qs, enc, dec, lambda n: images[n], batch_questions=18, answers_path=str(tmp_path / "a.jsonl"), **kw)
        b = run_pope(eng, qs, enc, dec, lambda n: images[n], batch_questions=4, answers_path=str(tmp_path / "b.jsonl"), **kw)
    finally:
        del eng.generate
    assert a["batch_invariant"] and b["batch_invariant"] and max(shared_rows) > 0
    fa, fb = (tmp_path / "a.jsonl").read_bytes(), (tmp_path / "b.jsonl").read_bytes()
    assert len(fa) > 0 and fa == fb
    assert not ops().GEMM_BATCH_INVARIANT and not ops().INVARIANT_SHARED_PREFIX
