"""Key census of every attention entry of llava_align_amd.ops: structured inputs (tests/attention_census.py) on which one missing,
doubled, misplaced or mis-masked key, or one wrong merge of online-softmax partials, moves the output by a large factor, checked
against an fp64 reference of the same operation on the same stored inputs with a rounding-sized bound (assert_census), in bf16 and
fp16, for the head layouts (H, Hkv) = (8, 8), (8, 2), (32, 32), (40, 40), (32, 8).

Reads do not conflict, so the rows of one launch share slots: one launch sweeps every context length, or every needle position.
Only the one-launch fused decode writes (the new token's K / V), so its rows get slots of their own; the new token is given the
K / V its slot already holds at that index, which keeps the slots equal to the logical context from launch to launch."""
import pytest
import torch

import attention_census as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
LMAX = 704
T_PRE = 640
PLENS = [1, 36, 63, 64, 65, 611, 640]
LAYOUTS = [(8, 8), (8, 2), (32, 32), (40, 40), (32, 8)]


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def dt(request):
    return request.param


@pytest.fixture(params=LAYOUTS, ids=[f"H{h}kv{k}" for h, k in LAYOUTS])
def layout(request):
    return request.param


def ops():
    from llava_align_amd import ops as O
    return O


def empty_pools(n_own, t_own, n_pre, t_pre, Hkv, dtype, Dm=D):
    """K = 0.5, V = POISON everywhere: whatever is read outside a context that put_context() wrote shows in the output"""
    k_own = torch.full((n_own, Hkv, t_own, Dm), 0.5, dtype=dtype, device=DEV)
    k_pre = torch.full((n_pre, Hkv, t_pre, Dm), 0.5, dtype=dtype, device=DEV)
    return k_own, torch.full_like(k_own, AC.POISON), k_pre, torch.full_like(k_pre, AC.POISON)


def i32(x):
    return torch.as_tensor(x, dtype=torch.int32, device=DEV).contiguous()


def rows_of(slot, n, pslot, plen):
    n = torch.as_tensor(n, device=DEV)
    return torch.stack([torch.full_like(n, slot), n, torch.full_like(n, pslot), torch.full_like(n, plen)], 1).to(torch.int32).contiguous()


def tail_targets(n, H):
    """[R, H]: head h of the row with n keys aims at key n-1-h (head 0: the newest key), wrapped into the row's keys"""
    n = torch.as_tensor(n, device=DEV)
    return (n[:, None] - 1 - torch.arange(H, device=DEV)[None, :]) % n[:, None]


def cyc_targets(n, H, choices):
    """[R, H]: (row, head) takes choices[(row + head) % len(choices)] (each a scalar or [R]), wrapped into the row's keys"""
    n = torch.as_tensor(n, device=DEV)
    R = n.numel()
    sel = (torch.arange(R, device=DEV)[:, None] + torch.arange(H, device=DEV)[None, :]) % len(choices)
    tg = torch.zeros(R, H, dtype=torch.long, device=DEV)
    for i, c in enumerate(choices):
        tg = torch.where(sel == i, torch.as_tensor(c, device=DEV).long().expand(R)[:, None].expand(R, H), tg)
    return tg % n[:, None]


# ------------------------------------------------------------------------------------------------ split-KV decode, contiguous and paged

def _paged(k_own, v_own, slot, n_tok, seed):
    """the first n_tok tokens of own slot `slot` behind a shuffled page table (3 table rows, the slot's own row in the middle);
    pages nobody holds keep K = 0.5, V = POISON"""
    from llava_align_amd.paged_kv import PAGE
    Hkv, Dm = k_own.shape[1], k_own.shape[3]
    held = -(-n_tok // PAGE)
    n_pages = held + 9
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    table = torch.full((3, held + 2), -1, dtype=torch.int32)
    pk = torch.full((n_pages, Hkv, PAGE, Dm), 0.5, dtype=k_own.dtype, device=DEV)
    pv = torch.full_like(pk, AC.POISON)
    for j in range(held):
        pg = perm.pop()
        table[slot, j] = pg
        m = min(PAGE, k_own.shape[2] - j * PAGE)
        pk[pg, :, :m], pv[pg, :, :m] = k_own[slot, :, j * PAGE:j * PAGE + m], v_own[slot, :, j * PAGE:j * PAGE + m]
    return pk, pv, table.to(DEV)


def _run_decode(form, q, pools, rows, H, Hkv, max_len, n_own_tok):
    O = ops()
    k_own, v_own, k_pre, v_pre = pools
    M = q.shape[0]
    q2 = q.reshape(M, H * D).contiguous()
    if form == "contiguous":
        return O.decode_attention(q2, k_own, v_own, rows, H, Hkv, D, k_prefix=k_pre, v_prefix=v_pre, max_len=max_len).view(M, H, D)
    pk, pv, table = _paged(k_own, v_own, 1, n_own_tok, seed=n_own_tok)
    ws = O.attention_workspace(M, H, D, max_len, DEV)
    return O.decode_attention_paged(q2, pk, pv, table, rows, H, Hkv, D, k_pre, v_pre, max_len, ws).view(M, H, D)


@pytest.mark.parametrize("form", ["contiguous", "paged"])
def test_decode_attention_census(form, dt, layout):
    """decode_attention / decode_attention_paged (split-KV chunks + combine, P in fp32: p_roundings = 0).  Per prefix length (none, then
    1 ... 640 keys in a separate prefix pool) one census launch - a uniform row, a rising and a falling ramp row for EVERY length up to
    704 - and one needle launch: the newest keys of every length (head h aims at key len-1-h), and every position of a 700-key context.
    Paged: the own range behind a shuffled page table, so every length ends inside, on and one past a 16-token page edge."""
    H, Hkv = layout
    scale = AC.f32(D ** -0.5)
    kc, vc = AC.census_context(Hkv, LMAX, D, dt, DEV, seed=11)
    kn, vn = AC.needle_context(Hkv, LMAX, D, dt, DEV, seed=12)
    v_max = float(vn.float().abs().max())
    for plen in [0] + PLENS:
        n = torch.arange(plen + 1, LMAX + 1, device=DEV)
        R = n.numel()
        max_len = LMAX if plen != 36 else LMAX + 64                    # once with an always-empty trailing chunk
        # census launch
        pools = empty_pools(3, LMAX - plen + 8, 3, T_PRE, Hkv, dt)
        AC.put_context(kc, vc, plen, pools[0], pools[1], 1, pools[2], pools[3], 2)
        q = torch.cat([AC.q_uniform(R, H, D, dt, DEV), AC.q_ramp(n, torch.ones(R), H, D, dt, scale, DEV),
                       AC.q_ramp(n, -torch.ones(R), H, D, dt, scale, DEV)])
        n3 = torch.cat([n, n, n])
        got = _run_decode(form, q, pools, rows_of(1, n3, 2, plen), H, Hkv, max_len, LMAX - plen)
        k, v = AC.context_of(*pools, 1, 2, plen, LMAX)
        ref = AC.reference(q, k, v, n3)
        assert (ref[:R] - AC.census_expected(n, D)[:, None, :]).abs().max().item() < 1e-12
        AC.assert_census(got[:R], ref[:R], dt, 0, what=f"{form} uniform plen {plen}: row r = len {plen + 1} + r")
        AC.assert_census(got[R:], ref[R:], dt, 0, what=f"{form} ramp plen {plen}: rows up then down, row r = len {plen + 1} + r % {R}")
        # needle launch
        pools = empty_pools(3, LMAX - plen + 8, 3, T_PRE, Hkv, dt)
        AC.put_context(kn, vn, plen, pools[0], pools[1], 1, pools[2], pools[3], 2)
        tg, nn = [tail_targets(n, H)], [n]
        if plen < 700:
            sw = AC.needle_sweep_targets(700, H, DEV)
            tg.append(sw); nn.append(torch.full((sw.shape[0],), 700, device=DEV))
        tg, nn = torch.cat(tg), torch.cat(nn)
        q = AC.q_needle(kn, tg, H)
        got = _run_decode(form, q, pools, rows_of(1, nn, 2, plen), H, Hkv, max_len, LMAX - plen)
        k, v = AC.context_of(*pools, 1, 2, plen, LMAX)
        AC.assert_census(got, AC.reference(q, k, v, nn), dt, 0, v_max=v_max,
                         what=f"{form} needle plen {plen}: rows < {R} newest keys of len {plen + 1} + r, then the sweep at 700")


# ------------------------------------------------------------------------------------------------ one-launch fused decode

FUSED_SLOTS = 176       # rows per launch, each with a slot of its own (704 lengths = 4 launches)


def _run_fused(q, k_ctx, v_ctx, n, plen, pools, H, Hkv, n_split, relaunch):
    """rows (slot r % FUSED_SLOTS, len n[r] counting the new token) in launches of FUSED_SLOTS; the new token of a row carries the K / V
    of key n-1 of the context; identity cos / sin table"""
    O = ops()
    k_own, v_own, k_pre, v_pre = pools
    M = q.shape[0]
    cs = torch.zeros(LMAX + 1, D // 2, 2, dtype=torch.float32, device=DEV)
    cs[..., 0] = 1
    qkv = torch.cat([q.reshape(M, H * D), k_ctx[:, n - 1].transpose(0, 1).reshape(M, Hkv * D), v_ctx[:, n - 1].transpose(0, 1).reshape(M, Hkv * D)], 1).contiguous()
    out = torch.empty(M, H, D, dtype=q.dtype, device=DEV)
    for b0 in range(0, M, FUSED_SLOTS):
        b1 = min(M, b0 + FUSED_SLOTS)
        nb = n[b0:b1]
        slot = torch.arange(b1 - b0, device=DEV)
        rows = torch.stack([slot, nb, torch.full_like(nb, 2), torch.full_like(nb, plen)], 1).to(torch.int32).contiguous()
        args = (qkv[b0:b1].contiguous(), i32(nb - 1), i32(nb - 1 - plen), i32(slot), cs, k_own, v_own, rows, H, Hkv, D)
        o = O.decode_attention_fused(*args, k_prefix=k_pre, v_prefix=v_pre, n_split=n_split)
        if b0 == 0:
            for _ in range(relaunch):                                   # tickets back at zero, merge order fixed: the same bits again
                assert torch.equal(O.decode_attention_fused(*args, k_prefix=k_pre, v_prefix=v_pre, n_split=n_split), o)
        out[b0:b1] = o.view(b1 - b0, H, D)
    return out


@pytest.mark.parametrize("n_split", [1, 2, 4])
def test_decode_attention_fused_census(n_split, dt, layout):
    """decode_attention_fused (16 waves x 4 lane groups per (row, head), old keys cut over 1 / 2 / 4 workgroups, the new token attended
    from registers; P in fp32: p_roundings = 0).  Without a prefix and behind 1 ... 640 prefix keys: the uniform census for every old-key
    count, ramps up and down, needles on the new token itself / the last old key / old key 0 for every length, and on every position of
    a 700-key context.  The first launch of each sweep is repeated and must give the same bits; the slots must come out unchanged."""
    H, Hkv = layout
    scale = AC.f32(D ** -0.5)
    kc, vc = AC.census_context(Hkv, LMAX, D, dt, DEV, seed=21)
    kn, vn = AC.needle_context(Hkv, LMAX, D, dt, DEV, seed=22)
    v_max = float(vn.float().abs().max())
    for plen in [0] + PLENS:
        n = torch.arange(plen + 1, LMAX + 1, device=DEV)                # len counts the new token: old keys plen .. 703
        R = n.numel()
        for ctx_name, (k_ctx, v_ctx) in (("census", (kc, vc)), ("needle", (kn, vn))):
            k_own, v_own, k_pre, v_pre = empty_pools(1, LMAX - plen + 8, 3, T_PRE, Hkv, dt)
            AC.put_context(k_ctx, v_ctx, plen, k_own, v_own, 0, k_pre, v_pre, 2)
            k_own, v_own = k_own.expand(FUSED_SLOTS, -1, -1, -1).contiguous(), v_own.expand(FUSED_SLOTS, -1, -1, -1).contiguous()
            pools = (k_own, v_own, k_pre, v_pre)
            before = (k_own[0].clone(), v_own[0].clone())
            if ctx_name == "census":
                q = torch.cat([AC.q_uniform(R, H, D, dt, DEV), AC.q_ramp(n, torch.ones(R), H, D, dt, scale, DEV),
                               AC.q_ramp(n, -torch.ones(R), H, D, dt, scale, DEV)])
                nn = torch.cat([n, n, n])
            else:
                tg = [cyc_targets(n, H, [n - 1, n - 2, torch.zeros_like(n)])]
                nn = [n]
                if plen < 699:
                    sw = AC.needle_sweep_targets(700, H, DEV)
                    tg.append(sw); nn.append(torch.full((sw.shape[0],), 700, device=DEV))
                tg, nn = torch.cat(tg), torch.cat(nn)
                q = AC.q_needle(k_ctx, tg, H)
            got = _run_fused(q, k_ctx, v_ctx, nn, plen, pools, H, Hkv, n_split, relaunch=3)
            assert bool((k_own == before[0][None]).all()) and bool((v_own == before[1][None]).all()), "a launch changed its slots"
            k, v = AC.context_of(k_own, v_own, k_pre, v_pre, 0, 2, plen, LMAX)
            ref = AC.reference(q, k, v, nn)
            if ctx_name == "census":
                AC.assert_census(got[:R], ref[:R], dt, 0, what=f"fused/{n_split} uniform plen {plen}: row r = {plen} + r old keys")
                AC.assert_census(got[R:], ref[R:], dt, 0, what=f"fused/{n_split} ramp plen {plen}: up then down, row r = {plen} + r % {R} old keys")
            else:
                AC.assert_census(got, ref, dt, 0, v_max=v_max,
                                 what=f"fused/{n_split} needle plen {plen}: rows < {R} (new token | last old key | key 0) at len {plen + 1} + r, then the sweep at 700")


# ------------------------------------------------------------------------------------------------ grouped MFMA prefix pass + own pass

GROUP_SIZES = [1, 15, 16, 17, 33]
OWN_T = 320


def _group_rows(plens, k, modulo):
    """(rows [M, 4] as a list, groups, group_rows) in a shuffled row order: group j has GROUP_SIZES[j] rows on prefix slot j + 1 / own
    slot j; two rows without a prefix on own slot 5.  Own length of logical row i: 1 + (i + 84 k) % modulo."""
    rows, groups, grp = [], [], []
    for j, (gs, pl) in enumerate(zip(GROUP_SIZES, plens)):
        groups.append([len(grp), gs, j + 1, pl])
        for _ in range(gs):
            grp.append(len(rows))
            rows.append([j, pl + 1 + (len(rows) + 84 * k) % modulo, j + 1, pl])
    for _ in range(2):
        rows.append([5, 1 + (len(rows) + 84 * k) % modulo, 0, 0])
    perm = torch.randperm(len(rows), generator=torch.Generator().manual_seed(k)).tolist()
    inv = {old: new for new, old in enumerate(perm)}
    return [rows[o] for o in perm], groups, [inv[r] for r in grp]


def test_decode_attention_grouped_census(dt, layout):
    """decode_attention_grouped: groups of 1 / 15 / 16 / 17 / 33 rows (one MFMA row tile, its edges, three tiles) on prefixes of
    1 ... 640 keys - every (group size, prefix length) pair as the prefix lengths rotate through the groups - with 1 / 2 / 4 / 16 chunks
    per work item, own ranges of 1 ... 256 keys through the one-wave own-merge kernel and 1 ... 300 through own split + combine.  The
    prefix pass rounds P to the storage type before P V (p_roundings = 1); the two rows without a prefix never meet it (0).
    Census launch: the rows take turns as uniform / rising / falling; needle launch: the last prefix key, the first own key, the
    newest key and a walk over the context take turns over (row, head)."""
    O = ops()
    H, Hkv = layout
    scale = AC.f32(D ** -0.5)
    LB = T_PRE + OWN_T
    kc, vc = AC.census_context(Hkv, LB, D, dt, DEV, seed=31)
    needles = [AC.needle_context(Hkv, LB, D, dt, DEV, seed=40 + 2 * j) for j in range(6)]
    v_max = max(float(v.float().abs().max()) for _, v in needles)
    k_needles = torch.stack([k for k, _ in needles])
    k_cfg = 0
    for rot in range(len(PLENS)):
        plens = [PLENS[(rot + j) % len(PLENS)] for j in range(5)]
        pool_sets, frags = {}, {}
        for name in ("census", "needle"):
            pools = empty_pools(6, OWN_T, 6, T_PRE, Hkv, dt)
            for j in range(6):
                kk, vv = (kc, vc) if name == "census" else needles[j]
                pl = plens[j] if j < 5 else 0
                AC.put_context(kk[:, :pl + 300], vv[:, :pl + 300], pl, pools[0], pools[1], j, pools[2], pools[3], j + 1 if j < 5 else 0)
            pf = torch.full((6, Hkv, 2 * T_PRE, D), float("nan"), dtype=dt, device=DEV)       # chunks behind a prefix stay NaN: never read
            O.prefix_fragments(pools[2], pools[3], pf, i32([0] + plens))
            pool_sets[name], frags[name] = pools, pf
        for cpi in (1, 2, 4, 16):
            for max_own, modulo in ((256, 256), (OWN_T, 300)):            # own-merge kernel | own split + combine
                rows, groups, grp_rows = _group_rows(plens, k_cfg, modulo)
                M = len(rows)
                rt = i32(rows)
                n, pl_r = rt[:, 1].long(), rt[:, 3].long()
                items = O.prefix_work_items(groups, cpi)
                ridx = torch.arange(M, device=DEV)
                for name in ("census", "needle"):
                    pools = pool_sets[name]
                    if name == "census":
                        sign = torch.tensor([0.0, 1.0, -1.0], device=DEV)[(ridx + k_cfg) % 3]
                        q = AC.q_ramp(n, sign, H, D, dt, scale, DEV)                   # sign 0: the uniform census
                    else:
                        walk = (ridx * 37 + k_cfg * 11) % n
                        tg = cyc_targets(n, H, [(pl_r - 1).clamp(min=0), pl_r, n - 1, walk])
                        kvh = (torch.arange(H, device=DEV) // (H // Hkv))[None].expand(M, H)
                        q = (AC.NEEDLE_BETA * k_needles[rt[:, 0].long()[:, None].expand(M, H), kvh, tg].float()).to(dt)      # each row's own context
                    got = O.decode_attention_grouped(q.view(M, H * D), pools[0], pools[1], pools[2], pools[3], rt, i32(groups), i32(grp_rows),
                                                     i32(items), len(items), H, Hkv, D, max(plens), max_own, prefix_frag=frags[name],
                                                     chunks_per_item=cpi).view(M, H, D)
                    ref = torch.empty(M, H, D, dtype=torch.float64, device=DEV)
                    terms = torch.empty_like(ref) if name == "needle" else None                                       # see assert_census
                    for j in range(6):
                        sel = (rt[:, 0] == j).nonzero().flatten()
                        pl = plens[j] if j < 5 else 0
                        k, v = AC.context_of(*pools, j, j + 1 if j < 5 else 0, pl, pl + 300)
                        ref[sel] = AC.reference(q[sel], k, v, n[sel])
                        if terms is not None:
                            terms[sel] = AC.reference(q[sel], k, v, n[sel], abs_v=True)
                    pre = pl_r > 0
                    tag = f"grouped {name} plens {plens} cpi {cpi} max_own {max_own} cfg {k_cfg}: (slot, len, pslot, plen) of the rows "
                    AC.assert_census(got[pre], ref[pre], dt, 1, v_max=v_max if name == "needle" else 1.0, terms64=None if terms is None else terms[pre], what=tag + str([r for r in rows if r[3]]))
                    AC.assert_census(got[~pre], ref[~pre], dt, 0, v_max=v_max if name == "needle" else 1.0, what=tag + str([r for r in rows if not r[3]]))
                k_cfg += 1


# ------------------------------------------------------------------------------------------------ prefill: flash, packed flash, the map

FLASH_TQ = [1, 31, 32, 33, 127, 128, 129, 300, 577]
# (Tq, pos0, plen) behind a prefix: 64-key tiles straddle the two pools at 36 and 611 keys; one chunked prefill (pos0 > plen)
FLASH_PRE = [(30, 611, 611), (65, 611, 611), (130, 36, 36), (40, 50, 36), (129, 64, 64), (32, 1, 1)]
FLASH_LB = 800


def _flash_case(ctx, Hkv, Dm, dtype, own_off):
    """pools + [(q_row0, Tq, pos0, slot, pslot, plen)]: the prefix-free sequences share own slot 1, those behind a prefix of p keys the
    own slot / prefix slot of that p"""
    k_ctx, v_ctx = ctx
    plens = sorted({s[2] for s in FLASH_PRE})
    pools = empty_pools(2 + len(plens), FLASH_LB + own_off, 1 + len(plens), T_PRE, Hkv, dtype, Dm)
    AC.put_context(k_ctx[:, :600], v_ctx[:, :600], 0, pools[0], pools[1], 1, pools[2], pools[3], 0, own_off)
    for i, p in enumerate(plens):
        AC.put_context(k_ctx[:, :p + 150], v_ctx[:, :p + 150], p, pools[0], pools[1], 2 + i, pools[2], pools[3], 1 + i, own_off)
    seqs, r = [], 0
    for tq in FLASH_TQ:
        seqs.append((r, tq, 0, 1, 0, 0)); r += tq
    for tq, pos0, p in FLASH_PRE:
        seqs.append((r, tq, pos0, 2 + plens.index(p), 1 + plens.index(p), p)); r += tq
    return pools, seqs, r


# (D, keys per head actually used, causal, scale, own_row_offset): the CLIP / LLM shapes, the Qwen-ViT layout (40-dim heads padded to 64
# with zeros and scale = 40 ** -0.5), a scale override at 128, own keys that start 5 rows into their slots
FLASH_VARIANTS = [(128, None, True, None, 0), (128, None, False, None, 0), (128, None, True, None, 5), (128, None, True, 0.05, 0),
                  (64, None, True, None, 0), (64, None, False, None, 0), (64, 40, False, 40 ** -0.5, 0), (64, 40, True, 40 ** -0.5, 0)]


@pytest.mark.parametrize("Dm,d_used,causal,scale,own_off", FLASH_VARIANTS,
                         ids=[f"D{v[0]}{'' if v[1] is None else 'of' + str(v[1])}-{'causal' if v[2] else 'full'}{'-scale' if v[3] else ''}{'-off' if v[4] else ''}" for v in FLASH_VARIANTS])
def test_flash_attention_census(Dm, d_used, causal, scale, own_off, dt, layout):
    """flash_attention (128-query blocks, 64-key tiles, P rounded to the storage type before P V: p_roundings = 1).  One launch per
    pattern holds sequences of 1 ... 577 query rows without a prefix and sequences behind prefixes of 1 / 36 / 64 / 611 keys.  Uniform:
    every causal row's own key count exactly.  Needle: the diagonal key, key 0 and a walk over the row's keys take turns over (row, head).
    Ramp: rows take turns rising and falling."""
    O = ops()
    H, Hkv = layout
    sc = AC.f32(Dm ** -0.5 if scale is None else scale)
    beta = AC.NEEDLE_BETA * (2.0 if d_used else 1.0)                       # 40 used dims: |K|^2 = 40, keep the needle's margin
    census = AC.census_context(Hkv, FLASH_LB, Dm, dt, DEV, seed=51, d_used=d_used)
    needle = AC.needle_context(Hkv, FLASH_LB, Dm, dt, DEV, seed=52, d_used=d_used)
    for name in ("uniform", "ramp", "needle"):
        ctx = needle if name == "needle" else census
        pools, seqs, Ttot = _flash_case(ctx, Hkv, Dm, dt, own_off)
        n = torch.cat([AC.flash_counts(s[1], s[2], causal, DEV) for s in seqs])
        ridx = torch.arange(Ttot, device=DEV)
        if name == "uniform":
            q = AC.q_uniform(Ttot, H, Dm, dt, DEV)
        elif name == "ramp":
            q = AC.q_ramp(n, torch.where(ridx % 2 == 0, 1.0, -1.0), H, Dm, dt, sc, DEV)
        else:
            q = AC.q_needle(ctx[0], cyc_targets(n, H, [n - 1, torch.zeros_like(n), (ridx * 29) % n]), H, beta=beta)
        got = O.flash_attention(q.view(Ttot, H * Dm), pools[0], pools[1], i32(seqs), len(seqs), max(s[1] for s in seqs), H, Hkv, Dm,
                                causal=causal, k_prefix=pools[2], v_prefix=pools[3], scale=scale, own_row_offset=own_off).view(Ttot, H, Dm)
        for (r0, tq, pos0, slot, pslot, plen) in seqs:
            k, v = AC.context_of(*pools, slot, pslot, plen, pos0 + tq, own_off)
            ref = AC.reference(q[r0:r0 + tq], k, v, n[r0:r0 + tq], scale=sc)
            if name == "uniform":
                assert (ref - AC.census_expected(n[r0:r0 + tq], Dm, d_used)[:, None, :]).abs().max().item() < 1e-12
            terms = AC.reference(q[r0:r0 + tq], k, v, n[r0:r0 + tq], scale=sc, abs_v=True) if name == "needle" else None     # see assert_census
            AC.assert_census(got[r0:r0 + tq], ref, dt, 1, v_max=float(ctx[1].float().abs().max()), terms64=terms,
                             what=f"flash {name}: sequence (Tq {tq}, pos0 {pos0}, plen {plen}), row i sees {'pos0 + i + 1' if causal else pos0 + tq} keys")


def test_flash_attention_packed_census(dt, layout):
    """flash_attention_packed: packs of 1 - 4 sequences of 1 ... 32 query rows behind prefixes of 611 / 36 / 100 keys and without one;
    every sequence in an own slot of its own (random K / V per slot in the needle launch: a wave that walks a neighbour's slot shows)."""
    O = ops()
    H, Hkv = layout
    scale = AC.f32(D ** -0.5)
    PL = [611, 36, 100, 0]
    census = AC.census_context(Hkv, T_PRE + 32, D, dt, DEV, seed=61)
    pre_needle = [AC.needle_context(Hkv, T_PRE, D, dt, DEV, seed=62 + 2 * i) for i in range(4)]
    seqs, packs, r = [], [], 0
    for i, p in enumerate(PL):
        first = len(seqs)
        for tq in range(1, 33):
            seqs.append((r, tq, p, len(seqs), i, p)); r += tq
        s, size = first, 1
        while s < len(seqs):
            members = list(range(s, min(s + size, len(seqs))))
            packs.append(members + [-1] * (4 - len(members)))
            s += len(members); size = size % 4 + 1
    Ttot = r
    n = torch.cat([AC.flash_counts(s[1], s[2], True, DEV) for s in seqs])
    ridx = torch.arange(Ttot, device=DEV)
    for name in ("uniform", "ramp", "needle"):
        pools = empty_pools(len(seqs), 40, 4, T_PRE, Hkv, dt)
        ctxs = []
        for (r0, tq, pos0, slot, pslot, plen) in seqs:
            if name == "needle":
                own = AC.needle_context(Hkv, 32, D, dt, DEV, seed=1000 + slot)
                kk, vv = torch.cat([pre_needle[pslot][0][:, :plen], own[0]], 1), torch.cat([pre_needle[pslot][1][:, :plen], own[1]], 1)
            else:
                kk, vv = census[0][:, :plen + 32], census[1][:, :plen + 32]
            AC.put_context(kk, vv, plen, pools[0], pools[1], slot, pools[2], pools[3], pslot)
            ctxs.append(kk)
        if name == "uniform":
            q = AC.q_uniform(Ttot, H, D, dt, DEV)
        elif name == "ramp":
            q = AC.q_ramp(n, torch.where(ridx % 2 == 0, 1.0, -1.0), H, D, dt, scale, DEV)
        else:
            tg = cyc_targets(n, H, [n - 1, torch.zeros_like(n), (ridx * 29) % n])
            q = torch.cat([AC.q_needle(ctxs[i], tg[s[0]:s[0] + s[1]], H) for i, s in enumerate(seqs)])
        got = O.flash_attention_packed(q.view(Ttot, H * D), pools[0], pools[1], i32(seqs), i32(packs), len(packs), H, Hkv, D,
                                       k_prefix=pools[2], v_prefix=pools[3]).view(Ttot, H, D)
        v_max = max(float(pools[1][:, :, :32].float().abs().max()), *(float(v.float().abs().max()) for _, v in pre_needle)) if name == "needle" else 1.0
        for (r0, tq, pos0, slot, pslot, plen) in seqs:
            k, v = AC.context_of(*pools, slot, pslot, plen, pos0 + tq)
            terms = AC.reference(q[r0:r0 + tq], k, v, n[r0:r0 + tq], abs_v=True) if name == "needle" else None               # see assert_census
            AC.assert_census(got[r0:r0 + tq], AC.reference(q[r0:r0 + tq], k, v, n[r0:r0 + tq]), dt, 1, v_max=v_max, terms64=terms,
                             what=f"packed flash {name}: sequence {slot} (Tq {tq}, plen {plen}), pack {[p for p in packs if slot in p][0]}")


def test_attention_probs_census(dt, layout):
    """attention_probs: with q = 0 the map is exactly 1 / (pos0 + i + 1) up to the diagonal and zero behind it; sequences of more than
    128 keys, behind a prefix, without one, and continuing past it (pos0 > plen).  The map is one fp32 softmax rounded once:
    p_roundings = 0, max|V| = 1 (a probability)."""
    O = ops()
    H, Hkv = layout
    scale = AC.f32(D ** -0.5)
    census = AC.census_context(Hkv, FLASH_LB, D, dt, DEV, seed=71)
    needle = AC.needle_context(Hkv, FLASH_LB, D, dt, DEV, seed=72)
    for (tq, pos0, plen) in [(200, 37, 37), (150, 0, 0), (70, 611, 611), (100, 50, 36)]:
        n = AC.flash_counts(tq, pos0, True, DEV)
        Tk = pos0 + tq
        ridx = torch.arange(tq, device=DEV)
        for name in ("uniform", "ramp", "needle"):
            ctx = needle if name == "needle" else census
            pools = empty_pools(5, 320, 3, T_PRE, Hkv, dt)
            AC.put_context(ctx[0][:, :Tk], ctx[1][:, :Tk], plen, pools[0], pools[1], 4, pools[2], pools[3], 1)
            if name == "uniform":
                qs = AC.q_uniform(tq, H, D, dt, DEV)
            elif name == "ramp":
                qs = AC.q_ramp(n, torch.where(ridx % 2 == 0, 1.0, -1.0), H, D, dt, scale, DEV)
            else:
                qs = AC.q_needle(ctx[0], cyc_targets(n, H, [n - 1, torch.zeros_like(n), (ridx * 29) % n]), H)
            q = torch.full((tq + 4, H * D), 7.0, dtype=dt, device=DEV)                 # the sequence's rows start at row 2 of q
            q[2:2 + tq] = qs.view(tq, H * D)
            got = O.attention_probs(q, pools[0], (2, tq, pos0, 4, 1, plen), H, Hkv, D, k_prefix=pools[2])
            assert got.shape == (H, tq, Tk) and got.dtype == dt
            k, _ = AC.context_of(*pools, 4, 1, plen, Tk)
            ref = AC.reference_probs(qs, k, n)
            behind = torch.arange(Tk, device=DEV)[None, :] >= n[:, None]
            assert not got[:, behind].any(), f"probs {name} (Tq {tq}, pos0 {pos0}, plen {plen}): weight behind the diagonal"
            if name == "uniform":
                want = torch.where(behind, 0.0, 1.0 / n[:, None].double())
                assert (ref - want[None]).abs().max().item() < 1e-15
            AC.assert_census(got.permute(1, 0, 2), ref.permute(1, 0, 2), dt, 0, what=f"probs {name} (Tq {tq}, pos0 {pos0}, plen {plen}): (row, head, key)")
