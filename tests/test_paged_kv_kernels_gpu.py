"""The three entry points of the paged own-KV pool (include/vdd_hip.h: vdd_rope_kv_write_paged, vdd_decode_attention_paged,
vdd_kv_pages_scatter) against their contiguous counterparts, bit for bit, in both storage types."""
import pytest
import torch

from llava_align_amd.paged_kv import PAGE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def dt(request):
    return request.param


def _rand(dt, *shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(dt)


def _rope_table(max_pos, D, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous().to(DEV)


def _shuffled_table(n_slots, pages_of_slot, max_pages, n_pages, seed):
    """int32 [n_slots, max_pages]: slot s holds pages_of_slot[s] pages drawn from a random permutation of the pool (non-contiguous,
    out of order), -1 behind them"""
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    assert sum(pages_of_slot) <= n_pages
    table = torch.full((n_slots, max_pages), -1, dtype=torch.int32)
    for s, n in enumerate(pages_of_slot):
        for j in range(n):
            table[s, j] = perm.pop()
    return table.to(DEV)


def _gather(pages, table, t_max):
    """pages [n_pages, Hkv, PAGE, D] read back through the table -> contiguous [n_slots, Hkv, t_max, D] (zeros where there is no page)"""
    S, Hkv, D = table.shape[0], pages.shape[1], pages.shape[3]
    out = torch.zeros(S, Hkv, t_max, D, dtype=pages.dtype, device=pages.device)
    for s in range(S):
        for j in range(t_max // PAGE):
            if int(table[s, j]) >= 0:
                out[s, :, j * PAGE:(j + 1) * PAGE] = pages[int(table[s, j])]
    return out


def _paged_copy(kc, table, n_pages):
    """the contiguous slots kc [S, Hkv, T, D] laid out in pages through `table`; pages nobody holds are filled with NaN"""
    S, Hkv, T, D = kc.shape
    pages = torch.full((n_pages, Hkv, PAGE, D), float("nan"), dtype=kc.dtype, device=kc.device)
    for s in range(S):
        for j in range(T // PAGE):
            if int(table[s, j]) >= 0:
                pages[int(table[s, j])] = kc[s, :, j * PAGE:(j + 1) * PAGE]
    return pages


@pytest.mark.parametrize("H,Hkv", [(32, 32), (40, 40), (32, 8)], ids=["7b", "13b", "gqa"])
def test_rope_kv_write_paged_equals_the_contiguous_write(dt, H, Hkv):
    from llava_align_amd import ops
    D, T, S = 128, 64, 6
    cpos_l = [0, 15, 16, 17, 63, 31, 5]
    slot_l = [0, 1, 2, 3, 4, 5, 1]
    M = len(cpos_l)
    qkv = _rand(dt, M, (H + 2 * Hkv) * D, seed=4)
    pos = torch.tensor([40 + c for c in cpos_l], dtype=torch.int32, device=DEV)
    cpos = torch.tensor(cpos_l, dtype=torch.int32, device=DEV)
    slot = torch.tensor(slot_l, dtype=torch.int32, device=DEV)
    cs = _rope_table(128, D)
    kc = torch.zeros(S, Hkv, T, D, dtype=dt, device=DEV)
    vc = torch.zeros_like(kc)
    q_ref = ops.rope_kv_write(qkv, pos, slot, cs, kc, vc, H, Hkv, D, cpos=cpos)
    n_pages = S * (T // PAGE) + 7
    table = _shuffled_table(S, [T // PAGE] * S, T // PAGE + 2, n_pages, seed=1)
    pk = torch.zeros(n_pages, Hkv, PAGE, D, dtype=dt, device=DEV)
    pv = torch.zeros_like(pk)
    q = ops.rope_kv_write_paged(qkv, pos, slot, cs, pk, pv, table, H, Hkv, D, cpos=cpos)
    assert torch.equal(q, q_ref)
    assert torch.equal(_gather(pk, table, T), kc) and torch.equal(_gather(pv, table, T), vc)
    assert int((pk != 0).any(-1).sum()) == M * Hkv == int((kc != 0).any(-1).sum())            # nothing else touched
    # rows without a page for their position - entry -1, an entry beyond the pool, an own index beyond the table, a slot beyond it -
    # leave every page unchanged and still rotate q
    before_k, before_v = pk.clone(), pv.clone()
    bad = table.clone()
    bad[0, 0] = -1
    bad[1, 0], bad[1, 1] = n_pages, n_pages + 5
    cpos2 = torch.tensor([3, 15, 16, (T // PAGE + 2) * PAGE, 9], dtype=torch.int32, device=DEV)
    slot2 = torch.tensor([0, 1, 1, 2, S], dtype=torch.int32, device=DEV)
    qkv2 = _rand(dt, 5, (H + 2 * Hkv) * D, seed=9)
    q2 = ops.rope_kv_write_paged(qkv2, pos[:5].contiguous(), slot2, cs, pk, pv, bad, H, Hkv, D, cpos=cpos2)
    assert torch.equal(pk, before_k) and torch.equal(pv, before_v)
    scratch_k, scratch_v = torch.zeros(S + 1, Hkv, 128, D, dtype=dt, device=DEV), torch.zeros(S + 1, Hkv, 128, D, dtype=dt, device=DEV)
    assert torch.equal(q2, ops.rope_kv_write(qkv2, pos[:5].contiguous(), slot2, cs, scratch_k, scratch_v, H, Hkv, D, cpos=cpos2))


OWN_LENS = [1, 15, 16, 17, 63, 64, 65, 300, 1100]
PREFIX_LENS = [0, 35, 611]


@pytest.mark.parametrize("H,Hkv", [(32, 32), (40, 40), (32, 8)], ids=["7b", "13b", "gqa"])
def test_decode_attention_paged_is_bit_identical_to_the_contiguous_kernel(dt, H, Hkv):
    """Same K / V behind a shuffled, non-contiguous page table: torch.equal on the output.  Own ranges of 1 ... 1,100 keys behind
    prefixes of 0 / 35 / 611 keys, so that own ranges start and end inside 64-key chunks and 16-token pages."""
    from llava_align_amd import ops
    D, T_own, T_pre = 128, 1104, 640
    S = len(OWN_LENS)
    kc, vc = _rand(dt, S, Hkv, T_own, D, seed=11), _rand(dt, S, Hkv, T_own, D, seed=12)
    kp, vp = _rand(dt, 3, Hkv, T_pre, D, seed=13), _rand(dt, 3, Hkv, T_pre, D, seed=14)
    rows_l = [[s, pl + n, ps, pl] for ps, pl in enumerate(PREFIX_LENS) for s, n in enumerate(OWN_LENS)]
    order = torch.randperm(len(rows_l), generator=torch.Generator().manual_seed(3)).tolist()
    rows = torch.tensor([rows_l[i] for i in order], dtype=torch.int32, device=DEV)
    M = rows.shape[0]
    q = _rand(dt, M, H * D, seed=15)
    max_len = T_pre + T_own
    ws = ops.attention_workspace(M, H, D, max_len, DEV)
    ref = ops.decode_attention(q, kc, vc, rows, H, Hkv, D, k_prefix=kp, v_prefix=vp, max_len=max_len, workspace=ws).clone()
    held = [-(-n // PAGE) for n in OWN_LENS]                               # a slot holds exactly the pages its own keys need
    n_pages = sum(held) + 40
    table = _shuffled_table(S, held, T_own // PAGE, n_pages, seed=2)
    pk, pv = _paged_copy(kc, table, n_pages), _paged_copy(vc, table, n_pages)
    out = ops.decode_attention_paged(q, pk, pv, table, rows, H, Hkv, D, kp, vp, max_len, ws)
    assert torch.isfinite(out.float()).all()                                # no key came from a page nobody holds
    assert torch.equal(out, ref)
    # a smaller step over surviving slots reads the same table (it is indexed by the own-slot id, not by the row's place)
    keep = torch.tensor([5, 2, 11, 20], device=DEV)
    sub = ops.decode_attention_paged(q[keep].contiguous(), pk, pv, table, rows[keep].contiguous(), H, Hkv, D, kp, vp, max_len, ws)
    assert torch.equal(sub, ref[keep])
    # a host mistake - the last page of the longest slot missing, another entry beyond the pool - gives a wrong number, not a fault
    bad = table.clone()
    bad[8, held[8] - 1] = -1
    bad[7, 0] = n_pages + 3
    wrong = ops.decode_attention_paged(q, pk, pv, bad, rows, H, Hkv, D, kp, vp, max_len, ws)
    hit = torch.tensor([r[0] in (7, 8) for r in rows.tolist()], device=DEV)
    assert torch.equal(wrong[~hit], ref[~hit]) and not torch.equal(wrong[hit], ref[hit])


def test_paged_entries_refuse_bad_pools_before_any_launch(dt):
    from llava_align_amd import ops
    H = Hkv = 8
    D = 128
    pk = torch.zeros(4, Hkv, PAGE, D, dtype=dt, device=DEV)
    table = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    rows = torch.tensor([[0, 1, 0, 0]], dtype=torch.int32, device=DEV)
    q = _rand(dt, 1, H * D)
    ws = ops.attention_workspace(1, H, D, 128, DEV)
    with pytest.raises(ValueError, match="paged own-KV"):
        ops.decode_attention_paged(q, pk[:, :, :8], pk[:, :, :8], table, rows, H, Hkv, D, pk, pk, 128, ws)            # not PAGE tokens per page
    with pytest.raises(ValueError, match="paged own-KV"):
        ops.decode_attention_paged(q, pk, pk, table.long(), rows, H, Hkv, D, pk, pk, 128, ws)
    lib = ops._lib_ready()
    code = 2 if dt == torch.bfloat16 else 1
    args = lambda stride, n_pages, n_slots, max_pages: (q.data_ptr(), pk.data_ptr(), pk.data_ptr(), table.data_ptr(), pk.data_ptr(), pk.data_ptr(),
                                                        rows.data_ptr(), q.data_ptr(), ws.data_ptr(), 1, H, Hkv, D, stride, n_pages, n_slots, max_pages,
                                                        pk.stride(0), PAGE, 128, 0.1, code, None)
    assert lib.vdd_decode_attention_paged(*args(pk.stride(0) + 8, 4, 2, 3)) == -1
    for bad in ((0, 2, 3), (4, 0, 3), (4, 2, 0)):
        assert lib.vdd_decode_attention_paged(*args(pk.stride(0), *bad)) == -1


@pytest.mark.parametrize("Hkv", [32, 40, 8])
def test_kv_pages_scatter_copies_exactly_and_touches_no_other_page(dt, Hkv):
    from llava_align_amd import ops
    D, T, S = 128, 64, 7
    ko, vo = _rand(dt, S, Hkv, T, D, seed=21), _rand(dt, S, Hkv, T, D, seed=22)
    n_pages = S * (T // PAGE) + 5
    table = _shuffled_table(S, [T // PAGE] * S, T // PAGE + 1, n_pages, seed=5)
    pk = torch.full((n_pages, Hkv, PAGE, D), 7.0, dtype=dt, device=DEV)
    pv = torch.full_like(pk, -3.0)
    slots_l, n_tok_l = [4, 0, 6, 2], [1, 17, 64, 33]
    slots = torch.tensor(slots_l, dtype=torch.int32, device=DEV)
    n_tok = torch.tensor(n_tok_l, dtype=torch.int32, device=DEV)
    ops.kv_pages_scatter(ko, vo, pk, pv, table, slots, n_tok, max(n_tok_l))
    want_k, want_v = torch.full((S, Hkv, T, D), 7.0, dtype=dt, device=DEV), torch.full((S, Hkv, T, D), -3.0, dtype=dt, device=DEV)
    for s, n in zip(slots_l, n_tok_l):
        want_k[s, :, :n], want_v[s, :, :n] = ko[s, :, :n], vo[s, :, :n]
    held = torch.zeros(n_pages, dtype=torch.bool, device=DEV)
    held[table[table >= 0].long()] = True
    assert torch.equal(_gather(pk, table, T), want_k) and torch.equal(_gather(pv, table, T), want_v)
    assert bool((pk[~held] == 7.0).all()) and bool((pv[~held] == -3.0).all())                 # pages nobody holds: untouched
    # a row whose pages are missing is skipped, the others are still copied
    bad = table.clone()
    bad[0, 1] = -1
    pk.fill_(7.0); pv.fill_(-3.0)
    ops.kv_pages_scatter(ko, vo, pk, pv, bad, slots, n_tok, max(n_tok_l))
    want_k[0, :, PAGE:] = 0
    got = _gather(pk, bad, T)
    assert torch.equal(got[0, :, :PAGE], ko[0, :, :PAGE]) and torch.equal(got[4], want_k[4]) and torch.equal(got[6], want_k[6])
    assert bool((pk[int(table[0, 1])] == 7.0).all())
