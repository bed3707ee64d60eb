"""vdd_decode_attention_grouped_list / vdd_decode_attention_shared_invariant_list through ops: the grouped decode attention whose work
list changes under ONE captured launch.  The list entries must give the bits of the static entries on the same tables (whatever the
capacity of the list), serve new tables from the same captured launch, and read a paged own pool to the bits of the contiguous one."""
import pytest
import torch

import attention_census as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, T_PRE = 128, 640
PLEN = {0: 611, 1: 100, 2: 64}            # prefix slot -> length (two of them no multiple of 64)
# (prefix slot or None, rows): groups of 6, 17 (two slices) and 1 rows, and rows in no group
LAYOUT = [(0, 6), (1, 17), (2, 1), (None, 6)]
R = sum(n for _, n in LAYOUT)


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def dt(request):
    return request.param


@pytest.fixture(params=[(8, 8), (8, 2)], ids=["H8kv8", "H8kv2"])
def layout(request):
    return request.param


def i32(x):
    return torch.as_tensor(x, dtype=torch.int32, device=DEV).contiguous()


def _case(dtype, H, Hkv, t_own, long_row=None, seed=0):
    """q, pools, fragment image and host rows: own ranges of 1 .. 40 keys (long_row: that row gets t_own - 3 own keys)"""
    from llava_align_amd import ops
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV, dtype)
    q = rn(R, H * D)
    ko, vo = rn(R, Hkv, t_own, D), rn(R, Hkv, t_own, D)
    kp, vp = rn(3, Hkv, T_PRE, D), rn(3, Hkv, T_PRE, D)
    frag = torch.empty(3, Hkv, 2 * T_PRE, D, dtype=dtype, device=DEV)
    ops.prefix_fragments(kp, vp, frag, i32([PLEN[0], PLEN[1], PLEN[2]]))
    rows, r = [], 0
    for ps, n in LAYOUT:
        for _ in range(n):
            own = 1 + (r * 7) % 40
            if long_row == r:
                own = t_own - 3
            pl = PLEN[ps] if ps is not None else 0
            rows.append([r, pl + own, ps or 0, pl])
            r += 1
    return q, ko, vo, kp, vp, frag, rows


def _tables_b(rows):
    """a later state of the list: the group of one emptied (its row dead: len 1, plen 0), one row of the 6-group dead, two rows of the
    17-group finished (dead rows), i.e. another membership and fewer items"""
    rows_b = [list(r) for r in rows]
    live = [True] * R
    for r in (2, 6 + 17, 8, 20):
        rows_b[r][1], rows_b[r][3] = 1, 0
        live[r] = False
    return rows_b, live


class _ListTables:
    """device tables of fixed capacity, rewritten in place"""

    def __init__(self, cap):
        self.cap = cap
        self.groups, self.group_rows, self.items, self.n = i32(torch.zeros(R, 4)), i32(torch.zeros(R)), i32(torch.zeros(cap, 4)), i32([0])
        self.rows, self.mode = i32(torch.zeros(R, 4)), i32(torch.zeros(R))

    def load(self, rows, groups, members, items, mode=None):
        self.rows.copy_(i32(rows))
        self.groups.zero_(); self.group_rows.zero_(); self.items.zero_()
        if groups:
            self.groups[: len(groups)].copy_(i32(groups)); self.group_rows[: len(members)].copy_(i32(members)); self.items[: len(items)].copy_(i32(items))
        self.n.copy_(i32([len(items)]))
        if mode is not None:
            self.mode.copy_(i32(mode))


def _static(ops, c, rows, groups, members, items, H, Hkv, t_own, cpi):
    q, ko, vo, kp, vp, frag, _ = c
    return ops.decode_attention_grouped(q, ko, vo, kp, vp, i32(rows), i32(groups if groups else [[0, 0, 0, 0]]), i32(members if members else [0]),
                                        i32(items if items else [[0, 0, 0, 0]]), len(items), H, Hkv, D, T_PRE, t_own, prefix_frag=frag,
                                        chunks_per_item=cpi, workspace=ops.attention_workspace(R, H, D, T_PRE + t_own, DEV))


def _list(ops, c, tb, H, Hkv, t_own, cpi, out=None, ws=None, pools=None, page_table=None):
    q, ko, vo, kp, vp, frag, _ = c
    ko, vo = pools if pools is not None else (ko, vo)
    ws = ops.attention_workspace(R, H, D, T_PRE + t_own, DEV) if ws is None else ws
    return ops.decode_attention_grouped_list(q, ko, vo, kp, vp, tb.rows, tb.groups, tb.group_rows, tb.items, tb.n, tb.cap, H, Hkv, D, T_PRE,
                                             t_own, frag, out=out, workspace=ws, chunks_per_item=cpi, page_table=page_table)


@pytest.mark.parametrize("t_own,long_row", [(64, None), (320, 9)], ids=["own_merge", "split"])
@pytest.mark.parametrize("cpi", [1, 2])
def test_list_entry_equals_static_entry(dt, layout, cpi, t_own, long_row):
    from llava_align_amd import ops
    H, Hkv = layout
    c = _case(dt, H, Hkv, t_own, long_row)
    rows = c[-1]
    groups, members, items, n = ops.list_prefix_work(rows, [True] * R, None, cpi, 65535)
    assert n == len(items) and len(groups) == 3
    want = _static(ops, c, rows, groups, members, items, H, Hkv, t_own, cpi)
    for cap in (n, 4 * n + 3, 65535):
        tb = _ListTables(cap)
        tb.load(rows, groups, members, items)
        got = _list(ops, c, tb, H, Hkv, t_own, cpi)
        assert torch.equal(got, want), f"capacity {cap}"
    # ... and against the per-row attention (a sanity bound, not the bit check: rounding of P in the MFMA pass)
    q, ko, vo, kp, vp, _, _ = c
    ref = ops.decode_attention(q, ko, vo, i32(rows), H, Hkv, D, k_prefix=kp, v_prefix=vp, max_len=T_PRE + t_own)
    assert (want.float() - ref.float()).abs().max().item() < 0.05


@pytest.mark.parametrize("cpi", [2, 1])
def test_invariant_list_entry_equals_static_entry(dt, layout, cpi):
    from llava_align_amd import ops
    H, Hkv = layout
    t_own = 64
    c = _case(dt, H, Hkv, t_own, seed=1)
    q, ko, vo, kp, vp, frag, rows = c
    mode = [int(r[3] > 0) for r in rows]
    for r in (7, 11, 22):                       # rows behind a prefix that is not canonical: per row, from the row-major pool
        mode[r] = 0
    groups, members, items, n = ops.list_prefix_work(rows, [True] * R, mode, cpi, 65535)
    assert (groups, members, items) == ops.invariant_prefix_work(rows, mode, cpi)
    kw = dict(chunks_per_item=cpi, workspace=ops.attention_workspace(R, H, D, T_PRE + t_own, DEV))
    want = ops.decode_attention_shared_invariant(q, ko, vo, kp, vp, i32(rows), i32(mode), i32(groups), i32(members), i32(items), n, H, Hkv, D,
                                                 T_PRE, t_own, T_PRE + t_own, frag, **kw)
    for cap in (n, 5 * n):
        tb = _ListTables(cap)
        tb.load(rows, groups, members, items, mode)
        got = ops.decode_attention_shared_invariant_list(q, ko, vo, kp, vp, tb.rows, tb.mode, tb.groups, tb.group_rows, tb.items, tb.n, cap, H,
                                                         Hkv, D, T_PRE, t_own, T_PRE + t_own, frag, **kw)
        assert torch.equal(got, want), f"capacity {cap}"


@pytest.mark.parametrize("invariant", [False, True], ids=["tuned", "invariant"])
def test_one_captured_launch_serves_changing_tables(dt, layout, invariant):
    from llava_align_amd import ops
    H, Hkv = layout
    t_own, cpi = 64, 2
    c = _case(dt, H, Hkv, t_own, seed=2)
    q, ko, vo, kp, vp, frag, rows_a = c
    rows_b, live_b = _tables_b(rows_a)
    mode = [int(r[3] > 0) for r in rows_a] if invariant else None
    work_a = ops.list_prefix_work(rows_a, [True] * R, mode, cpi, 65535)
    work_b = ops.list_prefix_work(rows_b, live_b, mode, cpi, 65535)
    assert work_b[3] < work_a[3] and len(work_b[0]) == len(work_a[0]) - 1
    tb = _ListTables(work_a[3] + 5)
    ws = ops.attention_workspace(R, H, D, T_PRE + t_own, DEV)
    out = torch.zeros(R, H * D, dtype=dt, device=DEV)

    def launch():
        if invariant:
            ops.decode_attention_shared_invariant_list(q, ko, vo, kp, vp, tb.rows, tb.mode, tb.groups, tb.group_rows, tb.items, tb.n, tb.cap, H,
                                                       Hkv, D, T_PRE, t_own, T_PRE + t_own, frag, out=out, workspace=ws, chunks_per_item=cpi)
        else:
            _list(ops, c, tb, H, Hkv, t_own, cpi, out=out, ws=ws)

    def static(rows, work):
        groups, members, items, n = work
        if invariant:
            return ops.decode_attention_shared_invariant(q, ko, vo, kp, vp, i32(rows), i32(mode), i32(groups), i32(members), i32(items), n, H,
                                                         Hkv, D, T_PRE, t_own, T_PRE + t_own, frag, chunks_per_item=cpi,
                                                         workspace=ops.attention_workspace(R, H, D, T_PRE + t_own, DEV))
        return _static(ops, c, rows, groups, members, items, H, Hkv, t_own, cpi)

    tb.load(rows_a, *work_a[:3], mode)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch()
    want_a, want_b = static(rows_a, work_a), static(rows_b, work_b)
    for rows, work, want in ((rows_a, work_a, want_a), (rows_b, work_b, want_b), (rows_a, work_a, want_a)):
        tb.load(rows, *work[:3], mode)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    assert not torch.equal(want_a, want_b)


def _pages_of(ko, vo, rows, max_pages, seed):
    """the own keys of every row scattered into pages handed out in a shuffled order; table row = own slot"""
    from llava_align_amd.paged_kv import PAGE
    Hkv = ko.shape[1]
    need = [-(-(r[1] - r[3]) // PAGE) for r in rows]
    n_pages = sum(need) + 7
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    table = torch.full((R, max_pages), -1, dtype=torch.int32)
    pk = torch.full((n_pages, Hkv, PAGE, D), 0.5, dtype=ko.dtype, device=DEV)
    pv = torch.full_like(pk, AC.POISON)
    for r, row in enumerate(rows):
        for j in range(need[r]):
            pg = perm.pop()
            table[row[0], j] = pg
            pk[pg], pv[pg] = ko[row[0], :, j * PAGE:(j + 1) * PAGE], vo[row[0], :, j * PAGE:(j + 1) * PAGE]
    return pk, pv, table.to(DEV)


@pytest.mark.parametrize("t_own,long_row", [(64, None), (320, 9)], ids=["own_merge", "split"])
def test_paged_list_entry_equals_contiguous(dt, layout, t_own, long_row):
    from llava_align_amd import ops
    from llava_align_amd.paged_kv import PAGE
    H, Hkv = layout
    cpi = 2
    c = _case(dt, H, Hkv, t_own, long_row, seed=3)
    rows = c[-1]
    work = ops.list_prefix_work(rows, [True] * R, None, cpi, 65535)
    tb = _ListTables(2 * work[3])
    tb.load(rows, *work[:3])
    want = _list(ops, c, tb, H, Hkv, t_own, cpi)
    pk, pv, table = _pages_of(c[1], c[2], rows, t_own // PAGE, seed=5)
    got = _list(ops, c, tb, H, Hkv, t_own, cpi, pools=(pk, pv), page_table=table)
    assert torch.equal(got, want)
    # a later state of the list through the same tables
    rows_b, live_b = _tables_b(rows)
    work_b = ops.list_prefix_work(rows_b, live_b, None, cpi, 65535)
    tb.load(rows_b, *work_b[:3])
    assert torch.equal(_list(ops, c, tb, H, Hkv, t_own, cpi, pools=(pk, pv), page_table=table), _list(ops, c, tb, H, Hkv, t_own, cpi))


@pytest.mark.parametrize("t_own,long_row", [(64, None), (320, 9)], ids=["own_merge", "split"])
def test_paged_grouped_key_census(dt, layout, t_own, long_row):
    """uniform census (q = 0, V[t, t % D] = 1 over the row's logical keys): every key of prefix and paged own range counted once"""
    from llava_align_amd import ops
    from llava_align_amd.paged_kv import PAGE
    H, Hkv = layout
    cpi = 2
    q, ko, vo, kp, vp, frag, rows = _case(dt, H, Hkv, t_own, long_row, seed=4)
    q = torch.zeros_like(q)
    vp = torch.full_like(vp, AC.POISON)
    vo = torch.full_like(vo, AC.POISON)
    for ps, pl in PLEN.items():
        vp[ps, :, :pl] = AC.census_v(pl, D, dt, DEV)[None]
    for slot, ln, _, pl in rows:
        vo[slot, :, :ln - pl] = AC.census_v(ln, D, dt, DEV)[pl:][None]
    ops.prefix_fragments(kp, vp, frag, i32([PLEN[0], PLEN[1], PLEN[2]]))
    pk, pv, table = _pages_of(ko, vo, rows, t_own // PAGE, seed=6)
    work = ops.list_prefix_work(rows, [True] * R, None, cpi, 65535)
    tb = _ListTables(work[3] + 1)
    tb.load(rows, *work[:3])
    c = (q, ko, vo, kp, vp, frag, rows)
    got = _list(ops, c, tb, H, Hkv, t_own, cpi, pools=(pk, pv), page_table=table).view(R, H, D)
    ref = AC.census_expected(torch.tensor([r[1] for r in rows], device=DEV), D)[:, None, :].expand(R, H, D)
    AC.assert_census(got, ref, dt, p_roundings=1, what="paged grouped list, uniform census")


def test_refusals_launch_nothing(dt):
    from llava_align_amd import ops
    H, Hkv, t_own, cpi = 8, 8, 64, 1
    c = _case(dt, H, Hkv, t_own, seed=7)
    q, ko, vo, kp, vp, frag, rows = c
    work = ops.list_prefix_work(rows, [True] * R, None, cpi, 65535)
    tb = _ListTables(work[3])
    tb.load(rows, *work[:3])
    lib = ops._lib_ready()
    ws = ops.attention_workspace(R, H, D, T_PRE + t_own, DEV)
    out = torch.full_like(q, 7.0)
    p = lambda t: t.data_ptr()
    dtc = ops._dt(q)

    def grouped(n_dev=p(tb.n), cap=tb.cap, fr=p(frag), pre_tmax=T_PRE, table=None, pages=(0, 0, 0), stride=ko.stride(0), own=t_own, sub=cpi, d=D):
        return lib.vdd_decode_attention_grouped_list(p(q), p(ko), p(vo), table, p(kp), p(vp), fr, p(tb.rows), p(tb.groups), p(tb.group_rows),
                                                     p(tb.items), n_dev, cap, p(out), p(ws), R, H, Hkv, d, stride, ko.shape[2], *pages, kp.stride(0),
                                                     pre_tmax, T_PRE, own, sub, D ** -0.5, dtc, None)

    def invariant(n_dev=p(tb.n), cap=tb.cap, fr=p(frag), pre_tmax=T_PRE, mode=p(tb.mode), sub=cpi):
        return lib.vdd_decode_attention_shared_invariant_list(p(q), p(ko), p(vo), p(kp), p(vp), fr, p(tb.rows), mode, p(tb.groups), p(tb.group_rows),
                                                              p(tb.items), n_dev, cap, p(out), p(ws), R, H, Hkv, D, ko.stride(0), ko.shape[2],
                                                              kp.stride(0), pre_tmax, T_PRE, t_own, T_PRE + t_own, sub, D ** -0.5, dtc, None)

    INVALID = -1
    for f in (grouped, invariant):
        assert f(n_dev=None) == INVALID
        assert f(cap=0) == INVALID and f(cap=-3) == INVALID and f(cap=65536) == INVALID
        assert f(fr=None) == INVALID and f(pre_tmax=T_PRE - 1) == INVALID
        assert f(sub=0) == INVALID
    assert grouped(own=0) == INVALID and grouped(d=64) == INVALID
    assert invariant(mode=None) == INVALID
    # a page table with a pool it cannot index: what vdd_decode_attention_paged refuses
    assert grouped(table=p(tb.group_rows), pages=(0, R, 4)) == INVALID
    assert grouped(table=p(tb.group_rows), pages=(9, R, 4), stride=ko.stride(0) + 1) == INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call launched something"
    with pytest.raises(ValueError):
        ops.decode_attention_grouped_list(q, ko, vo, kp, vp, tb.rows, tb.groups, tb.group_rows, tb.items, tb.n, tb.cap + 1, H, Hkv, D, T_PRE,
                                          t_own, frag, workspace=ws)
