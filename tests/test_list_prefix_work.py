"""ops.list_prefix_work: the host-built group tables of generate_list(group_images=True).  Pure Python, no GPU."""
import random

import pytest

from llava_align_amd import ops


def _ceil(a, b):
    return -(-a // b)


def _rows(spec):
    """spec: [(pslot, plen), ...] -> rows [[slot, len, pslot, plen]] with a few own keys each"""
    return [[i, pl + 3 + i % 5, ps, pl] for i, (ps, pl) in enumerate(spec)]


def _check(rows, live, row_mode, cpi, groups, members, items, n):
    shared = [i for i, r in enumerate(rows) if live[i] and r[3] > 0 and (row_mode is None or row_mode[i])]
    # every live shared row in exactly one group, nobody else in any
    assert sorted(members) == shared
    assert len(set(members)) == len(members)
    covered = []
    for off, n_rows, ps, pl in groups:
        assert n_rows > 0 and pl > 0
        mem = members[off:off + n_rows]
        assert mem == sorted(mem)
        for i in mem:
            assert (rows[i][2], rows[i][3]) == (ps, pl)
        covered += mem
    assert sorted(covered) == shared
    assert len({(g[2], g[3]) for g in groups}) == len(groups)        # one group per (pslot, plen)
    # item census
    want = sum(_ceil(g[1], 16) * _ceil(g[3], 64 * cpi) for g in groups)
    assert n == len(items) == want
    seen = set()
    for gi, r0, c, z in items:
        assert z == 0 and r0 % 16 == 0 and r0 < groups[gi][1] and c * 64 * cpi < groups[gi][3]
        seen.add((gi, r0, c))
    assert len(seen) == len(items)
    # longest first
    keys = [min(64 * cpi, groups[gi][3] - c * 64 * cpi) for gi, _, c, _ in items]
    assert keys == sorted(keys, reverse=True)


@pytest.mark.parametrize("cpi", [1, 2, 3])
def test_groups_items_and_membership(cpi):
    # groups of 1, 6 and 17 rows (two slices), plen 64 / 100 / 611 (not multiples of 64), rows without a prefix, dead rows
    spec = [(0, 611)] * 6 + [(1, 100)] * 17 + [(2, 64)] + [(0, 0)] * 3 + [(3, 611)] * 4
    rows = _rows(spec)
    live = [True] * len(rows)
    live[2] = live[7] = False                      # a dead row in the 6-group and one in the 17-group
    for i in range(27, 31):
        live[i] = False                            # the whole group behind prefix slot 3 is gone: an emptied group
    groups, members, items, n = ops.list_prefix_work(rows, live, None, cpi, 65535)
    _check(rows, live, None, cpi, groups, members, items, n)
    assert [g[1:] for g in groups] == [[5, 0, 611], [16, 1, 100], [1, 2, 64]]
    assert all(g[2] != 3 for g in groups)
    assert 2 not in members and 7 not in members and 24 not in members
    # 17 live rows: two slices
    live[7] = True
    groups, members, items, n = ops.list_prefix_work(rows, live, None, cpi, 65535)
    _check(rows, live, None, cpi, groups, members, items, n)
    assert groups[1][1] == 17 and sorted({it[1] for it in items if it[0] == 1}) == [0, 16]
    assert n == _ceil(611, 64 * cpi) + 2 * _ceil(100, 64 * cpi) + 1


def test_row_mode_keeps_per_row_rows_out():
    spec = [(0, 611)] * 4 + [(5, 35)] * 4 + [(0, 0)] * 2
    rows = _rows(spec)
    mode = [1] * 4 + [0] * 4 + [0] * 2
    live = [True] * 10
    groups, members, items, n = ops.list_prefix_work(rows, live, mode, ops.INVARIANT_PREFIX_CHUNKS, 100)
    _check(rows, live, mode, ops.INVARIANT_PREFIX_CHUNKS, groups, members, items, n)
    assert members == [0, 1, 2, 3] and len(groups) == 1
    # same tables as the static builder of the invariant mode
    g2, m2, i2 = ops.invariant_prefix_work(rows, mode)
    assert (groups, members, items) == (g2, m2, i2)


def test_deterministic_and_nothing_live():
    rng = random.Random(7)
    spec = [(rng.randrange(6), rng.choice([0, 64, 100, 611, 640])) for _ in range(120)]
    # one length per slot, as in the engine's pools
    plen_of = {}
    spec = [(ps, plen_of.setdefault(ps, pl)) for ps, pl in spec]
    rows = _rows(spec)
    live = [rng.random() < 0.7 for _ in rows]
    a = ops.list_prefix_work(rows, live, None, 2, 65535)
    b = ops.list_prefix_work([list(r) for r in rows], list(live), None, 2, 65535)
    assert a == b
    _check(rows, live, None, 2, *a)
    groups, members, items, n = ops.list_prefix_work(rows, [False] * len(rows), None, 2, 1)
    assert (groups, members, items, n) == ([], [], [], 0)


def test_raises_over_capacity_and_on_bad_arguments():
    rows = _rows([(0, 611)] * 17)
    live = [True] * 17
    n = ops.list_prefix_work(rows, live, None, 1, 20)[3]
    assert n == 20
    with pytest.raises(ValueError, match="exceed the capacity"):
        ops.list_prefix_work(rows, live, None, 1, 19)
    with pytest.raises(ValueError):
        ops.list_prefix_work(rows, live, None, 0, 100)
    with pytest.raises(ValueError):
        ops.list_prefix_work(rows, live[:-1], None, 1, 100)
