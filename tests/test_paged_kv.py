"""Paged own-KV pool of generate_list, host side (llava_align_amd/paged_kv.py) and C ABI surface.  No GPU needed: the allocator, the
provisioning / admission / preemption rules and a whole list call are arithmetic over (suffix lengths, answer lengths, sync_every,
admit_min, pool size)."""
import os
import re

import numpy as np
import pytest

from llava_align_amd.paged_kv import PAGE, ListPager, PageAllocator, is_poll, next_poll, pages_for, walk_list_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGED_ENTRIES = ("vdd_rope_kv_write_paged", "vdd_decode_attention_paged", "vdd_kv_pages_scatter")


def test_allocator_reserve_release_reuse_and_peak():
    a = PageAllocator(n_pages=10, n_rows=3, max_pages_per_row=4)
    assert a.in_use == a.peak == 1 and (a.table[:, 0] == 0).all() and (a.table[:, 1:] == -1).all()     # idle rows share page 0
    assert a.reserve(0, 1) and a.table[0, 0] == 1 and a.count[0] == 1
    assert a.reserve(0, PAGE) and a.count[0] == 1                       # 16 tokens: still one page
    assert a.reserve(0, PAGE + 1) and a.table[0].tolist() == [1, 2, -1, -1]
    assert a.reserve(1, 3 * PAGE) and a.table[1].tolist() == [3, 4, 5, -1]
    assert a.in_use == a.peak == 6 and a.missing(2, 64) == 4
    assert a.reserve(2, 64 + 999) and a.count[2] == 4                   # a row never takes more than max_pages_per_row
    assert a.in_use == 10 and not a.free
    assert not a.reserve(1, 4 * PAGE) and a.count[1] == 3               # all or nothing
    a.release(0)
    assert a.table[0].tolist() == [0, -1, -1, -1] and a.in_use == 8 and a.peak == 10
    assert a.reserve(1, 4 * PAGE) and a.table[1, 3] == 1                # the lowest freed page is reused first
    pages = [int(p) for r in range(3) for p in a.table[r, :a.count[r]]]
    assert len(pages) == len(set(pages)) and 0 not in pages             # no page belongs to two rows; page 0 is never handed out
    a.dirty = False
    a.release(0)                                                        # nothing to give back: the device table stays valid
    assert not a.dirty


def test_pool_below_one_full_question_is_refused():
    full = 3 * pages_for(20 + 160)
    with pytest.raises(ValueError, match="one question at full length"):
        ListPager(full, 8, 3, 20, 160, 8)
    assert ListPager(full + 1, 8, 3, 20, 160, 8).full == full


def test_polls():
    assert [s for s in range(1, 20) if is_poll(s, 8)] == [1, 3, 8, 16] and [s for s in range(1, 7) if is_poll(s, 2)] == [2, 4, 6]
    assert next_poll(0, 8) == 1 and next_poll(3, 8) == 8 and next_poll(8, 8) == 16


def test_preemption_takes_the_most_recently_admitted_first():
    p = ListPager(1 + 16, in_flight=4, nb=2, suffix_cap=16, max_new_tokens=32, sync_every=4)       # 16 pages for 4 slots of 2 rows
    for slot in (2, 0, 3, 1):                                           # admission order
        assert p.n_admissible(0, [16]) == 1
        p.admit(0, slot, 16)                                            # 16 suffix tokens + 1 step: 2 pages per row
    assert len(p.alloc.free) == 0 and p.n_admissible(0, [16]) == 0 and p.provision(1, [0, 1, 2, 3]) == []      # covered up to step 3
    # at step 16 every row needs a third page (16 + 20 tokens): 8 pages, none free -> 1 goes (+4), still short -> 3 goes (+4): fits
    assert p.provision(16, [0, 1, 2, 3]) == [3, 1] and p.preemptions == 2 and p.hold
    assert p.alloc.count[1] == p.alloc.count[3] == 0 and p.alloc.count[0] == p.alloc.count[2] == 3
    assert p.n_admissible(16, [16]) == 0                                # nobody has finished since the preemption
    p.retire(2)
    assert not p.hold and p.n_admissible(16, [16, 16, 16, 16]) == 2      # 10 pages free, 4 per question


def _lists(seed, n=60, cap=160):
    rng = np.random.default_rng(seed)
    return rng.integers(5, 30, n).tolist(), np.minimum(rng.geometric(0.03, n), cap).tolist()


@pytest.mark.parametrize("sync_every", [2, 4, 8])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_provisioning_never_leaves_a_live_row_uncovered(seed, sync_every):
    """A synthetic schedule of answer lengths walked on the host, at every pool size from the worst case down to one question: every
    K / V write of a live row finds a page, every question finishes, and the pool is never overdrawn."""
    T, L = _lists(seed)
    kw = dict(in_flight=12, nb=2, max_new_tokens=160, sync_every=sync_every, admit_min=2)
    free = walk_list_schedule(T, L, **kw)
    full, peak, worst = free["full"], free["kv_pages_peak"], free["worst"]
    assert free["uncovered"] == 0 and free["preemptions"] == 0 and full < peak < worst
    at_peak = walk_list_schedule(T, L, kv_page_budget=peak, **kw)       # a pool of exactly the peak changes nothing
    assert dict(at_peak, kv_pages=0) == dict(free, kv_pages=0)
    last = 0
    for budget in (peak - 1, (full + peak) // 2, full + 1):
        w = walk_list_schedule(T, L, kv_page_budget=budget, **kw)
        assert w["uncovered"] == 0 and w["kv_pages_peak"] <= budget and w["preemptions"] >= w["preempted"] and w["steps"] >= free["steps"]
        last = w["preemptions"]
    assert last >= 1                                                    # (a pool just below the peak may only delay an admission)
    with pytest.raises(ValueError):
        walk_list_schedule(T, L, kv_page_budget=full, **kw)


def test_a_midway_pool_does_not_thrash():
    """The list shape of the GPU preemption test (40 questions, 12 in flight, two branches, answers of ~50 tokens capped at 160, a
    pool midway between one question and the peak): at most half of the questions are ever preempted."""
    for seed in range(6):
        rng = np.random.default_rng(seed)
        T, L = rng.integers(19, 29, 40).tolist(), np.minimum(rng.geometric(0.019, 40), 160).tolist()
        kw = dict(in_flight=12, nb=2, max_new_tokens=160, sync_every=4, admit_min=2)
        free = walk_list_schedule(T, L, **kw)
        w = walk_list_schedule(T, L, kv_page_budget=(free["full"] + free["kv_pages_peak"]) // 2, **kw)
        assert 1 <= w["preempted"] <= 20 and w["uncovered"] == 0, (seed, w)


def test_page_size_is_one_constant():
    src = open(os.path.join(ROOT, "include", "vdd_hip.h")).read()
    assert int(re.search(r"#define\s+VDD_KV_PAGE\s+(\d+)", src).group(1)) == PAGE == 16


def test_entries_are_declared_exported_and_bound():
    from llava_align_amd import _build, load_lib, ops
    _build.build_lib()
    lib = load_lib()
    ops._lib_ready()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdd_hip.h")).read(), flags=re.S)
    for name in PAGED_ENTRIES:
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert hasattr(lib, name) and name in ops._SIGS
        args = lambda n, dtype: [None if ct is ops._P else n for ct in ops._SIGS[name][:-2]] + [dtype, None]
        for dtype in (1, 2):
            assert getattr(lib, name)(*args(0, dtype)) == 0             # M = 0: nothing to do
        for bad in (0, 3):
            assert getattr(lib, name)(*args(4, bad)) == -1              # refused before anything is launched
        assert getattr(lib, name)(*args(4, 2)) == -1                    # null pools / table: refused, no launch
    assert hasattr(ops, "rope_kv_write_paged") and hasattr(ops, "decode_attention_paged") and hasattr(ops, "kv_pages_scatter")
