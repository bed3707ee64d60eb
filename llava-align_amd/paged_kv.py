"""Host side of the paged own-KV pool of VddLlavaEngine.generate_list(paged_kv=True): the page allocator, the provisioning /
admission / preemption rules, and a walk of a whole list call over known answer lengths.  No torch: everything here is arithmetic
over (suffix lengths, answer lengths, sync_every, admit_min, pool size), so a schedule can be predicted and tested without a GPU.

Layout (include/vdd_hip.h): a page holds PAGE consecutive own tokens of one own slot, for all KV heads; own token i of slot s lives
in page table[s][i // PAGE] at index i % PAGE; -1 = no page.  The table is indexed by the own-slot id, which a slot keeps for the
whole call."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

PAGE = 16       # = VDD_KV_PAGE


def pages_for(n_tokens: int) -> int:
    return max(0, -(-int(n_tokens) // PAGE))


def is_poll(steps: int, sync_every: int) -> bool:
    """generate_list reads the finished flags after steps 1 and 3 (the first short answers) and after every sync_every-th step."""
    return steps % sync_every == 0 or (steps in (1, 3) and sync_every > 2)


def next_poll(steps: int, sync_every: int) -> int:
    s = steps + 1
    while not is_poll(s, sync_every):
        s += 1
    return s


class PageAllocator:
    """Free list + pages per row.  Page 0 is never handed out: it is the first page of every row that holds none - a free slot
    decodes a harmless row that writes and attends position 0 of a valid page, and all of them share this one (their outputs are
    discarded; nobody else reads it).  It counts as in use.  reserve() is all-or-nothing."""

    def __init__(self, n_pages: int, n_rows: int, max_pages_per_row: int):
        if n_rows < 1 or max_pages_per_row < 1 or n_pages < 2:
            raise ValueError(f"page pool of {n_pages} pages: the shared page of the idle rows + at least one more")
        self.n_pages, self.n_rows, self.max_pages = int(n_pages), int(n_rows), int(max_pages_per_row)
        self.table = np.full((n_rows, max_pages_per_row), -1, dtype=np.int32)
        self.table[:, 0] = 0
        self.count = [0] * n_rows                                       # pages of each row
        self.free: List[int] = list(range(n_pages - 1, 0, -1))          # a stack: the lowest free page goes out first
        self.in_use = self.peak = 1
        self.dirty = True                                               # the device copy of the table is stale

    def pad_table(self, n_rows: int, max_pages: int):
        """the table in the shape of a (larger) device tensor: more rows / columns, all -1"""
        if (n_rows, max_pages) != self.table.shape:
            t = np.full((max(n_rows, self.table.shape[0]), max(max_pages, self.table.shape[1])), -1, dtype=np.int32)
            t[:, 0] = 0
            t[:self.table.shape[0], :self.table.shape[1]] = self.table
            self.table = t

    def missing(self, row: int, n_tokens: int) -> int:
        """pages `row` lacks to hold n_tokens own tokens"""
        return max(0, min(pages_for(n_tokens), self.max_pages) - self.count[row])

    def reserve(self, row: int, n_tokens: int) -> bool:
        n = self.missing(row, n_tokens)
        if n > len(self.free):
            return False
        for _ in range(n):
            self.table[row, self.count[row]] = self.free.pop()
            self.count[row] += 1
        if n:
            self.in_use += n
            self.peak = max(self.peak, self.in_use)
            self.dirty = True
        return True

    def release(self, row: int):
        """the pages of `row` go back to the free list (the row is idle again: its first page is page 0)"""
        n = self.count[row]
        if n:
            self.free.extend(int(p) for p in self.table[row, :n][::-1])
            self.table[row, :] = -1
            self.table[row, 0] = 0
            self.count[row] = 0
            self.in_use -= n
            self.dirty = True


class ListPager:
    """The paging rules of one generate_list call over `in_flight` question slots of `nb` branch rows each (own-slot id of branch b of
    slot q: b * in_flight + q).  All rows of a question have the same suffix length T, so they hold the same number of pages.

    Provisioning: the host knows an upper bound of a live question's own length - T + the steps since its admission - and at
    every poll reserves what the steps until the NEXT poll can write.  Admission: the waiting questions that go into free slots
    need their suffix + one poll interval.  Preemption: when the live questions cannot all be provisioned, the most recently
    admitted one gives its pages back (its answer so far is discarded, it is prefilled again later), until the rest fits."""

    def __init__(self, n_pages: int, in_flight: int, nb: int, suffix_cap: int, max_new_tokens: int, sync_every: int):
        self.Q, self.nb, self.max_new, self.sync_every = int(in_flight), int(nb), int(max_new_tokens), int(sync_every)
        self.max_pages = pages_for(suffix_cap + max_new_tokens)
        self.full = self.nb * self.max_pages                            # pages of ONE question at full length
        if n_pages < self.full + 1:                                     # ... next to the idle rows' shared page
            raise ValueError(f"kv page pool of {n_pages} pages cannot hold one question at full length "
                             f"({self.full} pages + the idle rows' shared page): nothing could finish")
        self.alloc = PageAllocator(n_pages, self.nb * self.Q, self.max_pages)
        self.T: Dict[int, int] = {}             # slot -> suffix length of the question in it
        self.at: Dict[int, int] = {}            # slot -> step count at its admission
        self.seq: Dict[int, int] = {}           # slot -> admission number (recency)
        self._n = 0
        self.preemptions = 0
        self.hold = False                       # a preemption happened and nobody has finished since

    def rows_of(self, slot: int) -> List[int]:
        return [b * self.Q + slot for b in range(self.nb)]

    def _tokens(self, T: int, at: int, steps: int) -> int:
        return min(T + (next_poll(steps, self.sync_every) - at), T + self.max_new)

    def _missing(self, slot: int, steps: int) -> int:
        return self.nb * self.alloc.missing(slot, self._tokens(self.T[slot], self.at[slot], steps))     # row `slot` = branch 0

    def n_admissible(self, steps: int, suffix_lens: Sequence[int]) -> int:
        """How many of the waiting questions (their suffix lengths, in order) may take a slot now: the free pages must cover their
        suffixes and the steps up to the next poll.  None between a preemption and the next finished question while somebody is
        live: pages only come back when a question finishes, and an admission before that re-creates the shortage."""
        if self.hold and self.T:
            return 0
        left, n = len(self.alloc.free), 0
        for T in suffix_lens:
            left -= self.nb * min(pages_for(self._tokens(T, steps, steps)), self.max_pages)
            if left < 0:
                break
            n += 1
        return n

    def admit(self, steps: int, slot: int, T: int):
        self.T[slot], self.at[slot], self.seq[slot] = int(T), steps, self._n
        self._n += 1
        for r in self.rows_of(slot):
            if not self.alloc.reserve(r, self._tokens(T, steps, steps)):
                raise RuntimeError("admit: no pages left (ask n_admissible first)")

    def _drop(self, slot: int):
        del self.T[slot], self.at[slot], self.seq[slot]
        for r in self.rows_of(slot):
            self.alloc.release(r)

    def retire(self, slot: int):
        """the question in `slot` has finished: its pages are free again"""
        if slot in self.T:
            self._drop(slot)
            self.hold = False

    def provision(self, steps: int, live_slots: Sequence[int]) -> List[int]:
        """Cover every live slot up to the next poll.  Returns the slots preempted to make that possible, oldest admission first."""
        live = sorted(live_slots, key=lambda s: self.seq[s])
        victims = []
        while sum(self._missing(s, steps) for s in live) > len(self.alloc.free):
            v = live.pop()                                               # the most recently admitted
            self._drop(v)
            victims.append(v)
            self.hold = True
        for s in live:
            for r in self.rows_of(s):
                assert self.alloc.reserve(r, self._tokens(self.T[s], self.at[s], steps))
        self.preemptions += len(victims)
        return victims[::-1]

    def stats(self) -> dict:
        return dict(kv_pages=self.alloc.n_pages, kv_pages_peak=self.alloc.peak, preemptions=self.preemptions)


def walk_list_schedule(suffix_lens: Sequence[int], answer_lens: Sequence[int], in_flight: int, nb: int, max_new_tokens: int,
                       sync_every: int = 8, admit_min: Optional[int] = None, kv_page_budget: Optional[int] = None,
                       retire_fraction: float = 0.5) -> dict:
    """generate_list(paged_kv=True) on the host: the same polls, admissions, tail shrinks and page bookkeeping, driven by known answer
    lengths (tokens up to and including the EOS, or max_new_tokens) instead of a decode.  A question admitted after step a has
    finished at the poll after step s iff s - a >= its answer length - 1.  kv_page_budget None: the worst case (no preemption can
    happen), whose `kv_pages_peak` is the most pages a pool of any size would ever hold for this list.
    Returns kv_pages / kv_pages_peak / preemptions as the call's stats report them, + `full` (pages of one question at full
    length), `worst` (every slot at full length), `preempted` (distinct questions ever preempted), `steps`, `admissions`, and
    `uncovered` (writes that found no page: always 0)."""
    N = len(suffix_lens)
    Qc = max(1, min(int(in_flight), N))
    admit_min = max(1, Qc // 16) if admit_min is None else max(1, int(admit_min))
    admit_min = min(admit_min, max(1, Qc // 2))
    cap = max(suffix_lens)
    worst = nb * Qc * pages_for(cap + max_new_tokens) + 1    # every slot at full length + the idle rows' shared page
    pager = ListPager(worst if kv_page_budget is None else kv_page_budget, Qc, nb, cap, max_new_tokens, sync_every)
    waiting, cur = list(range(N)), list(range(Qc))          # cur: own-slot ids of the running step (the tail shrink drops some)
    slot_q = {s: -1 for s in cur}
    adm: Dict[int, int] = {}
    preempted, admissions, uncovered, steps = set(), 0, 0, 0
    unfinished = lambda q, s: s - adm[q] < answer_lens[q] - 1

    def admit(slots):
        nonlocal admissions
        for s in slots:
            q = waiting.pop(0)
            slot_q[s], adm[q] = q, steps
            pager.admit(steps, s, suffix_lens[q])
        admissions += 1

    admit(cur[:pager.n_admissible(0, [suffix_lens[q] for q in waiting[:Qc]])])
    while True:
        steps += 1
        for s in cur:                                       # the step's K / V write of every live row lands in a page it holds
            q = slot_q[s]
            if q >= 0 and unfinished(q, steps - 1) and pager.alloc.count[s] * PAGE < suffix_lens[q] + steps - adm[q]:
                uncovered += 1
        if not is_poll(steps, sync_every):
            continue
        unf = {s: slot_q[s] >= 0 and unfinished(slot_q[s], steps) for s in cur}
        for s in cur:
            if not unf[s] and slot_q[s] >= 0:
                pager.retire(s)
                slot_q[s] = -1
        victims = pager.provision(steps, [s for s in cur if unf[s]])
        for s in victims:
            preempted.add(slot_q[s])
            unf[s] = False
        waiting[:0] = [slot_q[s] for s in victims]
        for s in victims:
            slot_q[s] = -1
        if not waiting:
            if not any(unf.values()):
                break
            live = [s for s in cur if unf[s]]
            if len(live) <= retire_fraction * len(cur) and len(cur) > 8:
                cur = live
            continue
        free = [s for s in cur if not unf[s]]
        cand = free[:len(waiting)]
        n = pager.n_admissible(steps, [suffix_lens[q] for q in waiting[:len(cand)]])
        if n and (n >= min(admit_min, len(waiting)) or not any(unf.values())):
            admit(cand[:n])
    return dict(pager.stats(), full=pager.full, worst=worst, preempted=len(preempted), steps=steps, admissions=admissions, uncovered=uncovered)
