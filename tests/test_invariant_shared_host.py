"""Host side of the batch-invariant mode's shared-prefix form (ops.INVARIANT_SHARED_PREFIX), no GPU needed: the work list of
decode_attention_shared_invariant, which prefix slots the planner calls canonical, the scope of the flag, the keys captured steps and
kept prefills live under, and the drivers' option."""
import argparse

import pytest
import torch

from llava_align_amd import driver_common, ops
from llava_align_amd.engine import IMAGE_TOKEN_INDEX, VddLlavaEngine, WarpSpec, preset

IMG = IMAGE_TOKEN_INDEX


class PlanOnly(VddLlavaEngine):
    """The planner only needs the config: skip weight / kernel set-up."""

    def __init__(self):
        self.cfg = preset("llava-1.5-7b")
        self.dtype = torch.bfloat16
        self.group_attention = True
        self._prefill_cache = None


# ------------------------------------------------------------------------------------------------ the work list

def test_work_list_has_one_item_size_singletons_and_no_per_row_rows():
    # (slot, len, pslot, plen): three rows on image prefix 0, ONE row on image prefix 1, two image-free rows with a prefix, one without
    rows = [[0, 640, 0, 611], [1, 650, 0, 611], [2, 40, 2, 36], [3, 700, 1, 611], [4, 630, 0, 611], [5, 41, 2, 36], [6, 9, 0, 0]]
    mode = [1, 1, 0, 1, 1, 0, 0]
    for cpi in (1, 2, 4, 16):
        groups, members, items = ops.invariant_prefix_work(rows, mode, cpi)
        assert sorted(members) == [0, 1, 3, 4]                                        # every shared row once; per-row rows in no group
        assert sorted((g[1], g[2], g[3]) for g in groups) == [(1, 1, 611), (3, 0, 611)]   # the lone user of prefix 1 is a group of one
        for off, n, ps, pl in groups:
            assert all(rows[m][2] == ps and rows[m][3] == pl for m in members[off:off + n])
        per_slice = -(-611 // (64 * cpi))
        assert len(items) == sum(-(-g[1] // 16) * per_slice for g in groups) == 2 * per_slice      # the item count formula
        for gi, r0, c, zero in items:
            assert r0 % 16 == 0 and r0 < groups[gi][1] and 0 <= c < per_slice and zero == 0
        assert len({tuple(it) for it in items}) == len(items)
    # the default is the documented constant, and the list of a batch is the union of the lists of its parts: nothing follows the batch
    assert ops.invariant_prefix_work(rows, mode)[2] == ops.invariant_prefix_work(rows, mode, ops.INVARIANT_PREFIX_CHUNKS)[2]
    alone = ops.invariant_prefix_work([rows[3]], [1], 2)
    assert alone[0] == [[0, 1, 1, 611]] and alone[1] == [0] and len(alone[2]) == 5
    big = [[i, 620, 7, 611] for i in range(33)]
    assert len(ops.invariant_prefix_work(big, [1] * 33, 2)[2]) == 3 * 5
    assert ops.invariant_prefix_work(rows, [0] * 7, 2) == ([], [], [])
    with pytest.raises(ValueError):
        ops.invariant_prefix_work(rows, mode, 0)
    assert isinstance(ops.INVARIANT_PREFIX_CHUNKS, int) and ops.INVARIANT_PREFIX_CHUNKS >= 1


# ------------------------------------------------------------------------------------------------ canonical prefix slots

def _branches(ids, feats, names=("main", "unk")):
    from llava_align_amd.engine import branch_rows
    return [(nm, branch_rows(nm, ids), feats if nm == "main" else None) for nm in names]


def test_plan_marks_image_prefixes_canonical_and_batch_made_cuts_not():
    sys_tok = list(range(100, 135))
    img_a, img_b = torch.zeros(576, 8), torch.zeros(576, 8)
    ids = [sys_tok + [IMG] + [7, 8, 9], sys_tok + [IMG] + [7, 8, 9, 10], sys_tok + [IMG] + [5]]
    plan = PlanOnly()._plan(_branches(ids, [img_a, img_a, img_b], ("main", "unk", "none")), 576, True)
    # (sys + image a), (sys + image b) | (sys + <unk>), (sys): the image rows' cut is s_img + 576 whatever else is in the batch
    assert [(p["T"], p["canonical"]) for p in plan["prefix"]] == [(611, True), (611, True), (36, False), (35, False)]
    # the two-level split keeps the mark on the image slots; the system prompt's own slot is not canonical
    many = [sys_tok + [IMG] + [7 + i] for i in range(6)]
    plan = PlanOnly()._plan(_branches(many, [torch.zeros(576, 8) for _ in range(6)], ("main",)), 576, True)
    VddLlavaEngine._split_system_prompt(plan)
    assert [p["canonical"] for p in plan["prefix"]] == [True] * 6 + [False] and plan["prefix"][-1]["T"] == 35
    assert all(p["full_T"] == 611 for p in plan["prefix"][:6])


def test_plan_marks_repeated_rows_text_only_cuts_and_branch_shared_embeddings_not_canonical():
    eng = PlanOnly()
    sys_tok = list(range(100, 135))
    # repeated image-free rows: 40 questions with 2 distinct texts -> the `unk` rows share all but their last position
    texts = [[7, 8, 9, 10, 11, 12, 13, 14, 15], [20, 21, 22, 23, 24, 25, 26, 27]]
    ids = [sys_tok + [IMG] + texts[i % 2] for i in range(40)]
    imgs = [torch.zeros(576, 8) for _ in range(20)]
    plan = eng._plan(_branches(ids, [imgs[i // 2] for i in range(40)]), 576, True)
    kinds = {(p["T"], p["canonical"]) for p in plan["prefix"]}
    assert kinds == {(611, True), (35 + 1 + 8, False), (35 + 1 + 7, False)}
    # text-only prompts: the common leading tokens of THIS batch
    text_only = [sys_tok + [7, 8, 9 + i] for i in range(4)]
    plan = eng._plan([("main", text_only, None)], 576, True)
    assert [(p["T"], p["canonical"]) for p in plan["prefix"]] == [(37, False)]
    # prompts given as embeddings: a declared embeds_prefix is canonical, the rows two branches of one call share are not
    e = [torch.zeros(50, 8), torch.ones(50, 8)]
    plan = eng._plan([("main", [[], []], e), ("none", [[], []], e)], 576, True, embeds_only=True)
    assert [(p["T"], p["canonical"]) for p in plan["prefix"]] == [(49, False), (49, False)]
    plan = eng._plan([("main", [[], []], e), ("none", [[], []], e)], 576, True, embeds_only=True, embeds_prefix=[("imgA", 30), ("imgA", 30)])
    assert [(p["T"], p["canonical"]) for p in plan["prefix"]] == [(30, True)]


# ------------------------------------------------------------------------------------------------ the flag

def test_flag_is_scoped_restored_after_an_exception_and_inert_outside_the_mode():
    assert ops.INVARIANT_SHARED_PREFIX is False and not ops.GEMM_BATCH_INVARIANT and not ops.invariant_shared_prefix()
    with ops.batch_invariant():
        assert ops.GEMM_BATCH_INVARIANT and not ops.INVARIANT_SHARED_PREFIX and not ops.invariant_shared_prefix()
    with ops.batch_invariant(shared_prefix=True):
        assert ops.GEMM_BATCH_INVARIANT and ops.INVARIANT_SHARED_PREFIX and ops.invariant_shared_prefix()
        with ops.batch_invariant():                                  # nested: the inner scope decides, the outer one comes back
            assert ops.GEMM_BATCH_INVARIANT and not ops.invariant_shared_prefix()
        assert ops.invariant_shared_prefix()
    assert not ops.GEMM_BATCH_INVARIANT and not ops.INVARIANT_SHARED_PREFIX
    with pytest.raises(KeyError):
        with ops.batch_invariant(shared_prefix=True):
            raise KeyError("inside")
    assert not ops.GEMM_BATCH_INVARIANT and not ops.INVARIANT_SHARED_PREFIX
    # outside the mode the flag means nothing
    with ops.batch_invariant(False, shared_prefix=True):
        assert not ops.GEMM_BATCH_INVARIANT and not ops.invariant_shared_prefix()
        assert ops.fused_attention_rows() > 0 and ops.skinny_rows(4096, 4096) > 0
    old = ops.INVARIANT_SHARED_PREFIX
    try:
        ops.INVARIANT_SHARED_PREFIX = True
        assert not ops.invariant_shared_prefix() and ops.fused_attention_rows() > 0
    finally:
        ops.INVARIANT_SHARED_PREFIX = old


def test_step_key_and_reuse_key_carry_the_flag():
    eng = PlanOnly()
    step = lambda: eng._step_key(4, 2, 8, 1.0, 0.1, WarpSpec(temperature=0.5, top_k=None, top_p=None), False, False, True, True, [2], 0, False)
    reuse = lambda: eng._reuse_lookup([[1, 2, IMG, 3]], None, None, None, (False, True), True, 8)[1]
    with ops.batch_invariant():
        s_off, r_off = step(), reuse()
    with ops.batch_invariant(shared_prefix=True):
        s_on, r_on = step(), reuse()
    with ops.batch_invariant(False, shared_prefix=True):
        s_out, r_out = step(), reuse()
    s_tuned, r_tuned = step(), reuse()
    assert s_off != s_on and r_off != r_on                       # the flag separates graphs and kept prefills inside the mode ...
    assert s_out == s_tuned and r_out == r_tuned                 # ... and changes nothing outside it
    assert len({s_off, s_on, s_tuned}) == 3


# ------------------------------------------------------------------------------------------------ the drivers

def test_driver_option_parses_and_defaults_to_off():
    ap = argparse.ArgumentParser()
    driver_common.add_common_args(ap)
    base = ["--image-folder", "i", "--question-file", "q", "--answers-file", "a"]
    assert driver_common.mode_kw(ap.parse_args(base)) == {}
    assert driver_common.mode_kw(ap.parse_args(base + ["--invariant-shared-prefix"])) == dict(invariant_shared_prefix=True)
    qs = [{"question_id": i, "image": f"im{i // 2}.jpg", "text": "t"} for i in range(4)]
    run = driver_common.ShardedRun(qs, 0, 1, dict(cd_greedy=True), None)
    assert run.invariant and not run.shared_prefix
    run = driver_common.ShardedRun(qs, 0, 1, dict(cd_greedy=True), None, invariant_shared_prefix=True)
    assert run.invariant and run.shared_prefix
    with run.mode():
        assert ops.invariant_shared_prefix()
    assert not ops.GEMM_BATCH_INVARIANT and not ops.INVARIANT_SHARED_PREFIX
    # a sampled run is not in the mode: the option has no effect there
    run = driver_common.ShardedRun(qs, 0, 1, dict(seed=3), None, invariant_shared_prefix=True)
    assert not run.invariant and not run.shared_prefix
    with run.mode():
        assert not ops.GEMM_BATCH_INVARIANT and not ops.invariant_shared_prefix()


@pytest.mark.parametrize("mod,fn", [("pope_driver", "run_pope"), ("mme_driver", "run_mme"), ("qwen_driver", "run_qwen_pope"),
                                    ("blip_driver", "run_blip_pope"), ("sampling_driver", "run_sampling")])
def test_every_driver_takes_the_keyword_and_shows_the_option(mod, fn):
    import importlib
    import inspect
    m = importlib.import_module(f"llava_align_amd.{mod}")
    p = inspect.signature(getattr(m, fn)).parameters["invariant_shared_prefix"]
    assert p.default is False
    assert "mode_kw(a)" in inspect.getsource(m.main) and "--invariant-shared-prefix" in inspect.getsource(driver_common.add_common_args)
