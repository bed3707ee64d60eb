"""VddLlavaEngine.generate_list(group_images=True): the questions about one image attend its prefix once per step, through group tables
that the host rewrites under the captured step.  Checker of the invariant form: ONE generate() call under the same flag, bit for bit."""
import pytest
import torch

from test_engine_shapes_gpu import _engine, _prompts
from test_generate_list_gpu import W7B, _answer_lengths, _eos_set

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    e = _engine(W7B, n_layers=2, vit_layers=2)
    e.retire = False
    return e


def _well_formed(tokens, eos, cap, n):
    L = _answer_lengths(tokens, eos)
    eos_t = torch.tensor(eos, device=DEV)
    for q in range(n):
        k = int(L[q])
        assert k == tokens.shape[1] or k == cap or bool((tokens[q, k - 1] == eos_t).any())
        assert bool((tokens[q, k:] == 0).all())
    return L


def _list_equals_generate(refs, outs, eos, what):
    """Every question's tokens and step-0 top-10 from the list are, bit for bit, those of generate() under the same flag.  generate() is
    called twice and the list twice: the two list runs must agree with each other in every bit, and each question with a generate()
    run.  (Why twice: in one of four processes the FIRST generate() call of the process under the flag answered 2 of 30 questions
    differently from every other generate() and list run, DESIGN section 6d "Known defect"; in the mode a question's answer does not
    depend on its batch, so the other call vouches for it.  Whenever the two generate() calls disagree the questions are printed.)"""
    a, b = outs
    assert a.tokens.shape == b.tokens.shape and torch.equal(a.tokens, b.tokens), f"{what}: two list runs differ"
    assert torch.equal(a.top_tok, b.top_tok) and torch.equal(a.top_prob, b.top_prob)
    T = min([r.tokens.shape[1] for r in refs] + [a.tokens.shape[1]])
    for r in refs:                                                     # columns past T are padding in every run
        assert bool((r.tokens[:, T:] == 0).all())
    assert bool((a.tokens[:, T:] == 0).all())
    same = [(r.tokens[:, :T] == a.tokens[:, :T]).all(1) & (r.top_tok == a.top_tok).all(1) & (r.top_prob == a.top_prob).all(1) for r in refs]
    odd = (~(refs[0].tokens[:, :T] == refs[1].tokens[:, :T]).all(1)).nonzero().flatten().tolist()
    if odd:
        print(f"{what}: KNOWN DEFECT seen - two generate() calls under the flag differ in questions {odd}")
    bad = (~(same[0] | same[1])).nonzero().flatten().tolist()
    assert not bad, f"{what}: the list's questions {bad} equal neither generate() call"
    la = _answer_lengths(a.tokens, eos)
    assert int(la.min()) < int(la.max())
    return la


@pytest.mark.parametrize("case", ["six_per_image", "distinct_images", "vcd"])
def test_invariant_list_answers_equal_generate_under_the_shared_prefix_flag(eng, case):
    """30 questions, 7 in flight (groups straddle admission waves; a group loses and gains rows at every poll): tokens and step-0 top-10 of
    ONE generate() call under batch_invariant(shared_prefix=True)."""
    from llava_align_amd import ops
    ids, imgs = _prompts(5, 6, 32000, seed=17) if case != "distinct_images" else _prompts(30, 1, 32000, seed=23)
    eos = _eos_set(1500, 3)
    kw = dict(cd_alpha=1.0, cd_beta=0.1, cd_greedy=True, use_dd_unk=True, temperature=0.5, max_new_tokens=24, eos_token_id=eos, pad_token_id=0, n_top=10)
    if case == "vcd":
        g = torch.Generator().manual_seed(9)
        kw.update(images_cd=[im + 0.8 * torch.randn(im.shape, generator=g) for im in imgs], use_dd_unk=False)
    lkw = dict(in_flight=7, sync_every=2, admit_min=2, group_images=True)
    with ops.batch_invariant(shared_prefix=True):
        refs = [eng.generate(ids, images=imgs, sync_every=4, **kw) for _ in range(2)]
        outs = [eng.generate_list(ids, imgs, **lkw, **kw) for _ in range(2)]
    out = outs[0]
    assert refs[0].stats["n_groups"] > 0 and refs[0].stats["shared_rows"] > 0
    la = _list_equals_generate(refs, outs, eos, case)
    print(case, "answer lengths", sorted(la.tolist()), {k: out.stats.get(k) for k in ("n_groups", "shared_rows", "admissions", "steps", "items_capacity")})
    st = out.stats
    assert st["n_groups"] > 0 and st["group_images"] is True and 0 < st["shared_rows"] <= 7 and st["graph"] and st["admissions"] >= 3
    if case == "six_per_image":
        assert st["n_groups"] <= 5              # the list has 5 images (the image-free rows are per-row rows in this mode: no group)
    if case == "distinct_images":
        assert st["n_groups"] == st["shared_rows"] == 7


def _embedding_prompts():
    """the Qwen-VL / InstructBLIP call shape of test_embedding_prompts_through_the_list: 18 prompts, two per image, 40 shared rows"""
    g = torch.Generator(device=DEV).manual_seed(3)
    mk = lambda n: (torch.randn(n, 4096, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    shared = [mk(40) for _ in range(9)]
    emb = [torch.cat([shared[i // 2], mk(7 + i % 5)]) for i in range(18)]
    return emb, [(f"im{i // 2}", 40) for i in range(18)], [torch.cat([mk(40), e[40:]]) for e in emb]


@pytest.mark.parametrize("mode", ["plain", "dd_unk", "vcd"])
def test_invariant_list_of_embedding_prompts_equals_generate(eng, mode):
    """prompts as embeddings with a declared embeds_prefix (the canonical "emb" prefix; qwen_driver's call): the answers of generate()"""
    from llava_align_amd import ops
    emb, pre, emb_cd = _embedding_prompts()
    eos = _eos_set(900, 5)
    kw = dict(cd_alpha=1.0, cd_beta=0.1, cd_greedy=True, temperature=0.7, max_new_tokens=24, eos_token_id=eos, pad_token_id=0, n_top=10, use_dd_unk=mode == "dd_unk",
              **(dict(images_cd=emb_cd) if mode == "vcd" else {}))
    lkw = dict(in_flight=5, sync_every=2, admit_min=2, group_images=True)
    with ops.batch_invariant(shared_prefix=True):
        refs = [eng.generate(None, inputs_embeds=emb, embeds_prefix=pre, sync_every=4, **kw) for _ in range(2)]
        outs = [eng.generate_list(None, inputs_embeds=emb, embeds_prefix=pre, **lkw, **kw) for _ in range(2)]
    assert refs[0].stats["n_groups"] > 0
    _list_equals_generate(refs, outs, eos, "embeddings " + mode)
    st = outs[0].stats
    assert st["n_groups"] > 0 and st["shared_rows"] > 0 and st["group_images"] is True and st["admissions"] >= 3


def test_tuned_list_of_embedding_prompts_groups_declared_and_per_question_prefixes(eng):
    """tuned mode, embeddings: with embeds_prefix the rows about one image (both branches) form a group, without it the two branches of
    a question share everything but their last position - a group of two per question"""
    emb, pre, _ = _embedding_prompts()
    eos = _eos_set(900, 5)
    kw = dict(cd_alpha=1.0, cd_beta=0.1, temperature=0.7, max_new_tokens=24, eos_token_id=eos, pad_token_id=0, use_dd_unk=True, seed=5, in_flight=6,
              sync_every=2, admit_min=2)
    for extra, groups_at_most in ((dict(embeds_prefix=pre), 6), (dict(), 6)):
        a = eng.generate_list(None, inputs_embeds=emb, group_images=True, **extra, **kw)
        b = eng.generate_list(None, inputs_embeds=emb, group_images=True, **extra, **kw)
        assert torch.equal(a.tokens, b.tokens)
        _well_formed(a.tokens, eos, 24, 18)
        assert 0 < a.stats["n_groups"] <= groups_at_most and a.stats["shared_rows"] == 12 and a.stats["graph"]
        g_ = eng.generate_list(None, inputs_embeds=emb, group_images=True, cd_greedy=True, **extra, **kw)
        u_ = eng.generate_list(None, inputs_embeds=emb, cd_greedy=True, **extra, **kw)
        assert torch.equal(g_.tokens[:, 0], u_.tokens[:, 0])
        assert (g_.tokens[:, 1] == u_.tokens[:, 1]).float().mean().item() >= 0.9


def test_tuned_sampled_run_is_reproducible_well_formed_and_near_the_ungrouped_run(eng):
    ids, imgs = _prompts(5, 6, 32000, seed=17)
    eos = _eos_set(1500, 3)
    kw = dict(in_flight=12, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.7, max_new_tokens=24, eos_token_id=eos, pad_token_id=0, seed=11,
              sync_every=2, group_images=True)
    a = eng.generate_list(ids, imgs, **kw)
    b = eng.generate_list(ids, imgs, **kw)
    assert torch.equal(a.tokens, b.tokens)
    c = eng.generate_list(ids, imgs, **dict(kw, seed=12))
    T = min(a.tokens.shape[1], c.tokens.shape[1])
    assert not torch.equal(a.tokens[:, :T], c.tokens[:, :T])
    _well_formed(a.tokens, eos, 24, 30)
    st = a.stats
    assert st["admissions"] >= 2 and st["graph"] and st["group_images"] is True and st.get("tail_shrinks", 0) >= 1
    # 12 questions in flight x 2 branches, every row behind a prefix: at the most the list's 5 images (slots are refilled as answers end, so
    # the questions in flight are not consecutive) + the ONE group of the image-free rows behind the system prompt
    assert 2 <= st["n_groups"] <= 6 and st["shared_rows"] == 24
    # deterministic: the first decoded token against the ungrouped list (the bound tests/test_invariant_shared_gpu.py applies to grouped
    # against per-row arithmetic)
    det = dict(kw, cd_greedy=True)
    g_, u_ = eng.generate_list(ids, imgs, **det), eng.generate_list(ids, imgs, **dict(det, group_images=False))
    assert u_.stats["n_groups"] == 0 and "group_images" not in u_.stats                       # a default call reports what it always did
    assert torch.equal(g_.tokens[:, 0], u_.tokens[:, 0])                                       # step 0 comes from the prefill
    agree = (g_.tokens[:, 1] == u_.tokens[:, 1]).float().mean().item()
    print("first decoded token: grouped list agrees with the ungrouped list in", agree)
    assert agree >= 0.9


def test_tuned_paged_grouped_list_gives_the_contiguous_grouped_tokens(eng):
    from llava_align_amd.paged_kv import PAGE
    ids, imgs = _prompts(5, 6, 32000, seed=17)
    eos = _eos_set(1500, 3)
    kw = dict(in_flight=7, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, cd_greedy=True, temperature=0.7, max_new_tokens=24, eos_token_id=eos, pad_token_id=0,
              sync_every=2, admit_min=2, group_images=True)
    a = eng.generate_list(ids, imgs, **kw)
    b = eng.generate_list(ids, imgs, paged_kv=True, **kw)
    assert a.tokens.shape == b.tokens.shape and torch.equal(a.tokens, b.tokens)
    assert b.stats["paged_kv"] and b.stats["preemptions"] == 0 and b.stats["n_groups"] > 0 and b.stats["graph"] and b.stats["steps"] == a.stats["steps"]
    # a tight pool (one question at full length + 4 pages): questions are preempted, leave their groups and come back.  The tuned
    # prefix pass rotates its chunk walk with the group's index and slice, so a question restarted next to other neighbours may differ
    # in low-order bits: every answer is well formed, step 0 (the prefill's) is the same, and the first decoded token agrees as far as
    # grouped arithmetic agrees with itself under another grouping (the 0.9 of the test above)
    suffix = max(len(r) - r.tolist().index(-200) - 1 for r in ids)
    c = eng.generate_list(ids, imgs, paged_kv=True, kv_page_budget=2 * -(-(suffix + 24) // PAGE) + 1 + 4, **kw)
    print("tight pool:", c.stats["kv_pages"], "pages,", c.stats["preemptions"], "preemptions,", c.stats["n_groups"], "groups at the peak")
    assert c.stats["preemptions"] > 0 and c.stats["n_groups"] > 0
    _well_formed(c.tokens, eos, 24, 30)
    assert torch.equal(c.tokens[:, 0], a.tokens[:, 0])
    assert (c.tokens[:, 1] == a.tokens[:, 1]).float().mean().item() >= 0.9


def test_mode_refusals_and_the_default_call(eng):
    from llava_align_amd import ops
    ids, imgs = _prompts(2, 2, 32000, seed=5)
    kw = dict(in_flight=2, max_new_tokens=3, eos_token_id=2, pad_token_id=0, cd_greedy=True, temperature=0.5)
    with ops.batch_invariant(shared_prefix=True):
        with pytest.raises(ValueError, match="INVARIANT_SHARED_PREFIX"):
            eng.generate_list(ids, imgs, **kw)
        with pytest.raises(ValueError, match="no paged own-KV form"):
            eng.generate_list(ids, imgs, group_images=True, paged_kv=True, **kw)
    with ops.batch_invariant():
        with pytest.raises(ValueError, match="has no groups without its shared-prefix form"):
            eng.generate_list(ids, imgs, group_images=True, **kw)
        out = eng.generate_list(ids, imgs, **kw)
    assert out.stats["n_groups"] == 0 and "group_images" not in out.stats and "shared_rows" not in out.stats
    eng.group_attention = False
    try:
        with pytest.raises(ValueError, match="group_attention off"):
            eng.generate_list(ids, imgs, group_images=True, **kw)
    finally:
        eng.group_attention = True
    out = eng.generate_list(ids, imgs, **kw)
    assert out.stats["n_groups"] == 0
