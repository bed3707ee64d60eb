"""VddLlavaEngine.generate_list(paged_kv=True): own-KV memory that follows the tokens really generated.  The checker is the unpaged call
(batch-invariant mode + cd_greedy: token for token), and the capacity / preemption budgets come from a host walk of the schedule
(paged_kv.walk_list_schedule) over the unpaged run's answer lengths - arithmetic, not the run under test."""
import pytest
import torch

from test_engine_shapes_gpu import _engine, _prompts
from test_generate_list_gpu import W7B, _answer_lengths, _eos_set

from llava_align_amd.paged_kv import PAGE, walk_list_schedule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _suffix_lens(ids):
    return [len(r) - r.tolist().index(-200) - 1 for r in ids]


def _same_answers(a, b):
    T = min(a.tokens.shape[1], b.tokens.shape[1])
    return a.tokens.shape == b.tokens.shape and torch.equal(a.tokens[:, :T], b.tokens[:, :T])


@pytest.mark.parametrize("mode", [dict(use_dd_unk=True, temperature=0.5), dict(use_dd=True, use_dd_unk=True, temperature=1.0, top_p=0.9)], ids=["dd_unk", "both_top_p"])
def test_paged_list_answers_equal_the_unpaged_answers_in_batch_invariant_mode(mode):
    """The setup of test_list_answers_equal_the_batch_answers_in_batch_invariant_mode (40 questions, 12 in flight, answers of 1 ... 48
    tokens), paged against unpaged: tokens and step-0 top-10 bit for bit, from a captured step, with the tail shrink, no preemption
    (the pool defaults to the worst case here) and far fewer pages in use than the contiguous slots hold."""
    from llava_align_amd import ops
    eng = _engine(W7B, n_layers=3, vit_layers=2)
    ids, imgs = _prompts(40, 1, 32000, seed=91)
    eos = _eos_set(900, 5)
    kw = dict(cd_alpha=1.0, cd_beta=0.1, cd_greedy=True, max_new_tokens=48, eos_token_id=eos, pad_token_id=0, n_top=10, in_flight=12, sync_every=4,
              admit_min=2, **mode)
    with ops.batch_invariant():
        ref = eng.generate_list(ids, imgs, **kw)
        out = eng.generate_list(ids, imgs, paged_kv=True, **kw)
        again = eng.generate_list(ids, imgs, **kw)                           # the contiguous pools and their captured steps were kept
    assert torch.equal(ref.tokens, out.tokens) and torch.equal(ref.top_tok, out.top_tok) and torch.equal(ref.top_prob, out.top_prob)
    assert torch.equal(ref.tokens, again.tokens)
    st, rs = out.stats, ref.stats
    assert st["paged_kv"] and not rs["paged_kv"] and st["graph"] and st["preemptions"] == 0 and st["in_flight"] == st["in_flight_asked"] == 12
    assert st["tail_shrinks"] >= 1 and st["admissions"] == rs["admissions"] and st["steps"] == rs["steps"]
    suffix_cap = max(_suffix_lens(ids))
    assert st["kv_pages"] == st["n_rows"] * -(-(suffix_cap + 48) // PAGE) + 1
    print("pages peak", st["kv_pages_peak"], "of", st["kv_pages"], "own bytes", st["own_kv_bytes"], "unpaged", rs["own_kv_bytes"])
    assert st["kv_pages_peak"] * PAGE < st["n_rows"] * (suffix_cap + 48)
    L = _answer_lengths(ref.tokens, eos).tolist()
    w = walk_list_schedule(_suffix_lens(ids), L, 12, st["n_rows"] // 12, 48, sync_every=4, admit_min=2)
    assert (st["kv_pages_peak"], st["steps"], st["admissions"]) == (w["kv_pages_peak"], w["steps"], w["admissions"])      # the walk IS the schedule


@pytest.fixture(scope="module")
def long_list():
    """40 questions, 12 in flight, answers of ~50 tokens under a 160-token cap (the EOS density of
    test_retirement_carries_the_in_kernel_processors): most slots stay far below their worst case.  The unpaged run and, from its
    answer lengths, the walk's numbers: `full` (one question at full length), `peak` (most pages ever in use with an unlimited
    pool), `worst` (every slot at full length)."""
    from llava_align_amd import ops
    eng = _engine(W7B, n_layers=2, vit_layers=2)
    ids, imgs = _prompts(40, 1, 32000, seed=91)
    eos = _eos_set(600, 7)
    kw = dict(use_dd_unk=True, temperature=0.5, cd_alpha=1.0, cd_beta=0.1, cd_greedy=True, max_new_tokens=160, eos_token_id=eos, pad_token_id=0,
              in_flight=12, sync_every=4, admit_min=2)
    with ops.batch_invariant():
        ref = eng.generate_list(ids, imgs, **kw)
    L = _answer_lengths(ref.tokens, eos).tolist()
    walk = lambda budget=None: walk_list_schedule(_suffix_lens(ids), L, 12, 2, 160, sync_every=4, admit_min=2, kv_page_budget=budget)
    free = walk()
    print("answer lengths", sorted(L), "walk", free)
    assert free["full"] < free["kv_pages_peak"] < free["worst"], free          # or the list proves nothing
    return dict(eng=eng, ids=ids, imgs=imgs, kw=kw, ref=ref, walk=walk, full=free["full"], peak=free["kv_pages_peak"], worst=free["worst"])


def test_a_pool_of_the_peak_keeps_the_batch_full(long_list):
    from llava_align_amd import ops
    s = long_list
    with ops.batch_invariant():
        out = s["eng"].generate_list(s["ids"], s["imgs"], paged_kv=True, kv_page_budget=s["peak"], **s["kw"])
    st = out.stats
    print({k: st[k] for k in ("kv_pages", "kv_pages_peak", "preemptions", "in_flight", "steps", "admissions")})
    assert st["in_flight"] == st["in_flight_asked"] == 12 and st["preemptions"] == 0 and st["kv_pages"] == st["kv_pages_peak"] == s["peak"]
    assert st["graph"] and _same_answers(s["ref"], out)
    assert st["steps"] == s["ref"].stats["steps"] and st["admissions"] == s["ref"].stats["admissions"]


def test_a_pool_below_the_peak_preempts_and_still_answers_every_question(long_list):
    from llava_align_amd import ops
    s = long_list
    budget = (s["full"] + s["peak"]) // 2
    w = s["walk"](budget)
    print("budget", budget, "walk", w)
    assert w["preemptions"] >= 1 and w["preempted"] <= 20 and w["uncovered"] == 0, w           # no passing by thrashing
    with ops.batch_invariant():
        out = s["eng"].generate_list(s["ids"], s["imgs"], paged_kv=True, kv_page_budget=budget, **s["kw"])
    st = out.stats
    print({k: st[k] for k in ("kv_pages", "kv_pages_peak", "preemptions", "in_flight", "steps", "admissions")})
    assert st["preemptions"] >= 1 and st["preemptions"] == w["preemptions"] and st["kv_pages_peak"] == w["kv_pages_peak"] <= budget
    assert st["steps"] == w["steps"] and st["admissions"] == w["admissions"] and st["questions"] == 40
    assert _same_answers(s["ref"], out)                                                        # a restarted question gives the same answer
    with pytest.raises(ValueError, match="one question at full length"):
        s["eng"].generate_list(s["ids"], s["imgs"], paged_kv=True, kv_page_budget=s["full"], **s["kw"])
    with pytest.raises(ValueError, match="kv_page_budget"):
        s["eng"].generate_list(s["ids"], s["imgs"], kv_page_budget=budget, **s["kw"])


@pytest.mark.parametrize("in_flight", [8, 3])                # 3: six rows, where the unpaged path takes the fused kernel and the paged one does not
def test_sampled_paged_list_run_is_reproducible_and_well_formed(in_flight):
    eng = _engine(W7B, n_layers=2, vit_layers=2)
    ids, imgs = _prompts(5, 6, 32000, seed=17)               # 30 questions, 6 per image
    eos = _eos_set(1500, 3)
    kw = dict(in_flight=in_flight, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.7, max_new_tokens=24, eos_token_id=eos, pad_token_id=0, seed=11,
              sync_every=2, paged_kv=True)
    a = eng.generate_list(ids, imgs, **kw)
    b = eng.generate_list(ids, imgs, **kw)
    assert torch.equal(a.tokens, b.tokens)
    c = eng.generate_list(ids, imgs, **dict(kw, seed=12))
    T = min(a.tokens.shape[1], c.tokens.shape[1])
    assert not torch.equal(a.tokens[:, :T], c.tokens[:, :T])
    L = _answer_lengths(a.tokens, eos)
    eos_t = torch.tensor(eos, device=DEV)
    for q in range(30):
        n = int(L[q])
        assert n == a.tokens.shape[1] or n == 24 or bool((a.tokens[q, n - 1] == eos_t).any())   # ends with EOS unless it ran to the cap
        assert bool((a.tokens[q, n:] == 0).all())
    assert a.stats["admissions"] >= 3 and 0 < a.stats["mean_live_rows"] <= 2 * in_flight and a.stats["paged_kv"] and a.stats["graph"]
    # a tight pool: questions are preempted and drawn afresh - still reproducible for the seed, still well formed
    tight = dict(kw, kv_page_budget=2 * -(-(max(_suffix_lens(ids)) + 24) // PAGE) + 1 + 4)      # one question at full length + 4 pages
    d, e = eng.generate_list(ids, imgs, **tight), eng.generate_list(ids, imgs, **tight)
    print("tight pool:", d.stats["kv_pages"], "pages,", d.stats["preemptions"], "preemptions")
    assert torch.equal(d.tokens, e.tokens) and d.stats["preemptions"] == e.stats["preemptions"]
    Ld = _answer_lengths(d.tokens, eos)
    for q in range(30):
        n = int(Ld[q])
        assert n == d.tokens.shape[1] or n == 24 or bool((d.tokens[q, n - 1] == eos_t).any())
        assert bool((d.tokens[q, n:] == 0).all())
