"""No answer of an engine call may depend on bytes nobody wrote (tests/poison.py).

Every KV pool, fragment image, ViT pool, activation matrix, output and split-KV workspace of the engine comes from torch.empty.  A second
call with the same questions finds the pools holding the correct values of the first, so a read past a length, of a padded row or of a
chunk tail that is never written passes every other engine test.  Here every mode of the engine runs on FRESH engines (pools really are
reallocated) whose allocations are filled with 0.0, with NaN and with +3.0e4, and its tokens, step-0 top-10 and every score row must be
the same BITS under the three; and on ONE engine whose pools are scrubbed, or used by other questions, between identical calls (the
replay path of the captured graphs over stale memory).  There is no tolerance anywhere in this file.

One unpoisoned warm-up call per mode comes first: it fixes the process-level tuning choices (projection forms, GEMM schedules), which
change the fp32 summation order; its result is discarded.

Prompts: `_prompts(3, 4, 32000, seed)` - 12 questions, 4 per image, prefix 35 + 576 = 611 keys (9 chunks of 64 and a tail of 35), own
lengths 19 - 28, 12 new tokens, and an EOS set drawn by `_eos_set(1500, 3)` (1,500 ids, seed 3: 4.6 % of the vocabulary, what the list
tests use) so that the answers of one run end at different steps - every run asserts min < max of its answer lengths."""
import contextlib
import gc
import inspect

import pytest
import torch

from poison import holds_pattern, poisoned_alloc, scrub
from test_engine_shapes_gpu import _engine, _prompts
from test_generate_list_gpu import W7B, _answer_lengths, _eos_set

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATTERNS = ("zero", "nan", "big")
N_NEW = 12
ENGINE_MODULE = "llava_align_amd.engine"


# ------------------------------------------------------------------ engines: weights once per module, a new engine per run
@pytest.fixture(scope="module")
def base():
    """cfg + random weights of `_engine(W7B, n_layers=2, vit_layers=2)`, built once; the load_8bit forms quantise their weights in place,
    so each of them gets a weight set of its own (same seed), built at first use."""
    e = _engine(W7B, n_layers=2, vit_layers=2)
    state = {"cfg": e.cfg, None: e.w}
    del e
    _release()
    return state


def _release():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _fresh(base, use_graph=True, load_8bit=False, w8_only=False):
    from llava_align_amd.engine import LlavaWeights, VddLlavaEngine
    wkey = ("w8", w8_only) if load_8bit else None
    if wkey not in base:
        base[wkey] = LlavaWeights.random(base["cfg"], DEV, seed=5, std=0.02, lm_head_gain=2.0)          # `_engine`'s weights
    return VddLlavaEngine(base["cfg"], weights=base[wkey], device=DEV, use_graph=use_graph, load_8bit=load_8bit, w8_only=w8_only)


# ------------------------------------------------------------------ results as bits
def _bits(out, eos):
    """tokens, step-0 top-10 and every score row of a call, the floating ones through an integer view"""
    iv = {2: torch.int16, 4: torch.int32}
    snap = {"tokens": out.tokens.clone()}
    if out.top_tok is not None:
        snap["top_tok"] = out.top_tok.clone()
        snap["top_prob"] = out.top_prob.contiguous().view(iv[out.top_prob.element_size()]).clone()
    if out.scores is not None:
        for i, s in enumerate(out.scores):
            snap[f"scores[{i}]"] = s.contiguous().view(iv[s.element_size()]).clone()
    la = _answer_lengths(out.tokens, eos)
    assert int(la.min()) < int(la.max()), f"every answer has {int(la.min())} tokens: the EOS set ends none early"
    return snap


def _same_bits(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape, f"{what}: {k} has shapes {tuple(a[k].shape)} and {tuple(b[k].shape)}"
        if not torch.equal(a[k], b[k]):
            rows = (a[k] != b[k]).reshape(a[k].shape[0], -1).any(1).nonzero().flatten().tolist()
            raise AssertionError(f"{what}: {k} differs in rows {rows}")


def _lines(qualname):
    """first and last source line of `Class.function` of engine.py"""
    from llava_align_amd import engine as obj
    for part in qualname.split("."):
        obj = getattr(obj, part)
    src, first = inspect.getsourcelines(obj)
    return first, first + len(src) - 1


def _kvcache_lines():
    return _lines("KVCache.__init__")


# ------------------------------------------------------------------ the calls
EOS = _eos_set(1500, 3)
COMMON = dict(cd_alpha=1.0, cd_beta=0.1, max_new_tokens=N_NEW, eos_token_id=EOS, pad_token_id=0, n_top=10)
GEN = dict(COMMON, cd_greedy=True, output_scores=True, temperature=0.5)
LIST = dict(COMMON, cd_greedy=True, temperature=0.5, in_flight=5, admit_min=2, sync_every=2)


def _small(seed=61):
    return _prompts(3, 4, 32000, seed=seed)


def _noised(imgs, seed=9):
    """one noised image per question (the VCD branch), the same noise for the questions about one image"""
    g, made = torch.Generator().manual_seed(seed), {}
    for im in imgs:
        if id(im) not in made:
            made[id(im)] = im + 0.8 * torch.randn(im.shape, generator=g)
    return [made[id(im)] for im in imgs]


def _embedding_prompts(n=6):
    from test_generate_list_grouped_gpu import _embedding_prompts as full
    emb, pre, emb_cd = full()
    return emb[:n], pre[:n], emb_cd[:n]


class Mode:
    """call(eng) -> GenerateOutput;  scope() -> the ops mode the call runs under;  marker(stats): the path named by the id is the path
    that ran;  eng_kw: how the engine is built;  eos: the EOS set of the call (answer lengths)"""

    def __init__(self, call, marker, scope=contextlib.nullcontext, eng_kw=None, eos=EOS, prepare=None, sites=()):
        self.call, self.marker, self.scope, self.eng_kw, self.eos, self.prepare = call, marker, scope, eng_kw or {}, eos, prepare
        self.sites = sites                   # functions of engine.py whose allocations the census of this mode must hold


def _inv():
    from llava_align_amd import ops
    return ops.batch_invariant()


def _inv_shared():
    from llava_align_amd import ops
    return ops.batch_invariant(shared_prefix=True)


def _tuned(eng, seed=61):
    ids, imgs = _small(seed)
    return eng.generate(ids, images=imgs, use_dd_unk=True, **GEN)


def _tuned_vcd(eng):
    ids, imgs = _small()
    return eng.generate(ids, images=imgs, images_cd=_noised(imgs), **GEN)


def _both_top_p(eng):
    ids, imgs = _small()
    kw = dict(GEN, cd_greedy=False, temperature=1.0)
    return eng.generate(ids, images=imgs, use_dd=True, use_dd_unk=True, top_p=0.9, seed=7, **kw)


def _design_6d(eng):
    """the exact call of DESIGN section 6d "Known defect" (tests/test_generate_list_grouped_gpu.py, case six_per_image)"""
    ids, imgs = _prompts(5, 6, 32000, seed=17)
    return eng.generate(ids, images=imgs, sync_every=4, cd_alpha=1.0, cd_beta=0.1, cd_greedy=True, use_dd_unk=True, temperature=0.5,
                        max_new_tokens=24, eos_token_id=EOS, pad_token_id=0, n_top=10)


RETIRE_EOS = _eos_set(6000, 3)         # ~17 % of the vocabulary: half of the answers end within four steps, so rows retire


def _retire_prepare(eng):
    eng.retire, eng.kv_chunk = True, 4              # retirement needs max_new_tokens > kv_chunk (and no output_scores)


def _retire(eng):
    ids, imgs = _small()
    kw = dict(COMMON, cd_greedy=True, temperature=0.5, eos_token_id=RETIRE_EOS, max_new_tokens=16, sync_every=2)
    return eng.generate(ids, images=imgs, use_dd_unk=True, **kw)


def _retire_marker(st):
    assert st["retire_events"] >= 1 and st["rows_at_end"] < st["n_rows"], st        # rows left: KVCache.repack_own made new pools


EMB_EOS = _eos_set(900, 5)


def _embeds(eng):
    emb, pre, _ = _embedding_prompts()
    kw = dict(GEN, temperature=0.7, eos_token_id=EMB_EOS)
    return eng.generate(None, inputs_embeds=emb, embeds_prefix=pre, use_dd_unk=True, **kw)


def _list(eng, **extra):
    ids, imgs = _small()
    return eng.generate_list(ids, imgs, use_dd_unk=True, **dict(LIST, **extra))


_TIGHT = {}              # prompt seed and page budget of `list_paged_tight`, settled by its warm-up call


def _list_paged_tight(eng):
    """A page pool so tight that questions are preempted.  Whether a pool preempts depends on the answer lengths, which only a run
    gives: the unpoisoned warm-up call runs with the worst-case pool (no preemption; its answers are the contiguous list's) and hands
    its answer lengths to the host model of the pager (paged_kv.walk_list_schedule, which tests/test_generate_list_paged_gpu.py holds
    equal to the engine's own count).  The budget is the largest one, from the formula of
    test_tuned_paged_grouped_list_gives_the_contiguous_grouped_tokens (one question at full length + 1 + 4 pages) down to the smallest
    pool the pager takes (one question at full length + 1), for which the model preempts; prompt seeds with six own lengths of 26 - 28
    tokens (rows that cross the 32-token page boundary after a few steps) are tried in turn.  The patterned runs assert the engine's count."""
    from llava_align_amd.paged_kv import PAGE, walk_list_schedule
    kw = dict(LIST, use_dd_unk=True, paged_kv=True)
    if not _TIGHT:
        for seed in (64, 66, 72):
            ids, imgs = _small(seed)
            out = eng.generate_list(ids, imgs, **kw)
            suffix = [len(r) - r.tolist().index(-200) - 1 for r in ids]
            lens = _answer_lengths(out.tokens, EOS).tolist()
            full = 2 * -(-(max(suffix) + N_NEW) // PAGE)
            for budget in range(full + 1 + 4, full, -1):
                w = walk_list_schedule(suffix, lens, LIST["in_flight"], 2, N_NEW, sync_every=LIST["sync_every"], admit_min=LIST["admit_min"], kv_page_budget=budget)
                if w["preemptions"] > 0:
                    _TIGHT.update(seed=seed, budget=budget)
                    print(f"list_paged_tight: seed {seed}, answer lengths {lens}, {budget} pages, {w['preemptions']} preemptions expected")
                    return out
        raise AssertionError("no page budget preempts a question of these lists")
    ids, imgs = _small(_TIGHT["seed"])
    return eng.generate_list(ids, imgs, kv_page_budget=_TIGHT["budget"], **kw)


def _graph(st):
    assert st["graph"], st


def _shared(st):
    assert st["graph"] and st["n_groups"] > 0 and st["shared_rows"] > 0, st


def _list_marker(st):
    assert st["graph"] and st["admissions"] >= 3, st


def _paged_marker(st):
    assert st["graph"] and st["paged_kv"] and st["preemptions"] > 0, st


def _grouped_list(st):
    assert st["graph"] and st["n_groups"] > 0 and st["group_images"] is True and st["admissions"] >= 3, st


def _grouped_list_inv(st):
    _grouped_list(st)
    assert st["shared_rows"] > 0, st


def _no_graph(st):
    assert not st["graph"], st


MODES = {
    "tuned": Mode(_tuned, _graph, sites=("VisionTower._kv_cache", "_DecodeRunner.__init__", "VddLlavaEngine._pack")),
    "tuned_vcd": Mode(_tuned_vcd, _graph),
    "both_top_p": Mode(_both_top_p, _graph),
    "invariant": Mode(_tuned, _graph, scope=_inv),
    "invariant_shared": Mode(_tuned, _shared, scope=_inv_shared),
    "invariant_shared_6d": Mode(_design_6d, _shared, scope=_inv_shared),
    "invariant_shared_vcd": Mode(_tuned_vcd, _shared, scope=_inv_shared),
    "retire": Mode(_retire, _retire_marker, scope=_inv, eos=RETIRE_EOS, prepare=_retire_prepare, sites=("KVCache.repack_own",)),
    "embeds": Mode(_embeds, _graph, eos=EMB_EOS),
    "list": Mode(_list, _list_marker),
    "list_paged_tight": Mode(_list_paged_tight, _paged_marker),
    "list_grouped": Mode(lambda eng: _list(eng, group_images=True), _grouped_list),
    "list_grouped_inv": Mode(lambda eng: _list(eng, group_images=True), _grouped_list_inv, scope=_inv_shared),
    "w8": Mode(_tuned, _graph, eng_kw=dict(load_8bit=True)),
    "w8_only": Mode(_tuned, _graph, eng_kw=dict(load_8bit=True, w8_only=True)),
    "no_graph": Mode(_tuned, _no_graph, eng_kw=dict(use_graph=False)),
}


# ------------------------------------------------------------------ the poison is really there
def test_the_poison_is_in_the_buffers_before_any_kernel_runs(base):
    from llava_align_amd import ops
    from llava_align_amd.engine import KVCache
    lm = base["cfg"].lm
    first, last = _kvcache_lines()
    for pattern in ("nan", "big"):
        with poisoned_alloc(pattern) as census:
            ws = ops.attention_workspace(2, 32, 128, 128, DEV)
            kv = KVCache(lm, 1, 64, 2, 64, DEV, torch.bfloat16)
            idx = torch.empty(8, dtype=torch.float32, device=DEV)                      # called from this module: not the package's
        assert ws.dtype == torch.float32 and ws.numel() > 0 and holds_pattern(ws, pattern)
        assert holds_pattern(kv.ko[0], pattern) and holds_pattern(kv.kp[-1], pattern) and holds_pattern(kv.vo[-1], pattern)
        if pattern == "big":
            assert bool((ws == 3.0e4).all()) and bool((kv.ko[0].float() == torch.tensor(3.0e4).bfloat16().float()).all())
        assert census.bytes == ws.numel() * 4 + kv.nbytes() and census.bytes_in(ENGINE_MODULE, first, last) == kv.nbytes()
        assert census.calls == census.filled == 1 + 4 * lm.n_layers and idx.numel() == 8
        del ws, kv


# ------------------------------------------------------------------ fresh engines under the three patterns
@pytest.mark.parametrize("mode", sorted(MODES))
def test_answers_do_not_depend_on_what_fresh_buffers_hold(base, mode):
    m = MODES[mode]
    first, last = _kvcache_lines()
    snaps = {}
    for pattern in (None,) + PATTERNS:                        # None: the unpoisoned warm-up, result discarded
        with (poisoned_alloc(pattern) if pattern else contextlib.nullcontext()) as census:
            eng = _fresh(base, **m.eng_kw)
            if m.prepare:
                m.prepare(eng)
            with m.scope():
                out = m.call(eng)
            torch.cuda.synchronize()
        if pattern:
            m.marker(out.stats)
            pools = max(kv.nbytes() for kv in eng._kvs.values())
            assert census.bytes >= eng._kv.nbytes() and census.bytes_in(ENGINE_MODULE, first, last) >= pools, (census.bytes, pools)
            for fn in m.sites:
                assert census.bytes_in(ENGINE_MODULE, *_lines(fn)) > 0, f"{mode} [{pattern}]: nothing allocated in {fn}: {sorted(census.sites)}"
            snaps[pattern] = _bits(out, m.eos)
            print(f"{mode} [{pattern}]: {census.calls} allocator calls, {census.bytes:,d} bytes poisoned, pools {pools:,d}")
            if mode in ("invariant_shared", "tuned") and pattern == "nan":
                print(census.table())
        del eng, out
        _release()
    _same_bits(snaps["zero"], snaps["nan"], f"{mode}: zero against nan")
    _same_bits(snaps["zero"], snaps["big"], f"{mode}: zero against big")


# ------------------------------------------------------------------ one engine, stale state, captured graphs kept
def _call_b(mode):
    """other questions over the same slots: another seed, more images (other pixels), longer questions"""
    ids, imgs = _prompts(4, 4, 32000, seed=62)
    g = torch.Generator().manual_seed(63)
    ids = [torch.cat([r, torch.randint(3, 32000, (int(n),), generator=g)]) for r, n in zip(ids, torch.randint(5, 12, (len(ids),), generator=g))]
    other = {}
    for im in imgs:
        other.setdefault(id(im), -im)
    imgs = [other[id(im)] for im in imgs]
    if mode.startswith("list"):
        return lambda eng: eng.generate_list(ids, imgs, use_dd_unk=True, group_images=True, **LIST)
    return lambda eng: eng.generate(ids, images=imgs, use_dd_unk=True, **GEN)


@pytest.mark.parametrize("mode", ["tuned", "invariant_shared", "list_grouped_inv"])
def test_answers_do_not_depend_on_what_a_previous_call_left_behind(base, mode):
    m = MODES[mode]
    eng = _fresh(base, **m.eng_kw)
    call_b = _call_b(mode)
    with m.scope():
        a0 = m.call(eng)
        m.marker(a0.stats)
        a0 = _bits(a0, m.eos)
        pools = sum(kv.nbytes() for kv in eng._kvs.values())
        for pattern in ("nan", "big"):                        # the same call over scrubbed pools: addresses unchanged, graphs replayed
            graphs = len(eng._graphs)
            assert scrub(eng, pattern) >= pools
            out = m.call(eng)
            m.marker(out.stats)
            assert len(eng._graphs) == graphs
            _same_bits(a0, _bits(out, m.eos), f"{mode}: after scrub({pattern})")
        b = call_b(eng)                                       # every slot now holds someone else's keys
        assert b.tokens.shape[0] == 16
        out = m.call(eng)
        m.marker(out.stats)
        _same_bits(a0, _bits(out, m.eos), f"{mode}: A after B")
    del eng
    _release()
