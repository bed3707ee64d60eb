"""load_8bit where it still streamed w16: the batch-invariant mode (the drivers' own choice for every deterministic decode), the 17 - 64-row
weight-streaming forms and layer 0's qkv of the few-row step - each against the same call with ops.W8_DECODE off over ONE quantised model,
bit for bit in every score of every step.  The engines are the load_8bit engines of tests/test_w8_gemm_engine_gpu.py (two decoder layers at
LLaVA-1.5-7B widths, and the tiny preset).

In batch-invariant mode a projection with codes is the GEMM's data-parallel schedule on w16 ("gemm") or on the codes ("gemm8"), whichever
was measured faster, under kinds of its own ("linear8i", "to_norm8i", "swiglu8i").  The tests that must see 8-bit launches force those
kinds to "gemm8" - which form wins a timing run is not a property to assert - and the GEMM's tile is tuned for real, under choice tables
of the module's own that neither read nor write a persisted file."""
import json

import pytest
import torch

from test_engine_shapes_gpu import _compare, _prompts
from test_w8_gemm_engine_gpu import _bits, _engine, _engines

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS8 = ("linear8", "to_norm8", "swiglu8")


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _engines.clear()


_gemm_tiles = {}          # the module's GEMM tile choices, tuned once and shared by its tests (the prefill's shapes repeat in every one)


def _fresh_tables(monkeypatch, ops, force):
    monkeypatch.setattr(ops, "_gemm_choice", _gemm_tiles)
    monkeypatch.setattr(ops, "_form_choice", {})
    monkeypatch.setattr(ops, "_load_persisted", lambda device: None)
    monkeypatch.setattr(ops, "_persist", {"loaded": None, "path": None, "section": None})
    monkeypatch.setattr(ops, "FORCE_FORM", dict(force))


def _same_scores(a, b, qa=None, qb=None):
    assert len(a.scores) == len(b.scores) and len(a.scores) >= 4
    for step, (sa, sb) in enumerate(zip(a.scores, b.scores)):
        sa, sb = (sa if qa is None else sa[qa]), (sb if qb is None else sb[qb])
        assert torch.equal(_bits(sa), _bits(sb)), step


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_batch_invariant_mode_streams_codes_and_keeps_its_bits(monkeypatch, dtype):
    """12 questions x 2 branches, cd_greedy, under ops.batch_invariant(): 8-bit launches happen (none did before the mode read codes), every
    tuned GEMM on codes took the data-parallel schedule, every score equals the run with the switch off - and question 0 decoded alone
    equals question 0 inside the batch, the mode's own promise, with the codes on."""
    from llava_align_amd import ops
    _fresh_tables(monkeypatch, ops, {k + ops.INVARIANT_KIND_SUFFIX: "gemm8" for k in KINDS8})
    eng = _engine("7b", dtype)
    lm = eng.cfg.lm
    ids, imgs = _prompts(12, 1, lm.vocab, seed=43)
    kw = dict(use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.6, max_new_tokens=4, cd_greedy=True, output_scores=True)
    with ops.batch_invariant():
        n0 = ops.w8_launches()
        a = eng.generate(ids, images=imgs, **kw)
        n1 = ops.w8_launches()
        assert a.stats["n_rows"] == 24
        assert n1 >= n0 + 4 * lm.n_layers + 1                   # qkv, o, gate/up, down of every layer and the head (a captured launch counts once)
        w8_keys = [k for k in ops._gemm_choice if k[-1] > 8]
        assert w8_keys and all(k[4] is True and (ops._gemm_choice[k] >> 4) & 3 == 1 for k in w8_keys)
        assert all((ops._gemm_choice[k] & 15) | ((ops._gemm_choice[k] >> 6) << 4) in ops.W8_GEMM_TILES for k in w8_keys)
        one = eng.generate(ids[:1], images=imgs[:1], **kw)
        assert ops.w8_launches() >= n1 + 4 * lm.n_layers + 1 and one.stats["n_rows"] == 2
        n2 = ops.w8_launches()
        with ops.w8_decode(False):
            b = eng.generate(ids, images=imgs, **kw)
        assert ops.w8_launches() == n2
    # no tuned-mode key and no 16-bit key was written by the mode's choices on codes
    assert not any(k[0] in KINDS8 for k in ops._form_choice)
    _same_scores(a, b)
    assert torch.equal(a.tokens, b.tokens)
    _same_scores(a, one, 0, 0)
    assert torch.equal(a.tokens[0], one.tokens[0])


def test_the_invariant_choice_is_measured_under_kinds_of_its_own(monkeypatch):
    """Unforced: each projection's "gemm" / "gemm8" choice of the mode lands under kind + "i" (never under a tuned-mode kind), holds one of
    the two names, and the bits are those of the switch off whichever won."""
    from llava_align_amd import ops
    _fresh_tables(monkeypatch, ops, {})
    eng = _engine("7b")
    lm = eng.cfg.lm
    ids, imgs = _prompts(12, 1, lm.vocab, seed=47)
    kw = dict(images=imgs, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.8, max_new_tokens=4, cd_greedy=True, output_scores=True)
    with ops.batch_invariant():
        a = eng.generate(ids, **kw)
        with ops.w8_decode(False):
            b = eng.generate(ids, **kw)
    kinds = {k[0]: v for k, v in ops._form_choice.items() if k[0] != "layer"}
    assert set(kinds) == {k + "i" for k in KINDS8} and set(kinds.values()) <= {"gemm", "gemm8"}
    _same_scores(a, b)


@pytest.mark.parametrize("nb", [2, 3], ids=["24rows", "36rows"])
def test_tuned_mode_skinny8_equals_the_switch_off(monkeypatch, nb):
    """The weight-streaming forms on codes at 24 and 36 rows (two and three MFMA row tiles; the head's 32-column blocks), forced for the
    three 8-bit kinds, against "skinny" on w16."""
    from llava_align_amd import ops
    _fresh_tables(monkeypatch, ops, {**{k: "skinny8" for k in KINDS8}, "linear": "skinny", "to_norm": "skinny", "swiglu": "skinny"})
    eng = _engine("7b")
    lm = eng.cfg.lm
    ids, imgs = _prompts(12, 1, lm.vocab, seed=51 + nb)
    kw = dict(images=imgs, use_dd_unk=True, use_dd=nb == 3, cd_alpha=1.0, cd_beta=0.1, temperature=0.9, max_new_tokens=4, cd_greedy=True,
              output_scores=True)
    on_codes = {k for k in ops._gemm_choice if k[-1] > 8}
    n0 = ops.w8_launches()
    a = eng.generate(ids, **kw)
    n1 = ops.w8_launches()
    assert a.stats["n_rows"] == 12 * nb and n1 >= n0 + 4 * lm.n_layers + 1
    assert {k for k in ops._gemm_choice if k[-1] > 8} == on_codes      # no GEMM on codes was tuned: the launches were the weight-streaming kernels'
    with ops.w8_decode(False):
        b = eng.generate(ids, **kw)
    assert ops.w8_launches() == n1
    _same_scores(a, b)
    assert torch.equal(a.tokens, b.tokens)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_few_row_step_streams_layer0_qkv_as_codes(monkeypatch, dtype):
    """One question, two rows, the fused layer forced (and "skinny8" for its one plain projection, layer 0's qkv): every call of the
    few-row step issues 4 * n_layers + 1 8-bit launches - qkv, o, gate/up, down of every layer and the head; layer 0's qkv was 16-bit."""
    from llava_align_amd import ops
    from llava_align_amd.engine import LanguageModel
    _fresh_tables(monkeypatch, ops, {"linear8t": "skinny8", "linear": "skinny"})
    monkeypatch.setattr(ops, "FORCE_LAYER_FORM", "fused")
    eng = _engine("7b", dtype)
    lm = eng.cfg.lm
    per_call = []
    step = LanguageModel._decode_step_few_rows

    def counted(self, *args, **kwargs):
        n = ops.w8_launches()
        out = step(self, *args, **kwargs)
        per_call.append(ops.w8_launches() - n)
        return out
    monkeypatch.setattr(LanguageModel, "_decode_step_few_rows", counted)
    ids, imgs = _prompts(1, 1, lm.vocab, seed=57)
    kw = dict(images=imgs, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.4, max_new_tokens=4, cd_greedy=True, output_scores=True)
    a = eng.generate(ids, **kw)
    assert a.stats["n_rows"] == 2 and per_call and set(per_call) == {4 * lm.n_layers + 1}
    n_on = len(per_call)
    with ops.w8_decode(False):
        b = eng.generate(ids, **kw)
    assert len(per_call) > n_on and set(per_call[n_on:]) == {0}
    _same_scores(a, b)
    assert torch.equal(a.tokens, b.tokens)


def test_load_8bit_engine_at_36_rows_with_skinny8_among_the_forms_matches_the_fp32_reference():
    """Unpinned: every projection in the form its tuner measures, the weight-streaming kernels on codes among the candidates, held to the
    fp32 reference of the engine's own w16 weights with the tolerance of tests/test_w8_engine_gpu.py."""
    import copy

    from ref_llava import RefLlava
    eng = _engine("7b")
    w16 = copy.copy(eng.w)
    w16.t = {k: v for k, v in eng.w.t.items() if not k.endswith((".w8", ".w8s"))}
    ref = RefLlava(w16, device=DEV)
    ids, imgs = _prompts(12, 1, 32000, seed=61)
    out, checked = _compare(eng, ref, ids, imgs, dict(use_dd_unk=True, use_dd=True), dict(temperature=0.5), n_new=4, questions=range(12), tol=0.5)
    assert out.stats["n_rows"] == 36 and checked >= 1


def test_a_deterministic_pope_run_streams_codes(monkeypatch, tmp_path):
    """pope_driver.run_pope in its default mode (a cd_greedy run selects the batch-invariant mode itself) on a load_8bit tiny engine: 8-bit
    launches happen, and the answers file is the one written with the switch off."""
    from llava_align_amd import ops
    from llava_align_amd.pope_driver import run_pope
    from test_pope_driver_gpu import decode, encode
    _fresh_tables(monkeypatch, ops, {k + ops.INVARIANT_KIND_SUFFIX: "gemm8" for k in KINDS8})
    eng = _engine("tiny")
    assert eng.w.w8("l0.wqkv") is not None
    images = {f"img{i}.jpg": torch.randn(3, 56, 56, generator=torch.Generator().manual_seed(40 + i)) for i in range(3)}
    questions = [{"question_id": 100 + i, "image": f"img{i % 3}.jpg", "text": f"q{i}", "label": ("yes", "no")[i % 2]} for i in range(9)]
    kw = dict(model_id="tiny", batch_questions=6, unk_token_id=0, max_new_tokens=4, use_dd_unk=True, cd_alpha=1.0, cd_beta=0.1, temperature=0.5,
              cd_greedy=True)
    n0 = ops.w8_launches()
    a = run_pope(eng, questions, encode, decode, lambda n: images[n], answers_path=str(tmp_path / "on.jsonl"), **kw)
    n1 = ops.w8_launches()
    assert a["batch_invariant"] and n1 > n0
    with ops.w8_decode(False):
        b = run_pope(eng, questions, encode, decode, lambda n: images[n], answers_path=str(tmp_path / "off.jsonl"), **kw)
    assert ops.w8_launches() == n1
    on, off = [[json.loads(l) for l in open(tmp_path / f)] for f in ("on.jsonl", "off.jsonl")]
    assert len(on) == 9 and on == off
    assert a["answers"] == b["answers"]
