"""What the five evaluation drivers (pope_driver, mme_driver, qwen_driver, blip_driver, sampling_driver) do alike, as plain functions and
two small classes; what makes each driver worth having - which passes a batch runs, which priors, what its JSONL record looks like -
stays in its `run_*`, which reads top to bottom and calls these.

  ShardedRun              image-sorted order, ShardPlan, this rank's questions, the rank's seed offset, batch-invariant mode (+ its shared-prefix form)
  ResultRows              a rank's per-question results in the layout of the one result gather (shard.gather_results), with or without top lists
  distinct / to_all_rows  every DISTINCT prompt runs once; its step-0 top list goes back to all the rows that asked it
  load_distinct_images    one tensor OBJECT per image name (the engine shares ViT features and prefix KV by tensor identity)
  eos_set / answer_text   generated ids -> the answer string
  write_jsonl             the answers file (callers: rank 0 only)
  pope_scores_for         the plain and the calibrated POPE scorers, None where the reference's scorer divides by zero
  PRIOR_KW / plain_kw / sweep_settings / setting_kw / sweep_result     the prior passes' kwargs and the sampling sweeps
  add_common_args / add_script_args / chunk_of / read_questions / finish_distributed     the command lines

The command-line defaults differ per driver ON PURPOSE (each follows its reference script); add_common_args takes them from the caller:

  option          pope      mme          qwen         blip      sampling
  --image-folder  required  required     ""           ""        ""
  --temperature   1.0       None (*)     None (*)     1.0       1.0
  --top_p         None      None         None         1.0       None
  --noise_step    None      500          500          500       500
  --seed          None      None         42           42        42
  --dtype         float16   float16      bfloat16     float16   float16
  --batch         384       256          128          128       (--in-flight 90)
  (*) resolved after parsing: mme 0.2 (llava) / 1.0 (qwen); qwen 0.2, --sampling runs at 1.0
--question-file / --answers-file are required, --top_k is None, --cd_alpha 1.0 and --cd_beta 0.1 everywhere.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
from typing import Callable, Dict, List, Optional, Sequence

import torch

from . import calibrate as C
from . import ops
from .shard import ShardPlan, gather_results, get_chunk, resolve_batch_invariant

QUESTION_SUFFIX = " Please answer this question with one word."      # llava_calibrate.py:52,146; blip_calibrate.py:42,74; llava_sampling.py:71-76
PRIOR_KW = ("temperature", "top_p", "top_k", "seed", "cd_alpha", "cd_beta")      # what a content-free prior pass keeps of the generate kwargs: plain sampling
SWEEP_KW = ("temperature", "top_p", "top_k")                                     # what a sweep setting overrides


class ShardedRun:
    """One driver call's share of the question list: the questions sorted by (image, index) so that one image's questions are
    adjacent, split over the ranks by whole images (shard.ShardPlan; rank / world default to the initialised torch.distributed group, else
    one rank), an explicit `seed` offset by the rank, and whether the decode runs in batch-invariant mode (shard.resolve_batch_invariant)."""

    def __init__(self, questions: Sequence[dict], rank: Optional[int], world: Optional[int], generate_kw: dict, batch_invariant: Optional[bool],
                 invariant_shared_prefix: bool = False):
        order = sorted(range(len(questions)), key=lambda i: (questions[i]["image"], i))
        self.questions = questions
        self.plan = ShardPlan([questions[i]["image"] for i in order], rank, world)
        self.mine = [order[p_] for p_ in self.plan.mine]
        self.rank, self.world = self.plan.rank, self.plan.world
        if generate_kw.get("seed") is not None:
            generate_kw = dict(generate_kw, seed=int(generate_kw["seed"]) + self.rank)
        self.generate_kw = generate_kw
        self.invariant = resolve_batch_invariant(batch_invariant, self.world, generate_kw)
        # the mode's shared-prefix form (ops.INVARIANT_SHARED_PREFIX: image prefixes once per image, still batch-invariant): opt-in, and only
        # where the run is in the mode at all
        self.shared_prefix = bool(invariant_shared_prefix) and self.invariant

    def mode(self):
        return ops.batch_invariant(shared_prefix=self.shared_prefix) if self.invariant else contextlib.nullcontext()

    def batches(self, n: int):
        for b0 in range(0, len(self.mine), n):
            idx = self.mine[b0:b0 + n]
            yield idx, [self.questions[i] for i in idx]

    def rows(self, device, width: int, pad_token_id: Optional[int], n_sets: int) -> "ResultRows":
        return ResultRows(device, width, pad_token_id if pad_token_id is not None else 0, n_sets)

    def gather(self, rows: "ResultRows") -> dict:
        """ONE collective; every rank holds every question's results behind it."""
        return rows.gather(self.plan, len(self.questions))


def cut_at_eos(toks: List[int], eos_set) -> List[int]:
    for k, t in enumerate(toks):                       # cut at the first EOS (the rest is padding)
        if t in eos_set:
            return toks[:k + 1]
    return toks


class ResultRows:
    """Per-question results of a rank's chunk as device tensors - generated ids (padded to `width` columns) and the step-0 top-10
    (token, probability) lists of the main pass and of the prior passes side by side - in the layout of the one result gather
    (shard.gather_results).  n_sets = 0: answers only."""

    def __init__(self, device, width: int, pad: int, n_sets: int, k: int = 10):
        self.device, self.width, self.pad, self.n_sets, self.k = device, int(width), int(pad), n_sets, k
        self.qids: List[int] = []
        self.tokens, self.n_tok, self.top_tok, self.top_prob = [], [], [], []

    def add(self, qids: Sequence[int], main_tokens: torch.Tensor, tops: Sequence = ()):
        """tops: one (top_tok [n, k], top_prob [n, k]) pair per set, main pass first."""
        n, T = main_tokens.shape
        assert len(tops) == self.n_sets and T <= self.width and n == len(qids)
        self.qids += list(qids)
        self.tokens.append(torch.nn.functional.pad(main_tokens, (0, self.width - T), value=self.pad))
        self.n_tok.append(torch.full((n,), T, dtype=torch.long, device=self.device))
        if tops:
            self.top_tok.append(torch.cat([t for t, _ in tops], 1))
            self.top_prob.append(torch.cat([p_ for _, p_ in tops], 1))

    def gather(self, plan, n_total: int) -> dict:
        """-> host lists for ALL questions on every rank: tokens[i] (valid columns only), tops[s][i] = (tok list, prob list)."""
        dev, k = self.device, self.n_sets * self.k
        z = lambda *shape, dt=torch.long: torch.zeros(*shape, dtype=dt, device=dev)
        tops = (None, None) if not k else (torch.cat(self.top_tok) if self.top_tok else z(0, k), torch.cat(self.top_prob) if self.top_prob else z(0, k, dt=torch.float32))
        res = gather_results(torch.tensor(self.qids, dtype=torch.long, device=dev),
                             torch.cat(self.tokens) if self.tokens else z(0, self.width), torch.cat(self.n_tok) if self.n_tok else z(0), *tops,
                             n_total, pad=self.pad, capacity=plan.capacity, width=self.width, world=plan.world)
        if not bool((res["count"] == 1).all().item()):
            raise RuntimeError(f"result gather: {int((res['count'] != 1).sum())} of {n_total} questions were not delivered exactly once")
        n_tok, toks = res["n_tokens"].cpu().tolist(), res["tokens"].cpu().tolist()
        out = {"tokens": [r[:n] for r, n in zip(toks, n_tok)], "tops": []}
        if k:
            tt, tp, K = res["top_tok"].cpu().tolist(), res["top_prob"].cpu().tolist(), self.k
            out["tops"] = [[(tt[i][s_ * K:(s_ + 1) * K], tp[i][s_ * K:(s_ + 1) * K]) for i in range(n_total)] for s_ in range(self.n_sets)]
        return out


def distinct(keys: Sequence) -> tuple:
    """-> (pick, where): pick = the indices of the first occurrences, in order; where[i] = the position of keys[i] in pick.  POPE asks the same
    few dozen questions about hundreds of images, and a content-free prompt's step-0 label dict is a function of the prompt alone (the top-n of
    the warped distribution: nothing is drawn): run [rows[i] for i in pick], then `to_all_rows`."""
    first: Dict = {}
    pick = []
    for i, k in enumerate(keys):
        if k not in first:
            first[k] = len(pick)
            pick.append(i)
    return pick, [first[k] for k in keys]


def to_all_rows(out, where: Sequence[int]) -> tuple:
    """(top_tok, top_prob) of a pass over the distinct rows, indexed back to all rows."""
    back = torch.tensor(where, dtype=torch.long).to(out.top_tok.device, non_blocking=True)
    return out.top_tok[back], out.top_prob[back]


def load_distinct_images(names: Sequence[str], load_image: Callable[[str], torch.Tensor], device) -> List[torch.Tensor]:
    """-> one tensor per name, THE SAME OBJECT for the same name: the engine shares an image's features and prompt-prefix KV by tensor identity."""
    cache: Dict[str, torch.Tensor] = {}
    for name in names:
        if name not in cache:
            cache[name] = load_image(name).to(device)
    return [cache[name] for name in names]


def eos_set(eos_token_id) -> set:
    return set([eos_token_id] if isinstance(eos_token_id, int) else (eos_token_id or []))


def answer_text(decode: Callable[[List[int]], str], tokens: List[int], eos, stop_str: Optional[str] = None) -> str:
    text = decode(cut_at_eos(tokens, eos)).strip()
    if stop_str and text.endswith(stop_str):
        text = text[:-len(stop_str)]
    return text.strip()


def write_jsonl(path: str, records: Sequence[dict]) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")


def pope_scores_for(questions: Sequence[dict], answers: Sequence[dict], names: Sequence[str]) -> dict:
    """{name: scores} - 'string_match' = calibrate.pope_scores, any other name = calibrate.pope_scores_calibrated with that prior - or {} unless
    every question carries its label.  None: the reference scorers divide by tp + fp etc., undefined on degenerate (tiny / random) runs."""
    if not all("label" in q for q in questions):
        return {}
    gt = [{"question_id": q["question_id"], "label": q["label"]} for q in questions]
    scores = {}
    for name in names:
        try:
            scores[name] = C.pope_scores(gt, answers) if name == "string_match" else C.pope_scores_calibrated(gt, answers, name)
        except ZeroDivisionError:
            scores[name] = None
    return scores


def plain_kw(generate_kw: dict) -> dict:
    return {k: v for k, v in generate_kw.items() if k in PRIOR_KW}


def sweep_settings(sweep: Optional[Sequence[dict]]) -> List[dict]:
    return [dict(tag=None)] if sweep is None else [dict(s_) for s_ in sweep]


def setting_kw(generate_kw: dict, setting: dict) -> dict:
    return dict(generate_kw, **{k: setting[k] for k in SWEEP_KW if k in setting})


def sweep_result(sweep, settings: Sequence[dict], finish_one: Callable[[int, dict], dict], **top) -> dict:
    """finish_one(j, setting) -> the j-th setting's result.  No sweep: that result; a sweep: {"runs": {tag: result}, **top}."""
    if sweep is None:
        return finish_one(0, settings[0])
    return {"runs": {s_["tag"]: finish_one(j, s_) for j, s_ in enumerate(settings)}, **top}


REQUIRED = object()
_COMMON_ARGS = (("--image-folder", str, REQUIRED), ("--question-file", str, REQUIRED), ("--answers-file", str, REQUIRED), ("--temperature", float, None),
                ("--top_p", float, None), ("--top_k", int, None), ("--noise_step", int, 500), ("--cd_alpha", float, 1.0), ("--cd_beta", float, 0.1),
                ("--seed", int, None))


def add_common_args(ap, help: Optional[dict] = None, dtype: str = "float16", **defaults) -> None:
    """The options every driver's command line has.  defaults: {dest: the driver's default} where it is not the one above (the table in the module
    docstring); help: {dest: text}."""
    for flag, typ, default in _COMMON_ARGS:
        dest = flag[2:].replace("-", "_")
        default = defaults.pop(dest, default)
        ap.add_argument(flag, type=typ, help=(help or {}).get(dest), **(dict(required=True) if default is REQUIRED else dict(default=default)))
    ap.add_argument("--dtype", choices=("float16", "bfloat16"), default=dtype, help="model dtype (the reference loads LLaVA / Vicuna in fp16, builder.py:40)")
    ap.add_argument("--load-8bit", action="store_true", default=argparse.SUPPRESS, help="e4m3 weight storage for the few-row decode step (builder.py:26-31 load_8bit; VddLlavaEngine(load_8bit=True))")
    ap.add_argument("--w8-only", action="store_true", default=argparse.SUPPRESS,
                    help="with --load-8bit: keep the quantised language-model weights as e4m3 codes only - half the weight memory, every GEMM reads "
                         "codes (VddLlavaEngine(load_8bit=True, w8_only=True))")
    ap.add_argument("--invariant-shared-prefix", action="store_true", default=argparse.SUPPRESS,
                    help="batch-invariant runs only: read an image prefix once per image (ops.INVARIANT_SHARED_PREFIX); still the same answers at any batch "
                         "size and rank count, but not the bits of a run without the option; open-ended lists (generate_list) refuse it")
    if defaults:
        raise TypeError(f"not common options: {sorted(defaults)}")


def load_kw(a) -> dict:
    """The loader / engine keywords the common options select: `load_8bit=True` after --load-8bit, `w8_only=True` after --w8-only (the
    engine refuses it without --load-8bit), nothing otherwise."""
    kw = dict(load_8bit=True) if getattr(a, "load_8bit", False) else {}
    if getattr(a, "w8_only", False):
        kw["w8_only"] = True
    return kw


def mode_kw(a) -> dict:
    """The run keyword --invariant-shared-prefix selects (`invariant_shared_prefix=True`), nothing otherwise: off by default."""
    return dict(invariant_shared_prefix=True) if getattr(a, "invariant_shared_prefix", False) else {}


def add_script_args(ap, conv_mode: str = "llava_v1") -> None:
    """What the reference's MME / Qwen / InstructBLIP / sampling scripts take beside the common options: --num-chunks / --chunk-idx (get_chunk,
    MME/run_llava.py:32-40, :261-262; `chunk_of`), --use_cd, and --model-base / --conv-mode, which are parsed and unused."""
    ap.add_argument("--num-chunks", type=int, default=1)
    ap.add_argument("--chunk-idx", type=int, default=0)
    ap.add_argument("--use_cd", action="store_true")
    ap.add_argument("--model-base", default=None)
    ap.add_argument("--conv-mode", default=conv_mode)


def chunk_of(questions: list, a) -> list:
    if a.num_chunks > 1:
        return [questions[i] for i in get_chunk(len(questions), a.num_chunks, a.chunk_idx, group=1)]
    return questions


def read_questions(path: str) -> List[dict]:
    return [json.loads(q) for q in open(os.path.expanduser(path))]


def finish_distributed(world: int) -> None:
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
