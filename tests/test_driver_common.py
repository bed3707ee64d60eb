"""driver_common: the host logic the five evaluation drivers share (sharding preamble, distinct-prompt dedup, answer text, JSONL writing,
POPE scoring, result rows on one rank, command-line defaults).  No GPU: tensors live on the CPU and world = 1 exchanges nothing."""
import argparse
import json

import pytest
import torch

from llava_align_amd import driver_common as D


def test_distinct_first_occurrences_and_positions():
    assert D.distinct([]) == ([], [])
    assert D.distinct(["a", "b", "c"]) == ([0, 1, 2], [0, 1, 2])
    pick, where = D.distinct(["b", "a", "b", "c", "a", "b"])
    assert pick == [0, 1, 3] and where == [0, 1, 0, 2, 1, 0]
    assert D.distinct([(1, 2)] * 4) == ([0], [0, 0, 0, 0])                      # all equal: one row runs
    keys = ["q%d" % (i % 3) for i in range(10)]
    pick, where = D.distinct(keys)
    assert [keys[pick[w]] for w in where] == keys
    out = argparse.Namespace(top_tok=torch.arange(30).view(3, 10), top_prob=torch.arange(30.0).view(3, 10))
    tt, tp = D.to_all_rows(out, where)
    assert tt.shape == (10, 10) and all(torch.equal(tt[i], out.top_tok[i % 3]) and torch.equal(tp[i], out.top_prob[i % 3]) for i in range(10))


def test_cut_at_eos_and_answer_text():
    assert D.eos_set(None) == set() and D.eos_set(2) == {2} and D.eos_set([2, 5, 2]) == {2, 5}
    assert D.cut_at_eos([4, 5, 2, 0, 0], {2}) == [4, 5, 2] and D.cut_at_eos([2, 2], {2}) == [2]
    assert D.cut_at_eos([4, 5, 6], set()) == [4, 5, 6] and D.cut_at_eos([], {2}) == []          # an empty EOS set cuts nothing
    words = {2: "</s>", 4: " yes", 5: "it", 6: "is ", 0: "<pad>"}
    decode = lambda ids: "".join(words[t] for t in ids)
    assert D.answer_text(decode, [4, 5, 2, 0, 0], D.eos_set(2)) == "yesit</s>"
    assert D.answer_text(decode, [4, 5, 2, 0, 0], D.eos_set(2), stop_str="</s>") == "yesit"
    assert D.answer_text(decode, [4, 6, 2, 0], {2}, stop_str="</s>") == "yesis"                   # stripped again behind the stop string
    assert D.answer_text(decode, [4, 0], set(), stop_str="</s>") == "yes<pad>" and D.answer_text(decode, [], {2}) == ""


def test_sharded_run_partitions_whole_images_and_offsets_the_seed():
    qs = [{"question_id": i, "image": f"im{(i * 7) % 5}.jpg", "text": f"q{i}"} for i in range(23)]       # 5 images, interleaved
    for world in (1, 2, 3, 4):
        runs = [D.ShardedRun(qs, r, world, {"seed": 10, "temperature": 0.5}, None) for r in range(world)]
        assert sorted(i for run in runs for i in run.mine) == list(range(23))                            # a partition
        owners = {}
        for run in runs:
            assert (run.rank, run.world, run.plan.world) == (runs.index(run), world, world)
            assert run.generate_kw == {"seed": 10 + run.rank, "temperature": 0.5} and run.invariant is False
            for i in run.mine:
                assert owners.setdefault(qs[i]["image"], run.rank) == run.rank                           # whole images stay on one rank
            assert [qs[i]["image"] for i in run.mine] == sorted(qs[i]["image"] for i in run.mine)        # one image's questions adjacent
            got = list(run.batches(4))
            assert [i for idx, _ in got for i in idx] == run.mine and all(len(idx) <= 4 and sub == [qs[i] for i in idx] for idx, sub in got)
    kw = {"cd_greedy": True}
    run = D.ShardedRun(qs, 1, 2, kw, None)
    assert run.generate_kw is kw and run.invariant is True and D.ShardedRun(qs, 1, 2, kw, False).invariant is False     # no seed: nothing to offset
    assert isinstance(run.mode(), type(D.ops.batch_invariant())) and D.ShardedRun([], 0, 1, {}, None).mine == []


def test_load_distinct_images_hands_back_one_tensor_object_per_name():
    loads = []
    load = lambda name: loads.append(name) or torch.zeros(3, 2, 2)
    imgs = D.load_distinct_images(["a", "b", "a", "a", "b"], load, "cpu")
    assert loads == ["a", "b"] and imgs[0] is imgs[2] is imgs[3] and imgs[1] is imgs[4] and imgs[0] is not imgs[1]
    assert D.load_distinct_images(["a"], load, "cpu")[0] is not imgs[0] and loads == ["a", "b", "a"]       # nothing is kept between calls
    assert D.load_distinct_images([], load, "cpu") == []


def test_write_jsonl_round_trip_creates_the_parent_directory(tmp_path):
    recs = [{"question_id": 3, "text": "yes", "naive": {"yes": 0.75, "no": 0.25}, "metadata": {}}, {"question_id": "a/b.png", "text": "é\n"}]
    path = tmp_path / "new" / "dir" / "answers.jsonl"
    D.write_jsonl(str(path), recs)
    lines = path.read_text().splitlines()
    assert lines == [json.dumps(r) for r in recs] and [json.loads(l) for l in lines] == recs
    assert list(json.loads(lines[0])) == ["question_id", "text", "naive", "metadata"]                   # key order as given
    D.write_jsonl(str(path), recs[:1])
    assert path.read_text() == json.dumps(recs[0]) + "\n"


def test_pope_scores_for_degenerate_lists_give_none_not_an_exception():
    from llava_align_amd import calibrate as C
    qs = [{"question_id": i, "label": ("yes", "no")[i % 2]} for i in range(4)]
    no = [{"question_id": i, "text": "no", "naive": {"yes": 0.25, "no": 0.75}, "none": {"yes": 0.5, "no": 0.5}} for i in range(4)]
    with pytest.raises(ZeroDivisionError):                      # no positive: precision divides by zero
        C.pope_scores(qs, no)
    with pytest.raises(ZeroDivisionError):
        C.pope_scores_calibrated(qs, no, "naive")
    assert D.pope_scores_for(qs, no, ("string_match", "naive")) == {"string_match": None, "naive": None}
    yes = [dict(a, text="yes", naive={"yes": 0.75, "no": 0.25}) for a in no]
    got = D.pope_scores_for(qs, yes, ("string_match", "naive", "none"))
    assert list(got) == ["string_match", "naive", "none"]
    assert got["string_match"] == C.pope_scores(qs, yes) and got["naive"] == C.pope_scores_calibrated(qs, yes, "naive")
    assert got["none"] == C.pope_scores_calibrated(qs, yes, "none") and isinstance(got["naive"], dict)
    assert D.pope_scores_for(qs[:3] + [{"question_id": 3}], yes, ("string_match",)) == {}               # a question without its label: nothing is scored
    assert D.pope_scores_for(qs, yes, ()) == {}


def test_result_rows_gather_on_one_rank_with_tops_and_answers_only():
    plan = D.ShardedRun([{"image": "x"}] * 5, 0, 1, {}, None).plan
    rows = D.ResultRows("cpu", width=4, pad=9, n_sets=2)
    top = lambda n, base: (torch.arange(n * 10).view(n, 10) + base, (torch.arange(n * 10.0).view(n, 10) + base) / 1024)
    a, b, c, d = top(3, 0), top(3, 100), top(2, 200), top(2, 300)
    rows.add([4, 0, 2], torch.tensor([[1, 2, 3], [4, 5, 6], [7, 8, 2]]), [a, b])
    rows.add([1, 3], torch.tensor([[11, 12, 13, 14], [15, 16, 17, 18]]), [c, d])
    got = rows.gather(plan, 5)
    assert got["tokens"] == [[4, 5, 6], [11, 12, 13, 14], [7, 8, 2], [15, 16, 17, 18], [1, 2, 3]]     # by question index, valid columns only
    assert len(got["tops"]) == 2 and got["tops"][0][4] == (a[0][0].tolist(), a[1][0].tolist()) and got["tops"][1][0] == (b[0][1].tolist(), b[1][1].tolist())
    assert got["tops"][0][3] == (c[0][1].tolist(), c[1][1].tolist()) and got["tops"][1][1] == (d[0][0].tolist(), d[1][0].tolist())
    with pytest.raises(AssertionError):
        rows.add([0], torch.zeros(1, 2, dtype=torch.long), [a])                                        # one top list per set
    only = D.ResultRows("cpu", width=3, pad=0, n_sets=0)
    only.add([2, 0], torch.tensor([[5, 6], [7, 8]]))
    only.add([1], torch.tensor([[1, 2, 3]]), [])
    assert only.gather(plan, 3) == {"tokens": [[7, 8], [1, 2, 3], [5, 6]], "tops": []}
    short = D.ResultRows("cpu", width=3, pad=0, n_sets=0)
    short.add([0, 0], torch.tensor([[1], [2]]))
    with pytest.raises(RuntimeError, match="not delivered exactly once"):
        short.gather(plan, 2)
    assert D.ResultRows("cpu", 3, 0, n_sets=1).gather(plan, 0) == {"tokens": [], "tops": [[]]}


def test_sweep_helpers():
    kw = {"temperature": 0.2, "top_k": 5, "use_dd": True, "seed": 3, "cd_beta": 0.1, "cd_greedy": True}
    assert D.plain_kw(kw) == {"temperature": 0.2, "top_k": 5, "seed": 3, "cd_beta": 0.1} and set(D.plain_kw(kw)) <= set(D.PRIOR_KW)
    assert D.sweep_settings(None) == [{"tag": None}]
    sweep = [{"tag": "a", "temperature": 1.0, "top_p": None, "answers_path": "x"}, {"tag": "b", "top_k": 2}]
    settings = D.sweep_settings(sweep)
    assert settings == sweep and settings[0] is not sweep[0]
    assert D.setting_kw(kw, settings[0]) == dict(kw, temperature=1.0, top_p=None) and D.setting_kw(kw, settings[1]) == dict(kw, top_k=2)
    assert D.setting_kw(kw, {"tag": None}) == kw
    assert D.sweep_result(None, D.sweep_settings(None), lambda j, s: (j, s["tag"]), batch_invariant=True) == (0, None)
    assert D.sweep_result(sweep, settings, lambda j, s: (j, s["tag"]), batch_invariant=True) == {"runs": {"a": (0, "a"), "b": (1, "b")}, "batch_invariant": True}


COMMON = {"top_k": None, "cd_alpha": 1.0, "cd_beta": 0.1}
DEFAULTS = {       # the per-driver defaults follow each driver's reference script and differ on purpose
    "pope": dict(COMMON, seed=None, temperature=1.0, top_p=None, noise_step=None, dtype="float16", batch=384, max_new_tokens=64, use_dd=False,
                 use_dd_unk=False, cd_greedy=False, image_priors=[], preset="llava-1.5-7b", vision_tower=None),
    "mme": dict(COMMON, seed=None, temperature=None, top_p=None, noise_step=500, dtype="float16", batch=256, max_new_tokens=None, use_cd=False, use_dd=False,
                use_dd_unk=False, arch="llava", conv_mode="vicuna_v1", num_chunks=1, chunk_idx=0, num_beams=1, no_sweep=False, gt_root=None,
                model_base=None, preset="llava-1.5-7b", vision_tower=None, native_visual=False),
    "qwen": dict(COMMON, seed=42, temperature=None, top_p=None, noise_step=500, dtype="bfloat16", batch=128, use_cd=False, use_dd=False, use_dd_unk=False,
                 model_path="Qwen/Qwen-VL-Chat", model_base=None, image_folder="", conv_mode="llava_v1", num_chunks=1, chunk_idx=0, sampling=False,
                 no_sweep=False, native_visual=False),
    "blip": dict(COMMON, seed=42, temperature=1.0, top_p=1.0, noise_step=500, dtype="float16", batch=128, use_cd=False, model_base=None, image_folder="",
                 conv_mode="llava_v1", num_chunks=1, chunk_idx=0, max_txt_len=128),
    "sampling": dict(COMMON, seed=42, temperature=1.0, top_p=None, noise_step=500, dtype="float16", in_flight=90, max_new_tokens=1024, use_cd=False,
                     use_dd=False, use_dd_unk=False, model_base=None, image_folder="", conv_mode="llava_v1", num_chunks=1, chunk_idx=0, no_sweep=False,
                     naive=False, preset="llava-1.5-7b", vision_tower=None),
}
REQUIRED = {"pope": ["--model-path", "m", "--question-file", "q", "--image-folder", "i", "--answers-file", "a"],
            "mme": ["--model-path", "m", "--question-file", "q", "--image-folder", "i", "--answers-file", "a"],
            "qwen": ["--question-file", "q", "--answers-file", "a"],
            "blip": ["--blip-checkpoint", "b", "--llm-path", "l", "--bert-tokenizer", "t", "--question-file", "q", "--answers-file", "a"],
            "sampling": ["--model-path", "m", "--question-file", "q", "--answers-file", "a"]}


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_each_driver_command_line_keeps_its_defaults(name):
    import importlib
    parser = importlib.import_module(f"llava_align_amd.{name}_driver")._parser()
    a = vars(parser.parse_args(REQUIRED[name]))
    given = {k[2:].replace("-", "_") for k in REQUIRED[name][::2]}
    assert {k: v for k, v in a.items() if k not in given} == DEFAULTS[name]
    for k in REQUIRED[name][::2]:                                # what is required stays required
        argv = [x for i, x in enumerate(REQUIRED[name]) if REQUIRED[name][i - i % 2] != k]
        if k == "--model-path" and name == "qwen":
            continue
        with pytest.raises(SystemExit):
            parser.parse_args(argv)
    b = parser.parse_args(REQUIRED[name] + ["--seed", "7", "--temperature", "0.5", "--top_p", "0.9", "--top_k", "3", "--noise_step", "11", "--dtype", "bfloat16"])
    assert (b.seed, b.temperature, b.top_p, b.top_k, b.noise_step, b.dtype) == (7, 0.5, 0.9, 3, 11, "bfloat16")
