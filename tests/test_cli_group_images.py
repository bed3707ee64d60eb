"""`python -m llava_align_amd.sampling_driver --group-images`: the list call with the questions about one image grouped, from a generated
checkpoint directory."""
import json
import subprocess
import sys

import pytest

from test_cli import ROOT, _env
from tiny_checkpoint import write_checkpoint


@pytest.mark.gpu
def test_sampling_driver_group_images(tmp_path):
    info = write_checkpoint(str(tmp_path))
    out = str(tmp_path / "out" / "grouped-setting.jsonl")
    p = subprocess.run([sys.executable, "-m", "llava_align_amd.sampling_driver", "--model-path", info["ckpt"], "--question-file", info["questions"],
                        "--image-folder", info["images"], "--use_dd_unk", "--cd_alpha", "1", "--cd_beta", "0.1", "--max_new_tokens", "12", "--in-flight", "4",
                        "--no-sweep", "--group-images", "--answers-file", out], capture_output=True, text=True, env=_env(), timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    assert rep["run"] == "default" and rep["n_answers"] == info["n_questions"] and rep["answers_file"].endswith("grouped-default.jsonl")
    assert rep["stats"]["group_images"] is True and rep["stats"]["in_flight"] == 4
    a = [json.loads(l) for l in open(rep["answers_file"])]
    assert [x["question_id"] for x in a] == list(range(100, 100 + info["n_questions"]))


def test_parsers_take_the_flag():
    from llava_align_amd import qwen_driver, sampling_driver
    a = sampling_driver._parser().parse_args(["--model-path", "m", "--question-file", "q", "--answers-file", "a", "--group-images"])
    assert a.group_images is True
    assert not hasattr(sampling_driver._parser().parse_args(["--model-path", "m", "--question-file", "q", "--answers-file", "a"]), "group_images")
    assert any("--group-images" in s for act in qwen_driver._parser()._actions for s in act.option_strings)
