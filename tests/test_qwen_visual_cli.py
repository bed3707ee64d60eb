"""--native-visual parses and reaches checkpoint.load_qwen for both command lines (qwen_driver; mme_driver --arch qwen); without the
flag the model's own tower stays the default.  Host logic only: load_qwen is replaced by a recorder that stops the run."""
import json

import pytest
import torch


class Stop(Exception):
    pass


@pytest.fixture
def recorder(monkeypatch):
    from llava_align_amd import checkpoint as K
    from llava_align_amd import shard
    seen = []

    def load_qwen(path, device, dtype=torch.bfloat16, use_graph=True, native_visual=False):
        seen.append(native_visual)
        raise Stop
    monkeypatch.setattr(K, "load_qwen", load_qwen)
    monkeypatch.setattr(shard, "init_from_env", lambda *a, **k: (0, 1, torch.device("cpu")))
    return seen


@pytest.mark.parametrize("flag", [False, True])
def test_qwen_driver_native_visual(recorder, tmp_path, flag):
    from llava_align_amd import qwen_driver
    q = tmp_path / "q.jsonl"
    q.write_text(json.dumps({"question_id": 0, "image": "a.jpg", "text": "x"}) + "\n")
    argv = ["--question-file", str(q), "--answers-file", str(tmp_path / "a.jsonl")] + (["--native-visual"] if flag else [])
    with pytest.raises(Stop):
        qwen_driver.main(argv)
    assert recorder == [flag]


@pytest.mark.parametrize("flag", [False, True])
def test_mme_driver_native_visual(recorder, tmp_path, flag):
    from llava_align_amd import mme_driver
    q = tmp_path / "q.jsonl"
    q.write_text(json.dumps({"question_id": "artwork/a.jpg", "image": "a.jpg", "text": "x", "category": "artwork"}) + "\n")
    argv = ["--arch", "qwen", "--model-path", "m", "--image-folder", str(tmp_path), "--question-file", str(q),
            "--answers-file", str(tmp_path / "a.jsonl")] + (["--native-visual"] if flag else [])
    with pytest.raises(Stop):
        mme_driver.main(argv)
    assert recorder == [flag]


def test_embed_prompt_without_tower_has_no_batch_hook():
    """The default front-end is unchanged: no encode_batch, so the drivers call it exactly as before."""
    from types import SimpleNamespace
    from llava_align_amd.checkpoint import qwen_embed_prompt
    model = SimpleNamespace(config=SimpleNamespace(visual={"image_start_id": 100}))
    assert not hasattr(qwen_embed_prompt(model, lambda t: [1], "cpu"), "encode_batch")
