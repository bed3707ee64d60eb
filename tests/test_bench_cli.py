"""bench.py's command line and --dump-outputs on the host: a plain run is the default, --steps is validated, the dump is float32 /
float64 and a payload over the size cap becomes a fixed seeded sample of whole question rows."""
import numpy as np
import pytest
import torch

import bench


def _payload(n, width=64, k=10):
    g = torch.Generator().manual_seed(0)
    return {"tokens": torch.randint(0, 32000, (n, width), generator=g), "n_tokens": torch.full((n,), width),
            "top_tok": torch.randint(0, 32000, (n, k), generator=g), "top_prob": torch.rand(n, k, generator=g),
            "count": torch.ones(n, dtype=torch.long)}


def test_plain_run_is_the_default():
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None and a.choices_out is None
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full and b.dump_outputs == "out"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bad_step_counts_are_refused(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_dump_writes_every_row_as_float(tmp_path):
    res = _payload(12)
    names = bench.dump_outputs(str(tmp_path), res)
    assert names == ["n_tokens", "tokens", "top_prob", "top_tok"]
    for name in names:
        x = np.load(tmp_path / f"{name}.npy")
        assert x.dtype == (np.float32 if name == "top_prob" else np.float64)
        assert np.array_equal(x, res[name].numpy().astype(x.dtype))
    assert not (tmp_path / "count.npy").exists() and not (tmp_path / "rows.npy").exists()


def test_dump_over_the_cap_is_a_fixed_sample_of_rows(tmp_path):
    res = _payload(1000)
    cap = 100_000
    names = bench.dump_outputs(str(tmp_path / "a"), res, max_bytes=cap)
    bench.dump_outputs(str(tmp_path / "b"), res, max_bytes=cap)
    assert "rows" in names
    assert sum((tmp_path / "a" / f"{n}.npy").stat().st_size for n in names) <= cap + 128 * len(names)
    rows = np.load(tmp_path / "a" / "rows.npy").astype(np.int64)
    assert 0 < len(rows) < 1000 and np.all(np.diff(rows) > 0)
    for name in names:
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(x, y)
        if name != "rows":
            assert np.array_equal(x, res[name].numpy()[rows].astype(x.dtype))
