"""tests/poison.py on the host: which allocator calls are filled, what the census counts, that the allocators come back, and that every
allocating function of the package is accounted for by a poisoned test."""
import os
import sys
import types

import pytest
import torch

import poison
from poison import poisoned_alloc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN = "poison_standin_pkg"

STANDIN_SOURCE = '''
import torch

def floats(n, dtype=torch.float32):
    return torch.empty(n, dtype=dtype)

def ints(n):
    return torch.empty(n, dtype=torch.int32)

def like(t):
    return torch.empty_like(t)

def strided(n):
    return torch.empty_strided((n, 2), (2, 1), dtype=torch.float16)

def new(t, n):
    return t.new_empty(n)

make = lambda n: torch.empty(n, dtype=torch.bfloat16)
'''


@pytest.fixture()
def standin():
    """a stand-in "package" module: its allocator calls count as the package's when STANDIN is listed in `packages`"""
    mod = types.ModuleType(STANDIN + ".kernels")
    exec(compile(STANDIN_SOURCE, STANDIN + "/kernels.py", "exec"), mod.__dict__)
    return mod


def _cpu(pattern):
    return poisoned_alloc(pattern, device_types=("cpu",), packages=(STANDIN,))


def test_only_floating_allocations_of_the_package_are_filled(standin):
    with _cpu("nan") as census:
        f = standin.floats(33)
        assert bool(torch.isnan(f).all())
        assert bool(torch.isnan(standin.like(torch.zeros(5, 3, dtype=torch.bfloat16)).float()).all())
        assert bool(torch.isnan(standin.strided(7).float()).all())
        assert bool(torch.isnan(standin.new(torch.zeros(2, dtype=torch.float64), 9)).all())
        assert bool(torch.isnan(standin.make(4).float()).all())                      # a lambda is a call site like any other
        own = torch.empty(4096, dtype=torch.float32).fill_(1.0)                       # called from this module: returned as allocated
        assert bool((own == 1.0).all())
        i = standin.ints(4096)                                                        # NaN has no integer form: a fill would raise
        assert i.dtype == torch.int32
    assert census.calls == 6 and census.filled == 5
    with poisoned_alloc("nan", packages=(STANDIN,)) as census:                       # default devices: host tensors are left alone
        f = standin.floats(1024)
        f.fill_(2.0)
        assert bool((f == 2.0).all())
    assert census.calls == 1 and census.filled == 0 and census.bytes == 0 and census.sites == {}


def test_integer_tensors_are_returned_as_allocated(standin):
    """the wrapper never writes to an integer tensor: the allocator's own result object comes back, with no fill recorded"""
    with _cpu("big") as census:
        t = standin.ints(4096)
    assert not bool((t == 30000).all())
    assert t.dtype == torch.int32 and census.calls == 1 and census.filled == 0 and census.bytes == 0


def test_census_counts_calls_bytes_and_sites(standin):
    with _cpu("zero") as census:
        for n in (10, 20):
            standin.floats(n)                                     # one site, two calls: 40 + 80 bytes
        standin.floats(3, torch.float64)                          # the same site: 24 bytes
        standin.like(torch.ones(5, 3, dtype=torch.bfloat16))      # 30 bytes
        standin.ints(100)                                         # counted as a call, not filled
        standin.make(8)                                           # 16 bytes, site "<lambda>"
    assert census.calls == 6 and census.filled == 5 and census.bytes == 40 + 80 + 24 + 30 + 16
    assert sum(census.sites.values()) == census.bytes and len(census.sites) == 3
    by_fn = {s.split(":")[1]: b for s, b in census.sites.items()}
    assert by_fn == {"floats": 144, "like": 30, "<lambda>": 16}
    for site in census.sites:
        mod, fn, line = site.split(":")
        assert mod == STANDIN + ".kernels" and int(line) > 0
    first = min(int(s.rsplit(":", 1)[1]) for s in census.sites)
    assert census.bytes_in(STANDIN + ".kernels", first, first) == 144 and census.bytes_in("elsewhere", 0, 10 ** 6) == 0
    assert "floats" in census.table() and census.table().splitlines()[0].strip().startswith("144")


def test_allocators_are_restored_after_exit_and_after_an_exception(standin):
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)
    now = lambda: (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)
    with _cpu("nan"):
        assert torch.empty is not before[0] and torch.Tensor.new_empty is not before[3]
    assert now() == before
    with pytest.raises(KeyError, match="boom"):
        with _cpu("nan"):
            standin.floats(4)
            raise KeyError("boom")
    assert now() == before
    with _cpu("zero") as census:                                  # and the helper can be entered again
        assert bool((standin.floats(6) == 0).all())
    assert census.filled == 1 and now() == before


def test_nesting_raises_and_leaves_the_outer_block_working(standin):
    with _cpu("nan") as outer:
        with pytest.raises(RuntimeError, match="nest"):
            with _cpu("big"):
                pass
        assert bool(torch.isnan(standin.floats(3)).all())
    assert outer.filled == 1 and not hasattr(torch.empty, "__wrapped__")
    with pytest.raises(ValueError, match="pattern"):
        with _cpu("ones"):
            pass
    assert not hasattr(torch.empty, "__wrapped__")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_patterns_round_trip_in_the_storage_types(standin, dtype):
    want = {"zero": 0.0, "nan": float("nan"), "big": 3.0e4}
    assert sorted(poison.PATTERNS) == sorted(want) and poison.PATTERNS["zero"] == 0.0 and poison.PATTERNS["big"] == 3.0e4 and poison.PATTERNS["nan"] != poison.PATTERNS["nan"]
    for pattern, value in want.items():
        with _cpu(pattern):
            t = standin.floats(257, dtype)
        assert t.dtype == dtype and poison.holds_pattern(t, pattern)
        stored = torch.tensor(value).to(dtype)
        if pattern == "nan":
            assert bool(torch.isnan(t).all())
        else:
            assert torch.equal(t, stored.expand(257)) and bool(torch.isfinite(t).all())
    # +3.0e4 stays finite and large in every storage type (fp16's largest finite value is 65504), to within the type's rounding
    assert abs(float(torch.tensor(3.0e4).to(dtype)) - 3.0e4) <= 3.0e4 * 2.0 ** -8


def test_the_docstring_says_why_there_are_three_patterns():
    doc = poison.__doc__
    for word in ('"zero"', '"nan"', '"big"', "fmaxf", "RUNNING MAXIMUM", "baseline", "ARITHMETIC"):
        assert word in doc, word


# ------------------------------------------------------------------ completeness
# allocating functions that no poisoned test runs, each with its reason
EXCEPTIONS = {
    "engine:h2d_int32": "int32 pinned host staging buffer: integer tensors are never poisoned, and torch.cat writes all of it",
    "engine:VddLlavaEngine._stage_host_images": "pinned HOST staging buffer (host tensors are not poisoned); torch.stack writes the rows that are uploaded",
    "ops:stop_words_match": "int32 flag output: integer tensors are never poisoned",
    "vcd_sample:sample": "int64 token-id buffer: integer tensors are never poisoned",
    "shard:gather_results": "int64 all_gather buffer of the multi-GPU drivers: integer, and multi-GPU sharding is not covered",
}


def test_every_allocating_function_of_the_package_is_covered_or_excepted():
    """Walks the source of every module of the package for calls of the four allocators.  A new torch.empty in ops.py fails here until
    someone gives it a thunk in tests/test_poisoned_ops_gpu.py::CASES (wrappers), lists it in ENGINE_COVERED (engine.py, run by
    tests/test_poisoned_engine_gpu.py) or writes down in EXCEPTIONS why it needs neither."""
    import test_poisoned_ops_gpu as P
    found = poison.allocating_functions(os.path.join(ROOT, "llava-align_amd"))
    assert len(found) >= 40 and "ops:gemm" in found and "engine:KVCache.__init__" in found           # the walk really sees the package
    covered = set(P.CASES) | set(P.ENGINE_COVERED)
    assert not covered & set(EXCEPTIONS), sorted(covered & set(EXCEPTIONS))
    missing = sorted(set(found) - covered - set(EXCEPTIONS))
    assert not missing, f"allocating functions no poisoned test runs: {[(m, found[m]) for m in missing]}"
    stale = sorted((covered | set(EXCEPTIONS)) - set(found))
    assert not stale, f"listed, but no longer allocating (or renamed): {stale}"
    # the wrapper level is the wrapper level: every allocating function outside engine.py / shard.py has a thunk or an exception
    for name in found:
        if name.split(":")[0] in ("ops", "sampling", "qwen_visual", "vcd_sample", "vcd_add_noise"):
            assert name in P.CASES or name in EXCEPTIONS, name
    assert all(name.startswith("engine:") for name in P.ENGINE_COVERED)
    assert all(len(reason) > 20 for reason in EXCEPTIONS.values())


def test_the_walk_finds_lambdas_methods_and_new_empty(tmp_path):
    (tmp_path / "m.py").write_text(
        "import torch\nimport numpy as np\n"
        "buf = torch.empty(3)\n"
        "def plain(x):\n    return torch.empty_like(x)\n"
        "def host():\n    return np.empty(3)\n"
        "class K:\n    def __init__(self):\n        mk = lambda n: torch.empty(n)\n        self.a = mk(2)\n"
        "    def grow(self, t):\n        def inner():\n            return t.new_empty(4)\n        return inner()\n"
        "def strided():\n    return torch.empty_strided((2, 2), (2, 1))\n")
    found = poison.allocating_functions(str(tmp_path))
    assert found == {"m:<module>": [3], "m:plain": [5], "m:K.__init__": [10], "m:K.grow": [14], "m:strided": [17]}


def test_scrub_fills_pools_once_and_leaves_tables_and_weights_alone():
    """scrub on a stand-in engine (host tensors): shared pools are filled once, None entries and integer tables are skipped, the image
    cache is dropped"""
    k1 = torch.ones(2, 3)
    kv = types.SimpleNamespace(kp=[k1, k1], vp=[torch.ones(2, 3)] * 2, pfrag=[None, None], ko=[torch.ones(4), torch.ones(4)], vo=[torch.ones(4, dtype=torch.float16)] * 2,
                               pk=None, pv=None, page_table=torch.full((2, 2), -1, dtype=torch.int32))
    paged = types.SimpleNamespace(kp=[torch.ones(1)], vp=[torch.ones(1)], pfrag=[torch.ones(2)], ko=[torch.ones(1)], vo=[torch.ones(1)],
                                  pk=[torch.ones(5, dtype=torch.bfloat16)], pv=[torch.ones(5, dtype=torch.bfloat16)], page_table=torch.zeros(1, 1, dtype=torch.int32))
    cleared = []
    weights = torch.ones(7)
    eng = types.SimpleNamespace(_kvs={False: kv, "paged": paged}, vit=types.SimpleNamespace(_kv=(torch.ones(3), torch.ones(3))), w=weights,
                                clear_image_cache=lambda: cleared.append(True))
    n = poison.scrub(eng, "big")
    assert n == (6 + 6 + 4 + 4 + 4) * 4 - 4 * 2 + (1 + 1 + 2 + 1 + 1) * 4 + 2 * 5 * 2 + 2 * 3 * 4
    assert cleared == [True] and bool((weights == 1).all()) and bool((kv.page_table == -1).all()) and bool((paged.page_table == 0).all())
    for t in (k1, kv.vp[0], kv.ko[1], kv.vo[0], paged.pfrag[0], paged.pk[0], eng.vit._kv[1]):
        assert poison.holds_pattern(t, "big")
    eng.vit._kv = None                                            # a tower that has not run yet
    assert poison.scrub(eng, "nan") == n - 2 * 3 * 4 and bool(torch.isnan(k1).all())
