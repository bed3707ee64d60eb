"""Poisoned buffers: no answer may depend on bytes nobody wrote.

Every pool, workspace, activation matrix and output of the package comes from `torch.empty` (or `empty_like` / `empty_strided` /
`Tensor.new_empty`).  Fresh memory usually holds zeros and a second identical call finds the correct values of the first one, so a
read past a length, of a padded row or of a chunk tail that nobody wrote goes unnoticed.  Two tools make such a read visible:

`poisoned_alloc(pattern)`  a context manager: while it is active every floating-point result of the four allocators, when the call is
    made FROM ONE OF THE PACKAGE'S OWN PYTHON MODULES (decided by the caller's module name: torch's own Python code and the tests are
    left alone), is filled with the pattern before it is returned.  Integer tensors are returned as allocated, on purpose: the question
    is whether a VALUE leaks into an answer, not what a kernel does with a wild index.  Host (pinned or pageable) tensors are untouched
    unless "cpu" is listed in `device_types`.  An allocation made during graph capture is filled too: the fill is captured, so every
    replay poisons that temporary again, which asks more, not less.  No captured buffer of the package carries state between replays
    through an allocator call made inside the capture (state lives in buffers allocated before it), so no site is excluded.
`scrub(engine, pattern)`   fills, in place, every persistent floating buffer an engine keeps between calls (the KV pools of every cache,
    the vision tower's K/V pair) and drops the image features: addresses do not change, captured graphs stay valid - the replay path
    over stale memory.

Why three patterns:
  "zero"  0.0: what fresh memory usually holds - the baseline the other two are compared with;
  "nan"   a quiet NaN: shows in anything that does ARITHMETIC on the bytes (a sum, a product with a zero weight included);
  "big"   +3.0e4 (finite in fp16): fmaxf(m, NaN) == m, so a masked key that still takes part in a RUNNING MAXIMUM hides from a NaN -
          yet it changes the rescale and with it the roundings of a P that is rounded to the storage type.  A large finite value does
          not hide: it becomes the maximum.
A run is right when its results are bit-equal under all three.

Plain Python; imports without a GPU."""
import contextlib
import sys

import torch

PACKAGE = "llava_align_amd"
PATTERNS = {"zero": 0.0, "nan": float("nan"), "big": 3.0e4}
FLOAT_DTYPES = (torch.bfloat16, torch.float16, torch.float32, torch.float64)
ALLOCATORS = ("empty", "empty_like", "empty_strided", "new_empty")

_active = None


def pattern_value(pattern: str) -> float:
    if pattern not in PATTERNS:
        raise ValueError(f"pattern {pattern!r}: one of {sorted(PATTERNS)}")
    return PATTERNS[pattern]


def holds_pattern(t: torch.Tensor, pattern: str) -> bool:
    """Every element of `t` is the pattern as `t`'s dtype stores it (3.0e4 is 29952 in bf16)."""
    if pattern == "nan":
        return bool(torch.isnan(t).all())
    return bool((t == torch.tensor(pattern_value(pattern), dtype=t.dtype, device=t.device)).all())


class Census:
    """What one `poisoned_alloc` block poisoned: `calls` allocator calls from the package, `filled` of them filled (floating, on a listed
    device), `bytes` bytes filled, `sites` = {"module:function:line": bytes filled there}."""

    def __init__(self, pattern):
        self.pattern, self.calls, self.filled, self.bytes, self.sites = pattern, 0, 0, 0, {}

    def table(self) -> str:
        return "\n".join(f"{b:>14,d}  {s}" for s, b in sorted(self.sites.items(), key=lambda kv: (-kv[1], kv[0])))

    def bytes_in(self, module: str, first_line: int, last_line: int) -> int:
        """bytes poisoned by the call sites of `module` in the lines first_line .. last_line (a function's extent: lambdas report their
        own name, so a site is located by its line)"""
        total = 0
        for site, b in self.sites.items():
            mod, _fn, line = site.rsplit(":", 2)
            if mod == module and first_line <= int(line) <= last_line:
                total += b
        return total


def _from_package(name, packages) -> bool:
    return any(name == p or name.startswith(p + ".") for p in packages)


@contextlib.contextmanager
def poisoned_alloc(pattern, device_types=("cuda",), packages=(PACKAGE,)):
    """See the module docstring.  Yields the Census.  Does not nest; the allocators are restored on exception."""
    global _active
    value = pattern_value(pattern)
    if _active is not None:
        raise RuntimeError("poisoned_alloc does not nest")
    census = Census(pattern)
    device_types, packages = tuple(device_types), tuple(packages)

    def wrap(orig):
        def alloc(*args, **kwargs):
            t = orig(*args, **kwargs)
            f = sys._getframe(1)
            mod = f.f_globals.get("__name__", "")
            if _from_package(mod, packages):
                census.calls += 1
                if t.dtype in FLOAT_DTYPES and t.device.type in device_types:
                    t.fill_(value)
                    n = t.numel() * t.element_size()
                    site = f"{mod}:{f.f_code.co_name}:{f.f_lineno}"
                    census.filled += 1
                    census.bytes += n
                    census.sites[site] = census.sites.get(site, 0) + n
            return t
        alloc.__wrapped__ = orig
        return alloc

    saved = {n: getattr(torch, n) for n in ALLOCATORS[:3]}
    own_new_empty = torch.Tensor.__dict__.get("new_empty")           # normally None: the method lives on the C base class
    _active = census
    try:
        for n, orig in saved.items():
            setattr(torch, n, wrap(orig))
        torch.Tensor.new_empty = wrap(torch.Tensor.new_empty)
        yield census
    finally:
        for n, orig in saved.items():
            setattr(torch, n, orig)
        if own_new_empty is None:
            del torch.Tensor.new_empty
        else:
            torch.Tensor.new_empty = own_new_empty
        _active = None


def engine_buffers(engine):
    """Every persistent floating buffer reachable from the engine, each once: all pools of every KVCache in `engine._kvs` and the vision
    tower's K/V pair.  Not the weights, the page table or any integer table, and not ops._gemm_ws / ops._fused_split_ws (arrival counters
    with a documented must-be-zero contract)."""
    seen, out = set(), []

    def take(t):
        if t is not None and t.dtype in FLOAT_DTYPES and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            out.append(t)
    for kv in engine._kvs.values():
        for pool in (kv.kp, kv.vp, kv.pfrag, kv.ko, kv.vo, kv.pk or [], kv.pv or []):
            for t in pool:
                take(t)
    for t in (getattr(engine.vit, "_kv", None) or ()):
        take(t)
    return out


def scrub(engine, pattern) -> int:
    """Fill in place every buffer of `engine_buffers` and forget the image features.  Returns the bytes filled."""
    value = pattern_value(pattern)
    total = 0
    for t in engine_buffers(engine):
        t.fill_(value)
        total += t.numel() * t.element_size()
    engine.clear_image_cache()
    return total


def allocating_functions(package_dir):
    """{"module:Class.function": [line, ...]} of every function in the package's Python sources that calls torch.empty / torch.empty_like /
    torch.empty_strided or <tensor>.new_empty (found in the syntax tree; a lambda or a nested function counts for the function around
    it, code at module level for "<module>")."""
    import ast
    import os
    found = {}

    class Walk(ast.NodeVisitor):
        def __init__(self, module):
            self.module, self.stack = module, []

        def _scope(self, node):
            outer = bool(self.stack) and self.stack[-1][1]
            self.stack.append((node.name, isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) or outer))
            self.generic_visit(node)
            self.stack.pop()
        visit_ClassDef = visit_FunctionDef = visit_AsyncFunctionDef = _scope

        def visit_Call(self, node):
            f = node.func
            if isinstance(f, ast.Attribute) and (f.attr == "new_empty" or (f.attr in ALLOCATORS[:3] and isinstance(f.value, ast.Name) and f.value.id == "torch")):
                names = []
                for name, in_function in self.stack:            # the outermost function and the classes around it
                    names.append(name)
                    if in_function:
                        break
                found.setdefault(f"{self.module}:{'.'.join(names) or '<module>'}", []).append(node.lineno)
            self.generic_visit(node)

    for fn in sorted(os.listdir(package_dir)):
        if fn.endswith(".py"):
            with open(os.path.join(package_dir, fn)) as f:
                Walk(fn[:-3]).visit(ast.parse(f.read(), fn))
    return found
