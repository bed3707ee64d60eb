"""Dispatch trace of the projection wrappers of ops.py, on the CPU: which C entries a call reaches, with which integer arguments (the
GEMM config included), what it adds to the tuning tables, how it counts in w8_launches() and what it raises - for every wrapper, in the
three guises of a weight (16-bit tensor, 16-bit tensor + w8=(codes, scale), CodesWeight), over row counts on either side of every
threshold and under every switch, forced form and table entry that the dispatch reads.

The library is a recorder (no kernel runs), so the whole host path is walked down to the C call.  Some 40,000 outcomes are far too many
to spell out, so the table below holds, per wrapper variant and guise, the number of cases and the SHA-1 of their outcomes in order
(EXPECTED), and a few of them in words (READABLE).  Both were RECORDED from ops.py as it stood before its dispatch was folded into one
weight source, one launch helper, one form picker and one tuned-config lookup, and a refactor of that code leaves them alone: a changed
digest is a changed behaviour.  To see WHICH outcomes differ between the package's ops.py and another revision of the file:

    git show <rev>:llava-align_amd/ops.py > ops_rev.py && python tests/test_ops_dispatch_trace.py --diff ops_rev.py

and to replay the whole test against that revision: OPS_TRACE_FILE=ops_rev.py pytest tests/test_ops_dispatch_trace.py
(`python tests/test_ops_dispatch_trace.py --record` prints both tables for whatever OPS_TRACE_FILE / the package holds.)

What the trace does not reach: anything behind the C ABI; the OOM fallback of the rotation copies (a clone that fails); the cache file
(persistence is off: `_load_persisted` / `_store_persisted` only record that they were called, and with what); real timings - in the
tuner-on pass `_time_thunks` and the GEMM tuner's events are scripted, so WHICH candidate wins is the script's, not a measurement's."""
import contextlib
import hashlib
import importlib.util
import json
import os
import sys
from functools import lru_cache

import pytest
import torch

ROWS = (12, 24, 64, 65, 300)
SHAPES = ((1024, 1024), (256, 512), (256, 384), (254, 512))
SWIGLU_SHAPES = tuple((2 * F, K) for F in (256, 88) for K in (1024, 512, 384))
GUISES = ("tensor", "pair", "codes")
FORMS = ("skinny", "gemm", "slabs", "gemm8", "slabs8", "skinny8")
W8_ENTRIES = ("vdd_skinny_gemm_w8", "vdd_gemm_w8", "vdd_gemm_codes", "vdd_skinny_gemm_resid_ss_w8", "vdd_skinny_gemm_normed_w8",
              "vdd_skinny_swiglu_normed_w8", "vdd_skinny_swiglu_w8")
DT = torch.bfloat16


def _load_ops(path=None):
    path = path or os.environ.get("OPS_TRACE_FILE")
    if not path:
        from llava_align_amd import ops
        return ops
    import llava_align_amd  # noqa: F401
    name = "llava_align_amd._ops_traced_" + hashlib.sha1(os.path.abspath(path).encode()).hexdigest()[:8]
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


class _Recorder:
    """Stands for the loaded library: every vdd_* entry records (name, arguments) and answers 0, or -2 if it is in `refuse`.  Of the
    arguments the integers and floats are kept as they are; a pointer is kept as the name of the operand it points to ("new": a tensor
    the wrapper made itself - an output or a rotation copy)."""

    def __init__(self, sigs):
        self.sigs, self.calls, self.refuse, self.names = sigs, [], frozenset(), {}

    def __getattr__(self, name):
        if not name.startswith("vdd_"):
            raise AttributeError(name)
        ptr = [t.__name__ == "c_void_p" for t in self.sigs[name]]

        def entry(*args):
            assert len(args) == len(ptr), (name, len(args), len(ptr))
            names = self.names
            self.calls.append([name] + [(None if a is None else names.get(a, "new")) if p else a for a, p in zip(args, ptr)])
            return -2 if name in self.refuse else 0
        return entry


class _Event:
    """torch.cuda.Event for the GEMM tuner's timing loop: scripted times, so the winner is deterministic and not the first candidate."""
    ticks = 0

    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass

    def synchronize(self):
        pass

    def elapsed_time(self, other):
        _Event.ticks += 1
        return float((_Event.ticks * 37) % 101 + 1)


class _Env:
    """ops.py with the library, the stream, the dtype check and the GEMM workspace stubbed, and its tables emptied."""

    def __init__(self, path=None):
        self.ops = ops = _load_ops(path)
        self.rec = _Recorder(ops._SIGS)
        self.ws = torch.zeros(64, dtype=torch.uint8)
        self.timed, self.persist, self.pick = [], [], "last"
        self.mp = mp = pytest.MonkeyPatch()
        mp.setenv("VDD_GEMM_CHOICES", "off")
        mp.setattr(ops, "_lib_ready", lambda: self.rec)
        mp.setattr(ops, "_st", lambda t: 0)
        mp.setattr(ops, "_dt", lambda *ts: ops._MODEL_DT[next(t for t in ts if isinstance(t, torch.Tensor)).dtype])
        mp.setattr(ops, "_gemm_workspace", lambda device, M, N: self.ws)
        mp.setattr(ops, "GEMM_AUTOTUNE", False)
        mp.setattr(ops, "_form_choice", {})
        mp.setattr(ops, "_gemm_choice", {})
        mp.setattr(ops, "FORCE_FORM", {})
        mp.setattr(ops, "_persist", {"loaded": None, "path": None, "section": None})
        mp.setattr(ops, "_load_persisted", lambda device: self.persist.append(["load"]))
        mp.setattr(ops, "_store_persisted", lambda key, cfg: self.persist.append(["store", list(key), cfg]))
        mp.setattr(ops, "_time_thunks", self._time_thunks)
        mp.setattr(torch.cuda, "Event", _Event)
        self.capturing = False
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: self.capturing)

    def _time_thunks(self, thunks, n_rot, iters=8, reps=2):
        self.timed.append([list(thunks), n_rot])
        for fn in thunks.values():
            fn(0)
            fn(n_rot - 1)
        return list(thunks)[-1 if self.pick == "last" else 0]

    def close(self):
        self.mp.undo()


@lru_cache(maxsize=None)
def _operands(M, N, K):
    """One set of CPU operands per shape (zeros: nothing computes on them)."""
    z = lambda *s, dt=DT: torch.zeros(*s, dtype=dt)
    return dict(x=z(M, K), w16=z(N, K), codes=z(N, K, dt=torch.uint8), scale=torch.ones(N), resid=z(M, N), bias=z(N), ln_w=z(K),
                ss=z(M, (K + 15) // 16, dt=torch.float32))


class _Call:
    def __init__(self, ops, guise, M, N, K):
        self.__dict__.update(_operands(M, N, K))
        self.w = ops.CodesWeight(self.codes, self.scale, DT) if guise == "codes" else self.w16
        self.kw = dict(w8=(self.codes, self.scale)) if guise == "pair" else {}


def _variants(ops):
    """name -> (shapes, kind family or None, call)."""
    P, S = SHAPES, SWIGLU_SHAPES
    return {
        "gemm": (P, None, lambda o: ops.gemm(o.x, o.w, **o.kw)),
        "gemm.bias": (P, None, lambda o: ops.gemm(o.x, o.w, bias=o.bias, epi=ops.EPI_BIAS, **o.kw)),
        "gemm.config": (P, None, lambda o: ops.gemm(o.x, o.w, config=ops.gemm_config(8, 1), **o.kw)),
        "gemm.resid": (P, None, lambda o: ops.gemm(o.x, o.w, bias=o.bias, resid=o.resid, epi=ops.EPI_BIAS_RESID, **o.kw)),
        "gemm.swiglu": (S, None, lambda o: ops.gemm(o.x, o.w, epi=ops.EPI_SWIGLU, **o.kw)),
        "skinny_gemm": (P, None, lambda o: ops.skinny_gemm(o.x, o.w, **o.kw)),
        "skinny_gemm.resid": (P, None, lambda o: ops.skinny_gemm(o.x, o.w, resid=o.resid, **o.kw)),
        "skinny_gemm.slabs": (P, None, lambda o: ops.skinny_gemm(o.x, o.w, n_split=2, slabs=True, **o.kw)),
        "gemm_slabs": (P, None, lambda o: ops.gemm_slabs(o.x, o.w, 2, **o.kw)),
        "gemm_slabs.tile": (P, None, lambda o: ops.gemm_slabs(o.x, o.w, 4, tile=10, **o.kw)),
        "linear_resid_ss": (P, None, lambda o: ops.linear_resid_ss(o.x, o.w, o.resid, **o.kw)),
        "linear_normed": (P, None, lambda o: ops.linear_normed(o.x, o.ss, o.ln_w, 1e-5, o.w, **o.kw)),
        "linear_normed.bias": (P, None, lambda o: ops.linear_normed(o.x, o.ss, o.ln_w, 1e-5, o.w, bias=o.bias, **o.kw)),
        "swiglu_linear_normed": (S, None, lambda o: ops.swiglu_linear_normed(o.x, o.ss, o.ln_w, 1e-5, o.w, **o.kw)),
        "_skinny_swiglu": (S, None, lambda o: ops._skinny_swiglu(o.x, o.w, **o.kw)),
        "linear": (P, "linear", lambda o: ops.linear(o.x, o.w, **o.kw)),
        "linear.bias": (P, "linear", lambda o: ops.linear(o.x, o.w, bias=o.bias, **o.kw)),
        "linear.keep_bits": (P, "linear", lambda o: ops.linear(o.x, o.w, keep_bits=True, **o.kw)),
        "linear_to_norm": (P, "to_norm", lambda o: ops.linear_to_norm(o.x, o.w, **o.kw)),
        "swiglu_linear": (S, "swiglu", lambda o: ops.swiglu_linear(o.x, o.w, **o.kw)),
    }


def _kinds(family):
    """Every kind a wrapper of this family may read, whatever the guise: the trace sets each in turn for every guise, so an entry under
    another guise's kind shows as 'not read'."""
    return [family + s for s in ("", "8", "8t", "c", "8i")]


def _settings(variant, family):
    """(name, dict) of the settings applied one at a time."""
    out = [("base", {}), ("invariant", dict(inv=True)), ("w8_decode_off", dict(w8off=True))]
    out += [("refuse:" + e, dict(refuse=e)) for e in W8_ENTRIES]
    if family is not None or variant.startswith("gemm") and not variant.startswith("gemm_slabs"):
        out += [("gemm_choice:" + fam, dict(gchoice=fam)) for fam in ("16bit", "w8", "codes")]
        out += [("invariant+gemm_choice:" + fam, dict(gchoice=fam, inv=True)) for fam in ("16bit", "w8", "codes")]
    if family is not None:
        for kind in _kinds(family):
            for form in FORMS:
                out.append((f"force:{kind}={form}", dict(force={kind: form})))
                out.append((f"choice:{kind}={form}", dict(choice=(kind, form))))
        for form in ("gemm", "gemm8"):
            out.append((f"invariant+force:{family}8i={form}", dict(inv=True, force={family + "8i": form})))
            out.append((f"invariant+choice:{family}8i={form}", dict(inv=True, choice=(family + "8i", form))))
            out.append((f"invariant+choice:{family}8={form}", dict(inv=True, choice=(family + "8", form))))
    return out


_GEMM_CHOICE_PRESET = {"16bit": (0, (3, 2)), "w8": (8, (9, 1)), "codes": (16, (11, 0))}     # family: (added to the dtype, (tile, schedule))


def _run(env, call, o, M, N, K, inv=False, w8off=False, refuse=None, gchoice=None, force=None, choice=None, tuner=False, capturing=False, pick="last"):
    """One call under one setting -> its outcome as a JSON string."""
    ops, rec = env.ops, env.rec
    ops._form_choice.clear(); ops._gemm_choice.clear(); ops.FORCE_FORM.clear()
    rec.calls, rec.refuse = [], frozenset([refuse] if refuse else [])
    rec.names = {t.data_ptr(): n for n, t in _operands(M, N, K).items()}
    rec.names[env.ws.data_ptr()] = "ws"
    env.timed, env.persist, env.pick, env.capturing = [], [], pick, capturing
    _Event.ticks = 0
    dt = ops._MODEL_DT[DT]
    with contextlib.ExitStack() as st:
        if inv:
            st.enter_context(ops.batch_invariant())
        if w8off:
            st.enter_context(ops.w8_decode(False))
        if force:
            ops.FORCE_FORM.update(force)
        if choice:
            ops._form_choice[ops._form_key(choice[0], M, N, K, dt)] = choice[1]
        if gchoice:
            off, (tile, sched) = _GEMM_CHOICE_PRESET[gchoice]
            for n in (N, N // 2):
                for epi in range(6):
                    ops._gemm_choice[ops._gemm_key(M, n, K, epi, dt + off)] = ops.gemm_config(tile, sched)
        ops.GEMM_AUTOTUNE = bool(tuner)
        forms0, gemms0, n0, exc = dict(ops._form_choice), dict(ops._gemm_choice), ops.w8_launches(), None
        try:
            call(o)
        except Exception as e:                              # the type and the text are part of the trace
            exc = [type(e).__name__, str(e)]
        finally:
            ops.GEMM_AUTOTUNE = False
        res = dict(w8_launches=ops.w8_launches() - n0, exc=exc,
                   gemm_choice_added=sorted([list(k), v] for k, v in ops._gemm_choice.items() if gemms0.get(k) != v),
                   form_choice_added=sorted([list(k), v] for k, v in ops._form_choice.items() if forms0.get(k) != v))
    if tuner:                                               # hundreds of launches per tuning run: their digest, their census and both ends
        calls = rec.calls
        census = {}
        for c in calls:
            census[c[0]] = census.get(c[0], 0) + 1
        res.update(n_calls=census, sha=hashlib.sha1(json.dumps(calls).encode()).hexdigest()[:16], head=calls[:2], tail=calls[-3:],
                   timed=env.timed, persist=env.persist)
    else:
        res.update(calls=rec.calls)
    return json.dumps(res, sort_keys=True)


def _trace_static(env, variant, guise):
    """{"NxK|M [setting]": outcome} of one wrapper variant in one guise with the tuner off, in a fixed order."""
    shapes, family, call = _variants(env.ops)[variant]
    out = {}
    for N, K in shapes:
        for M in ROWS:
            o = _Call(env.ops, guise, M, N, K)
            for name, kw in _settings(variant, family):
                out[f"{N}x{K}|{M} [{name}]"] = _run(env, call, o, M, N, K, **kw)
    return out


TUNED_VARIANTS = ("gemm", "gemm.bias", "gemm.swiglu", "linear", "linear.keep_bits", "linear_to_norm", "swiglu_linear")
TUNED_SETTINGS = [("tuner", {}), ("tuner+first", dict(pick="first")), ("tuner+invariant", dict(inv=True)), ("tuner+capturing", dict(capturing=True)),
                  ("tuner+w8_decode_off", dict(w8off=True)), ("tuner+refuse:vdd_gemm_w8", dict(refuse="vdd_gemm_w8")),
                  ("tuner+refuse:vdd_gemm_codes", dict(refuse="vdd_gemm_codes")), ("tuner+gemm_choice:w8", dict(gchoice="w8"))]


def _trace_tuned(env, variant, guise):
    """The same with GEMM_AUTOTUNE on: the copies, the consumer norm, the stored keys.  Small weights: 24 rotation copies cost nothing."""
    shapes, family, call = _variants(env.ops)[variant]
    out = {}
    for N, K in ((512, 512), (176, 512)) if shapes is SWIGLU_SHAPES else ((256, 512), (254, 512)):
        for M in (12, 300):                                  # (either side of every threshold the tuner-on paths have: 16, 64, 128, 256 rows)
            o = _Call(env.ops, guise, M, N, K)
            for name, kw in TUNED_SETTINGS:
                out[f"{N}x{K}|{M} [{name}]"] = _run(env, call, o, M, N, K, tuner=True, **kw)
    return out


def _all_variants():
    return [v for v in _VARIANT_NAMES] + ["tuned:" + v for v in TUNED_VARIANTS]


_VARIANT_NAMES = ("gemm", "gemm.bias", "gemm.config", "gemm.resid", "gemm.swiglu", "skinny_gemm", "skinny_gemm.resid", "skinny_gemm.slabs",
                  "gemm_slabs", "gemm_slabs.tile", "linear_resid_ss", "linear_normed", "linear_normed.bias", "swiglu_linear_normed",
                  "_skinny_swiglu", "linear", "linear.bias", "linear.keep_bits", "linear_to_norm", "swiglu_linear")


def _trace(env, name, guise):
    return _trace_tuned(env, name[len("tuned:"):], guise) if name.startswith("tuned:") else _trace_static(env, name, guise)


def _digest(trace):
    return [len(trace), hashlib.sha1(json.dumps(trace, sort_keys=False).encode()).hexdigest()[:16]]


def _brief(outcome):
    """An outcome in words: the exception's type, or the entries in order - the GEMM's with their config."""
    o = json.loads(outcome)
    if o["exc"]:
        return o["exc"][0]
    cfg = {"vdd_gemm": 14, "vdd_gemm_w8": 12, "vdd_gemm_codes": 12}
    return " ".join(f"{c[0][4:]}:{c[cfg[c[0]]]}" if c[0] in cfg else c[0][4:] for c in o["calls"])


# variant -> guise -> [number of cases, SHA-1 (16 hex digits) of their outcomes in order]
EXPECTED = {
    "gemm": {"tensor": [320, "c3de74aab1fbf2a7"], "pair": [320, "679e3300779b6bb4"], "codes": [320, "da002e33c67de9c4"]},
    "gemm.bias": {"tensor": [320, "6331fff1ad520ded"], "pair": [320, "2aa7173f7ddf19e0"], "codes": [320, "d0b90713355bb681"]},
    "gemm.config": {"tensor": [320, "2f89e0a8f9ee80d9"], "pair": [320, "1450a1f62f260890"], "codes": [320, "50330a9bd96fd9a2"]},
    "gemm.resid": {"tensor": [320, "e70de3886365ff01"], "pair": [320, "e70de3886365ff01"], "codes": [320, "9449c27e757e2b25"]},
    "gemm.swiglu": {"tensor": [480, "74c118ad09667d56"], "pair": [480, "f100c3aea8c41fcb"], "codes": [480, "b4b0770aa4e62047"]},
    "skinny_gemm": {"tensor": [200, "2b45c41057c0cfe9"], "pair": [200, "5e92e19bf0804e35"], "codes": [200, "96a4e0c42d245e92"]},
    "skinny_gemm.resid": {"tensor": [200, "2446a430f5639d37"], "pair": [200, "2446a430f5639d37"], "codes": [200, "837ffa3168d985f9"]},
    "skinny_gemm.slabs": {"tensor": [200, "5201462373b1b0a1"], "pair": [200, "5201462373b1b0a1"], "codes": [200, "837ffa3168d985f9"]},
    "gemm_slabs": {"tensor": [200, "9506dfb40646efc9"], "pair": [200, "51bee7b09862dc6b"], "codes": [200, "d5020873f7094508"]},
    "gemm_slabs.tile": {"tensor": [200, "17bfb9be3d0caac3"], "pair": [200, "fa47476b2002217f"], "codes": [200, "0a521a85077b9c70"]},
    "linear_resid_ss": {"tensor": [200, "cc4e543b53bfddd1"], "pair": [200, "4922b192f41340f7"], "codes": [200, "15b9bd2dd7a3a383"]},
    "linear_normed": {"tensor": [200, "f274fbd203d71a18"], "pair": [200, "a782dc46bb563330"], "codes": [200, "f6c44b9f3f20c177"]},
    "linear_normed.bias": {"tensor": [200, "3af4bf1a1f149023"], "pair": [200, "8acdd5bf81f9bae6"], "codes": [200, "a7945b4a9749bb07"]},
    "swiglu_linear_normed": {"tensor": [300, "d59c2ec6aa806d0b"], "pair": [300, "2913d8159688d315"], "codes": [300, "4aefbfa8c4ea7258"]},
    "_skinny_swiglu": {"tensor": [300, "ccf2c6cd635a9a4f"], "pair": [300, "9423c37d115e27b3"], "codes": [300, "5279bcf327e246b0"]},
    "linear": {"tensor": [1640, "ab7b7546a9dc8156"], "pair": [1640, "370af7e9a93b45c2"], "codes": [1640, "8b8e793a2f9b6f44"]},
    "linear.bias": {"tensor": [1640, "3574d22735f5245e"], "pair": [1640, "158560806565230d"], "codes": [1640, "f1a48fceec3e545c"]},
    "linear.keep_bits": {"tensor": [1640, "ab7b7546a9dc8156"], "pair": [1640, "8282f681b1f8d70c"], "codes": [1640, "8b8e793a2f9b6f44"]},
    "linear_to_norm": {"tensor": [1640, "8c6fe3e101103a84"], "pair": [1640, "f572dd7666adb161"], "codes": [1640, "3fca93ae93f1a6b5"]},
    "swiglu_linear": {"tensor": [2460, "614e05a04c438c51"], "pair": [2460, "08c6215dfe84d09a"], "codes": [2460, "e1cfb2899d17d5dd"]},
    "tuned:gemm": {"tensor": [32, "428deb78d1324fec"], "pair": [32, "ed6b5a9fc006bd7f"], "codes": [32, "8bab96254db044d6"]},
    "tuned:gemm.bias": {"tensor": [32, "3e7a25ebc4000190"], "pair": [32, "015117f428e99afc"], "codes": [32, "b471cace1dfc56bf"]},
    "tuned:gemm.swiglu": {"tensor": [32, "c2bb402292b9c27a"], "pair": [32, "5f27b30c09b20053"], "codes": [32, "7a2cf67b3f21fb46"]},
    "tuned:linear": {"tensor": [32, "6db2bdb525464088"], "pair": [32, "ad2b74eccab91e58"], "codes": [32, "6594e4c21e516b56"]},
    "tuned:linear.keep_bits": {"tensor": [32, "6db2bdb525464088"], "pair": [32, "de71817d3e415f61"], "codes": [32, "6594e4c21e516b56"]},
    "tuned:linear_to_norm": {"tensor": [32, "2fc43299e008c980"], "pair": [32, "57f9c4ea64d73ec6"], "codes": [32, "35bbc3559aa18f84"]},
    "tuned:swiglu_linear": {"tensor": [32, "2c19f2e59bdaa391"], "pair": [32, "c3af849ecb51f732"], "codes": [32, "5c98d28ffeb759a6"]},
}

# "variant|guise|NxK|M [setting]" -> the outcome in words (`_brief`): what the digests above stand for, at the thresholds a reader knows
READABLE = {
    "linear|tensor|1024x1024|12 [base]": "skinny_gemm",
    "linear|tensor|1024x1024|24 [base]": "gemm:1",
    "linear|tensor|1024x1024|300 [base]": "gemm:1",
    "linear|tensor|1024x1024|12 [invariant]": "gemm:17",
    "linear|pair|1024x1024|12 [base]": "skinny_gemm",
    "linear|pair|1024x1024|24 [base]": "gemm:1",
    "linear|pair|1024x1024|300 [base]": "gemm:1",
    "linear|pair|1024x1024|12 [invariant]": "gemm:17",
    "linear|codes|1024x1024|12 [base]": "skinny_gemm_w8",
    "linear|codes|1024x1024|24 [base]": "gemm_codes:1",
    "linear|codes|1024x1024|300 [base]": "gemm_codes:1",
    "linear|codes|1024x1024|12 [invariant]": "gemm_codes:17",
    "swiglu_linear|tensor|512x1024|12 [base]": "skinny_swiglu",
    "swiglu_linear|tensor|512x1024|24 [base]": "gemm:1",
    "swiglu_linear|pair|512x1024|12 [base]": "skinny_swiglu",
    "swiglu_linear|pair|512x1024|24 [base]": "gemm:1",
    "swiglu_linear|codes|512x1024|12 [base]": "skinny_swiglu_w8",
    "swiglu_linear|codes|512x1024|24 [base]": "gemm_codes:1",
    "swiglu_linear|tensor|176x512|24 [base]": "gemm:1 silu_mul",
    "swiglu_linear|tensor|176x512|24 [w8_decode_off]": "gemm:1 silu_mul",
    "swiglu_linear|pair|176x512|24 [base]": "gemm:1 silu_mul",
    "swiglu_linear|pair|176x512|24 [w8_decode_off]": "gemm:1 silu_mul",
    "swiglu_linear|codes|176x512|24 [base]": "gemm_codes:1 silu_mul",
    "swiglu_linear|codes|176x512|24 [w8_decode_off]": "RuntimeError",
    "gemm|tensor|256x512|24 [gemm_choice:16bit]": "gemm:35",
    "gemm|tensor|256x512|24 [gemm_choice:w8]": "gemm:1",
    "gemm|tensor|256x512|24 [gemm_choice:codes]": "gemm:1",
    "gemm|pair|256x512|24 [gemm_choice:16bit]": "gemm:35",
    "gemm|pair|256x512|24 [gemm_choice:w8]": "gemm_w8:25",
    "gemm|pair|256x512|24 [gemm_choice:codes]": "gemm:1",
    "gemm|codes|256x512|24 [gemm_choice:16bit]": "gemm_codes:1",
    "gemm|codes|256x512|24 [gemm_choice:w8]": "gemm_codes:1",
    "gemm|codes|256x512|24 [gemm_choice:codes]": "gemm_codes:11",
    "linear_normed|tensor|256x512|12 [base]": "skinny_gemm_normed",
    "linear_normed|tensor|256x512|12 [refuse:vdd_skinny_gemm_normed_w8]": "skinny_gemm_normed",
    "linear_normed|pair|256x512|12 [base]": "skinny_gemm_normed_w8",
    "linear_normed|pair|256x512|12 [refuse:vdd_skinny_gemm_normed_w8]": "skinny_gemm_normed_w8 skinny_gemm_normed",
    "linear_normed|codes|256x512|12 [base]": "skinny_gemm_normed_w8",
    "linear_normed|codes|256x512|12 [refuse:vdd_skinny_gemm_normed_w8]": "ValueError",
}
_READABLE_CASES = [("linear", g, f"1024x1024|{M} [{s}]") for g in GUISES for M, s in ((12, "base"), (24, "base"), (300, "base"), (12, "invariant"))] \
    + [("swiglu_linear", g, f"512x1024|{M} [base]") for g in GUISES for M in (12, 24)] \
    + [("swiglu_linear", g, f"176x512|24 [{s}]") for g in GUISES for s in ("base", "w8_decode_off")] \
    + [("gemm", g, f"256x512|24 [gemm_choice:{fam}]") for g in GUISES for fam in ("16bit", "w8", "codes")] \
    + [("linear_normed", g, f"256x512|12 [{s}]") for g in GUISES for s in ("base", "refuse:vdd_skinny_gemm_normed_w8")]


@pytest.fixture(scope="module")
def env():
    e = _Env()
    yield e
    e.close()


def test_variant_list_is_complete(env):
    assert set(_VARIANT_NAMES) == set(_variants(env.ops)) and set(EXPECTED) == set(_all_variants())


@pytest.mark.parametrize("guise", GUISES)
@pytest.mark.parametrize("name", _all_variants())
def test_dispatch_trace(env, name, guise):
    trace = _trace(env, name, guise)
    for v, g, case in _READABLE_CASES:
        if (v, g) == (name, guise):
            assert _brief(trace[case]) == READABLE[f"{v}|{g}|{case}"], f"{v}|{g}|{case}"
    assert _digest(trace) == EXPECTED[name][guise], (
        f"the dispatch of {name} with a {guise} weight changed: `python tests/test_ops_dispatch_trace.py --diff <ops.py of the parent revision>` "
        f"lists the outcomes that differ")


def _record(path=None):
    e = _Env(path)
    try:
        return {name: {g: _trace(e, name, g) for g in GUISES} for name in _all_variants()}
    finally:
        e.close()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["--record"]:
        traces = _record()
        print("EXPECTED = {")
        for name, by_guise in traces.items():
            print(f"    {json.dumps(name)}: {json.dumps({g: _digest(t) for g, t in by_guise.items()})},")
        print("}\nREADABLE = {")
        for v, g, case in _READABLE_CASES:
            print(f"    {json.dumps(f'{v}|{g}|{case}')}: {json.dumps(_brief(traces[v][g][case]))},")
        print("}")
    elif len(sys.argv) == 3 and sys.argv[1] == "--diff":
        here, there = _record(), _record(sys.argv[2])
        n = 0
        for name in here:
            for g in GUISES:
                for case, got in here[name][g].items():
                    if got != there[name][g].get(case):
                        n += 1
                        print(f"{name}|{g}|{case}\n  {sys.argv[2]}: {str(there[name][g].get(case))[:1500]}\n  the package: {got[:1500]}")
        print(f"{n} outcomes differ")
        sys.exit(1 if n else 0)
    else:
        sys.exit("usage: python tests/test_ops_dispatch_trace.py --record | --diff OTHER_OPS_PY")
