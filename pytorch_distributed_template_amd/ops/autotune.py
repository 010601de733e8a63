"""Tuned kernel choices: the table, the policy, the timing and the one selection protocol.

Every GEMM, convolution and weight gradient of the ``native_ops`` package has several tile variants, and some
fusions only pay on some geometries. The first eager call of a distinct geometry times the
candidates with HIP events and keeps the fastest under a key (``<family>:<geometry>``); every later
call is a dictionary lookup. No kernel binding lives here: a call site hands :func:`choose` its key,
a function that builds the launch, and the value to use when tuning is not allowed.

Table. The shipped table (``_lib/autotune_gfx950.json``, tracked) is READ-ONLY at run time; new
entries go to a per-user cache (``PDT_AUTOTUNE_CACHE``, default
``~/.cache/pytorch_distributed_template_amd/autotune_gfx950.json``) overlaid on it at load;
``PDT_AUTOTUNE_SHIPPED=0`` ignores the shipped table (re-tuning experiments). Values are variant ids;
-1 = no candidate applies (the site's heuristic / generic path), ``AX_UNFUSED`` = the unfused
reference path measured faster than every candidate.

Policy (:func:`tune_allowed`). ``PDT_AUTOTUNE=0`` or ``--deterministic`` (``PDT_DETERMINISTIC=1``):
no timing at all -- shipped/cached choices, else the site's fixed default, so every run and every
rank picks the same variant (and the same split-K summation order). Never during a graph capture.
World size > 1: ranks must not time variants independently (different choices per rank, stragglers
inside the first backward): tuning is off unless ``native_ops.pretune_distributed`` (``native_ops/tuning.py``) runs -- rank 0
tunes one step inside :func:`forced_tuning` and broadcasts its table; every rank :func:`adopt`s it,
which freezes tuning for the rest of the process.

Developer knobs. ``PDT_TUNE_ROUNDS`` (default 2): the rounds of a variant sweep (:func:`time_candidates`);
more rounds cut the timing noise of a (re)tune run at the cost of its length (the comparison against a
reference path always uses two). ``PDT_NT_VARIANTS="0-29,31"``: the first tune of an ``nt5:`` /
``ntb2:`` key may only pick from these ids (a re-tune ignores it). ``PDT_RETUNE_WITH="45-48"``: a
targeted re-tune -- every ``nt5:`` / ``ntb2:`` key ALREADY in the table is timed once more, once per
process, against these ids plus its current choice, and switches when one of them is faster
(``PDT_RETUNE_PREFIX="ntb2:"``: only the keys of one family). ``PDT_RETUNE_WG``: the same for
``wg2:`` keys. ``PDT_RETUNE_AX``: the same for the ``ax*:`` keys; there the ids need not be among
the first tune's candidates, and a current choice < 0 (unfused) is not a candidate.
"""
from __future__ import annotations

import contextlib
import json
import os
from functools import lru_cache
from pathlib import Path

import torch

NOT_APPLICABLE = -5  # kernel return code: this variant cannot run this geometry
AX_UNFUSED = -2      # table value: the unfused reference path beat every candidate here

# the shipped table lives next to the kernel library (PDT_LIB_PATH moves both: A/B builds)
SHIPPED_PATH = (Path(os.environ["PDT_LIB_PATH"]).parent if os.environ.get("PDT_LIB_PATH")
                else Path(__file__).resolve().parents[1] / "_lib") / "autotune_gfx950.json"
CACHE_PATH = Path(os.environ.get("PDT_AUTOTUNE_CACHE", str(Path.home() / ".cache" / "pytorch_distributed_template_amd"
                                                           / "autotune_gfx950.json")))
_table: dict | None = None
_forced = _frozen = False  # forced_tuning(): rank 0 tunes although WORLD_SIZE > 1; adopt(): no rank tunes any more
_retuned: set = set()
# re-tune variable -> (variable holding a key prefix or None, keep only ids among the site's candidates?)
_RETUNE = {"PDT_RETUNE_WITH": ("PDT_RETUNE_PREFIX", True), "PDT_RETUNE_WG": (None, True),
           "PDT_RETUNE_AX": (None, False)}


def tuned() -> dict:
    global _table
    if _table is None:
        _table = {}
        paths = (SHIPPED_PATH, CACHE_PATH) if os.environ.get("PDT_AUTOTUNE_SHIPPED", "1") != "0" else (CACHE_PATH,)
        for path in paths:
            try:
                _table.update(json.loads(Path(path).read_text()))
            except Exception:
                pass
    return _table


def save():
    """Persist the table to the user cache (never the installed package)."""
    if os.environ.get("RANK", "0") != "0" or CACHE_PATH.resolve() == SHIPPED_PATH.resolve():
        return
    try:
        CACHE_PATH.parent.mkdir(parents=True, exist_ok=True)
        tmp = str(CACHE_PATH) + f".tmp{os.getpid()}"
        Path(tmp).write_text(json.dumps(_table, indent=0, sort_keys=True))
        os.replace(tmp, CACHE_PATH)
    except Exception:
        pass


def capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def tune_allowed() -> bool:
    if _frozen or capturing():
        return False
    if os.environ.get("PDT_AUTOTUNE", "1") == "0" or os.environ.get("PDT_DETERMINISTIC", "0") == "1":
        return False
    return _forced or int(os.environ.get("WORLD_SIZE", "1")) <= 1


@contextlib.contextmanager
def forced_tuning():
    """Tuning although WORLD_SIZE > 1 (rank 0's pre-tuning step)."""
    global _forced
    _forced = True
    try:
        yield
    finally:
        _forced = False


def adopt(table: dict) -> None:
    """Replace the table by ``table`` (rank 0's, after the broadcast) and freeze it."""
    global _frozen
    tuned().clear()
    _table.update(table)
    _frozen = True


def trial_ms(fn) -> float:
    """Device time of three back-to-back ``fn()`` (the only place this module touches the GPU)."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(3):
        fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1)


def time_candidates(ids, launch, rounds) -> dict:
    """{id: best trial, ms} of the applicable ``ids``: one warm ``launch(id)`` each, then ``rounds`` rounds of one
    trial each, interleaved (a clock / cache transient must not favour whichever candidates run first)."""
    best = {}
    for v in ids:
        rc = launch(v)
        if rc == NOT_APPLICABLE:  # e.g. the streaming 1x1 kernel on a 3x3 geometry
            continue
        if rc:
            raise RuntimeError(f"tune variant {v} failed with code {rc}")
        best[v] = float("inf")
    for _ in range(rounds):
        for v in best:
            best[v] = min(best[v], trial_ms(lambda: launch(v)))
    return best


def _ms(fn) -> float:
    return time_candidates((0,), lambda _: fn() and 0, 2)[0]  # (whatever fn returns is no kernel code)


def id_set(spec) -> set:  # "0-29,31" -> {0, ..., 29, 31}
    out = set()
    for part in spec.split(","):
        lo, _, hi = part.partition("-")
        out.update(range(int(lo), int(hi or lo) + 1))
    return out


def _retune_ids(key, table, var):
    """The ids a targeted re-tune (variable ``var``) times ``key`` against now, or None."""
    spec = os.environ.get(var)
    if not spec or key in _retuned or key not in table or not tune_allowed():
        return None
    prefix = _RETUNE[var][0]
    if prefix and not key.startswith(os.environ.get(prefix, "")):
        return None
    _retuned.add(key)
    return id_set(spec) | {int(table[key])}


def choose(key, setup, default, *, retune=None, first_only=None, ref=None, ref_value=AX_UNFUSED, ref_first=False):
    """The tuned choice for ``key``: the table's entry; else, when tuning is not allowed, ``default`` (a
    value, or a function called for it) -- returned, not stored; else the fastest candidate, timed now,
    stored and saved (-1: no candidate applies). ``setup()`` -> (candidate ids, ``launch``) is called
    on a miss only, so tune-only scratch is allocated only then; ``launch(id)`` returns the kernel's
    code. ``retune`` / ``first_only`` name the variables of a targeted re-tune / a restricted first tune
    (module docstring). ``ref()``: the unfused alternative; when it is faster than the winner the key
    stores ``ref_value``. ``ref_first``: one untimed ``ref()`` first (a path that tunes itself then)."""
    table = tuned()
    ids = _retune_ids(key, table, retune) if retune else None
    if ids is None and key in table:
        return int(table[key])
    if not tune_allowed():
        return default() if callable(default) else default
    cand, launch = setup()
    if ids is None:
        spec = os.environ.get(first_only) if first_only else None
        ids = id_set(spec) if spec else None
    elif not _RETUNE[retune][1]:
        cand, ids = sorted(v for v in ids if v >= 0), None
    if ids is not None:
        cand = [v for v in cand if v in ids]
    times = time_candidates(cand, launch, max(1, int(os.environ.get("PDT_TUNE_ROUNDS", "2"))))
    best = min(times, key=times.get) if times else -1
    if ref is not None:
        if ref_first:
            ref()
        if best >= 0 and _ms(ref) < _ms(lambda: launch(best)):
            best = ref_value
    table[key] = best
    save()
    return best


# One builder per key family, a pure function of the geometry (memoised: the hot path
# formats a key once per geometry). The strings are the shipped table's: never change them.
def _csv(*xs) -> str:
    return ",".join(str(x) for x in xs)


@lru_cache(maxsize=None)
def nt_key(Hs, Ws, Cs, Nimg, Hm, Wm, Ncol, K, sh, sw, nth, ntw, osh, with_stats, has_bias, pix=0, act=0) -> str:
    """conv_nt; ``pix``: elements per source pixel when not Cs; ``act``: epilogue id (it changes the best tile)."""
    return "nt5:" + _csv(Hs, Ws, Cs, Nimg, Hm, Wm, Ncol, K, sh, sw, nth, ntw, osh, int(with_stats), int(has_bias)) + \
        (f",p{pix}" if pix else "") + (f",a{int(act)}" if act else "")


@lru_cache(maxsize=None)
def ntb_key(Hs, Ws, Cs, Nimg, Hm, Wm, Ncol, K, sh, sw, nth, ntw, osh, has_addend, has_mask, two=False) -> str:
    """conv_nt with the fused BN-backward epilogue; ``two``: also a second unit's partials."""
    return "ntb2:" + _csv(Hs, Ws, Cs, Nimg, Hm, Wm, Ncol, K, sh, sw, nth, ntw, osh, int(has_addend), int(has_mask)) + \
        (",2" if two else "")


@lru_cache(maxsize=None)
def wg_key(M, Mo, No, Hs, Ws, C, Hm, Wm, sh, ntw, pix=0, bn=False) -> str:
    """conv_wgrad; ``bn``: with the BN backward apply in its dY staging (conv_wgrad_bn)."""
    return ("wgb:" if bn else "wg2:") + _csv(M, Mo, No, Hs, Ws, C, Hm, Wm, sh, ntw) + (f",p{pix}" if pix else "")


@lru_cache(maxsize=None)
def axf_key(H, W, Cs, N, Cout, has_res, has_ru, with_stats, KH=1, KW=1, ph=0) -> str:
    """Forward conv with the deferred BN apply in its A staging."""
    return "axf:" + _csv(H, W, Cs, N, Cout, int(has_res), int(has_ru), int(with_stats)) + \
        (f",k{KH}x{KW}p{ph}" if KH != 1 or KW != 1 else "")


def axb_key(H, W, Cout, N, Cin, side=False) -> str:
    """conv3 data gradient with bn3's backward apply in its A staging; ``side``: a downsample block."""
    return ("axd:" if side else "axb:") + _csv(H, W, Cout, N, Cin)


@lru_cache(maxsize=None)
def ax3_key(Ho, Wo, Cout, N, Cin, KH, KW, ph, has_addend=False, has_addend_mask=False, has_bnb_mask=False) -> str:
    """conv2 / conv1 data gradient with the BN backward apply in its A staging."""
    return "ax3:" + _csv(Ho, Wo, Cout, N, Cin, KH, KW, ph) + \
        (f",a{int(has_addend)}{int(has_addend_mask)}m{int(has_bnb_mask)}" if has_addend or has_bnb_mask else "")


def stem_key(N, H, W, Cout, wgrad=False) -> str:
    """Halo-patch stem kernel or the generic space-to-depth GEMM (forward / weight gradient)."""
    return ("stem2w:" if wgrad else "stem1:") + _csv(N, H, W, Cout)


@lru_cache(maxsize=None)
def f8_key(M, N, K, fmt_a, act, has_bias, residual=False, q8=None, colsum=False) -> str:
    """fp8 GEMM. ``residual``: an addend in a plain epilogue (a different best tile); ``q8`` =
    (format, only): the epilogue also writes the output's fp8 codes; ``colsum``: and its column sums."""
    return "f8c:" + _csv(M, N, K, fmt_a, act, int(has_bias)) + (",r" if residual else "") + \
        (f",q{q8[0]}{int(q8[1])}" if q8 is not None else "") + (",cs" if colsum else "")


@lru_cache(maxsize=None)
def wg8_key(M, Nout, K) -> str:
    """fp8 nn.Linear weight gradient."""
    return "wg8:" + _csv(M, Nout, K)
