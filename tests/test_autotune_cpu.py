"""The tuned-choice protocol of ``ops/autotune.py`` without a GPU or the kernel library: the
timing trial is replaced by scripted times, the cache lives in ``tmp_path``."""
import json
import os
import re

import pytest

from pytorch_distributed_template_amd.ops import autotune as at

NA = at.NOT_APPLICABLE


@pytest.fixture
def tuner(monkeypatch, tmp_path):
    """A fresh tuner: empty table, cache in tmp_path, tuning allowed, scripted trial times."""
    for var in ("PDT_AUTOTUNE", "PDT_DETERMINISTIC", "WORLD_SIZE", "RANK", "PDT_TUNE_ROUNDS", "PDT_NT_VARIANTS",
                "PDT_RETUNE_WITH", "PDT_RETUNE_PREFIX", "PDT_RETUNE_WG", "PDT_RETUNE_AX"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("PDT_AUTOTUNE_SHIPPED", "0")
    monkeypatch.setattr(at, "CACHE_PATH", tmp_path / "cache" / "tune.json")
    monkeypatch.setattr(at, "SHIPPED_PATH", tmp_path / "shipped.json")
    monkeypatch.setattr(at, "_table", None)
    monkeypatch.setattr(at, "_frozen", False)
    monkeypatch.setattr(at, "_forced", False)
    monkeypatch.setattr(at, "_retuned", set())
    return _Tuner(monkeypatch)


class _Tuner:
    """``ms``: candidate id (or "ref") -> scripted trial time. ``site(ids)`` makes the (setup,
    launch) pair of a call site whose launches tell the fake trial which id is running."""

    def __init__(self, monkeypatch):
        self.ms, self.codes = {}, {}
        self.launched, self.trials, self.setups, self.ref_calls = [], [], 0, 0
        self._now = None
        monkeypatch.setattr(at, "trial_ms", self._trial)

    def _trial(self, fn):
        fn()
        self.trials.append(self._now)
        return self.ms[self._now]

    def launch(self, v):
        self._now = v
        self.launched.append(v)
        return self.codes.get(v, 0)

    def ref(self):
        self._now = "ref"
        self.ref_calls += 1

    def site(self, ids):
        def setup():
            self.setups += 1
            return ids, self.launch
        return setup

    def cache(self):
        return json.loads(at.CACHE_PATH.read_text()) if at.CACHE_PATH.exists() else None


def _never():
    raise AssertionError("must not be called")


# ------------------------------------------------------------------ 1. table hit
def test_hit_returns_entry_and_asks_nothing(tuner):
    at.tuned()["k"] = "7"
    assert at.choose("k", _never, _never, ref=_never, retune="PDT_RETUNE_WITH", first_only="PDT_NT_VARIANTS") == 7
    assert tuner.trials == [] and at.tuned() == {"k": "7"} and tuner.cache() is None


# ------------------------------------------------------------------ 2. not allowed
@pytest.mark.parametrize("how", ["PDT_AUTOTUNE=0", "PDT_DETERMINISTIC=1", "WORLD_SIZE=2", "frozen"])
def test_not_allowed_returns_default_and_stores_nothing(tuner, monkeypatch, how):
    if how == "frozen":
        at.adopt({})
    else:
        monkeypatch.setenv(*how.split("="))
    assert not at.tune_allowed()
    assert at.choose("k", _never, 5) == 5
    assert at.choose("k", _never, lambda: 9, ref=_never) == 9
    assert at.tuned() == {} and tuner.cache() is None and tuner.trials == []


# ------------------------------------------------------------------ 3. miss, tuning allowed
def test_miss_stores_and_saves_the_fastest_applicable(tuner, monkeypatch):
    tuner.ms = {0: 3.0, 1: 1.0, 3: 2.0}
    tuner.codes = {2: NA}
    replaced = []
    real = os.replace
    monkeypatch.setattr(os, "replace", lambda a, b: (replaced.append((str(a), str(b))), real(a, b)))
    assert at.choose("k", tuner.site(range(4)), _never) == 1
    assert at.tuned() == {"k": 1} and tuner.cache() == {"k": 1} and tuner.setups == 1
    assert tuner.launched.count(2) == 1 and 2 not in tuner.trials  # warm launch only: never timed
    assert tuner.trials == [0, 1, 3, 0, 1, 3]  # two interleaved rounds (PDT_TUNE_ROUNDS default)
    assert [b for _, b in replaced] == [str(at.CACHE_PATH)] and replaced[0][0] != replaced[0][1]
    assert os.listdir(at.CACHE_PATH.parent) == [at.CACHE_PATH.name]  # no temporary left


def test_best_trial_counts_and_rounds_follow_the_variable(tuner, monkeypatch):
    monkeypatch.setenv("PDT_TUNE_ROUNDS", "3")
    seq = {0: iter([5.0, 1.0, 5.0]), 1: iter([2.0, 2.0, 2.0])}
    monkeypatch.setattr(at, "trial_ms", lambda fn: next(seq[(fn(), tuner._now)[1]]))
    assert at.choose("k", tuner.site((0, 1)), _never) == 0  # best trial, not the first or the mean


def test_warm_launch_error_is_raised_and_nothing_stored(tuner):
    tuner.codes = {1: 3}
    with pytest.raises(RuntimeError, match="tune variant 1 failed with code 3"):
        at.choose("k", tuner.site((0, 1)), _never)
    assert at.tuned() == {} and tuner.cache() is None


def test_no_applicable_candidate_stores_minus_one(tuner):
    tuner.codes = {0: NA, 1: NA}
    assert at.choose("k", tuner.site((0, 1)), _never, ref=tuner.ref) == -1
    assert at.tuned() == {"k": -1} and tuner.cache() == {"k": -1} and tuner.trials == []


def test_save_skipped_off_rank_zero(tuner, monkeypatch):
    monkeypatch.setenv("RANK", "1")
    tuner.ms = {0: 1.0}
    assert at.choose("k", tuner.site((0,)), _never) == 0
    assert at.tuned() == {"k": 0} and tuner.cache() is None


def test_save_never_writes_the_shipped_path(tuner, monkeypatch, tmp_path):
    shipped = tmp_path / "shipped.json"
    shipped.write_text('{"old": 1}')
    monkeypatch.setattr(at, "CACHE_PATH", tmp_path / "cache" / ".." / "shipped.json")  # the shipped file
    tuner.ms = {0: 1.0}
    assert at.choose("k", tuner.site((0,)), _never) == 0
    assert json.loads(shipped.read_text()) == {"old": 1}


def test_table_is_shipped_overlaid_with_cache(tuner, monkeypatch):
    at.SHIPPED_PATH.write_text('{"a": 1, "b": 2}')
    at.CACHE_PATH.parent.mkdir()
    at.CACHE_PATH.write_text('{"b": 3}')
    assert at.tuned() == {"b": 3}  # PDT_AUTOTUNE_SHIPPED=0 (the fixture)
    monkeypatch.setenv("PDT_AUTOTUNE_SHIPPED", "1")
    monkeypatch.setattr(at, "_table", None)
    assert at.tuned() == {"a": 1, "b": 3}


# ------------------------------------------------------------------ 4. reference comparison
def test_faster_reference_stores_the_unfused_value(tuner):
    tuner.ms = {0: 2.0, 1: 1.0, "ref": 0.5}
    assert at.choose("k", tuner.site((0, 1)), _never, ref=tuner.ref) == at.AX_UNFUSED
    assert at.tuned() == {"k": at.AX_UNFUSED} == tuner.cache()
    # sweep (two rounds), then the reference and the winner: one warm call + two trials each
    assert tuner.trials == [0, 1, 0, 1, "ref", "ref", 1, 1] and tuner.ref_calls == 3


def test_slower_reference_stores_the_winner(tuner):
    tuner.ms = {0: 2.0, 1: 1.0, "ref": 1.5}
    assert at.choose("k", tuner.site((0, 1)), _never, ref=tuner.ref, ref_value=-1) == 1
    assert tuner.cache() == {"k": 1}


def test_stem_form_runs_the_reference_once_untimed_first(tuner):
    tuner.ms = {0: 1.0, 1: 2.0, "ref": 0.5}
    assert at.choose("k", tuner.site((0, 1)), 1, ref=tuner.ref, ref_value=-1, ref_first=True) == -1
    assert tuner.ref_calls == 4 and tuner.trials.count("ref") == 2  # untimed + warm + two trials
    assert tuner.cache() == {"k": -1}


# ------------------------------------------------------------------ 5. re-tune variables
@pytest.mark.parametrize("var", ["PDT_RETUNE_WITH", "PDT_RETUNE_WG", "PDT_RETUNE_AX"])
def test_retune_times_an_existing_key_once(tuner, monkeypatch, var):
    monkeypatch.setenv(var, "4-5,9")
    tuner.ms = {v: 10.0 - v for v in range(12)}
    at.tuned().update({"k": 2})
    assert at.choose("k", tuner.site(range(12)), _never, retune=var) == 9
    assert sorted(set(tuner.launched)) == [2, 4, 5, 9]  # the given ids plus the current choice
    assert at.tuned()["k"] == 9 and tuner.cache()["k"] == 9
    n = len(tuner.launched)
    assert at.choose("k", _never, _never, retune=var) == 9 and len(tuner.launched) == n  # a plain hit now


@pytest.mark.parametrize("var", ["PDT_RETUNE_WITH", "PDT_RETUNE_WG", "PDT_RETUNE_AX"])
def test_retune_leaves_a_missing_key_to_a_full_first_tune(tuner, monkeypatch, var):
    monkeypatch.setenv(var, "1")
    tuner.ms = {0: 1.0, 1: 2.0, 2: 3.0}
    assert at.choose("new", tuner.site(range(3)), _never, retune=var) == 0
    assert sorted(set(tuner.launched)) == [0, 1, 2]


def test_retune_of_another_variable_or_without_one_is_a_hit(tuner, monkeypatch):
    monkeypatch.setenv("PDT_RETUNE_WG", "1")
    at.tuned().update({"k": 2})
    assert at.choose("k", _never, _never, retune="PDT_RETUNE_AX") == 2
    assert at.choose("k", _never, _never) == 2


def test_retune_not_allowed_is_a_hit(tuner, monkeypatch):
    monkeypatch.setenv("PDT_RETUNE_WITH", "1")
    monkeypatch.setenv("PDT_AUTOTUNE", "0")
    at.tuned().update({"k": 2})
    assert at.choose("k", _never, _never, retune="PDT_RETUNE_WITH") == 2


def test_retune_ax_drops_a_negative_choice_and_takes_ids_outside_the_candidates(tuner, monkeypatch):
    monkeypatch.setenv("PDT_RETUNE_AX", "40,41")
    tuner.ms = {40: 2.0, 41: 1.0, "ref": 5.0}
    at.tuned().update({"k": at.AX_UNFUSED})
    assert at.choose("k", tuner.site((0, 1, 3)), _never, retune="PDT_RETUNE_AX", ref=tuner.ref) == 41
    assert sorted(set(tuner.launched)) == [40, 41]


@pytest.mark.parametrize("var", ["PDT_RETUNE_WITH", "PDT_RETUNE_WG"])
def test_retune_of_library_variants_ignores_ids_the_site_does_not_have(tuner, monkeypatch, var):
    monkeypatch.setenv(var, "1,40")
    tuner.ms = {1: 1.0}
    at.tuned().update({"k": -1})
    assert at.choose("k", tuner.site(range(4)), _never, retune=var) == 1
    assert sorted(set(tuner.launched)) == [1]


def test_retune_prefix_excludes_other_families(tuner, monkeypatch):
    monkeypatch.setenv("PDT_RETUNE_WITH", "3")
    monkeypatch.setenv("PDT_RETUNE_PREFIX", "ntb2:")
    tuner.ms = {2: 2.0, 3: 1.0}
    at.tuned().update({"nt5:1": 2, "ntb2:1": 2, "wg2:1": 2})
    assert at.choose("nt5:1", _never, _never, retune="PDT_RETUNE_WITH") == 2
    assert at.choose("ntb2:1", tuner.site(range(4)), _never, retune="PDT_RETUNE_WITH") == 3
    monkeypatch.setenv("PDT_RETUNE_WG", "3")  # the prefix belongs to PDT_RETUNE_WITH alone
    assert at.choose("wg2:1", tuner.site(range(4)), _never, retune="PDT_RETUNE_WG") == 3


def test_nt_variants_restricts_a_first_tune_only(tuner, monkeypatch):
    monkeypatch.setenv("PDT_NT_VARIANTS", "1-2")
    tuner.ms = {0: 1.0, 1: 3.0, 2: 2.0, 3: 0.5}
    kw = dict(retune="PDT_RETUNE_WITH", first_only="PDT_NT_VARIANTS")
    assert at.choose("k", tuner.site(range(4)), _never, **kw) == 2
    assert sorted(set(tuner.launched)) == [1, 2]
    tuner.launched.clear()
    monkeypatch.setenv("PDT_RETUNE_WITH", "3")
    assert at.choose("k", tuner.site(range(4)), _never, **kw) == 3  # id 3 is outside PDT_NT_VARIANTS
    assert sorted(set(tuner.launched)) == [2, 3]
    assert at.choose("other", tuner.site(range(4)), _never) == 3  # a site that does not name the filter


# ------------------------------------------------------------------ 6. forced tuning, adopt
def test_forced_tuning_and_adopt(tuner, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert not at.tune_allowed()
    with pytest.raises(KeyError):
        with at.forced_tuning():
            assert at.tune_allowed()
            monkeypatch.setenv("PDT_DETERMINISTIC", "1")
            assert not at.tune_allowed()  # forcing lifts the world-size rule only
            monkeypatch.delenv("PDT_DETERMINISTIC")
            raise KeyError
    assert not at.tune_allowed()  # (left on an exception too)
    monkeypatch.setenv("WORLD_SIZE", "1")
    at.tuned()["stale"] = 1
    t = {"nt5:x": 4}
    at.adopt(t)
    assert at.tuned() == t and at.tuned() is not t and not at.tune_allowed()
    with at.forced_tuning():
        assert not at.tune_allowed()  # frozen wins


# ------------------------------------------------------------------ 7. key formats are frozen
def _ints(s):
    return [int(x) for x in s.split(",")]


def _rebuild(key):
    """The key the family's builder gives for the geometry parsed out of ``key``."""
    fam, _, rest = key.partition(":")
    if fam == "nt5":
        m = re.fullmatch(r"([\d,]+?)(?:,p(\d+))?(?:,a(\d+))?", rest)
        return at.nt_key(*_ints(m[1]), int(m[2] or 0), int(m[3] or 0))
    if fam == "ntb2":
        g = _ints(rest)
        return at.ntb_key(*g[:15], len(g) == 16 and g[15] == 2)
    if fam in ("wg2", "wgb"):
        m = re.fullmatch(r"([\d,]+?)(?:,p(\d+))?", rest)
        return at.wg_key(*_ints(m[1]), int(m[2] or 0), fam == "wgb")
    if fam == "axf":
        m = re.fullmatch(r"([\d,]+?)(?:,k(\d+)x(\d+)p(\d+))?", rest)
        return at.axf_key(*_ints(m[1]), *([int(m[2]), int(m[3]), int(m[4])] if m[2] else []))
    if fam in ("axb", "axd"):
        return at.axb_key(*_ints(rest), fam == "axd")
    if fam == "ax3":
        m = re.fullmatch(r"([\d,]+?)(?:,a([01])([01])m([01]))?", rest)
        return at.ax3_key(*_ints(m[1]), *([bool(int(m[i])) for i in (2, 3, 4)] if m[2] else []))
    if fam in ("stem1", "stem2w"):
        return at.stem_key(*_ints(rest), fam == "stem2w")
    if fam == "f8c":
        m = re.fullmatch(r"([\d,]+?)(,r)?(?:,q(\d)([01]))?(,cs)?", rest)
        return at.f8_key(*_ints(m[1]), bool(m[2]), (int(m[3]), int(m[4])) if m[3] else None, bool(m[5]))
    if fam == "wg8":
        return at.wg8_key(*_ints(rest))
    raise AssertionError(f"no key builder produces the family of {key!r}")


def _shipped():
    path = os.path.join(os.path.dirname(os.path.abspath(at.__file__)), os.pardir, "_lib", "autotune_gfx950.json")
    with open(path) as f:
        return json.load(f)


def test_every_shipped_key_is_what_its_builder_produces():
    table = _shipped()
    for key in table:
        assert _rebuild(key) == key
    fams = {k.partition(":")[0] for k in table}
    assert fams >= {"nt5", "ntb2", "wg2", "wgb", "axf", "axb", "axd", "ax3", "f8c", "wg8", "stem1", "stem2w"}
    # the optional suffixes are all exercised by real entries
    for pat in (r"nt5:.*,p4$", r"nt5:.*,a\d$", r"ntb2:.*,2$", r"wg2:.*,p4$", r"axf:.*,k3x3p1$", r"ax3:.*,a\d\dm\d$",
                r"f8c:.*,r$", r"f8c:.*,q\d\d$", r"f8c:.*,cs$"):
        assert any(re.match(pat, k) for k in table), pat


def test_key_builders_from_geometry():
    # spelled out once per family against real shipped entries: a builder change cannot hide behind the parser
    table = _shipped()
    keys = [
        at.nt_key(224, 224, 8, 1024, 112, 112, 64, 256, 2, 2, 8, 4, 1, True, False, 4),
        at.nt_key(1, 1, 768, 201728, 1, 1, 3072, 768, 1, 1, 1, 1, 1, False, False, 0, 3),
        at.ntb_key(14, 14, 256, 2048, 14, 14, 1024, 256, 1, 1, 1, 1, 1, True, True, True),
        at.wg_key(100352, 1024, 256, 14, 14, 256, 14, 14, 1, 1),
        at.wg_key(25690112, 64, 256, 224, 224, 8, 112, 112, 2, 4, 4, True),
        at.axf_key(14, 14, 1024, 2048, 256, True, False, True),
        at.axf_key(14, 14, 256, 2048, 256, False, False, True, 3, 3, 1),
        at.axb_key(14, 14, 1024, 2048, 256),
        at.axb_key(14, 14, 1024, 2048, 256, True),
        at.ax3_key(14, 14, 256, 2048, 256, 3, 3, 1),
        at.ax3_key(14, 14, 256, 2048, 1024, 1, 1, 0, True, True, True),
        at.stem_key(2048, 224, 224, 64),
        at.stem_key(2048, 224, 224, 64, True),
        at.f8_key(1024, 3072, 768, 0, 4, True),
        at.f8_key(1024, 768, 3072, 0, 0, True, True),
        at.f8_key(1024, 3072, 768, 1, 5, False, False, (1, 1), True),
        at.wg8_key(1024, 3072, 768),
    ]
    assert keys[0] == "nt5:224,224,8,1024,112,112,64,256,2,2,8,4,1,1,0,p4"
    assert keys[2] == "ntb2:14,14,256,2048,14,14,1024,256,1,1,1,1,1,1,1,2"
    assert keys[15] == "f8c:1024,3072,768,1,5,0,q11,cs"
    assert [k for k in keys if k not in table] == []
    assert at.nt_key(8, 8, 64, 2, 8, 8, 64, 64, 1, 1, 1, 1, 1, 0, 0, 4, 2) == \
        "nt5:8,8,64,2,8,8,64,64,1,1,1,1,1,0,0,p4,a2"
