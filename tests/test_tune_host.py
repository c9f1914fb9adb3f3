"""The autotuner's decisions on the host (crdr_amd/hip/tune.py): nothing in them needs a GPU once the timer is a seam.

`tune.time_call` is replaced by a function that calls fn() once and returns a time from a table keyed by the id `run` last received; `run(a)`
copies a prepared CPU tensor into `out`.  The keys start with "host": the F(4x4) agreement window of conv keys ("c" / "g" / "m") is not in
play.  Every test runs on the module's real state and puts back what it touched (the containers in place: ops aliases them).
"""
import json
import math

import pytest
import torch

from crdr_amd.hip import lib as L
from crdr_amd.hip import tune

BASE = [1.0, -2.0, 3.0, 0.5]
TIMES = {0: 5.0, 1: 3.0, 2: 1.0, 3: 0.5, 257: 4.0}   # ms per id; every other id: 10


@pytest.fixture
def tuner():
    """the module's state as it was, and a Trial factory on the fake timer"""
    keep = (dict(tune.algo_cache), list(tune.LOG), list(tune.REJECTED), list(tune.SKIPPED), dict(tune._zero_seen), tune.time_call)
    yield Trial
    for live, old in zip((tune.algo_cache, tune.LOG, tune.REJECTED, tune.SKIPPED, tune._zero_seen), keep):
        live.clear()
        live.update(old) if isinstance(live, dict) else live.extend(old)
    tune.time_call = keep[5]


class Trial:
    """run / result / reset / penalty of one tuning attempt, with the fake timer installed and every call recorded in `events`"""

    def __init__(self, outputs=None, refuse=(), throw=(), penalties=None):
        self.out = torch.zeros(4)
        self.outputs = {k: torch.tensor(v) for k, v in (outputs or {}).items()}
        self.refuse, self.throw, self.penalties = refuse, throw, penalties or {}
        self.last, self.events = None, []
        tune.time_call = self.time_call

    def time_call(self, fn, reps=2):
        fn()
        return TIMES.get(self.last, 10.0)

    def run(self, a):
        self.last = a
        self.events.append(("run", a))
        if a in self.throw:
            raise L.CrdrHipError("refused")
        if a in self.refuse:
            return False
        self.out.copy_(self.outputs.get(a, self.outputs.get(0, torch.tensor(BASE))))
        return True

    def result(self):
        return self.out

    def reset(self):
        self.events.append("reset")

    def penalty(self):
        return self.penalties.get(self.last, 0.0)


def test_selection_takes_the_fastest_candidate_that_agrees(tuner):
    key = ("host", "selection")
    off, nan = list(BASE), list(BASE)
    off[2] += 1e-3            # 3.3e-4 of the scale (3.0): above the default agree of 2e-5
    nan[0] = float("nan")
    t = tuner({2: off, 3: nan})
    log0, rej0 = len(tune.LOG), len(tune.REJECTED)
    assert tune.autotune(key, 3, 1, t.run, result=t.result) == 1   # ids 1, 257, 2, 258, 3, 259: 3 and 2 are faster, but wrong
    rej = tune.REJECTED[rej0:]
    assert [(k, a) for k, a, _ in rej] == [(key, 2), (key, 3)]
    assert rej[0][2] == pytest.approx(1e-3 / 3.0, rel=1e-3) and math.isnan(rej[1][2])
    assert tune.LOG[log0:] == [(key, 1, 5.0, 3.0)]
    assert tune.algo_cache[key] == 1


def test_penalty_is_charged_to_the_candidate_just_timed(tuner):
    t = tuner(penalties={1: 3.0})
    assert tune.autotune(("host", "penalty"), 2, 0, t.run, result=t.result, penalty=t.penalty) == 2
    t = tuner(penalties={2: 3.0})   # 1 ms + 3 ms: now behind id 1's 3 ms
    assert tune.autotune(("host", "penalty", 2), 2, 0, t.run, result=t.result, penalty=t.penalty) == 1


def test_refused_and_failing_candidates_are_passed_over(tuner):
    t = tuner(refuse=(1,), throw=(2,))
    assert tune.autotune(("host", "refusals"), 3, 0, t.run, result=t.result) == 3


def test_zero_result_defers_the_tuning_three_times(tuner):
    key = ("host", "zero")
    t = tuner({0: [0.0] * 4})
    log0, skip0 = len(tune.LOG), len(tune.SKIPPED)
    for call in (1, 2):
        assert tune.autotune(key, 3, 0, t.run, result=t.result) == 0
        assert key not in tune.algo_cache and len(tune.SKIPPED) == skip0 + call
    assert tune.autotune(key, 3, 0, t.run, result=t.result) == 0
    assert tune.algo_cache[key] == 0 and len(tune.SKIPPED) == skip0 + 3
    assert tune.LOG[log0:] == [(key, 0, 0.0, 0.0)]
    assert all(e == ("run", 0) for e in t.events), "no candidate runs against an all-zero baseline"


def test_reset_comes_before_every_compared_run(tuner):
    t = tuner()
    assert tune.autotune(("host", "reset"), 2, 0, t.run, result=t.result, reset=t.reset) == 2
    # per id: reset, the run whose result is compared, the timed run (the fake timer calls it once)
    assert t.events == [e for a in (0, 1, 2) for e in ("reset", ("run", a), ("run", a))]


def test_database_round_trip_and_filters(tuner, tmp_path):
    entries = {("c", 1, 2): 3, ("g", 4): 257, ("w", 5, (3, 3)): 7, ("wm", 6): 0}
    path = str(tmp_path / "db.json")
    tune.algo_cache.clear()
    tune.algo_cache.update(entries)
    tune.save(path)
    tune.algo_cache.clear()
    assert tune.load(path) == 4 and tune.algo_cache == entries
    assert tune.load(str(tmp_path / "missing.json")) == 0

    tune.algo_cache.clear()
    assert tune.load(path, only_kinds=("w", "wm")) == 2 and set(tune.algo_cache) == {("w", 5, (3, 3)), ("wm", 6)}
    tune.algo_cache.clear()
    assert tune.load(path, skip=lambda k: (3, 3) in k) == 3 and ("w", 5, (3, 3)) not in tune.algo_cache

    tune.algo_cache.clear()
    tune.algo_cache[("g", 4)] = 9   # an entry already in the cache is not overwritten (it still counts as loaded)
    assert tune.load(path) == 4 and tune.algo_cache[("g", 4)] == 9 and tune.algo_cache[("c", 1, 2)] == 3

    foreign = str(tmp_path / "foreign.json")
    with open(path) as f:
        db = json.load(f)
    assert db["signature"] == tune.signature()
    db["signature"] = "another-build"
    with open(foreign, "w") as f:
        json.dump(db, f)
    tune.algo_cache.clear()
    tune.algo_cache[("x",)] = 1
    assert tune.load(foreign) == 0 and tune.algo_cache == {("x",): 1}
    assert tune.load(foreign, ignore_signature=True) == 4 and len(tune.algo_cache) == 5


def test_shipped_database_loads_whole(tuner):
    with open(tune.DEFAULT_DB) as f:
        db = json.load(f)
    tune.algo_cache.clear()
    assert tune.load(tune.DEFAULT_DB) == len(db["algos"]) == len(tune.algo_cache)


def test_ops_keeps_the_names_the_benchmark_reads():
    from crdr_amd.hip import ops
    assert ops._algo_cache is tune.algo_cache and ops.TUNE_LOG is tune.LOG and ops.TUNE_REJECTED is tune.REJECTED
    assert ops.load_tune_cache is tune.load and ops.save_tune_cache is tune.save and ops.DEFAULT_TUNE_DB is tune.DEFAULT_DB
