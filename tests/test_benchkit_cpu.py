"""CPU: tools/benchkit.py, the recipe every bench tool times with.  The order of events of its timed loop is a contract
(its docstring states it); here a fake event factory and fake callables append to one log, and the log is held against that
order, with and without a sweep.  Also the record helpers: stats, write, progress.  No GPU and no torch device."""
import json
import os
import statistics
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

import benchkit  # noqa: E402

NAMES = ("a", "b", "c")
WARMUP, REPS = 2, 3


class Fakes:
    """events and callables that write to one log; the k-th event pair (from 0) measures 1.5 + k ms"""

    def __init__(self):
        self.log, self.made = [], 0

    def event(self):
        fakes, k = self, self.made
        self.made += 1

        class Event:
            def record(self):
                fakes.log.append(("record", k))

            def synchronize(self):
                fakes.log.append(("synchronize", k))

            def elapsed_time(self, other):
                fakes.log.append(("elapsed_time", k, other.k))
                return 1.5 + k // 2

        Event.k = k
        return Event()

    def fn(self, name):
        return lambda: self.log.append(("fn", name))

    def sync(self):
        self.log.append(("sync",))

    def sweep(self):
        self.log.append(("sweep",))


def expected_log(with_sweep):
    log = [("fn", n) for _ in range(WARMUP) for n in NAMES] + [("sync",)]
    k = 0
    for _ in range(REPS):
        for n in NAMES:
            log += ([("sweep",)] if with_sweep else []) + [("record", k), ("fn", n), ("record", k + 1), ("synchronize", k + 1),
                                                           ("elapsed_time", k, k + 1)]
            k += 2
    return log + [("sync",)]


@pytest.mark.parametrize("with_sweep", [True, False])
def test_timed_keeps_the_order_of_events(with_sweep):
    f = Fakes()
    med, times = benchkit.timed([(n, f.fn(n)) for n in NAMES], REPS, WARMUP, f.sync, f.sweep if with_sweep else None, event=f.event)
    assert f.log == expected_log(with_sweep)
    # variant i of round r took event pair 3 r + i, which measured 1.5 + 3 r + i
    want = {n: [1.5 + 3 * r + i for r in range(REPS)] for i, n in enumerate(NAMES)}
    assert times == want and list(times) == list(NAMES)
    assert all(len(v) == REPS for v in times.values())
    assert med == {n: statistics.median(v) for n, v in want.items()} == {"a": 4.5, "b": 5.5, "c": 6.5}


def test_timed_takes_any_iterable_of_variants_once():
    f = Fakes()
    med, _ = benchkit.timed({n: f.fn(n) for n in NAMES}.items(), 1, 0, f.sync, event=f.event)
    assert list(med) == list(NAMES) and f.log[0] == ("sync",) and f.log[-1] == ("sync",)


def test_stats_rounds_to_four_places():
    s = benchkit.stats({"x": [1.00004, 2.00005001, 3.99996], "y": [0.123449, 0.5]})
    assert s == {"median_ms": {"x": 2.0001, "y": 0.3117}, "min_ms": {"x": 1.0, "y": 0.1234}, "max_ms": {"x": 4.0, "y": 0.5}}
    assert list(s) == ["median_ms", "min_ms", "max_ms"]


def test_write_prints_and_keeps_the_document(tmp_path, capsys):
    doc = {"device": "none", "runs": [{"median_ms": {"a": 1.5}}]}
    out = tmp_path / "made" / "here" / "doc.json"
    benchkit.write(doc, str(out))
    printed = capsys.readouterr().out
    text = out.read_text()
    assert text.endswith("}\n") and printed == text  # print adds the newline the file ends with
    assert printed[:-1] == text[:-1] == json.dumps(doc, indent=1)
    assert json.loads(text) == doc


def test_write_without_out_writes_no_file(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    benchkit.write({"a": 1}, None)
    assert json.loads(capsys.readouterr().out) == {"a": 1}
    assert list(tmp_path.iterdir()) == []


def test_save_is_the_file_half_of_write(tmp_path, capsys):
    out = tmp_path / "rows" / "doc.json"
    benchkit.save({"runs": [1]}, str(out))
    assert capsys.readouterr().out == "" and out.read_text() == json.dumps({"runs": [1]}, indent=1) + "\n"


def test_progress_is_one_json_line_on_stderr(capsys):
    benchkit.progress({"rows": 64, "median_ms": {"gather": 0.1}})
    got = capsys.readouterr()
    assert got.out == "" and got.err.endswith("\n") and got.err.count("\n") == 1
    assert json.loads(got.err) == {"rows": 64, "median_ms": {"gather": 0.1}}


def test_ok_passes_zero_and_nothing_else():
    assert benchkit.ok(0) is None
    with pytest.raises(AssertionError):
        benchkit.ok(5)
