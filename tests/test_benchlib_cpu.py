"""tools/_benchlib.py, the parts with no GPU in them: the alternation order, the statistics of a row and the line table."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_benchlib", os.path.join(ROOT, "tools", "_benchlib.py"))
benchlib = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(benchlib)


def test_rotated_is_a_rotation_and_every_element_leads_equally_often():
    for seq in (("a", "b", "c"), ["x"], [(1, "s"), (2, "s"), "rollout", 4]):
        n = len(seq)
        leads = []
        for r in range(2 * n + 1):
            got = benchlib.rotated(seq, r)
            assert type(got) is type(seq) and len(got) == n
            k = r % n
            assert list(got) == list(seq[k:]) + list(seq[:k])
            leads.append(got[0])
        assert list(benchlib.rotated(seq, 0)) == list(seq)
        for x in seq:  # rounds 0 .. 2n - 1: every element leads exactly twice
            assert leads[:2 * n].count(x) == 2


def test_summary():
    rates = [3.0, 1.0, 2.0]
    s = benchlib.summary(rates)
    assert s == dict(median=2.0, min=1.0, max=3.0, spread=1.0, runs=[3.0, 1.0, 2.0])
    assert list(s) == ["median", "min", "max", "spread", "runs"]


def test_stats_row():
    assert benchlib.stats_row([3.0, 1.0, 2.0]) == dict(ms_median=2.0, ms_min=1.0, ms_max=3.0)
    row = benchlib.stats_row([4.0, 8.0], "ms_per_step")
    assert row == dict(ms_per_step_median=6.0, ms_per_step_min=4.0, ms_per_step_max=8.0)
    assert list(row) == ["ms_per_step_median", "ms_per_step_min", "ms_per_step_max"]


def test_lines():
    assert set(benchlib.LINES) == {"headline", "merit", "ss"}
    assert {k: v[1] for k, v in benchlib.LINES.items()} == dict(headline=300, merit=100, ss=60)
    for kw, _ in benchlib.LINES.values():
        assert set(kw) == {"mode", "line_search", "schedule"}
