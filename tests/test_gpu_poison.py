"""Poisoned-memory parity: no result may depend on memory the library did not write.

Every recipe of tests/poison_recipes.py builds its handle and makes its calls with torch.empty replaced (tests/poison.py): the
workspace, the packed buffers of the setters, the loop's own state tensors and every output are born filled with one of three
patterns -- every int 0 and every double +0.0 (ZERO), every int -1 and every double a NaN (MINUS), every int 1 and every double
a non-zero denormal (ONE).

1. every element of every tensor a recipe returns has the same bytes under all three patterns (integer views: a NaN must match
   a NaN of the same bits).  No element is masked: the recipes' perturbations keep every sample of the sampled loops finite, so
   every element of every output is one the library has to write;
2. the MINUS run also passes the oracle or restatement check the suite applies to that call (recipe.oracle), which rules out
   three runs that agree on the same wrong answer;
3. the whole table once more in one child process with TOLG_POISON_LDS=1 (every launch followed by a kernel that fills the LDS
   of every CU with NaNs) under ZERO, bitwise this process's ZERO run: what differs there was read from LDS before it was
   written."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

from tests.poison import MINUS, ONE, ZERO
from tests.poison_recipes import RECIPES, as_bits, make_solver, run_recipe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_zero_runs = {}  # recipe name -> the bits of its ZERO run, shared with the LDS test


def _zero_run(fn):
    if fn.name not in _zero_runs:
        _zero_runs[fn.name] = as_bits(run_recipe(fn, ZERO))
    return _zero_runs[fn.name]


def _differences(a, b):
    """[(tensor, number of elements whose bits differ, the first index)] between two runs' bits"""
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    out = []
    for k in sorted(a):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        d = a[k] != b[k]
        if d.any():
            out.append((k, int(d.sum()), tuple(int(i) for i in np.argwhere(d)[0])))
    return out


@pytest.mark.parametrize("fn", RECIPES, ids=[r.name for r in RECIPES])
def test_results_do_not_depend_on_uninitialised_memory(fn):
    zero = _zero_run(fn)
    assert zero, "the recipe returned no tensor"
    minus_out = run_recipe(fn, MINUS)
    minus = as_bits(minus_out)
    one = as_bits(run_recipe(fn, ONE))
    bad = {"MINUS": _differences(zero, minus), "ONE": _differences(zero, one)}
    assert not any(bad.values()), "%s differs from its ZERO run: %s" % (fn.name, bad)
    if fn.oracle is not None:
        from tests.poison import poisoned
        with poisoned(MINUS):
            fn.oracle(make_solver, minus_out)


def test_the_table_under_poisoned_lds():
    """TOLG_POISON_LDS is read once per process: every recipe in one child process with the variable set, under ZERO, gives
    the bits of this process's ZERO runs."""
    with tempfile.TemporaryDirectory() as d:
        child = os.path.join(d, "child.npz")
        env = dict(os.environ, TOLG_POISON_LDS="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        code = "from tests.poison_recipes import run_table_to_npz as f; f(%r, %r)" % (child, ZERO)
        flags = ["-s"] if sys.flags.no_user_site else []
        t0 = time.time()
        out = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        print("the child under TOLG_POISON_LDS=1 took %.1f s" % (time.time() - t0))
        assert out.returncode == 0, out.stderr[-2000:]
        got = dict(np.load(child))
    bad = {}
    for fn in RECIPES:
        here = _zero_run(fn)
        there = {k[len(fn.name) + 1:]: v for k, v in got.items() if k.startswith(fn.name + "/")}
        diff = _differences(here, there)
        if diff:
            bad[fn.name] = diff
    assert not bad, "differs under poisoned LDS: %s" % bad
