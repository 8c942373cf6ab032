"""The poison helper and the recipe table of tests/test_gpu_poison.py, without a GPU: the patterns are the stated bits, the
context manager restores torch.empty, and every C entry point that works on a handle is reached by some recipe."""
import os
import re

import numpy as np
import pytest
import torch

from trajectory_optimization_matrix_lie_groups_amd import _capi
from tests.poison import MINUS, ONE, PATTERNS, ZERO, poisoned
from tests.poison_recipes import EXEMPT, NAMES, RECIPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES = {ZERO: [0, 0, 0, 0], MINUS: [255, 255, 255, 255], ONE: [1, 0, 0, 0]}


@pytest.mark.parametrize("pattern", PATTERNS)
def test_each_pattern_fills_the_stated_bits(pattern):
    with poisoned(pattern, fill_cpu=True):
        d, i, u = torch.empty(3, 5, dtype=torch.float64), torch.empty(7, dtype=torch.int32), torch.empty(13, dtype=torch.uint8)
        s = torch.empty((), dtype=torch.float64)
    assert u.tolist() == (BYTES[pattern] * 4)[:13]
    assert i.tolist() == [{ZERO: 0, MINUS: -1, ONE: 1}[pattern]] * 7
    bits = d.view(torch.int64)
    want = {ZERO: 0, MINUS: -1, ONE: 0x0000000100000001}[pattern]
    assert (bits == want).all() and int(s.view(torch.int64)) == want
    if pattern == ZERO:
        assert (d == 0.0).all() and not torch.signbit(d).any()
    elif pattern == MINUS:
        assert torch.isnan(d).all()
    else:
        assert torch.isfinite(d).all() and (d != 0.0).all() and (d.abs() < np.finfo(np.float64).tiny).all()


def test_cpu_tensors_pass_through_by_default_and_unknown_patterns_are_refused(monkeypatch):
    from tests import poison
    filled = []
    monkeypatch.setattr(poison, "fill", lambda t, pattern: filled.append((tuple(t.shape), pattern)) or t)
    original = torch.empty
    with poisoned(MINUS):
        t = torch.empty(4, dtype=torch.float64)
        assert torch.empty is not original
    assert t.shape == (4,) and t.dtype == torch.float64 and filled == []   # a CPU tensor is returned as torch.empty made it
    with poisoned(MINUS, fill_cpu=True):
        torch.empty(2, 3, dtype=torch.int32)
    assert filled == [((2, 3), MINUS)]
    for bad in ("0x7F", "0xA5", "STALE", None):
        with pytest.raises(ValueError):
            with poisoned(bad):
                pass
    assert torch.empty is original
    assert PATTERNS == (ZERO, MINUS, ONE)


def test_torch_empty_is_restored_after_the_context_and_after_an_exception():
    original = torch.empty
    with poisoned(ONE, fill_cpu=True):
        assert torch.empty is not original
        with poisoned(ZERO, fill_cpu=True):  # nested: the inner one restores the outer replacement
            assert int(torch.empty(1, dtype=torch.int32)) == 0
        assert int(torch.empty(1, dtype=torch.int32)) == 1
    assert torch.empty is original
    with pytest.raises(RuntimeError, match="inside"):
        with poisoned(MINUS, fill_cpu=True):
            raise RuntimeError("inside")
    assert torch.empty is original


def test_recipe_names_are_unique():
    assert len(NAMES) == len(set(NAMES)) == len(RECIPES) > 0
    assert all(re.fullmatch(r"[A-Za-z0-9_]+", n) for n in NAMES)  # ("/" separates recipe and tensor in the child's .npz)
    assert all(fn.__doc__ for fn in RECIPES)


def _entry_points_on_a_handle():
    """The symbols of include/tolg.h (the list tests/test_capi_symbols.py holds against the library: _capi.SYMBOLS) whose
    declaration takes a tolg_handle_t as its first parameter."""
    hdr = open(os.path.join(ROOT, "include", "tolg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tolg_[a-z_]+)\s*\(", hdr)))
    assert declared == sorted(_capi.SYMBOLS)   # tests/test_capi_symbols.py's assertion: the binding's list is the header's
    return [n for n in declared if re.search(r"\b%s\s*\(\s*tolg_handle_t\b" % n, hdr)]


def test_every_entry_point_on_a_handle_is_reached_by_a_recipe():
    on_handle = _entry_points_on_a_handle()
    assert len(on_handle) >= 40 and "tolg_solve_begin" in on_handle and "tolg_version" not in on_handle
    assert set(EXEMPT) <= set(_capi.SYMBOLS)   # an exemption that names nothing is stale
    reached = set()
    for fn in RECIPES:
        assert set(fn.reaches) <= set(_capi.SYMBOLS), (fn.name, set(fn.reaches) - set(_capi.SYMBOLS))
        reached |= set(fn.reaches)
    assert not reached & set(EXEMPT)
    missing = [n for n in on_handle if n not in reached and n not in EXEMPT]
    assert not missing, "no recipe of tests/poison_recipes.py reaches %s" % missing
    assert "tolg_create" in reached
