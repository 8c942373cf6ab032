"""tools/symbol_diff.py, the pairing of two builds' symbols by name: with a rename, with a symbol one side lacks, without one."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("symbol_diff", os.path.join(ROOT, "tools", "symbol_diff.py"))
symbol_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(symbol_diff)

_ROLL = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_add_f64 v[0:1], v[2:3], v[4:5]", "s_endpgm"]
_STEP = ["v_mov_b32_e32 v0, s2", "s_cbranch_scc1 12", "s_endpgm"]
_STEP_MOVED = ["v_mov_b32_e32 v7, s3", "s_cbranch_scc1 14", "s_endpgm"]  # other registers, another jump distance
OLD = {"tolg::k_policy_rollout<4, 0, 0, 0>": _ROLL, "tolg::k_policy_rollout_lim<4, 0, 0, 0>": _ROLL,
       "tolg::k_policy_rollout_lim<6, 1, 0, 2, tolg::PlantArg>": _STEP, "tolg::k_gone<4>": _ROLL}
NEW = {"tolg::k_policy_rollout<4, 0, 0, 0>": _ROLL, "tolg::k_policy_rollout<4, 0, 0, 0, tolg::PolicyLim>": _ROLL,
       "tolg::k_policy_rollout<6, 1, 0, 2, tolg::PolicyLim, tolg::PlantArg>": _STEP_MOVED}
RENAME = (r"k_policy_rollout_lim<(\d+, \d+, \d+, \d+)", r"k_policy_rollout<\1, tolg::PolicyLim")


def _classes(rows):
    return {name: c for name, c, _, _ in rows}


def test_a_renamed_pair_is_compared_under_its_new_name():
    rows = symbol_diff.pair(OLD, NEW, [RENAME])
    assert [r[0] for r in rows] == sorted(set(NEW) | {"tolg::k_gone<4>"})
    got = _classes(rows)
    assert got["tolg::k_policy_rollout<4, 0, 0, 0, tolg::PolicyLim>"] == "identical"
    assert got["tolg::k_policy_rollout<4, 0, 0, 0>"] == "identical"
    # registers and the jump distance moved, the operations did not
    assert got["tolg::k_policy_rollout<6, 1, 0, 2, tolg::PolicyLim, tolg::PlantArg>"] == "same instructions"
    by = {r[0]: r for r in rows}
    assert by["tolg::k_policy_rollout<4, 0, 0, 0, tolg::PolicyLim>"][2:] == (_ROLL, _ROLL)


def test_a_symbol_of_one_side_only_is_different():
    rows = symbol_diff.pair(OLD, NEW, [RENAME])
    assert ("tolg::k_gone<4>", "different", _ROLL, None) in rows
    rows = symbol_diff.pair(NEW, OLD, [])
    assert ("tolg::k_gone<4>", "different", None, _ROLL) in rows


def test_without_a_rename_names_pair_as_they_are():
    assert symbol_diff.pair(OLD, NEW) == symbol_diff.pair(OLD, NEW, [])
    got = _classes(symbol_diff.pair(OLD, NEW))
    assert got == {"tolg::k_policy_rollout<4, 0, 0, 0>": "identical",
                   "tolg::k_policy_rollout_lim<4, 0, 0, 0>": "different",
                   "tolg::k_policy_rollout_lim<6, 1, 0, 2, tolg::PlantArg>": "different",
                   "tolg::k_policy_rollout<4, 0, 0, 0, tolg::PolicyLim>": "different",
                   "tolg::k_policy_rollout<6, 1, 0, 2, tolg::PolicyLim, tolg::PlantArg>": "different",
                   "tolg::k_gone<4>": "different"}
    assert OLD["tolg::k_policy_rollout_lim<4, 0, 0, 0>"] is _ROLL  # the inputs are left as they were
