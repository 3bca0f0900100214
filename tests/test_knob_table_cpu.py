"""The list of environment knobs is closed: every IAGO_* variable that iago_amd/ reads is a row of the LABNOTES.md table
"Tuning knobs" and is either a knob whose forms must give the same results -- then a named test holds that claim -- or
one that is listed here with the reason why no such claim applies.  A knob added without a test fails here, and so does
a misspelt variable name in one of the tests that set them (it would otherwise pass vacuously)."""
import glob
import os
import re

from tests.conftest import ROOT

# knob -> the test that holds "the same results under every value" (module path :: test)
RESULT_KNOBS = {
    "IAGO_LOOKAHEAD": "tests/test_mcts_gpu.py::test_policy_lookahead_builds_the_same_trees",            # lookahead=
    "IAGO_LOOKAHEAD_OVERLAP": "tests/test_mcts_gpu.py::test_policy_lookahead_builds_the_same_trees",    # lookahead_overlap=
    "IAGO_GRAPH_BLOCKS": "tests/test_knob_forms_gpu.py::test_graph_blocks_build_the_same_trees",
    "IAGO_FUSED_DESCENT": "tests/test_mcts_gpu.py::test_per_phase_descent_and_climbing_backup_build_the_same_trees",
    "IAGO_BACKUP_PATH": "tests/test_mcts_gpu.py::test_per_phase_descent_and_climbing_backup_build_the_same_trees",
    "IAGO_FUSED_LEAF_EVAL": "tests/test_knob_forms_gpu.py::test_split_leaf_evaluation_builds_the_same_trees",
    "IAGO_SIDE_PRIORITY": "tests/test_knob_forms_gpu.py::test_side_stream_priority_builds_the_same_trees",
    "IAGO_POLICY_SPLIT3": "tests/test_mcts_gpu.py::test_counted_kernels_equal_host_counted",             # SLPolicy.split3
    "IAGO_POLICY_PARTS": "tests/test_nets_shipped.py::test_slpolicy_one_launch_three_piece_split",       # split3_parts
    "IAGO_POLICY_GRID": "tests/test_knob_forms_gpu.py::test_setting_gives_the_default_results",
    "IAGO_VALUE_PERSIST": "tests/test_knob_forms_gpu.py::test_setting_gives_the_default_results",
    "IAGO_VALUE_TINY": "tests/test_knob_forms_gpu.py::test_setting_gives_the_default_results",
    "IAGO_TRUNK_STAGED": "tests/test_knob_forms_gpu.py::test_staged_trunk",
    "IAGO_PERSISTENT": "tests/test_search_persistent_gpu.py::test_trees_equal_the_per_playout_engine",  # persistent=
    "IAGO_PERSISTENT_GAMES": "tests/test_search_persistent_gpu.py::test_whole_games",
    "IAGO_SEARCH_SPLIT": "tests/test_split_default_sizes_gpu.py::test_a_equals_the_single_launch",       # split=
    "IAGO_GRAD_CHUNK_ROWS": "tests/test_policy_grad_gpu.py::test_rows_in_chunks_give_the_one_call_gradients",
    "IAGO_PERSISTENT_NET": "tests/test_search_persistent_gpu.py::test_scheduling_knobs_do_not_change_the_games",
    "IAGO_PERSISTENT_GPW": "tests/test_search_persistent_gpu.py::test_scheduling_knobs_do_not_change_the_games",
    "IAGO_PERSISTENT_PACE": "tests/test_search_persistent_gpu.py::test_scheduling_knobs_do_not_change_the_games",
    "IAGO_PERSISTENT_PACE_BACKLOG": "tests/test_search_persistent_gpu.py::test_scheduling_knobs_do_not_change_the_games",
    "IAGO_PERSISTENT_ROLL_DEFER": "tests/test_search_persistent_gpu.py::test_scheduling_knobs_do_not_change_the_games",
    "IAGO_PERSISTENT_PAIR": "tests/test_knob_forms_gpu.py::test_setting_gives_the_default_results",
    "IAGO_PERSISTENT_POLICY_XCDS": "tests/test_knob_forms_gpu.py::test_setting_gives_the_default_results",
    "IAGO_PERSISTENT_AHEAD": "tests/test_search_persistent_gpu.py::test_values_ahead_on_idle_net_workgroups",
    "IAGO_PERSISTENT_TABLE": "tests/test_position_table_gpu.py::test_b_trees_do_not_depend_on_the_tables_size",
    "IAGO_PERSISTENT_CUS": "tests/test_search_persistent_gpu.py::test_grid_follows_the_device",         # max_cus=
}

# knob -> why "the same results" is no claim about it
NOT_RESULT_KNOBS = {
    "IAGO_HIP_LIB": "path of the library to load: which build runs, not a form of it",
    "IAGO_PERSISTENT_LIMIT_MS": "clock limit after which a launch gives up: an error, never another result",
    "IAGO_PERSISTENT_GAME_LIMIT_MS": "the same clock limit for whole games",
    "IAGO_NATIVE_GRAD": "0 selects float32 autograd for the REINFORCE update: another arithmetic, compared at a tolerance "
                        "(tests/test_policy_grad_gpu.py::test_a_float32_model_takes_the_autograd_update)",
    "IAGO_ASYNC": "the game-asynchronous steps: fenced off as experimental, one smoke test "
                  "(tests/test_mcts_production_gpu.py::test_production_search_trees_bit_exact_vs_oracle)",
    "IAGO_ASYNC_PARTS": "experimental asynchronous steps (async_parts= in the same smoke tests)",
    "IAGO_ASYNC_NV": "experimental asynchronous steps: value workgroups per piece",
    "IAGO_VALUE_AHEAD": "the value look-ahead: fenced off as experimental, one smoke test "
                        "(tests/test_mcts_production_gpu.py::test_production_search_trees_bit_exact_vs_oracle)",
    "IAGO_VALUE_AHEAD_BOARDS": "experimental value look-ahead: boards per workgroup of a batch",
    "IAGO_VALUE_AHEAD_GRID": "experimental value look-ahead: workgroup cap of a batch",
}

NAME = r"IAGO_[A-Z0-9_]+"
READ = re.compile(r'(?:getenv\s*\(\s*|environ\.get\s*\(\s*|environ\s*\[\s*)"(%s)"' % NAME)


def read_by_the_code():
    names = set()
    for pattern in ("*.py", "csrc/*.hip", "csrc/*.hpp", "csrc/*.h"):
        for path in glob.glob(os.path.join(ROOT, "iago_amd", pattern)):
            with open(path) as f:
                names |= set(READ.findall(f.read()))
    return names


def in_the_table():
    with open(os.path.join(ROOT, "LABNOTES.md")) as f:
        text = f.read()
    head = text.index("### Tuning knobs")
    body = text[head:text.index("\n#", head + 4)]
    rows = [line for line in body.splitlines() if line.startswith("|")]
    assert len(rows) > 10
    return set(re.findall(NAME, "\n".join(rows)))


def test_every_knob_the_code_reads_is_in_the_table():
    code, table = read_by_the_code(), in_the_table()
    assert len(code) > 30                                          # (the search did find the reads)
    assert code == table, (sorted(code - table), sorted(table - code))


def test_every_knob_has_a_test_or_a_reason():
    code = read_by_the_code()
    assert not set(RESULT_KNOBS) & set(NOT_RESULT_KNOBS)
    listed = set(RESULT_KNOBS) | set(NOT_RESULT_KNOBS)
    assert code == listed, (sorted(code - listed), sorted(listed - code))
    assert all(reason.strip() for reason in NOT_RESULT_KNOBS.values())


def test_the_named_tests_exist():
    for knob, test_id in RESULT_KNOBS.items():
        path, name = test_id.split("::")
        with open(os.path.join(ROOT, path)) as f:
            assert re.search(r"^def %s\(" % re.escape(name), f.read(), re.M), (knob, test_id)


def test_the_knob_tests_spell_the_names_right():
    """Every IAGO_* name that the knob tests and their worker mention is one the code reads."""
    code = read_by_the_code()
    for name in ("test_knob_forms_gpu.py", "knob_worker.py"):
        with open(os.path.join(ROOT, "tests", name)) as f:
            used = set(re.findall(NAME, f.read()))
        assert used <= code, (name, sorted(used - code))
