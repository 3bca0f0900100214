"""BatchedMCTS's split= / IAGO_SEARCH_SPLIT: "auto", 0 or a positive multiple of 8 game CUs; anything else is refused
before anything is allocated (a value that can never split used to be taken silently as the single launch)."""
import pytest

from iago_amd import engine


@pytest.mark.parametrize("bad", [True, False, 1, 12, -8, 1.0, "x", "12", ""])
def test_split_values_that_cannot_split_are_refused(bad):
    with pytest.raises(ValueError, match="multiple of 8"):
        engine.BatchedMCTS(2048, None, None, None, split=bad)


@pytest.mark.parametrize("bad", ["12", "-8", "x", "True"])
def test_the_environment_variable_is_checked_too(bad, monkeypatch):
    monkeypatch.setenv("IAGO_SEARCH_SPLIT", bad)
    with pytest.raises(ValueError, match="IAGO_SEARCH_SPLIT"):
        engine.BatchedMCTS(2048, None, None, None)


@pytest.mark.parametrize("good,want", [("auto", "auto"), (0, 0), (8, 8), (32, 32), ("0", 0), ("64", 64)])
def test_split_values_taken(good, want):
    assert engine._split_arg(good) == want
