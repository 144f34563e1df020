"""util.linearise on toy lists (no GPU): the serial orders tests/tools/step_schedules.py runs the train step's stream
lists in.  Launches are plain strings here; the helper only looks at ("wait" / "record", event) items."""
import itertools

import pytest

from util import linearise


def test_events_order_producer_and_consumer_under_every_priority():
    a = ["a1", ("record", "e"), "a2"]
    b = [("wait", "inputs"), "b0", ("wait", "e"), "b1"]
    for perm in itertools.permutations(range(2)):
        order = linearise((a, b), perm)
        assert sorted(order) == ["a1", "a2", "b0", "b1"]
        assert order.index("a1") < order.index("b1"), perm
    # the higher list overtakes the moment its event exists: item by item, not list by list
    assert linearise((a, b), (1, 0)) == ["b0", "a1", "b1", "a2"]
    assert linearise((a, b), (0, 1)) == ["a1", "a2", "b0", "b1"]


def test_missing_wait_lets_some_priority_run_the_consumer_first():
    a = ["a1", ("record", "e"), "a2"]
    b = ["b0", "b1"]                                   # b1 reads what a1 writes, and says so nowhere
    firsts = {perm: (lambda o: o.index("b1") < o.index("a1"))(linearise((a, b), perm))
              for perm in itertools.permutations(range(2))}
    assert firsts == {(0, 1): False, (1, 0): True}


def test_allreduce_items_stay_and_three_lists_interleave():
    a = ["a1", ("record", "x"), ("wait", "z"), "a2"]
    b = [("wait", "x"), "b1", ("allreduce", "d"), ("record", "y")]
    c = [("wait", "y"), "c1", ("record", "z")]
    for perm in itertools.permutations(range(3)):
        assert linearise((a, b, c), perm) == ["a1", "b1", ("allreduce", "d"), "c1", "a2"], perm


def test_cyclic_wait_is_reported_as_a_deadlock():
    a = [("wait", "y"), "a1", ("record", "x")]
    b = [("wait", "x"), "b1", ("record", "y")]
    with pytest.raises(AssertionError, match="deadlocked"):
        linearise((a, b), (0, 1))
    with pytest.raises(AssertionError):                # a priority order names every list once
        linearise((a, b), (0, 0))
