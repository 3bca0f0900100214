"""The negamax backup rule (include/iago_hip_serving.h, IAGO_SEARCH_NEGAMAX; engine.BatchedMCTS(backup="negamax")) as a
replacement for oracle.mcts_py.Node.update_recursive.  TEST INFRASTRUCTURE ONLY.

A node's Q is the value from the view of the player who moved into it: the leaf's value (from the leaf mover's view) is
backed up as -leaf_value at the leaf, and its sign turns once per parent.  Node.update's arithmetic is untouched.

Every restatement the tests have -- oracle.mcts_py.MCTS, tests/wave_mcts.WaveMCTS (WaveNode is a Node),
tests/root_noise_ref.NoisyMCTS, tests/forced_ref.ForcedMCTS -- backs up through Node.update_recursive, so one rebinding
serves them all:

    with negamax_ref.rule():
        ... any of those searches ...

(restored when the block ends, however it ends)."""
import contextlib

from oracle import mcts_py


def update_recursive(self, leaf_value):
    node, value = self, -leaf_value
    while node is not None:
        node.update(value)
        node, value = node.parent, -value


@contextlib.contextmanager
def rule():
    """oracle.mcts_py.Node.update_recursive is the negamax rule inside the block."""
    reference = mcts_py.Node.update_recursive
    mcts_py.Node.update_recursive = update_recursive
    try:
        yield
    finally:
        mcts_py.Node.update_recursive = reference
