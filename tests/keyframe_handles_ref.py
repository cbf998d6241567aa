"""What the keyframe-handle tests share: the numpy restatement of the node directory of ccm_frame_set_bow and its cases.

Test infrastructure: nothing here is imported by the library."""
import numpy as np


def directory(node):
    """-> (order, nodes, first): a stable sort by (node, index) over node >= 0, the distinct nodes and their first positions"""
    node = np.asarray(node, "i4")
    idx = np.flatnonzero(node >= 0)
    order = idx[np.argsort(node[idx], kind="stable")].astype("i4")
    nodes, first = np.unique(node[order], return_index=True)
    return order, nodes.astype("i4"), np.concatenate([first, [len(order)]]).astype("i4")


def bow_cases():
    """Nodes that include -1, a single-feature node (3), a node of 130 features (7); a frame with every node -1."""
    rng = np.random.default_rng(11)
    mixed = np.concatenate([np.full(130, 7), [3], np.full(20, -1), rng.integers(10, 40, 200), np.full(64, 9)]).astype("i4")
    return [rng.permutation(mixed), np.full(50, -1, "i4")]
