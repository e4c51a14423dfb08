"""What the CPU and the GPU tests of the node2vec position features share: the configuration of the quality tests (the 512-node
planted-community case of tests/deepwalk_cases.py with biased walks, degree^0.75 negatives and a context table) and its pair lists from the
oracle, computed once.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import node2vec_oracle as nvo
from deepwalk_cases import clustered_case, step_seeds

# the bar comes from the fp64 oracle on the CPU (tests/test_node2vec_cpu.py: 0.994 to 0.996 for the init seeds 0-3, all >= 0.97)
QUALITY = dict(p=0.5, q=2.0, power=0.75, bar=0.95)
_LISTS = []


def quality_lists():
    """(indptr, indices, labels, cfg, [(start, rest) per step]): all 512 nodes the roots of one batch per step, the seeds of step_seeds."""
    if not _LISTS:
        indptr, indices, labels, c = clustered_case()
        cdf = nvo.negative_cdf(indptr, indices, QUALITY["power"])
        roots = np.arange(512)
        lists = []
        for s in range(c["steps"]):
            walk_seed, neg_seed = step_seeds(s)
            walks = nvo.node2vec_walk(indptr, indices, roots, c["length"], QUALITY["p"], QUALITY["q"], walk_seed)
            lists.append(nvo.pairs_from_walks(walks, 512, c["context"], c["negatives"], neg_seed, cdf))
        _LISTS.append((indptr, indices, labels, c, lists))
    return _LISTS[0]
