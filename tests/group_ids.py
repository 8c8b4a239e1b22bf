"""The grouped pair numbering (needle_amd/csrc/pair_ids.h GroupView), restated with NumPy for the tests of the
grouped cross-matcher: groups are numbered in the order their first member appears in the list, base[g] = the pairs of the
groups before g, and pair (a, b) of group g with ranks (ra, rb) among the group's n members is
base[g] + ra (2 n - ra - 1) / 2 + (rb - ra - 1)."""
import numpy as np


def tables(labels):
    """(group_of, rank_of, size, base) of a list of labels."""
    labels = np.asarray(labels, dtype=np.uint64)
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    order = np.argsort(np.argsort(first))                                        # sorted-unique position -> order of first appearance
    group_of = order[inverse]
    size = np.bincount(group_of)
    rank_of = np.zeros(len(labels), dtype=np.int64)
    for g in range(len(size)):
        rank_of[group_of == g] = np.arange(size[g])
    base = np.concatenate([[0], np.cumsum(size * (size - 1) // 2)])
    return group_of, rank_of, size, base


def pair_id(labels, a, b, known=None):
    """The id of (a, b), a < b, of one group (`known`: tables(labels), where many ids are asked for)."""
    group_of, rank_of, size, base = known or tables(labels)
    g = group_of[a]
    assert a < b and group_of[b] == g, (a, b)
    n, ra, rb = int(size[g]), int(rank_of[a]), int(rank_of[b])
    return int(base[g]) + ra * (2 * n - ra - 1) // 2 + (rb - ra - 1)


def pairs(labels):
    """[(a, b)] by id: every same-label pair of the list."""
    labels = list(labels)
    known = tables(labels)
    out = {}
    for a in range(len(labels)):
        for b in range(a + 1, len(labels)):
            if labels[a] == labels[b]:
                out[pair_id(labels, a, b, known)] = (a, b)
    assert sorted(out) == list(range(len(out)))
    return [out[k] for k in range(len(out))]


def live_pairs(labels, residents):
    """{(a, b): id} of the same-label pairs with an arriving end (b >= residents)."""
    return {(a, b): k for k, (a, b) in enumerate(pairs(labels)) if b >= residents}
