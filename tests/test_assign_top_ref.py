"""The candidate list's brute force (tests/assign_top_ref.py) against the record's (tests/assign_ref.py) where the contract ties them
together: slot 0 is the record, slot 1's score is second_score, count is min(K, accepting targets), K = 1 is the old record.  Random
accepted lists with forced ties: equal scores across targets, and both strands of one target with equal and with different scores."""
import numpy as np
import pytest

import assign_ref
import assign_top_ref


def random_accepted(rng, n_reads, n_targets):
    """scores from a small set, so that ties across targets and across the strands of one target are everywhere"""
    scores = np.array([0.25, 1.0 / 3.0, 0.5, 0.5 + 2.0 ** -53, 0.75])
    acc = []
    for r in range(n_reads):
        if r % 7 == 0:
            continue                                                # reads nothing accepts
        for t in rng.choice(n_targets, int(rng.integers(1, n_targets + 1)), replace=False):
            for st in ((0,), (1,), (0, 1))[int(rng.integers(0, 3))]:
                acc.append((r, int(t), st, float(scores[rng.integers(0, len(scores))]), int(rng.integers(1, 999)), int(rng.integers(1, 999)),
                            int(rng.integers(100, 999)), float(rng.random())))
    return [acc[i] for i in rng.permutation(len(acc))]


@pytest.mark.parametrize("seed", range(4))
def test_slots_0_and_1_are_the_record(seed):
    rng = np.random.default_rng(seed)
    n = 60
    acc = random_accepted(rng, n, 11)
    rec = assign_ref.reduce_best(n, acc)
    nt = assign_top_ref.n_targets(n, acc)
    assert (nt == 0).sum() >= 5 and (nt == 1).sum() >= 1 and (nt > 8).sum() >= 5
    for K in range(1, 9):
        c = assign_top_ref.reduce_top(n, acc, K)
        assert (c["count"] == np.minimum(K, nt)).all()
        for f, t in assign_top_ref.FIELDS:
            g, w = c[f][:, 0], rec[f]
            assert (g.view(np.uint64) == w.view(np.uint64)).all() if t is np.float64 else (g == w).all(), (K, f)
        if K >= 2:
            assert (c["score"][:, 1].view(np.uint64) == rec["second_score"].view(np.uint64)).all()
        # the slots of a smaller K are the first slots of a larger one; unused slots as the library makes them
        full = assign_top_ref.reduce_top(n, acc, 8)
        cut = {f: full[f][:, :K].copy() for f, _ in assign_top_ref.FIELDS}
        cut["count"] = np.minimum(full["count"], K).astype(np.uint32)
        assert not assign_top_ref.same(c, cut)
        for r in range(n):
            j = int(c["count"][r])
            assert (c["target"][r, j:] == -1).all() and (c["score"][r, j:] == -1.0).all() and (c["bases"][r, j:] == 0).all()
            assert len(set(c["target"][r, :j])) == j                                    # one candidate per target
            key = [(-c["score"][r, i], c["target"][r, i]) for i in range(j)]
            assert key == sorted(key)


def test_a_case_worked_out_by_hand():
    """read 0: (0,+,0.5) (1,+,0.75) (1,-,0.75) (2,-,0.75) (3,+,0.6) (3,-,0.7) -> 1 forward (the strands tie), 2 reverse (the targets tie:
    the lower index first), 3 REVERSE (its better strand) at 0.7, 0 forward; read 1: nothing; read 2: (4,-,0.3) alone."""
    acc = [(0, 0, 0, 0.5, 50, 40, 100, 1.5), (0, 1, 0, 0.75, 75, 60, 100, 2.5), (0, 1, 1, 0.75, 75, 61, 100, 3.5), (0, 2, 1, 0.75, 75, 62, 100, 4.5),
           (0, 3, 0, 0.6, 60, 50, 100, 5.5), (0, 3, 1, 0.7, 70, 51, 100, 6.5), (2, 4, 1, 0.3, 30, 20, 100, 7.5)]
    c = assign_top_ref.reduce_top(3, acc[::-1], 3)
    assert c["count"].tolist() == [3, 0, 1]
    assert c["target"].tolist() == [[1, 2, 3], [-1, -1, -1], [4, -1, -1]]
    assert c["rev"].tolist() == [[0, 1, 1], [0, 0, 0], [1, 0, 0]]
    assert c["score"].tolist() == [[0.75, 0.75, 0.7], [-1.0, -1.0, -1.0], [0.3, -1.0, -1.0]]
    assert c["hc_bases"].tolist() == [[60, 62, 51], [0, 0, 0], [20, 0, 0]] and c["variance"][0].tolist() == [2.5, 4.5, 6.5]
    c8 = assign_top_ref.reduce_top(3, acc, 8)
    assert c8["count"].tolist() == [4, 0, 1] and c8["target"][0, :5].tolist() == [1, 2, 3, 0, -1]
    assert assign_top_ref.same(c, assign_top_ref.reduce_top(3, acc[:-1], 3))              # (the comparison itself sees a difference)
    other = {f: v.copy() for f, v in c.items()}
    other["score"][0, 2] = np.nextafter(0.7, 1.0)
    assert assign_top_ref.same(c, other)
