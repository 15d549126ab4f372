"""CPU: the numpy restatement of the assignment solver (tests/hungarian_ref.py) against scipy's linear_sum_assignment, the
conditions on the shared cases that let the GPU test demand scipy's assignment exactly, and fused.hungarian_match on CPU tensors
against the head's path before the kernel.

The random cases (costs 3 N(0, 1) + 5 in fp32, the shapes of hungarian_ref.SHAPES) must be ROBUST: scipy's answer does not move
under 4 draws of relative noise 1e-9 on the fp64 costs, six or more orders above anything fp64 arithmetic on costs of this size
moves.  That is a condition on the inputs, asserted here, not a tolerance on the kernel.  The tie cases have integer costs, so
totals are exact and are compared with ==."""
import numpy as np
import pytest
import torch

import hungarian_ref as ref

RANDOM, TIES, BAD = ref.random_cases(), ref.tie_cases(), ref.bad_cases()


def test_the_cases_cover_the_shapes():
    assert len(RANDOM) == 84 and len(TIES) == 50
    assert {c.shape for _, c in RANDOM} == set(ref.SHAPES)
    assert all(c.dtype == np.float32 for _, c in RANDOM + TIES)


@pytest.mark.parametrize('shape', ref.SHAPES, ids=lambda s: '%dx%d' % s)
def test_restatement_gives_scipys_assignment_on_robust_cases(shape):
    rng = np.random.RandomState(11)
    for name, c in RANDOM:
        if c.shape != shape:
            continue
        c64 = c.astype(np.float64)
        want = ref.scipy_pairs(c64)
        for _ in range(4):                                          # the condition on the inputs
            noisy = ref.scipy_pairs(c64 * (1.0 + 1e-9 * rng.uniform(-1, 1, c64.shape)))
            assert np.array_equal(noisy[0], want[0]) and np.array_equal(noisy[1], want[1]), '%s is not robust' % name
        status, q, g, steps = ref.solve(c)
        assert status == 0 and ref.valid_pairing(q, g, c.shape), name
        assert np.array_equal(q, want[0]) and np.array_equal(g, want[1]), name
        # the search for row r scans at most the r assigned columns and one free one
        assert min(shape) <= steps <= min(shape) * (min(shape) + 1) // 2, (name, steps)


def test_tie_cases_are_optimal():
    for name, c in TIES:
        c64 = c.astype(np.float64)
        sq, sg = ref.scipy_pairs(c64)
        status, q, g, _ = ref.solve(c)
        assert status == 0 and ref.valid_pairing(q, g, c.shape), name
        assert c64[q, g].sum() == c64[sq, sg].sum(), name


def test_status_codes_agree_with_scipys_errors():
    from scipy.optimize import linear_sum_assignment
    for name, c, want in BAD:
        status, q, g, _ = ref.solve(c)
        assert status == want, name
        if want:
            with pytest.raises(ValueError, match={1: ref.INVALID, 2: ref.INFEASIBLE}[want]):
                linear_sum_assignment(c.astype(np.float64))
            k = min(c.shape)
            assert np.array_equal(q, np.arange(k)) and np.array_equal(g, np.arange(k)), name
        else:
            sq, sg = ref.scipy_pairs(c.astype(np.float64))
            assert np.array_equal(q, sq) and np.array_equal(g, sg), name
    assert ref.solve(np.zeros((5, 0), dtype=np.float32))[:1] == (0,) and ref.solve(np.zeros((5, 0), dtype=np.float32))[1].size == 0


def _present_path(costs, counts):
    """Mask2FormerHead.loss's table before the kernel: scipy per (output, image), positives in query order"""
    from scipy.optimize import linear_sum_assignment
    L, N, Q, _ = costs.shape
    firsts = [sum(counts[:n]) for n in range(N)]
    table = []
    for i in range(L):
        rows, tgts = [], []
        for n in range(N):
            if counts[n]:
                r, c = linear_sum_assignment(costs[i, n, :, :counts[n]].numpy())
                order = r.argsort(kind='stable')
                rows.append(torch.from_numpy(r[order]).long() + n * Q)
                tgts.append(torch.from_numpy(c[order]).long() + firsts[n])
        table.append(torch.stack([torch.cat(rows), torch.cat(tgts)]))
    return torch.stack(table)


def test_hungarian_match_on_cpu_tensors_is_the_present_path():
    from vitadapter import fused
    assert fused.ENABLED['hungarian'] is True
    g = torch.Generator().manual_seed(5)
    L, N, Q, counts = 3, 3, 20, [7, 0, 25]
    costs = torch.full((L, N, Q, max(counts)), float('inf'))
    for n, c in enumerate(counts):
        costs[:, n, :, :c] = torch.randn((L, Q, c), generator=g) * 3 + 5
    want = _present_path(costs, counts)
    for arg in (costs, list(costs)):
        table, status = fused.hungarian_match(arg, counts)
        assert status is None and table.dtype == torch.int64 and tuple(table.shape) == (L, 2, 7 + 20)
        assert torch.equal(table, want)
    again, _ = ref.table_of(costs.numpy(), counts, Q, ref.solve)
    assert np.array_equal(again, want.numpy())
    table, status = fused.hungarian_match(costs[:, :, :, :0], [0, 0, 0])
    assert status is None and tuple(table.shape) == (L, 2, 0)
    with pytest.raises(ValueError, match='counts'):
        fused.hungarian_match(costs, [7, 0])
    with pytest.raises(ValueError, match=ref.INFEASIBLE):
        fused.hungarian_match(torch.full((1, 1, 4, 2), float('inf')), [2])
