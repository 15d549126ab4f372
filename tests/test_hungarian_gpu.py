"""GPU: vah_assign_solve (csrc/assign.hip) through fused.hungarian_match on the cases of tests/hungarian_ref.py.

Random cases: tests/test_hungarian_ref_cpu.py asserts that scipy's answer on each of them does not move under relative noise of
1e-9, so the kernel - fp64 duals over the same fp32 costs - has to give scipy's assignment EXACTLY: the (L, 2, K) table equals the
one built from scipy per problem the way Mask2FormerHead.loss built it.  Tie cases (integer costs): the pairing is valid and its
fp64 total equals scipy's with ==.  Invalid and infeasible blocks: status 1 / 2 and the identity pairing, the other problems of the
same launch as if alone.  Shapes: every one of hungarian_ref.SHAPES on its own (one, two, three and four column slots of a
lane, both orientations, G = Q), and batches as a training step makes them (several outputs, ragged counts with +inf padding
columns, an image without targets in front of and behind one with)."""
import numpy as np
import pytest
import torch

import hungarian_ref as ref
from vitadapter import fused

pytestmark = pytest.mark.gpu
RANDOM, TIES, BAD = ref.random_cases(), ref.tie_cases(), ref.bad_cases()
BY_SHAPE = {s: [c for _, c in RANDOM if c.shape == s] for s in ref.SHAPES}


def dev():
    return torch.device('cuda:0')


def stack(blocks, Q):
    """blocks[i][n] (Q, G_n) or None -> costs (L, N, Q, Gmax) with +inf padding, counts"""
    L, N = len(blocks), len(blocks[0])
    counts = [0 if blocks[0][n] is None else blocks[0][n].shape[1] for n in range(N)]
    costs = np.full((L, N, Q, max(max(counts), 1)), np.inf, dtype=np.float32)
    for i in range(L):
        for n in range(N):
            if counts[n]:
                assert blocks[i][n].shape == (Q, counts[n])
                costs[i, n, :, :counts[n]] = blocks[i][n]
    return costs, counts


def run(costs, counts):
    table, status = fused.hungarian_match(torch.from_numpy(costs).to(dev()), counts)
    assert status is not None, 'the kernel path did not run'
    torch.cuda.synchronize()
    return table.cpu().numpy(), status.cpu().numpy()


def scipy_or_identity(block):
    try:
        return ref.scipy_solver(block.astype(np.float64))
    except ValueError as e:
        k = min(block.shape)
        return (1 if ref.INVALID in str(e) else 2), np.arange(k, dtype=np.int64), np.arange(k, dtype=np.int64)


@pytest.mark.parametrize('shape', ref.SHAPES, ids=lambda s: '%dx%d' % s)
def test_each_shape_on_its_own_gives_scipys_table(shape):
    Q, G = shape
    costs, counts = stack([[c] for c in BY_SHAPE[shape]], Q)
    table, status = run(costs, counts)
    want, _ = ref.table_of(costs, counts, Q, ref.scipy_solver)
    assert table.dtype == np.int64 and table.shape == (len(BY_SHAPE[shape]), 2, min(Q, G))
    assert np.array_equal(status, np.zeros_like(status))
    assert np.array_equal(table, want)
    assert np.all(np.diff(table[:, 0], axis=1) > 0)                # queries ascending


@pytest.mark.parametrize('gs', [(12, 100), (0, 150), (150, 12), (100, 0), (0, 0, 12, 0, 150)], ids=str)
def test_batches_as_a_step_makes_them(gs):
    Q, L = 100, 3
    blocks = [[None if g == 0 else BY_SHAPE[(Q, g)][(i + n) % 6] for n, g in enumerate(gs)] for i in range(L)]
    costs, counts = stack(blocks, Q)
    assert counts == list(gs) and (len(set(gs) - {0}) < 2 or np.isinf(costs).any())      # ragged: padding columns of +inf
    table, status = run(costs, counts)
    want, _ = ref.table_of(costs, counts, Q, ref.scipy_solver)
    assert table.shape == (L, 2, sum(min(Q, g) for g in gs))
    assert np.array_equal(status, np.zeros((L, len(gs)), dtype=np.int32))
    assert np.array_equal(table, want)                              # base_n behind an empty image included
    for n, g in enumerate(gs):                                      # per image: its own query rows, ascending
        lo = sum(min(Q, x) for x in gs[:n])
        rows = table[:, 0, lo:lo + min(Q, g)]
        assert np.all(rows // Q == n) and np.all(np.diff(rows, axis=1) > 0)


def test_tie_cases_are_valid_and_optimal():
    shapes = sorted({c.shape for _, c in TIES})
    for shape in shapes:
        group = [c for _, c in TIES if c.shape == shape]
        Q, G = shape
        costs, counts = stack([[c] for c in group], Q)
        table, status = run(costs, counts)
        assert np.array_equal(status, np.zeros_like(status))
        for i, c in enumerate(group):
            q, g = table[i, 0], table[i, 1]
            assert ref.valid_pairing(q, g, shape), (shape, i)
            c64 = c.astype(np.float64)
            sq, sg = ref.scipy_pairs(c64)
            assert c64[q, g].sum() == c64[sq, sg].sum(), (shape, i)


@pytest.mark.parametrize('shape', [(7, 3), (3, 7), (100, 12)], ids=lambda s: '%dx%d' % s)
def test_invalid_and_infeasible_blocks(shape):
    Q, G = shape
    bad = {name.rsplit('_', 1)[0]: c for name, c, _ in BAD if c.shape == shape and name.endswith('%dx%d' % shape)}
    good = BY_SHAPE[shape]
    blocks = [[bad['nan'], good[0]], [bad['ninf'], bad['infrow']], [good[-1], bad['inf_ok']]]
    costs, counts = stack(blocks, Q)
    table, status = run(costs, counts)
    assert np.array_equal(status, np.array([[1, 0], [1, 2], [0, 0]], dtype=np.int32))
    want, want_status = ref.table_of(costs, counts, Q, scipy_or_identity)
    assert np.array_equal(want_status, status)
    assert np.array_equal(table, want)                              # identity pairs where status != 0, scipy's elsewhere
    k = min(Q, G)
    assert np.array_equal(table[0, :, :k], np.stack([np.arange(k), np.arange(k)]))
    assert np.array_equal(table[1, :, k:], np.stack([Q + np.arange(k), G + np.arange(k)]))


def test_two_runs_give_the_same_bits_and_the_launch_captures():
    Q = 100
    blocks = [[BY_SHAPE[(Q, 12)][i], None, BY_SHAPE[(Q, 100)][i]] for i in range(3)]
    costs, counts = stack(blocks, Q)
    want, _ = ref.table_of(costs, counts, Q, ref.scipy_solver)
    c = torch.from_numpy(costs).to(dev())
    offsets = torch.tensor([0, 12, 12, 112], dtype=torch.int32, device=dev())
    a, sa = fused.hungarian_match(c, counts, gt_offsets=offsets)
    b, sb = fused.hungarian_match(list(c), counts)                  # the list form, offsets uploaded by the call
    assert torch.equal(a, b) and torch.equal(sa, sb) and np.array_equal(a.cpu().numpy(), want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused.hungarian_match(c, counts, gt_offsets=offsets)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        table, status = fused.hungarian_match(c, counts, gt_offsets=offsets)      # captured, not run
    torch.cuda.synchronize()
    table.fill_(-7)
    status.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy(), want) and not bool(status.any())
    c.copy_(torch.from_numpy(costs[::-1].copy()))                  # the replay reads the buffers it captured
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy(), want[::-1])


def test_offsets_that_are_no_counts_write_no_pair():
    """an offset pair out of order or beyond Gmax, seen on the device only: status 2, no pair, and it counts for nothing in the
    bases of the others"""
    Q, G = 7, 3
    good = BY_SHAPE[(Q, G)]
    costs, _ = stack([[good[0], good[1], good[2]]], Q)
    offsets = torch.tensor([0, 3, 2, 5], dtype=torch.int32, device=dev())      # image 1: -1 targets; image 2: 3 of them from 2
    c = torch.from_numpy(costs).to(dev())
    table = torch.full((1, 2, 6 + 4), -7, dtype=torch.int64, device=dev())
    status = torch.full((1, 3), -7, dtype=torch.int32, device=dev())
    import _vah
    _vah.check(_vah.lib.vah_assign_solve(c.data_ptr(), offsets.data_ptr(), 1, 3, Q, G, table.data_ptr(), status.data_ptr(),
                                         _vah.raw_stream(dev())), 'vah_assign_solve')
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [[0, 2, 0]]
    t = table.cpu().numpy()
    q0, g0 = ref.scipy_pairs(good[0].astype(np.float64))
    q2, g2 = ref.scipy_pairs(good[2].astype(np.float64))
    # K on the device is 6: row 0 is t[0, 0, :6] of the flat buffer, row 1 the next six words; nothing behind them is written
    flat = t.reshape(-1)
    assert np.array_equal(flat[:6], np.concatenate([q0, 2 * Q + q2])) and np.array_equal(flat[6:12], np.concatenate([g0, 2 + g2]))
    assert np.all(flat[12:] == -7)
