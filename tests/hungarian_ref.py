"""A numpy restatement of the solver of csrc/assign.hip (include/vitadapter_hip_assign.h) and the cases its tests share.

``solve(cost)`` is the shortest-augmenting-path method of scipy's linear_sum_assignment (rectangular Jonker-Volgenant) in
fp64 with the kernel's tie rule: among the columns of the lowest reduced cost an unassigned one first, then the lowest
column index.  The smaller dimension is the row set.  -> (status, queries, gts, steps): status 0 / 1 / 2 as the header
defines them, the pairs in ascending query order (the identity pairing when status is not 0), and the number of search
steps (row reads) the solve took - the figure DESIGN.md reports per problem.

``table_of(costs, counts, Q, solver)`` builds the (L, 2, K) table and the (L, N) status of a stacked (L, N, Q, Gmax) cost array
the way Mask2FormerHead.loss builds its table from per-problem results."""
import numpy as np

SHAPES = ((1, 1), (1, 3), (3, 1), (5, 5), (7, 3), (3, 7), (64, 64), (65, 9), (100, 12), (100, 100), (100, 150), (130, 20),
          (256, 40), (40, 256))
INVALID, INFEASIBLE = 'matrix contains invalid numeric entries', 'cost matrix is infeasible'


def solve(cost):
    cost = np.asarray(cost)
    Q, G = cost.shape
    k = min(Q, G)
    ident = (np.arange(k, dtype=np.int64), np.arange(k, dtype=np.int64))
    if k == 0:
        return 0, ident[0], ident[1], 0
    c64 = cost.astype(np.float64)
    if np.isnan(c64).any() or (c64 == -np.inf).any():
        return 1, ident[0], ident[1], 0
    tr = Q > G
    C = c64.T.copy() if tr else c64
    nr, nc = C.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    cols = np.arange(nc)
    steps = 0
    for cur in range(nr):
        sp = np.full(nc, np.inf)
        path = np.full(nc, -1)
        scanned = np.zeros(nc, dtype=bool)
        min_val, i, sink = 0.0, cur, -1
        while sink < 0:
            steps += 1
            open_ = ~scanned
            with np.errstate(invalid='ignore'):
                r = ((min_val + C[i]) - u[i]) - v
            better = open_ & (r < sp)
            sp[better], path[better] = r[better], i
            cand = np.where(open_, sp, np.inf)
            low = cand.min()
            if not low < np.inf:
                return 2, ident[0], ident[1], steps
            tie = open_ & (sp == low)
            free = tie & (row4col < 0)
            j = int(cols[free][0]) if free.any() else int(cols[tie][0])
            min_val = low
            scanned[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = int(row4col[j])
        for j in cols[scanned]:
            d = min_val - sp[j]
            v[j] -= d
            if row4col[j] >= 0:
                u[row4col[j]] += d
        u[cur] += min_val
        j = sink
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if tr:
        q = cols[row4col >= 0]
        return 0, q.astype(np.int64), row4col[q].astype(np.int64), steps
    return 0, np.arange(nr, dtype=np.int64), col4row.astype(np.int64), steps


def scipy_pairs(cost):
    """scipy's assignment of a block in ascending query order (what the head's argsort produces)"""
    from scipy.optimize import linear_sum_assignment
    r, c = linear_sum_assignment(cost)
    order = r.argsort(kind='stable')
    return r[order].astype(np.int64), c[order].astype(np.int64)


def random_cases(seed=0, reps=6):
    """[(name, (Q, G) fp32 block)]: costs 3 N(0, 1) + 5, every shape of SHAPES ``reps`` times"""
    rng = np.random.RandomState(seed)
    return [('%dx%d_%d' % (q, g, k), (3.0 * rng.randn(q, g) + 5.0).astype(np.float32)) for q, g in SHAPES for k in range(reps)]


def tie_cases(seed=1, count=50):
    """[(name, block)]: integer costs in {0 .. 3}, so that many assignments share the optimum and every sum is exact"""
    rng = np.random.RandomState(seed)
    shapes = [(5, 5), (7, 3), (3, 7), (20, 20), (65, 9), (9, 65), (100, 12), (30, 70), (70, 70), (130, 20)]
    return [('tie_%dx%d_%d' % (shapes[k % len(shapes)] + (k,)), rng.randint(0, 4, shapes[k % len(shapes)]).astype(np.float32))
            for k in range(count)]


def bad_cases():
    """[(name, block, status)]: a NaN, a -inf, a row of +inf (in either orientation), and +inf entries that leave it feasible"""
    rng = np.random.RandomState(2)
    out = []
    for q, g in ((7, 3), (3, 7), (100, 12)):
        c = (3.0 * rng.randn(q, g) + 5.0).astype(np.float32)
        a, b, d = c.copy(), c.copy(), c.copy()
        a[q // 2, g // 2] = np.nan
        b[q - 1, 0] = -np.inf
        if q >= g:
            d[:, g - 1] = np.inf                                    # a row of the solver: a ground truth nobody can take
        else:
            d[1, :] = np.inf
        e = c.copy()
        e[0, 0] = np.inf
        out += [('nan_%dx%d' % (q, g), a, 1), ('ninf_%dx%d' % (q, g), b, 1), ('infrow_%dx%d' % (q, g), d, 2), ('inf_ok_%dx%d' % (q, g), e, 0)]
    return out


def valid_pairing(q, g, shape):
    Q, G = shape
    k = min(Q, G)
    return (len(q) == len(g) == k and len(set(q.tolist())) == k and len(set(g.tolist())) == k and np.all(np.diff(q) > 0)
            and (k == 0 or (0 <= q.min() and q.max() < Q and 0 <= g.min() and g.max() < G)))


def table_of(costs, counts, Q, solver):
    """costs (L, N, Q, Gmax), counts per image -> (table (L, 2, K) int64, status (L, N) int32) with ``solver`` a function
    block -> (status, queries, gts, ...) applied to costs[i, n, :, :counts[n]]"""
    L, N = costs.shape[:2]
    firsts = [sum(counts[:n]) for n in range(N)]
    table, status = [], np.zeros((L, N), dtype=np.int32)
    for i in range(L):
        rows, tgts = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
        for n in range(N):
            if counts[n]:
                res = solver(costs[i, n, :, :counts[n]])
                status[i, n] = res[0]
                rows.append(res[1] + n * Q)
                tgts.append(res[2] + firsts[n])
        table.append(np.stack([np.concatenate(rows), np.concatenate(tgts)]))
    return np.stack(table), status


def scipy_solver(block):
    q, g = scipy_pairs(block)
    return 0, q, g
