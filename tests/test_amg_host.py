'''CPU-side checks of the smoothed-aggregation AMG preconditioner (matrix.HipMatrix.solve(solver='cg', precon='amg'), nutils_amd/amg.py, nh_amg.hip): a
numpy / scipy restatement of the algorithm -- aggregation, prolongator, Galerkin product, V-cycle, preconditioned CG -- with its invariants pinned; the
symbolic phase of nutils_amd.amg on CPU tensors, integer for integer against the restatement; its expand-sort-compress plans against scipy's products; and
the argument errors of the solve.  The restatement is the CPU reference of tests/test_gpu_amg.py.'''
import functools
import types
import numpy
import pytest
import scipy.sparse
import scipy.sparse.linalg

from test_cg_host import cg_reference, gamma

M32 = 0xffffffff


# ---- the algorithm, restated ---------------------------------------------------------------------------------------------

def keys(n, start=0):
    with numpy.errstate(over='ignore'):
        i = numpy.arange(start, n, dtype=numpy.uint64)
        h = (i + numpy.uint64(1)) * numpy.uint64(0x9E3779B97F4A7C15)
        h ^= h >> numpy.uint64(32)
        h *= numpy.uint64(0xD6E8FEB86659FD93)
        h ^= h >> numpy.uint64(32)
        return (((h >> numpy.uint64(33)) << numpy.uint64(32)) | i).astype(numpy.int64)


def free_part(A, free):
    '''A on the free rows and columns, structural zeros kept; the shape stays'''
    coo = A.tocoo()
    keep = free[coo.row] & free[coo.col]
    Af = scipy.sparse.csr_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), A.shape)
    Af.sort_indices()
    return Af


def structure(A):
    '''the pattern as a matrix of ones: products of such have no cancellation, and scipy drops the zeros it computes'''
    return scipy.sparse.csr_matrix((numpy.ones(A.nnz), A.indices, A.indptr), A.shape)


def aggregate(A, free):
    '''(agg, roots, rounds) by Luby rounds; agg = -1 on constrained dofs'''
    n = A.shape[0]
    coo = A.tocoo()
    keep = (coo.row != coo.col) & free[coo.row] & free[coo.col]
    er, ec = coo.row[keep], coo.col[keep]

    def spread(v, own=True):
        out = v.copy() if own else numpy.full_like(v, -1)
        numpy.maximum.at(out, er, v[ec])
        return out

    key = keys(n)
    undecided, root, rounds = free.copy(), numpy.zeros(n, dtype=bool), 0
    while undecided.any():
        k = numpy.where(undecided, key, -1)
        new = undecided & (k == spread(spread(k)))
        root |= new
        undecided &= spread(spread(new.astype(numpy.int64))) == 0
        rounds += 1
    owner = numpy.where(root, key, numpy.where(free, spread(numpy.where(root, key, -1), own=False), -1))
    owner = numpy.where(free & (owner < 0), spread(owner, own=False), owner)
    assert (owner[free] >= 0).all()
    number = numpy.cumsum(root) - 1
    return numpy.where(free, number[numpy.maximum(owner, 0) & M32], -1), numpy.flatnonzero(root), rounds


def sample(M, pattern):
    '''the values of M on the entries of `pattern` (0 where M has none)'''
    coo = pattern.tocoo()
    return numpy.asarray(M[coo.row, coo.col]).ravel() if pattern.nnz else numpy.zeros(0)


def on_pattern(M, pattern):
    pattern = pattern.tocsr()
    pattern.sort_indices()
    return scipy.sparse.csr_matrix((sample(M.tocsr(), pattern), pattern.indices, pattern.indptr), pattern.shape)


def level(A, free, coarse):
    '''one level of the hierarchy from its matrix: kind, weights, and for a coarsened level agg, P, R, A_c'''
    n = A.shape[0]
    lv = types.SimpleNamespace(A=A, free=free, n=n, nfree=int(free.sum()))
    diag = A.diagonal()
    assert (diag[free] != 0).all()
    lv.dinv = numpy.where(free, 1 / numpy.where(diag == 0, 1, diag), 0.)
    if lv.nfree <= coarse:
        lv.kind = 'dense'
        lv.idx = numpy.flatnonzero(free)
        lv.ainv = numpy.linalg.pinv(A.toarray()[numpy.ix_(lv.idx, lv.idx)], hermitian=True)
        return lv
    lv.Af = Af = free_part(A, free)
    lv.agg, lv.roots, lv.rounds = aggregate(A, free)
    lv.nc = len(lv.roots)
    if lv.nc == lv.nfree:
        lv.kind = 'diagonal'
        return lv
    lv.kind = 'coarsen'
    lv.rho = ((abs(Af) @ free.astype(float)) * lv.dinv).max()
    lv.omega = 4 / (3 * lv.rho)
    lv.w = lv.omega * lv.dinv
    idx = numpy.flatnonzero(free)
    lv.T = T = scipy.sparse.csr_matrix((numpy.ones(len(idx)), (idx, lv.agg[idx])), (n, lv.nc))
    S = structure(Af)
    ppat = (S @ T).tocsr()
    lv.AT = on_pattern(Af @ T, ppat)
    rows = numpy.repeat(numpy.arange(n), numpy.diff(lv.AT.indptr))
    lv.P = scipy.sparse.csr_matrix((sample(T, lv.AT) - lv.w[rows] * lv.AT.data, lv.AT.indices, lv.AT.indptr), (n, lv.nc))
    lv.R = lv.P.T.tocsr()
    lv.R.sort_indices()
    lv.AP = on_pattern(Af @ lv.P, S @ structure(lv.P))
    lv.Ac = on_pattern(lv.R @ (Af @ lv.P), structure(lv.R) @ S @ structure(lv.P))  # (associated as the plans are: A P first)
    return lv


def hierarchy(A, free, coarse=256):
    levels = []
    while True:
        lv = level(A, free, coarse)
        levels.append(lv)
        if lv.kind != 'coarsen':
            return levels
        A, free = lv.Ac, numpy.ones(lv.nc, dtype=bool)


def product(A, x):
    '''A x in the arithmetic of x (longdouble: scipy's product would round to double), for a vector or the columns of a matrix'''
    if x.dtype == float:
        return A @ x
    coo = A.tocoo()
    y = numpy.zeros((A.shape[0],) + x.shape[1:], dtype=x.dtype)
    numpy.add.at(y, coo.row, coo.data.astype(x.dtype).reshape((-1,) + (1,) * (x.ndim - 1)) * x[coo.col])
    return y


def cycle(levels, b, sweeps=1, l=0):
    '''z = M b, in the arithmetic of b (a vector, or a matrix whose columns are right-hand sides)'''
    lv = levels[l]
    col = lambda v: v.astype(b.dtype).reshape((-1,) + (1,) * (b.ndim - 1))
    if lv.kind == 'dense':
        z = numpy.zeros_like(b)
        z[lv.idx] = lv.ainv.astype(b.dtype) @ b[lv.idx]
        return z
    if lv.kind == 'diagonal':
        return col(lv.dinv) * b
    w, free = col(lv.w), col(lv.free)
    x = w * b
    for _ in range(sweeps - 1):
        x = numpy.where(free, x + w * (b - product(lv.A, x)), 0)
    r = numpy.where(free, b - product(lv.A, x), 0)
    x = x + product(lv.P, cycle(levels, product(lv.R, r), sweeps, l + 1))
    for _ in range(sweeps):
        x = numpy.where(free, x + w * (b - product(lv.A, x)), 0)
    return x


def pcg_reference(A, b, x, free, M, stop_rr, maxiter):
    '''The host loop of HipMatrix._cg with z = M(r), looking at the residual after every iteration: (x, iterations, starts, outcome)'''
    mask = lambda y: numpy.where(free, y, 0.)
    x = numpy.array(x, dtype=float)
    it = starts = 0
    while True:
        r = mask(b - A @ x)
        starts += 1
        if r @ r <= stop_rr:
            return x, it, starts, 'converged'
        if it >= maxiter:
            return x, it, starts, 'maxiter'
        z = M(r)
        p, rz = z.copy(), r @ z
        while it < maxiter:
            q = mask(A @ p)
            pq = p @ q
            if not (rz > 0 and pq > 0):
                return x, it, starts, 'flagged'
            alpha = rz / pq
            x, r = x + alpha * p, r - alpha * q
            it += 1
            if r @ r <= stop_rr:
                break
            z = M(r)
            rz, rz_old = r @ z, rz
            p = z + (rz / rz_old) * p


def segment_dot(ptr, ia, ib, a, b=None):
    '''nh_segment_dot in numpy'''
    prod = a[ia] if b is None else a[ia] * b[ib]
    out = numpy.zeros(len(ptr) - 1, dtype=prod.dtype)
    numpy.add.at(out, numpy.repeat(numpy.arange(len(ptr) - 1), numpy.diff(ptr)), prod)
    return out


# ---- problems ------------------------------------------------------------------------------------------------------------

def line(n, h):
    '''stiffness and mass matrix of n linear elements' nodes on a uniform line'''
    e = numpy.ones(n - 1)
    K = scipy.sparse.diags([-e, numpy.r_[1., 2 * numpy.ones(n - 2), 1.], -e], [-1, 0, 1]) / h
    M = scipy.sparse.diags([e, numpy.r_[2., 4 * numpy.ones(n - 2), 2.], e], [-1, 0, 1]) * (h / 6)
    return K, M


@functools.lru_cache(maxsize=None)
def problem(name):
    '''(A, free): 'laplace' the bilinear Laplace matrix on 40 x 37 nodes of [0, 1] x [0, 2] with one side held; 'chain' tridiag(-1, 2, -1) of 3000 dofs, every
    1000th held; 'diagonal'; 'orphan': a chain in which dof 0 is free and its only neighbour is held.  Made once, never written.'''
    if name == 'laplace':
        (Kx, Mx), (Ky, My) = line(40, 1 / 39), line(37, 2 / 36)
        A = scipy.sparse.csr_matrix(scipy.sparse.kron(Kx, My) + scipy.sparse.kron(Mx, Ky))
        free = numpy.ones((40, 37), dtype=bool)
        free[0] = False
        free = free.ravel()
    elif name == 'chain':
        n = 3000
        A = scipy.sparse.diags([-numpy.ones(n - 1), numpy.full(n, 2.), -numpy.ones(n - 1)], [-1, 0, 1], format='csr')
        free = numpy.ones(n, dtype=bool)
        free[::1000] = False
    elif name == 'diagonal':
        A = scipy.sparse.diags(numpy.random.default_rng(5).uniform(1, 10, 700), format='csr')
        free = numpy.ones(700, dtype=bool)
        free[::7] = False
    else:
        n = 600
        A = scipy.sparse.diags([-numpy.ones(n - 1), numpy.full(n, 2.), -numpy.ones(n - 1)], [-1, 0, 1], format='csr')
        free = numpy.ones(n, dtype=bool)
        free[[1, 300, 302]] = False  # dofs 0 and 301 keep no free neighbour
    A.sort_indices()
    return A, free


@functools.lru_cache(maxsize=None)
def reference(name, coarse):
    return hierarchy(*problem(name), coarse)


def symbolic(name, coarse):
    import torch
    from nutils_amd import amg
    A, free = problem(name)
    return amg.symbolic(torch.from_numpy(A.indptr.astype(numpy.int64)), torch.from_numpy(A.indices.astype(numpy.int64)), torch.from_numpy(free), coarse)


CASES = [('laplace', 16), ('chain', 256)]


# ---- tests ---------------------------------------------------------------------------------------------------------------

def test_hash_is_the_documented_mix():
    '''the keys in Python integers, and those of nutils_amd.amg'''
    from nutils_amd import amg
    for i in (0, 1, 5, 1479, 262443, 2 ** 31 - 1):
        h = ((i + 1) * 0x9E3779B97F4A7C15) % 2 ** 64
        h ^= h >> 32
        h = (h * 0xD6E8FEB86659FD93) % 2 ** 64
        h ^= h >> 32
        assert keys(i + 1, i)[0] == (h >> 33) << 32 | i
    assert numpy.array_equal(amg.keys(3000).numpy(), keys(3000))
    assert len(numpy.unique(keys(3000) >> 32)) > 2990  # (a mix, not the index)


@pytest.mark.parametrize('name', ['laplace', 'chain', 'diagonal', 'orphan'])
def test_aggregation_invariants(name):
    A, free = problem(name)
    n = A.shape[0]
    agg, roots, rounds = aggregate(A, free)
    print(f'{name}: {free.sum()} free dofs, {len(roots)} aggregates, {rounds} rounds')
    assert rounds <= 8
    assert (agg[~free] == -1).all() and (agg[free] >= 0).all()  # every free dof in exactly one aggregate, constrained ones in none
    assert numpy.array_equal(numpy.unique(agg[free]), numpy.arange(len(roots)))
    assert numpy.array_equal(agg[roots], numpy.arange(len(roots)))  # a root owns itself; numbering by ascending root index
    G = structure(free_part(A, free))
    G.setdiag(1)
    G2 = (G @ G).tocsr()  # within two edges
    between = G2[roots][:, roots]
    assert between.nnz == len(roots)  # roots are pairwise more than two edges apart: each reaches itself only
    assert (numpy.asarray(G2[numpy.flatnonzero(free), roots[agg[free]]]) > 0).all()  # every member is within two edges of its root
    if name == 'diagonal':
        assert len(roots) == free.sum()
    if name == 'orphan':
        for i in (0, 301):
            assert (agg == agg[i]).sum() == 1 and i in roots


def test_terminal_levels():
    assert [lv.kind for lv in reference('diagonal', 256)] == ['diagonal']
    assert [lv.kind for lv in reference('diagonal', 1024)] == ['dense']
    assert [lv.kind for lv in symbolic('diagonal', 256)] == ['diagonal']
    assert [lv.kind for lv in symbolic('diagonal', 1024)] == ['dense']
    assert [(lv.kind, lv.nfree) for lv in symbolic('orphan', 16)] == [(lv.kind, lv.nfree) for lv in reference('orphan', 16)]


@pytest.mark.parametrize('name,coarse', CASES)
def test_symbolic_phase_matches_the_restatement(name, coarse):
    '''aggregates and the patterns of P, R and A_c, integer for integer and level by level; a rebuild gives the same integers'''
    ref, got, again = reference(name, coarse), symbolic(name, coarse), symbolic(name, coarse)
    print(f'{name}: levels {[lv.nfree for lv in ref]}')
    assert [lv.kind for lv in got] == [lv.kind for lv in ref] and len(ref) >= (3 if name == 'laplace' else 2)
    assert [lv.nfree for lv in got] == [lv.nfree for lv in ref]
    same = lambda tensor, array: numpy.array_equal(tensor.numpy(), array)
    for r, g, h in zip(ref, got, again):
        assert same(g.rowptr, r.A.indptr) and same(g.colidx, r.A.indices)
        if r.kind != 'coarsen':
            continue
        assert g.nc == r.nc and same(g.agg, r.agg) and g.rounds == r.rounds
        assert same(g.prowptr, r.P.indptr) and same(g.pcol, r.P.indices)
        assert same(g.rrowptr, r.R.indptr) and same(g.rcol, r.R.indices)
        assert same(g.tind, sample(r.T, r.P))
        for name_ in ('agg', 'prowptr', 'pcol', 'rrowptr', 'rcol', 'rperm'):
            assert numpy.array_equal(getattr(g, name_).numpy(), getattr(h, name_).numpy())
        for plan in ('at', 'ap', 'rap'):
            for name_ in ('ptr', 'ia', 'ib'):
                a, b = getattr(getattr(g, plan), name_), getattr(getattr(h, plan), name_)
                assert (a is None and b is None) or numpy.array_equal(a.numpy(), b.numpy())


@pytest.mark.parametrize('name,coarse', CASES)
def test_plans_reproduce_the_products(name, coarse):
    '''A_f T, A_f P and P^T A_f P from the plans, by nh_segment_dot in numpy, against scipy's: every entry within gamma_(len + 2) sum |terms|; the products of an
    entry are consecutive, and sorted by the entry they belong to'''
    ref, got = reference(name, coarse), symbolic(name, coarse)
    for r, g in zip(ref, got):
        if r.kind != 'coarsen':
            continue
        a = r.A.data
        for what, plan, fa, fb, expect in (('A T', g.at, a, None, r.AT), ('A P', g.ap, a, r.P.data, r.AP), ('R A P', g.rap, r.R.data, r.AP.data, r.Ac)):
            ptr, ia, ib = plan.ptr.numpy(), plan.ia.numpy(), None if plan.ib is None else plan.ib.numpy()
            assert ptr[0] == 0 and ptr[-1] == len(ia) == plan.nprod and (numpy.diff(ptr) >= 1).all() and len(ptr) - 1 == plan.nseg
            rows = numpy.repeat(numpy.arange(expect.shape[0]), numpy.diff(expect.indptr))
            assert numpy.array_equal(plan.rows.numpy(), rows) and numpy.array_equal(plan.cols.numpy(), expect.indices)  # sorted by output entry
            value = segment_dot(ptr, ia, ib, fa, fb)
            bound = gamma(numpy.diff(ptr) + 2) * segment_dot(ptr, ia, ib, abs(fa), None if fb is None else abs(fb))
            err = abs(value - expect.data)
            print(f'{name} level {r.n}: {what}: {plan.nseg} entries of {plan.nprod} products, max error / bound {(err / numpy.maximum(bound, 1e-300)).max():.3f}')
            assert (err <= bound).all()
        assert numpy.array_equal(r.P.data[g.rperm.numpy()], r.R.data)  # the permutation that takes the values of P to those of R


def test_cycle_is_symmetric_positive_definite():
    '''M assembled densely on the Laplace problem with three levels, by applying the cycle to the unit vectors'''
    A, free = problem('laplace')
    for sweeps in (1, 2):
        M = cycle(reference('laplace', 16), numpy.eye(A.shape[0]), sweeps)
        scale = abs(M).max()
        print(f'sweeps={sweeps}: |M - M^T| / |M| = {abs(M - M.T).max() / scale:.2e}')
        assert abs(M - M.T).max() <= 1e-12 * scale
        assert not M[~free].any() and not M[:, ~free].any()
        assert numpy.linalg.eigvalsh(M[free][:, free])[0] > 0


@pytest.mark.parametrize('coarse', [256, 16])
def test_pcg_of_the_restatement(coarse):
    '''AMG-CG converges to rtol = 1e-10 against a direct solve, in at most a quarter of the iterations of Jacobi-CG'''
    A, free = problem('laplace')
    n = A.shape[0]
    levels = reference('laplace', coarse)
    assert len(levels) == (3 if coarse == 16 else 2)
    b = numpy.random.default_rng(4).normal(size=n)
    x0 = numpy.where(free, 0., 1 + .1 * numpy.arange(n))
    r0 = numpy.linalg.norm((b - A @ x0)[free])
    stop_rr = (1e-10 * r0) ** 2
    x, it, starts, outcome = pcg_reference(A, b, x0, free, lambda r: cycle(levels, r), stop_rr, n)
    _, it_jacobi, _, outcome_jacobi = cg_reference(A, b, x0, free, numpy.where(free, 1 / A.diagonal(), 0.), stop_rr, n, check=1)
    print(f'coarse={coarse}: levels {[lv.nfree for lv in levels]}, {it} iterations, Jacobi-CG {it_jacobi}')
    assert outcome == 'converged' and outcome_jacobi == 'converged'
    assert 4 * it <= it_jacobi
    assert numpy.array_equal(x[~free], x0[~free])
    res = numpy.linalg.norm((b - A @ x)[free])
    assert res <= 1e-10 * r0 * (1 + 1e-3)
    direct = x0.copy()
    direct[free] += scipy.sparse.linalg.spsolve(A[free][:, free].tocsc(), (b - A @ x0)[free])
    lmin = numpy.linalg.eigvalsh(A.toarray()[free][:, free])[0]
    assert numpy.linalg.norm(x - direct) <= res / lmin * (1 + 1e-6)


def test_solve_argument_errors():
    '''raised before anything touches a device (there is none here)'''
    from nutils_amd import matrix
    A = matrix.HipMatrix(numpy.array([2., 3.]), numpy.array([0, 1, 2]), numpy.array([0, 1]), 2)
    b = numpy.ones(2)
    for solver in ('bicgstab', 'fgmres'):
        with pytest.raises(matrix.MatrixError, match='invalid preconditioner'):
            A.solve(b, solver=solver, rtol=1e-8, precon='amg')
    with pytest.raises(matrix.MatrixError, match='invalid preconditioner'):
        A.solve(b, solver='cg', rtol=1e-8, precon='ilu')
    for bad, message in ((dict(coarse=0), 'coarse must be'), (dict(coarse=1025), 'coarse must be'), (dict(coarse=16.), 'coarse must be'), (dict(coarse=True), 'coarse must be'),
                         (dict(sweeps=0), 'sweeps must be'), (dict(sweeps=1.5), 'sweeps must be'), (dict(sweeps='2'), 'sweeps must be'),
                         (dict(levels=3), 'invalid arguments'), (dict(coarse=16, cycle='W'), 'invalid arguments')):
        with pytest.raises(matrix.MatrixError, match=message):
            A.solve(b, solver='cg', rtol=1e-8, precon='amg', preconargs=bad)
    for precon in ('diag', None):  # (arguments that nothing would read are an error, not ignored)
        with pytest.raises(matrix.MatrixError, match='preconargs are the arguments of'):
            A.solve(b, solver='cg', rtol=1e-8, precon=precon, preconargs=dict(coarse=16))
    assert A._dev is None  # nothing was uploaded


def test_dense_block_of_a_masked_level():
    '''far fewer free dofs than rows (the constraints projection of solver.System: the boundary support is free, everything else held): the dense level selects
    its free block from the pattern, nfree^2 entries at the most, renumbered'''
    import torch
    from nutils_amd import amg
    A, _ = problem('laplace')
    n = A.shape[0]
    free = numpy.zeros(n, dtype=bool)
    free[numpy.random.default_rng(7).choice(n, 60, replace=False)] = True
    free[100:140] = True  # (some of them neighbours)
    levels = amg.symbolic(torch.from_numpy(A.indptr.astype(numpy.int64)), torch.from_numpy(A.indices.astype(numpy.int64)), torch.from_numpy(free), 256)
    assert [lv.kind for lv in levels] == ['dense']
    lv, nfree = levels[0], int(free.sum())
    assert lv.nfree == nfree and lv.dk.numel() <= nfree ** 2 and lv.dk.numel() < A.nnz // 10
    dense = numpy.zeros((nfree, nfree))
    dense[lv.drow.numpy(), lv.dcol.numpy()] = A.data[lv.dk.numpy()]
    idx = numpy.flatnonzero(free)
    assert numpy.array_equal(lv.idx32.numpy(), idx)
    assert numpy.array_equal(dense, A.toarray()[numpy.ix_(idx, idx)])
