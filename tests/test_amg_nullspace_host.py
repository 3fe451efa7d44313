'''CPU-side checks of the AMG preconditioner with a user-given near-nullspace (preconargs=dict(nullspace=B), nutils_amd/amg.py, nh_aggregate_qr of
nh_amg.hip), on top of the restatement of tests/test_amg_host.py: the aggregate-wise QR, the node graph of the coarse levels, the k-column tentative
prolongator and the Galerkin products restated in numpy, in float64 or longdouble, with their invariants pinned; the symbolic phase of nutils_amd.amg on
CPU tensors, integer for integer against that restatement; the rigid-body modes against elasticity matrices assembled here; and the argument errors.  The
restatement is the CPU reference of tests/test_gpu_amg_nullspace.py.'''
import functools
import itertools
import types
import numpy
import pytest
import scipy.sparse

from test_amg_host import aggregate, free_part, structure, cycle, pcg_reference, problem as scalar_problem

ld = numpy.longdouble


# ---- the algorithm, restated ---------------------------------------------------------------------------------------------

def aggregate_qr(mptr, midx, k, B, dtype=float):
    '''(Q, Rc, dropped): the thin QR of B on the rows midx[mptr[a] : mptr[a + 1]] of every aggregate a, all aggregates at once, in the arithmetic `dtype`;
    sums run over the rows of an aggregate in the order of the list.  Columns left to right: n0, two passes of modified Gram-Schmidt against the finished
    columns, n1, dropped if n1 <= 2^-26 n0.'''
    nagg = len(mptr) - 1
    seg = numpy.repeat(numpy.arange(nagg), numpy.diff(mptr))
    V = B[midx].astype(dtype).reshape(len(midx), k)

    def total(x):
        out = numpy.zeros(nagg, dtype=dtype)
        numpy.add.at(out, seg, x)
        return out
    R, dropped = numpy.zeros((nagg, k, k), dtype=dtype), numpy.zeros((nagg, k), dtype=bool)
    for j in range(k):
        n0 = numpy.sqrt(total(V[:, j] ** 2))
        for _ in range(2):
            for l in range(j):
                c = total(V[:, l] * V[:, j])
                V[:, j] -= c[seg] * V[:, l]
                R[:, l, j] += c
        n1 = numpy.sqrt(total(V[:, j] ** 2))
        drop = n1 <= dtype(2.) ** -26 * n0
        V[:, j] = numpy.where(drop[seg], 0, V[:, j] / numpy.where(drop, 1, n1)[seg])
        R[:, j, j] = numpy.where(drop, 0, n1)
        dropped[:, j] = drop
    Q = numpy.zeros((len(B), k), dtype=dtype)
    Q[midx] = V
    return Q, R.reshape(nagg * k, k), dropped


def keys_of(M):
    '''row * ncols + col of the entries of a CSR matrix with sorted indices, ascending'''
    return numpy.repeat(numpy.arange(M.shape[0]), numpy.diff(M.indptr)) * M.shape[1] + M.indices


def on(pattern, M, m):
    '''the values m of M's entries, placed on the entries of `pattern` (which has them all), 0 elsewhere'''
    pkey = keys_of(pattern)
    pos = numpy.searchsorted(pkey, keys_of(M))
    assert pos.max(initial=-1) < len(pkey) and numpy.array_equal(pkey[pos], keys_of(M))
    out = numpy.zeros(len(pkey), dtype=m.dtype)
    out[pos] = m
    return out


def spmm(A, a, B, b, pattern):
    '''the values of A B on the entries of `pattern` (CSR, sorted, containing the product's) from the values a and b of the patterns A and B, in their
    arithmetic: the products listed row by row and summed in that order'''
    cnt = numpy.diff(B.indptr)[A.indices]
    src = numpy.repeat(numpy.arange(A.nnz), cnt)
    m = B.indptr[A.indices][src] + numpy.arange(len(src)) - (numpy.cumsum(cnt) - cnt)[src]
    key = numpy.repeat(numpy.arange(A.shape[0]), numpy.diff(A.indptr))[src] * B.shape[1] + B.indices[m]
    pkey = keys_of(pattern)
    pos = numpy.searchsorted(pkey, key)
    assert numpy.array_equal(pkey[pos], key)
    out = numpy.zeros(len(pkey), dtype=numpy.result_type(a, b))
    numpy.add.at(out, pos, a[src] * b[m])
    return out


def csr(data, pattern):
    return scipy.sparse.csr_matrix((numpy.asarray(data, dtype=float), pattern.indices, pattern.indptr), pattern.shape)


def sorted_csr(M):
    M = M.tocsr()
    M.sort_indices()
    return M


def level(A, free, coarse, B, nodesize, dtype=float):
    '''one level of the hierarchy with the near-nullspace B [n x k] from its matrix, in the arithmetic `dtype`: what `level` of test_amg_host gives (the
    matrices as float64 CSR), and nagg, mptr, midx, dropped, T; `x` holds the values q, p, ac, rc in `dtype`.  nodesize: 1 on level 0, k below.'''
    n, k = B.shape
    lv = types.SimpleNamespace(A=A, free=free, n=n, nfree=int(free.sum()), B=B, k=k, nodesize=nodesize)
    diag = A.diagonal()
    assert nodesize > 1 or (diag[free] != 0).all()
    dinv = numpy.where(free & (diag != 0), 1 / numpy.where(diag == 0, 1, diag).astype(dtype), 0)
    lv.dinv = dinv.astype(float)
    if lv.nfree <= coarse:
        lv.kind = 'dense'
        lv.idx = numpy.flatnonzero(free)
        lv.ainv = numpy.linalg.pinv(A.toarray()[numpy.ix_(lv.idx, lv.idx)], hermitian=True)
        return lv
    lv.Af = Af = free_part(A, free)
    if nodesize == 1:
        lv.agg, roots, lv.rounds = aggregate(A, free)
    else:
        node = numpy.arange(n) // nodesize
        N = scipy.sparse.csr_matrix((numpy.ones(n), (numpy.arange(n), node)), (n, n // nodesize))
        nodeagg, roots, lv.rounds = aggregate(sorted_csr(N.T @ structure(A) @ N), numpy.ones(n // nodesize, dtype=bool))
        lv.agg = nodeagg[node]
    lv.nagg, lv.nc = len(roots), len(roots) * k
    if lv.nagg * nodesize == lv.nfree:
        lv.kind = 'diagonal'
        return lv
    lv.kind = 'coarsen'
    af = Af.data.astype(dtype)
    absrow = numpy.zeros(n, dtype=dtype)
    numpy.add.at(absrow, numpy.repeat(numpy.arange(n), numpy.diff(Af.indptr)), abs(af))
    rho = (absrow * dinv).max()
    omega = 4 / (3 * rho)
    w = omega * dinv
    lv.rho, lv.omega, lv.w = float(rho), float(omega), w.astype(float)
    idx = numpy.flatnonzero(free)
    order = numpy.argsort(lv.agg[idx], kind='stable')
    lv.midx = idx[order]
    lv.mptr = numpy.searchsorted(lv.agg[idx][order], numpy.arange(lv.nagg + 1))
    q, rc, lv.dropped = aggregate_qr(lv.mptr, lv.midx, k, B, dtype)
    # T: row i of a free dof has the k entries agg(i) k + j; rows ascending, j ascending within: the order of a sorted CSR
    T = scipy.sparse.csr_matrix((numpy.ones(len(idx) * k), (numpy.repeat(idx, k), (lv.agg[idx][:, None] * k + numpy.arange(k)).ravel())), (n, lv.nc))
    assert T.has_sorted_indices and T.nnz == len(idx) * k
    t = q[idx].ravel()
    S = structure(Af)
    ppat = sorted_csr(S @ T)
    at = spmm(Af, af, T, t, ppat)
    p = on(ppat, T, t) - w[numpy.repeat(numpy.arange(n), numpy.diff(ppat.indptr))] * at
    perm = sorted_csr(csr(numpy.arange(1, ppat.nnz + 1), ppat).T)
    rpat, r = structure(perm), p[perm.data.astype(int) - 1]
    appat = sorted_csr(S @ structure(ppat))
    ap = spmm(Af, af, ppat, p, appat)
    acpat = sorted_csr(rpat @ appat)
    ac = spmm(rpat, r, appat, ap, acpat)
    lv.x = types.SimpleNamespace(q=q, p=p, ac=ac, rc=rc)
    lv.T, lv.Q, lv.Rc = csr(t, T), q.astype(float), rc.astype(float)
    lv.AT, lv.P, lv.R, lv.AP, lv.Ac = csr(at, ppat), csr(p, ppat), csr(r, rpat), csr(ap, appat), csr(ac, acpat)
    return lv


def hierarchy(A, free, B, coarse=256):
    levels, nodesize = [], 1
    while True:
        lv = level(A, free, coarse, B, nodesize)
        levels.append(lv)
        if lv.kind != 'coarsen':
            return levels
        A, free, B, nodesize = lv.Ac, numpy.ones(lv.nc, dtype=bool), lv.Rc, lv.k


# ---- problems ------------------------------------------------------------------------------------------------------------

def vertices(shape, seed=0):
    '''the vertices of workloads.quad_form / hex1_form: the unit grid, last axis fastest, perturbed by up to 0.2'''
    verts = numpy.stack(numpy.meshgrid(*[numpy.arange(n + 1.) for n in shape], indexing='ij'), -1).reshape(-1, len(shape))
    return verts + numpy.random.default_rng(seed).uniform(-.2, .2, verts.shape)


def elasticity(shape, seed=0, lam=1., mu=.65):
    '''(K, coords): the stiffness matrix of linear elasticity on multilinear elements over the perturbed unit grid, 2 x .. x 2 Gauss points, no dof held;
    dof = node d + component, nodes with the last axis fastest'''
    d = len(shape)
    coords = vertices(shape, seed)
    corners = numpy.array(list(itertools.product([0, 1], repeat=d)))
    strides = numpy.array([int(numpy.prod([n + 1 for n in shape[a + 1:]])) for a in range(d)])
    elems = numpy.array(list(itertools.product(*[range(n) for n in shape])))
    conn = ((elems[:, None, :] + corners[None]) * strides).sum(-1)
    X = coords[conn]  # [elements, corners, d]
    Ke = numpy.zeros((len(conn), 2 ** d, d, 2 ** d, d))
    for xi in itertools.product(.5 + numpy.array([-.5, .5]) / numpy.sqrt(3), repeat=d):
        factor = numpy.where(corners == 1, xi, 1 - numpy.array(xi))  # [corners, d]
        dN = numpy.stack([numpy.where(corners[:, b] == 1, 1., -1.) * numpy.prod(numpy.delete(factor, b, axis=1), axis=1) for b in range(d)], -1)
        J = numpy.einsum('eac,ab->ecb', X, dN)
        G = numpy.einsum('ab,ebc->eac', dN, numpy.linalg.inv(J))  # the physical gradients
        wdet = numpy.linalg.det(J) / 2 ** d
        assert (wdet > 0).all()
        Ke += wdet[:, None, None, None, None] * (lam * numpy.einsum('eai,ebj->eaibj', G, G) + mu * numpy.einsum('eaj,ebi->eaibj', G, G)
                                                  + mu * numpy.einsum('eac,ebc,ij->eaibj', G, G, numpy.eye(d)))
    dof = conn[:, :, None] * d + numpy.arange(d)
    rows = numpy.broadcast_to(dof[:, :, :, None, None], Ke.shape)
    cols = numpy.broadcast_to(dof[:, None, None, :, :], Ke.shape)
    K = sorted_csr(scipy.sparse.csr_matrix((Ke.ravel(), (rows.ravel(), cols.ravel())), (len(coords) * d,) * 2))
    return K, coords


@functools.lru_cache(maxsize=None)
def problem(name):
    '''(A, free, B): 'laplace', 'chain' and 'orphan' of test_amg_host with B = [1, x, y] and [1, x]; 'elasticity': 12 x 10 elements, the face x = 0 held, the
    three rigid-body modes.  B is what `amg.check_args` makes of the argument of a solve.  Made once, never written.'''
    from nutils_amd import amg
    if name == 'elasticity':
        A, coords = elasticity((12, 10))
        free = numpy.ones((13, 11, 2), dtype=bool)
        free[0] = False
        free, B = free.ravel(), amg.rigid_body_modes(coords)
    else:
        A, free = scalar_problem(name)
        n = A.shape[0]
        if name == 'laplace':
            x, y = numpy.meshgrid(numpy.linspace(0, 1, 40), numpy.linspace(0, 2, 37), indexing='ij')
            B = numpy.stack([numpy.ones(n), x.ravel(), y.ravel()], 1)
        else:
            B = numpy.stack([numpy.ones(n), numpy.arange(n) / n], 1)
    coarse, sweeps, checked = amg.check_args(dict(nullspace=B), A.shape[0])
    assert checked.shape == B.shape and numpy.array_equal(checked, B)
    return A, free, checked


CASES = [('laplace', 16), ('chain', 256), ('orphan', 16), ('elasticity', 32)]


@functools.lru_cache(maxsize=None)
def reference(name, coarse):
    A, free, B = problem(name)
    return hierarchy(A, free, B, coarse)


def symbolic(name, coarse):
    import torch
    from nutils_amd import amg
    A, free, B = problem(name)
    return amg.symbolic(torch.from_numpy(A.indptr.astype(numpy.int64)), torch.from_numpy(A.indices.astype(numpy.int64)), torch.from_numpy(free), coarse, B.shape[1])


# ---- tests ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,coarse', CASES)
def test_symbolic_phase_matches_the_restatement(name, coarse):
    '''aggregates, members and the patterns of P, R and A_c, integer for integer and level by level; the map from P into T's value array finds T; a rebuild
    gives the same integers'''
    ref, got, again = reference(name, coarse), symbolic(name, coarse), symbolic(name, coarse)
    k = problem(name)[2].shape[1]
    print(f'{name}: k = {k}, levels {[lv.nfree for lv in ref]}, kinds {[lv.kind for lv in ref]}, dropped columns {[int(lv.dropped.sum()) for lv in ref if lv.kind == "coarsen"]}')
    assert [lv.kind for lv in got] == [lv.kind for lv in ref] and len(ref) >= 2
    assert [(lv.n, lv.nfree, lv.nodesize) for lv in got] == [(lv.n, lv.nfree, lv.nodesize) for lv in ref]
    same = lambda tensor, array: numpy.array_equal(tensor.numpy(), array)
    for r, g, h in zip(ref, got, again):
        assert same(g.rowptr, r.A.indptr) and same(g.colidx, r.A.indices) and g.k == k
        if r.kind != 'coarsen':
            continue
        assert g.nagg == r.nagg and g.nc == r.nc == r.nagg * k and same(g.agg, r.agg) and g.rounds == r.rounds
        assert same(g.mptr, r.mptr) and same(g.midx, r.midx)
        assert same(g.prowptr, r.P.indptr) and same(g.pcol, r.P.indices)
        assert same(g.rrowptr, r.R.indptr) and same(g.rcol, r.R.indices)
        tmap = g.tmap.numpy()
        assert numpy.array_equal(tmap >= 0, on(r.P, r.T, numpy.ones(r.T.nnz)) > 0)
        assert numpy.array_equal(numpy.where(tmap >= 0, r.Q.ravel()[numpy.maximum(tmap, 0)], 0.), on(r.P, r.T, r.T.data))
        for name_ in ('agg', 'mptr', 'midx', 'tmap', 'prowptr', 'pcol', 'rrowptr', 'rcol', 'rperm'):
            assert numpy.array_equal(getattr(g, name_).numpy(), getattr(h, name_).numpy())
        for plan in ('at', 'ap', 'rap'):
            for name_ in ('ptr', 'ia', 'ib'):
                assert numpy.array_equal(getattr(getattr(g, plan), name_).numpy(), getattr(getattr(h, plan), name_).numpy())
    if name == 'orphan':  # two singleton aggregates: their second column has nothing left after the first
        assert ref[0].dropped.sum() == 2 and (numpy.diff(ref[0].mptr)[ref[0].dropped[:, 1]] == 1).all()


@pytest.mark.parametrize('name,coarse', CASES)
def test_plans_reproduce_the_products(name, coarse):
    '''A_f T (two factors), A_f P and P^T A_f P from the plans of nutils_amd.amg, summed in numpy on the restatement's values, against the restatement's own
    products: the same terms in another order, compared with the sum of their magnitudes'''
    from test_amg_host import segment_dot
    from test_cg_host import gamma
    for r, g in zip(reference(name, coarse), symbolic(name, coarse)):
        if r.kind != 'coarsen':
            continue
        a = r.A.data
        for what, plan, fa, fb, expect in (('A T', g.at, a, r.Q.ravel(), r.AT), ('A P', g.ap, a, r.P.data, r.AP), ('R A P', g.rap, r.R.data, r.AP.data, r.Ac)):
            ptr, ia, ib = plan.ptr.numpy(), plan.ia.numpy(), plan.ib.numpy()
            rows = numpy.repeat(numpy.arange(expect.shape[0]), numpy.diff(expect.indptr))
            assert numpy.array_equal(plan.rows.numpy(), rows) and numpy.array_equal(plan.cols.numpy(), expect.indices)
            err = abs(segment_dot(ptr, ia, ib, fa, fb) - expect.data)
            bound = gamma(numpy.diff(ptr) + 2) * segment_dot(ptr, ia, ib, abs(fa), abs(fb))
            assert (err <= bound).all(), what
        assert numpy.array_equal(r.P.data[g.rperm.numpy()], r.R.data)


@pytest.mark.parametrize('name,coarse', CASES)
def test_qr_invariants(name, coarse):
    '''per aggregate Q^T Q is the identity on the kept columns and 0 on the dropped ones, R is upper triangular with a non-negative diagonal that is 0 exactly
    where the column was dropped, and T Rc = B on the free rows'''
    for lv in reference(name, coarse):
        if lv.kind != 'coarsen':
            continue
        k = lv.k
        gram = (lv.T.T @ lv.T).toarray()
        expect = numpy.diag((~lv.dropped).ravel().astype(float))
        assert abs(gram - expect).max() <= 64 * numpy.finfo(float).eps
        R = lv.Rc.reshape(lv.nagg, k, k)
        assert not numpy.tril(R, -1).any() and (numpy.diagonal(R, axis1=1, axis2=2) >= 0).all()
        assert numpy.array_equal(numpy.diagonal(R, axis1=1, axis2=2) == 0, lv.dropped)
        assert not lv.Q[lv.dropped[numpy.maximum(lv.agg, 0)] & (lv.agg >= 0)[:, None]].any()
        assert not lv.Q[~lv.free].any()
        err = abs(lv.T @ lv.Rc - lv.B)[lv.free]
        print(f'{name} level {lv.n}: {lv.nagg} aggregates of {numpy.diff(lv.mptr).min()} .. {numpy.diff(lv.mptr).max()} dofs, |T Rc - B| = {err.max():.2e}, |B| = {abs(lv.B).max():.2e}')
        assert err.max() <= 64 * numpy.finfo(float).eps * abs(lv.B).max()


@pytest.mark.parametrize('name,coarse', [('laplace', 16), ('elasticity', 32)])
def test_cycle_is_symmetric_positive_definite(name, coarse):
    '''M assembled densely by applying the cycle to the unit vectors, as in test_amg_host'''
    A, free, B = problem(name)
    levels = reference(name, coarse)
    assert len(levels) >= 3
    for sweeps in (1, 2):
        M = cycle(levels, numpy.eye(A.shape[0]), sweeps)
        scale = abs(M).max()
        print(f'{name}, sweeps={sweeps}: |M - M^T| / |M| = {abs(M - M.T).max() / scale:.2e}')
        assert abs(M - M.T).max() <= 1e-12 * scale
        assert not M[~free].any() and not M[:, ~free].any()
        assert numpy.linalg.eigvalsh(M[free][:, free])[0] > 0


def iterations(A, free, levels, seed=4, rtol=1e-8):
    n = A.shape[0]
    b = numpy.random.default_rng(seed).normal(size=n)
    x0 = numpy.zeros(n)
    stop_rr = (rtol * numpy.linalg.norm(b[free])) ** 2
    x, it, starts, outcome = pcg_reference(A, b, x0, free, lambda r: cycle(levels, r), stop_rr, n)
    assert outcome == 'converged' and numpy.linalg.norm((b - A @ x)[free]) <= rtol * numpy.linalg.norm(b[free]) * (1 + 1e-3)
    return it


def test_pcg_of_the_restatement():
    '''elasticity: the rigid-body modes need at most half the iterations of the constant; 'orphan' with its dropped columns converges'''
    from test_amg_host import hierarchy as constant_hierarchy
    from nutils_amd import amg
    A, coords = elasticity((48, 48))
    free = numpy.ones((49, 49, 2), dtype=bool)
    free[0] = False
    free = free.ravel()
    levels = hierarchy(A, free, amg.rigid_body_modes(coords), 64)
    it, it_constant = iterations(A, free, levels), iterations(A, free, constant_hierarchy(A, free, 64))
    print(f'elasticity 48 x 48: levels {[lv.nfree for lv in levels]}, {it} iterations with the rigid-body modes, {it_constant} with the constant')
    assert len(levels) == 3 and 2 * it <= it_constant
    A, free, B = problem('orphan')
    it = iterations(A, free, reference('orphan', 16))
    print(f'orphan: {it} iterations')
    assert it <= 30


@pytest.mark.parametrize('shape', [(5, 4), (3, 4, 2)])
def test_rigid_body_modes(shape):
    '''translations, then rotations, in the layout dof = node d + component: the unconstrained stiffness matrix takes them to rounding'''
    from nutils_amd import amg
    K, coords = elasticity(shape)
    d = len(shape)
    B = amg.rigid_body_modes(coords)
    assert B.shape == (len(coords) * d, d * (d + 1) // 2) and B.dtype == float
    for c in range(d):
        assert numpy.array_equal(B[:, c].reshape(-1, d), numpy.broadcast_to(numpy.eye(d)[c], (len(coords), d)))
    assert numpy.linalg.matrix_rank(B) == B.shape[1]
    err = abs(K @ B).max()
    print(f'{d}-D: |K B| = {err:.2e}, |K| |B| = {(abs(K) @ abs(B)).max():.2e}')
    assert err <= 64 * numpy.finfo(float).eps * (abs(K) @ abs(B)).max()
    assert abs(K @ B[:, ::-1].cumsum(1)).max() <= 64 * numpy.finfo(float).eps * (abs(K) @ abs(B)).max() * B.shape[1]
    with pytest.raises(Exception, match='coords must have the shape'):
        amg.rigid_body_modes(numpy.zeros((4, 1)))


def test_argument_errors():
    '''raised before anything touches a device (there is none here)'''
    import torch
    from nutils_amd import amg, matrix
    A = matrix.HipMatrix(numpy.array([2., 3.]), numpy.array([0, 1, 2]), numpy.array([0, 1]), 2)
    b = numpy.ones(2)
    for bad, message in ((numpy.ones((3, 2)), 'nullspace must have the shape'), (numpy.ones((2, 2, 1)), 'nullspace must have the shape'), (numpy.ones(3), 'nullspace must have the shape'),
                         (numpy.ones((2, 7)), 'nullspace must have between 1 and 6'), (numpy.ones((2, 0)), 'nullspace must have between 1 and 6'),
                         (numpy.array([[1., numpy.nan], [0., 1.]]), 'nullspace has non-finite'), (numpy.array([1., numpy.inf]), 'nullspace has non-finite'),
                         (numpy.ones((2, 2), dtype=numpy.float32), 'nullspace must be float64'), (numpy.ones((2, 2), dtype=int), 'nullspace must be float64'),
                         (torch.ones((2, 7), dtype=torch.float64), 'nullspace must have between 1 and 6'), (torch.ones(2, dtype=torch.float32), 'nullspace must be float64'),
                         (torch.tensor([1., float('nan')], dtype=torch.float64), 'nullspace has non-finite'), ('rigid', 'nullspace must be')):
        with pytest.raises(matrix.MatrixError, match=message):
            A.solve(b, solver='cg', rtol=1e-8, precon='amg', preconargs=dict(nullspace=bad))
    with pytest.raises(matrix.MatrixError, match="invalid arguments \\['nullspaces'\\].*'nullspace'"):
        A.solve(b, solver='cg', rtol=1e-8, precon='amg', preconargs=dict(nullspaces=numpy.ones(2)))
    assert A._dev is None  # nothing was uploaded
    coarse, sweeps, B = amg.check_args(dict(nullspace=numpy.ones(5)), 5)
    assert (coarse, sweeps) == (256, 1) and B.shape == (5, 1)
    assert amg.check_args(None) == (256, 1, None) and amg.check_args(dict(coarse=8, nullspace=None)) == (8, 1, None)
    levels = amg.symbolic(torch.tensor([0, 1, 2]), torch.tensor([0, 1]), None, 1, 2)
    with pytest.raises(matrix.MatrixError, match='near-nullspace of 2 vectors'):
        amg.Hierarchy(levels, None, 1, None)
