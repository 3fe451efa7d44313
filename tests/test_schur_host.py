'''CPU-side checks of the block preconditioner for saddle-point systems (matrix.HipMatrix.getprecon('schur'), solve(solver='fgmres', precon=M), nh_schur_*,
nh_csr_schur_diagonal, nh_fgmres_iterate_schur): a numpy restatement of the preconditioner (`block_solve`, `restated`: the inverse Schur diagonal, the masked
product, test_amg_host.cycle on test_fgmres_amg_host.general_hierarchy of K with the first field's free dofs as the mask, the sum) pinned to the definition --
with an exact first block and the exact Schur complement flexible GMRES is there in two steps --, its step counts against the identity, the errors raised
before any device work, System.trialmask, and what the C ABI refuses.  `problem`, `restated` and `reference_steps` are the CPU reference of
tests/test_gpu_schur.py.'''
import ctypes
import functools
import types
import numpy
import pytest
import scipy.sparse

from nutils_amd import _lib, amg, matrix
import test_amg_host
from test_bicgstab_host import refused, csr, P
from test_fgmres_amg_host import fgmres_reference, general_hierarchy, handle
from test_minres_host import saddle

RTOL = 1e-10
RESTART = 30
COARSE = 40


# ---- problems ------------------------------------------------------------------------------------------------------------

def stokes(nx, ny):
    '''(K, cons, second): the staggered-grid Stokes matrix [[A, Bt], [B, 0]] on nx x ny cells of the unit square: u on the (nx + 1) ny vertical faces, v on the
    nx (ny + 1) horizontal ones, p on the nx ny cells, in that order, the second index fastest; A the 5-point Laplacians of u and v, B the first differences of
    the divergence, all scaled by hx hy.  The boundary faces (u on the left and right side, v on the bottom and top) and the first pressure dof are held at 0.5.'''
    hx, hy = 1 / nx, 1 / ny
    eye, kron = scipy.sparse.identity, scipy.sparse.kron
    lap = lambda n, h: scipy.sparse.diags([-numpy.ones(n - 1), 2 * numpy.ones(n), -numpy.ones(n - 1)], [-1, 0, 1]) / h ** 2
    diff = lambda n, h: scipy.sparse.diags([-numpy.ones(n), numpy.ones(n)], [0, 1], shape=(n, n + 1)) / h
    Au = kron(lap(nx + 1, hx), eye(ny)) + kron(eye(nx + 1), lap(ny, hy))
    Av = kron(lap(nx, hx), eye(ny + 1)) + kron(eye(nx), lap(ny + 1, hy))
    B = scipy.sparse.hstack([kron(diff(nx, hx), eye(ny)), kron(eye(nx), diff(ny, hy))])
    K = scipy.sparse.csr_matrix(scipy.sparse.bmat([[scipy.sparse.block_diag([Au, Av]), B.T], [B, None]]) * (hx * hy))
    K.sort_indices()
    nu, nv, npr = (nx + 1) * ny, nx * (ny + 1), nx * ny
    hold_u, hold_v, hold_p = numpy.zeros((nx + 1, ny), dtype=bool), numpy.zeros((nx, ny + 1), dtype=bool), numpy.zeros(npr, dtype=bool)
    hold_u[0] = hold_u[-1] = hold_v[:, 0] = hold_v[:, -1] = hold_p[0] = True
    cons = numpy.where(numpy.concatenate([hold_u.ravel(), hold_v.ravel(), hold_p]), .5, numpy.nan)
    second = numpy.arange(nu + nv + npr) >= nu + nv
    return K, cons, second


def large(n1=200000):
    '''(K, cons, second): a tridiagonal first block (-1, 4, -1) of n1 rows and a three-point B whose row i has (1, .5, -1) in the columns 3 i, 3 i + 1, 3 i + 2 (as
    far as they exist): 200 000 + 66 667 rows, more than the 262 144 a grid of 1024 workgroups covers at once.  Every 1000th dof is held at 0.5.'''
    n2 = (n1 + 2) // 3
    A = scipy.sparse.diags([-numpy.ones(n1 - 1), numpy.full(n1, 4.), -numpy.ones(n1 - 1)], [-1, 0, 1])
    rows = numpy.repeat(numpy.arange(n2), 3)
    cols = 3 * rows + numpy.tile(numpy.arange(3), n2)
    keep = cols < n1
    B = scipy.sparse.csr_matrix((numpy.tile([1., .5, -1.], n2)[keep], (rows[keep], cols[keep])), (n2, n1))
    K = scipy.sparse.csr_matrix(scipy.sparse.bmat([[A, B.T], [B, None]]))
    K.sort_indices()
    cons = numpy.full(n1 + n2, numpy.nan)
    cons[::1000] = .5
    return K, cons, numpy.arange(n1 + n2) >= n1


@functools.lru_cache(maxsize=None)
def problem(name):
    '''A namespace: K (scipy CSR), cons, second, free, f1, f2, rhs, start (held dofs at their values, zero elsewhere), r0.  'saddle': test_minres_host.saddle
    (120 + 40 rows); 'stokes8x7' (183 rows), 'stokes16x15' (751); 'large' (266 667).  Made once, never written.'''
    p = types.SimpleNamespace(name=name)
    if name == 'saddle':
        p.K, p.cons, p.rhs = saddle()
        p.second = numpy.arange(160) >= 120
    else:
        p.K, p.cons, p.second = large() if name == 'large' else stokes(*{'stokes8x7': (8, 7), 'stokes16x15': (16, 15)}[name])
        p.rhs = numpy.random.default_rng(11).normal(size=p.K.shape[0])
    p.free, p.start = matrix.constraints(p.K.shape[0], p.cons)
    p.f1, p.f2 = p.free & ~p.second, p.free & p.second
    p.r0 = numpy.linalg.norm((p.rhs - p.K @ p.start)[p.free])
    return p


# ---- the preconditioner, restated ------------------------------------------------------------------------------------------

def simple_diagonal(K, f1, dtype=float):
    '''shat_i = K_ii - sum over j in f1 of K_ij K_ji / K_jj, for every row i, in the arithmetic of `dtype`'''
    K = K.tocsr()
    d = K.diagonal().astype(dtype)
    dinv = numpy.where(f1, 1 / numpy.where(d == 0, 1, d), 0)
    coo = K.tocoo()  # (in the order of the value array)
    KT = K.T.tocsr()
    KT.sort_indices()
    assert numpy.array_equal(KT.indptr, K.indptr) and numpy.array_equal(KT.indices, K.indices)  # structurally symmetric: K_ji lies where K_ij does
    s = numpy.zeros(K.shape[0], dtype=dtype)
    numpy.add.at(s, coo.row, K.data.astype(dtype) * KT.data.astype(dtype) * dinv[coo.col])
    return d - s


def block_solve(K, f1, f2, first, schur):
    '''r -> z of the block upper-triangular solve on full-length vectors: z2 = schur(r) on f2 (0 elsewhere), t = f1(r - K z2), z1 = first(t), z = z1 + z2;
    `first` and `schur` take and return full-length vectors that vanish outside f1 and f2'''
    def M(r):
        z2 = schur(r)
        t = numpy.where(f1, r - K @ z2, 0.)
        return first(t) + z2
    return M


def restated(K, free, second, coarse=COARSE, shat=None, levels=None):
    '''the preconditioner as the device applies it: sinv = where(f2, 1 / shat, 0) with shat the SIMPLE diagonal unless given, the cycle of
    general_hierarchy(K, f1, coarse)'''
    f1, f2 = free & ~second, free & second
    shat = simple_diagonal(K, f1) if shat is None else shat
    assert (shat[f2] != 0).all() and numpy.isfinite(shat[f2]).all()
    sinv = numpy.where(f2, 1 / numpy.where(f2, shat, 1.), 0.)
    levels = general_hierarchy(K, f1, coarse) if levels is None else levels
    return block_solve(K, f1, f2, lambda t: test_amg_host.cycle(levels, t), lambda r: sinv * r)


@functools.lru_cache(maxsize=None)
def reference_steps(name, precon='schur'):
    '''Arnoldi steps of the restated solve to RTOL at restart 30, `check=1`: precon 'schur' (`restated`) or 'identity', whose cap is 20 n steps and counts
    when it is reached'''
    p = problem(name)
    n = p.K.shape[0]
    M = restated(p.K, p.free, p.second) if precon == 'schur' else (lambda r: r)
    x, it, outcome, _ = fgmres_reference(p.K, p.rhs, p.start, p.free, M, (RTOL * p.r0) ** 2, RESTART, 20 * n if precon == 'identity' else int(p.free.sum()), check=1)
    if precon == 'schur':
        assert outcome == 'converged', (name, outcome, it)
        assert numpy.linalg.norm((p.rhs - p.K @ x)[p.free]) <= RTOL * p.r0 * (1 + 1e-3)
    else:
        assert outcome in ('converged', 'maxiter')
    return it


def test_problem_sizes():
    assert [problem(name).K.shape[0] for name in ('saddle', 'stokes8x7', 'stokes16x15')] == [160, 183, 751]
    K, cons, second = large(2000)
    assert K.shape == (2667, 2667) and second.sum() == 667 and K[2666].nnz == 2
    for name in ('saddle', 'stokes8x7', 'stokes16x15'):
        p = problem(name)
        assert abs(p.K - p.K.T).max() == 0 and not p.K.diagonal()[p.second].any() and p.f1.any() and p.f2.any() and (~p.free & ~p.second).any()
        assert p.second[~p.free].any() == (name != 'saddle')  # (a held pressure dof on the Stokes grids)


def test_exact_blocks_converge_in_two_steps():
    '''with the inverse of the free first block in place of the cycle and the inverse of the exact Schur complement S = C - B A^-1 Bt in place of 1 / shat the
    preconditioned matrix K M is block lower triangular with identities on its diagonal, (K M - I)^2 = 0: flexible GMRES is there after two steps.  This pins
    the composition -- which block is solved first, the sign and the mask of the coupling product -- to the definition.'''
    p = problem('saddle')
    D = p.K.toarray()
    i1, i2 = numpy.flatnonzero(p.f1), numpy.flatnonzero(p.f2)
    A, Bt, B, C = D[numpy.ix_(i1, i1)], D[numpy.ix_(i1, i2)], D[numpy.ix_(i2, i1)], D[numpy.ix_(i2, i2)]
    Ainv = numpy.linalg.inv(A)
    Sinv = numpy.linalg.inv(C - B @ Ainv @ Bt)

    def on(idx, inverse):
        def apply(r):
            z = numpy.zeros_like(r)
            z[idx] = inverse @ r[idx]
            return z
        return apply
    M = block_solve(p.K, p.f1, p.f2, on(i1, Ainv), on(i2, Sinv))
    x, it, outcome, _ = fgmres_reference(p.K, p.rhs, p.start, p.free, M, (RTOL * p.r0) ** 2, RESTART, 160, check=1)
    res = numpy.linalg.norm((p.rhs - p.K @ x)[p.free])
    print(f'{it} steps, |r| / |r0| = {res / p.r0:.2e}')
    assert outcome == 'converged' and it == 2 and res <= RTOL * p.r0
    assert numpy.array_equal(x[~p.free], p.start[~p.free])
    # the other order of the blocks, or the coupling with the other sign, is not that preconditioner
    wrong = block_solve(-p.K, p.f1, p.f2, on(i1, Ainv), on(i2, Sinv))
    assert fgmres_reference(p.K, p.rhs, p.start, p.free, wrong, (RTOL * p.r0) ** 2, RESTART, 160, check=1)[1] > 2


@pytest.mark.parametrize('name', ['saddle', 'stokes8x7', 'stokes16x15'])
def test_step_counts(name):
    '''the restatement with the real pieces converges at rtol 1e-10, restart 30, coarse 40, in at most a quarter of the steps the identity takes (capped at
    20 n).  The counts the feature was proposed with: 51 / 406, 35 / 2690, 58 / 15 020 (the cap).'''
    p = problem(name)
    levels = general_hierarchy(p.K, p.f1, COARSE)
    steps, plain = reference_steps(name), reference_steps(name, 'identity')
    print(f'{name}: {p.K.shape[0]} rows, levels of the first block {[lv.nfree for lv in levels]}, {steps} steps with the block preconditioner, {plain} with the identity'
          + (' (the cap)' if plain == 20 * p.K.shape[0] else ''))
    assert 4 * steps <= plain


def perturbed(p):
    '''p.K with its first block changed to 1.05 A + 0.03 diag(A) (a Jacobian one step on, with a little more mass), on the same pattern'''
    coo = p.K.tocoo()
    block = ~p.second[coo.row] & ~p.second[coo.col]
    return scipy.sparse.csr_matrix((p.K.data * numpy.where(block, numpy.where(coo.row == coo.col, 1.08, 1.05), 1.), p.K.indices, p.K.indptr), p.K.shape)


@pytest.mark.parametrize('name', ['saddle', 'stokes8x7', 'stokes16x15'])
def test_lagged_preconditioner(name):
    '''the preconditioner of K on a matrix whose first block has moved: within 1.5 x + 2 of the steps with its own, the bar for lagged 'amg' objects'''
    p = problem(name)
    K2 = perturbed(p)
    stop_rr = (RTOL * numpy.linalg.norm((p.rhs - K2 @ p.start)[p.free])) ** 2
    counts = []
    for K in (K2, p.K):
        x, it, outcome, _ = fgmres_reference(K2, p.rhs, p.start, p.free, restated(K, p.free, p.second), stop_rr, RESTART, int(p.free.sum()), check=1)
        assert outcome == 'converged'
        counts.append(it)
    print(f'{name}: lagged {counts[1]} steps, own {counts[0]}')
    assert counts[1] <= 1.5 * counts[0] + 2


def test_restatement_leaves_held_dofs_alone():
    '''z vanishes on held dofs whatever r holds there, and r there does not reach the free ones'''
    p = problem('stokes8x7')
    M = restated(p.K, p.free, p.second)
    r = numpy.random.default_rng(2).normal(size=183)
    z = M(r)
    assert not z[~p.free].any() and z[p.f1].all() and z[p.f2].all()
    assert numpy.array_equal(M(numpy.where(p.free, r, 7.))[p.f2], z[p.f2])
    assert numpy.allclose(M(numpy.where(p.free, r, 0.)), z, rtol=0, atol=1e-12 * abs(z).max())


# ---- errors before any device work ---------------------------------------------------------------------------------------------

def small():
    '''a 4 x 4 saddle point on host arrays, dofs 0, 1 the first field and 2, 3 the second'''
    K = scipy.sparse.csr_matrix(numpy.array([[2., -1., 1., 0.], [-1., 2., 0., 1.], [1., 0., 0., 0.], [0., 1., 0., 0.]]))
    return matrix.HipMatrix(K.data, K.indptr.astype(numpy.int64), K.indices.astype(numpy.int64), 4)


def fake(shape=(4, 4), free=(True,) * 4):
    '''a 'schur' object as `getprecon` makes it, without what lives on a device: `solve` refuses before it looks there'''
    return amg.Preconditioner('schur', shape, numpy.array(free), False, None, None)


def test_getprecon_errors_come_before_any_device_work():
    A = small()
    pmask = numpy.array([False, False, True, True])
    for args, message in ((dict(), '`second` is required'), (dict(second=None), '`second` is required'),
                          (dict(second=numpy.ones(3, dtype=bool)), 'second must be a bool mask of shape'), (dict(second=numpy.ones((4, 1), dtype=bool)), 'second must be a bool mask of shape'),
                          (dict(second=numpy.array([0., 1., 1., 0.])), 'second must be a bool mask of shape'), (dict(second=numpy.array([2, 4])), 'index outside'),
                          (dict(second=numpy.array([-1, 2])), 'index outside'), (dict(second=numpy.array([3, 2])), 'strictly increasing'),
                          (dict(second=numpy.array([2, 2, 3])), 'strictly increasing'), (dict(second=~numpy.zeros(4, dtype=bool)), 'both fields need free dofs'),
                          (dict(second=numpy.zeros(4, dtype=bool)), 'both fields need free dofs'), (dict(second=numpy.array([], dtype=int)), 'both fields need free dofs'),
                          (dict(second=pmask, constrain=numpy.array([numpy.nan, numpy.nan, 1., 1.])), 'both fields need free dofs'),
                          (dict(second=pmask, constrain=numpy.array([True, True, False, False])), 'both fields need free dofs'),
                          (dict(second=pmask, schur=numpy.ones(3)), 'schur must be a float vector'), (dict(second=pmask, schur=numpy.ones((4, 1))), 'schur must be a float vector'),
                          (dict(second=pmask, schur=numpy.arange(4)), 'schur must be a float vector'), (dict(second=pmask, schur=numpy.array([1., 1., numpy.nan, 1.])), 'zero or non-finite'),
                          (dict(second=pmask, schur=numpy.array([1., 1., 1., numpy.inf])), 'zero or non-finite'), (dict(second=pmask, schur=numpy.array([1., 1., 0., 1.])), 'zero or non-finite'),
                          (dict(second=pmask, first=dict(levels=3)), "invalid arguments \\['levels'\\] for the 'amg'"), (dict(second=pmask, first=dict(coarse=0)), 'coarse must be'),
                          (dict(second=pmask, first=dict(sweeps=0)), 'sweeps must be'), (dict(second=pmask, first=dict(setup='block')), 'needs `nullspace`'),
                          (dict(second=pmask, first=dict(nullspace=numpy.ones((3, 1)))), 'nullspace must have the shape'), (dict(second=pmask, first=[1]), 'first must be a dict'),
                          (dict(second=pmask, first=dict(smoother='chebyshev')), 'symmetric=False'), (dict(second=pmask, first=dict(smoother='chebyshev', degree=3)), 'Lanczos'),
                          (dict(second=pmask, third=pmask), "invalid arguments \\['third'\\] for the 'schur'"), (dict(second=pmask, coarse=16), "invalid arguments \\['coarse'\\]"),
                          (dict(second=pmask, constrain=numpy.zeros(3)), 'constraints have shape')):
        with pytest.raises(matrix.MatrixError, match=message):
            A.getprecon('schur', **args)
    # a matrix that is not square, and names that are no preconditioner
    B = matrix.HipMatrix(numpy.array([2., -1., -3.]), numpy.array([0, 2, 3]), numpy.array([0, 1, 0]), 3)
    with pytest.raises(matrix.MatrixError, match='not square'):
        B.getprecon('schur', second=numpy.array([1]))
    for precon in ('ilu', 'Schur', None):
        with pytest.raises(matrix.MatrixError, match='invalid preconditioner'):
            A.getprecon(precon, second=pmask)
    assert A._dev is None and A._amg is None and A._tplan is None and B._dev is None


def test_solve_errors_come_before_any_device_work():
    A, b = small(), numpy.ones(4)
    M = fake()
    assert (M.kind, M.shape, M.symmetric) == ('schur', (4, 4), False) and 'schur' in repr(M)
    with pytest.raises(matrix.MatrixError, match='symmetric=False'):
        A.solve(b, solver='cg', rtol=1e-8, precon=M)
    amg_messages = {}
    for solver in ('bicgstab', 'minres'):
        with pytest.raises(matrix.MatrixError, match="'fgmres'") as info:
            A.solve(b, solver=solver, rtol=1e-8, precon=M)
        with pytest.raises(matrix.MatrixError) as twin:  # the message these solvers give an 'amg' object
            A.solve(b, solver=solver, rtol=1e-8, precon=amg.Preconditioner('amg', (4, 4), numpy.ones(4, dtype=bool), False, None, None))
        assert str(info.value) == str(twin.value)
    with pytest.raises(matrix.MatrixError, match='takes one right-hand side at a time'):
        A.solve_columns(numpy.ones((4, 2)), rtol=1e-8, precon=M)
    with pytest.raises(matrix.MatrixError, match='preconargs'):
        A.solve(b, solver='fgmres', rtol=1e-8, precon=M, preconargs=dict(coarse=16))
    with pytest.raises(matrix.MatrixError, match='built for a 5x5 matrix'):
        A.solve(b, solver='fgmres', rtol=1e-8, precon=fake((5, 5), (True,) * 5))
    with pytest.raises(matrix.MatrixError, match='another set of free dofs'):
        A.solve(b, solver='fgmres', rtol=1e-8, precon=M, constrain=numpy.array([numpy.nan, 1., numpy.nan, numpy.nan]))
    with pytest.raises(matrix.MatrixError, match='another set of free dofs'):
        A.solve(b, solver='fgmres', rtol=1e-8, precon=fake(free=(True, False, True, True)))
    with pytest.raises(matrix.MatrixError, match='tolerance'):
        A.solve(b, solver='fgmres', precon=M)
    with pytest.raises(matrix.MatrixError, match='restart'):
        A.solve(b, solver='fgmres', rtol=1e-8, precon=M, restart=0)
    with pytest.raises(matrix.MatrixError, match='invalid preconditioner'):  # the name is no preconditioner of `solve`: the object is
        A.solve(b, solver='fgmres', rtol=1e-8, precon='schur')
    with pytest.raises(matrix.MatrixError, match='vector of 4 entries'):
        M(numpy.ones(3))
    assert A._dev is None and A.iterations is None


# ---- System.trialmask --------------------------------------------------------------------------------------------------------

def test_trialmask():
    '''the mask of the named trial arguments over the packed vector, from `offsets`: a vector field of degree 2 and a scalar one of degree 1'''
    from nutils_amd import function, mesh
    from nutils_amd.solver import System
    domain, geom = mesh.unitsquare(4, 'square')
    u, v = (domain.field(name, btype='std', degree=2, shape=(2,)) for name in 'uv')
    p, q = (domain.field(name, btype='std', degree=1) for name in 'pq')
    grad = lambda w: function.grad(w, geom)
    res = domain.integral(((grad(v) * grad(u)).sum(-1).sum(-1) - function.div(v, geom) * p - q * function.div(u, geom)) * function.J(geom), degree=4)
    system = System(res, trial='u,p', test='v,q')
    assert system.trial_shapes == [(81, 2), (25,)] and system.size == 187
    pmask = system.trialmask('p')
    assert pmask.dtype == bool and pmask.shape == (187,) and numpy.array_equal(numpy.flatnonzero(pmask), numpy.arange(162, 187))
    assert numpy.array_equal(system.trialmask('u'), ~pmask) and system.trialmask('u', 'p').all() and system.trialmask('p', 'u').all() and not system.trialmask().any()
    packed, free = system._pack({'p': numpy.ones(25)}, {'p': numpy.where(numpy.arange(25) == 0, 2., numpy.nan)})
    assert numpy.array_equal(packed != 0, pmask) and numpy.array_equal(numpy.flatnonzero(~free), [162])  # the layout `_pack` and the Jacobian use
    with pytest.raises(ValueError, match='not a trial argument'):
        system.trialmask('q')
    swapped = System(res, trial='p,u', test='q,v')
    assert numpy.array_equal(numpy.flatnonzero(swapped.trialmask('p')), numpy.arange(25))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------

Q, R = ctypes.c_void_p(128), ctypes.c_void_p(256)  # more pointers that are never followed


def schur_handle(n=3, first=None):
    lib = _lib.load()
    out = ctypes.c_void_p()
    assert lib.nh_schur_create(first, ctypes.byref(csr(nrows=n, ncols=n)), P, P, Q, R, ctypes.byref(out)) == 0 and out
    return out


def test_abi_refusals():
    lib = _lib.load()
    A = ctypes.byref(csr())
    h3, h4 = handle(3), handle(4)
    s3 = schur_handle(3, h3)
    s4 = schur_handle(4, h4)
    out = ctypes.c_void_p()
    try:
        # nh_csr_schur_diagonal(A, vt, first, dinv, out, stream)
        diagonal = lambda A=A, vt=P, first=P, dinv=P, out=P: lib.nh_csr_schur_diagonal(A, vt, first, dinv, out, None)
        refused(diagonal(A=None), 'nh_csr_schur_diagonal', 'NULL matrix')
        refused(diagonal(A=ctypes.byref(csr(ncols=4))), 'nh_csr_schur_diagonal', 'square')
        refused(diagonal(out=None), 'nh_csr_schur_diagonal', 'NULL result')
        for name in ('vt', 'first', 'dinv'):
            refused(diagonal(**{name: None}), 'nh_csr_schur_diagonal', 'NULL transposed values')
        for fields, word in ((dict(nrows=-1), 'negative size'), (dict(lanes=3), 'power of two'), (dict(rowptr=None), 'NULL row pointers'), (dict(values=None), 'NULL values')):
            refused(diagonal(A=ctypes.byref(csr(**fields))), 'nh_csr_schur_diagonal', word)
        assert diagonal(A=ctypes.byref(csr(nrows=0, ncols=0, nnz=0))) == 0  # nothing to do: no launch
        # nh_schur_create(first, K, mask1, sinv, z2, t, out)
        create = lambda first=h3, K=A, mask1=P, sinv=P, z2=Q, t=R, out=ctypes.byref(out): lib.nh_schur_create(first, K, mask1, sinv, z2, t, out)
        refused(create(first=None), 'nh_schur_create', 'NULL hierarchy')
        refused(create(K=None), 'nh_schur_create', 'NULL matrix')
        refused(create(out=None), 'nh_schur_create', 'nowhere to put the handle')
        refused(create(first=h4), 'nh_schur_create', 'another size')
        refused(create(K=ctypes.byref(csr(ncols=4))), 'nh_schur_create', 'square')
        for name in ('mask1', 'sinv', 'z2', 't'):
            refused(create(**{name: None}), 'nh_schur_create', 'NULL mask')
        refused(create(z2=Q, t=Q), 'nh_schur_create', 'distinct')
        assert not out
        assert lib.nh_schur_free(None) == 0
        # nh_schur_apply(schur, r, z, stream)
        refused(lib.nh_schur_apply(None, P, ctypes.c_void_p(512), None), 'nh_schur_apply', 'NULL preconditioner')
        refused(lib.nh_schur_apply(s3, None, P, None), 'nh_schur_apply', 'NULL vector')
        refused(lib.nh_schur_apply(s3, P, None, None), 'nh_schur_apply', 'NULL vector')
        refused(lib.nh_schur_apply(s3, P, P, None), 'nh_schur_apply', 'result is the argument')
        refused(lib.nh_schur_apply(s3, P, Q, None), 'nh_schur_apply', 'scratch')
        refused(lib.nh_schur_apply(s3, R, P, None), 'nh_schur_apply', 'scratch')
        # nh_fgmres_iterate_schur: the refusals of nh_fgmres_iterate
        fresh = lambda: [P, P, ctypes.c_void_p(512), ctypes.c_void_p(1024), P]  # V, Z, z, t, w

        def iterate(A=A, schur=s3, vectors=None, work=P, restart=30, stop_rr=1e-20, niter=1):
            return lib.nh_fgmres_iterate_schur(A, None, schur, *(vectors or fresh()), work, restart, stop_rr, niter, None)
        refused(iterate(A=None), 'nh_fgmres_iterate_schur', 'NULL matrix')
        refused(iterate(schur=None), 'nh_fgmres_iterate_schur', 'NULL preconditioner')
        refused(iterate(schur=s4), 'nh_fgmres_iterate_schur', 'another size')
        for i in range(5):
            vectors = fresh()
            vectors[i] = None
            refused(iterate(vectors=vectors), 'nh_fgmres_iterate_schur', 'NULL vector')
        refused(iterate(vectors=[P] * 5), 'nh_fgmres_iterate_schur', 'result is its argument')
        refused(iterate(vectors=[P, P, Q, ctypes.c_void_p(512), P]), 'nh_fgmres_iterate_schur', 'scratch')
        refused(iterate(work=None), 'nh_fgmres_iterate_schur', 'NULL vector')
        refused(iterate(A=ctypes.byref(csr(ncols=4))), 'nh_fgmres_iterate_schur', 'square')
        refused(iterate(niter=-1), 'nh_fgmres_iterate_schur', 'negative iteration count')
        for restart in (0, -3):
            refused(iterate(restart=restart), 'nh_fgmres_iterate_schur', 'restart must be at least 1')
        for stop_rr in (-1e-300, float('nan')):
            refused(iterate(stop_rr=stop_rr), 'nh_fgmres_iterate_schur', 'negative')
        for fields, word in ((dict(nrows=-1), 'negative size'), (dict(lanes=3), 'power of two'), (dict(rowptr=None), 'NULL row pointers'), (dict(values=None), 'NULL values')):
            refused(iterate(A=ctypes.byref(csr(**fields))), 'nh_fgmres_iterate_schur', word)
        assert iterate(niter=0) == 0  # no steps: no launch
    finally:
        for each in (s3, s4):
            lib.nh_schur_free(each)
        for each in (h3, h4):
            lib.nh_amg_free(each)


def test_table_and_wrappers_know_the_entries():
    from nutils_amd import kernels
    lengths = dict(nh_csr_schur_diagonal=6, nh_schur_create=7, nh_schur_free=1, nh_schur_apply=4, nh_fgmres_iterate_schur=13)
    for name, count in lengths.items():
        assert len(_lib.SIGNATURES[name][1]) == count
    assert _lib.SIGNATURES['nh_fgmres_iterate_schur'] == _lib.SIGNATURES['nh_fgmres_iterate']  # the same arguments, the handle in the hierarchy's place
    assert callable(kernels.csr_schur_diagonal) and callable(kernels.fgmres_iterate_schur) and callable(kernels.Schur)
