'''The device BiCGStab solve for general square matrices (matrix.HipMatrix.solve(solver='bicgstab'), nh_csr.hip) on the GPU: the solve contract on
nonsymmetric matrices from one vector workgroup to strided grids, iteration counts against the numpy restatement of tests/test_bicgstab_host.py, indefinite
matrices and breakdowns, the stopping rules, and the product's two-dot epilogue on its own.

Sizes: 130 and 192 rows stay inside one vector workgroup; 1480 rows are six vector workgroups, the last one partial, and 24 product workgroups at 4 lanes;
262 444 rows are more than 1024 * 256, so the vector kernels stride, and at 64 lanes more than 2048 product workgroups, so the epilogue accumulates.'''
import functools
import numpy
import pytest
import scipy.sparse

from test_bicgstab_host import bicgstab_reference, skewed

pytestmark = pytest.mark.gpu

U = 2. ** -53
RTOL = 1e-10


def gamma(n):
    '''the constant of a sum of n terms in any order (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.4)'''
    n = numpy.asarray(n, dtype=float)
    return n * U / (1 - n * U)


def hip(core):
    '''a host matrix as a HipMatrix on device tensors (so that `_hostcsr` shows whether a solve exported it)'''
    from nutils_amd import device, matrix
    core = scipy.sparse.csr_matrix(core, dtype=float)
    core.sort_indices()
    return matrix.HipMatrix(device.to_dev(core.data, 'float64'), device.to_dev(core.indptr, 'int64'), device.to_dev(core.indices, 'int64'), core.shape[1])


def solve(A, rhs=None, iterated=True, **kwargs):
    '''A.solve(solver='bicgstab') that insists on the device route'''
    from nutils_amd import _lib
    with _lib.trace() as calls:
        try:
            return A.solve(rhs, solver='bicgstab', **kwargs)
        finally:
            assert 'nh_bicgstab_init' in calls and ('nh_bicgstab_iterate' in calls or not iterated), calls
            assert A._hostcsr is None  # neither values nor indices went to the host


# ---- problems ------------------------------------------------------------------------------------------------------------

def laplace(shape):
    from nutils_amd import function, mesh
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1 + i, n) for i, n in enumerate(shape)])
    basis = domain.basis('std', degree=1)
    K = domain.integral(function.outer(function.grad(basis, geom)).sum(-1) * function.J(geom), degree=2)
    cons = numpy.full(shape, numpy.nan)
    cons[0] = 1 + .1 * numpy.arange(shape[1])  # one side held at non-zero values
    return K, dict(constrain=cons.ravel()), numpy.random.default_rng(1).normal(size=cons.size)


def elasticity():
    from nutils_amd import function, mesh
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1, 4)] * 3)
    u = domain.field('u', btype='std', degree=1, shape=[3])
    v = domain.field('v', btype='std', degree=1, shape=[3])
    eps = lambda w: function.symgrad(w, geom)
    res = domain.integral(function.inner(eps(v), function.div(u, geom) * function.eye(3) + 1.3 * eps(u)) * function.J(geom), degree=2)
    clamped = numpy.zeros((4, 4, 4, 3), dtype=bool)
    clamped[0] = True
    lhs0 = numpy.zeros((4, 4, 4, 3))
    lhs0[0] = [.01, -.02, .03]
    lhs0[1:] = .5  # an initial guess on the free dofs
    return function.derivative(function.derivative(res, 'v'), 'u'), dict(constrain=clamped.ravel(), lhs0=lhs0.ravel()), numpy.random.default_rng(2).normal(size=192)


def tridiagonal(n=262444):
    N = scipy.sparse.diags([numpy.full(n - 1, -1.5), numpy.full(n, 4.), numpy.full(n - 1, -.5)], [-1, 0, 1], format='csr')
    cons = numpy.full(n, numpy.nan)
    cons[::1000] = 2.
    return N, dict(constrain=cons), numpy.random.default_rng(4).normal(size=n)


@functools.lru_cache(maxsize=None)
def problem(name):
    '''the nonsymmetric matrix on the device, its host twin, the solve's keywords and right-hand side, the free mask, the start vector, |r0|; for the small
    problems also the direct solution and the smallest singular value of the free block.  Made once, never written.'''
    from nutils_amd import device, function, matrix
    if name == 'tridiagonal':
        ref, kwargs, rhs = tridiagonal()
        A = hip(ref)
    else:
        K, kwargs, rhs = elasticity() if name == 'elasticity' else laplace({'laplace': (13, 10), 'wide': (40, 37)}[name])
        v, rp, ci = function.eval(function.as_csr(K))
        ref = skewed(scipy.sparse.csr_matrix((v, ci, rp), (len(rp) - 1,) * 2))
        # the same skewing on the device, from the value tensor: K_ij (1 + sign(j - i) / 2)
        S = function.eval(function.as_matrix(K))
        values, rowptr, colidx = S.triplet()
        torch = device.torch()
        rows = torch.repeat_interleave(torch.arange(S.shape[0], device=values.device), rowptr[1:] - rowptr[:-1])
        A = matrix.HipMatrix(values * (1 + .5 * torch.sign(colidx - rows)), rowptr, colidx, S.shape[1])
        assert numpy.abs(A @ rhs - ref @ rhs).max() <= 1e-13 * numpy.abs(ref @ rhs).max()
    assert A._hostcsr is None
    free, start = matrix.constraints(A.shape[1], kwargs.get('constrain'), kwargs.get('lhs0'))
    r0 = numpy.linalg.norm((rhs - ref @ start)[free])
    direct = smin = None
    if A.shape[0] < 2000:
        direct = matrix.ScipyMatrix(ref).solve(rhs, **kwargs)
        smin = numpy.linalg.svd(ref.toarray()[free][:, free], compute_uv=False)[-1]
        assert smin > 0
    return A, ref, kwargs, rhs, free, start, r0, direct, smin


@functools.lru_cache(maxsize=None)
def reference_iterations(name, precon):
    '''iterations the numpy restatement needs to the bound of the tests'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem(name)
    dinv = numpy.where(free, 1 / ref.diagonal(), 0.) if precon else None
    x, it, broke = bicgstab_reference(ref, rhs, start, free, dinv, (RTOL * r0) ** 2, int(free.sum()))
    assert not broke and numpy.linalg.norm((rhs - ref @ x)[free]) <= 10 * RTOL * r0
    return it


def contract(name, x):
    '''what a solve to RTOL promises: constrained dofs exactly, the true residual within the bound, the error within residual / sigma_min'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem(name)
    assert isinstance(x, numpy.ndarray) and numpy.array_equal(x[~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ x)[free])
    print(f'{name}: |r| / |r0| = {res / r0:.3e}' + ('' if direct is None else f', |x - x_direct| = {numpy.linalg.norm(x - direct):.3e}, bound {res / smin:.3e}'))
    assert res <= RTOL * r0 * (1 + 1e-3)
    if direct is not None:
        assert numpy.linalg.norm(x - direct) <= res / smin
    return res


def solve_contract(name, A=None):
    A0, ref, kwargs, rhs, free, start, r0, direct, smin = problem(name)
    A = A or A0
    for precon in ('diag', None):
        x = solve(A, rhs, rtol=RTOL, precon=precon, **kwargs)  # (default maxiter: the free dofs)
        contract(name, x)
        assert 0 < A.iterations <= free.sum()
        iterations = A.iterations
        assert numpy.array_equal(solve(A, rhs, rtol=RTOL, precon=precon, **kwargs).view(numpy.int64), x.view(numpy.int64))  # bit-identical
        assert A.iterations == iterations
        # every look at the device after one iteration; an absolute tolerance: the same contract, and the same iteration (it stops itself)
        y = solve(A, rhs, atol=RTOL * r0, precon=precon, check=1, **kwargs)
        contract(name, y)
        assert abs(A.iterations - iterations) <= 1  # (atol = RTOL r0 is the bound of rtol = RTOL up to the rounding of r0)


# ---- 1-4: the solve contract from one workgroup to strided grids ------------------------------------------------------------

def test_solve_contract():
    solve_contract('laplace')


def test_many_workgroups():
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('wide')
    assert A.shape[0] == 1480 and A.lanes == 4
    solve_contract('wide')
    wave_per_row = A._with_values(A.triplet()[0])
    wave_per_row.lanes = 64
    solve_contract('wide', wave_per_row)
    for precon in ('diag', None):
        solve(A, rhs, rtol=RTOL, precon=precon, **kwargs)
        it_ref = reference_iterations('wide', precon)
        print(f'wide, precon={precon}: {A.iterations} iterations on the device, {it_ref} in numpy')
        # the restatement's count moves by at most one under random summation orders; a lost preconditioner or a wrong beta costs tens of percent
        assert A.iterations <= 1.1 * it_ref + 2


def test_grid_caps():
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('tridiagonal')
    assert A.shape[0] > 1024 * 256
    B = A._with_values(A.triplet()[0])
    B.lanes = 64  # a row per wave: more than 2048 product workgroups' worth of rows
    assert A.shape[0] / (256 // B.lanes) > 2048
    for precon in ('diag', None):
        x = solve(B, rhs, rtol=RTOL, precon=precon, **kwargs)
        contract('tridiagonal', x)
        it_ref = reference_iterations('tridiagonal', 'diag')  # (a constant diagonal: Jacobi scales the system, the restatement's count is that of both)
        print(f'tridiagonal, precon={precon}: {B.iterations} iterations on the device, {it_ref} in numpy')
        assert B.iterations <= it_ref + 2


def test_elasticity_bool_constraints():
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('elasticity')
    from nutils_amd import device
    lengths = numpy.diff(device.to_host(A.triplet()[1]))
    assert A.shape[0] == 192 and (lengths.min(), lengths.max()) == (24, 81)
    assert kwargs['constrain'].dtype == bool and 'lhs0' in kwargs
    half_wave_per_row = A._with_values(A.triplet()[0])
    half_wave_per_row.lanes = 32  # (the rule takes 16 for this mesh, 32 from 6 cells per axis on)
    solve_contract('elasticity', half_wave_per_row)


# ---- 5: indefinite matrices and breakdowns (defined arithmetic outcomes, nothing faults) ----------------------------------

def test_indefinite_and_breakdown():
    from nutils_amd import matrix
    D = hip([[1., 0.], [0., -1.]])
    x = solve(D, numpy.array([1., 2.]), rtol=1e-12, precon=None)
    assert numpy.allclose(x, [1., -2.], rtol=1e-12, atol=0) and D.iterations == 2
    x = solve(D, numpy.array([1., 2.]), rtol=1e-12)  # (Jacobi makes this matrix the identity)
    assert numpy.allclose(x, [1., -2.], rtol=1e-12, atol=0) and D.iterations == 1
    with pytest.raises(matrix.MatrixError, match='not positive definite'):
        D.solve(numpy.array([1., 2.]), rtol=1e-12)  # 'cg' refuses it
    with pytest.raises(matrix.MatrixError, match='bicgstab: breakdown'):
        solve(D, numpy.array([1., 1.]), rtol=1e-12, precon=None)  # rhat . v = 1 - 1 = 0 at the first step (without Jacobi: with it the system is the identity)
    assert D.iterations == 0
    S = hip([[0., 1.], [1., 0.]])
    with pytest.raises(matrix.MatrixError, match='bicgstab: breakdown'):
        solve(S, numpy.array([1., 0.]), rtol=1e-12, precon=None)
    with pytest.raises(matrix.MatrixError, match='diagonal has zero entries'):
        S.solve(numpy.array([1., 0.]), solver='bicgstab', rtol=1e-12, precon='diag')
    assert S._hostcsr is None


# ---- 6: stopping and trivial systems ---------------------------------------------------------------------------------------

def test_stops_at_maxiter():
    from nutils_amd import matrix
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('laplace')
    with pytest.raises(matrix.ToleranceNotReached) as info:
        solve(A, rhs, rtol=RTOL, maxiter=3, **kwargs)
    best = info.value.best
    assert A.iterations == 3
    assert numpy.isfinite(best).all() and numpy.array_equal(best[~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ best)[free])
    assert RTOL * r0 < res < r0  # three iterations got somewhere, not there
    with pytest.warns(UserWarning, match='tolerance'):
        lenient = A.solve_leniently(rhs, solver='bicgstab', rtol=RTOL, maxiter=3, **kwargs)
    assert numpy.array_equal(lenient, best)
    assert numpy.array_equal(A.solve_leniently(rhs, solver='bicgstab', rtol=RTOL, **kwargs), solve(A, rhs, rtol=RTOL, **kwargs))


def test_device_vectors_and_trivial_systems():
    from nutils_amd import device
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('laplace')
    x = solve(A, device.to_dev(rhs, 'float64'), rtol=RTOL, **kwargs)
    assert x.is_cuda and numpy.array_equal(device.to_host(x), solve(A, rhs, rtol=RTOL, **kwargs))
    # a residual within the tolerance from the start: the initial vector comes back
    exact = ref @ start
    assert numpy.array_equal(solve(A, exact, iterated=False, rtol=RTOL, atol=1e-9, **kwargs), start) and A.iterations == 0
    # no right-hand side, no constraints: zero
    assert not solve(A, iterated=False, rtol=RTOL).any() and A.iterations == 0
    assert A.cg_iterations is None  # (no 'cg' solve was made on this matrix)


# ---- 7: the product's two-dot epilogue on its own ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['bilinear', 'p2vector', 'holes'])
def test_product_epilogue(name):
    from nutils_amd import device, kernels
    from test_gpu_matrix_hip import case, product_bound, LANES
    (values, rowptr, colidx), ncols, ref, x = case(name)
    nrows = ref.shape[0]
    rng = numpy.random.default_rng(11)
    w = rng.normal(size=nrows)
    mask = rng.uniform(size=nrows) < .6
    mask[:2] = [False, True]
    xd, wd, md = device.to_dev(x, 'float64'), device.to_dev(w, 'float64'), device.to_dev(mask, 'uint8')
    col32 = kernels.csr_compact(colidx, ncols)
    work = kernels.bicgstab_work()
    for keep, maskd in ((numpy.ones(nrows, dtype=bool), None), (mask, md)):
        y_ref = numpy.where(keep, ref @ x, 0.)
        # the device's y is within dy of y_ref (product_bound); its dots are sums of nrows products in some order, numpy's another: 2 gamma_(nrows + 1) each
        dy = numpy.where(keep, product_bound(ref, x), 0.)
        wy_bound = (numpy.abs(w) * dy).sum() + 2 * gamma(nrows + 1) * (numpy.abs(w) * (numpy.abs(y_ref) + dy)).sum()
        yy_bound = (dy * (2 * numpy.abs(y_ref) + dy)).sum() + 2 * gamma(nrows + 1) * ((numpy.abs(y_ref) + dy) ** 2).sum()
        for narrow in (col32, None):
            for lanes in LANES:
                plain = kernels.csr_spmv(values, rowptr, colidx, ncols, xd, rowmask=maskd, col32=narrow, lanes=lanes)
                y, dots = kernels.csr_spmv_dots(values, rowptr, colidx, ncols, xd, wd, rowmask=maskd, col32=narrow, lanes=lanes, work=work)
                assert numpy.array_equal(device.to_host(y).view(numpy.int64), device.to_host(plain).view(numpy.int64))  # byte for byte
                wy, yy = dots.tolist()
                assert abs(wy - w @ y_ref) <= wy_bound, (name, lanes, narrow is not None, wy - w @ y_ref, wy_bound)
                assert abs(yy - y_ref @ y_ref) <= yy_bound, (name, lanes, narrow is not None, yy - y_ref @ y_ref, yy_bound)
                assert yy >= 0 and (yy > 0) == bool(y_ref.any())


# ---- 8: a nonsymmetric matrix straight from the front end -----------------------------------------------------------------

def test_convection_diffusion_through_the_front_end():
    from nutils_amd import function, matrix, mesh
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1, 8), numpy.linspace(0, 2, 6)])
    basis = domain.basis('std', degree=1)
    grad = function.grad(basis, geom)
    K = domain.integral((function.outer(grad).sum(-1) + function.outer(basis, (grad * numpy.array([3., -2.])).sum(-1))) * function.J(geom), degree=2)
    A = function.eval(function.as_matrix(K))
    v, rp, ci = function.eval(function.as_csr(K))
    ref = scipy.sparse.csr_matrix((v, ci, rp), A.shape)
    assert isinstance(A, matrix.HipMatrix) and A._hostcsr is None and abs(ref - ref.T).max() > .1  # not symmetric
    cons = numpy.full((8, 6), numpy.nan)
    cons[0], cons[-1] = 1., 0.  # inflow and outflow sides held
    cons = cons.ravel()
    free = numpy.isnan(cons)
    rhs = numpy.random.default_rng(5).normal(size=48)
    x = solve(A, rhs, constrain=cons, rtol=RTOL)
    start = numpy.where(free, 0., cons)
    assert numpy.array_equal(x[~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ x)[free])
    assert res <= RTOL * numpy.linalg.norm((rhs - ref @ start)[free]) * (1 + 1e-3)
    direct = matrix.ScipyMatrix(ref).solve(rhs, constrain=cons)
    assert numpy.linalg.norm(x - direct) <= res / numpy.linalg.svd(ref.toarray()[free][:, free], compute_uv=False)[-1]
