'''CPU-side checks of the Chebyshev smoother of the AMG preconditioner (preconargs=dict(smoother='chebyshev', degree=2, eigsteps=10, eigratio=10.),
nutils_amd/amg.py, nh_csr_lanczos and nh_csr_chebyshev of nh_amg.hip), on top of the restatements of tests/test_amg_host.py and
tests/test_amg_nullspace_host.py: the Lanczos recurrence on S A_f S and the Chebyshev cycle restated in numpy, in float64 or longdouble, with their
invariants pinned; the coefficients of nutils_amd.amg against the Chebyshev polynomial itself; and the argument errors.  The restatement is the CPU
reference of tests/test_gpu_amg_chebyshev.py.'''
import functools
import numpy
import pytest
import scipy.sparse
import scipy.sparse.linalg

from test_cg_host import gamma, U
from test_amg_host import hierarchy, cycle, pcg_reference, product, keys, free_part, problem as scalar_problem
from test_amg_nullspace_host import hierarchy as hierarchy_with_nullspace, elasticity

ld = numpy.longdouble


# ---- the algorithm, restated ---------------------------------------------------------------------------------------------

def start_vector(n):
    '''the top 31 bits of the documented hash, as a number in [-1, 1)'''
    return (keys(n) >> 32) * 2. ** -30 - 1.


def lanczos(A, free, dinv, steps, u=None, dtype=float):
    '''(alpha, beta, taken): `steps` steps of the recurrence on S A_f S, S = sqrt(dinv), in the arithmetic `dtype`; alpha[j] and beta[j] = beta_(j+1) of the steps
    taken.  A beta that is 0 or not finite ends it.'''
    n = A.shape[0]
    s = numpy.sqrt(dinv.astype(dtype))
    q = numpy.where(free & (s != 0), start_vector(n) if u is None else u, 0).astype(dtype)
    norm = numpy.sqrt(q @ q)
    alpha, beta = [], []
    if not (norm > 0 and numpy.isfinite(norm)):
        return numpy.array(alpha, dtype=dtype), numpy.array(beta, dtype=dtype), 0
    q, qprev, b = q / norm, numpy.zeros(n, dtype=dtype), dtype(0)
    for j in range(steps):
        w = s * numpy.where(free, product(A, s * q), 0)
        a = q @ w
        w = w - a * q - b * qprev
        b = numpy.sqrt(w @ w)
        alpha.append(a)
        beta.append(b)
        if not (b > 0 and numpy.isfinite(b)):
            break
        qprev, q = q, w / b
    return numpy.array(alpha, dtype=dtype), numpy.array(beta, dtype=dtype), len(alpha)


def theta_of(alpha, beta):
    '''the largest eigenvalue of the tridiagonal matrix of the steps taken'''
    alpha, beta = numpy.asarray(alpha, dtype=float), numpy.asarray(beta, dtype=float)[:len(alpha) - 1]
    return numpy.linalg.eigvalsh(numpy.diag(alpha) + numpy.diag(beta, 1) + numpy.diag(beta, -1))[-1]


def coefficients(ub, lb, degree, dtype=float):
    '''[(c1, c2)] of the steps d = c1 d + c2 dinv (b - A x), x += d'''
    ub, lb = dtype(ub), dtype(lb)
    tc, delta = (ub + lb) / 2, (ub - lb) / 2
    out, rho = [(dtype(0), 1 / tc)], delta / tc
    for _ in range(1, degree):
        new = 1 / (2 * tc / delta - rho)
        out.append((new * rho, 2 * new / delta))
        rho = new
    return out


def with_bounds(levels, eigsteps=10, eigratio=10.):
    '''sets theta, ub and lb on every coarsened level (of a hierarchy made for this purpose: the cached ones of the other files are not written)'''
    for lv in levels:
        if lv.kind == 'coarsen':
            lv.theta = theta_of(*lanczos(lv.A, lv.free, lv.dinv, eigsteps)[:2])
            lv.ub = min(1.1 * lv.theta, lv.rho)
            lv.lb = lv.ub / eigratio
    return levels


def chebyshev_cycle(levels, b, degree, l=0):
    '''z = M b with the Chebyshev smoother on the levels' ub and lb, in the arithmetic of b (a vector, or a matrix whose columns are right-hand sides)'''
    lv = levels[l]
    if lv.kind != 'coarsen':
        return cycle(levels, b, 1, l)
    col = lambda v: v.astype(b.dtype).reshape((-1,) + (1,) * (b.ndim - 1))
    dinv, free = col(lv.dinv), col(lv.free)
    coef = coefficients(lv.ub, lv.lb, degree, b.dtype.type)
    d = coef[0][1] * dinv * b
    x = d
    for c1, c2 in coef[1:]:
        d = numpy.where(free, c1 * d + c2 * dinv * (b - product(lv.A, x)), 0)
        x = numpy.where(free, x + d, 0)
    r = numpy.where(free, b - product(lv.A, x), 0)
    x = x + product(lv.P, chebyshev_cycle(levels, product(lv.R, r), degree, l + 1))
    for k, (c1, c2) in enumerate(coef):
        t = c2 * dinv * (b - product(lv.A, x))
        d = numpy.where(free, c1 * d + t if k else t, 0)
        x = numpy.where(free, x + d, 0)
    return x


# ---- problems ------------------------------------------------------------------------------------------------------------

def held_face(shape):
    '''the free mask of `elasticity(shape)` with the face x = 0 held'''
    free = numpy.ones(tuple(n + 1 for n in shape) + (len(shape),), dtype=bool)
    free[0] = False
    return free.ravel()


@functools.lru_cache(maxsize=None)
def case(name):
    '''(A, free, levels with theta, ub, lb set): 'laplace' (40 x 37 nodes, the constant, coarse 16), 'elasticity2' ((32, 32) elements, the face x = 0 held, three
    rigid-body modes, coarse 64), 'elasticity3' ((9, 9, 9), six modes, coarse 64), 'small' ((12, 10), coarse 32).  Made once, never written afterwards.'''
    from nutils_amd import amg
    if name == 'laplace':
        A, free = scalar_problem('laplace')
        return A, free, with_bounds(hierarchy(A, free, 16))
    shape, coarse = {'elasticity2': ((32, 32), 64), 'elasticity3': ((9, 9, 9), 64), 'small': ((12, 10), 32)}[name]
    A, coords = elasticity(shape)
    free = held_face(shape)
    return A, free, with_bounds(hierarchy_with_nullspace(A, free, amg.rigid_body_modes(coords), coarse))


PROBLEMS = ['laplace', 'elasticity2', 'elasticity3']


def exact_diagonal(n=1024):
    '''(A, free, dinv, u): a diagonal matrix whose entries are powers of 4, every 8th row masked and every 8th + 1 with dinv = 0, and a start vector with 256
    entries +-1 on rows that take part (and ones on rows that do not, which the recurrence must ignore): sqrt(dinv), |u| = 16, q = +-1/16 and q . q = 1 are all exact'''
    rng = numpy.random.default_rng(6)
    diag = 4. ** rng.integers(-3, 4, n)
    free = numpy.ones(n, dtype=bool)
    free[::8] = False
    dinv = numpy.where(free, 1 / diag, 0.)
    dinv[1::8] = 0.
    take = free & (dinv != 0)
    signs = numpy.where(rng.integers(0, 2, n) == 1, 1., -1.)
    u = numpy.where(take, numpy.where(numpy.cumsum(take) <= 256, signs, 0.), 1.)
    return scipy.sparse.diags(diag, format='csr'), free, dinv, u


# ---- tests ---------------------------------------------------------------------------------------------------------------

def chebyshev_polynomial(degree, t):
    '''T_degree(t) in longdouble by the three-term recurrence'''
    t = numpy.asarray(t, dtype=ld)
    a, b = numpy.ones_like(t), t
    for _ in range(degree):
        a, b = b, 2 * t * b - a
    return a


@pytest.mark.parametrize('degree', [1, 2, 3, 4])
def test_coefficients_are_the_chebyshev_polynomial(degree):
    '''On a diagonal matrix with dinv diag = lambda_i the error after `degree` steps from x = 0 is T_d((tc - lambda) / delta) / T_d(tc / delta) times the solution.
    The coefficients are those of nutils_amd.amg, the steps those of the restatement.  Bound: a step makes at most 10 roundings (the residual, its two factors,
    the two terms of d and their sum, the sum x + d, and three in its two coefficients), each relative to a quantity of at most g |x*| with g = max(1, ub max c2)
    times 2 (|x| <= 2 |x*|: the polynomial lies in [-1, 1] on the interval and below it within [0, 1]); what a step adds is carried on by the remaining steps,
    whose recurrence grows at most linearly: degree^2 in all.'''
    from nutils_amd import amg
    ub, lb = 2.3, .23
    lam = numpy.linspace(ub / 50, ub, 200)
    diag = numpy.random.default_rng(3).uniform(1, 10, len(lam))
    dinv, b = lam / diag, numpy.random.default_rng(4).normal(size=len(lam))
    coef = amg.chebyshev_coefficients(ub, lb, degree).reshape(degree, 2)
    mine = numpy.array(coefficients(ub, lb, degree, ld)).astype(float)
    assert coef.shape == mine.shape and (abs(coef - mine) <= 8 * U * abs(mine)).all() and coef[0, 0] == 0
    x = d = coef[0, 1] * dinv * b
    for c1, c2 in coef[1:]:
        d = c1 * d + c2 * dinv * (b - diag * x)
        x = x + d
    tc, delta = (ld(ub) + ld(lb)) / 2, (ld(ub) - ld(lb)) / 2
    factor = chebyshev_polynomial(degree, (tc - lam.astype(ld)) / delta) / chebyshev_polynomial(degree, tc / delta)
    solution = b.astype(ld) / diag.astype(ld)
    err = numpy.abs((solution - x) - factor * solution).astype(float)
    bound = 20 * degree ** 2 * U * max(1., ub * coef[:, 1].max()) * abs(b / diag)
    print(f'degree {degree}: max error / bound = {(err / bound).max():.3f}, largest factor {float(abs(factor).max()):.3f}, on [lb, ub] {float(abs(factor[lam >= lb]).max()):.3f}')
    assert (err <= bound).all()
    assert (abs(factor[lam >= lb]) <= 1 / chebyshev_polynomial(degree, tc / delta) * (1 + 1e-12)).all()  # the minimax property, on the interval


@pytest.mark.parametrize('name', PROBLEMS)
def test_estimate(name):
    '''theta of 10 Lanczos steps from the hash-derived start vector on every coarsened level: never above the largest eigenvalue of D^-1 A_f, and at least 0.9 of it'''
    A, free, levels = case(name)
    coarsened = [lv for lv in levels if lv.kind == 'coarsen']
    assert len(coarsened) >= 2
    for l, lv in enumerate(coarsened):
        s = numpy.sqrt(lv.dinv)
        Ahat = scipy.sparse.diags(s) @ free_part(lv.A, lv.free) @ scipy.sparse.diags(s)
        lmax = numpy.linalg.eigvalsh(Ahat.toarray())[-1] if lv.n <= 1500 else scipy.sparse.linalg.eigsh(Ahat, k=1, which='LA', tol=0, return_eigenvectors=False)[0]
        alpha, beta, taken = lanczos(lv.A, lv.free, lv.dinv, 10)
        print(f'{name} level {l}: n = {lv.n}, rho = {lv.rho:.3f}, lambda_max = {lmax:.4f}, theta = {lv.theta:.4f} ({lv.theta / lmax:.4f}), ub = {lv.ub:.4f}')
        assert taken == 10 and lv.theta == theta_of(alpha, beta)
        assert lv.theta <= lmax * (1 + 1e-12)
        assert lv.theta >= .9 * lmax
        assert lmax <= lv.rho * (1 + 1e-12)  # (the Gershgorin number is a true bound)
        exact = theta_of(*lanczos(lv.A, lv.free, lv.dinv, 10, dtype=ld)[:2])
        assert abs(lv.theta - exact) <= 1e-10 * exact  # (float64 and longdouble agree: ten steps lose no orthogonality worth speaking of)


def test_estimate_of_a_diagonal_matrix():
    '''S A S = I.  With a start vector of 1024 entries +-1 and diagonal entries that are powers of 4 every operation is exact: alpha_0 = 1, beta_1 = 0, the
    recurrence stops after one step and theta = 1.  With the hash-derived start and a general diagonal the products round, beta_1 is a rounding and not 0,
    and the steps go on in that noise: every alpha is within gamma_(n + 8) of 1 and every beta within 8 u, so theta is within their sum of 1 (Gershgorin on
    the tridiagonal matrix).  Masked rows and rows with dinv = 0 take no part.'''
    A, free, dinv, u = exact_diagonal()
    alpha, beta, taken = lanczos(A, free, dinv, 10, u=u)
    assert taken == 1 and alpha[0] == 1 and beta[0] == 0 and theta_of(alpha, beta) == 1
    A, free = scalar_problem('diagonal')
    n = A.shape[0]
    alpha, beta, taken = lanczos(A, free, numpy.where(free, 1 / A.diagonal(), 0.), 10)
    theta = theta_of(alpha, beta)
    print(f'general diagonal: {taken} steps, theta - 1 = {theta - 1:.2e}, largest beta {beta.max():.2e}')
    assert abs(theta - 1) <= 2 * gamma(n + 8) + 16 * U


@pytest.mark.parametrize('name', ['laplace', 'small'])
def test_chebyshev_cycle_is_symmetric_positive_definite(name):
    '''M assembled densely by applying the cycle to the unit vectors, as test_cycle_is_symmetric_positive_definite of tests/test_amg_host.py does'''
    A, free, levels = case(name)
    assert len(levels) >= (3 if name == 'laplace' else 2)
    for degree in (1, 2, 3):
        M = chebyshev_cycle(levels, numpy.eye(A.shape[0]), degree)
        scale = abs(M).max()
        print(f'{name}, degree={degree}: |M - M^T| / |M| = {abs(M - M.T).max() / scale:.2e}')
        assert abs(M - M.T).max() <= 1e-12 * scale
        assert not M[~free].any() and not M[:, ~free].any()
        assert numpy.linalg.eigvalsh(M[free][:, free])[0] > 0


@functools.lru_cache(maxsize=None)
def iterations(name, smoother, count):
    '''iterations of the restatement's AMG-CG to rtol = 1e-8 from x = 0 with the right-hand side default_rng(4).normal'''
    A, free, levels = case(name)
    n = A.shape[0]
    b = numpy.random.default_rng(4).normal(size=n)
    M = (lambda r: cycle(levels, r, count)) if smoother == 'jacobi' else (lambda r: chebyshev_cycle(levels, r, count))
    x, it, starts, outcome = pcg_reference(A, b, numpy.zeros(n), free, M, (1e-8 * numpy.linalg.norm(b[free])) ** 2, n)
    assert outcome == 'converged'
    return it


@pytest.mark.parametrize('name', PROBLEMS)
def test_iteration_counts(name):
    '''degree 2 needs no more iterations than two Jacobi sweeps, which cost the same, and fewer products (5 a cycle and an iteration's own) than today's default of
    one sweep (3)'''
    jacobi1, jacobi2, cheb2, cheb3 = (iterations(name, *which) for which in (('jacobi', 1), ('jacobi', 2), ('chebyshev', 2), ('chebyshev', 3)))
    print(f'{name}: Jacobi sweeps 1: {jacobi1}, sweeps 2: {jacobi2}; Chebyshev degree 2: {cheb2}, degree 3: {cheb3}')
    assert cheb2 <= jacobi2
    assert 5 * cheb2 <= 3 * jacobi1
    assert cheb3 <= cheb2


def test_solve_argument_errors():
    '''raised before anything touches a device (there is none here)'''
    from nutils_amd import amg, matrix
    A = matrix.HipMatrix(numpy.array([2., 3.]), numpy.array([0, 1, 2]), numpy.array([0, 1]), 2)
    b = numpy.ones(2)
    cheb = lambda **kwargs: dict(smoother='chebyshev', **kwargs)
    for bad, message in ((dict(smoother='gauss-seidel'), 'smoother must be'), (dict(smoother=1), 'smoother must be'),
                         (cheb(degree=0), 'degree must be'), (cheb(degree=9), 'degree must be'), (cheb(degree=1.5), 'degree must be'), (cheb(degree=True), 'degree must be'),
                         (cheb(eigsteps=0), 'eigsteps must be'), (cheb(eigsteps=65), 'eigsteps must be'), (cheb(eigsteps=2.), 'eigsteps must be'),
                         (cheb(eigratio=1), 'eigratio must be'), (cheb(eigratio=numpy.nan), 'eigratio must be'), (cheb(eigratio=numpy.inf), 'eigratio must be'),
                         (cheb(eigratio='10'), 'eigratio must be'),
                         (cheb(sweeps=2), "sweeps counts the sweeps of the 'jacobi' smoother"),
                         (dict(degree=2), "arguments of smoother='chebyshev'"), (dict(smoother='jacobi', eigsteps=10), "arguments of smoother='chebyshev'"),
                         (dict(smoother='jacobi', eigratio=4.), "arguments of smoother='chebyshev'"),
                         (cheb(levels=3), 'invalid arguments'), (cheb(coarse=0), 'coarse must be')):
        with pytest.raises(matrix.MatrixError, match=message):
            A.solve(b, solver='cg', rtol=1e-8, precon='amg', preconargs=bad)
    for precon in ('diag', None):
        with pytest.raises(matrix.MatrixError, match='preconargs are the arguments of'):
            A.solve(b, solver='cg', rtol=1e-8, precon=precon, preconargs=cheb(degree=2))
    for solver in ('bicgstab', 'fgmres'):
        with pytest.raises(matrix.MatrixError, match='invalid preconditioner'):
            A.solve(b, solver=solver, rtol=1e-8, precon='amg', preconargs=cheb())
    assert A._dev is None  # nothing was uploaded
    B = numpy.ones((2, 1))
    coarse, sweeps, checked = amg.check_args(dict(nullspace=B), 2)  # (still three values)
    assert (coarse, sweeps) == (256, 1) and numpy.array_equal(checked, B)
    with pytest.raises(matrix.MatrixError, match='invalid arguments'):
        amg.check_args(cheb(), 2)  # (the smoother keys are split off before it)
    assert amg.split_smoother(None) == ({}, None) and amg.split_smoother(dict(smoother='jacobi', sweeps=2)) == (dict(sweeps=2), None)
    assert amg.split_smoother(cheb(coarse=16)) == (dict(coarse=16), dict(degree=2, eigsteps=10, eigratio=10.))
    assert amg.split_smoother(cheb(degree=numpy.int64(3), eigsteps=4, eigratio=4, sweeps=1)) == (dict(sweeps=1), dict(degree=3, eigsteps=4, eigratio=4.))


def test_start_vector_and_theta_of_the_package():
    '''nutils_amd.amg's start vector is the restatement's, number for number, and its host step from alpha, beta to theta is theta_of'''
    from nutils_amd import amg
    u = amg.start_vector(3000).numpy()
    assert numpy.array_equal(u, start_vector(3000)) and u.min() >= -1 and u.max() < 1 and abs(u.mean()) < .05
    A, free, levels = case('laplace')
    lv = levels[0]
    alpha, beta, taken = lanczos(lv.A, lv.free, lv.dinv, 10)
    out = numpy.zeros(21)
    out[0:20:2], out[1:20:2], out[20] = alpha, beta, taken
    assert amg.lanczos_theta(out) == (lv.theta, 10)
    out[20] = 3  # (three steps taken: the rest of the array is not read)
    assert amg.lanczos_theta(out) == (theta_of(alpha[:3], beta[:3]), 3)
    theta, taken = amg.lanczos_theta(numpy.zeros(21))
    assert numpy.isnan(theta) and taken == 0
