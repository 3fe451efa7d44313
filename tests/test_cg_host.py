'''CPU-side checks of the device conjugate-gradient solve (matrix.HipMatrix.solve(solver='cg'), nh_csr.hip): a numpy restatement of the three kernels of an
iteration and of the host loop around them, cell by cell, checked against a direct solve, on the indefinite matrices the solve must refuse, on a family of
diagonal systems that the iterations enqueued past convergence used to report as not positive definite, and on a system that needs a restart from the true
residual.  The restatement (`Recurrence`, `cg_reference`) is the CPU reference of tests/test_gpu_cg.py.'''
import functools
import numpy
import pytest
import scipy.sparse
import scipy.sparse.linalg

from test_bicgstab_host import laplace2d

U = 2. ** -53
DBL_MAX = numpy.finfo(float).max


# ---- the algorithm, restated ---------------------------------------------------------------------------------------------

class Recurrence:
    '''What lives on the device between nh_cg_init and the last nh_cg_iterate: x, r, p, q and the cells of the work array, each written by the kernel that
    writes it in nh_csr.hip (k_cg_init and k_cg_init_scalars: `init`; the product with its p . q epilogue, k_cg_update and k_cg_direction: `iterate`).  All
    vectors vanish on the rows `free` masks.  `product` is y = A x on the arithmetic of the vectors (float64, or longdouble for a reference of the device's
    arithmetic).  `idle`: an iteration that finds r . r <= the STOP cell does nothing; False is the rule the kernels had before, done only at r . r == 0.'''

    def __init__(self, product, free, dinv, x, idle=True):
        self.product, self.free, self.dinv, self.idle = product, free, dinv, idle
        self.x = x.copy()
        self.starts = 0

    def z(self):
        return self.r if self.dinv is None else self.dinv * self.r

    def init(self, r):
        self.r = r.copy()
        self.p = self.z().copy()
        self.RZP, self.RRP = self.r @ self.p, self.r @ self.r  # (the partials, summed)
        self.RR, self.RZ_A, self.RZ_B, self.FLAG_A, self.FLAG_B, self.STOP = self.RRP, self.RZP, self.RZP, False, False, 0.
        self.starts += 1

    def stop(self, stop_rr):
        self.STOP = stop_rr

    def iterate(self, niter=1):
        for _ in range(niter):
            # the product and its epilogue
            self.q = numpy.where(self.free, self.product(self.p), 0)
            pq = self.p @ self.q
            # k_cg_update
            rz, rr, bad = self.RZ_B, self.RR, self.FLAG_A
            done = rr <= self.STOP if self.idle else rr == 0
            if not done and not bad:
                bad = not (0 < rz <= DBL_MAX and 0 < pq <= DBL_MAX)
            self.RZ_A, self.FLAG_B = rz, bad
            if not (done and self.idle):
                if not done and not bad:  # move
                    alpha = rz / pq
                    self.x = self.x + alpha * self.p
                    self.r = self.r - alpha * self.q
                self.RZP, self.RRP = self.r @ self.z(), self.r @ self.r
            # k_cg_direction
            rz, rr, rz_old, bad = self.RZP, self.RRP, self.RZ_A, self.FLAG_B
            self.RR, self.RZ_B, self.FLAG_A = rr, rz_old if bad else rz, bad
            if bad or self.idle and rr <= self.STOP:
                continue
            beta = rz / rz_old if rz_old != 0 else 0 * rz
            self.p = self.z() + beta * self.p


def cg_reference(A, b, x, free, dinv, stop_rr, maxiter, check=16, idle=True):
    '''The host loop of HipMatrix._cg around a `Recurrence`: a start from the true residual mask(b - A x), `check` iterations between two looks at r . r and
    the flag, a new start once the recurrence is within the bound.  Returns (x, iterations, starts, outcome), outcome 'converged', 'maxiter' or 'flagged'.'''
    mask = lambda y: numpy.where(free, y, 0.)
    rec = Recurrence(lambda y: A @ y, free, dinv, numpy.array(x, dtype=float), idle)
    it = 0
    while True:
        rec.init(mask(b - A @ rec.x))
        assert numpy.isfinite(rec.RR)
        if rec.RR <= stop_rr:
            return rec.x, it, rec.starts, 'converged'
        if it >= maxiter:
            return rec.x, it, rec.starts, 'maxiter'
        rec.stop(stop_rr)
        while it < maxiter:
            steps = min(check, maxiter - it)
            rec.iterate(steps)
            it += steps
            if rec.FLAG_B:
                return rec.x, it, rec.starts, 'flagged'
            assert numpy.isfinite(rec.RR)
            if rec.RR <= stop_rr:
                break


# ---- problems ------------------------------------------------------------------------------------------------------------

SCALES = [2. ** (-6 * k) for k in range(18)]  # of the right-hand side: whatever the trajectory, some of them put the idle iterations into the subnormal range


@functools.lru_cache(maxsize=None)
def diagonal_family(permutation=None, scale=1e12, n=1480):
    '''(d, b): a positive diagonal matrix -- a lumped mass matrix, say -- and a right-hand side, both under a random symmetric permutation (another order of
    every sum) if `permutation` is a seed.  Made once, never written.'''
    rng = numpy.random.default_rng(20)
    d, b = scale * rng.uniform(1, 10, n), rng.normal(size=n)
    if permutation is not None:
        perm = numpy.random.default_rng(permutation).permutation(n)
        d, b = d[perm], b[perm]
    return d, b


@functools.lru_cache(maxsize=None)
def restart_case(n=300):
    '''(A, b, x0, solution) of a solve that needs a restart: unpreconditioned CG on the 1-D Laplace matrix from a large smooth start vector.  The residual of the
    recurrence, r -= alpha q some 300 times over, drifts from mask(b - A x) by rounding errors of the size u |A| |x0|; |r0| is lambda_min |x0|, so the drift is
    4e-12 |r0| whatever the size of x0, well above rtol = 1e-13 -- while the solution itself is small, so that a second start can meet the bound, and so
    that the error of evaluating a residual in double, u |A| |x|, is 1e-4 of the bound.  b = fl(A w), so the solution is w up to u |A| |w| / lambda_min = 7e-11
    (a direct solve from x0 is no better than u cond(A) |x0| = 5e-5).  Made once, never written.'''
    A = scipy.sparse.diags([-numpy.ones(n - 1), 2 * numpy.ones(n), -numpy.ones(n - 1)], [-1, 0, 1], format='csr')
    w = numpy.random.default_rng(6).normal(size=n)
    return A, A @ w, 1e6 * numpy.sin(numpy.pi * numpy.arange(1, n + 1) / (n + 1)), w


def gamma(n):
    '''the constant of a sum of n terms in any order (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.4)'''
    return n * U / (1 - n * U)


def one_step_of_jacobi(x, rhs, d):
    '''What Jacobi-CG from zero leaves of the diagonal system d x = rhs when nothing happens after its first iteration: x = alpha p bit for bit, with
    p = fl(rhs fl(1 / d)) and ONE scalar alpha = r . z / p . q.  In exact arithmetic alpha is 1, and then x = p is within 2u of fl(rhs / d) (a product with the
    rounded reciprocal is within one ulp of the rounded quotient).  In floating point r . z and p . q are two sums of n positive terms that agree term by term
    to 3u (q_i = fl(d_i p_i) against r_i), each summed to gamma_n in any order, and a division: |alpha - 1| <= 2 gamma_n + 4u, in practice 1 or one of its
    neighbours, and alpha p is rounded once more unless alpha is 1 (numpy: alpha = 1 - u in two of the four orders of summation below, and
    max |x - rhs / d| / |rhs / d| = 3.94u with it, 2.00u with alpha = 1).  Returns alpha.'''
    p = rhs * (1 / d)
    j = numpy.abs(p).argmax()
    guess = x[j] / p[j]
    alpha = [a for a in (numpy.nextafter(guess, 0), guess, numpy.nextafter(guess, 2)) if numpy.array_equal(a * p, x)]
    assert alpha, (guess, numpy.abs(x / p - 1).max() / U)  # an iteration past the first moved x
    alpha = min(alpha, key=lambda a: abs(a - 1))
    assert abs(alpha - 1) <= 2 * gamma(len(d)) + 4 * U, alpha
    assert (numpy.abs(x - rhs / d) <= (2 * U + (alpha != 1) * (abs(alpha - 1) + U) * (1 + 2 * U)) * numpy.abs(rhs / d)).all()
    return alpha


# ---- tests ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('idle', [True, False])
@pytest.mark.parametrize('jacobi', [True, False])
def test_reference_agrees_with_a_direct_solve(jacobi, idle):
    A = laplace2d(9, 7)
    n = A.shape[0]
    rng = numpy.random.default_rng(3)
    s = scipy.sparse.diags(rng.uniform(.5, 2., n))
    A = scipy.sparse.csr_matrix(s @ A @ s)  # (a diagonal that Jacobi has something to do with)
    b = rng.normal(size=n)
    free = rng.uniform(size=n) < .8
    x0 = numpy.where(free, 0., rng.normal(size=n))  # constrained dofs held at non-zero values
    dinv = numpy.where(free, 1 / A.diagonal(), 0.) if jacobi else None
    r0 = numpy.linalg.norm((b - A @ x0)[free])
    rtol = 1e-11
    x, it, starts, outcome = cg_reference(A, b, x0, free, dinv, (rtol * r0) ** 2, n, check=1, idle=idle)
    assert outcome == 'converged' and 0 < it < n and starts == 2
    assert numpy.array_equal(x[~free], x0[~free])
    res = numpy.linalg.norm((b - A @ x)[free])
    assert res <= rtol * r0 * (1 + 1e-3)  # (the second start found the true residual within the bound)
    direct = x0.copy()
    direct[free] += scipy.sparse.linalg.spsolve(A[free][:, free].tocsc(), (b - A @ x0)[free])
    lmin = numpy.linalg.eigvalsh(A.toarray()[free][:, free])[0]
    assert numpy.linalg.norm(x - direct) <= res / lmin * (1 + 1e-6)
    # looking every 16 iterations: the same solution to the same bound, whole rounds of iterations
    y, it16, starts, outcome = cg_reference(A, b, x0, free, dinv, (rtol * r0) ** 2, n, idle=idle)
    assert outcome == 'converged' and it16 == min(-(-it // 16) * 16, n)
    assert numpy.linalg.norm((b - A @ y)[free]) <= rtol * r0 * (1 + 1e-3)
    if idle:
        assert numpy.array_equal(x, y)  # the iterations past convergence did nothing


@pytest.mark.parametrize('idle', [True, False])
def test_reference_on_the_small_cases(idle):
    '''the 2 x 2 and 3 x 3 systems of test_gpu_matrix_hip.test_solve_errors: indefiniteness is flagged whatever the rule for idle iterations'''
    free = numpy.ones(2, dtype=bool)
    D = numpy.diag([1., -1.])
    for rhs in ([1., 1.], [1., 2.]):  # (with [1, 1] and Jacobi r . z = 0: a vanishing r . z is a breakdown unless r . r is within the bound)
        for dinv in (numpy.array([1., -1.]), None):
            for check in (1, 16):
                x, it, starts, outcome = cg_reference(D, numpy.array(rhs), numpy.zeros(2), free, dinv, 1e-16 * numpy.dot(rhs, rhs), 2, check=check, idle=idle)
                assert outcome == 'flagged' and not x.any()
    A = numpy.array([[0., 1., 0.], [1., 2., 0.], [0., 0., 4.]])
    free = numpy.array([False, True, True])
    x0 = numpy.array([1., 0., 0.])
    b = numpy.array([9., 3., 2.])
    r0 = numpy.linalg.norm((b - A @ x0)[free])
    x, it, starts, outcome = cg_reference(A, b, x0, free, numpy.array([0., .5, .25]), (1e-12 * r0) ** 2, 2, idle=idle)
    assert outcome == 'converged' and numpy.allclose(x, [1., 1., .5], rtol=1e-12, atol=0)


@pytest.mark.parametrize('permutation', [None, 1, 2, 3])
def test_iterations_past_convergence(permutation):
    '''Jacobi-CG solves a diagonal system in one iteration; the other 15 of the first round ran on, r . r falling by some 32 decades each, and at the ninth to
    eleventh r . z = sum dinv_i r_i^2 was 0 with r . r still positive: a positive diagonal matrix reported as not positive definite.  With the bound in the
    STOP cell they do nothing.  The unpermuted order and three permutations: the outcome must not hang on one order of summation.'''
    d, b = diagonal_family(permutation)
    n = len(d)
    A = scipy.sparse.diags(d, format='csr')
    free = numpy.ones(n, dtype=bool)
    flagged = []
    for scale in SCALES:
        rhs = scale * b
        stop_rr = (1e-10 * numpy.linalg.norm(rhs)) ** 2
        flagged.append(cg_reference(A, rhs, numpy.zeros(n), free, 1 / d, stop_rr, n, idle=False)[3] == 'flagged')
        x, it, starts, outcome = cg_reference(A, rhs, numpy.zeros(n), free, 1 / d, stop_rr, n)
        assert outcome == 'converged' and (it, starts) == (16, 2)
        alpha = one_step_of_jacobi(x, rhs, d)
    print(f'permutation {permutation}: the rule without a bound flags {sum(flagged)} of {len(SCALES)}; alpha - 1 = {(alpha - 1) / U:+.0f} u')
    assert sum(flagged) >= 3  # (the inputs bite: without the bound these solves fail)


def test_a_restart_happens():
    A, b, x0, w = restart_case()
    n = A.shape[0]
    free = numpy.ones(n, dtype=bool)
    r0 = numpy.linalg.norm(b - A @ x0)
    for check in (1, 16):
        x, it, starts, outcome = cg_reference(A, b, x0, free, None, (1e-13 * r0) ** 2, 10 * n, check=check)
        print(f'check={check}: {starts} starts, {it} iterations')
        assert outcome == 'converged' and starts >= 3  # (the last start only finds the true residual within the bound: at least two iterated)
        res = numpy.linalg.norm(b - A @ x)
        assert res <= 1e-13 * r0 * (1 + 1e-3) and numpy.linalg.norm(x - w) <= res / (2 - 2 * numpy.cos(numpy.pi / (n + 1)))
