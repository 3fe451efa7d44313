'''CPU-side checks of the device MINRES solve for symmetric indefinite systems (matrix.HipMatrix.solve(solver='minres'), nh_csr.hip): a numpy restatement of
the iteration the kernels implement, step by step and cell by cell (`Recurrence`), the host loop of HipMatrix._minres around it (`minres_solve_reference`)
and one start of it (`minres_reference`); what pins the restatement (the minimum over the Krylov space by numpy.linalg.lstsq, scipy's minres, a direct
solve); the errors a solve raises before any device work, and what the C ABI refuses before it touches the device.  The restatement and the matrices here
are the CPU reference of tests/test_gpu_minres.py.'''
import ctypes
import functools
import os
import numpy
import pytest
import scipy.sparse
import scipy.sparse.linalg

from nutils_amd import _lib, matrix
from test_bicgstab_host import laplace2d, refused, csr, P

U = 2. ** -53
NVEC = 8  # x, r, r1, r2, v, q, w1, w2
NINIT = 6  # r, r1, r2, v, w1, w2


def gamma(n):
    '''the constant of a sum of n terms in any order (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.4)'''
    n = numpy.asarray(n, dtype=float)
    return n * U / (1 - n * U)


# ---- the matrices ----------------------------------------------------------------------------------------------------------

def block(nx, ny):
    '''[[L + s, C], [C, -(0.3 L + s)]] with L the 5-point Laplacian on nx x ny, s = diag(linspace(.5, 3, m)), C = L / 2 + I: symmetric and quasi-definite, half
    of its eigenvalues negative, a diagonal from -4.2 to 7.  Every 9th dof is held at 1.5.  Returns (K, constrain, rhs).'''
    L = laplace2d(nx, ny)
    m = nx * ny
    s = scipy.sparse.diags(numpy.linspace(.5, 3, m))
    C = L / 2 + scipy.sparse.identity(m)
    K = scipy.sparse.csr_matrix(scipy.sparse.bmat([[L + s, C], [C, -(.3 * L + s)]]))
    K.sort_indices()
    cons = numpy.full(2 * m, numpy.nan)
    cons[::9] = 1.5
    return K, cons, numpy.random.default_rng(5).normal(size=2 * m)


def tridiagonal(n=262445):
    '''off-diagonals -1, diagonal +-(3 + i % 4), negative where i % 3 == 0: Gershgorin keeps |lambda| >= 1.  Every 1000th dof is held at 2.'''
    i = numpy.arange(n)
    d = numpy.where(i % 3 == 0, -1., 1.) * (3 + i % 4)
    K = scipy.sparse.diags([-numpy.ones(n - 1), d, -numpy.ones(n - 1)], [-1, 0, 1], format='csr')
    cons = numpy.full(n, numpy.nan)
    cons[::1000] = 2.
    return K, cons, numpy.random.default_rng(4).normal(size=n)


def saddle():
    '''[[L + 0.1 I, B^T], [B, 0]], 120 + 40 rows, B sparse random of full rank: a saddle point whose second diagonal block is zero.  Every 9th dof of the first
    block is held at -.5.'''
    L = laplace2d(12, 10)
    rng = numpy.random.default_rng(6)
    B = scipy.sparse.random(40, 120, density=.08, random_state=rng, data_rvs=lambda size: rng.normal(size=size)) + scipy.sparse.csr_matrix((numpy.ones(40), (numpy.arange(40), 3 * numpy.arange(40) + 1)), (40, 120))
    K = scipy.sparse.csr_matrix(scipy.sparse.bmat([[L + .1 * scipy.sparse.identity(120), B.T], [B, None]]))
    K.sort_indices()
    cons = numpy.full(160, numpy.nan)
    cons[:120:9] = -.5
    return K, cons, numpy.random.default_rng(7).normal(size=160)


# ---- the algorithm, restated -----------------------------------------------------------------------------------------------

ST_DONE, ST_BAD = 1., 2.  # a status; 0 is "iterate"
# where the cells of the work array lie (the enum of nh_csr.hip); the first three are what kernels.minres_work documents
CELLS = dict(RR=0, FLAG=1, COUNT=2, ST=3, BETA=4, OLDB=5, DBAR=6, EPSLN=7, PHIBAR=8, CS=9, SN=10, COUNT_U=11, FLAG_U=12, ST_L=16, ALPHA=17)


class Recurrence:
    '''What lives on the device between nh_minres_init and the last nh_minres_iterate: the vectors x, r (the carried 2-norm residual), r1, r2, v, q, w1, w2 and
    the cells of the work array, each written by the step that writes it in nh_csr.hip (k_minres_init, k_minres_init_scalars, k_minres_first: `init`; the
    product with its v . q epilogue, k_minres_lanczos, k_minres_update: the three steps of an iteration; k_minres_finish, at the end of every `iterate`).
    Preconditioned MINRES of Paige and Saunders in the variable names of scipy.sparse.linalg.minres, M^-1 = diag(dinv) > 0 or the identity (dinv None); the
    y of scipy is not stored: it is dinv r2.  alpha is v . A v, taken before the r1 term is subtracted.  A step that receives a status passes it on and does
    nothing else.  All vectors vanish on the rows `free` masks.  `product` is y = A x on the arithmetic of the vectors (float64, or longdouble for a
    reference of the device's arithmetic).'''

    def __init__(self, product, free, dinv, x):
        self.product, self.free, self.dinv = product, free, dinv
        self.x = x.copy()
        self.starts = 0

    def M(self, y):
        return y if self.dinv is None else self.dinv * y

    def A(self, y):
        return numpy.where(self.free, self.product(y), 0)

    def init(self, r):
        t = r.dtype.type
        self.r, self.r1, self.r2 = r.copy(), r.copy(), r.copy()
        self.w1, self.w2, self.q, self.v = (numpy.zeros_like(r) for _ in range(4))
        ry, rr = r @ self.M(r), r @ r
        self.RRP = rr  # (the partials, summed)
        bad = not (numpy.isfinite(rr) and numpy.isfinite(ry) and (ry > 0 or (ry == 0 and rr == 0)))
        beta = numpy.sqrt(ry) if not bad else t(0)
        self.RR, self.FLAG, self.COUNT = rr, bad, 0
        self.ST = ST_BAD if bad else ST_DONE if rr == 0 else 0.
        self.FLAG_U, self.COUNT_U = bad, 0
        self.BETA, self.OLDB, self.DBAR, self.EPSLN, self.PHIBAR, self.CS, self.SN = beta, t(0), t(0), t(0), beta, t(-1), t(0)
        self.ST_L = self.ALPHA = None  # (not written yet)
        if self.ST == 0:
            self.v = self.M(r) / beta
        self.starts += 1

    def iterate(self, niter, stop_rr):
        for _ in range(niter):
            self.multiply()
            self.lanczos(stop_rr)
            self.update()
        self.RR, self.FLAG, self.COUNT = self.RRP, self.FLAG_U, self.COUNT_U  # k_minres_finish

    def multiply(self):
        if self.ST != 0:
            return
        self.q = self.A(self.v)
        self.VQ = self.v @ self.q

    def lanczos(self, stop_rr):
        '''alpha, r1 <- r2, r2 <- A v - (beta / oldb) r1 - (alpha / beta) r2, r2 . dinv r2; it is this step that finds r . r within the bound'''
        st = self.ST if self.ST != 0 else ST_DONE if self.RRP <= stop_rr else 0.
        if st == 0 and not numpy.isfinite(self.VQ):
            st = ST_BAD
        self.ST_L = st
        if st != 0:
            return
        self.ALPHA = alpha = self.VQ
        self.L = self.BETA, self.OLDB, self.DBAR, self.EPSLN, self.PHIBAR, self.CS, self.SN, self.COUNT_U  # (the cells that cross the iteration, relayed)
        y = self.q
        if self.OLDB != 0:
            y = y - (self.BETA / self.OLDB) * self.r1
        y = y - (alpha / self.BETA) * self.r2
        self.r1, self.r2 = self.r2, y
        self.RYP = y @ self.M(y)

    def update(self):
        '''beta, the rotation, w1 <- w2, w2 <- (v - oldeps w1 - delta w2) / gamma, x += phi w2, r <- sn^2 r - (phibar cs / beta) r2, v <- dinv r2 / beta'''
        if self.ST_L != 0:
            self.ST = self.ST_L
            if self.ST_L == ST_BAD:
                self.FLAG_U = True
            return
        beta, oldb, dbar, epsln, phibar, cs, sn, count = self.L
        alpha, ry = self.ALPHA, self.RYP
        zero = self.x.dtype.type(0)
        bad = not (numpy.isfinite(ry) and ry >= 0)
        betan = numpy.sqrt(ry) if not bad else zero
        oldeps = epsln
        delta = cs * dbar + sn * alpha
        gbar = sn * dbar - cs * alpha
        epsln = sn * betan
        dbar = -cs * betan
        gam = numpy.hypot(gbar, betan)
        bad = bad or not (gam > 0 and numpy.isfinite(gam))
        if not bad:
            cs, sn = gbar / gam, betan / gam
            phi, phibar = cs * phibar, sn * phibar
            bad = not (numpy.isfinite(phi) and numpy.isfinite(delta))
        if bad:
            self.ST, self.FLAG_U = ST_BAD, True
            return
        self.ST = ST_DONE if betan == 0 else 0.  # (beta = 0 with gamma > 0: the Krylov space is exhausted; the step is taken)
        self.BETA, self.OLDB, self.DBAR, self.EPSLN, self.PHIBAR, self.CS, self.SN, self.COUNT_U = betan, beta, dbar, epsln, phibar, cs, sn, count + 1
        w = (self.v - oldeps * self.w1 - delta * self.w2) / gam
        self.w1, self.w2 = self.w2, w
        self.x = self.x + phi * w
        self.r = sn * sn * self.r
        if betan != 0:
            self.r = self.r - (phibar * cs / betan) * self.r2
            self.v = self.M(self.r2) / betan
        self.RRP = self.r @ self.r


def minres_reference(A, rhs, start, free, dinv, stop_rr, maxiter):
    '''One start of the recurrence from the true residual mask(rhs - A start), iterated until it stops itself or has moved x `maxiter` times.  Returns
    (x, iterations that moved x, flag).'''
    rec = Recurrence(lambda y: A @ y, free, dinv, numpy.array(start, dtype=float))
    rec.init(numpy.where(free, rhs - A @ rec.x, 0.))
    while rec.ST == 0 and rec.COUNT < maxiter:
        rec.iterate(1, stop_rr)
    if rec.ST == 0:
        rec.iterate(0, stop_rr)
    return rec.x, rec.COUNT, rec.FLAG


def minres_solve_reference(A, b, x, free, dinv, stop_rr, maxiter, check=16):
    '''The host loop of HipMatrix._minres around a `Recurrence`: a start from the true residual mask(b - A x), up to `check` iterations between two looks at
    r . r, the flag and the count, a new start once the recurrence is within the bound or has raised its flag after progress.  Returns (x, iterations,
    starts, outcome), outcome 'converged', 'maxiter', 'breakdown' (at the first step after a start) or 'non-finite'.'''
    mask = lambda y: numpy.where(free, y, 0.)
    rec = Recurrence(lambda y: A @ y, free, dinv, numpy.array(x, dtype=float))
    it = 0
    while True:
        rec.init(mask(b - A @ rec.x))
        if not numpy.isfinite(rec.RR):
            return rec.x, it, rec.starts, 'non-finite'
        if rec.RR <= stop_rr:
            return rec.x, it, rec.starts, 'converged'
        if it >= maxiter:
            return rec.x, it, rec.starts, 'maxiter'
        start = it
        while it < maxiter:
            rec.iterate(min(check, maxiter - it), stop_rr)
            it = start + rec.COUNT
            if rec.FLAG:
                if not rec.COUNT:
                    return rec.x, it, rec.starts, 'breakdown'
                break
            if not numpy.isfinite(rec.RR):
                return rec.x, it, rec.starts, 'non-finite'
            if rec.RR <= stop_rr:
                break


# ---- what pins the restatement ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def small():
    '''block(8, 8) reduced to its free dofs: (K, cons, rhs, free, start, r0 = mask(rhs - K start), the free block dense, its singular values)'''
    K, cons, rhs = block(8, 8)
    free, start = matrix.constraints(K.shape[1], cons)
    r0 = numpy.where(free, rhs - K @ start, 0.)
    Kff = K.toarray()[free][:, free]
    return K, cons, rhs, free, start, r0, Kff, numpy.linalg.svd(Kff, compute_uv=False)


def krylov_basis(Aff, r, k):
    '''an orthonormal basis of span(r, A r, .., A^(k-1) r), by Arnoldi with every vector orthogonalised twice against all before it'''
    Q = [r / numpy.linalg.norm(r)]
    for _ in range(k - 1):
        w = Aff @ Q[-1]
        for _ in range(2):
            for q in Q:
                w = w - (q @ w) * q
        Q.append(w / numpy.linalg.norm(w))
    return numpy.array(Q).T


def steps(jacobi, k, stop_rr=0.):
    '''the recurrence on block(8, 8) after k iterations'''
    K, cons, rhs, free, start, r0, Kff, sv = small()
    dinv = numpy.where(free, 1 / numpy.abs(K.diagonal()), 0.) if jacobi else None
    rec = Recurrence(lambda y: K @ y, free, dinv, start)
    rec.init(r0)
    rec.iterate(k, stop_rr)
    return rec


@pytest.mark.parametrize('jacobi', [False, True], ids=['plain', 'jacobi'])
def test_iterates_minimise_over_the_krylov_space(jacobi):
    '''After k = 1 .. 10 steps the iterate has the residual norm -- in the 2-norm without a preconditioner, in the M^-1-norm with Jacobi, where the system is
    M^-1/2 K M^-1/2 -- of the least-squares minimum over the Krylov space, and phibar is that norm.  Bound: the computed iterate is the exact one of a Lanczos
    process whose k steps each commit a relative error of gamma_(len + 8) (a row of at most 6 entries, two axpys, a normalisation), which the solution of
    the projected problem carries into the residual with a factor of at most the condition number (7 .. 9 here): k gamma_16 cond |r0| in all, 2e-13 |r0|
    at k = 10.  The two agree to 1e-14 |r0| in fact.'''
    K, cons, rhs, free, start, r0, Kff, sv = small()
    assert free.sum() == 113 and (numpy.linalg.eigvalsh(Kff) < 0).sum() > 40 and 6 < sv[0] / sv[-1] < 10
    m = numpy.sqrt(1 / numpy.abs(K.diagonal()[free])) if jacobi else numpy.ones(free.sum())  # M^-1/2
    Ah, rh = m[:, None] * Kff * m, m * r0[free]
    cond = numpy.linalg.cond(Ah)
    nrm = numpy.linalg.norm(rh)
    for k in range(1, 11):
        rec = steps(jacobi, k)
        assert rec.COUNT == k and not rec.FLAG and rec.ST == 0
        Q = krylov_basis(Ah, rh, k)
        c = numpy.linalg.lstsq(Ah @ Q, rh, rcond=None)[0]
        best = numpy.linalg.norm(rh - Ah @ (Q @ c))
        true = numpy.linalg.norm(m * (rhs - K @ rec.x)[free])
        bound = k * gamma(16) * cond * nrm
        print(f'k = {k}: minimum {best:.6e}, |r| - minimum {true - best:.1e}, phibar - minimum {rec.PHIBAR - best:.1e}, bound {bound:.1e}')
        assert abs(true - best) <= bound and abs(rec.PHIBAR - best) <= bound
        assert numpy.array_equal(rec.x[~free], start[~free])
        for y in (rec.r, rec.r1, rec.r2, rec.v, rec.q, rec.w1, rec.w2):
            assert not y[~free].any()


@pytest.mark.parametrize('jacobi', [False, True], ids=['plain', 'jacobi'])
def test_carried_residual_follows_the_true_one(jacobi):
    '''r <- sn^2 r - (phibar cs / beta) r2 is an identity of the Lanczos relation A V_k = V_(k+1) T_k, which holds step by step to rounding whatever becomes of
    the orthogonality.  A step's local error is gamma_c (|A| |x_k - x_(k-1)| + |r_(k-1)|) with c = 16 as above, and |x_k - x_(k-1)| <= 2 |r_(k-1)| / sigma_min
    since both residuals are at most |r_(k-1)|; residual norms do not rise, so over k steps the gap is within k gamma_16 (2 cond + 1) |r0|, and times
    max(1, |M|^1/2 |M^-1|^1/2) with Jacobi, where it is the M^-1-norm that does not rise.  Measured: 2e-14 |r0| over a solve to 1e-10.'''
    K, cons, rhs, free, start, r0, Kff, sv = small()
    d = numpy.abs(K.diagonal()[free])
    scale = numpy.sqrt(d.max() / d.min()) if jacobi else 1.
    nrm = numpy.linalg.norm(r0)
    rec = steps(jacobi, 0)
    worst = 0
    for k in range(1, 114):
        rec.iterate(1, (1e-10 * nrm) ** 2)
        if rec.ST != 0:
            break
        gap = numpy.linalg.norm(numpy.where(free, rhs - K @ rec.x, 0.) - rec.r)
        worst = max(worst, gap / nrm)
        assert gap <= k * gamma(16) * (2 * sv[0] / sv[-1] + 1) * scale * nrm, (k, gap / nrm)
        if not jacobi:
            assert abs(rec.PHIBAR - numpy.sqrt(rec.RRP)) <= k * gamma(16) * (2 * sv[0] / sv[-1] + 1) * nrm
    print(f'jacobi={jacobi}: stopped after {rec.COUNT} iterations, largest gap {worst:.1e} |r0|')
    assert rec.ST == ST_DONE and not rec.FLAG and 40 < rec.COUNT < 100
    assert rec.RR <= (1e-10 * nrm) ** 2 and rec.RR == rec.RRP
    before = [y.copy() for y in (rec.x, rec.r, rec.r1, rec.r2, rec.v, rec.w1, rec.w2)], rec.COUNT
    rec.iterate(3, (1e-10 * nrm) ** 2)  # past the stop nothing moves
    assert rec.COUNT == before[1] and all(numpy.array_equal(a, c) for a, c in zip(before[0], (rec.x, rec.r, rec.r1, rec.r2, rec.v, rec.w1, rec.w2)))


@pytest.mark.parametrize('name,jacobi', [('block8', False), ('block8', True), ('block27', False), ('block27', True), ('saddle', False)])
def test_reference_agrees_with_scipy_and_a_direct_solve(name, jacobi):
    K, cons, rhs = saddle() if name == 'saddle' else block(*{'block8': (8, 8), 'block27': (27, 27)}[name])
    n = K.shape[0]
    free, start = matrix.constraints(n, cons)
    dinv = numpy.where(free, 1 / numpy.abs(K.diagonal()), 0.) if jacobi else None
    b = (rhs - K @ start)[free]
    r0 = numpy.linalg.norm(b)
    x, it, flag = minres_reference(K, rhs, start, free, dinv, (1e-10 * r0) ** 2, int(free.sum()))
    print(f'{name}, jacobi={jacobi}: {it} iterations for {free.sum()} free dofs')
    assert not flag and 0 < it < .95 * free.sum()
    assert numpy.array_equal(x[~free], start[~free])
    res = numpy.linalg.norm((rhs - K @ x)[free])
    assert res <= 1e-10 * r0 * (1 + 1e-3)
    Kff = K[free][:, free]
    smin = numpy.linalg.svd(Kff.toarray(), compute_uv=False)[-1]
    assert smin > 1e-3
    direct = start.copy()
    direct[free] += scipy.sparse.linalg.spsolve(Kff.tocsc(), b)
    assert numpy.linalg.norm(x - direct) <= res / smin * (1 + 1e-6) + 1e-13 * numpy.linalg.norm(direct)
    try:
        y, info = scipy.sparse.linalg.minres(Kff, b, rtol=1e-11, maxiter=5 * n)
    except TypeError:  # (scipy before 1.12 calls it tol)
        y, info = scipy.sparse.linalg.minres(Kff, b, tol=1e-11, maxiter=5 * n)
    assert info == 0
    assert numpy.linalg.norm(x[free] - start[free] - y) <= (res + numpy.linalg.norm(b - Kff @ y)) / smin
    # through the host loop: the same iteration, a second start that finds the true residual within the bound or goes on
    z, its, starts, outcome = minres_solve_reference(K, rhs, start, free, dinv, (1e-10 * r0) ** 2, int(free.sum()))
    assert outcome == 'converged' and its >= it and starts >= 2
    if starts == 2:
        assert its == it and numpy.array_equal(z.view(numpy.int64), x.view(numpy.int64))


def test_estimate_never_rises_on_a_definite_matrix():
    K = laplace2d(9, 7)
    n = K.shape[0]
    rng = numpy.random.default_rng(3)
    b = rng.normal(size=n)
    free = rng.uniform(size=n) < .8
    rec = Recurrence(lambda y: K @ y, free, None, numpy.zeros(n))
    rec.init(numpy.where(free, b, 0.))
    estimates, stop_rr = [rec.PHIBAR], 1e-20 * rec.RR
    while rec.ST == 0 and rec.COUNT < n:
        rec.iterate(1, stop_rr)
        if rec.ST == 0:
            estimates.append(rec.PHIBAR)
    assert rec.ST == ST_DONE and len(estimates) > 10
    assert (numpy.diff(estimates) <= 0).all()


def test_same_result_for_any_check():
    '''the iterations enqueued past convergence do nothing: iterations, starts and the bytes of x do not depend on `check`; nor does a maxiter that is no
    multiple of it'''
    K, cons, rhs, free, start, r0, Kff, sv = small()
    stop_rr = (1e-10 * numpy.linalg.norm(r0)) ** 2
    results = [minres_solve_reference(K, rhs, start, free, None, stop_rr, 113, check=check) for check in (1, 5, 16)]
    x, it, starts, outcome = results[0]
    assert outcome == 'converged' and it > 7
    for y, it_c, starts_c, outcome_c in results[1:]:
        assert (it_c, starts_c, outcome_c) == (it, starts, outcome) and numpy.array_equal(y.view(numpy.int64), x.view(numpy.int64))
    cut = [minres_solve_reference(K, rhs, start, free, None, stop_rr, 7, check=check) for check in (1, 5, 16)]
    for y, *rest in cut:
        assert rest == [7, 2, 'maxiter'] and numpy.array_equal(y.view(numpy.int64), cut[0][0].view(numpy.int64))


def test_defined_small_cases():
    free = numpy.ones(2, dtype=bool)
    D = numpy.diag([1., -1.])
    x, it, flag = minres_reference(D, numpy.array([1., 2.]), numpy.zeros(2), free, None, 1e-24, 2)
    assert not flag and it == 2 and numpy.allclose(x, [1., -2.], rtol=1e-12, atol=0)
    # v . A v = 0 at the first step is no breakdown of MINRES: the step leaves x where it is (cs = 0) and the second one solves the system
    x, it, flag = minres_reference(D, numpy.array([1., 1.]), numpy.zeros(2), free, None, 1e-24, 2)
    assert not flag and it == 2 and numpy.allclose(x, [1., -1.], rtol=1e-12, atol=0)
    x, it, flag = minres_reference(numpy.array([[0., 1.], [1., 0.]]), numpy.array([1., 0.]), numpy.zeros(2), free, None, 1e-24, 2)
    assert not flag and it == 2 and numpy.allclose(x, [0., 1.], rtol=1e-12, atol=1e-16)
    # an eigenvector for a right-hand side: beta = 0 with gamma > 0, the Krylov space is exhausted, the step is taken and the iteration stops
    x, it, flag = minres_reference(D, numpy.array([0., 2.]), numpy.zeros(2), free, None, 1e-24, 2)
    assert not flag and it == 1 and numpy.array_equal(x, [0., -2.])
    # the zero matrix: gamma = 0, the flag
    assert minres_reference(numpy.zeros((2, 2)), numpy.array([1., 1.]), numpy.zeros(2), free, None, 1e-24, 2)[1:] == (0, True)
    assert minres_solve_reference(numpy.zeros((2, 2)), numpy.array([1., 1.]), numpy.zeros(2), free, None, 1e-24, 2)[1:] == (0, 1, 'breakdown')
    assert minres_solve_reference(D, numpy.array([1., numpy.inf]), numpy.zeros(2), free, None, 1e-24, 2)[1:] == (0, 1, 'non-finite')
    # a preconditioner that is not positive: r . M^-1 r < 0
    assert minres_reference(D, numpy.array([1., 2.]), numpy.zeros(2), free, numpy.array([1., -1.]), 1e-24, 2)[1:] == (0, True)


def test_a_nonsymmetric_matrix_is_not_solved():
    '''the recurrence takes symmetry for granted: on a nonsymmetric matrix its residual goes its own way, the true one stays, and the host loop, which trusts the
    true one alone, runs out of iterations'''
    from test_bicgstab_host import skewed
    N = skewed(laplace2d(9, 7), 2.)
    n = N.shape[0]
    b = numpy.random.default_rng(3).normal(size=n)
    free = numpy.ones(n, dtype=bool)
    r0 = numpy.linalg.norm(b)
    x, it, starts, outcome = minres_solve_reference(N, b, numpy.zeros(n), free, None, (1e-10 * r0) ** 2, 40)
    assert outcome == 'maxiter' and it == 40
    assert numpy.linalg.norm(b - N @ x) > 1e-6 * r0


# ---- C ABI -----------------------------------------------------------------------------------------------------------------

NAMES = 'nh_minres_work_doubles', 'nh_minres_init', 'nh_minres_iterate'


def test_names_in_signatures_and_header():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'nutils_hip.h')).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and name + '(' in header
    assert len(_lib.SIGNATURES['nh_minres_init'][1]) == 4 + NINIT  # n, dinv, the vectors but x and q, work, stream
    assert len(_lib.SIGNATURES['nh_minres_iterate'][1]) == 7 + NVEC  # A, rowmask, dinv, the vectors, work, stop_rr, niter, stream


def iterate(A, vectors=None, work=P, stop_rr=1e-20, niter=1):
    return _lib.load().nh_minres_iterate(A, None, None, *([P] * NVEC if vectors is None else vectors), work, stop_rr, niter, None)


def test_abi_refusals():
    lib = _lib.load()
    A = ctypes.byref(csr())
    refused(iterate(None), 'nh_minres_iterate', 'NULL matrix')
    for i in range(NVEC):
        vectors = [P] * NVEC
        vectors[i] = None
        refused(iterate(A, vectors), 'nh_minres_iterate', 'NULL vector')
    refused(iterate(A, work=None), 'nh_minres_iterate', 'NULL vector')
    refused(iterate(ctypes.byref(csr(ncols=4))), 'nh_minres_iterate', 'square')
    refused(iterate(A, niter=-1), 'nh_minres_iterate', 'negative iteration count')
    refused(iterate(A, stop_rr=-1e-300), 'nh_minres_iterate', 'negative')
    refused(iterate(A, stop_rr=float('nan')), 'nh_minres_iterate', 'negative')
    for fields, word in ((dict(nrows=-1), 'negative size'), (dict(lanes=3), 'power of two'), (dict(rowptr=None), 'NULL row pointers'), (dict(values=None), 'NULL values')):
        refused(iterate(ctypes.byref(csr(**fields))), 'nh_minres_iterate', word)
    refused(lib.nh_minres_init(-1, None, *[P] * NINIT, P, None), 'nh_minres_init', 'negative size')
    for i in range(NINIT):
        vectors = [P] * NINIT
        vectors[i] = None
        refused(lib.nh_minres_init(3, None, *vectors, P, None), 'nh_minres_init', 'NULL vector')
    refused(lib.nh_minres_init(3, None, *[P] * NINIT, None, None), 'nh_minres_init', 'NULL vector')
    none = ctypes.byref(csr(nrows=0, ncols=0, nnz=0, values=None, rowptr=None, colidx=None))
    assert iterate(none, vectors=[None] * NVEC, niter=4) == 0  # an empty matrix: no launch
    assert lib.nh_minres_work_doubles() > max(CELLS.values())


# ---- solve: errors before any device work ----------------------------------------------------------------------------------

def test_solve_errors_come_before_any_device_work():
    A = matrix.HipMatrix(numpy.array([2., -1., -1., -3.]), numpy.array([0, 2, 4]), numpy.array([0, 1, 0, 1]), 2)
    with pytest.raises(matrix.MatrixError, match='tolerance'):
        A.solve(numpy.ones(2), solver='minres')
    with pytest.raises(matrix.MatrixError, match='tolerance'):
        A.solve(numpy.ones(2), solver='minres', atol=0., rtol=0.)
    with pytest.raises(matrix.MatrixError, match='preconditioner'):
        A.solve(numpy.ones(2), solver='minres', rtol=1e-8, precon='amg')
    with pytest.raises(matrix.MatrixError, match='preconditioner'):
        A.solve(numpy.ones(2), solver='minres', rtol=1e-8, preconargs=dict(coarse=16))
    with pytest.raises(matrix.MatrixError, match='one vector'):
        A.solve(numpy.ones((2, 2)), solver='minres', rtol=1e-8)
    assert A._dev is None and A.iterations is None  # nothing was uploaded
