'''CPU-side checks of the device BiCGStab solve (matrix.HipMatrix.solve(solver='bicgstab'), nh_csr.hip): what the C ABI refuses before it touches the
device, the errors a solve raises before any device work, and a numpy restatement of the algorithm the kernels implement, checked against a direct solve.
The restatement (`bicgstab_reference`) is the CPU reference of tests/test_gpu_bicgstab.py.  A second restatement follows the kernels step by step and cell by
cell (`Recurrence`, `bicgstab_solve_reference`: the host loop of HipMatrix._bicgstab around it), agrees with the first bit for bit, and is the reference of
tests/test_gpu_bicgstab_steps.py, together with three small integer systems that break down in their second iteration, verified here in exact rational
arithmetic.'''
import ctypes
import fractions
import numpy
import pytest
import scipy.sparse
import scipy.sparse.linalg

from nutils_amd import _lib, matrix

P = ctypes.c_void_p(64)  # a non-NULL pointer that is never followed: every call below fails its argument checks first
NVEC = 9  # x, r, rhat, p, v, s, t, phat, shat


def csr(nrows=3, ncols=3, nnz=5, values=P, rowptr=P, colidx=P, col32=None, lanes=0):
    return _lib.Csr(nrows, ncols, nnz, values, rowptr, colidx, col32, lanes)


def refused(rc, *words):
    msg = _lib.load().nh_last_error()
    assert rc == -1, rc
    for word in words:
        assert word.encode() in msg, msg
    with pytest.raises(_lib.NutilsHipError):
        _lib.check(rc)


# ---- the algorithm, restated ---------------------------------------------------------------------------------------------

def bicgstab_reference(A, b, x, free, dinv, stop_rr, maxiter):
    '''Right-preconditioned BiCGStab on the rows `free` keeps, as the device kernels do it: M^-1 = diag(dinv) or the identity (dinv None), all vectors zero
    on masked rows, stop when the recurrence has r . r <= stop_rr.  Returns (x, iterations that moved x, breakdown).'''
    mask = lambda y: numpy.where(free, y, 0.)
    M = (lambda y: y) if dinv is None else (lambda y: dinv * y)
    x = numpy.array(x, dtype=float)
    r = mask(b - A @ x)
    rhat, rho, alpha, omega, p, v = r.copy(), 1., 1., 1., numpy.zeros_like(r), numpy.zeros_like(r)
    for it in range(maxiter):
        if r @ r <= stop_rr:
            return x, it, False
        rho, rho_old = rhat @ r, rho
        beta = (rho / rho_old) * (alpha / omega)
        if rho == 0 or not numpy.isfinite(rho) or not numpy.isfinite(beta):
            return x, it, True
        p = r + beta * (p - omega * v)
        phat = M(p)
        v = mask(A @ phat)
        rv = rhat @ v
        alpha = rho / rv if rv else numpy.nan
        if not numpy.isfinite(alpha):
            return x, it, True
        s = r - alpha * v
        shat = M(s)
        t = mask(A @ shat)
        tt = t @ t
        omega = (t @ s) / tt if tt else 0.
        if omega == 0 or not numpy.isfinite(omega):
            if s @ s > stop_rr:
                return x, it, True
            omega = 0.  # (no second half with s within the bound, t = 0 say: convergence at the half step)
        x += alpha * phat + omega * shat
        r = s - omega * t
    return x, maxiter, False


ST_DONE, ST_BAD = 1., 2.  # a status; 0 is "iterate"
# where the cells of the work array lie (the enum of nh_csr.hip); the first three are what kernels.bicgstab_work documents
CELLS = dict(RR=0, FLAG=1, COUNT=2, ST=3, ST_H=4, ST_U=5, RHO=6, RHO_OLD=7, ALPHA=8, OMEGA=9, COUNT_U=10)


class Recurrence:
    '''What lives on the device between nh_bicgstab_init and the last nh_bicgstab_iterate: the vectors x, r, rhat, p, v, s, t, phat, shat and the cells RR, FLAG,
    COUNT, ST, ST_H, ST_U, RHO, RHO_OLD, ALPHA, OMEGA, COUNT_U of the work array, each written by the step that writes it in nh_csr.hip (k_bicgstab_init and
    k_bicgstab_init_scalars: `init`; the product with its rhat . v epilogue, k_bicgstab_half, the product with its t . s and t . t epilogue, k_bicgstab_update,
    k_bicgstab_direction: the five steps of `iterate`).  A step that receives a status passes it on and does nothing else.  All vectors vanish on the rows
    `free` masks.  `product` is y = A x on the arithmetic of the vectors (float64, or longdouble for a reference of the device's arithmetic).  Without a
    preconditioner (dinv None) phat is p and shat is s, as on the device.  v, s, t, shat start as zeros (the device leaves them unset until an iteration writes
    them).'''

    def __init__(self, product, free, dinv, x):
        self.product, self.free, self.dinv = product, free, dinv
        self.x = x.copy()
        self.starts = 0

    def M(self, y):
        return y if self.dinv is None else self.dinv * y

    def A(self, y):
        return numpy.where(self.free, self.product(y), 0)

    def init(self, r):
        self.r, self.rhat, self.p = r.copy(), r.copy(), r.copy()
        self.phat = self.M(self.p)
        self.v, self.s, self.t = (numpy.zeros_like(r) for _ in range(3))
        self.shat = self.s if self.dinv is None else numpy.zeros_like(r)
        self.RRP = self.r @ self.r  # (the partials, summed)
        bad = not numpy.isfinite(self.RRP)
        self.RR, self.FLAG, self.COUNT = self.RRP, bad, 0
        self.ST = ST_BAD if bad else ST_DONE if self.RRP == 0 else 0.
        self.RHO = self.RRP
        self.RHO_OLD = self.ALPHA = self.OMEGA = r.dtype.type(1)
        self.zero = r.dtype.type(0)
        self.ST_H = self.ST_U = self.COUNT_U = None  # (not written yet)
        self.starts += 1

    def iterate(self, niter, stop_rr):
        for _ in range(niter):
            self.product1()
            self.half()
            self.product2()
            self.update(stop_rr)
            self.direction(stop_rr)

    def product1(self):
        if self.ST != 0:
            return
        self.v = self.A(self.phat)
        self.WY = self.rhat @ self.v

    def half(self):
        if self.ST != 0:
            self.ST_H = self.ST
            return
        rv, rho = self.WY, self.RHO
        alpha = rho / rv if rv != 0 else self.zero
        bad = not (rv != 0 and numpy.isfinite(rv) and numpy.isfinite(alpha))
        self.ST_H, self.RHO_OLD, self.ALPHA = ST_BAD if bad else 0., rho, alpha
        if bad:
            return
        self.s = self.r - alpha * self.v
        self.shat = self.M(self.s)
        self.SS = self.s @ self.s

    def product2(self):
        if self.ST_H != 0:
            return
        self.t = self.A(self.shat)
        self.WY, self.YY = self.t @ self.s, self.t @ self.t

    def update(self, stop_rr):
        if self.ST_H != 0:
            self.ST_U, self.COUNT_U = self.ST_H, self.COUNT
            return
        ts, tt, ss, alpha = self.WY, self.YY, self.SS, self.ALPHA
        omega = ts / tt if tt != 0 else self.zero
        bad = False
        if not (omega != 0 and numpy.isfinite(omega)):  # no second half: with s within the bound that is convergence at the half step
            omega = self.zero
            bad = not ss <= stop_rr
        self.ST_U, self.OMEGA, self.COUNT_U = ST_BAD if bad else 0., omega, self.COUNT if bad else self.COUNT + 1
        if bad:
            return
        self.x = self.x + (alpha * self.phat + omega * self.shat)
        self.r = self.s - omega * self.t
        self.RHOP, self.RRP = self.rhat @ self.r, self.r @ self.r

    def direction(self, stop_rr):
        self.COUNT = self.COUNT_U
        if self.ST_U != 0:
            self.ST = self.ST_U
            if self.ST_U == ST_BAD:
                self.FLAG = True
            return
        rho, rr, omega = self.RHOP, self.RRP, self.OMEGA
        done = rr <= stop_rr
        beta = self.zero if done or omega == 0 else (rho / self.RHO_OLD) * (self.ALPHA / omega)
        bad = not done and not (rho != 0 and numpy.isfinite(rho) and omega != 0 and numpy.isfinite(beta))
        self.RR, self.ST, self.RHO = rr, ST_DONE if done else ST_BAD if bad else 0., rho
        if bad:
            self.FLAG = True
        if done or bad:
            return
        self.p = self.r + beta * (self.p - omega * self.v)
        self.phat = self.M(self.p)


def bicgstab_solve_reference(A, b, x, free, dinv, stop_rr, maxiter, check=16):
    '''The host loop of HipMatrix._bicgstab around a `Recurrence`: a start from the true residual mask(b - A x) with a fresh shadow residual, up to `check`
    iterations between two looks at r . r, the flag and the count, a new start once the recurrence is within the bound or has broken down after progress.
    Returns (x, iterations, starts, outcome), outcome 'converged', 'maxiter', 'breakdown' (at the first step after a start) or 'non-finite'.'''
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


# ---- three systems that break down in their second iteration -----------------------------------------------------------------

# name: (A, b, x at the breakdown, r at the breakdown), from x = 0 without a preconditioner (the diagonals have zeros).  The name is the quantity that
# vanishes: rhat . r in the direction step of iteration 1, rhat . v in the half step of iteration 2, t . s (with s . s above the bound) in the update of
# iteration 2.  Everything the recurrence computes up to there is a dyadic rational of a few bits (`exact_breakdown`), so float64 is exact in any order of
# summation, fused or not, and so it is on kron(identity(N), A) with b tiled: the dots grow by the factor N, every ratio and every entry stays.
BREAKDOWNS = {
    'rhat . r': ([[-2, -2, -2], [-1, 1, 1], [1, 0, -2]], [2, 0, 0], [-1, .5, -.5], [0, -1, 0]),
    'rhat . v': ([[2, -2, 2], [0, 2, -2], [1, 1, 0]], [1, 1, 0], [.5, 1.5, 1], [1, 0, -2]),
    't . s': ([[2, 0, 1], [2, 0, 2], [0, 1, 1]], [0, 0, -1], [.5, 1, -1], [0, 1, -1]),
}


def tiled(name, N):
    '''(kron(identity(N), A) as CSR, b tiled, x tiled, r tiled) of a case of BREAKDOWNS'''
    A, b, x, r = BREAKDOWNS[name]
    K = scipy.sparse.csr_matrix(scipy.sparse.kron(scipy.sparse.identity(N), scipy.sparse.csr_matrix(numpy.array(A, dtype=float))))
    K.sort_indices()
    return (K,) + tuple(numpy.tile(numpy.array(y, dtype=float), N) for y in (b, x, r))


def exact_breakdown(A, b):
    '''BiCGStab from x = 0 without a preconditioner in exact rational arithmetic, until something vanishes.  Returns (what vanished, iterations that moved x,
    x, r, scalars, entries): every scalar (dots, alpha, omega, rho' / rho and alpha / omega separately, beta) and every vector entry computed on the way.'''
    F = fractions.Fraction
    product = lambda y: [sum(F(a) * yj for a, yj in zip(row, y)) for row in A]
    dot = lambda y, z: sum(yi * zi for yi, zi in zip(y, z))
    x, r = [F(0)] * len(b), [F(bi) for bi in b]
    rhat, p, rho = list(r), list(r), dot(r, r)
    scalars, entries, moved = [rho], list(r), 0
    while True:
        v = product(p)
        rv = dot(rhat, v)
        scalars.append(rv)
        entries += v
        if rv == 0:
            return 'rhat . v', moved, x, r, scalars, entries
        alpha = rho / rv
        s = [ri - alpha * vi for ri, vi in zip(r, v)]
        t = product(s)
        ts, tt = dot(t, s), dot(t, t)
        scalars += [alpha, ts, tt, dot(s, s)]
        entries += s + t
        if ts == 0 or tt == 0:
            return ('t . s' if dot(s, s) > 0 else 'converged at the half step'), moved, x, r, scalars, entries
        omega = ts / tt
        x = [xi + alpha * pi + omega * si for xi, pi, si in zip(x, p, s)]
        r = [si - omega * ti for si, ti in zip(s, t)]
        moved += 1
        rho, rho_old = dot(rhat, r), rho
        scalars += [omega, rho, dot(r, r)]
        entries += x + r
        if dot(r, r) == 0:
            return 'converged', moved, x, r, scalars, entries
        if rho == 0:
            return 'rhat . r', moved, x, r, scalars, entries
        scalars += [rho / rho_old, alpha / omega, (rho / rho_old) * (alpha / omega)]
        p = [ri + scalars[-1] * (pi - omega * vi) for ri, pi, vi in zip(r, p, v)]
        entries += p


def skewed(K, gamma=.5):
    '''K + gamma (triu(K, 1) - tril(K, -1)): nonsymmetric, with the symmetric part of K'''
    K = scipy.sparse.csr_matrix(K)
    return scipy.sparse.csr_matrix(K + gamma * (scipy.sparse.triu(K, 1) - scipy.sparse.tril(K, -1)))


def laplace2d(nx, ny):
    lap = lambda n: scipy.sparse.diags([-numpy.ones(n - 1), 2 * numpy.ones(n), -numpy.ones(n - 1)], [-1, 0, 1])
    return scipy.sparse.csr_matrix(scipy.sparse.kron(lap(nx), scipy.sparse.identity(ny)) + scipy.sparse.kron(scipy.sparse.identity(nx), lap(ny)))


@pytest.mark.parametrize('jacobi', [True, False])
def test_reference_agrees_with_a_direct_solve(jacobi):
    N = skewed(laplace2d(9, 7))
    n = N.shape[0]
    rng = numpy.random.default_rng(3)
    N = scipy.sparse.csr_matrix(scipy.sparse.diags(rng.uniform(.5, 2., n)) @ N)  # (a diagonal that Jacobi has something to do with)
    b = rng.normal(size=n)
    free = rng.uniform(size=n) < .8
    x0 = numpy.where(free, 0., rng.normal(size=n))  # constrained dofs held at non-zero values
    dinv = numpy.where(free, 1 / N.diagonal(), 0.) if jacobi else None
    r0 = numpy.linalg.norm((b - N @ x0)[free])
    rtol = 1e-11
    x, it, broke = bicgstab_reference(N, b, x0, free, dinv, (rtol * r0) ** 2, n)
    assert not broke and 0 < it < n
    assert numpy.array_equal(x[~free], x0[~free])
    res = numpy.linalg.norm((b - N @ x)[free])
    assert res <= 10 * rtol * r0  # (the recurrence's residual met the bound; the true one follows it to rounding)
    direct = x0.copy()
    direct[free] += scipy.sparse.linalg.spsolve(N[free][:, free].tocsc(), (b - N @ x0)[free])
    smin = numpy.linalg.svd(N.toarray()[free][:, free], compute_uv=False)[-1]
    assert numpy.linalg.norm(x - direct) <= res / smin * (1 + 1e-6)


def test_reference_on_the_defined_small_cases():
    free = numpy.ones(2, dtype=bool)
    D = numpy.diag([1., -1.])
    x, it, broke = bicgstab_reference(D, numpy.array([1., 2.]), numpy.zeros(2), free, None, 1e-24, 2)
    assert not broke and it == 2 and numpy.allclose(x, [1., -2.], rtol=1e-12, atol=0)
    assert bicgstab_reference(D, numpy.array([1., 1.]), numpy.zeros(2), free, None, 1e-24, 2)[1:] == (0, True)  # rhat . v = 0 at the first step
    assert bicgstab_reference(numpy.array([[0., 1.], [1., 0.]]), numpy.array([1., 0.]), numpy.zeros(2), free, None, 1e-24, 2)[1:] == (0, True)


def agreement_case(jacobi):
    '''the system of test_reference_agrees_with_a_direct_solve'''
    N = skewed(laplace2d(9, 7))
    n = N.shape[0]
    rng = numpy.random.default_rng(3)
    N = scipy.sparse.csr_matrix(scipy.sparse.diags(rng.uniform(.5, 2., n)) @ N)
    b = rng.normal(size=n)
    free = rng.uniform(size=n) < .8
    x0 = numpy.where(free, 0., rng.normal(size=n))
    dinv = numpy.where(free, 1 / N.diagonal(), 0.) if jacobi else None
    r0 = numpy.linalg.norm((b - N @ x0)[free])
    return N, b, x0, free, dinv, (1e-11 * r0) ** 2


@pytest.mark.parametrize('jacobi', [True, False])
def test_recurrence_agrees_with_the_reference(jacobi):
    '''one start of the step-by-step restatement, in float64, is the older restatement bit for bit'''
    N, b, x0, free, dinv, stop_rr = agreement_case(jacobi)
    n = len(b)
    x, it, broke = bicgstab_reference(N, b, x0, free, dinv, stop_rr, n)
    assert not broke and 0 < it < n
    for check in (1, 16):
        rec = Recurrence(lambda y: N @ y, free, dinv, x0)
        rec.init(numpy.where(free, b - N @ x0, 0.))
        while rec.ST == 0:
            rec.iterate(check, stop_rr)
        assert rec.ST == ST_DONE and not rec.FLAG and rec.COUNT == it and rec.RR <= stop_rr
        assert numpy.array_equal(rec.x.view(numpy.int64), x.view(numpy.int64))
        for y in (rec.r, rec.rhat, rec.p, rec.v, rec.s, rec.t, rec.phat, rec.shat):
            assert not y[~free].any()
    # the host loop around it: the second start finds the true residual above the bound or not, the first is the one above
    y, its, starts, outcome = bicgstab_solve_reference(N, b, x0, free, dinv, stop_rr, n, check=1)
    assert outcome == 'converged' and its >= it and starts >= 2
    if starts == 2:
        assert its == it and numpy.array_equal(y.view(numpy.int64), x.view(numpy.int64))
    assert numpy.array_equal(y[~free], x0[~free]) and numpy.linalg.norm((b - N @ y)[free]) <= stop_rr ** .5 * (1 + 1e-3)


@pytest.mark.parametrize('jacobi', [True, False])
def test_same_result_for_any_check(jacobi):
    '''the iterations enqueued past convergence do nothing: iterations, starts and the bytes of x do not depend on `check`; nor does a maxiter that is no
    multiple of it'''
    N, b, x0, free, dinv, stop_rr = agreement_case(jacobi)
    n = len(b)
    results = [bicgstab_solve_reference(N, b, x0, free, dinv, stop_rr, n, check=check) for check in (1, 5, 16)]
    x, it, starts, outcome = results[0]
    assert outcome == 'converged' and it > 7
    for y, it_c, starts_c, outcome_c in results[1:]:
        assert (it_c, starts_c, outcome_c) == (it, starts, outcome) and numpy.array_equal(y.view(numpy.int64), x.view(numpy.int64))
    cut = [bicgstab_solve_reference(N, b, x0, free, dinv, stop_rr, 7, check=check) for check in (1, 5, 16)]
    for y, *rest in cut:
        assert rest == [7, 2, 'maxiter'] and numpy.array_equal(y.view(numpy.int64), cut[0][0].view(numpy.int64))


def dyadic(q, bits=16):
    '''a rational with a power of two for a denominator, numerator and denominator within `bits` bits: products of two of them summed over 2^18 terms are
    exact in float64 (2 * 16 + 18 = 50 < 53)'''
    return q.denominator & (q.denominator - 1) == 0 and q.denominator <= 2 ** bits and abs(q.numerator) <= 2 ** bits


@pytest.mark.parametrize('name', list(BREAKDOWNS))
def test_breakdowns_are_exact(name):
    '''The three systems in exact rational arithmetic: each breaks down where its name says, after one iteration that moved x, at the x and r of the table;
    every scalar (alpha, omega, rho' / rho and alpha / omega separately among them) and every entry up to there is dyadic, so float64 computes them exactly.
    Then the float64 restatement on the tiled system: the same x and r byte for byte, the flag up after one moving iteration, r . r = N times that of the
    tile, and iterations enqueued after the breakdown change nothing.'''
    A, b, x_at, r_at = BREAKDOWNS[name]
    kind, moved, x, r, scalars, entries = exact_breakdown(A, b)
    assert (kind, moved) == (name, 1)
    assert x == [fractions.Fraction(xi) for xi in x_at] and r == [fractions.Fraction(ri) for ri in r_at]
    assert all(dyadic(q) for q in scalars) and all(dyadic(q) for q in entries), (scalars, entries)
    rr = sum(ri * ri for ri in r_at)
    assert rr == {'rhat . r': 1, 'rhat . v': 5, 't . s': 2}[name]
    assert numpy.linalg.matrix_rank(numpy.array(A, dtype=float)) == 3
    N = 500
    K, bN, xN, rN = tiled(name, N)
    free = numpy.ones(3 * N, dtype=bool)
    rec = Recurrence(lambda y: K @ y, free, None, numpy.zeros(3 * N))
    rec.init(bN)
    rec.iterate(5, 1e-20)
    state = lambda: [y.copy() for y in (rec.x, rec.r, rec.p)] + [rec.RR, rec.FLAG, rec.COUNT]
    assert (rec.RR, rec.FLAG, rec.COUNT, rec.ST) == (N * rr, True, 1, ST_BAD)
    assert numpy.array_equal(rec.x.view(numpy.int64), xN.view(numpy.int64)) and numpy.array_equal(rec.r.view(numpy.int64), rN.view(numpy.int64))
    before = state()
    rec.iterate(3, 1e-20)
    assert all(numpy.array_equal(a, c) for a, c in zip(before, state()))
    # through the host loop: a restart, and a solution
    x, it, starts, outcome = bicgstab_solve_reference(K, bN, numpy.zeros(3 * N), free, None, (1e-10 * numpy.linalg.norm(bN)) ** 2, 3 * N)
    print(f'{name}: {it} iterations, {starts} starts')
    assert outcome == 'converged' and starts >= 3 and it > 1
    assert numpy.linalg.norm(bN - K @ x) <= 1e-10 * numpy.linalg.norm(bN) * (1 + 1e-3)


def test_solve_reference_on_the_defined_small_cases():
    free = numpy.ones(2, dtype=bool)
    D = numpy.diag([1., -1.])
    x, it, starts, outcome = bicgstab_solve_reference(D, numpy.array([1., 2.]), numpy.zeros(2), free, None, 1e-24, 2)
    assert (it, outcome) == (2, 'converged') and numpy.allclose(x, [1., -2.], rtol=1e-12, atol=0)
    assert bicgstab_solve_reference(D, numpy.array([1., 1.]), numpy.zeros(2), free, None, 1e-24, 2)[1:] == (0, 1, 'breakdown')
    assert bicgstab_solve_reference(numpy.array([[0., 1.], [1., 0.]]), numpy.array([1., 0.]), numpy.zeros(2), free, None, 1e-24, 2)[1:] == (0, 1, 'breakdown')
    assert bicgstab_solve_reference(D, numpy.array([1., numpy.inf]), numpy.zeros(2), free, None, 1e-24, 2)[1:] == (0, 1, 'non-finite')


# ---- C ABI ---------------------------------------------------------------------------------------------------------------

def iterate(A, vectors=None, work=P, stop_rr=1e-20, niter=1):
    return _lib.load().nh_bicgstab_iterate(A, None, None, *([P] * NVEC if vectors is None else vectors), work, stop_rr, niter, None)


def test_abi_refusals():
    lib = _lib.load()
    A = ctypes.byref(csr())
    refused(iterate(None), 'nh_bicgstab_iterate', 'NULL matrix')
    for i in range(NVEC - 2):  # (phat and shat may be NULL without a preconditioner)
        vectors = [P] * NVEC
        vectors[i] = None
        refused(iterate(A, vectors), 'nh_bicgstab_iterate', 'NULL vector')
    refused(iterate(A, work=None), 'nh_bicgstab_iterate', 'NULL vector')
    for i in (NVEC - 2, NVEC - 1):  # ... but not with one
        vectors = [P] * NVEC
        vectors[i] = None
        refused(lib.nh_bicgstab_iterate(A, None, P, *vectors, P, 1e-20, 1, None), 'nh_bicgstab_iterate', 'NULL vector')
    refused(iterate(ctypes.byref(csr(ncols=4))), 'nh_bicgstab_iterate', 'square')
    refused(iterate(A, niter=-1), 'nh_bicgstab_iterate', 'negative iteration count')
    refused(iterate(A, stop_rr=-1e-300), 'nh_bicgstab_iterate', 'negative')
    refused(iterate(A, stop_rr=float('nan')), 'nh_bicgstab_iterate', 'negative')
    for fields, word in ((dict(nrows=-1), 'negative size'), (dict(lanes=3), 'power of two'), (dict(rowptr=None), 'NULL row pointers'), (dict(values=None), 'NULL values')):
        refused(iterate(ctypes.byref(csr(**fields))), 'nh_bicgstab_iterate', word)
        refused(lib.nh_csr_spmv_dots(ctypes.byref(csr(**fields)), P, P, None, P, P, None), 'nh_csr_spmv_dots', word)
    refused(lib.nh_bicgstab_init(-1, None, P, P, P, None, P, None), 'nh_bicgstab_init', 'negative size')
    for i in range(3):  # r, rhat, p
        vectors = [P] * 3
        vectors[i] = None
        refused(lib.nh_bicgstab_init(3, None, *vectors, None, P, None), 'nh_bicgstab_init', 'NULL vector')
    refused(lib.nh_bicgstab_init(3, None, P, P, P, None, None, None), 'nh_bicgstab_init', 'NULL vector')
    refused(lib.nh_bicgstab_init(3, P, P, P, P, None, P, None), 'nh_bicgstab_init', 'NULL vector')  # a preconditioner needs phat
    refused(lib.nh_csr_spmv_dots(None, P, P, None, P, P, None), 'NULL matrix')
    for i in range(4):  # x, w, y, work
        args = [P, P, None, P, P]
        args[i + (i > 1)] = None
        refused(lib.nh_csr_spmv_dots(A, *args, None), 'nh_csr_spmv_dots', 'NULL vector')


def test_empty_matrices_succeed_without_a_launch():
    lib = _lib.load()
    none = ctypes.byref(csr(nrows=0, ncols=0, nnz=0, values=None, rowptr=None, colidx=None))
    assert iterate(none, vectors=[None] * NVEC, niter=4) == 0
    assert lib.nh_bicgstab_work_doubles() >= 3


# ---- solve: errors before any device work --------------------------------------------------------------------------------

def test_solve_errors_come_before_any_device_work():
    A = matrix.HipMatrix(numpy.array([2., -1., -3., 2.]), numpy.array([0, 2, 4]), numpy.array([0, 1, 0, 1]), 2)
    with pytest.raises(matrix.MatrixError, match='tolerance'):
        A.solve(numpy.ones(2), solver='bicgstab')
    with pytest.raises(matrix.MatrixError, match='tolerance'):
        A.solve(numpy.ones(2), solver='bicgstab', atol=0., rtol=0.)
    with pytest.raises(matrix.MatrixError, match='preconditioner'):
        A.solve(numpy.ones(2), solver='bicgstab', rtol=1e-8, precon='ilu')
    with pytest.raises(matrix.MatrixError, match='one vector'):
        A.solve(numpy.ones((2, 2)), solver='bicgstab', rtol=1e-8)
    with pytest.raises(matrix.MatrixError):
        A.solve(numpy.ones(2), solver='bicgstab', rtol=1e-8, constrain=numpy.zeros(3))
    assert A._dev is None and A.iterations is None  # nothing was uploaded
