'''CPU-side checks of the device GMRES solve (matrix.HipMatrix.solve(solver='fgmres'), nh_csr.hip): a numpy restatement of what the kernels do, cell by cell
and in their order of operations (`Cycle`), with the host loop of HipMatrix._fgmres around it (`gmres_reference`); the restatement pinned to the definition of
GMRES -- its residual estimate after j steps is the minimum of |r0 - A M^-1 K_j y| over the Krylov space, found by numpy.linalg.lstsq -- and to its two other
promises, estimates that never rise within a cycle and convergence within as many steps as there are free dofs; what the C ABI refuses before it touches the
device; the errors a solve raises before any device work.  `gmres_reference` is the CPU reference of tests/test_gpu_gmres.py.'''
import ctypes
import numpy
import pytest
import scipy.sparse
import scipy.sparse.linalg

from nutils_amd import _lib, matrix
from test_bicgstab_host import refused, csr, skewed, laplace2d, agreement_case, P

U = 2. ** -53
ST_DONE, ST_BAD, ST_FULL = 1., 2., 3.  # a status; 0 is "iterate"
VANISH = 2. ** -40  # GS_VANISH of nh_csr.hip
CELLS = dict(RR=0, FLAG=1, COUNT=2, ST=3, HN=4)  # the head of the work array (the enum of nh_csr.hip); the first three are what kernels.gmres_work documents
HEAD = 8


def cells(m):
    '''where the arrays of the work array start (gmres_cells of nh_csr.hip): h1, h2, cs, sn, g, y of m + 1 doubles each, then r, column j at r + j (m + 1)'''
    names = 'h1', 'h2', 'cs', 'sn', 'g', 'y', 'r'
    return {name: HEAD + i * (m + 1) for i, name in enumerate(names)}


# ---- the algorithm, restated ---------------------------------------------------------------------------------------------

class Cycle:
    '''What lives on the device between nh_gmres_init and nh_gmres_update: the basis V (restart + 1 vectors), z, w, and the cells RR, FLAG, COUNT, ST, HN, the
    arrays H1, H2, CS, SN, G, Y and the columns of R, each written by the step that writes it in nh_csr.hip (k_gmres_norm, k_gmres_init_scalars and
    k_gmres_normalize: `init`; the product, twice k_gmres_dots / k_gmres_dots_sum / k_gmres_axpy, k_gmres_scalars, k_gmres_normalize: `step`; k_gmres_solve
    and k_gmres_xupdate: `update`).  A step that finds a status does nothing.  All vectors vanish on the rows `free` masks.  `product` is y = A x on the
    arithmetic of the vectors (float64, or longdouble for a reference of the device's arithmetic).  `passes`: Gram-Schmidt passes (the device makes two).
    `estimates` collects RR after every step that took a column.'''

    def __init__(self, product, free, dinv, x, restart, passes=2):
        self.product, self.free, self.dinv, self.m, self.passes = product, free, dinv, int(restart), passes
        self.x = x.copy()
        self.cycles = 0
        self.estimates = []

    def M(self, y):
        return y if self.dinv is None else self.dinv * y

    def A(self, y):
        return numpy.where(self.free, self.product(y), 0)

    def init(self, r):
        m, t = self.m, r.dtype.type
        self.V = numpy.zeros((m + 1, len(r)), dtype=r.dtype)
        self.H1, self.H2, self.CS, self.SN, self.G, self.Y = (numpy.zeros(m + 1, dtype=r.dtype) for _ in range(6))
        self.R = numpy.zeros((m, m + 1), dtype=r.dtype)  # R[j]: column j
        self.z, self.w = numpy.zeros_like(r), numpy.zeros_like(r)  # (the device leaves them as they are until a step writes them)
        rr = r @ r
        bad = not numpy.isfinite(rr)
        self.RR, self.FLAG, self.COUNT = rr, bad, 0
        self.ST = ST_BAD if bad else ST_DONE if rr == 0 else 0.
        self.HN = self.G[0] = numpy.sqrt(rr)
        self.zero = t(0)
        self.normalize(r)
        self.cycles += 1
        self.estimates.append([])

    def normalize(self, src):
        if self.ST != 0:
            return
        v = src / self.HN
        self.V[self.COUNT] = v
        self.z = self.M(v)

    def step(self, stop_rr):
        if self.ST != 0:
            return
        j, m = self.COUNT, self.m
        w = self.A(self.z)
        for h in (self.H1, self.H2)[:self.passes]:
            h[:j + 1] = self.V[:j + 1] @ w
            for k in range(j + 1):
                w = w - h[k] * self.V[k]
        self.w, ww = w, w @ w
        # k_gmres_scalars
        R, CS, SN, G = self.R[j], self.CS, self.SN, self.G
        p = self.H1[0] + self.H2[0]
        col2 = p * p
        for k in range(j):
            q = self.H1[k + 1] + self.H2[k + 1]
            col2 = col2 + q * q
            R[k] = CS[k] * p + SN[k] * q
            p = CS[k] * q - SN[k] * p
        col2 = col2 + ww
        vanish = not ww > (VANISH * VANISH) * col2
        st, flag, count = ST_BAD, True, j
        if numpy.isfinite(col2) and not (vanish and not abs(p) > VANISH * numpy.sqrt(col2)):
            q = self.zero if vanish else numpy.sqrt(ww)
            d = max(numpy.hypot(p, q), abs(p), q)
            cj, sj, gj = p / d, q / d, G[j]
            gn = -sj * gj
            rr = gn * gn
            if numpy.isfinite(rr):
                R[j], CS[j], SN[j], G[j], G[j + 1] = d, cj, sj, cj * gj, gn
                self.RR, self.HN = rr, q
                count, flag = j + 1, vanish
                st = ST_DONE if vanish or rr <= stop_rr else ST_FULL if j + 1 >= m else 0.
                self.estimates[-1].append(rr)
        self.FLAG, self.COUNT, self.ST = flag, count, st
        self.normalize(w)

    def iterate(self, niter, stop_rr):
        for _ in range(niter):
            self.step(stop_rr)

    def update(self):
        count = self.COUNT
        y = self.Y
        y[:count] = self.G[:count]
        for k in range(count - 1, -1, -1):
            y[k] = y[k] / self.R[k][k]
            y[:k] -= self.R[k][:k] * y[k]
        s = numpy.zeros_like(self.x)
        for k in range(count):
            s = s + y[k] * self.V[k]
        self.x = self.x + self.M(s)


def gmres_reference(A, b, x, free, dinv, stop_rr, restart, maxiter, check=16, passes=2, full=False):
    '''The host loop of HipMatrix._fgmres around a `Cycle`: a cycle from the true residual mask(b - A x), up to `check` steps between two looks at the
    estimate, the flag and the count, the update, the next cycle.  Returns (x, Arnoldi steps, outcome), outcome 'converged', 'maxiter', 'singular' or
    'non-finite'; with `full` also the Cycle.'''
    mask = lambda y: numpy.where(free, y, 0.)
    m = max(1, min(int(restart), int(free.sum())))
    cyc = Cycle(lambda y: A @ y, free, dinv, numpy.array(x, dtype=float), m, passes)
    it, since, rr_start, outcome = 0, None, None, None  # since: cycles finished since one ended on a vanished direction
    while outcome is None:
        cyc.init(mask(b - A @ cyc.x))
        rr = cyc.RR
        if not numpy.isfinite(rr):
            outcome = 'non-finite'
        elif rr <= stop_rr:
            outcome = 'converged'
        elif since in (0, 1) and not rr < rr_start:  # (that cycle or the one after it: see HipMatrix._fgmres)
            outcome = 'singular'
        elif it >= maxiter:
            outcome = 'maxiter'
        else:
            start, rr_start = it, rr
            while it < maxiter:
                cyc.iterate(min(check, maxiter - it), stop_rr)
                it = start + cyc.COUNT
                if cyc.FLAG or cyc.RR <= stop_rr or cyc.COUNT >= m:
                    break
            since = 0 if cyc.FLAG else None if since is None else since + 1
            cyc.update()
    return (cyc.x, it, outcome) + ((cyc,) if full else ())


# ---- the restatement is GMRES ----------------------------------------------------------------------------------------------

def dense_case(n, seed, jacobi, constrained):
    rng = numpy.random.default_rng(seed)
    A = 3 * numpy.eye(n) + rng.normal(size=(n, n)) / numpy.sqrt(n)  # nonsymmetric, well conditioned
    A = numpy.diag(rng.uniform(.5, 2., n)) @ A  # (a diagonal that Jacobi has something to do with)
    b = rng.normal(size=n)
    free = rng.uniform(size=n) < .75 if constrained else numpy.ones(n, dtype=bool)
    free[:2] = True
    x0 = numpy.where(free, 0., rng.normal(size=n))
    dinv = numpy.where(free, 1 / numpy.diag(A), 0.) if jacobi else None
    return A, b, free, x0, dinv


@pytest.mark.parametrize('jacobi', [True, False], ids=['jacobi', 'plain'])
@pytest.mark.parametrize('constrained', [True, False], ids=['constrained', 'free'])
@pytest.mark.parametrize('n', [5, 9, 12])
def test_estimate_is_the_least_squares_minimum(n, constrained, jacobi):
    '''After j steps of a cycle sqrt(RR) = min_y |r0 - B y|, B = A M^-1 K_j on the free rows, K_j = [r0, (A M^-1) r0, ..] with columns scaled to unit length
    (the same space).

    The tolerance.  lstsq is backward stable: its y^ minimises |(r0 + dr) - (B + dB) y| with |dB| <= e |B|, |dr| <= e |r0|, e a modest multiple of u.  The
    minimum of the perturbed problem is at most |r0 - B y*| + |dB| |y*| + |dr| for the true minimiser y*, and the other way round with y^, so the two
    minima differ by at most e (|B| max(|y*|, |y^|) + |r0|) <= e |r0| (1 + cond(B)), as |y| <= |r0| / sigma_min(B).  The columns of K_j, made by j rounded
    products and scalings, are within (n + 2) u per product of those of an exact Krylov sequence from nearby data: another dB of that form with e = j (n + 2) u.
    Forming the residual r0 - B y^ costs gamma_(j + 1) (|r0| + |B| |y^|), the same expression again.  The restatement's own estimate is that of a backward
    stable GMRES (two-pass Gram-Schmidt, Givens rotations): exact for a matrix within c j n u |A M^-1| of the given one, which moves the minimum by at most
    that times |y*|, y* now in the orthonormal basis, |y*| <= |r0| / sigma_min(A M^-1 V_j), and cond(A M^-1 V_j) <= cond(B).  Together: with e = 8 j (n + 2) u for the sum
    of the four, tol = e |r0| (1 + cond(B)).  cond(B) is computed and up to j = 4 the tolerance stays below 1e-8 |r0|, far
    below the minimum there; the condition of the power basis grows with every column and the tolerance with it, while the differences printed stay of the order
    of u |r0|.'''
    A, b, free, x0, dinv = dense_case(n, 20 + n, jacobi, constrained)
    nfree = int(free.sum())
    r0 = numpy.where(free, b - A @ x0, 0.)
    op = lambda y: numpy.where(free, A @ (y if dinv is None else dinv * y), 0.)
    cyc = Cycle(lambda y: A @ y, free, dinv, x0, nfree)
    cyc.init(r0)
    K = []
    k = r0 / numpy.linalg.norm(r0)
    for j in range(1, nfree + 1):
        K.append(k)
        cyc.step(0.)
        assert cyc.COUNT == j and cyc.FLAG == (j == nfree)  # (the last direction a space of nfree dimensions has room for vanishes: the lucky breakdown)
        B = numpy.array([op(c) for c in K]).T
        y = numpy.linalg.lstsq(B, r0, rcond=None)[0]
        minimum = numpy.linalg.norm(r0 - B @ y)
        cond = numpy.linalg.cond(B)
        tol = 8 * j * (n + 2) * U * numpy.linalg.norm(r0) * (1 + cond)
        print(f'n={n} j={j}: estimate {numpy.sqrt(cyc.RR):.6e}, minimum {minimum:.6e}, difference {abs(numpy.sqrt(cyc.RR) - minimum):.1e}, tolerance {tol:.1e}, cond {cond:.1e}')
        assert j > 4 or tol <= 1e-8 * numpy.linalg.norm(r0)
        assert abs(numpy.sqrt(cyc.RR) - minimum) <= tol
        k = op(k)
        k = k / numpy.linalg.norm(k)
    assert cyc.ST == ST_DONE and cyc.RR == 0
    # ... and the update makes that minimum the true residual, to the same tolerance
    cyc.update()
    assert numpy.array_equal(cyc.x[~free], x0[~free])
    assert numpy.linalg.norm(numpy.where(free, b - A @ cyc.x, 0.)) <= tol


@pytest.mark.parametrize('jacobi', [True, False], ids=['jacobi', 'plain'])
@pytest.mark.parametrize('restart', [3, 5, 30, 1000])
def test_reference_agrees_with_a_direct_solve(restart, jacobi):
    '''the contract of a solve, the estimates never rising within a cycle, and full GMRES within as many steps as there are free dofs'''
    N, b, x0, free, dinv, stop_rr = agreement_case(jacobi)
    n, nfree = len(b), int(free.sum())
    x, it, outcome, cyc = gmres_reference(N, b, x0, free, dinv, stop_rr, restart, 20 * n, full=True)
    print(f'restart={restart}: {it} steps in {cyc.cycles} cycles')
    assert outcome == 'converged' and it > 0
    assert numpy.array_equal(x[~free], x0[~free])
    res = numpy.linalg.norm((b - N @ x)[free])
    assert res <= stop_rr ** .5  # (the true residual, not the estimate: that is what ends the solve)
    direct = x0.copy()
    direct[free] += scipy.sparse.linalg.spsolve(N[free][:, free].tocsc(), (b - N @ x0)[free])
    smin = numpy.linalg.svd(N.toarray()[free][:, free], compute_uv=False)[-1]
    assert numpy.linalg.norm(x - direct) <= res / smin * (1 + 1e-6)
    for estimates in cyc.estimates:
        assert len(estimates) <= min(restart, nfree)
        assert all(b <= a for a, b in zip(estimates, estimates[1:]))  # never rises: |sn| <= 1 by construction, and rounding is monotone
    if restart >= nfree:
        assert it <= nfree
        assert cyc.cycles <= 3  # the cycle, and one that finds the true residual within the bound or a rounding above it
    for y in (cyc.z, cyc.w, *cyc.V):
        assert not y[~free].any()


@pytest.mark.parametrize('jacobi', [True, False], ids=['jacobi', 'plain'])
def test_same_result_for_any_check(jacobi):
    '''the steps enqueued after the stop and after the last column of a cycle do nothing: steps, cycles and the bytes of x do not depend on `check`; nor with
    a maxiter that is no multiple of it or of restart'''
    N, b, x0, free, dinv, stop_rr = agreement_case(jacobi)
    n = len(b)
    for restart, maxiter, expect in ((5, 20 * n, 'converged'), (30, 20 * n, 'converged'), (5, 13, 'maxiter')):
        results = [gmres_reference(N, b, x0, free, dinv, stop_rr, restart, maxiter, check=check, full=True) for check in (1, 5, 16)]
        x, it, outcome, cyc = results[0]
        assert outcome == expect and (it == 13 if expect == 'maxiter' else it > 16)
        for y, it_c, outcome_c, cyc_c in results[1:]:
            assert (it_c, outcome_c, cyc_c.cycles) == (it, outcome, cyc.cycles) and numpy.array_equal(y.view(numpy.int64), x.view(numpy.int64))


def test_one_pass_loses_orthogonality():
    '''why the device makes two passes: on a 1480-row matrix of the kind the GPU tests use, an unrestarted cycle to a residual of 1e-10 |r0| leaves V^T V - I at
    7e-6 with one pass of classical Gram-Schmidt (the loss grows as the residual falls) and at a few u with two'''
    N = skewed(laplace2d(40, 37))
    n = N.shape[0]
    b = numpy.random.default_rng(1).normal(size=n)
    free = numpy.ones(n, dtype=bool)
    dinv = 1 / N.diagonal()
    worst = {}
    for passes in (1, 2):
        cyc = Cycle(lambda y: N @ y, free, dinv, numpy.zeros(n), 300, passes)
        cyc.init(b)
        cyc.iterate(300, 1e-20 * (b @ b))
        count = cyc.COUNT
        assert cyc.ST == ST_DONE and 50 < count < 150
        worst[passes] = numpy.abs(cyc.V[:count] @ cyc.V[:count].T - numpy.eye(count)).max()
    print(worst)
    assert worst[2] <= 1e-13 < 1e-9 < worst[1]


def test_reference_on_the_defined_small_cases():
    free = numpy.ones(2, dtype=bool)
    zero = numpy.zeros(2)
    # the identity: the first direction is all there is, the lucky breakdown
    x, it, outcome = gmres_reference(numpy.eye(2), numpy.array([3., -4.]), zero, free, None, 1e-24, 30, 2)
    assert (it, outcome) == (1, 'converged') and numpy.allclose(x, [3., -4.], rtol=1e-15, atol=0)
    # diag(1, 0) with (1, 1): the first cycle removes what can be removed, the second finds nothing
    x, it, outcome = gmres_reference(numpy.diag([1., 0.]), numpy.array([1., 1.]), zero, free, None, 1e-24, 30, 2)
    assert outcome == 'singular' and it in (1, 2) and x[0] == 1  # (a rounding in x_0 leaves the second cycle a direction of that size: a step, and no progress)
    assert gmres_reference(numpy.zeros((2, 2)), numpy.array([1., 1.]), zero, free, None, 1e-24, 30, 2)[1:] == (0, 'singular')
    assert gmres_reference(numpy.eye(2), numpy.array([1., numpy.inf]), zero, free, None, 1e-24, 30, 2)[1:] == (0, 'non-finite')
    D = numpy.diag([1., -1.])  # indefinite: two steps
    x, it, outcome = gmres_reference(D, numpy.array([1., 2.]), zero, free, None, 1e-24, 30, 2)
    assert (it, outcome) == (2, 'converged') and numpy.allclose(x, [1., -2.], rtol=1e-14, atol=0)
    # nothing free: the start vector comes back without a step
    x, it, outcome = gmres_reference(D, numpy.array([1., 2.]), numpy.array([5., 6.]), ~free, None, 0., 30, 0)
    assert (it, outcome) == (0, 'converged') and numpy.array_equal(x, [5., 6.])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------

def iterate(A, vectors=(P, P, P), work=P, restart=30, stop_rr=1e-20, niter=1):
    return _lib.load().nh_gmres_iterate(A, None, None, *vectors, work, restart, stop_rr, niter, None)


def test_abi_refusals():
    lib = _lib.load()
    A = ctypes.byref(csr())
    refused(iterate(None), 'nh_gmres_iterate', 'NULL matrix')
    for i in range(3):  # V, z, w
        vectors = [P] * 3
        vectors[i] = None
        refused(iterate(A, vectors), 'nh_gmres_iterate', 'NULL vector')
    refused(iterate(A, work=None), 'nh_gmres_iterate', 'NULL vector')
    refused(iterate(ctypes.byref(csr(ncols=4))), 'nh_gmres_iterate', 'square')
    refused(iterate(A, niter=-1), 'nh_gmres_iterate', 'negative iteration count')
    refused(iterate(A, restart=0), 'nh_gmres_iterate', 'restart')
    refused(iterate(A, restart=-3), 'nh_gmres_iterate', 'restart')
    refused(iterate(A, stop_rr=-1e-300), 'nh_gmres_iterate', 'negative')
    refused(iterate(A, stop_rr=float('nan')), 'nh_gmres_iterate', 'negative')
    for fields, word in ((dict(nrows=-1), 'negative size'), (dict(lanes=3), 'power of two'), (dict(rowptr=None), 'NULL row pointers'), (dict(values=None), 'NULL values')):
        refused(iterate(ctypes.byref(csr(**fields))), 'nh_gmres_iterate', word)
    refused(lib.nh_gmres_init(-1, 30, None, P, P, P, P, None), 'nh_gmres_init', 'negative size')
    refused(lib.nh_gmres_init(3, 0, None, P, P, P, P, None), 'nh_gmres_init', 'restart')
    for i in range(4):  # r, V, z, work
        args = [P] * 4
        args[i] = None
        refused(lib.nh_gmres_init(3, 30, None, *args, None), 'nh_gmres_init', 'NULL vector')
    refused(lib.nh_gmres_update(-1, 30, None, P, P, P, None), 'nh_gmres_update', 'negative size')
    refused(lib.nh_gmres_update(3, 0, None, P, P, P, None), 'nh_gmres_update', 'restart')
    for i in range(3):  # V, x, work
        args = [P] * 3
        args[i] = None
        refused(lib.nh_gmres_update(3, 30, None, *args, None), 'nh_gmres_update', 'NULL vector')
    assert lib.nh_gmres_work_doubles(0) == -1 and b'restart' in lib.nh_last_error()
    assert lib.nh_gmres_work_doubles(-1) == -1


def test_work_array_and_empty_matrices():
    lib = _lib.load()
    none = ctypes.byref(csr(nrows=0, ncols=0, nnz=0, values=None, rowptr=None, colidx=None))
    assert iterate(none, vectors=[None] * 3, niter=4) == 0
    assert lib.nh_gmres_update(0, 30, None, None, None, P, None) == 0
    for m in (1, 5, 30, 150):
        size = lib.nh_gmres_work_doubles(m)
        c = cells(m)
        assert size >= c['r'] + m * (m + 1) + (m + 1) * 1024  # the cells of `cells`, the partials of w . w and of m dots
    assert lib.nh_gmres_work_doubles(50000) > 50000 * 50001  # (no 32-bit arithmetic on the way)


# ---- solve: errors before any device work --------------------------------------------------------------------------------

def test_solve_errors_come_before_any_device_work():
    A = matrix.HipMatrix(numpy.array([2., -1., -3., 2.]), numpy.array([0, 2, 4]), numpy.array([0, 1, 0, 1]), 2)
    with pytest.raises(matrix.MatrixError, match='tolerance'):
        A.solve(numpy.ones(2), solver='fgmres')
    with pytest.raises(matrix.MatrixError, match='tolerance'):
        A.solve(numpy.ones(2), solver='fgmres', atol=0., rtol=0.)
    with pytest.raises(matrix.MatrixError, match='preconditioner'):
        A.solve(numpy.ones(2), solver='fgmres', rtol=1e-8, precon='ilu')
    with pytest.raises(matrix.MatrixError, match='one vector'):
        A.solve(numpy.ones((2, 2)), solver='fgmres', rtol=1e-8)
    with pytest.raises(matrix.MatrixError, match='does not match'):
        A.solve(numpy.ones(3), solver='fgmres', rtol=1e-8)
    with pytest.raises(matrix.MatrixError):
        A.solve(numpy.ones(2), solver='fgmres', rtol=1e-8, constrain=numpy.zeros(3))
    for restart in (0, -1, 2.5, 30., None, 'many', True):
        with pytest.raises(matrix.MatrixError, match='restart'):
            A.solve(numpy.ones(2), solver='fgmres', rtol=1e-8, restart=restart)
    B = matrix.HipMatrix(numpy.array([2., -1., -3.]), numpy.array([0, 2, 3]), numpy.array([0, 1, 0]), 3)
    with pytest.raises(matrix.MatrixError, match='not square'):
        B.solve(numpy.ones(2), solver='fgmres', rtol=1e-8)
    assert A._dev is None and A.iterations is None and B._dev is None  # nothing was uploaded
