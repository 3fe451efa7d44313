'''CPU-side checks of the device BiCGStab solve (matrix.HipMatrix.solve(solver='bicgstab'), nh_csr.hip): what the C ABI refuses before it touches the
device, the errors a solve raises before any device work, and a numpy restatement of the algorithm the kernels implement, checked against a direct solve.
The restatement (`bicgstab_reference`) is the CPU reference of tests/test_gpu_bicgstab.py.'''
import ctypes
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
