'''CPU-side checks of the block interface of the device matrix backend (matrix.HipMatrix.matmat / solve_columns, nh_csr_multi.hip): every argument error is a
MatrixError raised before any device work, the C entry points refuse bad arguments with a message before a launch, and empty matrices succeed without one.'''
import ctypes
import numpy
import pytest

from nutils_amd import _lib, matrix

P = ctypes.c_void_p(64)  # a non-NULL pointer that is never followed: every call below fails its argument checks first


def small(ncols=2):
    '''diag(2, 3), or with a third, empty column; from host arrays: `_dev` stays None until something runs on the device'''
    return matrix.HipMatrix(numpy.array([2., 3.]), numpy.array([0, 1, 2]), numpy.array([0, 1]), ncols)


def csr(nrows=3, ncols=3, nnz=5, values=P, rowptr=P, colidx=P, col32=None, lanes=0):
    return _lib.Csr(nrows, ncols, nnz, values, rowptr, colidx, col32, lanes)


def refused(rc, *words, status=-1):
    msg = _lib.load().nh_last_error()
    assert rc == status, rc
    for word in words:
        assert word.encode() in msg, msg


SOLVE_ERRORS = [
    ('no rhs', dict(rhs=None), 'is missing'),
    ('1-D rhs', dict(rhs=numpy.ones(2)), 'block of columns'),
    ('3-D rhs', dict(rhs=numpy.ones((2, 2, 2))), 'block of columns'),
    ('no columns', dict(rhs=numpy.ones((2, 0))), 'block of columns'),
    ('wrong row count', dict(rhs=numpy.ones((3, 2))), 'does not match matrix shape'),
    ('lhs0 of a wrong length', dict(lhs0=numpy.ones(3)), 'initial block has shape'),
    ('lhs0 of a wrong width', dict(lhs0=numpy.ones((2, 3))), 'initial block has shape'),
    ('lhs0 transposed', dict(lhs0=numpy.ones((4, 2)), rhs=numpy.ones((2, 4))), 'initial block has shape'),
    ('constrain of shape (n, k)', dict(constrain=numpy.full((2, 2), numpy.nan)), 'constraints have shape'),
    ('bicgstab', dict(solver='bicgstab'), "offers solver='cg'"),
    ('minres', dict(solver='minres'), 'one right-hand side at a time'),
    ('fgmres', dict(solver='fgmres'), "'fgmres'"),
    ('direct', dict(solver='direct'), "offers solver='cg'"),
    ('amg', dict(precon='amg'), "'amg' takes one right-hand side at a time"),
    ('unknown preconditioner', dict(precon='spilu'), "precon='diag' or None"),
    ('preconargs', dict(preconargs=dict(coarse=4)), 'preconargs'),
    ('no tolerance', dict(rtol=0.), 'tolerance'),
]


@pytest.mark.parametrize('kwargs,word', [c[1:] for c in SOLVE_ERRORS], ids=[c[0] for c in SOLVE_ERRORS])
def test_solve_columns_errors_come_before_any_device_work(kwargs, word):
    A = small()
    args = dict(rhs=numpy.ones((2, 2)), rtol=1e-8)
    args.update(kwargs)
    with pytest.raises(matrix.MatrixError, match=word):
        A.solve_columns(args.pop('rhs'), **args)
    assert A._dev is None


def test_solve_columns_needs_a_square_matrix():
    A = small(ncols=3)
    with pytest.raises(matrix.MatrixError, match='not square'):
        A.solve_columns(numpy.ones((2, 2)), rtol=1e-8)
    assert A._dev is None


@pytest.mark.parametrize('X', [numpy.ones(3), numpy.ones((2, 2)), numpy.ones((3, 0)), numpy.ones((3, 2, 2)), None], ids=['1-D', 'wrong row count', 'no columns', '3-D', 'None'])
def test_matmat_errors_come_before_any_device_work(X):
    A = small(ncols=3)
    with pytest.raises(matrix.MatrixError):
        A.matmat(X)
    assert A._dev is None


def test_the_single_vector_interface_still_refuses_blocks():
    A = small()
    with pytest.raises(matrix.MatrixError, match='one vector'):
        A.solve(numpy.ones((2, 2)), rtol=1e-8)
    with pytest.raises(matrix.MatrixError):
        A @ numpy.ones((2, 2))
    assert A._dev is None and A.column_iterations is None


def test_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    A = ctypes.byref(csr())
    spmm = lambda A=A, k=2, x=P, ldx=2, b=None, ldb=0, y=P, ldy=2: lib.nh_csr_spmm(A, k, 1., x, ldx, 0., b, ldb, None, y, ldy, None)
    refused(spmm(A=None), 'nh_csr_spmm', 'NULL matrix')
    refused(spmm(A=ctypes.byref(csr(lanes=3))), 'nh_csr_spmm', 'power of two')
    refused(spmm(k=0), 'nh_csr_spmm', 'at least one column')
    refused(spmm(ldx=1), 'nh_csr_spmm', 'leading dimension')
    refused(spmm(ldy=1), 'nh_csr_spmm', 'leading dimension')
    refused(spmm(b=P, ldb=1), 'nh_csr_spmm', 'leading dimension')
    refused(spmm(x=None), 'nh_csr_spmm', 'NULL argument block')
    refused(spmm(y=None), 'nh_csr_spmm', 'NULL result block')
    iterate = lambda A=A, k=2, vectors=(P,) * 5, niter=1: lib.nh_cgm_iterate(A, k, None, None, *vectors, niter, None)
    refused(iterate(A=None), 'nh_cgm_iterate', 'NULL matrix')
    refused(iterate(k=0), 'nh_cgm_iterate', 'at least one column')
    refused(iterate(k=9), 'nh_cgm_iterate', 'at most 8 columns', status=-3)
    refused(iterate(A=ctypes.byref(csr(ncols=4))), 'nh_cgm_iterate', 'square')
    refused(iterate(niter=-1), 'nh_cgm_iterate', 'negative iteration count')
    for i in range(5):  # x, r, p, q, work
        vectors = [P] * 5
        vectors[i] = None
        refused(iterate(vectors=vectors), 'nh_cgm_iterate', 'NULL vector')
    refused(lib.nh_cgm_init(-1, 2, None, P, P, P, None), 'nh_cgm_init', 'negative size')
    refused(lib.nh_cgm_init(3, 0, None, P, P, P, None), 'nh_cgm_init', 'at least one column')
    refused(lib.nh_cgm_init(3, 9, None, P, P, P, None), 'nh_cgm_init', 'at most 8 columns', status=-3)
    refused(lib.nh_cgm_init(3, 2, None, None, P, P, None), 'nh_cgm_init', 'NULL vector')
    refused(lib.nh_cgm_init(3, 2, None, P, P, None, None), 'nh_cgm_init', 'NULL vector')
    assert lib.nh_cgm_work_doubles(0) == -1 and lib.nh_cgm_work_doubles(9) == -1
    assert all(lib.nh_cgm_work_doubles(k) >= 4 * k for k in range(1, 9))


def test_empty_matrices_succeed_without_a_launch():
    lib = _lib.load()
    none = ctypes.byref(csr(nrows=0, ncols=0, nnz=0, values=None, rowptr=None, colidx=None))
    assert lib.nh_csr_spmm(none, 3, 1., None, 3, 0., None, 0, None, None, 3, None) == 0
    assert lib.nh_cgm_iterate(none, 3, None, None, None, None, None, None, P, 4, None) == 0
