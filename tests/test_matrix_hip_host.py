'''CPU-side checks of the device-resident matrix backend (matrix.HipMatrix, nh_csr.hip): what the C ABI refuses before it touches the device, the
lanes-per-row rule, the constraint convention, backend selection and the errors a solve raises before any device work.'''
import ctypes
import numpy
import pytest

from nutils_amd import _lib, matrix

INT32_MAX = 2 ** 31 - 1
P = ctypes.c_void_p(64)  # a non-NULL pointer that is never followed: every call below fails its argument checks first


def csr(nrows=3, ncols=3, nnz=5, values=P, rowptr=P, colidx=P, col32=None, lanes=0):
    return _lib.Csr(nrows, ncols, nnz, values, rowptr, colidx, col32, lanes)


def refused(rc, *words):
    msg = _lib.load().nh_last_error()
    assert rc == -1, rc
    for word in words:
        assert word.encode() in msg, msg
    with pytest.raises(_lib.NutilsHipError):
        _lib.check(rc)


BAD_MATRICES = [
    (dict(nrows=-1), 'negative size'),
    (dict(ncols=-1), 'negative size'),
    (dict(nnz=-1), 'negative size'),
    (dict(lanes=3), 'power of two'),
    (dict(lanes=128), 'power of two'),
    (dict(lanes=-2), 'power of two'),
    (dict(rowptr=None), 'NULL row pointers'),
    (dict(values=None), 'NULL values'),
    (dict(colidx=None), 'NULL values or column indices'),
    (dict(col32=P, ncols=INT32_MAX + 1), 'int32 column indices'),
]


@pytest.mark.parametrize('fields,word', BAD_MATRICES, ids=[' '.join(f'{k}={v if not isinstance(v, ctypes.c_void_p) else "ptr"}' for k, v in f.items()) for f, _ in BAD_MATRICES])
def test_bad_matrix_is_refused_by_every_entry_point(fields, word):
    lib = _lib.load()
    A = ctypes.byref(csr(**fields))
    refused(lib.nh_csr_spmv(A, 1., P, 0., None, None, P, None), 'nh_csr_spmv', word)
    refused(lib.nh_csr_diagonal(A, P, None), 'nh_csr_diagonal', word)
    refused(lib.nh_cg_iterate(A, None, None, P, P, P, P, P, 1, None), 'nh_cg_iterate', word)


def test_null_arguments():
    lib = _lib.load()
    A = ctypes.byref(csr())
    refused(lib.nh_csr_spmv(None, 1., P, 0., None, None, P, None), 'NULL matrix')
    refused(lib.nh_csr_spmv(A, 1., None, 0., None, None, P, None), 'NULL argument vector')
    refused(lib.nh_csr_spmv(A, 1., P, 0., None, None, None, None), 'NULL result vector')
    refused(lib.nh_csr_diagonal(None, P, None), 'NULL matrix')
    refused(lib.nh_csr_diagonal(A, None, None), 'NULL result vector')
    refused(lib.nh_csr_compact(5, 3, None, P, None), 'nh_csr_compact', 'NULL')
    refused(lib.nh_csr_compact(5, 3, P, None, None), 'nh_csr_compact', 'NULL')
    refused(lib.nh_csr_compact(-1, 3, P, P, None), 'negative size')
    refused(lib.nh_csr_compact(5, INT32_MAX + 1, P, P, None), 'int32 column indices')
    refused(lib.nh_cg_iterate(None, None, None, P, P, P, P, P, 1, None), 'NULL matrix')
    for i in range(5):  # x, r, p, q, work
        vectors = [P] * 5
        vectors[i] = None
        refused(lib.nh_cg_iterate(A, None, None, *vectors, 1, None), 'nh_cg_iterate', 'NULL vector')
    refused(lib.nh_cg_iterate(A, None, None, P, P, P, P, P, -1, None), 'negative iteration count')
    refused(lib.nh_cg_iterate(ctypes.byref(csr(ncols=4)), None, None, P, P, P, P, P, 1, None), 'square')
    refused(lib.nh_cg_init(-1, None, P, P, P, None), 'negative size')
    refused(lib.nh_cg_init(3, None, None, P, P, None), 'NULL vector')
    refused(lib.nh_cg_init(3, None, P, P, None, None), 'NULL vector')


def test_empty_matrices_succeed_without_a_launch():
    lib = _lib.load()
    none = ctypes.byref(csr(nrows=0, ncols=0, nnz=0, values=None, rowptr=None, colidx=None))
    assert lib.nh_csr_spmv(none, 1., None, 0., None, None, None, None) == 0
    assert lib.nh_csr_diagonal(none, None, None) == 0
    assert lib.nh_cg_iterate(none, None, None, None, None, None, None, P, 4, None) == 0
    assert lib.nh_csr_compact(0, 7, None, None, None) == 0
    assert lib.nh_cg_work_doubles() >= 2


def test_spmv_lanes():
    lib = _lib.load()
    assert matrix.spmv_lanes(0, 0) == matrix.spmv_lanes(0, 5) == matrix.spmv_lanes(7, 0) == 1
    previous = 1
    for per_row in list(range(1, 200)) + [375, 1000, 10 ** 6]:
        for nrows in (1, 7, 1000):
            L = matrix.spmv_lanes(nrows, per_row * nrows)
            assert 1 <= L <= 64 and L & (L - 1) == 0
            assert L == lib.nh_csr_lanes(nrows, per_row * nrows)  # (the rule behind lanes = 0 of the ABI)
            assert L == matrix.spmv_lanes(1, per_row)
        assert L >= previous  # monotone in nnz / nrows
        previous = L
    assert previous == 32
    # the matrices the rule was measured on: 9, 27, 81 entries per row, P2 vector rows
    assert [matrix.spmv_lanes(1, n) for n in (3, 9, 27, 81, 185, 375)] == [2, 4, 16, 32, 32, 32]


def test_constraints_follow_the_reference_convention():
    nan = numpy.nan
    free, lhs = matrix.constraints(4)
    assert free.dtype == bool and free.all() and lhs.dtype == float and not lhs.any()
    # float array: NaN = free, a number = the value the dof is held at (overrides lhs0 there)
    lhs0 = numpy.array([1., 2., 3., 4.])
    free, lhs = matrix.constraints(4, numpy.array([nan, 5., nan, 0.]), lhs0)
    assert free.tolist() == [True, False, True, False]
    assert lhs.tolist() == [1., 5., 3., 0.]
    assert lhs0.tolist() == [1., 2., 3., 4.]  # (the caller's array is not written)
    free, lhs = matrix.constraints(3, numpy.array([nan, 7., nan]))
    assert free.tolist() == [True, False, True] and lhs.tolist() == [0., 7., 0.]
    # bool array: True = held at lhs0 (zero without one)
    free, lhs = matrix.constraints(4, numpy.array([True, False, False, True]), lhs0)
    assert free.tolist() == [False, True, True, False] and lhs.tolist() == [1., 2., 3., 4.]
    free, lhs = matrix.constraints(2, numpy.array([True, False]))
    assert free.tolist() == [False, True] and lhs.tolist() == [0., 0.]
    for bad in (numpy.zeros(3), numpy.zeros((4, 1)), numpy.zeros(5, dtype=bool)):
        with pytest.raises(matrix.MatrixError):
            matrix.constraints(4, bad)
    with pytest.raises(matrix.MatrixError):
        matrix.constraints(4, None, numpy.zeros(3))
    with pytest.raises(matrix.MatrixError):
        matrix.constraints(2, numpy.array(['a', 'b']))


def triplet():
    return numpy.array([2., -1., -1., 2.]), numpy.array([0, 2, 4]), numpy.array([0, 1, 0, 1])


def test_backend_selection():
    before = matrix.backend.current
    with matrix.backend('hip'):
        assert matrix.backend.current is not before
        A = matrix.assemble_csr(*triplet(), 2)
        assert isinstance(A, matrix.HipMatrix) and A.shape == (2, 2) and A.size == 4
        assert isinstance(matrix.reassemble_csr(*triplet(), 2), matrix.HipMatrix)
        with matrix.backend('scipy'):
            assert isinstance(matrix.assemble_csr(*triplet(), 2), matrix.ScipyMatrix)
        assert isinstance(matrix.assemble_csr(*triplet(), 2), matrix.HipMatrix)
    assert matrix.backend.current is before
    with pytest.raises(RuntimeError):
        with matrix.backend('HIP'):
            raise RuntimeError
    assert matrix.backend.current is before
    with pytest.raises(ValueError):
        with matrix.backend('mkl'):
            pass
    assert isinstance(matrix.assemble_csr(*triplet(), 2), matrix.ScipyMatrix)


def test_host_triplets_are_validated_and_exported_without_a_device():
    values, rowptr, colidx = triplet()
    A = matrix.HipMatrix(values, rowptr, colidx, 2)
    data, indices, indptr = A.export('csr')
    assert numpy.array_equal(data, values) and numpy.array_equal(indices, colidx) and numpy.array_equal(indptr, rowptr)
    assert numpy.array_equal(A.export('dense'), [[2., -1.], [-1., 2.]])
    data, (row, col) = A.export('coo')
    assert row.tolist() == [0, 0, 1, 1] and col.tolist() == [0, 1, 0, 1]
    with pytest.raises(NotImplementedError):
        A.export('ell')
    with pytest.raises(matrix.MatrixError):
        matrix.HipMatrix(values, rowptr, numpy.array([0, 1, 0, 2]), 2)


def test_tolerance_not_reached():
    best = numpy.arange(3.)
    e = matrix.ToleranceNotReached(best)
    assert isinstance(e, matrix.MatrixError) and e.best is best
    assert 'tolerance' in str(e)


def test_solve_errors_come_before_any_device_work():
    A = matrix.HipMatrix(*triplet(), 2)
    with pytest.raises(matrix.MatrixError, match='tolerance'):
        A.solve(numpy.ones(2))
    with pytest.raises(matrix.MatrixError, match='tolerance'):
        A.solve(numpy.ones(2), solver='cg', atol=0., rtol=0.)
    with pytest.raises(matrix.MatrixError, match='one vector'):
        A.solve(numpy.ones((2, 2)), rtol=1e-8)
    with pytest.raises(matrix.MatrixError, match='shape'):
        A.solve(numpy.ones(3), rtol=1e-8)
    with pytest.raises(matrix.MatrixError, match='preconditioner'):
        A.solve(numpy.ones(2), rtol=1e-8, precon='ilu')
    with pytest.raises(matrix.MatrixError):
        A.solve(numpy.ones(2), rtol=1e-8, constrain=numpy.zeros(3))
    with pytest.raises(matrix.MatrixError, match='square'):
        matrix.HipMatrix(numpy.ones(2), numpy.array([0, 1, 2]), numpy.array([0, 2]), 3).solve(numpy.ones(2), rtol=1e-8)
    with pytest.raises(matrix.MatrixError):
        A @ numpy.ones(3)
    assert A._dev is None  # nothing was uploaded


def test_as_matrix_wraps_integrals_only():
    from nutils_amd import function
    with pytest.raises(TypeError):
        function.as_matrix(numpy.eye(2))
