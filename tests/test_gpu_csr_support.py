'''The support of a device-resident matrix (nh_csr_support, kernels.csr_support, HipMatrix.rowsupp / colsupp) on the GPU against numpy's `abs(data) > tol`
scattered by row and by column: matrices with empty rows, without entries, rectangular, with rows longer than any lane count and with more rows than the grid
covers in one pass; int32 and int64 column indices; every lanes-per-row instantiation; tolerances that make the comparison's strictness and the empty support
visible; either result left out; repeated calls.'''
import functools
import numpy
import pytest

from test_gpu_matrix_hip import case
from test_gpu_cg import tridiagonal

pytestmark = pytest.mark.gpu

NAMES = ('holes', 'empty', 'rectangular', 'p2vector', 'tridiagonal')
LANES = (0, 1, 2, 4, 8, 16, 32, 64)


@functools.lru_cache(maxsize=None)
def triplet(name):
    '''(device triplet, ncols, host values, rowptr, colidx): uploaded or assembled once per session, never written'''
    from nutils_amd import device
    if name == 'tridiagonal':
        K = tridiagonal()[0]
        K.sort_indices()
        v, rp, ci, ncols = K.data, K.indptr.astype(numpy.int64), K.indices.astype(numpy.int64), K.shape[1]
        assert len(rp) - 1 == 262444  # more rows than 2048 workgroups of 64 take in one pass at 4 lanes or more: the grid strides
        dev = device.to_dev(v, 'float64'), device.to_dev(rp, 'int64'), device.to_dev(ci, 'int64')
    else:
        dev, ncols, ref, _ = case(name)
        v, rp, ci = ref.data, ref.indptr, ref.indices
    return dev, ncols, numpy.asarray(v), numpy.asarray(rp), numpy.asarray(ci)


def tolerances(v):
    '''ascending, so that a result array the allocator hands out again holds a LARGER support than the one expected: a missing zero-fill shows.
    0; the median |a|; a value that occurs in the matrix (the comparison is strict: its own entries fall out); max |a| (nothing is left)'''
    if not len(v):
        return [0., 1.]
    a = numpy.sort(abs(v))
    return sorted({0., float(numpy.median(a)), float(a[(3 * len(a)) // 4]), float(a[-1])})


def expected(v, rp, ci, ncols, tol):
    keep = abs(v) > tol
    rows = numpy.repeat(numpy.arange(len(rp) - 1), numpy.diff(rp))
    rowsupp, colsupp = numpy.zeros(len(rp) - 1, dtype=bool), numpy.zeros(ncols, dtype=bool)
    rowsupp[rows[keep]] = True
    colsupp[ci[keep]] = True
    return rowsupp, colsupp


@pytest.mark.parametrize('narrow', [True, False], ids=['int32', 'int64'])
@pytest.mark.parametrize('name', NAMES)
def test_support(name, narrow):
    from nutils_amd import device, kernels, _lib
    (values, rowptr, colidx), ncols, v, rp, ci = triplet(name)
    col32 = kernels.csr_compact(colidx, ncols) if narrow and len(v) else None
    for tol in tolerances(v):
        rows, cols = expected(v, rp, ci, ncols, tol)
        if len(v) and tol == abs(v).max():
            assert not rows.any() and not cols.any()
        for lanes in LANES if name != 'tridiagonal' else (0, 64):
            with _lib.trace() as calls:
                rs, cs = kernels.csr_support(values, rowptr, colidx, ncols, tol, col32=col32, lanes=lanes)
            assert calls == ['nh_csr_support']
            rs, cs = device.to_host(rs), device.to_host(cs)
            assert rs.dtype == numpy.uint8 and numpy.array_equal(rs, rows.astype(numpy.uint8)), (tol, lanes)
            assert cs.dtype == numpy.uint8 and numpy.array_equal(cs, cols.astype(numpy.uint8)), (tol, lanes)
        # a second call gives the same bytes; either result may be left out
        rs2, cs2 = kernels.csr_support(values, rowptr, colidx, ncols, tol, col32=col32)
        assert numpy.array_equal(device.to_host(rs2), rs) and numpy.array_equal(device.to_host(cs2), cs)
        only_rows, none = kernels.csr_support(values, rowptr, colidx, ncols, tol, cols=False, col32=col32)
        assert none is None and numpy.array_equal(device.to_host(only_rows), rs)
        none, only_cols = kernels.csr_support(values, rowptr, colidx, ncols, tol, rows=False, col32=col32)
        assert none is None and numpy.array_equal(device.to_host(only_cols), cs)


@pytest.mark.parametrize('name', NAMES)
def test_matrix_interface(name):
    '''HipMatrix.rowsupp / colsupp: host bool vectors, tol = 0 by default, the matrix not exported'''
    from nutils_amd import matrix
    (values, rowptr, colidx), ncols, v, rp, ci = triplet(name)
    A = matrix.HipMatrix(values, rowptr, colidx, ncols)
    for tol in [None] + tolerances(v):
        rows, cols = expected(v, rp, ci, ncols, tol or 0.)
        rs, cs = (A.rowsupp(), A.colsupp()) if tol is None else (A.rowsupp(tol), A.colsupp(tol))
        assert rs.dtype == bool and rs.shape == (A.shape[0],) and numpy.array_equal(rs, rows)
        assert cs.dtype == bool and cs.shape == (A.shape[1],) and numpy.array_equal(cs, cols)
    assert A._hostcsr is None
    with pytest.raises(matrix.MatrixError):
        A.colsupp(-1.)


def test_strictness_by_hand():
    '''|a| > tol, not >=: 'holes' at tol = 3 keeps 4, 6, -7 (rows 2 and 4; columns 0, 4, 5)'''
    from nutils_amd import matrix
    (values, rowptr, colidx), ncols, *_ = triplet('holes')
    A = matrix.HipMatrix(values, rowptr, colidx, ncols)
    assert A.rowsupp(3.).tolist() == [False, False, True, False, True, False]
    assert A.colsupp(3.).tolist() == [True, False, False, False, True, True]
    assert A.rowsupp().tolist() == [False, True, True, False, True, False]
