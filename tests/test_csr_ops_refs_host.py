'''The references of tests/csr_ops_refs.py against scipy, computed the way the host path of HipMatrix computes them (`_transpose_host`, `_submatrix_host`,
`_add_host`: the scipy operation, then sum_duplicates and sort_indices): triplets equal index for index and values bit for bit.  And the host side of
`HipMatrix.submatrix` -- the selector checks, the fallback for unordered indices, the whole matrix returned as itself -- on matrices of host arrays, with
nothing uploaded.  No GPU, no library.'''
import warnings

import numpy
import pytest
import scipy.sparse

import csr_ops_refs as refs
from csr_ops_refs import Csr, I64


def to_scipy(m):
    return scipy.sparse.csr_matrix((m.values, m.colidx, m.rowptr), (len(m.rowptr) - 1, m.ncols))


def from_scipy(core):
    '''matrix.HipMatrix._from_scipy'''
    core = core.tocsr()
    core.sum_duplicates()
    core.sort_indices()
    return Csr(core.data, core.indptr.astype(I64), core.indices.astype(I64), core.shape[1])


def scipy_add(a, b, sign):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)  # (inf - inf)
        return from_scipy(to_scipy(a) + sign * to_scipy(b))


HOST_CASES = refs.CASES + ('tridiagonal',)


@pytest.mark.parametrize('name', HOST_CASES)
def test_transpose(name):
    m = refs.case(name)
    rowptr_t, colidx_t, pos = refs.ref_transpose(m.rowptr, m.colidx, m.ncols)
    assert numpy.array_equal(numpy.sort(pos), numpy.arange(len(m.values)))  # a permutation
    t = refs.transposed(m)
    assert refs.same(t, from_scipy(to_scipy(m).T))
    assert refs.same(refs.transposed(t), m)


@pytest.mark.parametrize('name', refs.CASES)
def test_select(name):
    m = refs.case(name)
    core = to_scipy(m)
    for which, (r, c) in refs.masks(m).items():
        rows = numpy.arange(core.shape[0]) if r is None else numpy.flatnonzero(r)
        cols = numpy.arange(core.shape[1]) if c is None else numpy.flatnonzero(c)
        assert refs.same(refs.selected(m, r, c), from_scipy(core[rows, :][:, cols])), which
        rowptr_s, colidx_s, pos, _ = refs.ref_select(m.values, m.rowptr, m.colidx, m.ncols, r, c)
        assert (numpy.diff(pos) > 0).all() and len(rowptr_s) == len(rows) + 1, which  # entries keep their order


def test_select_keeps_special_values():
    m = refs.case('wide')
    s = refs.selected(m, numpy.ones(5, dtype=bool), numpy.ones(70, dtype=bool))
    assert refs.same(s, m) and numpy.isnan(m.values).sum() == 2 and (m.values == 0).sum() == 2 and numpy.signbit(m.values[m.values == 0]).sum() == 1


@pytest.mark.parametrize('sign', [1., -1.])
@pytest.mark.parametrize('name', refs.PAIRS)
def test_add(name, sign):
    a, b = refs.pair(name)
    s = refs.ref_add(a, b, sign)
    assert refs.same(s, scipy_add(a, b, sign), computed=True)
    assert refs.same(s, refs.ref_add(a, Csr(-b.values, b.rowptr, b.colidx, b.ncols), -sign), computed=True)  # A - B is A + (-B)


def test_add_cancellation():
    '''what the 'cancel' pair is for: an entry that cancels is gone, one that cancels to a rounding stays, NaN stays'''
    a, b = refs.pair('cancel')
    s = refs.ref_add(a, b, 1.)
    dense = to_scipy(s).toarray()
    assert s.colidx[s.rowptr[0]:s.rowptr[1]].tolist() == [0, 2, 3] and dense[0, 2] == (.1 + .2) - .3 != 0
    assert s.colidx[s.rowptr[1]:s.rowptr[2]].tolist() == [0, 1, 2, 3] and numpy.isnan(dense[1, 1:3]).all()
    assert s.rowptr[2] == s.rowptr[3] and s.rowptr[4] == s.rowptr[5]
    assert len(refs.ref_add(*refs.pair('all_cancel'), 1.).values) == 0
    assert len(refs.ref_add(*refs.pair('all_cancel'), -1.).values) == (refs.pair('all_cancel')[0].values != 0).sum()


def test_add_of_tridiagonal_and_its_transpose():
    m = refs.case('tridiagonal')
    t = refs.transposed(m)  # the same pattern with other values: the antisymmetric part has no diagonal
    s = refs.ref_add(m, t, -1.)
    assert refs.same(s, scipy_add(m, t, -1.), computed=True) and len(s.values) == len(m.values) - (len(m.rowptr) - 1)


# ---- HipMatrix.submatrix on the host: nothing is uploaded ---------------------------------------------------------------------------------------------

def hipmatrix(name='random'):
    from nutils_amd import matrix
    m = refs.case(name)
    return matrix.HipMatrix(m.values, m.rowptr, m.colidx, m.ncols), m


def triplet(A):
    values, colidx, rowptr = A.export('csr')
    return Csr(values, rowptr, colidx, A.shape[1])


def test_submatrix_rejects_bad_selectors_before_any_upload():
    from nutils_amd import matrix
    A, m = hipmatrix()
    nrows, ncols = A.shape
    allrows, allcols = numpy.ones(nrows, dtype=bool), numpy.ones(ncols, dtype=bool)
    for rows, cols in [(numpy.ones(nrows + 1, dtype=bool), allcols), (allrows, numpy.ones(ncols - 1, dtype=bool)),  # wrong length
                       ([0, nrows], allcols), (allrows, [0, ncols]), ([-nrows - 1, 0], allcols), ([3, nrows, 1], allcols),  # out of range, sorted or not
                       ([0., 1.], allcols), (allrows, numpy.array([.5])), (allrows, ['a']),  # neither bool nor integer
                       (numpy.ones((nrows, 1), dtype=bool), allcols)]:  # not a vector
        with pytest.raises(matrix.MatrixError):
            A.submatrix(rows, cols)
    assert A._dev is None


def test_submatrix_of_everything_is_the_matrix():
    A, m = hipmatrix()
    nrows, ncols = A.shape
    assert A.submatrix(numpy.ones(nrows, dtype=bool), numpy.ones(ncols, dtype=bool)) is A
    assert A.submatrix(numpy.arange(nrows), numpy.arange(ncols)) is A
    assert A.submatrix(numpy.ones(nrows, dtype=bool), list(range(ncols))) is A
    assert A._dev is None


def test_unordered_selection_keeps_the_host_path():
    A, m = hipmatrix()
    core = to_scipy(m)
    nrows, ncols = A.shape
    for rows, cols in [([5, 2, 9], [0, 3, 4]), ([1, 1, 2], numpy.ones(ncols, dtype=bool)), (numpy.ones(nrows, dtype=bool), [7, 0]), ([-1, 0], [-2])]:
        S = A.submatrix(rows, cols)
        r = numpy.flatnonzero(rows) if numpy.asarray(rows).dtype == bool else numpy.asarray(rows)
        c = numpy.flatnonzero(cols) if numpy.asarray(cols).dtype == bool else numpy.asarray(cols)
        assert refs.same(triplet(S), from_scipy(core[r, :][:, c]))
        assert A._dev is None and S._dev is None


def test_selector():
    from nutils_amd import matrix
    assert matrix._selector([1, 3], 4, 'row').tolist() == [False, True, False, True]  # numeric.asboolean
    assert matrix._selector([], 3, 'row').tolist() == [False] * 3
    assert matrix._selector(numpy.array([2], dtype=numpy.uint8), 3, 'row').tolist() == [False, False, True]
    assert matrix._selector([3, 1], 4, 'row') is None and matrix._selector([1, 1], 4, 'row') is None and matrix._selector([-1], 4, 'row') is None


def test_repeated_columns_keep_the_host_path():
    '''a host triplet may repeat a column inside a row (the validation lets it pass, as the reference's does); the device algebra takes sorted unique rows for
    granted, so such a matrix is transposed where scipy sums the duplicates'''
    from nutils_amd import matrix
    A = matrix.HipMatrix(numpy.array([1., 2., 3.]), numpy.array([0, 2, 3]), numpy.array([1, 1, 0]), 2)
    assert not A._unique() and hipmatrix()[0]._unique()
    T = A.T
    assert A._dev is None and T.export('dense').tolist() == [[0., 3.], [3., 0.]]
