'''The matrix algebra of HipMatrix on the device (nh_csr_ops.hip): `T`, `submatrix` and sums of different patterns against the numpy references of
csr_ops_refs.py, which test_csr_ops_refs_host.py pins to scipy -- indices equal, values as int64 views.  Every test asserts with `_lib.trace()` which entry
points ran (the new ones at the first call, nh_index_copy alone when a plan is used again) and that no matrix got a host copy.

Shapes are the smallest at which each kernel can go wrong (csr_ops_refs.case): no entries; empty first, middle and last rows and columns; 5 x 70 and 70 x 5; row
and column lengths below, at and above every lane count and the 64 entries that one wave sorts in registers; a dense row and a dense column of 3000 entries
('cross': the column is an output row of the transpose beyond the 2048 entries a workgroup sorts in LDS, the slow path); and the 262 444-row tridiagonal matrix
at which every grid strides (csr_ops_refs.tridiagonal has the derivation).'''
import functools

import numpy
import pytest

import csr_ops_refs as refs
from csr_ops_refs import Csr
from test_gpu_matrix_hip import case as assembled_case, product_bound

pytestmark = pytest.mark.gpu

POWERS = (1, 2, 4, 8, 16, 32, 64)


@functools.lru_cache(maxsize=None)
def tensors(name):
    '''the device triplet of a case, uploaded once and never written'''
    from nutils_amd import device
    m = refs.case(name)
    return device.to_dev(m.values, 'float64'), device.to_dev(m.rowptr, 'int64'), device.to_dev(m.colidx, 'int64'), m.ncols


def fresh(name, lanes=None):
    '''a new HipMatrix (no plans yet) on the case's tensors, and its host twin'''
    from nutils_amd import matrix
    A = matrix.HipMatrix(*tensors(name))
    if lanes:
        A.lanes = lanes
    return A, refs.case(name)


def upload(m):
    from nutils_amd import device, matrix
    return matrix.HipMatrix(device.to_dev(m.values, 'float64'), device.to_dev(m.rowptr, 'int64'), device.to_dev(m.colidx, 'int64'), m.ncols)


def triplet(A):
    from nutils_amd import device
    torch = device.torch()
    values, rowptr, colidx = A.triplet()
    assert values.dtype == torch.float64 and rowptr.dtype == torch.int64 and colidx.dtype == torch.int64
    assert rowptr.numel() == A.shape[0] + 1 and values.numel() == colidx.numel() == A.nnz
    return Csr(device.to_host(values), device.to_host(rowptr), device.to_host(colidx), A.shape[1])


def no_host_copies(*matrices):
    assert all(A._hostcsr is None for A in matrices)


def finite(m):
    return m._replace(values=numpy.where(numpy.isfinite(m.values), m.values, 1.))


def to_scipy(m):
    import scipy.sparse
    return scipy.sparse.csr_matrix((m.values, m.colidx, m.rowptr), (len(m.rowptr) - 1, m.ncols))


# ---- transpose ------------------------------------------------------------------------------------------------------------------------------------------

def check_transpose(A, m):
    from nutils_amd import _lib, device
    torch = device.torch()
    with _lib.trace() as calls:
        T = A.T
    assert 'nh_csr_transpose' in calls and calls.count('nh_index_copy') == (1 if len(m.values) else 0), calls
    ref = refs.transposed(m)
    assert refs.same(triplet(T), ref)
    pos = device.to_host(A._tplan.pos)
    assert numpy.array_equal(numpy.sort(pos), numpy.arange(len(m.values))) and numpy.array_equal(pos, refs.ref_transpose(m.rowptr, m.colidx, m.ncols)[2])
    # a second matrix on the same tensors: its own plan, identical index tensors
    from nutils_amd import matrix
    A2 = matrix.HipMatrix(*A.triplet(), A.shape[1])
    T2 = A2.T
    assert A2._tplan is not A._tplan and all(torch.equal(a, b) for a, b in zip(T.triplet()[1:] + (A._tplan.pos,), T2.triplet()[1:] + (A2._tplan.pos,)))
    assert refs.same(triplet(T.T), m)
    # the plan again, for other values: one gather, the index tensors shared
    fin = finite(m)
    B = A._with_values(device.to_dev(fin.values, 'float64'))
    with _lib.trace() as calls:
        BT = B.T
    assert calls == (['nh_index_copy'] if len(m.values) else []), calls
    assert BT.triplet()[1] is T.triplet()[1] and BT.triplet()[2] is T.triplet()[2]
    x = numpy.random.default_rng(3).normal(size=A.shape[0])
    host = to_scipy(refs.transposed(fin))
    err = numpy.abs(BT @ x - host @ x)
    assert (err <= product_bound(host, x)).all(), (err / numpy.maximum(product_bound(host, x), 1e-300)).max()
    no_host_copies(A, A2, T, T2, B, BT)
    return T


@pytest.mark.parametrize('name', refs.CASES)
def test_transpose(name):
    check_transpose(*fresh(name))


@pytest.mark.parametrize('name', ['rectangular', 'bilinear'])
def test_transpose_assembled(name):
    '''on what the assembly leaves in HBM, with and without the int32 columns'''
    from nutils_amd import matrix
    dev, ncols, ref, x = assembled_case(name)
    m = Csr(ref.data, ref.indptr.astype(refs.I64), ref.indices.astype(refs.I64), ncols)
    check_transpose(matrix.HipMatrix(*dev, ncols), m)
    A = matrix.HipMatrix(*dev, ncols)
    assert A._columns() is not None
    check_transpose(A, m)


# ---- submatrix ------------------------------------------------------------------------------------------------------------------------------------------

def check_submatrix(A, m, which, integers=False):
    from nutils_amd import _lib
    r, c = refs.masks(m)[which]
    r = numpy.ones(A.shape[0], dtype=bool) if r is None else r
    c = numpy.ones(A.shape[1], dtype=bool) if c is None else c
    with _lib.trace() as calls:
        S = A.submatrix(numpy.flatnonzero(r), numpy.flatnonzero(c)) if integers else A.submatrix(r, c)
    if r.all() and c.all():
        assert S is A and not calls
        return S
    ref = refs.selected(m, r, c)
    assert calls == ['nh_csr_select_count'] + (['nh_csr_select_fill', 'nh_index_copy'] if len(ref.values) else []), (which, calls)  # (nothing kept: nothing to fill)
    assert S.shape == (r.sum(), c.sum()) and refs.same(triplet(S), ref), (which, A.lanes)
    no_host_copies(A, S)
    return S


@pytest.mark.parametrize('name', refs.CASES)
def test_submatrix(name):
    for which in refs.masks(refs.case(name)):
        check_submatrix(*fresh(name), which)
        check_submatrix(*fresh(name), which, integers=True)


@pytest.mark.parametrize('lanes', POWERS)
@pytest.mark.parametrize('name', ['rowlens', 'cross'])
def test_submatrix_at_every_lane_count(name, lanes):
    for which in ('rows', 'cols', 'both'):
        check_submatrix(*fresh(name, lanes), which)


def test_submatrix_of_assembled_rectangular():
    '''different masks for rows and columns, on the int32 columns of the product'''
    from nutils_amd import matrix
    dev, ncols, ref, x = assembled_case('rectangular')
    m = Csr(ref.data, ref.indptr.astype(refs.I64), ref.indices.astype(refs.I64), ncols)
    for narrow in (False, True):
        for which in ('rows', 'cols', 'both', 'other'):
            A = matrix.HipMatrix(*dev, ncols)
            assert not narrow or A._columns() is not None
            check_submatrix(A, m, which)


def test_submatrix_of_everything():
    A, m = fresh('random')
    assert A.submatrix(numpy.ones(A.shape[0], dtype=bool), numpy.arange(A.shape[1])) is A


def test_cg_on_the_free_block():
    '''CG on A.submatrix(free, free) is the iteration of the masked solve of A: the same number of iterations, the same solution to the bound of both'''
    from nutils_amd import function, matrix
    from test_gpu_bicgstab import laplace
    K, kwargs, rhs = laplace((13, 10))
    A = function.eval(function.as_matrix(K))
    free, lhs = matrix.constraints(A.shape[1], kwargs['constrain'])
    x = A.solve(rhs, solver='cg', rtol=1e-10, **kwargs)
    masked = A.iterations
    S = A.submatrix(free, free)
    assert S.shape == (free.sum(),) * 2
    xs = S.solve((rhs - A @ lhs)[free], solver='cg', rtol=1e-10)
    print(f'iterations: masked {masked}, submatrix {S.iterations}; |difference| {numpy.abs(lhs[free] + xs - x[free]).max():.3e}')
    assert S.iterations == masked
    assert numpy.abs(lhs[free] + xs - x[free]).max() <= 1e-8 * numpy.abs(x).max()
    no_host_copies(A, S)


# ---- plans ----------------------------------------------------------------------------------------------------------------------------------------------

def test_plans_are_handed_on():
    from nutils_amd import _lib, device
    A, m = fresh('random')
    r, c = refs.masks(m)['both']
    S, T = A.submatrix(r, c), A.T
    col32 = S._columns()
    assert col32 is not None
    v2 = numpy.random.default_rng(8).normal(size=len(m.values))
    B = A._with_values(device.to_dev(v2, 'float64'))
    with _lib.trace() as calls:
        S2, T2 = B.submatrix(r, c), B.T
    assert calls == ['nh_index_copy'] * 2, calls
    assert all(a is b for a, b in zip(S2.triplet()[1:] + T2.triplet()[1:], S.triplet()[1:] + T.triplet()[1:]))
    assert S2._col32 is col32  # (the matrix made before lives: what it had found out about the pattern carries over)
    m2 = m._replace(values=v2)
    assert refs.same(triplet(S2), refs.selected(m2, r, c)) and refs.same(triplet(T2), refs.transposed(m2))
    assert refs.same(triplet(S), refs.selected(m, r, c))  # (and the first one still has its own values)
    # another mask: a new plan, for this matrix only
    r2, c2 = refs.masks(m)['other']
    with _lib.trace() as calls:
        S3 = B.submatrix(r2, c2)
    assert 'nh_csr_select_count' in calls and 'nh_csr_select_fill' in calls and B._subplan is not A._subplan
    assert refs.same(triplet(S3), refs.selected(m2, r2, c2)) and S3.triplet()[2] is not S.triplet()[2]
    with _lib.trace() as calls:
        S4 = A.submatrix(r, c)
    assert calls == ['nh_index_copy'] and S4.triplet()[2] is S.triplet()[2]
    no_host_copies(A, B, S, S2, S3, S4, T, T2)


# ---- sums -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', refs.PAIRS)
def test_sum(name):
    from nutils_amd import _lib
    a, b = refs.pair(name)
    A, B = upload(a), upload(b)
    for sign in (1., -1.):
        ref = refs.ref_add(a, b, sign)  # (test_csr_ops_refs_host.py: scipy's triplet, so its nnz)
        union = len(refs.ref_union([(a.rowptr, a.colidx), (b.rowptr, b.colidx)])[1])
        with _lib.trace() as calls:
            C = A + B if sign > 0 else A - B
        assert [n for n in calls if n.startswith('nh_csr')] == ['nh_csr_add_values', 'nh_csr_select_count'] + ['nh_csr_select_fill'] * (0 < len(ref.values) < union), calls
        assert 'nh_pattern_union_fill' in calls
        assert C.nnz == len(ref.values) and refs.same(triplet(C), ref, computed=True), (name, sign)
        no_host_copies(A, B, C)
    assert refs.same(triplet(A - B), triplet(A + (-B)), computed=True)
    with _lib.trace() as calls:
        D = A + 2. * A  # one pattern: values only, as before, zeros kept
    assert not calls and D.triplet()[2] is A.triplet()[2]


# ---- every grid strides ---------------------------------------------------------------------------------------------------------------------------------

def test_striding_grids():
    '''csr_ops_refs.tridiagonal: 262 444 rows, 787 330 entries'''
    from nutils_amd import _lib
    A, m = fresh('tridiagonal')
    T = A.T
    t = refs.transposed(m)
    assert refs.same(triplet(T), t)
    r, c = refs.masks(m)['both']
    for lanes in (2, 64):
        A.lanes, A._subplan = lanes, None
        with _lib.trace() as calls:
            S = A.submatrix(r, c)
        assert 'nh_csr_select_fill' in calls and refs.same(triplet(S), refs.selected(m, r, c)), lanes
    with _lib.trace() as calls:
        D = A - T  # the same pattern on other tensors: the union, and the diagonal cancels
    assert 'nh_csr_add_values' in calls and 'nh_csr_select_fill' in calls
    assert D.nnz == A.nnz - A.shape[0] and refs.same(triplet(D), refs.ref_add(m, t, -1.), computed=True)
    no_host_copies(A, T, S, D)
