'''The batched conjugate-gradient solve (matrix.HipMatrix.solve_columns, nh_csr_multi.hip) on the GPU: independent columns against the solve contract, against a
direct solve and against the single-vector solve byte for byte; the shared bound of the reference's stopping rule; groups of eight columns; the iterations
enqueued past convergence; a restart from the true residuals; a breakdown in one column; a `maxiter` between two looks; the grid caps; device in, device out.

Problems and helpers are those of test_gpu_cg and test_cg_host.'''
import functools
import numpy
import pytest
import scipy.sparse

from test_gpu_cg import problem, same_bytes, with_lanes, hip, RTOL
from test_cg_host import cg_reference, diagonal_family, restart_case, SCALES

pytestmark = pytest.mark.gpu


def solve_columns(A, rhs, **kwargs):
    '''(A.solve_columns that insists on the batched device route, the number of nh_cgm_init calls it made)'''
    from nutils_amd import _lib
    with _lib.trace() as calls:
        try:
            return A.solve_columns(rhs, **kwargs), calls.count('nh_cgm_init')
        finally:
            assert 'nh_cgm_init' in calls and 'nh_cgm_iterate' in calls and 'nh_csr_spmm' in calls, calls
            assert 'nh_cg_iterate' not in calls and 'nh_cg_init' not in calls and 'nh_csr_spmv' not in calls, calls
            assert A._hostcsr is None  # neither values nor indices went to the host


@functools.lru_cache(maxsize=None)
def wide_columns():
    '''Five right-hand sides on 'wide' (the 40 x 37 bilinear Laplace, one side held at non-zero values).  In terms of the residual block r0 = mask(rhs - A start)
    they are the problem's own, 1e-6 of it, a zero column and two random ones.  The held values are not zero, so the right-hand side whose residual vanishes is
    A start, not 0, and the one whose residual is 1e-6 of the first is A start + 1e-6 (rhs - A start): those are columns 2 and 1.  Returns (rhs block, |r0_j|,
    direct solutions); made once, never written.'''
    from nutils_amd import matrix
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    rng = numpy.random.default_rng(12)
    held = ref @ start
    B = numpy.stack([rhs, held + 1e-6 * (rhs - held), held, rng.normal(size=len(rhs)), rng.normal(size=len(rhs))], axis=1)
    r0s = numpy.linalg.norm((B - held[:, None])[free], axis=0)
    assert r0s[0] == r0 and abs(r0s[1] / r0 - 1e-6) < 1e-12 and r0s[2] == 0 and (r0s[3:] > 0).all()
    directs = numpy.stack([matrix.ScipyMatrix(ref).solve(B[:, j], **kwargs) for j in range(B.shape[1])], axis=1)
    return B, r0s, directs


def column_contract(name, B, X, bound, directs=None):
    '''what a solve to an absolute bound promises, per column: constrained dofs exactly, the true residual within the bound (with the slack test_gpu_cg.contract
    has for scipy's own rounding), the error within residual / lambda_min.  Returns the residual norms.'''
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem(name)
    assert isinstance(X, numpy.ndarray) and X.shape == B.shape
    res = numpy.linalg.norm((B - ref @ X)[free], axis=0)
    for j in range(B.shape[1]):
        assert numpy.array_equal(X[~free, j], start[~free]), j
        print(f'{name}, column {j}: |r| / bound = {res[j] / bound:.3e}' + ('' if directs is None else f', |x - x_direct| = {numpy.linalg.norm(X[:, j] - directs[:, j]):.3e}, bound {res[j] / lmin:.3e}'))
        assert res[j] <= bound * (1 + 1e-3), j
        if directs is not None:
            assert numpy.linalg.norm(X[:, j] - directs[:, j]) <= res[j] / lmin, j
    return res


@pytest.mark.parametrize('precon', ['diag', None])
@pytest.mark.parametrize('lanes', [4, 64])
def test_independent_columns(lanes, precon):
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    A = with_lanes(A, lanes)
    B, r0s, directs = wide_columns()
    atol = RTOL * r0s.max()
    X, inits = solve_columns(A, B, atol=atol, precon=precon, **kwargs)  # (default maxiter: the free dofs; check=16)
    counts, its = list(A.column_iterations), A.iterations
    column_contract('wide', B, X, atol, directs)
    assert same_bytes(X[:, 2].copy(), start) and counts[2] == 0  # the column without a residual is its start vector
    assert 0 < counts[1] < counts[0]  # the shared bound is 1e-4 of the small column's residual and 1e-10 of the large one's
    assert its % 16 == 0 and max(counts) <= its <= free.sum()
    # every column is the single-vector solve of that column
    for j in range(B.shape[1]):
        x = A.solve(B[:, j], atol=atol, precon=precon, check=1, **kwargs)
        assert same_bytes(X[:, j].copy(), x), (j, numpy.abs(X[:, j] - x).max())
        assert counts[j] == A.cg_iterations, (j, counts, A.cg_iterations)
    # the looks do not matter, and a repeat is the same
    Y, inits1 = solve_columns(A, B, atol=atol, precon=precon, check=1, **kwargs)
    assert same_bytes(X, Y) and A.column_iterations == counts and max(counts) <= A.iterations <= its
    assert same_bytes(solve_columns(A, B, atol=atol, precon=precon, **kwargs)[0], X) and A.column_iterations == counts and A.iterations == its
    # the count against the numpy restatement at the shared bound (the rule of test_gpu_cg: another order of summation moves it by an iteration or two)
    dinv = numpy.where(free, 1 / ref.diagonal(), 0.) if precon else None
    x_ref, it_ref, starts, outcome = cg_reference(ref, rhs, start, free, dinv, atol ** 2, int(free.sum()), check=1)
    print(f'wide, lanes={lanes}, precon={precon}: counts {counts}, {its} enqueued, {inits} starts on the device; column 0 in numpy: {it_ref} iterations, {starts} starts')
    assert outcome == 'converged' and counts[0] <= 1.1 * it_ref + 2


def test_relative_bound():
    '''rtol is relative to the LARGEST first residual of the call (matrix/_base.py:204-222 of the reference): one bound for all columns'''
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    B, r0s, directs = wide_columns()
    X, inits = solve_columns(A, B, rtol=RTOL, **kwargs)
    res = column_contract('wide', B, X, RTOL * r0s.max(), directs)
    counts = A.column_iterations
    # a bound of its own would have the small column work as long as the large one, and the column without a residual iterate on its rounding errors
    assert counts[2] == 0 and same_bytes(X[:, 2].copy(), start) and 0 < counts[1] < counts[0]
    assert res[1] > RTOL * r0s[1]  # (the small column stopped at the shared bound, far above one of its own)


def test_groups_and_iterations_past_convergence():
    '''The diagonal family of test_cg_host, 18 right-hand sides: groups of 8, 8 and 2 columns.  Jacobi-CG is there after one iteration; of the iterations that `check`
    enqueues after it none may raise (their r . z underflows before r . r does), and the columns whose start is within the shared bound never move.'''
    d, b = diagonal_family()
    A = hip(scipy.sparse.diags(d, format='csr'))
    B = numpy.stack([scale * b for scale in SCALES], axis=1)
    assert B.shape[1] == 18
    atol = RTOL * numpy.linalg.norm(b)
    singles = []
    for j in range(18):
        singles.append((A.solve(B[:, j], atol=atol, check=1), A.cg_iterations))
    expect = [0 if numpy.linalg.norm(B[:, j]) <= atol else 1 for j in range(18)]
    assert expect[:6] == [1] * 6 and not any(expect[6:]) and [it for x, it in singles] == expect
    for check in (16, 32):
        X, inits = solve_columns(A, B, atol=atol, check=check)
        assert A.column_iterations == expect and A.iterations == check
        assert inits == 4  # a start per group, and the first group's look at its true residuals
        for j in range(18):
            assert same_bytes(X[:, j].copy(), singles[j][0]), j


def test_restart():
    '''The restart case of test_cg_host as column 0 and the same right-hand side from a zero start as column 1.  The recurrence of column 0 drifts from its true
    residual by 4e-12 |r0|, well above the bound: when both recurrences are within it the true residual of column 0 is not, and it goes on from there.'''
    from nutils_amd import _lib
    ref, rhs, lhs0, solution = restart_case()
    A = problem('restart')[0]
    n = len(rhs)
    B = numpy.stack([rhs, rhs], axis=1)
    L = numpy.stack([lhs0, numpy.zeros(n)], axis=1)
    atol = 1e-13 * numpy.linalg.norm(rhs - ref @ lhs0)
    for check in (16, 1):
        X, inits = solve_columns(A, B, lhs0=L, atol=atol, precon=None, maxiter=10 * n, check=check)
        res = numpy.linalg.norm(B - ref @ X, axis=0)
        print(f'restart, check={check}: counts {A.column_iterations}, {A.iterations} enqueued, {inits} starts; |r| / bound = {res / atol}')
        assert inits >= 3  # the first start, at least one restart, the last look
        assert (res <= atol * (1 + 1e-3)).all()
        assert all(count > 0 for count in A.column_iterations)
    # an (n,) start is broadcast over the columns; a column does not depend on its neighbours
    Y, inits = solve_columns(A, B, lhs0=lhs0, atol=atol, precon=None, maxiter=10 * n)
    assert same_bytes(Y[:, 0].copy(), Y[:, 1].copy()) and same_bytes(Y[:, 0].copy(), X[:, 0].copy())


@pytest.mark.parametrize('check', [1, 16])
@pytest.mark.parametrize('precon', ['diag', None])
def test_breakdown_in_one_column(precon, check):
    from nutils_amd import matrix
    A = hip(scipy.sparse.diags([1., -1.], format='csr'))
    with pytest.raises(matrix.MatrixError, match='not positive definite'):
        A.solve_columns(numpy.eye(2), rtol=1e-8, precon=precon, check=check)
    X, inits = solve_columns(A, numpy.array([[1.], [0.]]), rtol=1e-8, precon=precon, check=check)
    assert X.tolist() == [[1.], [0.]] and A.column_iterations == [1]


def test_maxiter_between_two_looks():
    from nutils_amd import matrix
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    B, r0s, directs = wide_columns()
    with pytest.raises(matrix.ToleranceNotReached) as info:
        solve_columns(A, B, rtol=RTOL, maxiter=21, check=16, **kwargs)
    best = info.value.best
    assert A.iterations == 21 and A.column_iterations[0] == 21 and A.column_iterations[2] == 0
    assert best.shape == B.shape and numpy.isfinite(best).all() and numpy.array_equal(best[~free], numpy.repeat(start[~free, None], 5, axis=1))
    res = numpy.linalg.norm((B - ref @ best)[free], axis=0)
    assert RTOL * r0s.max() < res[0] < r0s[0]  # 21 iterations got somewhere, not there


def test_grid_caps():
    '''262 444 rows: the vector kernels stride, and at a row per wave so do the product and its epilogue'''
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('tridiagonal')
    assert A.shape[0] > 1024 * 256
    A = with_lanes(A, 64)
    assert A.shape[0] / (256 // A.lanes) > 2048
    B = numpy.stack([rhs, -rhs], axis=1)
    r0s = numpy.linalg.norm((B - (ref @ start)[:, None])[free], axis=0)
    for precon in ('diag', None):
        X, inits = solve_columns(A, B, rtol=RTOL, precon=precon, **kwargs)
        column_contract('tridiagonal', B, X, RTOL * r0s.max())
        assert same_bytes(solve_columns(A, B, rtol=RTOL, precon=precon, **kwargs)[0], X)
        print(f'tridiagonal, precon={precon}: counts {A.column_iterations}, {A.iterations} enqueued')


def test_device_in_device_out():
    from nutils_amd import device
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    B, r0s, directs = wide_columns()
    X, inits = solve_columns(A, B, rtol=RTOL, **kwargs)
    Bd = device.to_dev(B, 'float64')
    Xd, inits = solve_columns(A, Bd, rtol=RTOL, **kwargs)
    assert Xd.is_cuda and Xd.device == Bd.device and tuple(Xd.shape) == B.shape and same_bytes(device.to_host(Xd), X)
    assert same_bytes(device.to_host(Bd), B)  # the right-hand side is never written
    # a column slice of a wider tensor is a right-hand side too
    Wd = device.to_dev(numpy.concatenate([B[:, 3:], B], axis=1), 'float64')
    Yd, inits = solve_columns(A, Wd[:, 2:7], rtol=RTOL, **kwargs)
    assert same_bytes(device.to_host(Yd), X)
