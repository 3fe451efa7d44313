'''The device conjugate-gradient solve (matrix.HipMatrix.solve(solver='cg'), nh_csr.hip) on the GPU beyond one workgroup and past convergence: one iteration
against the numpy restatement of tests/test_cg_host.py evaluated in longdouble, with derived bounds; the solve contract and the iteration counts where
several workgroups' partials are summed and where the grids stride; the iterations that `check` enqueues past convergence; a restart; a `maxiter` that is no
multiple of `check`.

Sizes: 1480 rows are six vector workgroups, the last one partial (200 of 256 threads), and 24 product workgroups at 4 lanes per row, 370 at 64; 262 444 rows
are more than 1024 * 256, so the vector kernels stride, and at 64 lanes more than 2048 product workgroups' worth, so the product and its epilogue stride.'''
import functools
import numpy
import pytest
import scipy.sparse

from test_cg_host import Recurrence, cg_reference, diagonal_family, restart_case, one_step_of_jacobi, gamma, SCALES, U

pytestmark = pytest.mark.gpu

RTOL = 1e-10


def hip(core):
    '''a host matrix as a HipMatrix on device tensors (so that `_hostcsr` shows whether a solve exported it)'''
    from nutils_amd import device, matrix
    core = scipy.sparse.csr_matrix(core, dtype=float)
    core.sort_indices()
    return matrix.HipMatrix(device.to_dev(core.data, 'float64'), device.to_dev(core.indptr, 'int64'), device.to_dev(core.indices, 'int64'), core.shape[1])


def solve(A, rhs=None, **kwargs):
    '''(A.solve(solver='cg') that insists on the device route, the number of nh_cg_init calls it made)'''
    from nutils_amd import _lib
    with _lib.trace() as calls:
        try:
            return A.solve(rhs, **kwargs), calls.count('nh_cg_init')
        finally:
            assert 'nh_cg_init' in calls and 'nh_cg_iterate' in calls, calls
            assert A._hostcsr is None  # neither values nor indices went to the host


def with_lanes(A, lanes):
    B = A._with_values(A.triplet()[0])
    B.lanes = lanes
    return B


# ---- problems ------------------------------------------------------------------------------------------------------------

def tridiagonal(n=262444):
    K = scipy.sparse.diags([-numpy.ones(n - 1), numpy.full(n, 4.), -numpy.ones(n - 1)], [-1, 0, 1], format='csr')
    cons = numpy.full(n, numpy.nan)
    cons[::1000] = 2.
    return K, dict(constrain=cons), numpy.random.default_rng(4).normal(size=n)


@functools.lru_cache(maxsize=None)
def problem(name):
    '''the matrix on the device, its host twin, the solve's keywords and right-hand side, the free mask, the start vector, |r0|; for the small problems also
    the direct solution (of 'restart': the vector its right-hand side was made of) and the smallest eigenvalue of the free block.  Made once, never written.'''
    from nutils_amd import function, matrix
    from test_gpu_bicgstab import laplace
    if name == 'wide':  # the 40 x 37 bilinear Laplace, one side held at non-zero values
        K, kwargs, rhs = laplace((40, 37))
        A = function.eval(function.as_matrix(K))
        v, rp, ci = function.eval(function.as_csr(K))
        ref = scipy.sparse.csr_matrix((v, ci, rp), A.shape)
    else:
        if name == 'tridiagonal':
            ref, kwargs, rhs = tridiagonal()
        else:
            ref, rhs, lhs0, solution = restart_case()
            kwargs = dict(lhs0=lhs0)
        A = hip(ref)
    assert A._hostcsr is None
    free, start = matrix.constraints(A.shape[1], kwargs.get('constrain'), kwargs.get('lhs0'))
    r0 = numpy.linalg.norm((rhs - ref @ start)[free])
    direct = lmin = None
    if A.shape[0] < 2000:
        direct = solution if name == 'restart' else matrix.ScipyMatrix(ref).solve(rhs, **kwargs)
        lmin = numpy.linalg.eigvalsh(ref.toarray()[free][:, free])[0]
        assert lmin > 0
    return A, ref, kwargs, rhs, free, start, r0, direct, lmin


@functools.lru_cache(maxsize=None)
def reference_iterations(name, precon, rtol=RTOL, maxiter=None):
    '''(iterations, starts) of the numpy restatement, looking at the residual after every iteration'''
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem(name)
    dinv = numpy.where(free, 1 / ref.diagonal(), 0.) if precon else None
    x, it, starts, outcome = cg_reference(ref, rhs, start, free, dinv, (rtol * r0) ** 2, maxiter or int(free.sum()), check=1)
    assert outcome == 'converged' and numpy.linalg.norm((rhs - ref @ x)[free]) <= rtol * r0 * (1 + 1e-3)
    return it, starts


def contract(name, x, rtol=RTOL):
    '''what a solve to rtol promises (test_gpu_matrix_hip.test_solve): constrained dofs exactly, the true residual within the bound, the error within
    residual / lambda_min'''
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem(name)
    assert isinstance(x, numpy.ndarray) and numpy.array_equal(x[~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ x)[free])
    print(f'{name}: |r| / |r0| = {res / r0:.3e}' + ('' if direct is None else f', |x - x_direct| = {numpy.linalg.norm(x - direct):.3e}, bound {res / lmin:.3e}'))
    assert res <= rtol * r0 * (1 + 1e-3)
    if direct is not None:
        assert numpy.linalg.norm(x - direct) <= res / lmin


def same_bytes(a, b):
    return numpy.array_equal(a.view(numpy.int64), b.view(numpy.int64))


# ---- one iteration against the restatement in longdouble ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def one_step(jacobi):
    '''Inputs of an iteration on 'wide' (x, r = mask(b - A x) and dinv as float64 vectors: the device gets the same bits), what nh_cg_init and one
    nh_cg_iterate make of them in longdouble, and how far float64 kernels may be from that.  With u = 2^-53, gamma_k = k u / (1 - k u), n = 1480, hats on
    what the device holds; every bound is evaluated on the reference's values:

    init       p^ = z^ = fl(dinv r): |p^ - p| <= dp = u |p| (nothing without a preconditioner).  r . z is a sum of n products of two or three factors in
               some order, against a reference that rounds too: relative error e_rz0 = gamma_(n+3) sum |r_i z_i| / |r . z|.
    product    q^ = mask(A p^): |q^ - q| <= dq = 2 gamma_(len+1) |A| |p| (product_bound of test_gpu_matrix_hip: the sum of a row in any order) + |A| dp.
    p . q      d_pq = sum (|p| dq + dp |q| + dp dq) + gamma_(n+2) sum (|p| + dp) (|q| + dq), relative error e_pq = d_pq / |p . q|.
    alpha      = fl(r.z^ / p.q^): e_alpha = (1 + e_rz0) (1 + u) / (1 - e_pq) - 1.
    x, r       fl(x + alpha^ p^), fl(r - alpha^ q^): the error of the product, one rounding of it (none if fused) and one of the sum:
               dx = |alpha p| e_ap + u m + u (|x| + m), e_ap = (1 + e_alpha) (1 + u) - 1, m = |alpha p| (1 + e_ap) (1 + u);
               dr = d_aq + u t + u (|r| + t), d_aq = |alpha| ((1 + e_alpha) dq + e_alpha |q|), t = (|alpha q| + d_aq) (1 + u).
    r . r      d_rr = sum (2 |r'| dr + dr^2) + gamma_(n+2) sum (|r'| + dr)^2: this is work[0].
    r . z      the same with a factor |dinv_i| per term and gamma_(n+3): relative error e_rz1.
    beta       = fl(r.z'^ / r.z^): e_beta = (1 + e_rz1) (1 + u) / (1 - e_rz0) - 1.
    p          fl(z'^ + beta^ p^): dz = |dinv| dr + u |dinv| (|r'| + dr), then as for x with e_bp = (1 + e_beta) (1 + u) - 1.

    Each scalar's relative bound is gamma_n sum |terms| / |sum| plus what its terms inherit; a workgroup's partial dropped or taken twice moves r . z or
    r . r by a sixth and p . q by a 24th or a 370th of its terms, twelve and ten decades above these bounds, and alpha, beta carry it into every entry of
    x, r and p.  The elementwise bounds get a factor 1 + 2^-10 for the reference's own roundings (2^-64 each).'''
    from test_gpu_matrix_hip import product_bound
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    n = len(rhs)
    ld = numpy.longdouble
    dinv = numpy.where(free, 1 / ref.diagonal(), 0.) if jacobi else None
    r_in = numpy.where(free, rhs - ref @ start, 0.)
    dense = ref.toarray().astype(ld)
    rec = Recurrence(lambda y: dense @ y, free, None if dinv is None else dinv.astype(ld), start.astype(ld))
    rec.init(r_in.astype(ld))
    p0, rz0 = rec.p, rec.RZ_B
    rec.iterate(1)
    q, x1, r1, p1, rr1, rz1 = rec.q, rec.x, rec.r, rec.p, rec.RR, rec.RZ_B
    pq = p0 @ q
    alpha, beta = rz0 / pq, rz1 / rz0
    assert alpha > 0 and beta > 0 and rr1 > 0
    f = lambda a: numpy.abs(numpy.asarray(a, dtype=float))  # (bounds are float64: their own rounding is 1e-16 of them)
    absA = abs(ref)
    w = f(dinv) if jacobi else numpy.ones(n)
    up = U if jacobi else 0.
    dp = up * f(p0)
    e_rz0 = gamma(n + 3) * (f(r_in) * f(p0)).sum() / float(rz0)
    dq = numpy.where(free, product_bound(ref, f(p0)) + absA @ dp, 0.)
    e_pq = ((f(p0) * dq + dp * f(q) + dp * dq).sum() + gamma(n + 2) * ((f(p0) + dp) * (f(q) + dq)).sum()) / float(pq)
    e_alpha = (1 + e_rz0) * (1 + U) / (1 - e_pq) - 1
    e_ap = (1 + e_alpha) * (1 + up) - 1
    m = f(alpha * p0) * (1 + e_ap) * (1 + U)
    dx = f(alpha * p0) * e_ap + U * m + U * (f(start) + m)
    d_aq = float(alpha) * ((1 + e_alpha) * dq + e_alpha * f(q))
    t = (f(alpha * q) + d_aq) * (1 + U)
    dr = d_aq + U * t + U * (f(r_in) + t)
    d_rr = (2 * f(r1) * dr + dr ** 2).sum() + gamma(n + 2) * ((f(r1) + dr) ** 2).sum()
    e_rz1 = ((w * (2 * f(r1) * dr + dr ** 2)).sum() + gamma(n + 3) * (w * (f(r1) + dr) ** 2).sum()) / float(rz1)
    e_beta = (1 + e_rz1) * (1 + U) / (1 - e_rz0) - 1
    dz = w * dr + up * w * (f(r1) + dr)
    e_bp = (1 + e_beta) * (1 + up) - 1
    s = f(beta * p0) * (1 + e_bp) * (1 + U)
    dp1 = dz + f(beta * p0) * e_bp + U * s + U * (f(w * r1) + dz + s)
    slack = 1 + 2. ** -10
    print(f'one step, jacobi={jacobi}: relative bounds r.z {e_rz0:.1e}, p.q {e_pq:.1e}, alpha {e_alpha:.1e}, r.r {d_rr / float(rr1):.1e}, beta {e_beta:.1e}')
    assert max(e_rz0, e_pq, e_alpha, e_rz1, e_beta, d_rr / float(rr1)) < 1e-9  # (the bounds are sharp enough to see a partial go missing)
    return dict(r_in=r_in, dinv=dinv, x=(x1, dx * slack), r=(r1, dr * slack), p=(p1, dp1 * slack), q=(q, dq * slack), rr=(rr1, d_rr * slack))


@pytest.mark.parametrize('jacobi', [True, False], ids=['jacobi', 'plain'])
@pytest.mark.parametrize('narrow', [True, False], ids=['col32', 'col64'])
@pytest.mark.parametrize('lanes', [4, 64])
def test_one_iteration(lanes, narrow, jacobi):
    '''nh_cg_init and one nh_cg_iterate, called directly, against `one_step`: x, r, p, q and work[0] within the derived bounds; masked rows of x untouched, of
    r, p, q exactly zero; a repeat byte-identical.  Six vector workgroups (the last partial) and 24 or 370 product workgroups contribute partials.'''
    from nutils_amd import device, kernels
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    assert A.shape[0] == 1480 and A.lanes == 4 and 0 < (~free).sum() < 100
    expect = one_step(jacobi)
    values, rowptr, colidx = A.triplet()
    col32 = kernels.csr_compact(colidx, A.shape[1]) if narrow else None
    mask = device.to_dev(free, 'uint8')
    dinv = device.to_dev(expect['dinv'], 'float64') if jacobi else None

    def run():
        x, r = device.to_dev(start, 'float64'), device.to_dev(expect['r_in'], 'float64')
        p, q = device.empty(len(start), 'float64'), device.empty(len(start), 'float64')
        work = kernels.cg_work()
        kernels.cg_init(dinv, r, p, work)
        kernels.cg_iterate(values, rowptr, colidx, A.shape[1], rowmask=mask, dinv=dinv, x=x, r=r, p=p, q=q, work=work, niter=1, col32=col32, lanes=lanes)
        return dict(x=device.to_host(x), r=device.to_host(r), p=device.to_host(p), q=device.to_host(q), rr=device.to_host(work[:2]))

    got, again = run(), run()
    assert got['rr'][1] == 0  # no flag
    for name in 'qxrp':
        value, bound = expect[name]
        err = numpy.abs(got[name] - value).astype(float)
        print(f'{name}: max error / bound = {(err / numpy.maximum(bound, 1e-300)).max():.3f}')
        assert (err <= bound).all(), (name, (err / numpy.maximum(bound, 1e-300)).max())
    value, bound = expect['rr']
    print(f'r . r: error / bound = {abs(float(got["rr"][0] - value)) / bound:.3f}')
    assert abs(float(got['rr'][0] - value)) <= bound
    assert same_bytes(got['x'][~free], start[~free])
    for name in 'rpq':
        assert not got[name][~free].any()
    for name in got:
        assert same_bytes(got[name], again[name]), name


# ---- the solve contract where partials are summed and where the grids stride -----------------------------------------------

@pytest.mark.parametrize('lanes', [4, 64])
def test_many_workgroups(lanes):
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    A = with_lanes(A, lanes)
    for precon in ('diag', None):
        x, inits = solve(A, rhs, rtol=RTOL, precon=precon, **kwargs)  # (default maxiter: the free dofs)
        contract('wide', x)
        assert 0 < A.cg_iterations <= free.sum() and A.cg_iterations % 16 == 0
        assert same_bytes(solve(A, rhs, rtol=RTOL, precon=precon, **kwargs)[0], x)
        y, inits = solve(A, rhs, rtol=RTOL, precon=precon, check=1, **kwargs)
        contract('wide', y)
        it_ref, starts = reference_iterations('wide', precon)
        print(f'wide, lanes={lanes}, precon={precon}: {A.cg_iterations} iterations and {inits} starts on the device, {it_ref} and {starts} in numpy')
        # (the rule of test_gpu_bicgstab: another order of summation moves the count by an iteration or two, a lost preconditioner or a wrong beta by tens of percent)
        assert A.cg_iterations <= 1.1 * it_ref + 2
        assert same_bytes(x, y)  # the iterations that check=16 enqueues past convergence do nothing


def test_grid_caps():
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('tridiagonal')
    assert A.shape[0] > 1024 * 256
    B = with_lanes(A, 64)  # a row per wave: more than 2048 product workgroups' worth of rows
    assert A.shape[0] / (256 // B.lanes) > 2048
    for precon in ('diag', None):
        x, inits = solve(B, rhs, rtol=RTOL, precon=precon, **kwargs)
        contract('tridiagonal', x)
        assert same_bytes(solve(B, rhs, rtol=RTOL, precon=precon, **kwargs)[0], x)
        y, inits = solve(B, rhs, rtol=RTOL, precon=precon, check=1, **kwargs)
        contract('tridiagonal', y)
        it_ref, starts = reference_iterations('tridiagonal', precon)
        print(f'tridiagonal, precon={precon}: {B.cg_iterations} iterations and {inits} starts on the device, {it_ref} and {starts} in numpy')
        assert B.cg_iterations <= it_ref + 2


# ---- past convergence ------------------------------------------------------------------------------------------------------

def test_iterations_past_convergence():
    '''The diagonal family of test_cg_host: Jacobi-CG is there after one iteration, `check` enqueues 15 or 31 more, and whatever their trajectory through the
    subnormal range would have been, some of the 18 right-hand sides put r . z = 0 < r . r into it.  None may raise, and x is what one iteration left.'''
    d, b = diagonal_family()
    A = hip(scipy.sparse.diags(d, format='csr'))
    assert A.lanes == 1
    for check in (16, 32):
        for scale in SCALES:
            x, inits = solve(A, scale * b, rtol=RTOL, check=check)
            assert (A.cg_iterations, inits) == (check, 2)
            alpha = one_step_of_jacobi(x, scale * b, d)
        print(f'check={check}: alpha - 1 = {(alpha - 1) / U:+.0f} u')


@pytest.mark.parametrize('name', ['8I', 'powers of two'])
def test_exact_convergence(name):
    '''Systems on which an iteration is exact: r . r = 0 after the first, and the 15 that follow it must neither move x nor take p . q = 0 for a breakdown.
    With A = 8 I every product is a scaling by a power of two, with or without Jacobi (alpha = 1 or 1 / 8: r . z and p . q are the same sums up to that
    scaling, one row per thread in both kernels); so it is with Jacobi on a diagonal of powers of two.  WITHOUT a preconditioner that diagonal takes as many
    iterations as it has distinct entries and rounds in each (the restatement: 706127 u from b / d), so there the solve contract is what holds.'''
    n = 1480
    rng = numpy.random.default_rng(8)
    d = numpy.full(n, 8.) if name == '8I' else 2. ** rng.integers(-3, 4, n)
    b = rng.normal(size=n)
    A = hip(scipy.sparse.diags(d, format='csr'))
    for precon in ('diag', None):
        x, inits = solve(A, b, rtol=RTOL, precon=precon)  # (default maxiter and check)
        assert A.cg_iterations == 16
        if name == '8I' or precon:
            assert same_bytes(x, b / d) and inits == 2
        else:
            assert numpy.linalg.norm(b - d * x) <= RTOL * numpy.linalg.norm(b) * (1 + 1e-3)


def test_restart():
    '''the restart case of test_cg_host: the recurrence's residual is within rtol = 1e-13 when the true one is not, and the solve goes on from the true one'''
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('restart')
    for check in (16, 1):
        x, inits = solve(A, rhs, rtol=1e-13, precon=None, maxiter=10 * len(rhs), check=check, **kwargs)
        it_ref, starts = reference_iterations('restart', None, rtol=1e-13, maxiter=10 * len(rhs))
        print(f'restart, check={check}: {A.cg_iterations} iterations and {inits} starts on the device, {it_ref} and {starts} in numpy (check=1)')
        contract('restart', x, rtol=1e-13)


def test_maxiter_between_two_looks():
    from nutils_amd import matrix
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    with pytest.raises(matrix.ToleranceNotReached) as info:
        solve(A, rhs, rtol=RTOL, maxiter=21, check=16, **kwargs)
    best = info.value.best
    assert A.cg_iterations == 21
    assert numpy.isfinite(best).all() and numpy.array_equal(best[~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ best)[free])
    assert RTOL * r0 < res < r0  # 21 iterations got somewhere, not there
