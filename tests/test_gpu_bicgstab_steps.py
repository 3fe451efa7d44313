'''The device BiCGStab solve (matrix.HipMatrix.solve(solver='bicgstab'), nh_csr.hip) on the GPU step by step: one iteration against the restatement of
tests/test_bicgstab_host.py evaluated in longdouble, with derived bounds; three integer systems that break down in their second iteration, on which float64 is
exact, at the kernel level and through the restart of `solve`; the relays of the status as `solve` sees them: the same bytes for every `check`, a `maxiter`
that is no multiple of `check`, convergence at the half step, a non-finite residual.

Sizes: 1480 rows ('wide' of test_gpu_bicgstab, and the diagonal matrix) are six vector workgroups, the last one partial, and 24 product workgroups at 4 lanes per
row, 370 at 64; 1500 rows (500 tiles of 3) the same; 262 500 rows (87 500 tiles) are more than 1024 * 256, so the vector kernels stride, and at 64 lanes more
than 2048 product workgroups' worth, so the product strides and its epilogue accumulates.'''
import functools
import numpy
import pytest
import scipy.sparse

from test_bicgstab_host import Recurrence, bicgstab_solve_reference, tiled, BREAKDOWNS, CELLS
from test_gpu_bicgstab import problem, hip, solve, contract, gamma, RTOL, U

pytestmark = pytest.mark.gpu

VECTORS = 'x', 'r', 'rhat', 'p', 'v', 's', 't', 'phat', 'shat'


def same_bytes(a, b):
    return numpy.array_equal(a.view(numpy.int64), b.view(numpy.int64))


def with_lanes(A, lanes):
    B = A._with_values(A.triplet()[0])
    B.lanes = lanes
    return B


class Device:
    '''the vectors and the work array of a recurrence on the device, and the two entry points on them.  x and r are given; every other vector starts as NaN,
    so that an entry a kernel should have written and did not shows.  phat and shat exist only with a preconditioner.'''

    def __init__(self, csr, x, r, mask=None, dinv=None, col32=False, lanes=0):
        from nutils_amd import device, kernels
        self.values, self.rowptr, self.colidx = csr
        self.n = len(x)
        self.col32 = kernels.csr_compact(self.colidx, self.n) if col32 else None
        self.lanes = lanes
        self.mask = None if mask is None else device.to_dev(mask, 'uint8')
        self.dinv = None if dinv is None else device.to_dev(dinv, 'float64')
        self.vec = {name: device.to_dev(numpy.full(self.n, numpy.nan), 'float64') for name in VECTORS if self.dinv is not None or name not in ('phat', 'shat')}
        self.vec['x'], self.vec['r'] = device.to_dev(x, 'float64'), device.to_dev(r, 'float64')
        self.work = kernels.bicgstab_work()
        kernels.bicgstab_init(self.dinv, self.vec['r'], self.vec['rhat'], self.vec['p'], self.vec.get('phat'), self.work)

    def iterate(self, niter, stop_rr):
        from nutils_amd import kernels
        kernels.bicgstab_iterate(self.values, self.rowptr, self.colidx, self.n, rowmask=self.mask, dinv=self.dinv, phat=self.vec.get('phat'), shat=self.vec.get('shat'),
                                 work=self.work, stop_rr=stop_rr, niter=niter, col32=self.col32, lanes=self.lanes, **{name: self.vec[name] for name in VECTORS[:7]})

    def state(self):
        '''every vector and the named cells of the work array, on the host'''
        from nutils_amd import device
        return dict({name: device.to_host(y) for name, y in self.vec.items()}, work=device.to_host(self.work[:max(CELLS.values()) + 1]))


# ---- 2: one iteration against the restatement in longdouble --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def one_step(jacobi):
    '''Inputs of an iteration on 'wide' (x, r = mask(b - A x) and dinv as float64 vectors: the device gets the same bits), what nh_bicgstab_init and one
    nh_bicgstab_iterate make of them in longdouble, and how far float64 kernels may be from that.  With u = 2^-53, gamma_k = k u / (1 - k u), n = 1480, hats on
    what the device holds, w = |dinv| (1 without a preconditioner, and then phat = p, shat = s and the roundings marked [J] do not happen); every bound is
    evaluated on the reference's values.  dot(a, da, b, db) bounds the error of a sum of n products a^_i b^_i in any order, fused or not, against a . b:
    sum (|a| db + da |b| + da db) + gamma_(n+2) sum (|a| + da) (|b| + db).  A scaled vector c^ y^ with a relative bound e_c on c and dy on y is within
    scaled(c, e_c, y, dy) = |c| ((1 + e_c) dy + e_c |y|) of c y before it is rounded.

    init       rhat = p = r, exactly.  phat^ = fl(dinv r) [J]: dphat = u |phat|.  rho^ = r . r, a sum of n squares: e_rho0 = gamma_(n+2).
    product 1  v^ = mask(A phat^): dv = 2 gamma_(len+1) |A| (|phat| + dphat) (product_bound of test_gpu_matrix_hip: the sum of a row in any order) + |A| dphat.
    rhat . v   d_rv = dot(rhat, 0, v, dv), e_rv = d_rv / |rhat . v|.
    alpha      = fl(rho^ / rv^): e_alpha = (1 + e_rho0) (1 + u) / (1 - e_rv) - 1.
    s          = fl(r - alpha^ v^): the error of the product, one rounding of it (none if fused) and one of the difference:
               d_av = scaled(alpha, e_alpha, v, dv), m = (|alpha v| + d_av) (1 + u), ds = d_av + u m + u (|r| + m).
    shat       = fl(dinv s^) [J]: dshat = w ds + u w (|s| + ds).
    product 2  t^ = mask(A shat^): dt = 2 gamma_(len+1) |A| (|shat| + dshat) + |A| dshat.
    t.s, t.t   d_ts = dot(t, dt, s, ds), d_tt = dot(t, dt, t, dt), relative e_ts, e_tt.
    omega      = fl(ts^ / tt^): e_omega = (1 + e_ts) (1 + u) / (1 - e_tt) - 1.
    x          = fl(x + fl(alpha^ phat^ + omega^ shat^)): the errors of the two products, a rounding of each (of at most one if fused), one of their sum and one
               of the sum with x: d1 = scaled(alpha, e_alpha, phat, dphat), d2 = scaled(omega, e_omega, shat, dshat), m1 = (|alpha phat| + d1) (1 + u),
               m2 = (|omega shat| + d2) (1 + u), m = (m1 + m2) (1 + u), dx = d1 + d2 + 2 u (m1 + m2) + u (|x| + m).
    r'         = fl(s^ - omega^ t^): d_ot = scaled(omega, e_omega, t, dt), m = (|omega t| + d_ot) (1 + u), dr = ds + d_ot + u m + u (|s| + ds + m).
    r' . r'    d_rr = dot(r', dr, r', dr): this is work[0].  rho' = rhat . r': d_rho1 = dot(rhat, 0, r', dr), relative e_rho1.
    beta       = fl(fl(rho'^ / rho^) fl(alpha^ / omega^)): e_beta = (1 + e_rho1) (1 + u) / (1 - e_rho0) (1 + e_alpha) (1 + u) / (1 - e_omega) (1 + u) - 1.
    p'         = fl(r'^ + beta^ fl(p - omega^ v^)), p = r exactly: d_ov = scaled(omega, e_omega, v, dv), m = (|omega v| + d_ov) (1 + u),
               dg = d_ov + u m + u (|p| + m) for g = p - omega v; d_bg = scaled(beta, e_beta, g, dg), m = (|beta g| + d_bg) (1 + u),
               dp' = dr + d_bg + u m + u (|r'| + dr + m).
    phat'      = fl(dinv p'^) [J]: dphat' = w dp' + u w (|p'| + dp').

    Each scalar's relative bound is gamma_n sum |terms| / |sum| plus what its terms inherit; a workgroup's partial dropped or taken twice moves r . r, rhat . r
    by a sixth and rhat . v, t . s, t . t by a 24th or a 370th of their terms, many decades above these bounds, and alpha, omega, beta carry it into every entry
    of s, t, x, r and p.  The elementwise bounds get a factor 1 + 2^-10 for the reference's own roundings (2^-64 each).'''
    from test_gpu_matrix_hip import product_bound
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('wide')
    n = len(rhs)
    ld = numpy.longdouble
    dinv = numpy.where(free, 1 / ref.diagonal(), 0.) if jacobi else None
    r_in = numpy.where(free, rhs - ref @ start, 0.)
    stop_rr = (RTOL * r0) ** 2
    dense = ref.toarray().astype(ld)
    rec = Recurrence(lambda y: dense @ y, free, None if dinv is None else dinv.astype(ld), start.astype(ld))
    rec.init(r_in.astype(ld))
    phat0, rho0 = rec.phat, rec.RHO
    rec.iterate(1, ld(stop_rr))
    assert (rec.ST, rec.FLAG, rec.COUNT) == (0, False, 1)
    v, s, shat, t, x1, r1, p1, phat1 = rec.v, rec.s, rec.shat, rec.t, rec.x, rec.r, rec.p, rec.phat
    alpha, omega, rho1, rr1 = rec.ALPHA, rec.OMEGA, rec.RHO, rec.RR
    rv, ts, tt = rho0 / alpha, rec.WY, rec.YY
    beta = (rho1 / rho0) * (alpha / omega)
    f = lambda a: numpy.abs(numpy.asarray(a, dtype=float))  # (bounds are float64: their own rounding is 1e-16 of them)
    absA = abs(ref)
    w = f(dinv) if jacobi else numpy.ones(n)
    up = U if jacobi else 0.
    g2 = gamma(n + 2)
    dot = lambda a, da, b, db: (a * db + da * b + da * db).sum() + g2 * ((a + da) * (b + db)).sum()
    scaled = lambda c, e_c, y, dy: float(abs(c)) * ((1 + e_c) * dy + e_c * y)
    product = lambda y, dy: numpy.where(free, product_bound(ref, y + dy) + absA @ dy, 0.)
    r_, v_, s_, t_, phat_, shat_ = f(r_in), f(v), f(s), f(t), f(phat0), f(shat)
    zero = numpy.zeros(n)
    dphat = up * phat_
    e_rho0 = g2
    dv = product(phat_, dphat)
    e_rv = dot(r_, zero, v_, dv) / float(abs(rv))
    e_alpha = (1 + e_rho0) * (1 + U) / (1 - e_rv) - 1
    d_av = scaled(alpha, e_alpha, v_, dv)
    m = (f(alpha * v) + d_av) * (1 + U)
    ds = d_av + U * m + U * (r_ + m)
    dshat = w * ds + up * w * (s_ + ds)
    dt = product(shat_, dshat)
    e_ts = dot(t_, dt, s_, ds) / float(abs(ts))
    e_tt = dot(t_, dt, t_, dt) / float(tt)
    e_omega = (1 + e_ts) * (1 + U) / (1 - e_tt) - 1
    d1, d2 = scaled(alpha, e_alpha, phat_, dphat), scaled(omega, e_omega, shat_, dshat)
    m1, m2 = (f(alpha * phat0) + d1) * (1 + U), (f(omega * shat) + d2) * (1 + U)
    dx = d1 + d2 + 2 * U * (m1 + m2) + U * (f(start) + (m1 + m2) * (1 + U))
    d_ot = scaled(omega, e_omega, t_, dt)
    m = (f(omega * t) + d_ot) * (1 + U)
    dr = ds + d_ot + U * m + U * (s_ + ds + m)
    d_rr = dot(f(r1), dr, f(r1), dr)
    e_rho1 = dot(r_, zero, f(r1), dr) / float(abs(rho1))
    e_beta = (1 + e_rho1) * (1 + U) / (1 - e_rho0) * (1 + e_alpha) * (1 + U) / (1 - e_omega) * (1 + U) - 1
    d_ov = scaled(omega, e_omega, v_, dv)
    m = (f(omega * v) + d_ov) * (1 + U)
    dg = d_ov + U * m + U * (r_ + m)
    g_ = f(r_in.astype(ld) - omega * v)
    d_bg = scaled(beta, e_beta, g_, dg)
    m = (f(beta) * g_ + d_bg) * (1 + U)
    dp1 = dr + d_bg + U * m + U * (f(r1) + dr + m)
    dphat1 = w * dp1 + up * w * (f(p1) + dp1)
    slack = 1 + 2. ** -10
    relative = dict(zip(('rho', 'rhat.v', 'alpha', 't.s', 't.t', 'omega', 'r.r', "rho'", 'beta'), (e_rho0, e_rv, e_alpha, e_ts, e_tt, e_omega, d_rr / float(rr1), e_rho1, e_beta)))
    print(f'one step, jacobi={jacobi}: relative bounds ' + ', '.join(f'{name} {e:.1e}' for name, e in relative.items()))
    assert max(relative.values()) < 1e-9, relative  # (the bounds are sharp enough to see a partial go missing)
    expect = dict(v=(v, dv), s=(s, ds), t=(t, dt), x=(x1, dx), r=(r1, dr), p=(p1, dp1), rhat=(r_in.astype(ld), zero))
    if jacobi:
        expect.update(shat=(shat, dshat), phat=(phat1, dphat1))
    scalars = dict(RR=(rr1, d_rr), RHO=(rho1, e_rho1 * float(abs(rho1))), RHO_OLD=(rho0, e_rho0 * float(rho0)), ALPHA=(alpha, e_alpha * float(abs(alpha))),
                   OMEGA=(omega, e_omega * float(abs(omega))))
    return dict(r_in=r_in, dinv=dinv, stop_rr=stop_rr, vectors={name: (value, bound * slack) for name, (value, bound) in expect.items()},
                scalars={name: (value, bound * slack) for name, (value, bound) in scalars.items()})


@pytest.mark.parametrize('jacobi', [True, False], ids=['jacobi', 'plain'])
@pytest.mark.parametrize('narrow', [True, False], ids=['col32', 'col64'])
@pytest.mark.parametrize('lanes', [4, 64])
def test_one_iteration(lanes, narrow, jacobi):
    '''nh_bicgstab_init and one nh_bicgstab_iterate, called directly, against `one_step`: v, s, t, x, r, p (with Jacobi also phat and shat), work[0] and the
    cells RHO, RHO_OLD, ALPHA, OMEGA within the derived bounds; masked rows of x untouched, of every other vector exactly zero; no flag, one iteration counted; a
    repeat byte-identical.  Six vector workgroups (the last partial) and 24 or 370 product workgroups contribute partials.'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('wide')
    assert A.shape[0] == 1480 and A.lanes == 4 and 0 < (~free).sum() < 100
    expect = one_step(jacobi)

    def run():
        dev = Device(A.triplet(), start, expect['r_in'], mask=free, dinv=expect['dinv'], col32=narrow, lanes=lanes)
        dev.iterate(1, expect['stop_rr'])
        return dev.state()

    got, again = run(), run()
    assert set(got) == set(expect['vectors']) | {'work'}
    assert got['work'][CELLS['FLAG']] == 0 and got['work'][CELLS['COUNT']] == 1
    for name, (value, bound) in expect['vectors'].items():
        err = numpy.abs(got[name] - value).astype(float)
        print(f'{name}: max error / bound = {(err / numpy.maximum(bound, 1e-300)).max():.3f}')
        assert (err <= bound).all(), (name, (err / numpy.maximum(bound, 1e-300)).max())
    for name, (value, bound) in expect['scalars'].items():
        err = abs(float(got['work'][CELLS[name]] - value))
        print(f'{name}: error / bound = {err / bound:.3f}')
        assert err <= bound, (name, err / bound)
    assert same_bytes(got['x'][~free], start[~free])
    for name in VECTORS[1:]:
        if name in got:
            assert not got[name][~free].any(), name  # (NaN where a kernel left a masked row unwritten)
    for name in got:
        assert same_bytes(got[name], again[name]), name


# ---- 3: a breakdown after progress, exactly -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiles(name, N):
    '''(the tiled system of a case of BREAKDOWNS as device CSR tensors, its host twin, b, x and r at the breakdown, r . r of one tile).  Made once, never
    written.'''
    from nutils_amd import device
    K, b, x, r = tiled(name, N)
    csr = device.to_dev(K.data, 'float64'), device.to_dev(K.indptr, 'int64'), device.to_dev(K.indices, 'int64')
    return csr, K, b, x, r, float(numpy.dot(BREAKDOWNS[name][3], BREAKDOWNS[name][3]))


def breakdown(name, N, lanes, constrained=None):
    '''five iterations enqueued in one call from x = 0 (2.5 on constrained rows): the flag after one iteration that moved x, x and r those of the table byte for
    byte, r . r the number of free tiles times that of a tile; three more iterations change no byte of x, r, p or work[:3]'''
    csr, K, b, x_at, r_at, rr = tiles(name, N)
    free = numpy.ones(3 * N, dtype=bool) if constrained is None else ~constrained
    x0 = numpy.where(free, 0., 2.5)
    dev = Device(csr, x0, numpy.where(free, b, 0.), mask=None if constrained is None else free, lanes=lanes)
    stop_rr = 1e-20 * rr * N
    dev.iterate(5, stop_rr)
    got = dev.state()
    assert got['work'][:3].tolist() == [rr * free.sum() / 3, 1., 1.], got['work'][:3]
    assert same_bytes(got['x'], numpy.where(free, x_at, 2.5))
    assert same_bytes(got['r'], numpy.where(free, r_at, 0.))
    dev.iterate(3, stop_rr)
    after = dev.state()
    for key in 'x', 'r', 'p':
        assert same_bytes(got[key], after[key]), key
    assert same_bytes(got['work'][:3], after['work'][:3])


@pytest.mark.parametrize('lanes', [4, 64])
@pytest.mark.parametrize('name', list(BREAKDOWNS))
def test_breakdown_after_progress(name, lanes):
    breakdown(name, 500, lanes)


@pytest.mark.parametrize('name', list(BREAKDOWNS))
def test_breakdown_after_progress_on_strided_grids(name):
    N = 87500
    assert 3 * N > 1024 * 256 and 3 * N / (256 // 64) > 2048
    breakdown(name, N, 64)


@pytest.mark.parametrize('name', list(BREAKDOWNS))
def test_breakdown_after_progress_with_constrained_tiles(name):
    constrained = numpy.repeat(numpy.arange(500) % 7 == 0, 3)
    assert constrained.sum() == 3 * 72
    breakdown(name, 500, 4, constrained)


# ---- 4: the restart, through solve -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(BREAKDOWNS))
def test_restart_after_a_breakdown(name):
    '''The breakdown in the second iteration raises nothing: `solve` starts again from the true residual at the x the first iteration left, and meets its
    contract.  The restarted recurrence terminates in the 3-dimensional Krylov space of a tile; its count may move by an iteration under another order of
    summation, so it is printed beside the restatement's, not compared.'''
    from nutils_amd import _lib
    N = 500
    csr, K, b, x_at, r_at, rr = tiles(name, N)
    A = hip(K)
    block = numpy.array(BREAKDOWNS[name][0], dtype=float)
    direct = numpy.tile(numpy.linalg.solve(block, numpy.array(BREAKDOWNS[name][1], dtype=float)), N)
    smin = numpy.linalg.svd(block, compute_uv=False)[-1]
    r0 = numpy.linalg.norm(b)

    def run():
        with _lib.trace() as calls:
            x = A.solve(b, solver='bicgstab', precon=None, rtol=RTOL)
        assert 'nh_bicgstab_iterate' in calls and A._hostcsr is None
        return x, A.iterations, calls.count('nh_bicgstab_init')

    x, iterations, starts = run()
    y, it_ref, starts_ref, outcome = bicgstab_solve_reference(K, b, numpy.zeros(3 * N), numpy.ones(3 * N, dtype=bool), None, (RTOL * r0) ** 2, 3 * N)
    res = numpy.linalg.norm(b - K @ x)
    print(f'{name}: {iterations} iterations and {starts} starts on the device, {it_ref} and {starts_ref} in numpy ({outcome}); |r| / |r0| = {res / r0:.3e}, '
          f'|x - x_direct| = {numpy.linalg.norm(x - direct):.3e}, bound {res / smin:.3e}')
    assert starts >= 2
    assert res <= RTOL * r0 * (1 + 1e-3)
    assert numpy.linalg.norm(x - direct) <= res / smin
    assert iterations > 1
    again, iterations_again, starts_again = run()
    assert same_bytes(again, x) and (iterations_again, starts_again) == (iterations, starts)


# ---- 5: the relays seen from solve -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precon', ['diag', None])
def test_same_bytes_for_any_check(precon):
    '''the iteration stops itself on the device: the iterations that `check` enqueues past convergence move nothing and count nothing'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('wide')
    results = []
    for check in (1, 5, 16):
        x = solve(A, rhs, rtol=RTOL, precon=precon, check=check, **kwargs)
        results.append((x, A.iterations))
    contract('wide', results[0][0])
    print(f'wide, precon={precon}: iterations {[it for x, it in results]} for check = 1, 5, 16')
    for x, it in results[1:]:
        assert it == results[0][1] and same_bytes(x, results[0][0])


def test_maxiter_between_two_looks():
    from nutils_amd import matrix
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('wide')
    best = []
    for check in (16, 1):
        with pytest.raises(matrix.ToleranceNotReached) as info:
            solve(A, rhs, rtol=RTOL, maxiter=21, check=check, **kwargs)
        assert A.iterations == 21
        best.append(info.value.best)
    assert same_bytes(best[0], best[1])
    assert numpy.isfinite(best[0]).all() and numpy.array_equal(best[0][~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ best[0])[free])
    assert RTOL * r0 < res < r0  # 21 iterations got somewhere, not there


@pytest.mark.parametrize('lanes', [4, 64])
def test_half_step_convergence(lanes):
    '''A diagonal matrix of powers of two with both signs, an integer right-hand side, Jacobi: phat = b / d, v = b, rhat . v and rho are the same integer in any
    order of summation, alpha = 1, s = 0, t = 0, and t . t = 0 with s . s within the bound is convergence at the half step: x = 0 + 1 (b / d), one
    iteration.  Byte for byte x is 0. + b / d, NOT b / d: where b_i = 0 and d_i < 0 the quotient is -0., and the sum of x_i = +0. and alpha phat_i = -0. is +0.
    in correct arithmetic (round to nearest).  Everywhere else the two have the same bytes, and everywhere the same value.'''
    n = 1480
    rng = numpy.random.default_rng(12)
    d = rng.choice([-1., 1.], n) * 2. ** rng.integers(-3, 4, n)
    b = rng.integers(-4, 5, n).astype(float)
    assert (d > 0).any() and (d < 0).any() and b.any() and set(numpy.log2(numpy.abs(d))) == set(range(-3, 4))
    assert ((b == 0) & (d < 0)).any()  # (the entries on which b / d itself is -0.)
    A = with_lanes(hip(scipy.sparse.diags(d, format='csr')), lanes)
    x = solve(A, b, rtol=1e-12, precon='diag')
    assert A.iterations == 1
    assert numpy.array_equal(x, b / d) and same_bytes(x, 0. + b / d)
    assert same_bytes(x[b != 0], (b / d)[b != 0])


def test_non_finite_residual():
    from nutils_amd import matrix
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('wide')
    bad = rhs.copy()
    bad[numpy.flatnonzero(free)[700]] = numpy.inf
    with pytest.raises(matrix.MatrixError, match='bicgstab: non-finite residual'):
        solve(A, bad, iterated=False, rtol=RTOL, **kwargs)
    assert A.iterations == 0
    contract('wide', solve(A, rhs, rtol=RTOL, **kwargs))  # the matrix is usable afterwards
