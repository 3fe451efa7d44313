'''The device MINRES solve for symmetric indefinite matrices (matrix.HipMatrix.solve(solver='minres'), nh_csr.hip) on the GPU: the solve contract from one
vector workgroup to strided grids, iteration counts against the numpy restatement of tests/test_minres_host.py, one iteration (the first, and the third, where
the r1 term and both old w vectors are live) against that restatement evaluated in longdouble with derived bounds, the stop, and the stopping rules.

Sizes: 128 rows (block(8, 8)) and 160 (the saddle point) stay inside one vector workgroup; 1458 rows (block(27, 27)) are six vector workgroups, the last one
partial, and 23 product workgroups at 4 lanes per row, 365 at 64; 262 445 rows (odd) are more than 1024 * 256, so the vector kernels stride, and at 64
lanes more than 2048 product workgroups' worth, so the product strides and its epilogue accumulates.'''
import copy
import functools
import numpy
import pytest
import scipy.linalg
import scipy.sparse

from test_minres_host import Recurrence, minres_solve_reference, block, tridiagonal, saddle, CELLS
from test_gpu_bicgstab import hip, gamma, U

pytestmark = pytest.mark.gpu

RTOL = 1e-10
NAMES = 'block8', 'block27', 'tridiagonal', 'saddle'
PRECONS = {name: ('diag', None) if name != 'saddle' else (None,) for name in NAMES}
VECTORS = 'x', 'r', 'r1', 'r2', 'v', 'q', 'w1', 'w2'
RRP = 32 + 2 * 2048 + 1024  # where the partials of r . r start in the work array (M_RRP of nh_csr.hip)


def same_bytes(a, b):
    return numpy.array_equal(a.view(numpy.int64), b.view(numpy.int64))


def solve(A, rhs=None, iterated=True, **kwargs):
    '''A.solve(solver='minres') that insists on the device route'''
    from nutils_amd import _lib
    with _lib.trace() as calls:
        try:
            return A.solve(rhs, solver='minres', **kwargs)
        finally:
            assert 'nh_minres_init' in calls and (('nh_minres_iterate' in calls) == iterated), calls
            assert A._hostcsr is None  # neither values nor indices went to the host


def with_lanes(A, lanes):
    B = A._with_values(A.triplet()[0])
    B.lanes = lanes
    return B


@functools.lru_cache(maxsize=None)
def host_problem(name):
    '''(the host matrix, the solve's keywords, the right-hand side, the free mask, the start vector, |r0|, and for the small ones the direct solution and the
    smallest singular value of the free block).  Made once, never written.'''
    from nutils_amd import matrix
    ref, cons, rhs = tridiagonal() if name == 'tridiagonal' else saddle() if name == 'saddle' else block(*{'block8': (8, 8), 'block27': (27, 27)}[name])
    assert abs(ref - ref.T).max() == 0
    kwargs = dict(constrain=cons)
    free, start = matrix.constraints(ref.shape[1], cons)
    r0 = numpy.linalg.norm((rhs - ref @ start)[free])
    direct = smin = None
    if ref.shape[0] < 2000:
        direct = matrix.ScipyMatrix(ref).solve(rhs, **kwargs)
        dense = ref.toarray()[free][:, free]
        smin = numpy.linalg.svd(dense, compute_uv=False)[-1]
        assert smin > 1e-3 and (numpy.linalg.eigvalsh(dense) < 0).sum() >= 30  # nonsingular, and indefinite
    return ref, kwargs, rhs, free, start, r0, direct, smin


@functools.lru_cache(maxsize=None)
def problem(name):
    '''the matrix on the device, and `host_problem`'''
    A = hip(host_problem(name)[0])
    assert A._hostcsr is None
    return (A,) + host_problem(name)


def jacobi(ref, free):
    return numpy.where(free, 1 / numpy.abs(numpy.where(free, ref.diagonal(), 1.)), 0.)


@functools.lru_cache(maxsize=None)
def reference_iterations(name, precon):
    '''iterations the numpy restatement, host loop included, needs to the bound of the tests'''
    ref, kwargs, rhs, free, start, r0, direct, smin = host_problem(name)
    x, it, starts, outcome = minres_solve_reference(ref, rhs, start, free, jacobi(ref, free) if precon else None, (RTOL * r0) ** 2, int(free.sum()))
    assert outcome == 'converged' and numpy.linalg.norm((rhs - ref @ x)[free]) <= RTOL * r0
    return it


def contract(name, x):
    '''what a solve to RTOL promises: constrained dofs exactly, the true residual within the bound, the error within residual / sigma_min'''
    ref, kwargs, rhs, free, start, r0, direct, smin = host_problem(name)
    assert isinstance(x, numpy.ndarray) and numpy.array_equal(x[~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ x)[free])
    print(f'{name}: |r| / |r0| = {res / r0:.3e}' + ('' if direct is None else f', |x - x_direct| = {numpy.linalg.norm(x - direct):.3e}, bound {res / smin:.3e}'))
    assert res <= RTOL * r0 * (1 + 1e-3)
    if direct is not None:
        assert numpy.linalg.norm(x - direct) <= res / smin
    return res


# ---- 1: the solve contract from one workgroup to strided grids, and the counts -----------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_solve_contract(name):
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem(name)
    assert A.shape[0] == {'block8': 128, 'block27': 1458, 'tridiagonal': 262445, 'saddle': 160}[name]
    if name == 'tridiagonal':
        assert A.shape[0] % 2 and A.shape[0] > 1024 * 256
    for precon in PRECONS[name]:
        x = solve(A, rhs, rtol=RTOL, precon=precon, **kwargs)  # (default maxiter: the free dofs)
        contract(name, x)
        assert 0 < A.iterations <= free.sum()
        iterations = A.iterations
        it_ref = reference_iterations(name, precon)
        print(f'{name}, precon={precon}: {iterations} iterations on the device, {it_ref} in numpy')
        assert abs(iterations - it_ref) <= 2  # (the two differ in the order of their sums)
        assert same_bytes(solve(A, rhs, rtol=RTOL, precon=precon, **kwargs), x) and A.iterations == iterations  # bit-identical
        # every look at the device after one iteration: the iteration stops itself, so the same bytes and the same count
        assert same_bytes(solve(A, rhs, rtol=RTOL, precon=precon, check=1, **kwargs), x) and A.iterations == iterations
        # an absolute tolerance: the same contract (atol = RTOL r0 is the bound of rtol = RTOL up to the rounding of r0)
        y = solve(A, rhs, atol=RTOL * r0, precon=precon, **kwargs)
        contract(name, y)
        assert abs(A.iterations - iterations) <= 1


@pytest.mark.parametrize('name', ['block27', 'tridiagonal'])
def test_wave_per_row_and_int64_columns(name):
    '''64 lanes per row (on the tridiagonal matrix more than 2048 product workgroups' worth of rows: the product strides), and the int64 column indices of the
    assembly, which are the same arithmetic as their int32 copy'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem(name)
    B = with_lanes(A, 64)
    assert name != 'tridiagonal' or A.shape[0] / (256 // B.lanes) > 2048
    x = solve(B, rhs, rtol=RTOL, **kwargs)
    contract(name, x)
    assert abs(B.iterations - reference_iterations(name, 'diag')) <= 2
    wide = with_lanes(A, 64)
    wide._columns = lambda: None  # (no narrowed copy: the kernels read the int64 indices)
    assert same_bytes(solve(wide, rhs, rtol=RTOL, **kwargs), x) and wide.iterations == B.iterations


# ---- 2: one iteration against the restatement in longdouble ----------------------------------------------------------------------

class Device:
    '''the vectors and the work array of a recurrence on the device, and the two entry points on them.  Started by nh_minres_init from x and r (every other
    vector NaN before, so that an entry a kernel should have written and did not shows), or from a given state of the restatement: its vectors and cells
    uploaded, r . r as one partial.'''

    def __init__(self, csr, n, mask=None, dinv=None, col32=False, lanes=0):
        from nutils_amd import device, kernels
        self.values, self.rowptr, self.colidx = csr
        self.n = n
        self.col32 = kernels.csr_compact(self.colidx, n) if col32 else None
        self.lanes = lanes
        self.mask = None if mask is None else device.to_dev(mask, 'uint8')
        self.dinv = None if dinv is None else device.to_dev(dinv, 'float64')

    def init(self, x, r):
        from nutils_amd import device, kernels
        self.vec = {name: device.to_dev(numpy.full(self.n, numpy.nan), 'float64') for name in VECTORS}
        self.vec['x'], self.vec['r'] = device.to_dev(x, 'float64'), device.to_dev(r, 'float64')
        self.work = kernels.minres_work()
        kernels.minres_init(self.dinv, *(self.vec[name] for name in ('r', 'r1', 'r2', 'v', 'w1', 'w2')), self.work)
        return self

    def upload(self, rec):
        from nutils_amd import device, kernels
        self.vec = {name: device.to_dev(numpy.asarray(getattr(rec, name), dtype=float), 'float64') for name in VECTORS}
        work = numpy.zeros(kernels.minres_work().numel())
        for name in ('ST', 'BETA', 'OLDB', 'DBAR', 'EPSLN', 'PHIBAR', 'CS', 'SN', 'COUNT_U', 'FLAG_U', 'RR', 'FLAG', 'COUNT'):
            work[CELLS[name]] = getattr(rec, name)
        work[RRP] = rec.RRP
        self.work = device.to_dev(work, 'float64')
        return self

    def iterate(self, niter, stop_rr):
        from nutils_amd import kernels
        kernels.minres_iterate(self.values, self.rowptr, self.colidx, self.n, rowmask=self.mask, dinv=self.dinv, work=self.work, stop_rr=stop_rr, niter=niter,
                               col32=self.col32, lanes=self.lanes, **self.vec)

    def state(self):
        '''every vector and the named cells of the work array, on the host'''
        from nutils_amd import device
        return dict({name: device.to_host(y) for name, y in self.vec.items()}, work=device.to_host(self.work[:max(CELLS.values()) + 1]))


def in_longdouble(rec, ref):
    '''a copy of a float64 recurrence that goes on in longdouble, on a dense product'''
    ld = numpy.longdouble
    dense = ref.toarray().astype(ld)
    new = copy.copy(rec)
    new.product = lambda y: dense @ y
    for name, value in vars(rec).items():
        if isinstance(value, numpy.ndarray) and value.dtype == float:
            setattr(new, name, value.astype(ld))
        elif isinstance(value, (float, numpy.floating)) and name not in ('ST', 'ST_L'):
            setattr(new, name, ld(value))
    return new


@functools.lru_cache(maxsize=None)
def one_step(third, precon):
    '''One iteration on block(27, 27) in longdouble, and how far float64 kernels may be from it.  The first step (third = False) starts from what nh_minres_init
    makes of x and r = mask(b - A x); the third from the state of the float64 restatement after two steps, uploaded, so that its inputs are exact.  With u =
    2^-53, gamma_k = k u / (1 - k u), n = 1458, hats on what the device holds, w = dinv (1 without a preconditioner, and then the roundings marked [J] do not
    happen); every bound is evaluated on the reference's values.  dot(a, da, b, db) bounds the error of a sum of n products a^_i b^_i in any order, fused or
    not, against a . b: sum (|a| db + da |b| + da db) + gamma_(n+3) sum (|a| + da) (|b| + db).  A quotient fl(a^ / b^) with an absolute bound da and a relative
    one e_b is within (da / |b|) (1 + u) / (1 - e_b) + |a / b| ((1 + u) / (1 - e_b) - 1) of a / b: div(a, da, b, e_b).

    inputs     first step: beta = sqrt(r . w r), a sum of n terms of three factors: e_ry = gamma_(n+3), e_b = 1 / (sqrt(1 - e_ry) (1 - u)) - 1, phibar = beta;
               v^ = fl(fl(w r) [J] / beta^): dv = |v| ((1 + u)^2 / (1 - e_b) - 1).  Third step: e_b = 0, dv = 0.  r1, r2, r, w1, w2, x, cs, sn, dbar, epsln, oldb: exact.
    product    q^ = mask(A v^): dq = 2 gamma_(len+1) |A| (|v| + dv) (product_bound of test_gpu_matrix_hip) + |A| dv.
    alpha      = v^ . q^: d_alpha = dot(v, dv, q, dq), absolute (alpha may be small against its terms).
    r2'        = fl(q^ - c1^ r1 - c2^ r2), c1 = fl(beta^ / oldb): e_c1 = (1 + e_b) (1 + u) - 1, c2 = fl(alpha^ / beta^): d_c2 = div(alpha, d_alpha, beta, e_b);
               m1 = |c1 r1| (1 + e_c1) (1 + u), m2 = (|c2| + d_c2) |r2| (1 + u), the two products rounded (not if fused) and two differences:
               dy = dq + e_c1 |c1 r1| + d_c2 |r2| + u (m1 + m2) + 2 u (1 + u) (|q| + dq + m1 + m2).  r1' = r2, exactly.
    r2' . w r2'  d_ry = sum w (2 |y| dy + dy^2) + gamma_(n+3) sum w (|y| + dy)^2, e_ry = d_ry / ry; beta' = sqrt: e_bn = 1 / (sqrt(1 - e_ry) (1 - u)) - 1.
    rotation   delta = fl(cs dbar + sn alpha^): d_delta = |sn| d_alpha + 2 u (1 + u) (|cs dbar| + |sn| (|alpha| + d_alpha)); gbar = fl(sn dbar - cs alpha^) likewise;
               epsln' = fl(sn beta'^), dbar' = fl(-cs beta'^): relative (1 + e_bn) (1 + u) - 1.  gamma = hypot(gbar^, beta'^), a function with partial derivatives
               of at most 1, computed to 1 ulp = 2 u: d_gam = d_gbar + beta' e_bn, plus 2 u (gamma + that); e_gam = d_gam / gamma.  cs' = fl(gbar^ / gamma^):
               d_cs = div(gbar, d_gbar, gamma, e_gam); sn' = fl(beta'^ / gamma^): e_sn = (1 + e_bn) (1 + u) / (1 - e_gam) - 1.  phi = fl(cs'^ phibar^):
               d_phi = |phibar| (d_cs (1 + e_b) + |cs'| e_b), plus u (|phi| + that); phibar' = fl(sn'^ phibar^): e_pb = (1 + e_sn) (1 + e_b) (1 + u) - 1.
    w2'        = fl(fl(v^ - oldeps w1 - delta^ w2) / gamma^): t1 = |oldeps w1|, t2 = (|delta| + d_delta) |w2|, the numerator within
               dN = dv + d_delta |w2| + u (t1 + t2) + 2 u (1 + u) (|v| + dv + (t1 + t2) (1 + u)); dw = div(N, dN, gamma, e_gam).  w1' = w2, exactly.
    x'         = fl(x + fl(phi^ w2'^)): d = d_phi (|w| + dw) + |phi| dw, m = (|phi w| + d) (1 + u), dx = d + u m + u (|x| + m).
    r'         = fl(fl(s2^ r) - fl(c3^ r2'^)), s2 = fl(sn'^ sn'^): e_s2 = (1 + e_sn)^2 (1 + u) - 1; pc = fl(phibar'^ cs'^): d_pc = |phibar'| ((1 + e_pb) d_cs + e_pb |cs'|),
               plus u (|pc| + that); c3 = fl(pc^ / beta'^): d_c3 = div(pc, d_pc, beta', e_bn).  d1 = e_s2 |s2 r|, m1 = |s2 r| (1 + e_s2) (1 + u),
               d2 = d_c3 (|y| + dy) + |c3| dy, m2 = (|c3 y| + d2) (1 + u), dr = d1 + d2 + 2 u (m1 + m2).  r' . r' is work[0]: d_rr = dot(r', dr, r', dr).
    v'         = fl(fl(w r2'^) [J] / beta'^): dt = w dy + u w (|y| + dy) [J], dv' = div(t, dt, beta', e_bn).

    A workgroup's partial dropped or taken twice moves r2 . w r2 and r . r by a sixth and v . q by a 23rd or a 365th of their terms, many decades above these
    bounds, and alpha, beta' and the rotation carry it into every entry of r2, w2, x, r and v.  The elementwise bounds get a factor 1 + 2^-10 for the
    reference's own roundings (2^-64 each).'''
    from test_gpu_matrix_hip import product_bound
    ref, kwargs, rhs, free, start, r0, direct, smin = host_problem('block27')
    n = len(rhs)
    ld = numpy.longdouble
    dinv = jacobi(ref, free) if precon else None
    r_in = numpy.where(free, rhs - ref @ start, 0.)
    stop_rr = (RTOL * r0) ** 2
    f = lambda a: numpy.abs(numpy.asarray(a, dtype=float))  # (bounds are float64: their own rounding is 1e-16 of them)
    g3 = gamma(n + 3)
    w = f(dinv) if precon else numpy.ones(n)
    up = U if precon else 0.
    if third:
        rec64 = Recurrence(lambda y: ref @ y, free, dinv, start)
        rec64.init(r_in)
        rec64.iterate(2, stop_rr)
        assert (rec64.ST, rec64.FLAG, rec64.COUNT) == (0, False, 2) and rec64.OLDB != 0 and rec64.w1.any() and rec64.w2.any()
        pre = in_longdouble(rec64, ref)
        upload, e_b, dv = rec64, 0., numpy.zeros(n)
    else:
        dense = ref.toarray().astype(ld)
        pre = Recurrence(lambda y: dense @ y, free, None if dinv is None else dinv.astype(ld), start.astype(ld))
        pre.init(r_in.astype(ld))
        upload = None
        e_b = 1 / ((1 - g3) ** .5 * (1 - U)) - 1
        dv = f(pre.v) * ((1 + up) * (1 + U) / (1 - e_b) - 1)
    post = copy.copy(pre)
    post.iterate(1, ld(stop_rr))
    assert (post.ST, post.FLAG, post.COUNT) == (0, False, 3 if third else 1)
    dot = lambda a, da, b, db: (a * db + da * b + da * db).sum() + g3 * ((a + da) * (b + db)).sum()
    div = lambda a, da, b, e: da / abs(b) * (1 + U) / (1 - e) + abs(a / b) * ((1 + U) / (1 - e) - 1)
    absA = abs(ref)
    v_, r1_, r2_, w1_, w2_, x_, r_ = (f(getattr(pre, name)) for name in ('v', 'r1', 'r2', 'w1', 'w2', 'x', 'r'))
    beta, oldb, cs0, sn0, dbar0, eps0, phibar0 = (float(getattr(pre, name)) for name in ('BETA', 'OLDB', 'CS', 'SN', 'DBAR', 'EPSLN', 'PHIBAR'))
    q_, y_, wn_, rn_, vn_ = (f(getattr(post, name)) for name in ('q', 'r2', 'w2', 'r', 'v'))
    alpha, betan, cs1, sn1, phibar1, ry = (float(getattr(post, name)) for name in ('ALPHA', 'BETA', 'CS', 'SN', 'PHIBAR', 'RYP'))
    dq = numpy.where(free, product_bound(ref, v_ + dv) + absA @ dv, 0.)
    d_alpha = dot(v_, dv, q_, dq)
    c1, e_c1 = (beta / oldb, (1 + e_b) * (1 + U) - 1) if oldb else (0., 0.)
    c2, d_c2 = alpha / beta, div(alpha, d_alpha, beta, e_b)
    m1, m2 = abs(c1) * r1_ * (1 + e_c1) * (1 + U), (abs(c2) + d_c2) * r2_ * (1 + U)
    dy = dq + e_c1 * abs(c1) * r1_ + d_c2 * r2_ + U * (m1 + m2) + 2 * U * (1 + U) * (q_ + dq + m1 + m2)
    e_ry = ((w * (2 * y_ * dy + dy * dy)).sum() + g3 * (w * (y_ + dy) ** 2).sum()) / ry
    e_bn = 1 / ((1 - e_ry) ** .5 * (1 - U)) - 1
    delta, gbar = cs0 * dbar0 + sn0 * alpha, sn0 * dbar0 - cs0 * alpha
    d_delta = abs(sn0) * d_alpha + 2 * U * (1 + U) * (abs(cs0 * dbar0) + abs(sn0) * (abs(alpha) + d_alpha))
    d_gbar = abs(cs0) * d_alpha + 2 * U * (1 + U) * (abs(sn0 * dbar0) + abs(cs0) * (abs(alpha) + d_alpha))
    e_scaled = (1 + e_bn) * (1 + U) - 1
    gam = float(numpy.hypot(gbar, betan))
    d_gam = d_gbar + betan * e_bn
    d_gam += 2 * U * (gam + d_gam)
    e_gam = d_gam / gam
    d_cs = div(gbar, d_gbar, gam, e_gam)
    e_sn = (1 + e_bn) * (1 + U) / (1 - e_gam) - 1
    phi = cs1 * phibar0
    d_phi = abs(phibar0) * (d_cs * (1 + e_b) + abs(cs1) * e_b)
    d_phi += U * (abs(phi) + d_phi)
    e_pb = (1 + e_sn) * (1 + e_b) * (1 + U) - 1
    t1, t2 = abs(eps0) * w1_, (abs(delta) + d_delta) * w2_
    dN = dv + d_delta * w2_ + U * (t1 + t2) + 2 * U * (1 + U) * (v_ + dv + (t1 + t2) * (1 + U))
    dw = dN / gam * (1 + U) / (1 - e_gam) + wn_ * ((1 + U) / (1 - e_gam) - 1)
    d = d_phi * (wn_ + dw) + abs(phi) * dw
    m = (abs(phi) * wn_ + d) * (1 + U)
    dx = d + U * m + U * (x_ + m)
    s2, e_s2 = sn1 * sn1, (1 + e_sn) ** 2 * (1 + U) - 1
    pc = phibar1 * cs1
    d_pc = abs(phibar1) * ((1 + e_pb) * d_cs + e_pb * abs(cs1))
    d_pc += U * (abs(pc) + d_pc)
    c3, d_c3 = pc / betan, div(pc, d_pc, betan, e_bn)
    d1, d2 = e_s2 * s2 * r_, d_c3 * (y_ + dy) + abs(c3) * dy
    m1, m2 = s2 * r_ * (1 + e_s2) * (1 + U), (abs(c3) * y_ + d2) * (1 + U)
    dr = d1 + d2 + 2 * U * (m1 + m2)
    d_rr = dot(rn_, dr, rn_, dr)
    dt = w * dy + up * w * (y_ + dy)
    dvn = dt / betan * (1 + U) / (1 - e_bn) + vn_ * ((1 + U) / (1 - e_bn) - 1)
    slack = 1 + 2. ** -10
    relative = dict(zip(('beta', "beta'", 'gamma', "sn'", "phibar'", 'r.r'), (e_b, e_bn, e_gam, e_sn, e_pb, d_rr / float(post.RRP))))
    absolute = dict(zip(('alpha', 'delta', "cs'", 'phi'), (d_alpha / abs(beta), d_delta / abs(beta), d_cs, d_phi / abs(phibar0))))
    print(f'one step, third={third}, precon={precon}: relative bounds ' + ', '.join(f'{name} {e:.1e}' for name, e in relative.items()) + '; against their scale '
          + ', '.join(f'{name} {e:.1e}' for name, e in absolute.items()))
    assert max(relative.values()) < 1e-9 and max(absolute.values()) < 1e-9, (relative, absolute)  # (the bounds are sharp enough to see a partial go missing)
    zero = numpy.zeros(n)
    vectors = dict(q=(post.q, dq), r1=(pre.r2, zero), r2=(post.r2, dy), w1=(pre.w2, zero), w2=(post.w2, dw), x=(post.x, dx), r=(post.r, dr), v=(post.v, dvn))
    scalars = dict(RR=(post.RRP, d_rr), ALPHA=(post.ALPHA, d_alpha), BETA=(post.BETA, e_bn * betan), OLDB=(pre.BETA, e_b * abs(beta)), DBAR=(post.DBAR, e_scaled * abs(cs0 * betan)),
                   EPSLN=(post.EPSLN, e_scaled * abs(sn0 * betan)), PHIBAR=(post.PHIBAR, e_pb * abs(phibar1)), CS=(post.CS, d_cs), SN=(post.SN, e_sn * abs(sn1)))
    return dict(r_in=r_in, dinv=dinv, stop_rr=stop_rr, upload=upload, count=3 if third else 1,
                vectors={name: (value, bound * slack) for name, (value, bound) in vectors.items()},
                scalars={name: (value, float(bound) * slack) for name, (value, bound) in scalars.items()})


def check_step(got, expect, free, start):
    '''a state after one iteration against `one_step`; returns the largest error / bound'''
    worst = 0.
    assert set(got) == set(expect['vectors']) | {'work'}
    assert got['work'][CELLS['FLAG']] == 0 and got['work'][CELLS['COUNT']] == expect['count'] and got['work'][CELLS['ST']] == 0
    for name, (value, bound) in expect['vectors'].items():
        err = numpy.abs(got[name] - value).astype(float)
        ratio = (err / numpy.maximum(bound, 1e-300)).max()
        print(f'{name}: max error / bound = {ratio:.3f}')
        assert (err <= bound).all(), (name, ratio)
        worst = max(worst, ratio)
    for name, (value, bound) in expect['scalars'].items():
        err = abs(float(got['work'][CELLS[name]] - value))
        ratio = err / max(bound, 1e-300)
        print(f'{name}: error / bound = {ratio:.3f}')
        assert err <= bound, (name, ratio)
        worst = max(worst, ratio)
    assert same_bytes(got['x'][~free], start[~free])
    for name in VECTORS[1:]:
        assert not got[name][~free].any(), name  # (NaN where a kernel left a masked row unwritten)
    return worst


@pytest.mark.parametrize('precon', ['diag', None])
@pytest.mark.parametrize('narrow', [True, False], ids=['col32', 'col64'])
@pytest.mark.parametrize('lanes', [4, 64])
@pytest.mark.parametrize('third', [False, True], ids=['first', 'third'])
def test_one_iteration(third, lanes, narrow, precon):
    '''nh_minres_init and one nh_minres_iterate (the first step), or one nh_minres_iterate on the uploaded state of the restatement after two (the third step:
    the r1 term and both old w vectors are live), called directly, against `one_step`: q, r1, r2, w1, w2, x, r, v, work[0] and the cells ALPHA, BETA, OLDB,
    DBAR, EPSLN, PHIBAR, CS, SN within the derived bounds; masked rows of x untouched, of every other vector exactly zero; no flag, the count one up; a
    repeat byte-identical.  Six vector workgroups (the last partial) and 23 or 365 product workgroups contribute partials.'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('block27')
    assert A.shape[0] == 1458 and A.lanes == 4 and 0 < (~free).sum() < 200
    expect = one_step(third, precon)

    def run():
        dev = Device(A.triplet(), A.shape[0], mask=free, dinv=expect['dinv'], col32=narrow, lanes=lanes)
        dev = dev.upload(expect['upload']) if third else dev.init(start, expect['r_in'])
        dev.iterate(1, expect['stop_rr'])
        return dev.state()

    got, again = run(), run()
    check_step(got, expect, free, start)
    for name in got:
        assert same_bytes(got[name], again[name]), name


# ---- 3: the stop, and the stopping rules ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('precon', ['diag', None])
def test_steps_after_the_stop_move_nothing(precon):
    '''the iteration run to its stop at the kernel level, 16 steps at a time: r . r within the bound, the count that of `solve`; five steps more change no byte of
    x, r, r1, r2, v, w1, w2 and of work[0 .. 2] (the one product after the stop writes q alone)'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('block27')
    solve(A, rhs, rtol=RTOL, precon=precon, **kwargs)
    dev = Device(A.triplet(), A.shape[0], mask=free, dinv=jacobi(ref, free) if precon else None, col32=True, lanes=A.lanes)
    dev.init(start, numpy.where(free, rhs - ref @ start, 0.))
    stop_rr = (RTOL * r0) ** 2
    for _ in range(20):
        dev.iterate(16, stop_rr)
        got = dev.state()
        if got['work'][0] <= stop_rr:
            break
    rr, flag, count = got['work'][:3]
    assert rr <= stop_rr and not flag  # (the status cell is set by the step after the deciding one: with a count of 128 that step is in the next call)
    assert abs(count - A.iterations) <= 2  # (`solve` starts from the same residual up to the rounding of the product)
    dev.iterate(5, stop_rr)
    after = dev.state()
    for name in ('x', 'r', 'r1', 'r2', 'v', 'w1', 'w2'):
        assert same_bytes(got[name], after[name]), name
    assert same_bytes(got['work'][:3], after['work'][:3]) and after['work'][CELLS['ST']] == 1
    # the carried residual is the residual, by the bound of tests/test_minres_host.py: k gamma_16 (2 cond + 1) |r0|, times sqrt(max |d| / min |d|) with Jacobi
    d = numpy.abs(ref.diagonal()[free])
    bound = count * gamma(16) * (2 * abs(ref).sum(1).max() / smin + 1) * (numpy.sqrt(d.max() / d.min()) if precon else 1.) * r0
    gap = numpy.linalg.norm(got['r'] - numpy.where(free, rhs - ref @ got['x'], 0.))
    print(f'precon={precon}: {int(count)} iterations, |r - (b - A x)| = {gap / r0:.1e} |r0|, bound {bound / r0:.1e} |r0|')
    assert gap <= bound


def test_stops_at_maxiter():
    from nutils_amd import matrix
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('block27')
    best = []
    for check in (16, 1):
        with pytest.raises(matrix.ToleranceNotReached) as info:
            solve(A, rhs, rtol=RTOL, maxiter=5, check=check, **kwargs)
        assert A.iterations == 5
        best.append(info.value.best)
    assert same_bytes(best[0], best[1])
    assert numpy.isfinite(best[0]).all() and numpy.array_equal(best[0][~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ best[0])[free])
    assert RTOL * r0 < res < r0  # five iterations got somewhere, not there


def test_device_vectors_and_trivial_systems():
    from nutils_amd import device
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('block8')
    x = solve(A, device.to_dev(rhs, 'float64'), rtol=RTOL, **kwargs)
    assert x.is_cuda and same_bytes(device.to_host(x), solve(A, rhs, rtol=RTOL, **kwargs))
    # no right-hand side, no constraints: zero, without an iteration
    assert not solve(A, iterated=False, rtol=RTOL).any() and A.iterations == 0
    assert not solve(A, numpy.zeros(A.shape[0]), iterated=False, rtol=RTOL).any() and A.iterations == 0
    # a residual within the tolerance from the start: the initial vector comes back
    assert numpy.array_equal(solve(A, ref @ start, iterated=False, rtol=RTOL, atol=1e-9, **kwargs), start) and A.iterations == 0
    assert A.cg_iterations is None  # (no 'cg' solve was made on this matrix)


def test_refusals_on_the_device():
    from nutils_amd import matrix
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('saddle')
    with pytest.raises(matrix.MatrixError, match='zero entries'):
        A.solve(rhs, solver='minres', rtol=RTOL, precon='diag', **kwargs)
    assert A._hostcsr is None
    bad = rhs.copy()
    bad[numpy.flatnonzero(free)[70]] = numpy.inf
    with pytest.raises(matrix.MatrixError, match='minres: non-finite residual'):
        solve(A, bad, iterated=False, rtol=RTOL, precon=None, **kwargs)
    Z = hip(scipy.sparse.csr_matrix(([0., 0.], ([0, 1], [0, 1])), (2, 2)))
    with pytest.raises(matrix.MatrixError, match='minres: breakdown'):
        solve(Z, numpy.ones(2), rtol=RTOL, precon=None)  # gamma = 0 at the first step
    assert Z.iterations == 0
    D = hip([[1., 0.], [0., -1.]])
    x = solve(D, numpy.array([1., 1.]), rtol=1e-12, precon=None)  # v . A v = 0 at the first step is no breakdown of MINRES
    assert numpy.allclose(x, [1., -1.], rtol=1e-12, atol=0) and D.iterations == 2
    x = solve(D, numpy.array([0., 2.]), rtol=1e-12, precon=None)  # an eigenvector: the Krylov space is exhausted after one step, which is taken
    assert numpy.array_equal(x, [0., -2.]) and D.iterations == 1


def test_a_nonsymmetric_matrix_is_not_solved():
    '''symmetry is not checked: the recurrence converges to something the true residual rejects, and the solve says so'''
    from nutils_amd import matrix
    from test_bicgstab_host import skewed, laplace2d
    N = skewed(laplace2d(9, 7), 2.)
    A = hip(N)
    b = numpy.random.default_rng(3).normal(size=63)
    with pytest.raises(matrix.ToleranceNotReached) as info:
        solve(A, b, rtol=RTOL, precon=None, maxiter=40)
    assert A.iterations == 40 and numpy.isfinite(info.value.best).all()
    assert numpy.linalg.norm(b - N @ info.value.best) > 1e-6 * numpy.linalg.norm(b)


# ---- 4: a symmetric indefinite matrix straight from the front end -----------------------------------------------------------------

def test_helmholtz_through_the_front_end():
    from nutils_amd import function, matrix, mesh
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1, 10), numpy.linspace(0, 2, 8)])
    basis = domain.basis('std', degree=1)
    stiffness = function.outer(function.grad(basis, geom)).sum(-1) * function.J(geom)
    mass = function.outer(basis) * function.J(geom)
    cons = numpy.full((10, 8), numpy.nan)
    cons[0], cons[-1] = 1., -.5  # two sides held
    cons = cons.ravel()
    free = numpy.isnan(cons)
    csr = lambda itg: (lambda v, rp, ci: scipy.sparse.csr_matrix((v, ci, rp), (80, 80)))(*function.eval(function.as_csr(domain.integral(itg, degree=2))))
    Kh, Mh = csr(stiffness), csr(mass)
    lam = scipy.linalg.eigh(Kh.toarray()[free][:, free], Mh.toarray()[free][:, free], eigvals_only=True)
    k2 = float(lam[3] + lam[4]) / 2  # between two eigenvalues: four negative ones, none near zero
    A = function.eval(function.as_matrix(domain.integral(stiffness + (-k2) * mass, degree=2)))
    ref = scipy.sparse.csr_matrix(Kh - k2 * Mh)
    assert isinstance(A, matrix.HipMatrix) and A._hostcsr is None
    rhs = numpy.random.default_rng(5).normal(size=80)
    assert numpy.abs(A @ rhs - ref @ rhs).max() <= 1e-13 * numpy.abs(ref @ rhs).max() and A._hostcsr is None
    eig = numpy.linalg.eigvalsh(ref.toarray()[free][:, free])
    smin = numpy.abs(eig).min()
    assert (eig < 0).sum() == 4 and smin > 1e-3 * numpy.abs(eig).max()  # indefinite and nonsingular
    for precon in ('diag', None):
        x = solve(A, rhs, constrain=cons, rtol=RTOL, precon=precon)
        start = numpy.where(free, 0., cons)
        assert numpy.array_equal(x[~free], start[~free])
        res = numpy.linalg.norm((rhs - ref @ x)[free])
        assert res <= RTOL * numpy.linalg.norm((rhs - ref @ start)[free]) * (1 + 1e-3)
        direct = matrix.ScipyMatrix(ref).solve(rhs, constrain=cons)
        assert numpy.linalg.norm(x - direct) <= res / smin
