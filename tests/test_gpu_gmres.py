'''The device GMRES solve (matrix.HipMatrix.solve(solver='fgmres'), nh_csr.hip) on the GPU: the solve contract on the nonsymmetric matrices of
tests/test_gpu_bicgstab.py at three settings of `restart`, step counts against the numpy restatement of tests/test_gmres_host.py, the chunk of basis vectors
the Gram-Schmidt kernels take at a time, the orthogonality of the basis, one Arnoldi step against the restatement in longdouble with derived bounds, the
estimates within a cycle, the steps enqueued after a stop, and the stopping rules and errors of `solve`.

Sizes: 130 and 192 rows stay inside one vector workgroup; 1480 rows ('wide') are 740 pairs of doubles, three Gram-Schmidt workgroups with the last one partial
(six of the kernel that sums r . r), and 24 product workgroups at 4 lanes; 262 444 rows ('tridiagonal') are more than 512 * 256 pairs, so the Gram-Schmidt
kernels stride; 1001 rows have no pairs at all (an odd length: one double per load).'''
import functools
import numpy
import pytest
import scipy.sparse

from test_gmres_host import gmres_reference, Cycle, cells, CELLS, ST_DONE, ST_FULL
from test_gpu_bicgstab import problem, contract, hip, gamma, RTOL, U

pytestmark = pytest.mark.gpu

SMALL = 'laplace', 'elasticity', 'wide'


def same_bytes(a, b):
    return numpy.array_equal(a.view(numpy.int64), b.view(numpy.int64))


def solve(A, rhs=None, iterated=True, **kwargs):
    '''A.solve(solver='fgmres') that insists on the device route'''
    from nutils_amd import _lib
    with _lib.trace() as calls:
        try:
            return A.solve(rhs, solver='fgmres', **kwargs)
        finally:
            assert 'nh_gmres_init' in calls and ('nh_gmres_iterate' in calls) == iterated, calls
            assert A._hostcsr is None  # neither values nor indices went to the host


def jacobi(name, precon):
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem(name)
    return numpy.where(free, 1 / ref.diagonal(), 0.) if precon else None


@functools.lru_cache(maxsize=None)
def reference(name, precon, restart):
    '''(steps, x) of the numpy restatement to the bound of the tests'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem(name)
    x, it, outcome = gmres_reference(ref, rhs, start, free, jacobi(name, precon), (RTOL * r0) ** 2, restart, int(free.sum()))
    assert outcome == 'converged' and numpy.linalg.norm((rhs - ref @ x)[free]) <= RTOL * r0 * (1 + 1e-3)
    return it, x


# ---- the solve contract -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precon', ['diag', None], ids=['jacobi', 'plain'])
@pytest.mark.parametrize('name,restart', [(name, restart) for name in SMALL for restart in (5, 30, 'full')] + [('tridiagonal', 5), ('tridiagonal', 30)])
def test_solve_contract(name, restart, precon):
    '''constrained dofs exactly, the true residual within the bound, the error within residual / sigma_min; a second solve the same bytes; a look at the device
    after every step the same bytes and the same count'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem(name)
    nfree = int(free.sum())
    if restart == 'full':
        restart = nfree + 7  # (clipped to nfree: unrestarted)
    x = solve(A, rhs, rtol=RTOL, precon=precon, restart=restart, **kwargs)  # (default maxiter: the free dofs)
    contract(name, x)
    steps = A.iterations
    print(f'{name}, restart {restart}, precon {precon}: {steps} steps')
    assert 0 < steps <= nfree
    assert same_bytes(solve(A, rhs, rtol=RTOL, precon=precon, restart=restart, **kwargs), x) and A.iterations == steps
    assert same_bytes(solve(A, rhs, rtol=RTOL, precon=precon, restart=restart, check=1, **kwargs), x) and A.iterations == steps


def test_wave_per_row_and_wide_indices():
    '''the product of the step at 64 lanes, with int32 and with int64 column indices: the same contract'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('wide')
    B = A._with_values(A.triplet()[0])
    B.lanes = 64
    contract('wide', solve(B, rhs, rtol=RTOL, **kwargs))
    B._columns = lambda: None  # the int64 indices of the assembly
    contract('wide', solve(B, rhs, rtol=RTOL, **kwargs))
    assert B._col32 is not None  # (made by the first solve: the second did without)


def test_odd_length_and_device_vectors():
    '''1001 rows: vectors of odd length are read one double at a time; a right-hand side on the device gives a result on the device'''
    from nutils_amd import device, matrix
    n = 1001
    N = scipy.sparse.diags([numpy.full(n - 1, -1.5), numpy.full(n, 4.), numpy.full(n - 1, -.5)], [-1, 0, 1], format='csr')
    cons = numpy.full(n, numpy.nan)
    cons[::100] = 2.
    rhs = numpy.random.default_rng(6).normal(size=n)
    A = hip(N)
    direct = matrix.ScipyMatrix(N).solve(rhs, constrain=cons)
    free = numpy.isnan(cons)
    start = numpy.where(free, 0., cons)
    r0 = numpy.linalg.norm((rhs - N @ start)[free])
    smin = numpy.linalg.svd(N.toarray()[free][:, free], compute_uv=False)[-1]
    for restart in (7, 30):
        x = solve(A, rhs, rtol=RTOL, constrain=cons, restart=restart)
        res = numpy.linalg.norm((rhs - N @ x)[free])
        assert numpy.array_equal(x[~free], start[~free]) and res <= RTOL * r0 * (1 + 1e-3) and numpy.linalg.norm(x - direct) <= res / smin
        it_ref = gmres_reference(N, rhs, start, free, numpy.where(free, .25, 0.), (RTOL * r0) ** 2, restart, n)[1]
        assert abs(A.iterations - it_ref) <= 2
    xd = solve(A, device.to_dev(rhs, 'float64'), rtol=RTOL, constrain=cons)
    assert xd.is_cuda and same_bytes(device.to_host(xd), x)


# ---- step counts, and the chunk of the multi-dot kernel ---------------------------------------------------------------------

@pytest.mark.parametrize('precon', ['diag', None], ids=['jacobi', 'plain'])
@pytest.mark.parametrize('name,restart', [('wide', 5), ('wide', 30), ('wide', 2000), ('tridiagonal', 30)])
def test_step_counts(name, restart, precon):
    '''`iterations` against the restatement on the same matrix, within 2 (the rule of tests/test_gpu_cg.py: the two differ in the order of their sums)'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem(name)
    solve(A, rhs, rtol=RTOL, precon=precon, restart=restart, **kwargs)
    it_ref = reference(name, precon, restart)[0]
    print(f'{name}, restart {restart}, precon {precon}: {A.iterations} steps on the device, {it_ref} in numpy')
    assert abs(A.iterations - it_ref) <= 2


@pytest.mark.parametrize('which', ['C - 1', 'C', 'C + 1', '2 C + 1'])
def test_chunk_boundaries(which):
    '''cycles whose last steps have one basis vector less than a chunk, a full chunk, a chunk and one, two chunks and one'''
    from nutils_amd import kernels
    C = kernels.GMRES_CHUNK
    restart = {'C - 1': C - 1, 'C': C, 'C + 1': C + 1, '2 C + 1': 2 * C + 1}[which]
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('wide')
    x = solve(A, rhs, rtol=RTOL, restart=restart, **kwargs)
    contract('wide', x)
    it_ref, x_ref = reference('wide', 'diag', restart)
    print(f'restart {restart}: {A.iterations} steps on the device, {it_ref} in numpy, |x - x_numpy| = {numpy.linalg.norm(x - x_ref):.2e}')
    assert abs(A.iterations - it_ref) <= 2
    assert numpy.linalg.norm(x - x_ref) <= 2 * RTOL * r0 * (1 + 1e-3) / smin  # (both within residual / sigma_min of the solution)


# ---- the kernels, driven directly ----------------------------------------------------------------------------------------------

class Device:
    '''the vectors and the work array of a cycle on the device, and the three entry points on them.  x and r are given; V, z and w start as NaN, so that an
    entry a kernel should have written and did not shows.'''

    def __init__(self, A, x, r, restart, mask=None, dinv=None, col32=True, lanes=0):
        from nutils_amd import device, kernels
        self.values, self.rowptr, self.colidx = A.triplet()
        self.n, self.m = len(x), restart
        self.col32 = kernels.csr_compact(self.colidx, self.n) if col32 else None
        self.lanes = lanes
        self.mask = None if mask is None else device.to_dev(mask, 'uint8')
        self.dinv = None if dinv is None else device.to_dev(dinv, 'float64')
        nan = lambda size: device.to_dev(numpy.full(size, numpy.nan), 'float64')
        self.V, self.z, self.w = nan((restart + 1) * self.n), nan(self.n), nan(self.n)
        self.x, self.r = device.to_dev(x, 'float64'), device.to_dev(r, 'float64')
        self.work = kernels.gmres_work(restart)
        self.work.fill_(numpy.nan)
        kernels.gmres_init(self.dinv, self.r, self.V, self.z, self.work, restart=restart)

    def iterate(self, niter, stop_rr):
        from nutils_amd import kernels
        kernels.gmres_iterate(self.values, self.rowptr, self.colidx, self.n, rowmask=self.mask, dinv=self.dinv, V=self.V, z=self.z, w=self.w, work=self.work,
                              restart=self.m, stop_rr=stop_rr, niter=niter, col32=self.col32, lanes=self.lanes)

    def update(self):
        from nutils_amd import kernels
        kernels.gmres_update(self.dinv, self.V, self.x, self.work, restart=self.m)

    def head(self):
        '''(estimate, flag, count, status)'''
        return self.work[:4].tolist()

    def state(self):
        '''every vector and the cells of the work array below the partials, on the host'''
        from nutils_amd import device
        c = cells(self.m)
        return dict(V=device.to_host(self.V).reshape(self.m + 1, self.n), z=device.to_host(self.z), w=device.to_host(self.w), x=device.to_host(self.x),
                    work=device.to_host(self.work[:c['r'] + self.m * (self.m + 1)]))


def wide_cycle(restart, precon=True, **kwargs):
    A, ref, kw, rhs, free, start, r0, direct, smin = problem('wide')
    dinv = jacobi('wide', precon)
    r_in = numpy.where(free, rhs - ref @ start, 0.)
    return Device(A, start, r_in, restart, mask=free, dinv=dinv, **kwargs), ref, free, dinv, r_in, start, r0


# ---- orthogonality ------------------------------------------------------------------------------------------------------------

def test_orthogonality():
    '''One full cycle of 72 steps on 'wide' (an unrestarted solve takes 89): max |V^T V - I| <= 1e-13 over the 72 basis vectors.  Two passes of classical
    Gram-Schmidt leave 1.3e-15; the restatement with one pass, run beside it, leaves 2e-9, and a build whose second pass subtracts nothing left 3.2e-10 on
    the device: the test fails if the second pass is lost.'''
    dev, ref, free, dinv, r_in, start, r0 = wide_cycle(72)
    dev.iterate(72, 0.)
    est, flag, count, st = dev.head()
    assert (flag, count, st) == (0, 72, ST_FULL)
    V = dev.state()['V'][:72]
    worst = numpy.abs(V @ V.T - numpy.eye(72)).max()
    one = Cycle(lambda y: ref @ y, free, dinv, start, 72, passes=1)
    one.init(r_in)
    one.iterate(72, 0.)
    one_pass = numpy.abs(one.V[:72] @ one.V[:72].T - numpy.eye(72)).max()
    print(f'max |V^T V - I| = {worst:.2e} on the device, {one_pass:.2e} with one pass in numpy')
    assert one_pass > 1e-11  # (1.96e-9 when this was written, against the bound of 1e-13 below)
    assert worst <= 1e-13
    assert not V[:, ~free].any()


# ---- one Arnoldi step against longdouble -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def one_step(precon):
    '''Inputs of the first step of a cycle on 'wide' (r = mask(b - A x) and dinv as float64 vectors: the device gets the same bits), what nh_gmres_init and one
    nh_gmres_iterate make of them in longdouble, and how far float64 kernels may be from that.  u = 2^-53, gamma_k = k u / (1 - k u), n = 1480, hats on what the
    device holds, W = |dinv| (1 without a preconditioner, and then z = v and the roundings marked [J] do not happen); every bound is evaluated on the reference's
    values.  dot(a, da, b, db) bounds the error of a sum of n products a^_i b^_i in any order, fused or not, against a . b:
    sum (|a| db + da |b| + da db) + gamma_(n+2) sum (|a| + da) (|b| + db).  sub(y, dy, c, dc, v, dv) bounds fl(y^ - c^ v^) against y - c v: the error of the
    product, d = |c| dv + dc (|v| + dv), one rounding of it (none if fused) and one of the difference: with m = (|c v| + d) (1 + u), dy + d + u m + u (|y| + dy + m).

    init       rr^ = r . r, a sum of n squares: e_rr = gamma_(n+2).  beta^ = fl(sqrt(rr^)): e_beta = e_rr + u (the root halves a relative error).
               v0^ = fl(r / beta^): e_v0 = (1 + u) / (1 - e_beta) - 1, dv0 = e_v0 |v0|.  z^ = fl(dinv v0^) [J]: dz = W dv0 + u W (|v0| + dv0).
    product    w^ = mask(A z^): dw = 2 gamma_(len+1) |A| (|z| + dz) (product_bound of test_gpu_matrix_hip: the sum of a row in any order) + |A| dz.
    pass 1     h1^ = v0^ . w^: d_h1 = dot(v0, dv0, w, dw).  w1^ = fl(w^ - h1^ v0^): dw1 = sub(w, dw, h1, d_h1, v0, dv0).
    pass 2     h2^ = v0^ . w1^ (h2 itself is zero but for the reference's roundings): d_h2 = dot(v0, dv0, w1, dw1).  w2^ = fl(w1^ - h2^ v0^):
               dw2 = sub(w1, dw1, h2, d_h2, v0, dv0).  ww^ = w2^ . w2^: d_ww = dot(w2, dw2, w2, dw2), e_ww = d_ww / ww.
    scalars    p^ = fl(h1^ + h2^): d_p = d_h1 + d_h2 + u (|h1| + |h2| + d_h1 + d_h2).  q^ = fl(sqrt(ww^)): d_q = (e_ww + u) q.
               d^ = hypot(p^, q^), within 2 u of the true root: the root is 1-Lipschitz in either argument: d_d = d_p + d_q + 2 u (d + d_p + d_q).
               c^ = fl(p^ / d^): d_c = (d_p + |c| d_d) / (d - d_d) + u (|c| + the same); s^ = fl(q^ / d^) likewise with d_q.
               g0^ = fl(c^ beta^): d_g0 = |c| e_beta beta + d_c beta (1 + e_beta), plus u of the whole; g1^ = fl(-s^ beta^) likewise; RR^ = fl(g1^ g1^):
               d_RR = 2 |g1| d_g1 + d_g1^2 + u (|g1| + d_g1)^2.
    normalize  v1^ = fl(w2^ / q^): dv1 = (dw2 + |v1| d_q) / (q - d_q), plus u of the whole.  z^ = fl(dinv v1^) [J]: dz1 = W dv1 + u W (|v1| + dv1).

    A workgroup's partial dropped or taken twice moves h1 and ww by about a third of their terms, decades above these bounds, and h1, q carry it into every
    entry of w, v1 and z.  The elementwise bounds get a factor 1 + 2^-10 for the reference's own roundings (2^-64 each).'''
    from test_gpu_matrix_hip import product_bound
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('wide')
    n = len(rhs)
    ld = numpy.longdouble
    dinv = jacobi('wide', precon)
    r_in = numpy.where(free, rhs - ref @ start, 0.)
    dense = ref.toarray().astype(ld)
    cyc = Cycle(lambda y: dense @ y, free, None if dinv is None else dinv.astype(ld), start.astype(ld), 30)
    cyc.init(r_in.astype(ld))
    beta, v0, z0 = cyc.HN, cyc.V[0].copy(), cyc.z.copy()
    w0 = cyc.A(z0)
    h1 = v0 @ w0
    w1 = w0 - h1 * v0
    cyc.step(ld(0))
    assert (cyc.ST, cyc.FLAG, cyc.COUNT) == (0, False, 1)
    h2, w2, v1, z1 = cyc.H2[0], cyc.w, cyc.V[1], cyc.z
    assert abs(h1 - cyc.H1[0]) <= 1e-18 * abs(h1) and abs(h2) < 1e-17 * abs(h1)
    q, d, c, s, g0, g1, RR = cyc.HN, cyc.R[0][0], cyc.CS[0], cyc.SN[0], cyc.G[0], cyc.G[1], cyc.RR
    f = lambda a: numpy.abs(numpy.asarray(a, dtype=float))  # (bounds are float64: their own rounding is 1e-16 of them)
    absA = abs(ref)
    W = f(dinv) if precon else numpy.ones(n)
    up = U if precon else 0.
    g2 = gamma(n + 2)
    dot = lambda a, da, b, db: (a * db + da * b + da * db).sum() + g2 * ((a + da) * (b + db)).sum()

    def sub(y, dy, c, dc, v, dv):
        e = f(c) * dv + dc * (v + dv)
        m = (f(c) * v + e) * (1 + U)
        return dy + e + U * m + U * (y + dy + m)

    product = lambda y, dy: numpy.where(free, product_bound(ref, y + dy) + absA @ dy, 0.)
    e_beta = g2 + U
    e_v0 = (1 + U) / (1 - e_beta) - 1
    dv0 = e_v0 * f(v0)
    dz = W * dv0 + up * W * (f(v0) + dv0)
    dw = product(f(z0), dz)
    d_h1 = dot(f(v0), dv0, f(w0), dw)
    dw1 = sub(f(w0), dw, h1, d_h1, f(v0), dv0)
    d_h2 = dot(f(v0), dv0, f(w1), dw1)
    dw2 = sub(f(w1), dw1, h2, d_h2, f(v0), dv0)
    ww = float(w2 @ w2)
    e_ww = dot(f(w2), dw2, f(w2), dw2) / ww
    d_p = d_h1 + d_h2 + U * (f(h1) + f(h2) + d_h1 + d_h2)
    d_q = (e_ww + U) * float(q)
    d_d = d_p + d_q + 2 * U * (float(d) + d_p + d_q)
    quotient = lambda a, da: ((da + f(a) * d_d) / (float(d) - d_d)) * (1 + U) + U * f(a)
    d_c, d_s = quotient(c, d_p), quotient(s, d_q)
    rotated = lambda a, da: (f(a) * e_beta * float(beta) + da * float(beta) * (1 + e_beta)) * (1 + U) + U * f(a) * float(beta)
    d_g0, d_g1 = rotated(c, d_c), rotated(s, d_s)
    d_RR = 2 * f(g1) * d_g1 + d_g1 ** 2 + U * (f(g1) + d_g1) ** 2
    dv1 = ((dw2 + f(v1) * d_q) / (float(q) - d_q)) * (1 + U) + U * f(v1)
    dz1 = W * dv1 + up * W * (f(v1) + dv1)
    relative = dict(h1=d_h1 / f(h1), q=d_q / float(q), d=d_d / float(d), c=d_c / f(c), s=d_s / f(s), g0=d_g0 / f(g0), g1=d_g1 / f(g1), RR=d_RR / float(RR))
    print(f'one step, precon={precon}: relative bounds ' + ', '.join(f'{name} {float(e):.1e}' for name, e in relative.items()) + f'; h2: {d_h2:.1e} absolute')
    assert max(relative.values()) < 1e-9, relative  # (the bounds are sharp enough to see a partial go missing)
    assert d_h2 < 1e-9 * f(h1)
    slack = 1 + 2. ** -10
    vectors = dict(v0=(v0, dv0), v1=(v1, dv1), z=(z1, dz1), w=(w2, dw2))
    scalars = dict(RR=(RR, d_RR), HN=(q, d_q), h1=(h1, d_h1), h2=(h2, d_h2), cs=(c, d_c), sn=(s, d_s), g0=(g0, d_g0), g1=(g1, d_g1), r=(d, d_d))
    return dict(r_in=r_in, dinv=dinv, vectors={name: (value, bound * slack) for name, (value, bound) in vectors.items()},
                scalars={name: (value, float(bound) * slack) for name, (value, bound) in scalars.items()})


@pytest.mark.parametrize('precon', [True, False], ids=['jacobi', 'plain'])
@pytest.mark.parametrize('narrow', [True, False], ids=['col32', 'col64'])
@pytest.mark.parametrize('lanes', [4, 64])
def test_one_step(lanes, narrow, precon):
    '''nh_gmres_init and one nh_gmres_iterate, called directly, against `one_step`: v0, v1, z, w, the two passes' dots, the rotation, g, the pivot and the
    estimate within the derived bounds; masked rows exactly zero; no flag, one column counted; a repeat byte-identical.  Three Gram-Schmidt workgroups (the last
    partial) and 24 or 370 product workgroups contribute.'''
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('wide')
    assert A.shape[0] == 1480 and A.lanes == 4 and 0 < (~free).sum() < 100
    expect = one_step(precon)
    m = 30
    c = cells(m)
    where = dict(RR=CELLS['RR'], HN=CELLS['HN'], h1=c['h1'], h2=c['h2'], cs=c['cs'], sn=c['sn'], g0=c['g'], g1=c['g'] + 1, r=c['r'])

    def run():
        dev = Device(A, start, expect['r_in'], m, mask=free, dinv=expect['dinv'], col32=narrow, lanes=lanes)
        dev.iterate(1, 0.)
        return dev.state()

    got, again = run(), run()
    work = got['work']
    assert (work[CELLS['FLAG']], work[CELLS['COUNT']], work[CELLS['ST']]) == (0, 1, 0)
    vectors = dict(v0=got['V'][0], v1=got['V'][1], z=got['z'], w=got['w'])
    for name, (value, bound) in expect['vectors'].items():
        err = numpy.abs(vectors[name] - value).astype(float)
        print(f'{name}: max error / bound = {(err / numpy.maximum(bound, 1e-300)).max():.3f}')
        assert (err <= bound).all(), (name, (err / numpy.maximum(bound, 1e-300)).max())
        assert not vectors[name][~free].any(), name  # (NaN where a kernel left a masked row unwritten)
    for name, (value, bound) in expect['scalars'].items():
        err = abs(float(work[where[name]] - value))
        print(f'{name}: error / bound = {err / bound:.3f}')
        assert err <= bound, (name, err / bound)
    assert numpy.isnan(got['V'][2:]).all()  # nothing beyond v1 was touched
    for name in got:
        assert numpy.array_equal(got[name].view(numpy.int64), again[name].view(numpy.int64)), name


# ---- the estimates of a cycle, and what happens after it stops ----------------------------------------------------------------------

@pytest.mark.parametrize('precon', [True, False], ids=['jacobi', 'plain'])
def test_estimates_never_rise(precon):
    '''Read after every step, the estimates of a cycle never rise by more than a factor 1 + 4 u.  (By construction they do not rise at all: the sine of a
    rotation is q / d with d no smaller than q, at most 1 after rounding, and g' = fl(s g), RR = fl(g' g') are monotone in |g|.  The factor leaves room for a
    division or a product that rounds otherwise: two roundings in g', doubled by the square.)'''
    dev, ref, free, dinv, r_in, start, r0 = wide_cycle(30, precon)
    estimates = [dev.head()[0]]
    assert abs(estimates[0] - r_in @ r_in) <= 2 * gamma(1482) * (r_in @ r_in)  # r . r: the device's order of summation and numpy's
    for j in range(30):
        dev.iterate(1, 0.)
        est, flag, count, st = dev.head()
        assert (flag, count, st) == (0, j + 1, ST_FULL if j == 29 else 0)
        estimates.append(est)
    print(f'precon={precon}: ' + ' '.join(f'{e:.2e}' for e in estimates))
    assert all(b <= a * (1 + 4 * U) for a, b in zip(estimates, estimates[1:]))
    assert estimates[-1] < .5 * estimates[0]  # (and they do fall)
    # the update makes the estimate the true residual: the rounding of 30 steps apart (the bound of the restatement's own check, on its estimate)
    dev.update()
    x = dev.state()['x']
    true = numpy.linalg.norm(numpy.where(free, problem('wide')[3] - ref @ x, 0.))
    print(f'estimate {estimates[-1] ** .5:.6e}, true residual {true:.6e}')
    assert abs(true - estimates[-1] ** .5) <= 1e-10 * estimates[0] ** .5
    assert numpy.array_equal(x[~free], start[~free])


@pytest.mark.parametrize('stop', ['done', 'full'])
def test_stopped_steps_move_nothing(stop):
    '''after the stop (the estimate within the bound; the restart-th column taken) further steps change no byte of V, z, w, x or the cells'''
    restart = 100 if stop == 'done' else 5
    dev, ref, free, dinv, r_in, start, r0 = wide_cycle(restart)
    stop_rr = (1e-3 * r0) ** 2
    st = 0
    while st == 0:
        dev.iterate(16, stop_rr)
        est, flag, count, st = dev.head()
    assert flag == 0 and (st == ST_DONE and est <= stop_rr and 1 < count < 100 and count % 16 if stop == 'done' else st == ST_FULL and count == 5 and est > stop_rr)
    before = dev.state()
    dev.iterate(7, stop_rr)
    after = dev.state()
    for name in before:
        assert numpy.array_equal(before[name].view(numpy.int64), after[name].view(numpy.int64)), name
    assert numpy.isnan(before['V'][int(count):]).all() and not numpy.isnan(before['V'][:int(count)]).any()  # (a finished cycle does not normalise a direction it will not use)
    dev.update()
    dev.iterate(3, stop_rr)  # ... nor after the update
    final = dev.state()
    for name in 'V', 'z', 'w':
        assert numpy.array_equal(before[name].view(numpy.int64), final[name].view(numpy.int64)), name
    assert final['work'][:4].tolist() == [est, flag, count, st]
    assert numpy.array_equal(final['x'][~free], start[~free]) and not numpy.array_equal(final['x'], start)


# ---- maxiter, singular matrices, the lucky breakdown, trivial systems, NaN: the stopping rules and errors of solve --------------------------------------------------------------------------------

@pytest.mark.parametrize('check', [16, 5, 1])
def test_stops_at_maxiter(check):
    '''a maxiter that is no multiple of `check` or `restart`'''
    from nutils_amd import matrix
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('wide')
    with pytest.raises(matrix.ToleranceNotReached) as info:
        solve(A, rhs, rtol=RTOL, maxiter=13, restart=5, check=check, **kwargs)
    best = info.value.best
    assert A.iterations == 13
    assert numpy.isfinite(best).all() and numpy.array_equal(best[~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ best)[free])
    print(f'check={check}: |r| / |r0| = {res / r0:.3e}')
    assert RTOL * r0 < res <= r0  # (GMRES never makes a residual larger)
    x_ref, it_ref, outcome = gmres_reference(ref, rhs, start, free, jacobi('wide', True), (RTOL * r0) ** 2, 5, 13, check=check)
    assert (it_ref, outcome) == (13, 'maxiter') and numpy.linalg.norm(best - x_ref) <= 1e-9 * numpy.linalg.norm(x_ref)
    with pytest.warns(UserWarning, match='tolerance'):
        lenient = A.solve_leniently(rhs, solver='fgmres', rtol=RTOL, maxiter=13, restart=5, check=check, **kwargs)
    assert numpy.array_equal(lenient, best)


def test_singular_matrix():
    from nutils_amd import matrix
    S = hip([[1., 0.], [0., 0.]])
    with pytest.raises(matrix.MatrixError, match='fgmres: singular matrix'):
        solve(S, numpy.array([1., 1.]), rtol=1e-12, precon=None)
    with pytest.raises(matrix.MatrixError, match='diagonal has zero entries'):
        S.solve(numpy.array([1., 1.]), solver='fgmres', rtol=1e-12)
    Z = hip(scipy.sparse.csr_matrix(([0., 0.], [0, 1], [0, 1, 2]), (2, 2)))  # a zero column at the first step
    with pytest.raises(matrix.MatrixError, match='fgmres: singular matrix'):
        solve(Z, numpy.array([1., 1.]), rtol=1e-12, precon=None)
    assert Z.iterations == 0 and S._hostcsr is None


def test_lucky_breakdown():
    '''the identity: the first direction is all there is'''
    n = 1000
    I = hip(scipy.sparse.identity(n, format='csr'))
    rhs = numpy.random.default_rng(7).normal(size=n)
    for precon in ('diag', None):
        x = solve(I, rhs, rtol=1e-12, precon=precon)
        assert I.iterations == 1 and (numpy.abs(x - rhs) <= 8 * U * numpy.abs(rhs)).all()  # (r / |r|, the rotation, g / d and y v: a few roundings)
    D = hip([[1., 0.], [0., -1.]])  # indefinite: two steps without Jacobi, which makes it the identity
    x = solve(D, numpy.array([1., 2.]), rtol=1e-12, precon=None)
    assert numpy.allclose(x, [1., -2.], rtol=1e-12, atol=0) and D.iterations == 2
    x = solve(D, numpy.array([1., 2.]), rtol=1e-12)
    assert numpy.allclose(x, [1., -2.], rtol=1e-12, atol=0) and D.iterations == 1


def test_trivial_systems():
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('laplace')
    # every dof constrained: the constraints come back, without a step
    held = numpy.arange(float(len(rhs)))
    assert numpy.array_equal(solve(A, rhs, iterated=False, rtol=RTOL, constrain=held), held) and A.iterations == 0
    # a residual within the tolerance from the start: the initial vector comes back
    assert numpy.array_equal(solve(A, ref @ start, iterated=False, rtol=RTOL, atol=1e-9, **kwargs), start) and A.iterations == 0
    # no right-hand side, no constraints: zero
    assert not solve(A, iterated=False, rtol=RTOL).any() and A.iterations == 0


def test_non_finite():
    from nutils_amd import device, matrix
    A, ref, kwargs, rhs, free, start, r0, direct, smin = problem('laplace')
    values = A.triplet()[0].clone()
    values[len(values) // 2] = numpy.nan
    B = A._with_values(values)
    for precon in (None, 'diag'):
        with pytest.raises(matrix.MatrixError, match='fgmres: non-finite residual'):
            solve(B, rhs, iterated=False, rtol=RTOL, precon=precon, **kwargs)  # (the first residual already: whatever the start vector holds, times NaN)
    assert B.iterations == 0
