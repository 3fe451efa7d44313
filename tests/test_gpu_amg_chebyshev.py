'''The Chebyshev smoother of the AMG preconditioner (preconargs=dict(smoother='chebyshev', ...), nutils_amd/amg.py, nh_csr_chebyshev and nh_csr_lanczos of
nh_amg.hip) on the GPU, against the numpy restatement of tests/test_amg_chebyshev_host.py: the two kernels one by one against longdouble, one cycle, the solve
contract and the iteration counts, the unchanged default, and solver.System.

Problems: 'wide', the 40 x 37 bilinear Laplace of tests/test_gpu_cg.py with one side held at non-zero values (1480 rows: six vector workgroups, the last
partial; three levels with coarse=16); the chain tridiag(-1, 2, -1) of 262 444 rows of tests/test_gpu_amg.py (the row and vector grids stride past their caps);
'hex', linear elasticity on 9^3 perturbed hexahedra with the face x = 0 held and the six rigid-body modes (3000 rows of up to 81 entries, coarse=64).'''
import functools
import numpy
import pytest
import scipy.sparse
import scipy.sparse.linalg

from test_cg_host import gamma, U
from test_amg_host import hierarchy, pcg_reference, product, free_part
from test_amg_nullspace_host import hierarchy as hierarchy_with_nullspace, elasticity
from test_amg_chebyshev_host import lanczos, theta_of, start_vector, with_bounds, chebyshev_cycle, held_face, exact_diagonal
from test_gpu_cg import hip, problem, contract, same_bytes, RTOL
from test_gpu_amg import chain, download, solve

pytestmark = pytest.mark.gpu

ld = numpy.longdouble


# ---- problems ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hex_problem():
    '''(A on the device, its host twin, constraints, right-hand side, free mask, start vector, |r0|, the rigid-body modes).  Made once, never written.'''
    from nutils_amd import amg
    shape = (9, 9, 9)
    ref, coords = elasticity(shape)
    free = held_face(shape)
    cons = numpy.where(free, numpy.nan, 0.)
    rhs = numpy.random.default_rng(4).normal(size=len(cons))
    start = numpy.where(free, 0., cons)
    return hip(ref), ref, cons, rhs, free, start, numpy.linalg.norm((rhs - ref @ start)[free]), amg.rigid_body_modes(coords)


def system(name):
    '''(A, ref, constrain, rhs, free, start, r0, B or None, coarse) of 'wide', 'chain' or 'hex' '''
    if name == 'hex':
        return hex_problem() + (64,)
    if name == 'chain':
        return chain() + (None, 256)
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    ref = scipy.sparse.csr_matrix(ref)
    ref.sort_indices()
    return A, ref, kwargs['constrain'], rhs, free, start, r0, None, 16


@functools.lru_cache(maxsize=None)
def device_hierarchy(name, degree):
    '''(amg.Hierarchy with the Chebyshev smoother, its levels downloaded as the restatement's namespaces with the device's own ub and lb)'''
    from nutils_amd import amg, device
    A, ref, cons, rhs, free, start, r0, B, coarse = system(name)
    values, rowptr, colidx = A.triplet()
    levels = amg.symbolic(rowptr, colidx, device.to_dev(free, 'uint8') != 0, coarse, None if B is None else B.shape[1])
    h = amg.Hierarchy(levels, values, 1, None if B is None else device.to_dev(B.ravel(), 'float64').reshape(B.shape), dict(degree=degree, eigsteps=10, eigratio=10.))
    host = download(h)
    for ns, d in zip(host, h.data):
        if ns.kind == 'coarsen':
            ns.theta, ns.ub, ns.lb, ns.coef = d.theta, d.ub, d.lb, device.to_host(d.coef)
    return h, host


@functools.lru_cache(maxsize=None)
def reference_levels(name):
    '''the restatement's own hierarchy with its own estimates'''
    A, ref, cons, rhs, free, start, r0, B, coarse = system(name)
    return with_bounds(hierarchy(ref, free, coarse) if B is None else hierarchy_with_nullspace(ref, free, B, coarse))


@functools.lru_cache(maxsize=None)
def reference_iterations(name, degree):
    A, ref, cons, rhs, free, start, r0, B, coarse = system(name)
    levels = reference_levels(name)
    x, it, starts, outcome = pcg_reference(ref, rhs, start, free, lambda r: chebyshev_cycle(levels, r, degree), (RTOL * r0) ** 2, int(free.sum()))
    assert outcome == 'converged'
    return it


def times(name, ref, x):
    '''A x in longdouble'''
    x = x.astype(ld)
    return 2 * x - numpy.r_[0, x[:-1]] - numpy.r_[x[1:], 0] if name == 'chain' else product(ref, x)


# ---- 1. nh_csr_chebyshev --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,lanes,narrow', [('wide', 1, True), ('wide', 4, True), ('wide', 64, True), ('wide', 1, False), ('wide', 4, False), ('wide', 64, False), ('chain', 64, True)])
def test_chebyshev_step(name, lanes, narrow):
    '''dout = c1 d + c2 dinv (b - A x), y = x + dout against longdouble, the general step and the first.  t = b - A x is a sum of len + 1 terms in any order:
    product_bound of tests/test_gpu_matrix_hip.py with one extra term and the tail |b|.  The second term g t, g = c2 dinv, carries g dt and two roundings (of g and
    of the product); the first term c1 d one (none if fused) and the sum one; y = x + dout one more.  Masked rows are exactly +0 in both; a repeat gives the same
    bytes; the first step reads no d: its output buffer starts full of NaN.'''
    from test_gpu_matrix_hip import product_bound
    from nutils_amd import amg, device, kernels
    A, ref, cons, rhs, free, start, r0, B, coarse = system(name)
    ref = scipy.sparse.csr_matrix(ref)
    n = len(rhs)
    if name == 'chain':
        assert (n + 3) // 4 > 2048  # four rows a workgroup at 64 lanes: the grid strides past its cap
    rng = numpy.random.default_rng(21)
    x, b, d = numpy.where(free, rng.normal(size=n), 0.), rng.normal(size=n), rng.normal(size=n)
    dinv = numpy.where(free, 1 / ref.diagonal(), 0.)
    c1, c2 = amg.chebyshev_coefficients(2.3, .23, 3)[4:]
    values, rowptr, colidx = A.triplet()
    dev = lambda v: device.to_dev(v, 'float64')
    kwargs = dict(rowmask=device.to_dev(free, 'uint8'), col32=kernels.csr_compact(colidx, n) if narrow else None, lanes=lanes)

    def run(first):
        dout = dev(numpy.full(n, numpy.nan))
        y, out = kernels.csr_chebyshev(values, rowptr, colidx, n, dev(x), None if first else dev(d), dev(dinv), dev(b), dev(numpy.array([c1, c2])), dout=dout, **kwargs)
        assert out is dout
        return device.to_host(y), device.to_host(out)

    t = b.astype(ld) - times(name, ref, x)
    dt = product_bound(ref, x, extra=1, tail=abs(b))
    g = abs(c2 * dinv)
    for first in (True, False):
        y, dout = run(first)
        assert numpy.isfinite(y).all() and numpy.isfinite(dout).all()
        head = numpy.zeros(n) if first else abs(c1 * d)
        expect_d = numpy.where(free, (0 if first else ld(c1) * d.astype(ld)) + ld(c2) * dinv.astype(ld) * t, 0)
        expect_y = numpy.where(free, x.astype(ld) + expect_d, 0)
        m = g * (numpy.abs(t).astype(float) + dt)
        bound_d = (g * dt + 2 * U * m + U * head + U * (head + m * (1 + 2 * U))) * (1 + 2. ** -10)
        bound_y = bound_d + U * (abs(x) + numpy.abs(expect_d).astype(float) + bound_d) * (1 + 2. ** -10)
        err_d, err_y = numpy.abs(dout - expect_d).astype(float), numpy.abs(y - expect_y).astype(float)
        print(f'{name}, {lanes} lanes, {"int32" if narrow else "int64"}, first={first}: max error / bound: dout {(err_d[free] / bound_d[free]).max():.3f}, y {(err_y[free] / bound_y[free]).max():.3f}')
        assert (err_d <= bound_d).all() and (err_y <= bound_y).all()
        for got in (y, dout):
            assert not got[~free].any() and not numpy.signbit(got[~free]).any()
        again = run(first)
        assert same_bytes(y, again[0]) and same_bytes(dout, again[1])
    # in place: dout is d
    d_dev = dev(d)
    y, out = kernels.csr_chebyshev(values, rowptr, colidx, n, dev(x), d_dev, dev(dinv), dev(b), dev(numpy.array([c1, c2])), dout=d_dev, **kwargs)
    assert same_bytes(device.to_host(y), run(False)[0]) and same_bytes(device.to_host(d_dev), run(False)[1])


def test_chebyshev_argument_errors():
    from nutils_amd import device, kernels, _lib
    A, ref, cons, rhs, free, start, r0, B, coarse = system('wide')
    n = len(rhs)
    values, rowptr, colidx = A.triplet()
    v = device.zeros(n, 'float64')
    coef = device.zeros(2, 'float64')
    with pytest.raises(_lib.NutilsHipError, match='must not be the argument'):
        kernels.csr_chebyshev(values, rowptr, colidx, n, v, None, v.clone(), v.clone(), coef, y=v)
    with pytest.raises(_lib.NutilsHipError, match='NULL vector'):
        kernels.csr_chebyshev(values, rowptr, colidx, n, v, None, None, v.clone(), coef)
    with pytest.raises(_lib.NutilsHipError, match='steps must be'):
        kernels.csr_lanczos(values, rowptr, colidx, n, v, v.clone(), 0)
    empty = device.zeros(0, 'float64')
    ptr0 = device.zeros(1, 'int64')
    idx0 = device.zeros(0, 'int64')
    y, dout = kernels.csr_chebyshev(empty, ptr0, idx0, 0, empty, None, empty, empty, coef)
    assert y.numel() == 0 and dout.numel() == 0
    assert not device.to_host(kernels.csr_lanczos(empty, ptr0, idx0, 0, empty, empty, 3)).any()


# ---- 2. nh_csr_lanczos ------------------------------------------------------------------------------------------------------

def run_lanczos(A, free, dinv, u, steps=10, values=None):
    from nutils_amd import device, kernels
    v, rowptr, colidx = A.triplet()
    out = kernels.csr_lanczos(v if values is None else values, rowptr, colidx, A.shape[1], device.to_dev(numpy.sqrt(dinv), 'float64'), device.to_dev(u, 'float64'), steps,
                              rowmask=device.to_dev(free, 'uint8'), col32=A._columns(), lanes=A.lanes)
    return device.to_host(out)


@pytest.mark.parametrize('name', ['wide', 'hex'])
def test_lanczos(name):
    '''alpha_0 and beta_1 of the device against the restatement in longdouble, theta of ten steps against the largest eigenvalue, a repeat byte-identical, and
    masked rows out of it.  With e_q = gamma_(n+4) the relative error of an entry of q_0 (the sum of n squares, its root, the division) and W_i = s_i sum_j |a_ij|
    s_j |q_j|: an entry of w carries dw_i = (gamma_(len+4) + e_q + 2 u) W_i (the row sum in any order, the roundings of s q and of the product with s_i, the
    device's s being the rounded root); alpha = q . w carries (e_q + gamma_(n+1)) sum |q_i| W_i + sum |q_i| dw_i; an entry of v = w - alpha q carries dv_i = dw_i +
    (|alpha| e_q + d_alpha) |q_i| + 2 u (W_i + |alpha q_i|), and beta = |v| carries |dv| + gamma_(n+2) beta.'''
    A, ref, cons, rhs, free, start, r0, B, coarse = system(name)
    n = len(rhs)
    dinv = numpy.where(free, 1 / ref.diagonal(), 0.)
    u = start_vector(n)
    out = run_lanczos(A, free, dinv, u)
    assert out[-1] == 10 and same_bytes(out, run_lanczos(A, free, dinv, u))
    alpha, beta, taken = lanczos(ref, free, dinv, 1, dtype=ld)
    s = numpy.sqrt(dinv)
    q = numpy.where(free, u, 0.)
    q = numpy.abs(q / numpy.linalg.norm(q))
    length = int(numpy.diff(ref.indptr).max())
    W = s * (abs(free_part(ref, free)) @ (s * q))
    e_q = gamma(n + 4)
    dw = (gamma(length + 4) + e_q + 2 * U) * W
    d_alpha = ((e_q + gamma(n + 1)) * (q @ W) + q @ dw) * (1 + 2. ** -10)
    dv = dw + (abs(float(alpha[0])) * e_q + d_alpha) * q + 2 * U * (W + abs(float(alpha[0])) * q)
    d_beta = (numpy.linalg.norm(dv) + gamma(n + 2) * float(beta[0])) * (1 + 2. ** -10)
    print(f'{name}: alpha_0 = {out[0]!r}, error / bound = {abs(float(out[0] - alpha[0])) / d_alpha:.1e}; beta_1 = {out[1]!r}, error / bound = {abs(float(out[1] - beta[0])) / d_beta:.1e}')
    assert abs(float(out[0] - alpha[0])) <= d_alpha and abs(float(out[1] - beta[0])) <= d_beta
    theta = theta_of(out[0:20:2], out[1:20:2])
    Ahat = scipy.sparse.diags(s) @ free_part(ref, free) @ scipy.sparse.diags(s)
    lmax = numpy.linalg.eigvalsh(Ahat.toarray())[-1] if n <= 1500 else scipy.sparse.linalg.eigsh(Ahat, k=1, which='LA', tol=0, return_eigenvectors=False)[0]
    print(f'{name}: theta = {theta:.5f}, lambda_max = {lmax:.5f}, ratio {theta / lmax:.4f}; the restatement has theta = {theta_of(*lanczos(ref, free, dinv, 10)[:2]):.5f}')
    assert theta <= lmax * (1 + 1e-12) and theta >= .9 * lmax
    # masked rows never enter: other (finite) entries in their rows and columns change no bit, though u is not 0 there
    from nutils_amd import device
    v, rp, ci = (device.to_host(t) for t in A.triplet())
    rows = numpy.repeat(numpy.arange(n), numpy.diff(rp))
    scaled = numpy.where(free[rows] & free[ci], v, 1000. * v + 1.)
    assert (~free).any() and u[~free].all() and (scaled != v).any()
    assert same_bytes(out, run_lanczos(A, free, dinv, u, values=device.to_dev(scaled, 'float64')))


def test_lanczos_stops():
    '''S A S = I with exact arithmetic (exact_diagonal of the host tests: powers of 4, 256 entries +-1): alpha_0 = 1, beta_1 = 0, one step taken, the rest of
    the array as it was zero-filled; rows that are masked or have s = 0 take no part although u is 1 there.  A start vector that is 0 wherever a row takes part
    takes no step at all.'''
    ref, free, dinv, u = exact_diagonal()
    A = hip(ref)
    out = run_lanczos(A, free, dinv, u)
    print(f'alpha_0 = {out[0]!r}, beta_1 = {out[1]!r}, steps {out[-1]}')
    assert out[-1] == 1 and out[0] == 1 and not out[1:-1].any()
    assert theta_of(out[:2], out[1:2]) == 1
    out = run_lanczos(A, free, dinv, numpy.where(free & (dinv != 0), 0., 1.))
    assert not out.any()


# ---- 3. one cycle ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,degree', [('wide', 2), ('wide', 3), ('hex', 2), ('hex', 3)])
def test_cycle(name, degree):
    '''nh_amg_apply with the Chebyshev smoother against the restatement's cycle in longdouble on the same hierarchy values and the device's own ub and lb.  The
    tolerance is measured as in tests/test_gpu_amg.py: the distance (maximum norm) of the float64 restatement from the longdouble one on the same input, times 8.
    The device's estimate is that of the restatement to a rounding's worth, and its coefficients are those of its bounds.'''
    from nutils_amd import amg, device
    h, levels = device_hierarchy(name, degree)
    A, ref, cons, rhs, free, start, r0, B, coarse = system(name)
    for l, (lv, mine) in enumerate(zip(levels, reference_levels(name))):
        if lv.kind == 'coarsen':
            print(f'{name} level {l}: theta = {lv.theta:.6f} (restatement {mine.theta:.6f}), rho = {lv.rho:.4f}, ub = {lv.ub:.6f}, lb = {lv.lb:.6f}')
            assert lv.ub == min(1.1 * lv.theta, lv.rho) and lv.lb == lv.ub / 10.
            assert numpy.array_equal(lv.coef, amg.chebyshev_coefficients(lv.ub, lv.lb, degree))
    assert sum(lv.kind == 'coarsen' for lv in levels) >= 2
    assert abs(levels[0].theta - reference_levels(name)[0].theta) <= 1e-9 * levels[0].theta  # (level 0 has the same matrix in both; below, the hierarchies differ by roundings)
    r = numpy.where(free, numpy.random.default_rng(13).normal(size=len(rhs)), 0.)
    exact = chebyshev_cycle(levels, r.astype(ld), degree)
    d64 = float(numpy.abs(chebyshev_cycle(levels, r, degree) - exact).max())
    r_dev = device.to_dev(r, 'float64')
    got = device.to_host(h.apply(r_dev))
    dist = float(numpy.abs(got - exact).max())
    print(f'{name}, degree {degree}: {len(levels)} levels: |float64 restatement - longdouble| = {d64:.3e}, |device - longdouble| = {dist:.3e}, |z| = {float(numpy.abs(exact).max()):.3e}')
    assert d64 > 0 and dist <= 8 * d64
    assert not got[~free].any()
    assert same_bytes(got, device.to_host(h.apply(r_dev)))


# ---- 4., 5. the solve --------------------------------------------------------------------------------------------------------

def residual_contract(name, x):
    A, ref, cons, rhs, free, start, r0, B, coarse = system(name)
    assert isinstance(x, numpy.ndarray) and numpy.array_equal(x[~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ x)[free])
    print(f'{name}: |r| / |r0| = {res / r0:.3e}')
    assert res <= RTOL * r0 * (1 + 1e-3)


@pytest.mark.parametrize('name', ['wide', 'hex'])
def test_solve_contract(name):
    from nutils_amd import _lib
    A, ref, cons, rhs, free, start, r0, B, coarse = system(name)
    assert name != 'wide' or start[~free].any()  # (held at non-zero values)
    base = dict(coarse=coarse) if B is None else dict(coarse=coarse, nullspace=B)
    args = dict(rtol=RTOL, constrain=cons)
    for degree in (2, 3):
        preconargs = dict(base, smoother='chebyshev', degree=degree)
        with _lib.trace() as calls:
            x = solve(A, rhs, preconargs=preconargs, **args)
        assert 'nh_csr_lanczos' in calls and calls.count('nh_amg_create') == 1
        residual_contract(name, x)
        if name == 'wide':
            contract('wide', x)
        assert same_bytes(solve(A, rhs, preconargs=preconargs, **args), x)  # a second solve
        y = solve(A, rhs, check=1, preconargs=preconargs, **args)
        it, it_ref = A.iterations, reference_iterations(name, degree)
        print(f'{name}, degree {degree}: {it} iterations on the device, {it_ref} in numpy')
        assert it == A.cg_iterations <= 1.1 * it_ref + 2
        assert same_bytes(x, y)  # the iterations that check=16 enqueues past convergence do nothing
        if degree == 2:
            assert same_bytes(solve(A, rhs, preconargs=dict(base, smoother='chebyshev'), **args), x)  # (the defaults)
            cheb2 = it
    if name == 'hex':
        solve(A, rhs, check=1, preconargs=dict(base, smoother='jacobi', sweeps=2), **args)
        print(f'hex: Chebyshev degree 2: {cheb2} iterations, Jacobi sweeps 2: {A.iterations}')
        assert cheb2 <= A.iterations


def test_default_is_unchanged():
    '''smoother='jacobi' is the cycle without the key, byte for byte, and calls neither new kernel'''
    from nutils_amd import _lib
    A, ref, cons, rhs, free, start, r0, B, coarse = system('hex')
    for extra in (dict(), dict(sweeps=2)):
        x = solve(A, rhs, rtol=RTOL, constrain=cons, preconargs=dict(coarse=coarse, nullspace=B, **extra))
        it = A.iterations
        with _lib.trace() as calls:
            y = solve(A, rhs, rtol=RTOL, constrain=cons, preconargs=dict(coarse=coarse, nullspace=B, smoother='jacobi', **extra))
        assert same_bytes(x, y) and A.iterations == it
        assert 'nh_csr_lanczos' not in calls and 'nh_csr_chebyshev' not in calls


def test_not_positive_definite():
    '''a negative diagonal has no root: the estimate is not a number, and the setup says so'''
    from nutils_amd import matrix
    A, ref, cons, rhs, free, start, r0, B, coarse = system('wide')
    with pytest.raises(matrix.MatrixError, match='amg: matrix is not positive definite'):
        (-A).solve(rhs, solver='cg', precon='amg', rtol=RTOL, constrain=cons, preconargs=dict(coarse=coarse, smoother='chebyshev'))  # (raised by the setup: no iteration)


# ---- 6. solver.System --------------------------------------------------------------------------------------------------------

def test_system(monkeypatch):
    '''the Laplace example under matrix.backend('hip') with linargs naming the smoother, against the 'diag' route within the bound of
    tests/test_gpu_amg.py::test_system_and_plan_cache; the estimate and the cycle run on the device; the symbolic phase runs once across a re-valued Jacobian and
    across a change of smoother'''
    from nutils_amd import amg, matrix, _lib
    from nutils_amd.solver import System
    from test_gpu_system_device import laplace_forms
    sqr, res = laplace_forms(32, 'std', 1)
    cons = System(sqr, trial='u').solve_constraints(droptol=1e-15)
    calls, symbolic = [], amg.symbolic
    monkeypatch.setattr(amg, 'symbolic', lambda *args, **kwargs: calls.append(1) or symbolic(*args, **kwargs))
    rtol = 1e-10
    preconargs = dict(coarse=64, smoother='chebyshev')
    with matrix.backend('hip'):
        dev = System(res, trial='u', test='v')
        with _lib.trace() as trace:
            x = dev.solve(constrain=cons, linargs=dict(solver='cg', precon='amg', rtol=rtol, preconargs=preconargs))['u']
        jac = dev._device_jac[1]
        it = dev.linear_iterations[-1]
        y = System(res, trial='u', test='v').solve(constrain=cons, linargs=dict(solver='cg', precon='diag', rtol=rtol))['u']
    assert 'nh_csr_lanczos' in trace and 'nh_pcg_iterate' in trace and 'nh_amg_create' in trace and len(calls) == 1
    assert isinstance(jac, matrix.HipMatrix) and jac._hostcsr is None
    free = numpy.isnan(cons['u']).ravel()
    assert numpy.array_equal(x.ravel()[~free], y.ravel()[~free])
    host = System(res, trial='u', test='v')
    K = host.assemble_jacobian({}).export('dense')
    r0 = numpy.linalg.norm(numpy.asarray(host.assemble_residual({'u': numpy.nan_to_num(cons['u'])})).ravel()[free])
    lmin = numpy.linalg.eigvalsh(K[free][:, free])[0]
    dist = numpy.linalg.norm((x - y).ravel()[free])
    print(f'{it} iterations; |x_amg - x_diag| = {dist:.3e}, bound {2 * rtol * r0 * (1 + 1e-3) / lmin:.3e}')
    assert lmin > 0 and dist <= 2 * rtol * r0 * (1 + 1e-3) / lmin
    again = jac._with_values(jac.triplet()[0] * 2.)  # the Jacobian of a next Newton step: new values on the same index tensors
    rhs = numpy.random.default_rng(15).normal(size=jac.shape[0])
    args = dict(solver='cg', precon='amg', rtol=rtol, constrain=~free)
    z = again.solve(rhs, preconargs=preconargs, **args)
    it_cheb = again.iterations
    assert len(calls) == 1 and again._hostcsr is None
    assert numpy.linalg.norm((rhs - 2 * (K @ z))[free]) <= rtol * numpy.linalg.norm(rhs[free]) * (1 + 1e-3)
    again.solve(rhs, preconargs=dict(coarse=64), **args)  # (the smoother belongs to the numeric phase)
    print(f're-valued: Chebyshev degree 2: {it_cheb} iterations, Jacobi: {again.iterations}')
    assert len(calls) == 1 and it_cheb <= again.iterations
