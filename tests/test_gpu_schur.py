'''The block preconditioner for saddle-point systems on the GPU (matrix.HipMatrix.getprecon('schur'), solve(solver='fgmres', precon=M), nh_csr_schur_diagonal,
nh_schur_apply, nh_fgmres_iterate_schur): the SIMPLE diagonal against a longdouble evaluation, one application byte for byte against its composition from
public pieces, one flexible cycle looked at after every step, the solve contract with step counts against the numpy restatement of tests/test_schur_host.py
and against the device's own unpreconditioned GMRES, a lagged object, the grid caps, and a Taylor-Hood Stokes problem through solver.System.

Sizes: 160 rows ('saddle': one vector workgroup, a random B), 183 ('stokes8x7'), 751 ('stokes16x15': three vector workgroups, the last one partial),
266 667 ('large': more rows than the 262 144 a vector grid at its cap covers at once).'''
import functools
import types
import numpy
import pytest
import scipy.sparse

import test_gpu_fgmres_amg
import test_schur_host
from test_gmres_host import ST_FULL
from test_gpu_bicgstab import hip, U
from test_gpu_cg import same_bytes
from test_schur_host import RTOL, RESTART, COARSE

pytestmark = pytest.mark.gpu

ld = numpy.longdouble


# ---- problems ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def problem(name):
    '''test_schur_host.problem with the matrix on the device: A (a HipMatrix on device tensors), ref (its host twin), kwargs (constrain), coarse.  Made once.'''
    from nutils_amd import matrix
    p = types.SimpleNamespace(**vars(test_schur_host.problem(name)))
    p.ref, p.A, p.kwargs = p.K, hip(p.K), dict(constrain=p.cons)
    p.coarse = 256 if name == 'large' else COARSE
    assert isinstance(p.A, matrix.HipMatrix) and p.A._hostcsr is None
    return p


@functools.lru_cache(maxsize=None)
def precon(name):
    '''the 'schur' object of a problem with the SIMPLE diagonal; built once'''
    p = problem(name)
    return p.A.getprecon('schur', constrain=p.cons, second=p.second, first=dict(coarse=p.coarse))


def solve(A, rhs, M, iterated=True, **kwargs):
    '''A.solve(solver='fgmres', precon=M) that insists on the device route and on the entry point of the block preconditioner'''
    from nutils_amd import _lib
    with _lib.trace() as calls:
        try:
            return A.solve(rhs, solver='fgmres', precon=M, **kwargs)
        finally:
            assert 'nh_gmres_init' in calls and ('nh_fgmres_iterate_schur' in calls) == iterated and 'nh_fgmres_iterate' not in calls and 'nh_gmres_iterate' not in calls, sorted(set(calls))
            assert not {'nh_segment_dot', 'nh_amg_create', 'nh_schur_create', 'nh_csr_schur_diagonal', 'nh_csr_transpose'} & set(calls)  # the object is ready: no setup
            assert A._hostcsr is None  # neither values nor indices went to the host


def contract(p, x, ref=None):
    '''what a solve to RTOL promises: held dofs exactly, the true residual on the free dofs within the bound'''
    ref = p.ref if ref is None else ref
    assert isinstance(x, numpy.ndarray) and numpy.array_equal(x[~p.free], p.start[~p.free])
    r0 = numpy.linalg.norm((p.rhs - ref @ p.start)[p.free])
    res = numpy.linalg.norm((p.rhs - ref @ x)[p.free])
    print(f'|r| / |r0| = {res / r0:.3e}')
    assert res <= RTOL * r0 * (1 + 1e-3)


# ---- 1. the SIMPLE diagonal -------------------------------------------------------------------------------------------------

def diagonal_inputs(p, first):
    '''(vt, dinv) on the device for a matrix and a mask of the first field: the values of the transpose by the device's own transpose, 1 / diag on the mask'''
    from nutils_amd import device
    vt, rowptr_t, colidx_t = p.A.T.triplet()
    assert bool((rowptr_t == p.A.triplet()[1]).all()) and bool((colidx_t == p.A.triplet()[2]).all())
    d = p.ref.diagonal()
    dinv = numpy.where(first, 1 / numpy.where(d == 0, 1., d), 0.)
    assert same_bytes(device.to_host(vt), scipy.sparse.csr_matrix(p.ref.T).sorted_indices().data)
    return vt, dinv


@pytest.mark.parametrize('narrow', [True, False], ids=['int32', 'int64'])
@pytest.mark.parametrize('lanes', [4, 64])
@pytest.mark.parametrize('name', ['saddle', 'stokes16x15'])
def test_simple_diagonal(name, lanes, narrow):
    '''nh_csr_schur_diagonal on every row against out_i = K_ii - sum over the entries k of row i with first[col_k] of v_k vt_k dinv[col_k] in longdouble, dinv as
    the kernel is given it.  The bound is derived: a term is two rounded products (or one and a fused multiply-add); the terms of a row, at most m_i of them with
    the diagonal entry, are added in some order, each taking part in at most m_i - 1 additions; one subtraction: (m_i + 2) u sum |terms_i| to first order.'''
    from nutils_amd import device, kernels
    p = problem(name)
    n = p.ref.shape[0]
    values, rowptr, colidx = p.A.triplet()
    vt, dinv = diagonal_inputs(p, p.f1)
    out = kernels.csr_schur_diagonal(values, rowptr, colidx, n, vt, device.to_dev(p.f1, 'uint8'), device.to_dev(dinv, 'float64'),
                                     col32=kernels.csr_compact(colidx, n) if narrow else None, lanes=lanes)
    out = device.to_host(out)
    coo = p.ref.tocoo()  # (in the order of the value array)
    terms = numpy.where(p.f1[coo.col], p.ref.data.astype(ld) * scipy.sparse.csr_matrix(p.ref.T).sorted_indices().data.astype(ld) * dinv[coo.col].astype(ld), 0)
    exact, size = p.ref.diagonal().astype(ld), numpy.abs(p.ref.diagonal()).astype(ld)
    numpy.subtract.at(exact, coo.row, terms)
    numpy.add.at(size, coo.row, numpy.abs(terms))
    m = numpy.diff(p.ref.indptr)
    bound = ((m + 2) * U * size).astype(float)
    err = numpy.abs(out - exact).astype(float)
    print(f'{name}, lanes {lanes}, {"int32" if narrow else "int64"}: max error / bound = {(err / numpy.maximum(bound, 1e-300)).max():.3f}, rows of at most {m.max()} entries')
    assert (err <= bound).all() and bound[p.f2].all()
    # what the object holds is this diagonal, read on the second field's free dofs: the same bytes at the matrix's own lanes and columns
    M = precon(name)
    own = device.to_host(kernels.csr_schur_diagonal(values, rowptr, colidx, n, vt, M.schur.mask1, M.hierarchy.data[0].dinv, col32=p.A._columns(), lanes=p.A.lanes))
    sinv = device.to_host(M.schur.sinv)
    assert same_bytes(sinv[p.f2], 1 / own[p.f2]) and not sinv[~p.f2].any() and same_bytes(device.to_host(M.hierarchy.data[0].dinv), dinv)
    assert numpy.abs(own - test_schur_host.simple_diagonal(p.ref, p.f1))[p.f2].max() <= 1e-13 * numpy.abs(own[p.f2]).max()


def test_simple_diagonal_edges():
    '''A row of the second field without an entry in the first field gives K_ii exactly; repeated calls give the same bytes; a pattern that is not structurally
    symmetric raises and names the way out.'''
    from nutils_amd import device, kernels, matrix
    base = test_schur_host.problem('saddle')
    K = scipy.sparse.csr_matrix(base.K + scipy.sparse.diags(numpy.where(base.second, -.25, 0.)))
    K.sort_indices()
    assert K.nnz == base.K.nnz + 40
    p = types.SimpleNamespace(ref=K, A=hip(K))
    row = 130
    first = base.f1.copy()
    first[K.indices[K.indptr[row]:K.indptr[row + 1]]] = False
    assert base.f2[row] and first.sum() < base.f1.sum() and K.indptr[row + 1] - K.indptr[row] > 2
    vt, dinv = diagonal_inputs(p, first)
    values, rowptr, colidx = p.A.triplet()
    args = values, rowptr, colidx, 160, vt, device.to_dev(first, 'uint8'), device.to_dev(dinv, 'float64')
    out = device.to_host(kernels.csr_schur_diagonal(*args, lanes=4))
    assert out[row] == -.25 and (out[base.f2] < -.25).sum() >= 30  # (the others have their sum subtracted)
    for lanes in (4, 64):
        assert same_bytes(device.to_host(kernels.csr_schur_diagonal(*args, lanes=lanes)), device.to_host(kernels.csr_schur_diagonal(*args, lanes=lanes)))
    # an entry of B^T without its twin in B
    coo = base.K.tocoo()
    drop = numpy.flatnonzero((coo.row == row) & base.f1[coo.col])[0]
    keep = numpy.arange(coo.nnz) != drop
    lopsided = hip(scipy.sparse.csr_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), coo.shape))
    with pytest.raises(matrix.MatrixError, match='not structurally symmetric: pass .* schur='):
        lopsided.getprecon('schur', constrain=base.cons, second=base.second, first=dict(coarse=COARSE))
    M = lopsided.getprecon('schur', constrain=base.cons, second=base.second, first=dict(coarse=COARSE), schur=numpy.full(160, -2.))  # the way out
    assert M.kind == 'schur'
    with pytest.raises(matrix.MatrixError, match='zero or non-finite'):  # a device tensor is looked at on the device
        lopsided.getprecon('schur', constrain=base.cons, second=base.second, first=dict(coarse=COARSE), schur=device.to_dev(numpy.where(numpy.arange(160) == row, 0., -2.), 'float64'))


# ---- 2. one application, byte for byte ---------------------------------------------------------------------------------------------

def composition(p, M, r):
    '''M(r) from public pieces: numpy sinv * r, the masked product of the matrix, the 'amg' object of the first block, the sum'''
    from nutils_amd import device
    sinv = device.to_host(M.schur.sinv)
    z2 = sinv * r
    t = p.A.spmv(device.to_dev(z2, 'float64'), alpha=-1., beta=1., b=device.to_dev(r, 'float64'), rowmask=device.to_dev(p.f1, 'uint8'))
    M1 = p.A.getprecon('amg', constrain=~p.f1, symmetric=False, coarse=p.coarse)
    return device.to_host(M1(t)) + z2


def application(p, M):
    from nutils_amd import device
    n = len(p.rhs)
    r = numpy.random.default_rng(17).normal(size=n)  # (entries on held dofs too)
    expect = composition(p, M, r)
    z = M(r)
    assert isinstance(z, numpy.ndarray) and same_bytes(z, expect)
    assert not z[~p.free].any() and z[p.f1].all() and z[p.f2].all()
    r_dev = device.to_dev(r, 'float64')
    z_dev = M(r_dev)
    assert z_dev.is_cuda and same_bytes(device.to_host(z_dev), expect) and same_bytes(device.to_host(r_dev), r)  # device in, device out; r is not written
    # r is not read on held dofs
    poisoned = numpy.where(p.free, r, numpy.nan)
    assert same_bytes(M(poisoned), expect)
    return expect


@pytest.mark.parametrize('name', ['saddle', 'stokes8x7', 'stokes16x15'])
def test_application(name):
    '''M(r) for a random r has the bytes of its composition; so has the object built on a diagonal the user gives, as a host array and as a device tensor'''
    from nutils_amd import device
    p, M = problem(name), precon(name)
    assert (M.kind, M.symmetric, M.shape) == ('schur', False, p.A.shape) and numpy.array_equal(M.free, p.free) and M.values is p.A.triplet()[0]
    assert numpy.array_equal(device.to_host(M.mask) != 0, p.free) and numpy.array_equal(device.to_host(M.schur.mask1) != 0, p.f1)
    z = application(p, M)
    shat = numpy.random.default_rng(18).uniform(-2., -1., size=len(p.rhs))
    shat[~p.f2] = numpy.nan  # read on the second field's free dofs only
    for given in (shat, device.to_dev(shat, 'float64')):
        N = p.A.getprecon('schur', constrain=p.cons, second=numpy.flatnonzero(p.second), schur=given, first=dict(coarse=p.coarse))  # (`second` as indices)
        assert same_bytes(device.to_host(N.schur.sinv), numpy.where(p.f2, 1 / numpy.where(p.f2, shat, 1.), 0.))
        y = application(p, N)
        assert not same_bytes(y, z)


# ---- 3. one flexible cycle, read after every step ------------------------------------------------------------------------------------

class Device(test_gpu_fgmres_amg.Device):
    '''the vectors and the work array of a flexible cycle on the device, stepped by nh_fgmres_iterate_schur'''

    def iterate(self, niter, stop_rr):
        from nutils_amd import kernels
        kernels.fgmres_iterate_schur(self.values, self.rowptr, self.colidx, self.n, rowmask=self.mask, schur=self.M.schur.handle, V=self.V, Z=self.Z, z=self.z,
                                     t=self.t, w=self.w, work=self.work, restart=self.m, stop_rr=stop_rr, niter=niter, col32=self.col32)


def test_one_cycle():
    '''a cycle of 30 steps on the 751 rows, read after every step: column j of Z has the bytes of M(V_j); the estimates never rise by more than the factor
    1 + 4 u of tests/test_gpu_gmres.py; steps enqueued past the end of the cycle move no byte of V, Z, z, w or the cells; the update leaves the held dofs alone
    and its true residual is the estimate'''
    from nutils_amd import device
    p, M = problem('stokes16x15'), precon('stokes16x15')
    m, n = RESTART, len(p.rhs)
    dev = Device(p, M, m)
    estimates = [dev.head()[0]]
    for j in range(m):
        dev.iterate(1, 0.)
        est, flag, count, st = dev.head()
        assert (flag, count, st) == (0, j + 1, ST_FULL if j == m - 1 else 0)
        estimates.append(est)
        assert same_bytes(device.to_host(dev.Z[j * n:(j + 1) * n]), device.to_host(M(dev.V[j * n:(j + 1) * n])))
        assert bool(dev.Z[(j + 1) * n:].isnan().all())  # nothing beyond column j was touched
    print(' '.join(f'{e:.2e}' for e in estimates))
    assert all(b <= a * (1 + 4 * U) for a, b in zip(estimates, estimates[1:]))
    assert estimates[-1] < .5 * estimates[0]  # (and they do fall)
    before = dev.state()
    for name in ('V', 'Z'):
        assert not before[name][:m][:, ~p.free].any() and not numpy.isnan(before[name][:m]).any()
    dev.iterate(3, 0.)
    after = dev.state()
    for name in before:
        assert same_bytes(before[name], after[name]), name
    dev.update()
    x = dev.state()['x']
    assert numpy.array_equal(x[~p.free], p.start[~p.free]) and not numpy.array_equal(x, p.start)
    true = numpy.linalg.norm(numpy.where(p.free, p.rhs - p.ref @ x, 0.))
    print(f'estimate {estimates[-1] ** .5:.6e}, true residual {true:.6e}')
    assert abs(true - estimates[-1] ** .5) <= 1e-10 * estimates[0] ** .5


# ---- 4. solves ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['saddle', 'stokes16x15'])
def test_solve(name):
    '''the contract of tests/test_gpu_fgmres_amg.py; steps within 1.1 x + 2 of the restatement's; at most a quarter of the steps of the device's own GMRES
    without a preconditioner (whose maxiter is capped just above four times the count: reaching the cap is more steps still); a repeat and a look after every
    step return the same bytes; a maxiter between two looks raises with the exact count'''
    from nutils_amd import matrix
    p, M = problem(name), precon(name)
    x = solve(p.A, p.rhs, M, rtol=RTOL, restart=RESTART, **p.kwargs)
    contract(p, x)
    steps, it_ref = p.A.iterations, test_schur_host.reference_steps(name)
    print(f'{name}: levels of the first block {[lv.nfree for lv in M.hierarchy.levels]}, {steps} steps on the device, {it_ref} in numpy')
    assert 0 < steps <= 1.1 * it_ref + 2
    assert same_bytes(solve(p.A, p.rhs, M, rtol=RTOL, restart=RESTART, **p.kwargs), x) and p.A.iterations == steps
    assert same_bytes(solve(p.A, p.rhs, M, rtol=RTOL, restart=RESTART, check=1, **p.kwargs), x) and p.A.iterations == steps
    cap = 4 * steps + 8
    try:
        p.A.solve(p.rhs, solver='fgmres', precon=None, rtol=RTOL, restart=RESTART, maxiter=cap, **p.kwargs)
    except matrix.ToleranceNotReached:
        assert p.A.iterations == cap
    print(f'{name}: GMRES({RESTART}) without a preconditioner {p.A.iterations} steps' + (' (the cap)' if p.A.iterations == cap else ''))
    assert 4 * steps <= p.A.iterations
    with pytest.raises(matrix.ToleranceNotReached) as info:
        solve(p.A, p.rhs, M, rtol=RTOL, restart=RESTART, maxiter=13, check=16, **p.kwargs)
    assert p.A.iterations == 13 and numpy.isfinite(info.value.best).all() and numpy.array_equal(info.value.best[~p.free], p.start[~p.free])
    res = numpy.linalg.norm((p.rhs - p.ref @ info.value.best)[p.free])
    assert RTOL * p.r0 < res < p.r0  # (thirteen steps got somewhere, not there)


def test_solve_on_device_vectors_and_refusals():
    from nutils_amd import device, matrix
    p, M = problem('saddle'), precon('saddle')
    x = solve(p.A, p.rhs, M, rtol=RTOL, **p.kwargs)
    xd = solve(p.A, device.to_dev(p.rhs, 'float64'), M, rtol=RTOL, **p.kwargs)
    assert xd.is_cuda and same_bytes(device.to_host(xd), x)
    done = solve(p.A, p.rhs, M, iterated=False, atol=2 * RTOL * p.r0, constrain=p.cons, lhs0=x)
    assert p.A.iterations == 0 and same_bytes(done, x)
    with pytest.raises(matrix.MatrixError, match='symmetric=False'):
        p.A.solve(p.rhs, solver='cg', precon=M, rtol=RTOL, **p.kwargs)
    for solver in ('bicgstab', 'minres'):
        with pytest.raises(matrix.MatrixError, match="'fgmres'"):
            p.A.solve(p.rhs, solver=solver, precon=M, rtol=RTOL, **p.kwargs)
    with pytest.raises(matrix.MatrixError, match='another set of free dofs'):
        p.A.solve(p.rhs, solver='fgmres', precon=M, rtol=RTOL)
    with pytest.raises(matrix.MatrixError, match='diagonal has zero entries'):  # what the saddle point does to the preconditioners there were
        p.A.solve(p.rhs, solver='fgmres', precon='diag', rtol=RTOL, **p.kwargs)


# ---- 5. a lagged object --------------------------------------------------------------------------------------------------------------

def perturbed(p):
    '''the values of p.ref with its first block changed to 1.05 A + 0.03 diag(A) (a Jacobian one step on, with a little more mass): on the same pattern'''
    coo = p.ref.tocoo()
    block = ~p.second[coo.row] & ~p.second[coo.col]
    return p.ref.data * numpy.where(block, numpy.where(coo.row == coo.col, 1.08, 1.05), 1.)


@pytest.mark.parametrize('name', ['saddle', 'stokes8x7', 'stokes16x15'])
def test_lagged_object(name):
    '''the object of K on K' = K._with_values(...) with the first block perturbed: the contract on K', within 1.5 x + 2 of the steps with the object of K' itself,
    the bar of tests/test_gpu_fgmres_amg.py for lagged 'amg' objects (the restatement: 51 / 49, 44 / 34, 86 / 64).  The symbolic phase and the transpose's plan
    are handed on: the second object is built without either.'''
    from nutils_amd import device, _lib
    p, M = problem(name), precon(name)
    data = perturbed(p)
    ref = scipy.sparse.csr_matrix((data, p.ref.indices, p.ref.indptr), p.ref.shape)
    A2 = p.A._with_values(device.to_dev(data, 'float64'))
    assert A2._amg is p.A._amg and A2._tplan is p.A._tplan and A2._tplan is not None
    with _lib.trace() as calls:
        M2 = A2.getprecon('schur', constrain=p.cons, second=p.second, first=dict(coarse=p.coarse))
    assert 'nh_csr_transpose' not in calls and 'nh_csr_schur_diagonal' in calls and 'nh_schur_create' in calls and A2._amg is p.A._amg
    x = solve(A2, p.rhs, M2, rtol=RTOL, restart=RESTART, **p.kwargs)
    contract(p, x, ref)
    own = A2.iterations
    y = solve(A2, p.rhs, M, rtol=RTOL, restart=RESTART, **p.kwargs)
    contract(p, y, ref)
    print(f'{name}: lagged {A2.iterations} steps, own {own}')
    assert A2.iterations <= 1.5 * own + 2


# ---- 6. the grid caps --------------------------------------------------------------------------------------------------------------

def test_grid_caps():
    '''266 667 rows: the vector kernels of the application stride past their grid cap.  The byte identity of one application and the solve contract.'''
    p, M = problem('large'), precon('large')
    assert p.A.shape[0] == 266667 > 1024 * 256 and len(M.hierarchy.levels) >= 5
    application(p, M)
    x = solve(p.A, p.rhs, M, rtol=RTOL, restart=RESTART, **p.kwargs)
    contract(p, x)
    print(f'{p.A.iterations} steps')
    assert 0 < p.A.iterations <= 60


# ---- 7. through solver.System ---------------------------------------------------------------------------------------------------------

def test_system(monkeypatch):
    '''The lid-driven Stokes problem on 8 x 8 Taylor-Hood elements (a vector u of degree 2, p of degree 1, 659 dofs; u held on the boundary, one pressure dof
    held) under matrix.backend('hip'): the Jacobian stays in HBM, the object is built on it with `trialmask('p')` and the component indicators of u as the
    near-nullspace of the first block, and goes to the solve through `linargs`.  Against the host route (a direct solve) within |r| / sigma_min, the comparison
    of tests/test_gpu_fgmres_amg.py.'''
    from nutils_amd import function, matrix, mesh, _lib
    from nutils_amd.solver import System
    from test_gpu_system_device import device_route_only
    ne = 8
    domain, geom = mesh.unitsquare(ne, 'square')
    u, v = (domain.field(name, btype='std', degree=2, shape=(2,)) for name in 'uv')
    pr, q = (domain.field(name, btype='std', degree=1) for name in 'pq')
    grad = lambda w: function.grad(w, geom)
    res = domain.integral(((grad(v) * grad(u)).sum(-1).sum(-1) - function.div(v, geom) * pr - q * function.div(u, geom)) * function.J(geom), degree=4)
    nn = 2 * ne + 1
    ucons = numpy.full((nn, nn, 2), numpy.nan)
    ucons[0] = ucons[-1] = ucons[:, 0] = 0.
    ucons[:, -1] = 0., 0.
    ucons[1:-1, -1, 0] = 1.  # the lid
    pcons = numpy.full((ne + 1) ** 2, numpy.nan)
    pcons[0] = 0.
    cons = {'u': ucons.reshape(-1, 2), 'p': pcons}
    host = System(res, trial='u,p', test='v,q')
    assert host.size == 659 and host.is_linear
    expect = host.solve(constrain=cons)
    packed, free = host._pack({}, cons)
    with matrix.backend('hip'):
        dev = System(res, trial='u,p', test='v,q')
        jac = dev.assemble_jacobian({})
        assert isinstance(jac, matrix.HipMatrix)
        pmask = dev.trialmask('p')
        B = numpy.zeros((dev.size, 2))
        B[:dev.offsets[1]] = numpy.tile(numpy.eye(2), (nn * nn, 1))
        M = jac.getprecon('schur', constrain=~free, second=pmask, first=dict(coarse=COARSE, nullspace=B))
        with device_route_only(monkeypatch) as lengths, _lib.trace() as calls:
            got = dev.solve(constrain=cons, linargs=dict(solver='fgmres', precon=M, rtol=1e-10))
        again = dev._device_jac[1]
    assert 'nh_fgmres_iterate_schur' in calls and 'nh_fgmres_iterate' not in calls and 'nh_gmres_iterate' not in calls and 'nh_schur_create' not in calls
    assert isinstance(again, matrix.HipMatrix) and again._hostcsr is None
    assert len(dev.linear_iterations) == 1 and dev.linear_iterations[0] == again.iterations > 0
    print(f'{dev.size} dofs, nnz {again.nnz}, levels of the first block {[lv.nfree for lv in M.hierarchy.levels]}: {again.iterations} steps; lengths that came to the host {sorted(set(lengths))}')
    assert lengths and max(lengths) <= dev.size < again.nnz
    assert M.hierarchy.levels[0].k == 2 and int(M.free.sum()) == int(free.sum())
    x = numpy.concatenate([numpy.asarray(got[t]).ravel() for t in ('u', 'p')])
    y = numpy.concatenate([numpy.asarray(expect[t]).ravel() for t in ('u', 'p')])
    assert numpy.array_equal(x[~free], y[~free]) and numpy.array_equal(x[~free], packed[~free])
    K = host.assemble_jacobian({}).export('dense')
    assert not K.diagonal()[pmask].any()  # the zero block
    r = numpy.linalg.norm(numpy.asarray(host.assemble_residual({t: got[t] for t in ('u', 'p')})).ravel()[free])
    smin = numpy.linalg.svd(K[free][:, free], compute_uv=False)[-1]
    err = numpy.linalg.norm((x - y)[free])
    print(f'|x_dev - x_host| = {err:.3e}, |r| / smin = {r / smin:.3e}')
    assert smin > 0 and err <= r / smin
