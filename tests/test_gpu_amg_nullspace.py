'''The AMG preconditioner with a user-given near-nullspace (preconargs=dict(nullspace=B), nutils_amd/amg.py, nh_aggregate_qr of nh_amg.hip) on the GPU,
against the numpy restatement of tests/test_amg_nullspace_host.py: the QR kernel alone on synthetic member lists, the numeric setup level by level, one
cycle against the restatement in longdouble, the solve contract and the iteration counts on elasticity with the rigid-body modes, dropped columns and the
diagonal terminal level, and solver.System with the plan cache.

Every tolerance on values is measured the way test_cycle of tests/test_gpu_amg.py measures its own: the distance of the float64 restatement from the longdouble
one on the same input, times 8 -- another order of summation gives an error of that size.

Problems: 2-D elasticity on 48 x 48 perturbed quadrilaterals (workloads.quad_form, 4802 dofs, three levels with coarse=64) and 3-D elasticity on 8^3 perturbed
hexahedra (workloads.hex1_form, 2187 dofs), one face held; the 40 x 37 Laplace of tests/test_gpu_cg.py with B = [1, x, y]; the chains of tests/test_gpu_amg.py
and tests/test_amg_host.py with B = [1, x].'''
import functools
import numpy
import pytest
import scipy.sparse

from test_amg_host import cycle, pcg_reference, hierarchy as constant_hierarchy, problem as scalar_problem
from test_amg_nullspace_host import aggregate_qr, level, hierarchy, vertices, ld
from test_gpu_cg import hip, problem, contract, same_bytes, RTOL
from test_gpu_amg import chain, download, solve

pytestmark = pytest.mark.gpu


# ---- problems ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def elasticity(d):
    '''(A on the device, its host twin, constraints, right-hand side, free mask, start vector, |r0|, the rigid-body modes, node coordinates) of 2-D elasticity on
    48 x 48 quadrilaterals or 3-D on 8^3 hexahedra, the face x = 0 held.  Made once, never written.'''
    from nutils_amd import amg, device, function, matrix, sample, workloads
    shape = (48, 48) if d == 2 else (8, 8, 8)
    if d == 2:
        A = function.eval(function.as_matrix(workloads.quad_form(shape, 'std', 1, 2)))
    else:
        values, rowptr, colidx, ncols = sample._MatrixPlan(workloads.hex1_form(shape)).run({})
        A = matrix.HipMatrix(values, rowptr, colidx, ncols)
    assert isinstance(A, matrix.HipMatrix) and A._hostcsr is None
    values, rowptr, colidx = (device.to_host(t) for t in A.triplet())
    ref = scipy.sparse.csr_matrix((values, colidx, rowptr), A.shape)
    coords = vertices(shape)
    cons = numpy.full([n + 1 for n in shape] + [d], numpy.nan)
    cons[0] = 0.
    cons = cons.ravel()
    free = numpy.isnan(cons)
    rhs = numpy.random.default_rng(4).normal(size=len(cons))
    start = numpy.where(free, 0., cons)
    return A, ref, cons, rhs, free, start, numpy.linalg.norm((rhs - ref @ start)[free]), amg.rigid_body_modes(coords), coords


def system(name):
    '''(A, ref, constrain, rhs, free, start, r0, B) of 'quad' and 'hex' (elasticity, the rigid-body modes), 'wide' (the Laplace, B = [1, x, y]), 'chain' and
    'orphan' (B = [1, x])'''
    if name in ('quad', 'hex'):
        return elasticity(2 if name == 'quad' else 3)[:8]
    if name == 'wide':
        A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
        x, y = numpy.meshgrid(numpy.linspace(0, 1, 40), numpy.linspace(0, 2, 37), indexing='ij')
        return A, ref, kwargs['constrain'], rhs, free, start, r0, numpy.stack([numpy.ones(1480), x.ravel(), y.ravel()], 1)
    if name == 'chain':
        A, ref, cons, rhs, free, start, r0 = chain()
    else:
        A, ref, cons, rhs, free, start, r0 = orphan()
    n = len(rhs)
    return A, ref, cons, rhs, free, start, r0, numpy.stack([numpy.ones(n), numpy.arange(n) / n], 1)


@functools.lru_cache(maxsize=None)
def orphan():
    ref, free = scalar_problem('orphan')
    cons = numpy.where(free, numpy.nan, 2.)
    rhs = numpy.random.default_rng(4).normal(size=len(cons))
    start = numpy.where(free, 0., cons)
    return hip(ref), ref, cons, rhs, free, start, numpy.linalg.norm((rhs - ref @ start)[free])


@functools.lru_cache(maxsize=None)
def device_hierarchy(name, coarse):
    '''(amg.Hierarchy, its levels downloaded as the restatement's namespaces with B and Q beside: the same values, for `cycle` and `level`)'''
    from nutils_amd import amg, device
    A, ref, cons, rhs, free, start, r0, B = system(name)
    values, rowptr, colidx = A.triplet()
    h = amg.Hierarchy(amg.symbolic(rowptr, colidx, device.to_dev(free, 'uint8') != 0, coarse, B.shape[1]), values, 1, device.to_dev(B.ravel(), 'float64').reshape(B.shape))
    levels = download(h)
    for ns, lv, d in zip(levels, h.levels, h.data):
        ns.B, ns.nodesize = device.to_host(d.B), lv.nodesize
        if lv.kind == 'coarsen':
            ns.Q = device.to_host(d.q)
    return h, levels


@functools.lru_cache(maxsize=None)
def reference_iterations(name, coarse, constant=False):
    '''iterations of the restatement's AMG-CG on the restatement's own hierarchy, looking at the residual after every iteration; the level sizes and kinds'''
    A, ref, cons, rhs, free, start, r0, B = system(name)
    ref = scipy.sparse.csr_matrix(ref)
    ref.sort_indices()
    levels = constant_hierarchy(ref, free, coarse) if constant else hierarchy(ref, free, B, coarse)
    x, it, starts, outcome = pcg_reference(ref, rhs, start, free, lambda r: cycle(levels, r), (RTOL * r0) ** 2, int(free.sum()))
    assert outcome == 'converged'
    return it, [lv.nfree for lv in levels], [lv.kind for lv in levels]


def residual_contract(name, x):
    A, ref, cons, rhs, free, start, r0, B = system(name)
    assert isinstance(x, numpy.ndarray) and numpy.array_equal(x[~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ x)[free])
    print(f'{name}: |r| / |r0| = {res / r0:.3e}')
    assert res <= RTOL * r0 * (1 + 1e-3)


def within(what, got, r64, exact):
    '''|got - exact| <= 8 |r64 - exact| in the maximum norm, r64 and exact the restatement in float64 and in longdouble'''
    d64 = float(numpy.abs(r64 - exact).max(initial=0))
    dist = float(numpy.abs(got - exact).max(initial=0))
    print(f'{what}: |float64 restatement - longdouble| = {d64:.3e}, |device - longdouble| = {dist:.3e}, largest entry {float(numpy.abs(exact).max(initial=0)):.3e}')
    assert dist <= 8 * d64, what


# ---- 1. nh_aggregate_qr alone ------------------------------------------------------------------------------------------------

def members(sizes, rng, spare):
    '''(mptr, midx, n): aggregates of the given sizes on rows scattered over n = sum + spare rows, ascending within an aggregate; `spare` rows are in none'''
    n = int(numpy.sum(sizes)) + spare
    mptr = numpy.r_[0, numpy.cumsum(sizes)].astype(numpy.int64)
    midx = rng.permutation(n)[:mptr[-1]]
    if len(sizes) < 1000:
        for a in range(len(sizes)):
            midx[mptr[a]:mptr[a + 1]].sort()
    return mptr, midx.astype(numpy.int64), n


def run_qr(mptr, midx, k, B):
    from nutils_amd import device, kernels
    args = device.to_dev(mptr, 'int64'), device.to_dev(midx.astype(numpy.int32), 'int32'), k, device.to_dev(B.ravel(), 'float64').reshape(B.shape)
    Q, Rc = (device.to_host(t) for t in kernels.aggregate_qr(*args))
    Q2, Rc2 = (device.to_host(t) for t in kernels.aggregate_qr(*args))
    assert same_bytes(Q, Q2) and same_bytes(Rc, Rc2)  # a repeat gives the same bytes
    return Q, Rc


def check_qr(what, mptr, midx, k, B, expect_dropped=None):
    from nutils_amd import kernels
    nagg = len(mptr) - 1
    Q, Rc = run_qr(mptr, midx, k, B)
    q64, r64, dropped64 = aggregate_qr(mptr, midx, k, B)
    qld, rld, dropped = aggregate_qr(mptr, midx, k, B, ld)
    print(f'{what}: k = {k}, {nagg} aggregates of {numpy.diff(mptr).min()} .. {numpy.diff(mptr).max()} rows, {kernels.csr_lanes(nagg, len(midx))} lanes each, {int(dropped.sum())} columns dropped')
    assert numpy.array_equal(dropped, dropped64)
    if expect_dropped is not None:
        assert numpy.array_equal(dropped, expect_dropped)
    assert Q.shape == B.shape and Rc.shape == (nagg * k, k)
    R = Rc.reshape(nagg, k, k)
    diagonal = numpy.diagonal(R, axis1=1, axis2=2)
    assert numpy.array_equal(diagonal == 0, dropped) and (diagonal >= 0).all()  # the same drop decisions, R[j, j] exactly 0 there
    assert not numpy.tril(R, -1).any()  # upper triangular
    outside = numpy.ones(len(B), dtype=bool)
    outside[midx] = False
    assert not Q[outside].any() and not numpy.signbit(Q[outside]).any()
    seg = numpy.repeat(numpy.arange(nagg), numpy.diff(mptr))
    assert not Q[midx][dropped[seg]].any()  # q_j exactly 0 where dropped
    within(f'{what}: Q', Q, q64, qld)
    within(f'{what}: Rc', Rc, r64, rld)


@pytest.mark.parametrize('k', [1, 2, 3, 6])
def test_aggregate_qr_sizes(k):
    '''aggregates of 1, 2, k - 1, k, k + 1, 63, 64, 65, 300 and 5000 rows side by side (rows strided over the lanes many times over next to groups whose lanes
    have no row), random normal B: an aggregate with fewer rows than columns drops the columns past its rows'''
    rng = numpy.random.default_rng(20 + k)
    sizes = numpy.tile([1, 2, k - 1, k, k + 1, 63, 64, 65, 300, 5000], 3)
    mptr, midx, n = members(sizes, rng, 500)
    B = rng.normal(size=(n, k))
    check_qr('sizes', mptr, midx, k, B, numpy.arange(k)[None, :] >= sizes[:, None])


def test_aggregate_qr_many():
    '''600 000 aggregates of 0 - 4 rows with k = 2: one lane each, more than 2048 workgroups' worth, so the grid strides'''
    from nutils_amd import kernels
    rng = numpy.random.default_rng(25)
    sizes = rng.integers(0, 5, 600000)
    mptr, midx, n = members(sizes, rng, 1000)
    assert kernels.csr_lanes(len(sizes), len(midx)) == 1 and len(sizes) / 256 > 2048
    check_qr('many', mptr, midx, 2, rng.normal(size=(n, 2)), numpy.arange(2)[None, :] >= sizes[:, None])


def test_aggregate_qr_drops():
    '''columns that must go: a repeated column, a zero column, a multiple of the sum of two others, and one-row aggregates; the coordinates far from the origin
    (the rotations of a distant aggregate are nearly translations: the case the second pass is for) must not'''
    rng = numpy.random.default_rng(26)
    sizes = numpy.tile([40, 1, 7, 40, 9], 8)
    mptr, midx, n = members(sizes, rng, 100)
    k = 4
    B = rng.normal(size=(n, k))
    seg = numpy.full(n, -1)
    seg[midx] = numpy.repeat(numpy.arange(len(sizes)), sizes)
    kind = seg % 5
    B[kind == 0, 2] = B[kind == 0, 0]  # repeated
    B[kind == 2, 1] = 0.  # zero
    B[kind == 3, 3] = 3 * (B[kind == 3, 0] + B[kind == 3, 2])  # dependent
    expect = numpy.zeros((len(sizes), k), dtype=bool)
    expect[0::5, 2] = expect[2::5, 1] = expect[3::5, 3] = True
    expect[1::5, 1:] = True
    check_qr('drops', mptr, midx, k, B, expect)
    x, first = 1e6 + rng.uniform(0, 1, (n, 2)), (numpy.arange(n) % 2 == 0)[:, None]
    B = numpy.where(first, numpy.stack([numpy.ones(n), numpy.zeros(n), -x[:, 1]], 1), numpy.stack([numpy.zeros(n), numpy.ones(n), x[:, 0]], 1))
    expect = numpy.zeros((len(sizes), 3), dtype=bool)  # only the one-row aggregates drop: the columns their row does not start
    expect[1::5] = numpy.where(first[midx[mptr[1:-1:5]]], [False, True, True], [True, False, True])
    check_qr('far', mptr, midx, 3, B, expect)


def test_aggregate_qr_argument_errors():
    from nutils_amd import device, kernels, _lib
    mptr, midx, B = device.to_dev(numpy.array([0, 2]), 'int64'), device.to_dev(numpy.array([0, 3], dtype=numpy.int32), 'int32'), device.zeros(6, 'float64').reshape(3, 2)
    with pytest.raises(ValueError, match='member rows must lie in'):
        kernels.aggregate_qr(mptr, midx, 2, B)
    with pytest.raises(ValueError, match='mptr must rise'):
        kernels.aggregate_qr(device.to_dev(numpy.array([0, 3]), 'int64'), midx, 2, B)
    with pytest.raises(_lib.NutilsHipError, match='k must be between 1 and 6'):
        _lib.call('nh_aggregate_qr', 1, device.ptr(mptr), device.ptr(midx), 2, 7, 3, device.ptr(B), device.ptr(B), device.ptr(B), device.stream())


# ---- 2. the numeric setup, level by level ----------------------------------------------------------------------------------

@pytest.mark.parametrize('name,coarse', [('quad', 64), ('wide', 16)])
def test_numeric_setup(name, coarse):
    '''Every level of the device's hierarchy against the restatement fed with the DEVICE's matrix and near-nullspace of that level (errors do not chain): the
    patterns of P, R and A_c integer-equal, the drop decisions the same; Q, P, A_c and Rc within 8 times the distance of the float64 restatement from the
    longdouble one; R is P transposed value for value.  Two builds give the same bytes.'''
    from nutils_amd import amg, device
    h, levels = device_hierarchy(name, coarse)
    print(f'{name}: levels {[lv.nfree for lv in levels]}, kinds {[lv.kind for lv in levels]}')
    assert len(levels) == (3 if name == 'quad' else 4) and levels[-1].kind == 'dense'
    for l, lv in enumerate(levels[:-1]):
        r64, exact = (level(lv.A, lv.free, coarse, lv.B, lv.nodesize, dtype) for dtype in (float, ld))
        assert r64.kind == 'coarsen' and r64.nc == lv.nc and numpy.array_equal(r64.dropped, exact.dropped)
        for got, want in ((lv.P, r64.P), (lv.R, r64.R), (levels[l + 1].A, r64.Ac)):
            assert numpy.array_equal(got.indptr, want.indptr) and numpy.array_equal(got.indices, want.indices)
        Rc = levels[l + 1].B
        assert numpy.array_equal(numpy.diagonal(Rc.reshape(-1, lv.B.shape[1], lv.B.shape[1]), axis1=1, axis2=2) == 0, exact.dropped)
        for what in ('rho', 'omega'):
            got, want = getattr(lv, what), getattr(r64, what)
            print(f'level {l}: {what} = {got!r}, {(got - want) / numpy.spacing(want):+.0f} ulp from the restatement')
            assert abs(got - want) <= 4 * numpy.spacing(want)
        within(f'level {l}: Q', lv.Q, r64.x.q, exact.x.q)
        within(f'level {l}: P', lv.P.data, r64.x.p, exact.x.p)
        within(f'level {l}: A_c', levels[l + 1].A.data, r64.x.ac, exact.x.ac)
        within(f'level {l}: Rc', Rc, r64.x.rc, exact.x.rc)
        assert numpy.array_equal(lv.R.data, lv.P.T.tocsr().data)  # R is P transposed, value for value
    A, ref, cons, rhs, free, start, r0, B = system(name)
    again = amg.Hierarchy(h.levels, A.triplet()[0], 1, device.to_dev(B.ravel(), 'float64').reshape(B.shape))
    for d, e in zip(h.data, again.data):
        for what in ('values', 'dinv', 'w', 'B', 'q', 'pvalues', 'rvalues', 'ainv'):
            if getattr(d, what, None) is not None:
                assert same_bytes(device.to_host(getattr(d, what)), device.to_host(getattr(e, what))), what


# ---- 3. one cycle ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,coarse', [('quad', 64), ('wide', 16), ('orphan', 16)])
def test_cycle(name, coarse):
    '''nh_amg_apply against the restatement's cycle in longdouble on the same hierarchy values, under the rule of test_cycle of tests/test_gpu_amg.py; 'orphan' has
    dropped columns on every level: coarse dofs with a zero row, column and weight'''
    from nutils_amd import device
    h, levels = device_hierarchy(name, coarse)
    A, ref, cons, rhs, free, start, r0, B = system(name)
    if name == 'orphan':
        assert all((lv.dinv == 0).sum() == 2 for lv in levels[1:-1])
    r = numpy.where(free, numpy.random.default_rng(13).normal(size=len(rhs)), 0.)
    exact = cycle(levels, r.astype(ld))
    d64 = float(numpy.abs(cycle(levels, r) - exact).max())
    r_dev = device.to_dev(r, 'float64')
    got = device.to_host(h.apply(r_dev))
    dist = float(numpy.abs(got - exact).max())
    print(f'{name}: {len(levels)} levels: |float64 restatement - longdouble| = {d64:.3e}, |device - longdouble| = {dist:.3e}, |z| = {float(numpy.abs(exact).max()):.3e}')
    assert d64 > 0 and dist <= 8 * d64
    assert not got[~free].any()
    assert same_bytes(got, device.to_host(h.apply(r_dev)))


# ---- 4. the solve ------------------------------------------------------------------------------------------------------------

def test_rigid_body_modes_in_the_layout_of_the_forms():
    '''the matrices of workloads.quad_form and hex1_form take amg.rigid_body_modes of their vertices to rounding: dof = node d + component, nodes with the last
    axis fastest'''
    for d in (2, 3):
        A, ref, cons, rhs, free, start, r0, B, coords = elasticity(d)
        err, scale = abs(ref @ B).max(), (abs(ref) @ abs(B)).max()
        print(f'{d}-D: |K B| = {err:.2e}, |K| |B| = {scale:.2e}')
        assert B.shape == (len(coords) * d, d * (d + 1) // 2) and err <= 64 * numpy.finfo(float).eps * scale


@pytest.mark.parametrize('name', ['quad', 'hex'])
def test_solve_contract(name):
    '''elasticity with the rigid-body modes, coarse=64: the residual contract, a repeat byte-equal, the restatement's iteration count, and at most half the
    device's own count with the constant'''
    from nutils_amd import _lib
    A, ref, cons, rhs, free, start, r0, B = system(name)
    args = dict(rtol=RTOL, constrain=cons, check=1)
    with _lib.trace() as calls:
        x = solve(A, rhs, preconargs=dict(coarse=64, nullspace=B), **args)
    it = A.iterations
    assert 'nh_aggregate_qr' in calls
    residual_contract(name, x)
    assert same_bytes(solve(A, rhs, preconargs=dict(coarse=64, nullspace=B), **args), x)
    it_ref, sizes, kinds = reference_iterations(name, 64)
    with _lib.trace() as calls:
        solve(A, rhs, preconargs=dict(coarse=64), **args)
    assert 'nh_aggregate_qr' not in calls
    print(f'{name}: levels {sizes}, {it} iterations on the device, {it_ref} in numpy, {A.iterations} on the device with the constant')
    assert it <= 1.1 * it_ref + 2
    assert 2 * it <= A.iterations


# ---- 5. rank drop and the terminal level -------------------------------------------------------------------------------------

def test_orphan():
    '''singleton aggregates with B = [1, x] drop their second column on every level: zero rows and columns of the coarse matrices, and the solve converges'''
    A, ref, cons, rhs, free, start, r0, B = system('orphan')
    x = solve(A, rhs, rtol=RTOL, constrain=cons, check=1, preconargs=dict(coarse=16, nullspace=B))
    residual_contract('orphan', x)
    it_ref, sizes, kinds = reference_iterations('orphan', 16)
    print(f'orphan: levels {sizes}, {A.iterations} iterations on the device, {it_ref} in numpy')
    assert A.iterations <= 1.1 * it_ref + 2


def test_chain():
    '''the chain of 262 444 with B = [1, x]: the held dofs cut it into 263 pieces, each of which ends as one node of two dofs: a 'diagonal' level of 526 dofs'''
    from nutils_amd import device
    A, ref, cons, rhs, free, start, r0, B = system('chain')
    x = solve(A, rhs, rtol=RTOL, constrain=cons, check=1, preconargs=dict(nullspace=device.to_dev(B.ravel(), 'float64').reshape(B.shape)))  # (a device tensor: nothing goes up)
    it = A.iterations
    residual_contract('chain', x)
    levels = A._amg[3]
    it_ref, sizes, kinds = reference_iterations('chain', 256)
    print(f'chain: levels {sizes}, {it} iterations on the device, {it_ref} in numpy')
    assert [lv.kind for lv in levels] == kinds and [lv.nfree for lv in levels] == sizes
    assert levels[-1].kind == 'diagonal' and levels[-1].n == 526 and A._amg[2] == 2
    assert it <= 1.1 * it_ref + 2


# ---- 6. solver.System and the plan cache ------------------------------------------------------------------------------------------

def test_system_and_plan_cache(monkeypatch):
    '''2-D elasticity under matrix.backend('hip') with linargs naming the preconditioner and its near-nullspace, against the 'diag' route; the symbolic phase runs
    once per pattern, mask, `coarse` and k: not for a re-valued Jacobian, again for another k'''
    from nutils_amd import amg, matrix, mesh, function, _lib
    from nutils_amd.solver import System
    nelems = 16
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1, nelems + 1)] * 2)
    u = domain.field('u', btype='std', degree=1, shape=[2])
    v = domain.field('v', btype='std', degree=1, shape=[2])
    eps = lambda w: function.symgrad(w, geom)
    res = domain.integral(function.inner(eps(v), function.div(u, geom) * function.eye(2) + 1.3 * eps(u)) * function.J(geom), degree=2)
    cons = numpy.full((nelems + 1, nelems + 1, 2), numpy.nan)
    cons[0] = 0.
    cons[-1] = [0., .05]
    cons = {'u': cons.reshape(-1, 2)}
    grid = numpy.linspace(0, 1, nelems + 1)
    B = amg.rigid_body_modes(numpy.stack(numpy.meshgrid(grid, grid, indexing='ij'), -1).reshape(-1, 2))
    calls, symbolic = [], amg.symbolic
    monkeypatch.setattr(amg, 'symbolic', lambda *args, **kwargs: calls.append(1) or symbolic(*args, **kwargs))
    rtol = 1e-10
    with matrix.backend('hip'):
        dev = System(res, trial='u', test='v')
        with _lib.trace() as trace:
            x = dev.solve(constrain=cons, linargs=dict(solver='cg', precon='amg', rtol=rtol, preconargs=dict(coarse=64, nullspace=B)))['u']
        jac = dev._device_jac[1]
        it = dev.linear_iterations[-1]
        y = System(res, trial='u', test='v').solve(constrain=cons, linargs=dict(solver='cg', precon='diag', rtol=rtol))['u']
    assert 'nh_pcg_iterate' in trace and 'nh_amg_create' in trace and 'nh_aggregate_qr' in trace and len(calls) == 1
    assert isinstance(jac, matrix.HipMatrix) and jac._hostcsr is None and jac._amg[2] == 3 and len(jac._amg[3]) >= 2
    free = numpy.isnan(cons['u']).ravel()
    assert numpy.array_equal(x.ravel()[~free], y.ravel()[~free])
    # both routes solve K x = b to |r| <= rtol |r0|: they differ by at most (|r_x| + |r_y|) / lmin <= 2 rtol |r0| / lmin
    host = System(res, trial='u', test='v')
    K = host.assemble_jacobian({}).export('dense')
    assert abs(K @ B).max() <= 64 * numpy.finfo(float).eps * (abs(K) @ abs(B)).max()  # (the layout of the field is that of the modes)
    r0 = numpy.linalg.norm(numpy.asarray(host.assemble_residual({'u': numpy.nan_to_num(cons['u'])})).ravel()[free])
    lmin = numpy.linalg.eigvalsh(K[free][:, free])[0]
    dist = numpy.linalg.norm((x - y).ravel()[free])
    print(f'{it} iterations; |x_amg - x_diag| = {dist:.3e}, bound {2 * rtol * r0 * (1 + 1e-3) / lmin:.3e}')
    assert lmin > 0 and dist <= 2 * rtol * r0 * (1 + 1e-3) / lmin
    # the Jacobian of a next Newton step: new values on the same index tensors
    again = jac._with_values(jac.triplet()[0] * 2.)
    rhs = numpy.random.default_rng(15).normal(size=jac.shape[0])
    args = dict(solver='cg', precon='amg', rtol=rtol, constrain=~free)
    z = again.solve(rhs, preconargs=dict(coarse=64, nullspace=B), **args)
    assert len(calls) == 1 and again._hostcsr is None
    assert numpy.linalg.norm((rhs - 2 * (K @ z))[free]) <= rtol * numpy.linalg.norm(rhs[free]) * (1 + 1e-3)
    again.solve(rhs, preconargs=dict(coarse=64, nullspace=B[:, :2]), **args)  # (another k is another hierarchy)
    assert len(calls) == 2
    again.solve(rhs, preconargs=dict(coarse=64, nullspace=B[:, :2] * 2.), **args)  # (other values of the same shape are not)
    assert len(calls) == 2
    again.solve(rhs, preconargs=dict(coarse=64), **args)
    assert len(calls) == 3 and again._amg[2] is None
