'''The smoothed-aggregation AMG preconditioner of the device CG solve (matrix.HipMatrix.solve(solver='cg', precon='amg'), nutils_amd/amg.py, nh_amg.hip) on the
GPU, against the numpy / scipy restatement of tests/test_amg_host.py: the kernels one by one (segment products, the Jacobi sweep), the numeric setup level by
level, one cycle against the restatement in longdouble, the solve contract and the iteration counts, the terminal levels, and solver.System with the plan
cache.

Problems: 'wide', the 40 x 37 bilinear Laplace of tests/test_gpu_cg.py with one side held (1480 rows: six vector workgroups; three levels with coarse=16), and
the chain tridiag(-1, 2, -1) of 262 444 rows with every 1000th held (the row and vector grids stride; seven levels).'''
import functools
import types
import numpy
import pytest
import scipy.sparse

from test_cg_host import gamma, U
from test_amg_host import hierarchy, level, cycle, pcg_reference, segment_dot, sample
from test_gpu_cg import hip, problem, contract, same_bytes, RTOL

pytestmark = pytest.mark.gpu

ld = numpy.longdouble


# ---- problems ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def chain(n=262444):
    '''(A on the device, its host twin, constraints, right-hand side, free mask, start vector, |r0|).  Made once, never written.'''
    ref = scipy.sparse.diags([-numpy.ones(n - 1), numpy.full(n, 2.), -numpy.ones(n - 1)], [-1, 0, 1], format='csr')
    cons = numpy.full(n, numpy.nan)
    cons[::1000] = 2.
    rhs = numpy.random.default_rng(4).normal(size=n)
    free = numpy.isnan(cons)
    start = numpy.where(free, 0., cons)
    return hip(ref), ref, cons, rhs, free, start, numpy.linalg.norm((rhs - ref @ start)[free])


def system(name):
    '''(A, ref, constrain, rhs, free, start, r0) of 'wide' or 'chain' '''
    if name == 'chain':
        return chain()
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    return A, ref, kwargs['constrain'], rhs, free, start, r0


@functools.lru_cache(maxsize=None)
def device_hierarchy(name, coarse):
    '''(amg.Hierarchy, its levels downloaded as the restatement's namespaces: the same values, for `cycle`)'''
    from nutils_amd import amg, device
    A, ref, cons, rhs, free, start, r0 = system(name)
    values, rowptr, colidx = A.triplet()
    h = amg.Hierarchy(amg.symbolic(rowptr, colidx, device.to_dev(free, 'uint8') != 0, coarse), values)
    return h, download(h)


def download(h):
    from nutils_amd import device
    host = device.to_host
    csr = lambda values, colidx, rowptr, ncols: scipy.sparse.csr_matrix((host(values), host(colidx), host(rowptr)), (rowptr.numel() - 1, ncols))
    out = []
    for lv, d in zip(h.levels, h.data):
        ns = types.SimpleNamespace(A=csr(d.values, lv.colidx, lv.rowptr, lv.n), n=lv.n, nfree=lv.nfree, kind=lv.kind, dinv=host(d.dinv),
                                   free=numpy.ones(lv.n, dtype=bool) if lv.free is None else host(lv.free))
        if lv.kind == 'dense':
            ns.idx, ns.ainv = numpy.flatnonzero(ns.free), host(d.ainv).reshape(lv.nfree, lv.nfree)
        elif lv.kind == 'coarsen':
            ns.nc, ns.w, ns.rho, ns.omega = lv.nc, host(d.w), d.rho.item(), d.omega.item()
            ns.P, ns.R = csr(d.pvalues, lv.pcol, lv.prowptr, lv.nc), csr(d.rvalues, lv.rcol, lv.rrowptr, lv.n)
        out.append(ns)
    return out


@functools.lru_cache(maxsize=None)
def reference_iterations(name, coarse):
    '''iterations of the restatement's AMG-CG, on the restatement's own hierarchy, looking at the residual after every iteration'''
    A, ref, cons, rhs, free, start, r0 = system(name)
    levels = hierarchy(scipy.sparse.csr_matrix(ref), free, coarse)
    x, it, starts, outcome = pcg_reference(ref, rhs, start, free, lambda r: cycle(levels, r), (RTOL * r0) ** 2, int(free.sum()))
    assert outcome == 'converged'
    return it, [lv.nfree for lv in levels]


def solve(A, rhs, **kwargs):
    '''A.solve(solver='cg', precon='amg') that insists on the device route and on the cycle as preconditioner'''
    from nutils_amd import _lib
    with _lib.trace() as calls:
        try:
            return A.solve(rhs, solver='cg', precon='amg', **kwargs)
        finally:
            assert 'nh_pcg_iterate' in calls and 'nh_cg_iterate' not in calls and 'nh_cg_init' not in calls, sorted(set(calls))
            assert A._hostcsr is None  # neither values nor indices of the matrix went to the host


# ---- 1. nh_segment_dot ------------------------------------------------------------------------------------------------------

def plan_of(lengths, nsrc, rng):
    from nutils_amd import device
    ptr = numpy.r_[0, numpy.cumsum(lengths)].astype(numpy.int64)
    ia, ib = rng.integers(0, nsrc, ptr[-1]), rng.integers(0, nsrc, ptr[-1])
    plan = types.SimpleNamespace(ptr=device.to_dev(ptr, 'int64'), ia=device.to_dev(ia, 'int32'), ib=device.to_dev(ib, 'int32'), nseg=len(lengths), nprod=int(ptr[-1]))
    return plan, ptr, ia, ib


@pytest.mark.parametrize('name', ['mixed', 'long', 'one', 'many'])
def test_segment_dot(name):
    '''Small integers, so that float64 is exact whatever the order: byte-equal to numpy.  'mixed': lengths 0, 1, 5 and 300 side by side (16 lanes per segment: 300 is
    walked in strides); 'long': 300 throughout (32 lanes); 'one': a single segment; 'many': 600 000 short ones, more than 2048 workgroups' worth.  With and without
    the second factor; a repeat gives the same bytes.  Then random doubles against longdouble, within gamma_(len + 2) sum |terms|.'''
    from nutils_amd import device, kernels
    rng = numpy.random.default_rng(11)
    lengths = {'mixed': numpy.tile([0, 1, 5, 300, 1, 0, 5], 9), 'long': numpy.full(70, 300), 'one': numpy.array([7]), 'many': rng.integers(0, 4, 600000)}[name]
    nsrc = 5000
    plan, ptr, ia, ib = plan_of(lengths, nsrc, rng)
    if name == 'many':
        assert kernels.csr_lanes(plan.nseg, plan.nprod) == 1 and plan.nseg / 256 > 2048
    a, b = rng.integers(-8, 9, nsrc).astype(float), rng.integers(-8, 9, nsrc).astype(float)
    a_dev, b_dev = device.to_dev(a, 'float64'), device.to_dev(b, 'float64')
    for second in (b, None):
        got = device.to_host(kernels.segment_dot(plan, a_dev, None if second is None else b_dev))
        assert same_bytes(got, segment_dot(ptr, ia, ib, a, second) + 0.)  # (+ 0.: an empty segment is +0)
        assert same_bytes(got, device.to_host(kernels.segment_dot(plan, a_dev, None if second is None else b_dev)))
    a, b = rng.normal(size=nsrc), rng.normal(size=nsrc)
    got = device.to_host(kernels.segment_dot(plan, device.to_dev(a, 'float64'), device.to_dev(b, 'float64')))
    err = numpy.abs(got - segment_dot(ptr, ia, ib, a.astype(ld), b.astype(ld))).astype(float)
    bound = gamma(lengths + 2) * segment_dot(ptr, ia, ib, abs(a), abs(b))
    print(f'{name}: max error / bound = {(err / numpy.maximum(bound, 1e-300)).max():.3f}')
    assert (err <= bound).all()


# ---- 2. the Jacobi sweep ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['wide', 'chain'])
def test_jacobi_sweep(name):
    '''y = x + w (b - A x) against longdouble.  b - A x is a sum of len + 1 terms in any order: product_bound of tests/test_gpu_matrix_hip.py with one extra term and
    the tail |b|, times |w|; then the two roundings of the update, of the product w (b - A x) and of the sum.  Masked rows are exactly 0.'''
    from test_gpu_matrix_hip import product_bound
    from nutils_amd import device, kernels
    A, ref, cons, rhs, free, start, r0 = system(name)
    ref = scipy.sparse.csr_matrix(ref)
    n = len(rhs)
    rng = numpy.random.default_rng(12)
    x, b = numpy.where(free, rng.normal(size=n), 0.), rng.normal(size=n)
    w = numpy.where(free, .6 / ref.diagonal(), 0.)
    values, rowptr, colidx = A.triplet()
    run = lambda: device.to_host(kernels.csr_jacobi(values, rowptr, colidx, n, device.to_dev(x, 'float64'), device.to_dev(w, 'float64'), device.to_dev(b, 'float64'),
                                                   rowmask=device.to_dev(free, 'uint8'), col32=A._columns(), lanes=A.lanes))
    got = run()
    dense = None if name == 'chain' else ref.toarray().astype(ld)
    Ax = dense @ x.astype(ld) if dense is not None else (2 * x.astype(ld) - numpy.r_[0, x[:-1]].astype(ld) - numpy.r_[x[1:], 0].astype(ld))
    t = b.astype(ld) - Ax
    expect = numpy.where(free, x.astype(ld) + w.astype(ld) * t, 0)
    dt = product_bound(ref, x, extra=1, tail=abs(b))
    m = abs(w) * (numpy.abs(t).astype(float) + dt)
    bound = (abs(w) * dt + U * m + U * (abs(x) + m * (1 + U))) * (1 + 2. ** -10)
    err = numpy.abs(got - expect).astype(float)
    print(f'{name}: max error / bound = {(err[free] / bound[free]).max():.3f}')
    assert (err <= bound).all()
    assert not got[~free].any() and not numpy.signbit(got[~free]).any()
    assert same_bytes(got, run())


# ---- 3. the numeric setup, level by level ----------------------------------------------------------------------------------

@pytest.mark.parametrize('name,coarse', [('wide', 16), ('chain', 256)])
def test_numeric_setup(name, coarse):
    '''Every level of the device's hierarchy against the restatement fed with the DEVICE's matrix of that level (errors do not chain): the patterns of P, R
    and A_c integer-equal; rho and omega within 4 ulp.  Values twice.  Against a longdouble evaluation of the sums on what the device holds (its weights, its P
    and R; the entries of the plans are those of the patterns just compared): P within gamma_(len + 2) (|T| + |w| sum |a|) per entry, A_c = R (A P) within the bound
    of its two nested sums, gamma_(len + 2) |R| (|A P| + d) + |R| d with d = gamma_(len' + 2) |A| |P| the bound of an entry of A P -- the device's own rounding and
    nothing else.  And against the restatement's float64 P and A_c themselves: the same bounds once for the device and once for scipy, plus what the 4 ulp between
    the two omegas carry into P and, through P, into A_c.  Two builds give the same bytes.'''
    from nutils_amd import amg, device
    h, levels = device_hierarchy(name, coarse)
    print(f'{name}: levels {[lv.nfree for lv in levels]}, kinds {[lv.kind for lv in levels]}')
    # (the held dofs cut the chain into 263 pieces, each of which ends as one dof: its last level has no edges)
    assert len(levels) == (3 if name == 'wide' else 7) and levels[-1].kind == ('dense' if name == 'wide' else 'diagonal')
    for l, (lv, plan) in enumerate(zip(levels, h.levels)):
        if lv.kind != 'coarsen':
            continue
        r = level(lv.A, lv.free, coarse)
        assert r.kind == 'coarsen' and r.nc == lv.nc
        for got, want in ((lv.P, r.P), (lv.R, r.R), (levels[l + 1].A, r.Ac)):
            assert numpy.array_equal(got.indptr, want.indptr) and numpy.array_equal(got.indices, want.indices)
        for what in ('rho', 'omega'):
            got, want = getattr(lv, what), getattr(r, what)
            print(f'level {l}: {what} = {got!r}, {(got - want) / numpy.spacing(want):+.0f} ulp from the restatement')
            assert abs(got - want) <= 4 * numpy.spacing(want)
        # values: the sums of the plans (whose entries are those of the patterns just compared) in longdouble, on what the device holds of A, w, P and R
        at, ap, rap = ([device.to_host(t) for t in (p.ptr, p.ia, p.ib if p.ib is not None else p.ia)] for p in (plan.at, plan.ap, plan.rap))
        a, w, P, R = lv.A.data, lv.w[numpy.repeat(numpy.arange(lv.n), numpy.diff(r.P.indptr))], lv.P.data, lv.R.data
        T = sample(r.T, r.P)
        err = numpy.abs(P - (T - w.astype(ld) * segment_dot(at[0], at[1], None, a.astype(ld)))).astype(float)
        absAT = segment_dot(at[0], at[1], None, abs(a))
        bound = gamma(numpy.diff(at[0]) + 2) * (T + abs(w) * absAT)
        print(f'level {l}: P: max error / bound = {(err / bound).max():.3f}')
        assert (err <= bound).all()
        # against the restatement's own float64 P: the bound once for the device and once for scipy, and the weights' 4 ulp of omega (8 u) and one rounding each of omega dinv
        boundP = 2 * bound + 10 * U * abs(w) * absAT
        err = abs(P - r.P.data)
        print(f'level {l}: P against the restatement: max error / bound = {(err / boundP).max():.3f}')
        assert (err <= boundP).all()
        assert numpy.array_equal(R, lv.P.T.tocsr().data)  # R is P transposed, value for value
        AP = segment_dot(*ap, a.astype(ld), P.astype(ld))
        dAP = gamma(numpy.diff(ap[0]) + 2) * segment_dot(*ap, abs(a), abs(P))
        absAP = numpy.abs(AP).astype(float)
        err = numpy.abs(levels[l + 1].A.data - segment_dot(*rap, R.astype(ld), AP)).astype(float)
        bound = gamma(numpy.diff(rap[0]) + 2) * segment_dot(*rap, abs(R), absAP + dAP) + segment_dot(*rap, abs(R), dAP)
        print(f'level {l}: A_c: max error / bound = {(err / bound).max():.3f}')
        assert (err <= bound).all()
        # against the restatement's own float64 A_c = R' (A P') on ITS P' and R' = P'^T: the nested bound once for the device and once for scipy, and what the
        # difference dP <= boundP of the two prolongators carries into the product, |dP|^T |A| |P| + |R| |A| |dP| + |dP|^T |A| |dP|
        dP = scipy.sparse.csr_matrix((boundP, r.P.indices, r.P.indptr), r.P.shape)
        absA = abs(r.Af)
        carried = dP.T @ (absA @ abs(lv.P)) + abs(lv.R) @ (absA @ dP) + dP.T @ (absA @ dP)
        boundAc = 2 * bound + sample(carried.tocsr(), r.Ac)
        err = abs(levels[l + 1].A.data - r.Ac.data)
        print(f'level {l}: A_c against the restatement: max error / bound = {(err / boundAc).max():.3f}')
        assert (err <= boundAc).all()
    A, ref, cons, rhs, free, start, r0 = system(name)
    again = amg.Hierarchy(h.levels, A.triplet()[0])
    for d, e in zip(h.data, again.data):
        for what in ('values', 'dinv', 'w', 'pvalues', 'rvalues', 'ainv'):
            if getattr(d, what, None) is not None:
                assert same_bytes(device.to_host(getattr(d, what)), device.to_host(getattr(e, what))), what


# ---- 4. one cycle ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,coarse', [('wide', 16), ('chain', 256)])
def test_cycle(name, coarse):
    '''nh_amg_apply against the restatement's cycle in longdouble on the same hierarchy values.  The tolerance is measured: the distance (maximum norm) of the float64
    restatement from the longdouble one on the same input, times 8 -- another order of summation gives an error of that size, not of that value.'''
    from nutils_amd import device
    h, levels = device_hierarchy(name, coarse)
    A, ref, cons, rhs, free, start, r0 = system(name)
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


# ---- 5., 6. the solve --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('coarse', [256, 16])
def test_solve_contract(coarse):
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    args = dict(rtol=RTOL, preconargs=dict(coarse=coarse), **kwargs)
    x = solve(A, rhs, **args)
    contract('wide', x)
    assert same_bytes(solve(A, rhs, **args), x)
    y = solve(A, rhs, check=1, **args)
    contract('wide', y)
    it_ref, sizes = reference_iterations('wide', coarse)
    print(f'wide, coarse={coarse}: levels {sizes}, {A.iterations} iterations on the device, {it_ref} in numpy')
    assert A.iterations == A.cg_iterations <= 1.1 * it_ref + 2
    assert same_bytes(x, y)  # the iterations that check=16 enqueues past convergence do nothing


def test_chain():
    '''262 181 free dofs in seven levels: the residual contract, the iteration count of the restatement, and at most a quarter of the device's own Jacobi-CG count'''
    A, ref, cons, rhs, free, start, r0 = chain()
    x = solve(A, rhs, rtol=RTOL, constrain=cons, check=1)
    it = A.iterations
    assert numpy.array_equal(x[~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ x)[free])
    assert res <= RTOL * r0 * (1 + 1e-3)
    it_ref, sizes = reference_iterations('chain', 256)
    A.solve(rhs, rtol=RTOL, constrain=cons, check=1)
    print(f'chain: levels {sizes}, |r| / |r0| = {res / r0:.3e}, {it} iterations on the device, {it_ref} in numpy, Jacobi-CG {A.iterations}')
    assert len(sizes) == 7
    assert it <= 1.1 * it_ref + 2
    assert 4 * it <= A.iterations


# ---- 7. terminal levels and edge cases ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [700, 100])
def test_diagonal_matrix(n):
    '''more free dofs than `coarse`: a level without edges, z = dinv b; fewer: the dense level.  Either way the cycle is the inverse, and CG is there after one iteration'''
    rng = numpy.random.default_rng(14)
    d, b = rng.uniform(1, 10, n), rng.normal(size=n)
    cons = numpy.full(n, numpy.nan)
    cons[::7] = 1.
    A = hip(scipy.sparse.diags(d, format='csr'))
    x = solve(A, b, rtol=RTOL, constrain=cons, check=1)
    assert A.iterations == 1
    free = numpy.isnan(cons)
    # x = alpha M b with alpha = r . z / p . q, two sums of n positive terms that agree term by term to a few roundings (one_step_of_jacobi of test_cg_host)
    assert numpy.array_equal(x[~free], cons[~free]) and (numpy.abs(x - b / d)[free] <= (2 * gamma(n) + 8 * U) * numpy.abs(b / d)[free]).all()


def test_few_free_dofs_among_many(monkeypatch):
    '''262 444 rows of which 200 are free (the shape of the constraints projection of solver.System: the boundary support free, the rest held): level 0 is the dense
    level, the cycle is the inverse of the free block and CG is there after one iteration; what comes to the host is that block's entries, never a vector of n or
    nnz entries (the solve is given a device tensor, so the solution stays too)'''
    import scipy.sparse.linalg
    from nutils_amd import device
    A, ref, cons, rhs, free, start, r0 = chain()
    n = len(rhs)
    free = numpy.zeros(n, dtype=bool)
    free[5000:5120] = True
    free[numpy.random.default_rng(16).choice(n, 80, replace=False)] = True
    nfree = int(free.sum())
    assert nfree <= 200
    hold = numpy.where(free, numpy.nan, 1.5)
    lengths, to_host = [], device.to_host
    monkeypatch.setattr(device, 'to_host', lambda tensor: lengths.append(tensor.numel()) or to_host(tensor))
    x = solve(A, device.to_dev(rhs, 'float64'), rtol=RTOL, constrain=hold, check=1)
    monkeypatch.undo()
    print(f'{nfree} free dofs of {n}: {A.iterations} iteration(s), lengths that came to the host {sorted(set(lengths))}')
    assert A.iterations == 1
    assert lengths and max(lengths) <= 3 * nfree and sum(lengths) <= 3 * nfree ** 2  # (a tridiagonal block: at most 3 nfree entries, thrice: values, rows, columns)
    x = device.to_host(x)
    assert numpy.array_equal(x[~free], hold[~free])
    idx = numpy.flatnonzero(free)
    direct = scipy.sparse.linalg.spsolve(ref[idx][:, idx].tocsc(), (rhs - ref @ numpy.where(free, 0., 1.5))[idx])
    lmin = numpy.linalg.eigvalsh(ref[idx][:, idx].toarray())[0]
    res = numpy.linalg.norm((rhs - ref @ x)[free])
    r_start = numpy.linalg.norm((rhs - ref @ numpy.where(free, 0., 1.5))[free])
    assert res <= RTOL * r_start * (1 + 1e-3) and numpy.linalg.norm(x[idx] - direct) <= res / lmin + 8 * U * numpy.linalg.norm(direct)


def test_maxiter_between_two_looks():
    from nutils_amd import matrix
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    with pytest.raises(matrix.ToleranceNotReached) as info:
        solve(A, rhs, rtol=RTOL, maxiter=6, check=4, **kwargs)
    best = info.value.best
    assert A.iterations == 6
    assert numpy.isfinite(best).all() and numpy.array_equal(best[~free], start[~free])
    res = numpy.linalg.norm((rhs - ref @ best)[free])
    assert RTOL * r0 < res < r0  # six iterations got somewhere, not there


def test_negative_definite_matrix_is_refused():
    from nutils_amd import matrix
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = problem('wide')
    with pytest.raises(matrix.MatrixError, match='cg: matrix is not positive definite'):
        solve(-A, rhs, rtol=RTOL, **kwargs)


# ---- 8. solver.System and the plan cache ------------------------------------------------------------------------------------------

def test_system_and_plan_cache(monkeypatch):
    '''the Laplace example under matrix.backend('hip') with linargs naming the preconditioner, against the 'diag' route; the symbolic phase runs once per pattern and
    mask: not for a re-valued Jacobian (`_with_values`), again for another mask'''
    from nutils_amd import amg, matrix, _lib
    from nutils_amd.solver import System
    from test_gpu_system_device import laplace_forms
    sqr, res = laplace_forms(32, 'std', 1)
    cons = System(sqr, trial='u').solve_constraints(droptol=1e-15)
    calls, symbolic = [], amg.symbolic
    monkeypatch.setattr(amg, 'symbolic', lambda *args, **kwargs: calls.append(1) or symbolic(*args, **kwargs))
    rtol = 1e-10
    with matrix.backend('hip'):
        dev = System(res, trial='u', test='v')
        with _lib.trace() as trace:
            x = dev.solve(constrain=cons, linargs=dict(solver='cg', precon='amg', rtol=rtol, preconargs=dict(coarse=64)))['u']
        jac = dev._device_jac[1]
        it = dev.linear_iterations[-1]
        y = System(res, trial='u', test='v').solve(constrain=cons, linargs=dict(solver='cg', precon='diag', rtol=rtol))['u']
    assert 'nh_pcg_iterate' in trace and 'nh_amg_create' in trace and len(calls) == 1
    assert isinstance(jac, matrix.HipMatrix) and jac._hostcsr is None
    free = numpy.isnan(cons['u']).ravel()
    assert numpy.array_equal(x.ravel()[~free], y.ravel()[~free])
    # both routes solve K x = b to |r| <= rtol |r0|: they differ by at most (|r_x| + |r_y|) / lmin <= 2 rtol |r0| / lmin
    host = System(res, trial='u', test='v')
    K = host.assemble_jacobian({}).export('dense')
    r0 = numpy.linalg.norm(numpy.asarray(host.assemble_residual({'u': numpy.nan_to_num(cons['u'])})).ravel()[free])
    lmin = numpy.linalg.eigvalsh(K[free][:, free])[0]
    dist = numpy.linalg.norm((x - y).ravel()[free])
    print(f'{it} iterations; |x_amg - x_diag| = {dist:.3e}, bound {2 * rtol * r0 * (1 + 1e-3) / lmin:.3e}')
    assert lmin > 0 and dist <= 2 * rtol * r0 * (1 + 1e-3) / lmin
    # the Jacobian of a next Newton step: new values on the same index tensors
    again = jac._with_values(jac.triplet()[0] * 2.)
    rhs = numpy.random.default_rng(15).normal(size=jac.shape[0])
    args = dict(solver='cg', precon='amg', rtol=rtol, preconargs=dict(coarse=64))
    z = again.solve(rhs, constrain=~free, **args)
    assert len(calls) == 1 and again._hostcsr is None
    assert numpy.linalg.norm((rhs - 2 * (K @ z))[free]) <= rtol * numpy.linalg.norm(rhs[free]) * (1 + 1e-3)
    again.solve(rhs, constrain=~free, **args)
    assert len(calls) == 1
    other = ~free
    other[numpy.flatnonzero(free)[:3]] = True  # three more dofs held
    again.solve(rhs, constrain=other, **args)
    assert len(calls) == 2
    again.solve(rhs, constrain=other, **dict(args, preconargs=dict(coarse=32)))  # (another `coarse` is another hierarchy)
    assert len(calls) == 3
