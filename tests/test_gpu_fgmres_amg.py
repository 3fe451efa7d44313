'''Flexible GMRES preconditioned by the AMG cycle, and the preconditioner objects that feed it (matrix.HipMatrix.getprecon, solve(solver='fgmres', precon=M),
nh_fgmres_iterate) on the GPU: the solve contract on nonsymmetric matrices at four settings of `restart`, step counts against the numpy restatement of
tests/test_fgmres_amg_host.py on its own hierarchy and against the device's Jacobi-GMRES, one cycle looked at on the device after every step, a dense level 0,
the objects (bytes of the solves they replace, no setup at the second use, one application), lagged hierarchies, solver.System, and the stops and errors.

Sizes: 1480 rows ('wide': three Gram-Schmidt workgroups, levels 1443 / 119 / 11 at coarse=40); 3000 ('chain': three levels at coarse=256); 1001 ('odd': vectors
of odd length, one double per access); 262 444 ('tridiagonal': more than 512 * 256 pairs of doubles, so the kernel that keeps Z strides past its grid cap);
192 ('elasticity': 4^3 trilinear nodes with the six rigid-body modes, coarse=40).'''
import functools
import types
import numpy
import pytest
import scipy.sparse

import test_amg_host
import test_gpu_bicgstab
import test_gpu_cg
from test_bicgstab_host import skewed
from test_gmres_host import cells, ST_FULL
from test_fgmres_amg_host import fgmres_reference, general_hierarchy
from test_gpu_bicgstab import hip, gamma, RTOL, U

pytestmark = pytest.mark.gpu

ld = numpy.longdouble
VELOCITY = numpy.array([3., -2.])


def same_bytes(a, b):
    return a.shape == b.shape and numpy.array_equal(a.view(numpy.int64), b.view(numpy.int64))


# ---- problems ------------------------------------------------------------------------------------------------------------

def convection_diffusion(velocity):
    '''the form of test_gpu_bicgstab.test_convection_diffusion_through_the_front_end on 40 x 37 nodes: (integral, constraints, right-hand side)'''
    from nutils_amd import function, mesh
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1, 40), numpy.linspace(0, 2, 37)])
    basis = domain.basis('std', degree=1)
    grad = function.grad(basis, geom)
    K = domain.integral((function.outer(grad).sum(-1) + function.outer(basis, (grad * numpy.asarray(velocity)).sum(-1))) * function.J(geom), degree=2)
    cons = numpy.full((40, 37), numpy.nan)
    cons[0], cons[-1] = 1., 0.  # inflow and outflow sides held
    return K, cons.ravel(), numpy.random.default_rng(5).normal(size=1480)


@functools.lru_cache(maxsize=None)
def problem(name):
    '''A namespace: A (on the device), ref (its host twin), kwargs (constrain, lhs0), rhs, free, start, r0, direct and smin (small problems), coarse and args
    (the other keywords of getprecon).  'wide', 'elasticity' and 'tridiagonal' are test_gpu_bicgstab's nonsymmetric problems; 'wide9' is 'wide' skewed by 0.9
    instead of 0.5; 'chain' is test_amg_host's chain skewed; 'odd' has 1001 rows; 'convdiff' / 'convdiff6' come from the front end; 'block' is 'wide' with a
    10 x 10 block of nodes free.  Made once, never written.'''
    from nutils_amd import amg, function, matrix
    p = types.SimpleNamespace(coarse=40, args={})
    if name in ('wide', 'elasticity', 'tridiagonal'):
        p.A, p.ref, p.kwargs, p.rhs = test_gpu_bicgstab.problem(name)[:4]
        if name == 'elasticity':
            grid = numpy.linspace(0, 1, 4)
            p.args = dict(nullspace=amg.rigid_body_modes(numpy.stack(numpy.meshgrid(grid, grid, grid, indexing='ij'), -1).reshape(-1, 3)))
        if name == 'tridiagonal':
            p.coarse = 256
    elif name in ('wide9', 'block'):
        w = problem('wide')
        sym = test_gpu_cg.problem('wide')[1]  # the symmetric matrix both are skewed from
        p.ref, p.rhs, p.kwargs = skewed(sym, .9 if name == 'wide9' else .5), w.rhs, w.kwargs
        if name == 'block':
            hold = numpy.full((40, 37), 1.5)
            hold[12:22, 9:19] = numpy.nan
            p.kwargs, p.coarse = dict(constrain=hold.ravel()), 256
        p.A = hip(p.ref)
    elif name in ('chain', 'odd'):
        if name == 'chain':
            p.ref, free = test_amg_host.problem('chain')
            p.ref, p.coarse = skewed(p.ref), 256
            cons = numpy.where(free, numpy.nan, 2.)
        else:
            n = 1001
            p.ref = scipy.sparse.diags([numpy.full(n - 1, -1.5), numpy.full(n, 4.), numpy.full(n - 1, -.5)], [-1, 0, 1], format='csr')
            cons = numpy.full(n, numpy.nan)
            cons[::100] = 2.
        p.A, p.kwargs, p.rhs = hip(p.ref), dict(constrain=cons), numpy.random.default_rng(6).normal(size=p.ref.shape[0])
    else:
        K, cons, p.rhs = convection_diffusion(VELOCITY * {'convdiff': 1, 'convdiff6': 2}[name])
        p.A = function.eval(function.as_matrix(K))
        v, rp, ci = function.eval(function.as_csr(K))
        p.ref, p.kwargs = scipy.sparse.csr_matrix((v, ci, rp), p.A.shape), dict(constrain=cons)
        assert abs(p.ref - p.ref.T).max() > .01  # not symmetric
    assert isinstance(p.A, matrix.HipMatrix) and p.A._hostcsr is None
    p.ref = scipy.sparse.csr_matrix(p.ref)
    p.free, p.start = matrix.constraints(p.A.shape[1], p.kwargs.get('constrain'), p.kwargs.get('lhs0'))
    p.r0 = numpy.linalg.norm((p.rhs - p.ref @ p.start)[p.free])
    p.direct = p.smin = None
    if p.A.shape[0] < 4000:  # (the chain of 3000 rows included: a dense SVD of 2997^2, once)
        p.direct = matrix.ScipyMatrix(p.ref).solve(p.rhs, **p.kwargs)
        p.smin = numpy.linalg.svd(p.ref.toarray()[p.free][:, p.free], compute_uv=False)[-1]
        assert p.smin > 0
    return p


@functools.lru_cache(maxsize=None)
def precon(name):
    '''the 'amg' object of a problem, symmetric=False; built once'''
    p = problem(name)
    return p.A.getprecon('amg', constrain=p.kwargs.get('constrain'), symmetric=False, coarse=p.coarse, **p.args)


def contract(p, x):
    '''what a solve to RTOL promises (test_gpu_bicgstab.contract): constrained dofs exactly, the true residual within the bound, the error within
    residual / sigma_min'''
    assert isinstance(x, numpy.ndarray) and numpy.array_equal(x[~p.free], p.start[~p.free])
    res = numpy.linalg.norm((p.rhs - p.ref @ x)[p.free])
    print(f'|r| / |r0| = {res / p.r0:.3e}' + ('' if p.direct is None else f', |x - x_direct| = {numpy.linalg.norm(x - p.direct):.3e}, bound {res / p.smin:.3e}'))
    assert res <= RTOL * p.r0 * (1 + 1e-3)
    if p.direct is not None:
        assert numpy.linalg.norm(x - p.direct) <= res / p.smin
    return res


def solve(A, rhs, M, iterated=True, **kwargs):
    '''A.solve(solver='fgmres', precon=M) that insists on the device route and on the flexible step'''
    from nutils_amd import _lib
    with _lib.trace() as calls:
        try:
            return A.solve(rhs, solver='fgmres', precon=M, **kwargs)
        finally:
            assert 'nh_gmres_init' in calls and ('nh_fgmres_iterate' in calls) == iterated and 'nh_gmres_iterate' not in calls, sorted(set(calls))
            assert 'nh_segment_dot' not in calls and 'nh_block_segment_dot' not in calls and 'nh_amg_create' not in calls  # the object is ready: no setup
            assert A._hostcsr is None  # neither values nor indices went to the host


@functools.lru_cache(maxsize=None)
def reference(name, restart):
    '''(steps, level sizes) of the numpy restatement on its own hierarchy, to the bound of the tests'''
    p = problem(name)
    levels = general_hierarchy(p.ref, p.free, p.coarse)
    x, it, outcome, _ = fgmres_reference(p.ref, p.rhs, p.start, p.free, lambda r: test_amg_host.cycle(levels, r), (RTOL * p.r0) ** 2, restart, int(p.free.sum()), check=1)
    assert outcome == 'converged' and numpy.linalg.norm((p.rhs - p.ref @ x)[p.free]) <= RTOL * p.r0 * (1 + 1e-3)
    return it, [lv.nfree for lv in levels]


# ---- the solve contract -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,restart', [(name, restart) for name in ('wide', 'chain', 'odd', 'elasticity') for restart in (5, 30, 'full')]
                         + [('tridiagonal', 5), ('tridiagonal', 30), ('chain', 1), ('wide', 1)])
def test_solve_contract(name, restart):
    '''constrained dofs exactly, the true residual within the bound, the error within residual / sigma_min; the flexible entry point and not the fixed one; a
    second solve the same bytes; a look at the device after every step the same bytes and the same count.  restart=1: one column of Z, every step a restart
    (the restatement takes 41 steps on the chain, 37 at restart 30).'''
    p, M = problem(name), precon(name)
    nfree = int(p.free.sum())
    if restart == 'full':
        restart = nfree + 7  # (clipped to nfree: unrestarted)
    x = solve(p.A, p.rhs, M, rtol=RTOL, restart=restart, **p.kwargs)  # (default maxiter: the free dofs)
    contract(p, x)
    steps = p.A.iterations
    print(f'{name}, restart {restart}: levels {[lv.nfree for lv in M.hierarchy.levels]}, {steps} steps')
    assert 0 < steps <= nfree
    assert same_bytes(solve(p.A, p.rhs, M, rtol=RTOL, restart=restart, **p.kwargs), x) and p.A.iterations == steps
    assert same_bytes(solve(p.A, p.rhs, M, rtol=RTOL, restart=restart, check=1, **p.kwargs), x) and p.A.iterations == steps


def test_level_sizes():
    '''the hierarchies are those the sizes above were chosen for'''
    assert [lv.nfree for lv in precon('wide').hierarchy.levels] == [1443, 119, 11]
    assert [lv.nfree for lv in precon('chain').hierarchy.levels] == [2997, 833, 232]
    assert len(precon('elasticity').hierarchy.levels) >= 2 and precon('elasticity').hierarchy.levels[0].k == 6
    assert len(precon('tridiagonal').hierarchy.levels) >= 5
    assert precon('wide').symmetric is False and precon('wide').kind == 'amg' and precon('wide').shape == (1480, 1480)


# ---- step counts ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,restart', [('wide', 30), ('wide', 5), ('chain', 30), ('convdiff', 30), ('convdiff', 10)])
def test_step_counts(name, restart):
    '''`iterations` against the restatement on the restatement's own hierarchy: at most 1.1 x + 2, the bar tests/test_gpu_amg.py sets for CG with this cycle;
    on the chain and on convection-diffusion at restart 30, at most a quarter of the steps the device's Jacobi-GMRES takes for the same call'''
    p, M = problem(name), precon(name)
    x = solve(p.A, p.rhs, M, rtol=RTOL, restart=restart, **p.kwargs)
    contract(p, x)
    steps = p.A.iterations
    it_ref, sizes = reference(name, restart)
    print(f'{name}, restart {restart}: levels {sizes}, {steps} steps on the device, {it_ref} in numpy')
    assert [lv.nfree for lv in M.hierarchy.levels] == sizes
    assert steps <= 1.1 * it_ref + 2
    if restart == 30 and name in ('chain', 'convdiff'):
        y = p.A.solve(p.rhs, solver='fgmres', precon='diag', rtol=RTOL, restart=restart, maxiter=10 * len(p.rhs), **p.kwargs)
        contract(p, y)
        print(f'{name}: Jacobi-GMRES {p.A.iterations} steps')
        assert 4 * steps <= p.A.iterations


# ---- one cycle, looked at on the device after every step ----------------------------------------------------------------------------

class Device:
    '''the vectors and the work array of a flexible cycle on the device, and the three entry points on them.  V, Z, z, t and w start as NaN, so that an entry
    a kernel should have written and did not shows.'''

    def __init__(self, p, M, restart):
        from nutils_amd import device, kernels
        self.values, self.rowptr, self.colidx = p.A.triplet()
        self.n, self.m, self.M = len(p.start), restart, M
        self.col32 = kernels.csr_compact(self.colidx, self.n)
        self.mask = device.to_dev(p.free, 'uint8')
        nan = lambda size: device.to_dev(numpy.full(size, numpy.nan), 'float64')
        self.V, self.Z, self.z, self.t, self.w = nan((restart + 1) * self.n), nan(restart * self.n), nan(self.n), nan(self.n), nan(self.n)
        self.x = device.to_dev(p.start, 'float64')
        self.r = device.to_dev(numpy.where(p.free, p.rhs - p.ref @ p.start, 0.), 'float64')
        self.work = kernels.gmres_work(restart)
        self.work.fill_(numpy.nan)
        kernels.gmres_init(None, self.r, self.V, self.z, self.work, restart=restart)

    def iterate(self, niter, stop_rr):
        from nutils_amd import kernels
        kernels.fgmres_iterate(self.values, self.rowptr, self.colidx, self.n, rowmask=self.mask, amg=self.M.hierarchy.handle, V=self.V, Z=self.Z, z=self.z,
                               t=self.t, w=self.w, work=self.work, restart=self.m, stop_rr=stop_rr, niter=niter, col32=self.col32)

    def update(self):
        from nutils_amd import kernels
        kernels.gmres_update(None, self.Z, self.x, self.work, restart=self.m)

    def head(self):
        '''(estimate, flag, count, status)'''
        return self.work[:4].tolist()

    def state(self):
        from nutils_amd import device
        c = cells(self.m)
        return dict(V=device.to_host(self.V).reshape(self.m + 1, self.n), Z=device.to_host(self.Z).reshape(self.m, self.n), z=device.to_host(self.z),
                    w=device.to_host(self.w), x=device.to_host(self.x), work=device.to_host(self.work[:c['r'] + self.m * (self.m + 1)]))


@pytest.mark.parametrize('name', ['wide', 'wide9'])
def test_one_cycle(name):
    '''A cycle of 30 steps read after every step.  Column j of Z has the bytes of M(V_j), one application of the object to the basis vector; the estimates
    never rise (by more than the factor 1 + 4 u of tests/test_gpu_gmres.py, which leaves room for a division that rounds otherwise) -- also on the matrix
    skewed by 0.9, where the cycle helps least; V^T V - I stays within 1e-13, the bound of that file for its basis; steps enqueued past the end of the cycle
    move no byte of V, Z, z, w or the cells.  The update: x = x0 + sum_k y_k Z_k with y as the device solved it, recomputed in longdouble: a sum of 30 products
    in a fixed order and one addition, so elementwise within gamma_31 sum |y_k| |Z_k| + u |x|; and the true residual is the estimate, to the 1e-10 |r0| of
    test_gpu_gmres.test_estimates_never_rise.'''
    from nutils_amd import device
    p, M = problem(name), precon(name)
    m, n = 30, len(p.rhs)
    dev = Device(p, M, m)
    estimates = [dev.head()[0]]
    for j in range(m):
        dev.iterate(1, 0.)
        est, flag, count, st = dev.head()
        assert (flag, count, st) == (0, j + 1, ST_FULL if j == m - 1 else 0)
        estimates.append(est)
        zj = dev.Z[j * n:(j + 1) * n]
        assert same_bytes(device.to_host(zj), device.to_host(M(dev.V[j * n:(j + 1) * n])))
        assert bool(dev.Z[(j + 1) * n:].isnan().all())  # nothing beyond column j was touched
    print(f'{name}: ' + ' '.join(f'{e:.2e}' for e in estimates))
    assert all(b <= a * (1 + 4 * U) for a, b in zip(estimates, estimates[1:]))
    assert estimates[-1] < .5 * estimates[0]  # (and they do fall)
    before = dev.state()
    V = before['V'][:m]
    worst = numpy.abs(V @ V.T - numpy.eye(m)).max()
    print(f'max |V^T V - I| = {worst:.2e}')
    assert worst <= 1e-13
    for name_ in ('V', 'Z'):
        assert not before[name_][:m][:, ~p.free].any() and not numpy.isnan(before[name_][:m]).any()
    dev.iterate(3, 0.)
    after = dev.state()
    for name_ in before:
        assert same_bytes(before[name_], after[name_]), name_
    # the update
    dev.update()
    final = dev.state()
    y = final['work'][cells(m)['y']:cells(m)['y'] + m]
    Z = before['Z']
    exact = p.start.astype(ld) + (y.astype(ld)[:, None] * Z.astype(ld)).sum(0)
    size = numpy.abs(y)[:, None] * numpy.abs(Z)
    bound = (gamma(m + 1) * size.sum(0) + U * (numpy.abs(p.start) + size.sum(0))) * (1 + 2. ** -10)
    err = numpy.abs(final['x'] - exact).astype(float)
    print(f'update: max error / bound = {(err / numpy.maximum(bound, 1e-300)).max():.3f}')
    assert (err <= bound).all()
    assert numpy.array_equal(final['x'][~p.free], p.start[~p.free]) and not numpy.array_equal(final['x'], p.start)
    true = numpy.linalg.norm(numpy.where(p.free, p.rhs - p.ref @ final['x'], 0.))
    print(f'estimate {estimates[-1] ** .5:.6e}, true residual {true:.6e}')
    assert abs(true - estimates[-1] ** .5) <= 1e-10 * estimates[0] ** .5


# ---- a dense level 0 ------------------------------------------------------------------------------------------------------------

def test_dense_level_zero():
    '''100 free dofs of 1480, a 10 x 10 block of nodes of the skewed matrix: level 0 is the dense level, its general inverse is the inverse of the free block, and
    the solve is there after one step (with the symmetric pseudo-inverse the restatement takes 22)'''
    p, M = problem('block'), precon('block')
    assert [lv.kind for lv in M.hierarchy.levels] == ['dense'] and int(p.free.sum()) == 100
    x = solve(p.A, p.rhs, M, rtol=RTOL, check=1, **p.kwargs)
    contract(p, x)
    assert p.A.iterations == 1


# ---- the objects ------------------------------------------------------------------------------------------------------------------

def spd():
    A, ref, kwargs, rhs, free, start, r0, direct, lmin = test_gpu_cg.problem('wide')
    return A, ref, kwargs, rhs, free


@pytest.mark.parametrize('args', [dict(coarse=16), dict(coarse=40, sweeps=2), dict(coarse=16, smoother='chebyshev', degree=2)], ids=['coarse16', 'sweeps2', 'chebyshev'])
def test_cg_with_an_object_gives_the_bytes_of_the_string(args):
    from nutils_amd import _lib
    A, ref, kwargs, rhs, free = spd()
    x = A.solve(rhs, solver='cg', precon='amg', preconargs=args, rtol=RTOL, **kwargs)
    iterations = A.iterations
    M = A.getprecon('amg', constrain=kwargs['constrain'], **args)
    assert M.symmetric and M.kind == 'amg'
    for _ in range(2):  # (the second use of the object: nothing of the first is left in it)
        with _lib.trace() as calls:
            y = A.solve(rhs, solver='cg', precon=M, rtol=RTOL, **kwargs)
        assert same_bytes(x, y) and A.iterations == A.cg_iterations == iterations
        assert 'nh_pcg_iterate' in calls and not {'nh_segment_dot', 'nh_block_segment_dot', 'nh_amg_create', 'nh_csr_lanczos', 'nh_cg_iterate'} & set(calls), sorted(set(calls))


@pytest.mark.parametrize('solver', ['cg', 'minres', 'bicgstab', 'fgmres'])
def test_diag_object_gives_the_bytes_of_the_string(solver):
    A, ref, kwargs, rhs, free = spd()
    M = A.getprecon('diag', constrain=kwargs['constrain'])
    assert M.kind == 'diag' and M.symmetric and numpy.array_equal(M.free, free)
    x = A.solve(rhs, solver=solver, precon='diag', rtol=RTOL, **kwargs)
    iterations = A.iterations
    y = A.solve(rhs, solver=solver, precon=M, rtol=RTOL, **kwargs)
    assert same_bytes(x, y) and A.iterations == iterations > 0
    if solver == 'fgmres':  # the nonsymmetric twin too
        p = problem('wide')
        N = p.A.getprecon('diag', constrain=p.kwargs['constrain'])
        assert same_bytes(p.A.solve(p.rhs, solver=solver, precon='diag', rtol=RTOL, **p.kwargs), p.A.solve(p.rhs, solver=solver, precon=N, rtol=RTOL, **p.kwargs))


def test_one_application():
    '''M(r) on a host vector and on a device tensor, against the hierarchy's own apply; the 'diag' object against dinv r'''
    from nutils_amd import device
    p, M = problem('wide'), precon('wide')
    r = numpy.where(p.free, numpy.random.default_rng(13).normal(size=len(p.rhs)), 0.)
    r_dev = device.to_dev(r, 'float64')
    expect = device.to_host(M.hierarchy.apply(r_dev))
    on_host, on_device = M(r), M(r_dev)
    assert isinstance(on_host, numpy.ndarray) and on_device.is_cuda
    assert same_bytes(on_host, expect) and same_bytes(device.to_host(on_device), expect) and not expect[~p.free].any() and expect.any()
    D = p.A.getprecon('diag', constrain=p.kwargs['constrain'])
    assert same_bytes(D(r), numpy.where(p.free, (1 / p.ref.diagonal()) * r, 0.))
    assert D(r_dev).is_cuda


def test_symbolic_phase_is_shared_with_the_solve(monkeypatch):
    '''getprecon takes the symbolic phase from the matrix's cache and leaves it there, whatever `symmetric` is'''
    from nutils_amd import amg
    A, ref, kwargs, rhs, free = spd()
    B = A._with_values(A.triplet()[0])
    B._amg = None
    calls, symbolic = [], amg.symbolic
    monkeypatch.setattr(amg, 'symbolic', lambda *args, **kw: calls.append(1) or symbolic(*args, **kw))
    B.getprecon('amg', constrain=kwargs['constrain'], coarse=16)
    B.getprecon('amg', constrain=kwargs['constrain'], coarse=16, symmetric=False)
    B.solve(rhs, solver='cg', precon='amg', preconargs=dict(coarse=16), rtol=RTOL, **kwargs)
    assert len(calls) == 1
    B._with_values(B.triplet()[0] * 2.).getprecon('amg', constrain=kwargs['constrain'], coarse=16)
    assert len(calls) == 1


# ---- lagged hierarchies ------------------------------------------------------------------------------------------------------------

def test_lagged_cycle():
    '''the object of velocity (3, -2) on the matrix of velocity (6, -4), a matrix on the same index tensors: the contract, in at most 1.5 x + 2 of the steps with
    its own object (the restatement of tests/test_fgmres_amg_host.py on its own right-hand side: 40 against 38; the device here: 40 against 37)'''
    p3, p6 = problem('convdiff'), problem('convdiff6')
    assert all(bool((a == b).all()) for a, b in zip(p3.A.triplet()[1:], p6.A.triplet()[1:]))
    A6 = p3.A._with_values(p6.A.triplet()[0])
    assert A6._amg is p3.A._amg
    x = solve(A6, p6.rhs, precon('convdiff6'), rtol=RTOL, **p6.kwargs)
    contract(p6, x)
    own = A6.iterations
    y = solve(A6, p6.rhs, precon('convdiff'), rtol=RTOL, **p6.kwargs)
    contract(p6, y)
    print(f'lagged {A6.iterations} steps, own {own}')
    assert A6.iterations <= 1.5 * own + 2


def test_lagged_cg():
    '''CG on K + 5 M with the object of K, coarse=40: at most 1.5 x + 2 of the iterations with its own object (the device: 48 against 48; the reference the feature was
    proposed with, at its own settings: 40 against 38)'''
    from nutils_amd import function, mesh
    A, ref, kwargs, rhs, free = spd()
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1, 40), numpy.linspace(0, 2, 37)])
    basis = domain.basis('std', degree=1)
    mass = function.eval(function.as_matrix(domain.integral(function.outer(basis) * function.J(geom), degree=2)))
    assert all(bool((a == b).all()) for a, b in zip(A.triplet()[1:], mass.triplet()[1:]))
    shifted = A._with_values(A.triplet()[0] + 5 * mass.triplet()[0])
    v, rp, ci = (a.cpu().numpy() for a in shifted.triplet())
    host = scipy.sparse.csr_matrix((v, ci, rp), shifted.shape)
    args = dict(constrain=kwargs['constrain'], coarse=40)
    x = shifted.solve(rhs, solver='cg', precon=shifted.getprecon('amg', **args), rtol=RTOL, **kwargs)
    own = shifted.iterations
    y = shifted.solve(rhs, solver='cg', precon=A.getprecon('amg', **args), rtol=RTOL, **kwargs)
    print(f'lagged {shifted.iterations} iterations, own {own}')
    assert shifted.iterations <= 1.5 * own + 2
    start = numpy.where(free, 0., kwargs['constrain'])
    r0 = numpy.linalg.norm((rhs - host @ start)[free])
    for z in (x, y):
        assert numpy.array_equal(z[~free], start[~free]) and numpy.linalg.norm((rhs - host @ z)[free]) <= RTOL * r0 * (1 + 1e-3)


# ---- solver.System -----------------------------------------------------------------------------------------------------------------

def test_system():
    '''a linear convection-diffusion System on 33 x 33 nodes under matrix.backend('hip'): the Jacobian stays in HBM, the object is built on it once and goes to
    the solve through `linargs`; against the host route (a direct solve) within |r| / sigma_min, as tests/test_gpu_system_fgmres.py compares'''
    from nutils_amd import function, matrix, mesh, _lib
    from nutils_amd.solver import System
    domain, geom = mesh.unitsquare(32, 'square')
    u, v = domain.field('u', btype='std', degree=1), domain.field('v', btype='std', degree=1)
    dV = function.J(geom)
    grad = lambda w: function.grad(w, geom)
    res = domain.integral((grad(v) * grad(u)).sum(-1) * dV, degree=2) + domain.integral(v * (grad(u) * VELOCITY).sum(-1) * dV, degree=2)
    res -= domain.boundary['top'].integral(v * function.PointFunc(lambda x: numpy.cos(x[:, 0]), geom) * dV, degree=2)
    g = function.PointFunc(lambda x: numpy.sin(x[:, 1]), geom)
    right = domain.boundary['right']
    sqr = domain.boundary['left'].integral(u * u * dV, degree=2)
    sqr += right.integral(u * u * dV, degree=2) - 2 * right.integral(u * g * dV, degree=2) + right.integral(g * g * dV, degree=2)
    cons = System(sqr, trial='u').solve_constraints(droptol=1e-15)
    free = numpy.isnan(cons['u']).ravel()
    host = System(res, trial='u', test='v')
    expect = host.solve(constrain=cons)['u']
    with matrix.backend('hip'):
        dev = System(res, trial='u', test='v')
        dev.solve(constrain=cons, linargs=dict(solver='fgmres', precon='diag', rtol=1e-10, maxiter=5000))
        jacobi, jac = dev.linear_iterations[-1], dev._device_jac[1]
        assert isinstance(jac, matrix.HipMatrix) and jac._hostcsr is None
        M = jac.getprecon('amg', constrain=~free, symmetric=False, coarse=40)
        with _lib.trace() as calls:
            x = dev.solve(constrain=cons, linargs=dict(solver='fgmres', precon=M, rtol=1e-10))['u']
        again = dev._device_jac[1]
    assert 'nh_fgmres_iterate' in calls and 'nh_gmres_iterate' not in calls and 'nh_amg_create' not in calls and again._hostcsr is None
    assert len(dev.linear_iterations) == 1 and dev.linear_iterations[0] == again.iterations > 0
    print(f'{dev.size} dofs, levels {[lv.nfree for lv in M.hierarchy.levels]}: {dev.linear_iterations[0]} steps with the cycle, {jacobi} with Jacobi')
    assert len(M.hierarchy.levels) >= 2 and dev.linear_iterations[0] < jacobi
    x, expect = numpy.asarray(x).ravel(), numpy.asarray(expect).ravel()
    assert numpy.array_equal(x[~free], expect[~free])
    K = host.assemble_jacobian({}).export('dense')
    assert abs(K - K.T).max() > 1e-3
    r = numpy.linalg.norm(numpy.asarray(host.assemble_residual({'u': x.reshape(host.trial_shapes[0])})).ravel()[free])
    smin = numpy.linalg.svd(K[free][:, free], compute_uv=False)[-1]
    err = numpy.linalg.norm((x - expect)[free])
    print(f'|x_dev - x_host| = {err:.3e}, |r| / smin = {r / smin:.3e}')
    assert smin > 0 and err <= r / smin


# ---- stops and errors -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('check', [16, 4, 1])
def test_stops_at_maxiter(check):
    '''a maxiter that is no multiple of `check` or `restart`: ToleranceNotReached with the vector reached'''
    from nutils_amd import matrix
    p, M = problem('wide'), precon('wide')
    with pytest.raises(matrix.ToleranceNotReached) as info:
        solve(p.A, p.rhs, M, rtol=RTOL, maxiter=13, restart=5, check=check, **p.kwargs)
    best = info.value.best
    assert p.A.iterations == 13
    assert numpy.isfinite(best).all() and numpy.array_equal(best[~p.free], p.start[~p.free])
    res = numpy.linalg.norm((p.rhs - p.ref @ best)[p.free])
    print(f'check={check}: |r| / |r0| = {res / p.r0:.3e}')
    assert RTOL * p.r0 < res < p.r0  # (thirteen steps got somewhere, not there)
    with pytest.warns(UserWarning, match='tolerance'):
        lenient = p.A.solve_leniently(p.rhs, solver='fgmres', precon=M, rtol=RTOL, maxiter=13, restart=5, check=check, **p.kwargs)
    assert numpy.array_equal(lenient, best)


def test_errors_and_device_vectors():
    from nutils_amd import device, matrix
    p, M = problem('wide'), precon('wide')
    # a zero on the diagonal of a free row: no hierarchy, no Jacobi object
    values, rowptr, colidx = p.A.triplet()
    values = values.clone()
    values[rowptr[700]:rowptr[701]][colidx[rowptr[700]:rowptr[701]] == 700] = 0.  # (row 700 is free)
    assert p.free[700] and bool((values == 0).any())
    broken = p.A._with_values(values)
    for kind in ('amg', 'diag'):
        with pytest.raises(matrix.MatrixError, match='diagonal has zero entries'):
            broken.getprecon(kind, constrain=p.kwargs['constrain'])
    # another mask, another shape
    other = p.kwargs['constrain'].copy()
    other[700] = 0.
    with pytest.raises(matrix.MatrixError, match='another set of free dofs'):
        p.A.solve(p.rhs, solver='fgmres', precon=M, rtol=RTOL, constrain=other)
    with pytest.raises(matrix.MatrixError, match='another set of free dofs'):
        p.A.solve(p.rhs, solver='fgmres', precon=M, rtol=RTOL)
    with pytest.raises(matrix.MatrixError, match='built for a 1480x1480 matrix'):
        problem('odd').A.solve(problem('odd').rhs, solver='fgmres', precon=M, rtol=RTOL, **problem('odd').kwargs)
    with pytest.raises(matrix.MatrixError, match='symmetric=False'):
        p.A.solve(p.rhs, solver='cg', precon=M, rtol=RTOL, **p.kwargs)
    with pytest.raises(matrix.MatrixError, match="'fgmres'"):
        p.A.solve(p.rhs, solver='bicgstab', precon=M, rtol=RTOL, **p.kwargs)
    # a right-hand side on the device gives a result on the device, with the bytes of the host call
    x = solve(p.A, p.rhs, M, rtol=RTOL, **p.kwargs)
    xd = solve(p.A, device.to_dev(p.rhs, 'float64'), M, rtol=RTOL, **p.kwargs)
    assert xd.is_cuda and same_bytes(device.to_host(xd), x)
    # a residual that is within the bound at the start: no step
    done = solve(p.A, p.rhs, M, iterated=False, atol=2 * RTOL * p.r0, constrain=p.kwargs['constrain'], lhs0=x)
    assert p.A.iterations == 0 and same_bytes(done, x)
