'''solver.System on the device route (matrix.backend('hip'): the merged Jacobian a HipMatrix in HBM, constraints the row mask of its Krylov solve, `linargs`
to every linear solve) against the host route (pinned mirror, free submatrix, scipy's direct solver): the Laplace example end to end, with nothing of the
matrix's size crossing PCIe; a vector system; one nonlinear, nonsymmetric Cahn-Hilliard step; and what `linargs` does where it is not needed.

The bound of the linear comparisons is the contract of tests/test_gpu_cg.py: with K the host route's Jacobian restricted to the free dofs, lmin its smallest
eigenvalue (dense eigvalsh) and r the true free residual of the device result, |x_dev - x_host| <= |r| / lmin.'''
import contextlib
import numpy
import pytest

from test_gpu_examples import cahnhilliard

pytestmark = pytest.mark.gpu

CG = dict(solver='cg', rtol=1e-12)


def laplace_forms(nelems, btype, degree):
    '''the functional of the constraints and the residual of tests/test_gpu_examples.py::laplace'''
    from nutils_amd import mesh, function
    domain, geom = mesh.unitsquare(nelems, 'square')
    u = domain.field('u', btype=btype, degree=degree)
    v = domain.field('v', btype=btype, degree=degree)
    dV = function.J(geom)
    grad = lambda w: function.grad(w, geom)
    res = domain.integral((grad(v) * grad(u)).sum(-1) * dV, degree=degree * 2)
    flux = function.PointFunc(lambda x: numpy.cos(1) * numpy.cosh(x[:, 1]), geom)
    res -= domain.boundary['right'].integral(v * flux * dV, degree=degree * 2)
    g = function.PointFunc(lambda x: numpy.cosh(1) * numpy.sin(x[:, 0]), geom)
    sqr = domain.boundary['left'].integral(u * u * dV, degree=degree * 2)
    top = domain.boundary['top']
    sqr += top.integral(u * u * dV, degree=degree * 2) - 2 * top.integral(u * g * dV, degree=degree * 2) + top.integral(g * g * dV, degree=degree * 2)
    return sqr, res


def within_contract(what, system, trial, x_dev, x_host, free):
    '''|x_dev - x_host| <= |r| / lmin on the free dofs of a linear `system` (a host-route one); the other dofs agree exactly'''
    x_dev, x_host, free = (numpy.asarray(a).ravel() for a in (x_dev, x_host, free))
    assert numpy.array_equal(x_dev[~free], x_host[~free], equal_nan=True)
    K = system.assemble_jacobian({}).export('dense')
    r = numpy.linalg.norm(numpy.asarray(system.assemble_residual({trial: numpy.nan_to_num(x_dev).reshape(system.trial_shapes[0])}))[free])
    lmin = numpy.linalg.eigvalsh(K[free][:, free])[0]
    assert lmin > 0
    err = numpy.linalg.norm((x_dev - x_host)[free])
    print(f'{what}: |x_dev - x_host| = {err:.3e}, |r| / lmin = {r / lmin:.3e} (|r| = {r:.3e}, lmin = {lmin:.3e}, |x_host| = {numpy.linalg.norm(x_host[free]):.3e})')
    assert err <= r / lmin


@contextlib.contextmanager
def device_route_only(monkeypatch):
    '''inside: `_HostMirror` cannot be made, and every device.to_host is recorded -> the list of the lengths that came back'''
    from nutils_amd import device, solver

    def no_mirror(*args, **kwargs):
        raise AssertionError('the device route built a _HostMirror')
    lengths, to_host = [], device.to_host

    def recording(tensor):
        lengths.append(tensor.numel())
        return to_host(tensor)
    with monkeypatch.context() as m:
        m.setattr(solver, '_HostMirror', no_mirror)
        m.setattr(device, 'to_host', recording)
        yield lengths


@pytest.mark.parametrize('nelems,btype,degree', [(4, 'std', 1), (4, 'spline', 2), (32, 'std', 1)])
def test_laplace_example(monkeypatch, nelems, btype, degree):
    '''25, 36 and 1089 dofs (five vector workgroups, the last one partial): constraints by projection and the solve, both with CG on the device.  The device
    route's solve takes the device route's constraints, as in the example; the host solve it is compared with takes the same ones, since the bound is that of
    one linear system (the constraints themselves are compared with the host route's just before).'''
    from nutils_amd import matrix, _lib
    from nutils_amd.solver import System
    sqr, res = laplace_forms(nelems, btype, degree)
    host_c, host_s = System(sqr, trial='u'), System(res, trial='u', test='v')
    cons = host_c.solve_constraints(droptol=1e-15)
    assert host_c.linear_iterations == [None]  # (scipy's direct solver counts nothing)

    dev_c, dev_s = System(sqr, trial='u'), System(res, trial='u', test='v')
    with matrix.backend('hip'), device_route_only(monkeypatch) as lengths, _lib.trace() as calls:
        dcons = dev_c.solve_constraints(droptol=1e-15, linargs=CG)
        mark = len(lengths)
        dlhs = dev_s.solve(constrain=dcons, linargs=CG)['u']
        jac_c, jac_s = dev_c._device_jac[1], dev_s._device_jac[1]
    assert isinstance(jac_c, matrix.HipMatrix) and isinstance(jac_s, matrix.HipMatrix)
    assert jac_c._hostcsr is None and jac_s._hostcsr is None
    assert 'nh_cg_iterate' in calls and 'nh_csr_support' in calls, sorted(set(calls))
    assert not hasattr(dev_c, '_free_plan') and not hasattr(dev_s, '_free_plan') and dev_c._mirror is None and dev_s._mirror is None
    for system, jac, back in ((dev_c, jac_c, lengths[:mark]), (dev_s, jac_s, lengths[mark:])):
        print(f'{system.size} dofs, nnz {jac.nnz}: lengths that came to the host {sorted(set(back))}, Krylov iterations {system.linear_iterations}')
        # vectors of n entries come home (residual, support, solution) and nothing longer: below nnz wherever a matrix has more entries than rows.  (The boundary
        # functional of the 32 x 32 mesh has 760 entries in 1089 rows: there no vector is shorter than nnz, and the bound on the lengths is n alone.)
        assert back and max(back) <= system.size and (max(back) < jac.nnz or jac.nnz <= system.size)
        assert system.linear_iterations and all(n > 0 for n in system.linear_iterations)
    assert len(dev_c.linear_iterations) == 1 and len(dev_s.linear_iterations) == 1
    assert jac_s.nnz > dev_s.size  # (the Jacobian of the example itself is where "nothing of nnz length" bites)

    assert numpy.array_equal(numpy.isnan(dcons['u']), numpy.isnan(cons['u']))
    lhs = host_s.solve(constrain=dcons)['u']
    print(f'|lhs - lhs of the host route from its own constraints| = {numpy.abs(lhs - host_s.solve(constrain=cons)["u"]).max():.3e}')
    within_contract('cons', host_c, 'u', dcons['u'], cons['u'], ~numpy.isnan(cons['u']))
    within_contract('lhs', host_s, 'u', dlhs, lhs, numpy.isnan(cons['u']))


def test_constant_matrix_is_made_once():
    from nutils_amd import matrix
    from nutils_amd.solver import System
    sqr, res = laplace_forms(4, 'std', 1)
    system = System(res, trial='u', test='v')
    with matrix.backend('hip'):
        a, b = system.assemble_jacobian({}), system.assemble_jacobian({})
    assert isinstance(a, matrix.HipMatrix) and a is b and system.is_constant_matrix


def test_vector_system(monkeypatch):
    '''trilinear elasticity on 6^3 elements (tests/test_gpu_hex1.py::test_solver: clamped at x = 0, displaced at x = 1), 1029 dofs of which 735 free'''
    from nutils_amd import mesh, function, matrix, _lib
    from nutils_amd.solver import System
    cons = numpy.full((7, 7, 7, 3), numpy.nan)
    cons[0] = 0.
    cons[-1] = [0., .05, -.1]
    cons = cons.reshape(-1, 3)
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1, 7)] * 3)
    u = domain.field('u', btype='std', degree=1, shape=[3])
    v = domain.field('v', btype='std', degree=1, shape=[3])
    eps = lambda w: function.symgrad(w, geom)
    res = domain.integral(function.inner(eps(v), function.div(u, geom) * function.eye(3) + 1.3 * eps(u)) * function.J(geom), degree=2)
    host = System(res, trial='u', test='v')
    lhs = host.solve(constrain={'u': cons})['u']
    dev = System(res, trial='u', test='v')
    with matrix.backend('hip'), device_route_only(monkeypatch) as lengths, _lib.trace() as calls:
        dlhs = dev.solve(constrain={'u': cons}, linargs=CG)['u']
    assert 'nh_cg_iterate' in calls
    print(f'{dev.size} dofs, nnz {dev._device_jac[1].nnz}: lengths that came to the host {sorted(set(lengths))}, Krylov iterations {dev.linear_iterations}')
    assert max(lengths) <= dev.size < dev._device_jac[1].nnz and dev.linear_iterations[0] > 0
    assert dlhs.shape == lhs.shape == (343, 3) and numpy.abs(lhs[numpy.isnan(cons)]).max() > 1e-3
    within_contract('elasticity', host, 'u', dlhs, lhs, numpy.isnan(cons))


def test_cahnhilliard_step(golden, monkeypatch):
    '''One implicit Cahn-Hilliard step (tests/test_gpu_examples.py::test_cahnhilliard_residual_jacobian: 2 x 81 dofs, two merged blocks, field-dependent
    entries, a saddle: indefinite) by Newton with Jacobi-BiCGStab on the device, against the golden step at that test's own 1e-8.'''
    from nutils_amd import matrix, _lib
    from nutils_amd.solver import System
    g = golden('cahnhilliard_p2_4')
    domain, nrg = cahnhilliard(g)
    n = len(g['arg_φ'])
    start = {'φ': g['arg_φ0'], 'φ0': g['arg_φ0'], 'η': numpy.zeros(n)}
    host_system = System(nrg, trial='φ,η')
    host = host_system.solve(arguments=start, tol=1e-8)
    system = System(nrg, trial='φ,η')
    assert not system.is_linear and not system.is_constant_matrix
    with matrix.backend('hip'), device_route_only(monkeypatch) as lengths, _lib.trace() as calls:
        sol = system.solve(arguments=start, tol=1e-8, linargs=dict(solver='bicgstab', rtol=1e-10))
    assert 'nh_bicgstab_iterate' in calls and 'nh_cg_iterate' not in calls
    jac = system._device_jac[1]
    assert isinstance(jac, matrix.HipMatrix) and jac._hostcsr is None and max(lengths) <= system.size < jac.nnz
    assert system.linear_iterations and all(k > 0 for k in system.linear_iterations)
    for name in 'φη':
        print(f'{name}: device route {numpy.abs(sol[name] - g["step_" + name]).max():.3e}, host route {numpy.abs(host[name] - g["step_" + name]).max():.3e} from the golden step; '
              f'BiCGStab iterations per Newton step {system.linear_iterations}')
    assert numpy.abs(sol['φ'] - g['step_φ']).max() < 1e-8
    assert numpy.abs(sol['η'] - g['step_η']).max() < 1e-8
    # `assemble_jacobian`: a fresh value tensor per call on the same index tensors and int32 copy, with the values the host route gets
    from nutils_amd import device
    with matrix.backend('hip'):
        a, b = system.assemble_jacobian(sol), system.assemble_jacobian(sol)
    (av, arp, aci), (bv, brp, bci) = a.triplet(), b.triplet()
    assert a is not b and av.data_ptr() != bv.data_ptr() and arp is brp and aci is bci and a._col32 is not None and b._col32 is a._col32 and jac.triplet()[1] is arp
    values, colidx, rowptr = host_system.assemble_jacobian(sol).export('csr')
    assert numpy.array_equal(device.to_host(av), values) and numpy.array_equal(device.to_host(bv), values)
    assert numpy.array_equal(device.to_host(arp), rowptr) and numpy.array_equal(device.to_host(aci), colidx)


def test_without_linargs():
    '''the device solve is iterative and nothing chooses its tolerance: MatrixError; the direct solver ignores `linargs`: the same bytes'''
    from nutils_amd import matrix
    from nutils_amd.solver import System
    sqr, res = laplace_forms(4, 'std', 1)
    cons = System(sqr, trial='u').solve_constraints(droptol=1e-15)
    with matrix.backend('hip'):
        with pytest.raises(matrix.MatrixError, match='tolerance'):
            System(res, trial='u', test='v').solve(constrain=cons)
        with pytest.raises(matrix.MatrixError, match='tolerance'):
            System(res, trial='u', test='v').solve(constrain=cons, linargs=dict(solver='cg'))
    plain = System(res, trial='u', test='v').solve(constrain=cons)['u']
    with_args = System(res, trial='u', test='v').solve(constrain=cons, linargs=dict(rtol=1e-8))['u']
    assert plain.tobytes() == with_args.tobytes()
    cons_args = System(sqr, trial='u').solve_constraints(droptol=1e-15, linargs=dict(rtol=1e-8))
    assert cons['u'].tobytes() == cons_args['u'].tobytes()
