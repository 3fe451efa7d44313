'''solver.System on the device route with the device solver for symmetric indefinite systems: a Helmholtz problem with a load and Dirichlet constraints under
matrix.backend('hip') with linargs=dict(solver='minres', rtol=1e-10), against the host route's direct solve, by the comparison
tests/test_gpu_system_fgmres.py makes for 'fgmres', with the smallest singular value in the place of the smallest eigenvalue.'''
import numpy
import pytest

from test_gpu_system_device import device_route_only

pytestmark = pytest.mark.gpu

MINRES = dict(solver='minres', rtol=1e-10)
K2 = 17.  # between the second and the third eigenvalue of the Laplacian on the unit square held at one side, 12.3 and 22.2


def helmholtz_residual(nelems):
    from nutils_amd import mesh, function
    domain, geom = mesh.unitsquare(nelems, 'square')
    u = domain.field('u', btype='std', degree=1)
    v = domain.field('v', btype='std', degree=1)
    dV = function.J(geom)
    grad = lambda w: function.grad(w, geom)
    load = function.PointFunc(lambda x: numpy.cos(3 * x[:, 0]) * (1 + x[:, 1]), geom)
    return domain.integral((grad(v) * grad(u)).sum(-1) * dV, degree=2) - domain.integral(K2 * v * u * dV, degree=2) - domain.integral(v * load * dV, degree=2)


def test_helmholtz(monkeypatch):
    '''169 dofs, one side held at non-zero values: the Jacobian stays in HBM, the solve is MINRES on the device, its iterations are counted, and the solution is
    within |r| / sigma_min of the host route's'''
    from nutils_amd import matrix, _lib
    from nutils_amd.solver import System
    res = helmholtz_residual(12)
    cons = numpy.full((13, 13), numpy.nan)
    cons[0] = .3 + .1 * numpy.arange(13)
    cons = dict(u=cons.ravel())
    free = numpy.isnan(cons['u'])
    host = System(res, trial='u', test='v')
    lhs = numpy.asarray(host.solve(constrain=cons)['u']).ravel()
    K = host.assemble_jacobian({}).export('dense')
    assert numpy.abs(K - K.T).max() <= 1e-14 * numpy.abs(K).max()
    eig = numpy.linalg.eigvalsh(K[free][:, free])
    smin = numpy.abs(eig).min()
    assert 0 < (eig < 0).sum() < 10 and smin > 1e-4 * numpy.abs(eig).max()  # symmetric, indefinite, nonsingular

    dev = System(res, trial='u', test='v')
    with matrix.backend('hip'), device_route_only(monkeypatch) as lengths, _lib.trace() as calls:
        dlhs = numpy.asarray(dev.solve(constrain=cons, linargs=MINRES)['u']).ravel()
        jac = dev._device_jac[1]
    assert isinstance(jac, matrix.HipMatrix) and jac._hostcsr is None
    assert 'nh_minres_init' in calls and 'nh_minres_iterate' in calls, sorted(set(calls))
    assert not {'nh_cg_iterate', 'nh_bicgstab_iterate', 'nh_gmres_iterate'} & set(calls)
    print(f'{dev.size} dofs, nnz {jac.nnz}: lengths that came to the host {sorted(set(lengths))}, MINRES iterations {dev.linear_iterations}')
    assert lengths and max(lengths) <= dev.size < jac.nnz
    assert len(dev.linear_iterations) == 1 and dev.linear_iterations[0] > 0 and dev.linear_iterations[0] == jac.iterations

    assert numpy.array_equal(dlhs[~free], lhs[~free]) and numpy.array_equal(dlhs[~free], cons['u'][~free])
    r = numpy.linalg.norm(numpy.asarray(host.assemble_residual({'u': dlhs.reshape(host.trial_shapes[0])})).ravel()[free])
    err = numpy.linalg.norm((dlhs - lhs)[free])
    print(f'|x_dev - x_host| = {err:.3e}, |r| / sigma_min = {r / smin:.3e} (|r| = {r:.3e}, sigma_min = {smin:.3e}, |x_host| = {numpy.linalg.norm(lhs[free]):.3e})')
    assert err <= r / smin
