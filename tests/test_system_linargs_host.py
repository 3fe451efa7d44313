'''Host-side logic of `linargs` and of the device route through solver.System, without a GPU: which backends qualify (`assemble_device`), what the solve loop
asks of its matrix on either route (assembly stubbed, a matrix that records its calls), and the three places a new entry point appears in.'''
import ctypes
import inspect
import os
import re
import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostOnly:  # (fake-backend precedent: tests/test_host_logic.py)
    @staticmethod
    def assemble(values, rowptr, colidx, ncols):
        return 'host'


class WithHandOver(HostOnly):
    @staticmethod
    def assemble_device(values_dev, rowptr_dev, colidx_dev, ncols):
        return 'device'


class Recorder:
    '''a 4 x 4 matrix that solves with numpy and keeps the keywords of every call'''

    def __init__(self, lenient=True):
        self.K = numpy.diag([2., 4., 5., 10.]) + numpy.diag([1., 1., 1.], 1)
        self.calls = []
        self.iterations = 7
        if lenient:
            self.solve_leniently = lambda rhs, **kwargs: self._solve('solve_leniently', rhs, **kwargs)

    def _solve(self, name, rhs, constrain=None, **kwargs):
        self.calls.append((name, len(rhs), None if constrain is None else constrain.tolist(), kwargs))
        free = numpy.ones(len(self.K), dtype=bool) if constrain is None else ~constrain
        if len(rhs) < len(self.K):  # (the host route hands the free block's right-hand side over; the matrix stands for the reduced one)
            return numpy.linalg.solve(self.K[self.sub][:, self.sub], rhs)
        x = numpy.zeros(len(self.K))
        x[free] = numpy.linalg.solve(self.K[free][:, free], rhs[free])
        return x

    def solve(self, rhs, **kwargs):
        return self._solve('solve', rhs, **kwargs)


def laplace_system():
    from nutils_amd import mesh, function
    from nutils_amd.solver import System
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1, 4)])
    u = domain.field('u', btype='std', degree=1)
    v = domain.field('v', btype='std', degree=1)
    return System(domain.integral((function.grad(v, geom) * function.grad(u, geom)).sum(-1) * function.J(geom), degree=2), trial='u', test='v')


def stubbed(monkeypatch, jac, linear=True):
    '''a System of four dofs whose assembly is the Recorder's matrix: residual K x - b (linear) or K x - b + 0.1 x^3 (not)'''
    system = laplace_system()
    assert system.size == 4 and system.is_linear
    b = numpy.array([1., -2., 3., .5])
    seen = []

    def residual(args):
        x = numpy.asarray(args['u'], dtype=float)
        return jac.K @ x - b + (0. if linear else .1 * x ** 3)

    def start_jacobian(args, free, enqueued=None):
        seen.append(None if free is None else free.tolist())
        jac.sub = free
        return lambda copy=False: jac
    monkeypatch.setattr(system, 'assemble_residual', residual)
    monkeypatch.setattr(system, '_start_jacobian', start_jacobian)
    monkeypatch.setattr(system, 'assemble_jacobian_residual', lambda args, free=None, copy=True: (start_jacobian(args, free)(), residual(args)))
    system.is_linear = linear
    return system, seen


def test_backends_that_qualify():
    from nutils_amd import matrix
    from nutils_amd.solver import System
    assert callable(matrix._HipBackend.assemble_device)
    assert System._device_backend() is None  # scipy, the default
    with matrix.backend(HostOnly):
        assert System._device_backend() is None
    with matrix.backend(WithHandOver):
        assert System._device_backend() is WithHandOver
    with matrix.backend('hip'):
        assert System._device_backend() is matrix._HipBackend
    assert System._device_backend() is None


def test_signatures():
    from nutils_amd.solver import System
    for method in (System.solve, System.solve_constraints):
        assert inspect.signature(method).parameters['linargs'].default is None
    assert 'solveargs' in inspect.signature(System.step).parameters


CONS = {'u': numpy.array([numpy.nan, numpy.nan, numpy.nan, 1.5])}
HELD = [False, False, False, True]


@pytest.mark.parametrize('backend', [HostOnly, WithHandOver])
def test_linear_solve_on_either_route(monkeypatch, backend):
    '''the host route reduces to the free dofs and solves for them; the device route keeps the matrix whole and passes the held dofs as `constrain`; without
    `linargs` no keyword reaches the matrix, with them exactly those; `linear_iterations` has one entry per solve'''
    from nutils_amd import matrix
    device_route = backend is WithHandOver
    out = []
    for linargs in (None, dict(solver='cg', rtol=1e-9)):
        jac = Recorder()
        system, seen = stubbed(monkeypatch, jac)
        with matrix.backend(backend):
            out.append(system.solve(constrain=CONS, **({} if linargs is None else dict(linargs=linargs)))['u'])
        assert seen == ([None] if device_route else [[not h for h in HELD]])
        assert jac.calls == [('solve', 4 if device_route else 3, HELD if device_route else None, linargs or {})]
        assert system.linear_iterations == [7]
    expect = numpy.array([0., 0., 0., 1.5])
    expect[:3] = numpy.linalg.solve(jac.K[:3, :3], (numpy.array([1., -2., 3., .5]) - jac.K @ expect)[:3])
    for x in out:
        assert numpy.allclose(x, expect, rtol=1e-14, atol=0)


@pytest.mark.parametrize('backend', [HostOnly, WithHandOver])
@pytest.mark.parametrize('lenient', [True, False])
def test_newton_solve_on_either_route(monkeypatch, backend, lenient):
    '''with `linargs` a Newton step asks for `solve_leniently` where the matrix has one, with rtol = 1e-3 unless a tolerance is named; without, it calls `solve` bare'''
    from nutils_amd import matrix
    for linargs, expect in ((None, {}), (dict(solver='bicgstab'), dict(solver='bicgstab', rtol=1e-3)), (dict(atol=1e-9), dict(atol=1e-9)), (dict(rtol=1e-6), dict(rtol=1e-6))):
        jac = Recorder(lenient)
        system, seen = stubbed(monkeypatch, jac, linear=False)
        given = None if linargs is None else dict(linargs)
        with matrix.backend(backend):
            system.solve(constrain=CONS, tol=1e-10, **({} if linargs is None else dict(linargs=linargs)))
        assert len(jac.calls) >= 2 and len(system.linear_iterations) == len(jac.calls)
        name = 'solve_leniently' if lenient and linargs is not None else 'solve'
        assert all(call[0] == name and call[3] == expect for call in jac.calls), jac.calls
        assert all((call[2] == HELD) == (backend is WithHandOver) for call in jac.calls)
        assert linargs == given  # (the caller's dict is not written into)


def test_solve_constraints_passes_linargs_and_asks_for_the_support(monkeypatch):
    for with_support in (False, True):
        jac = Recorder()
        jac.K = numpy.diag([2., 0., 1e-20, 3.])
        jac.export = lambda form: (numpy.array([2., 1e-20, 3.]), numpy.array([0, 2, 3]), numpy.array([0, 1, 1, 2, 3]))
        if with_support:
            jac.colsupp = lambda tol: numpy.array([True, False, False, True])
            jac.export = None
        system, seen = stubbed(monkeypatch, jac)
        linargs = dict(solver='cg', atol=1e-12)
        cons = system.solve_constraints(droptol=1e-15, linargs=linargs)['u']
        assert jac.calls == [('solve', 4, [False, True, True, False], linargs)] and system.linear_iterations == [7]
        assert numpy.isnan(cons).tolist() == [False, True, True, False]
        assert numpy.allclose(cons[[0, 3]], [.5, .5 / 3], rtol=1e-14, atol=0)
        jac.calls.clear()
        system.solve_constraints(droptol=1e-15)
        assert jac.calls == [('solve', 4, [False, True, True, False], {})]


def test_support_entry_point_in_its_three_places():
    from nutils_amd import _lib, kernels, matrix
    header = open(os.path.join(ROOT, 'include', 'nutils_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'int\s+nh_csr_support\s*\(\s*const nh_csr \*A,\s*double tol,\s*unsigned char \*rowsupp_dev,\s*unsigned char \*colsupp_dev,\s*void \*stream\s*\)\s*;', header)
    restype, argtypes = _lib.SIGNATURES['nh_csr_support']
    assert restype is ctypes.c_int and argtypes == [ctypes.POINTER(_lib.Csr), ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(_lib.LIBPATH), 'nh_csr_support')
    assert callable(kernels.csr_support) and callable(matrix.HipMatrix.rowsupp) and callable(matrix.HipMatrix.colsupp)
    # argument errors are reported before anything touches the device
    lib = _lib.load()
    assert lib.nh_csr_support(None, 0., None, None, None) == -1 and b'NULL matrix' in lib.nh_last_error()
    bad = _lib.Csr(0, 0, 0, None, None, None, None, 0)
    assert lib.nh_csr_support(ctypes.byref(bad), -1., None, None, None) == -1 and b'tolerance' in lib.nh_last_error()
    assert lib.nh_csr_support(ctypes.byref(bad), 0., None, None, None) == 0
