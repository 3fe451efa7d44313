'''The host loop of the device Krylov solves (nutils_amd.krylov.solve, and the rules of krylov.Cg, Bicgstab, Minres, Fgmres) run on the CPU: the numpy
recurrences of the host test modules stand in for the device behind the interface of `krylov.Recurrence`, and every solve is compared with the loop those
modules restate (`cg_reference`, `pcg_reference`, `bicgstab_solve_reference`, `minres_solve_reference`, `gmres_reference`): the bytes of x, the iterations, the
number of starts, and the outcome -- a return, ToleranceNotReached with x for its `best`, or MatrixError with the message of the solver.  The adapters override
only what touches the device (the residual, the kernels, the read-back); what decides is the code that runs on the GPU.  The last test asserts that the cases
reach every outcome of every restated loop.'''
import numpy
import pytest
import scipy.sparse

from nutils_amd import krylov, matrix
import test_amg_host
import test_bicgstab_host
import test_cg_host
import test_gmres_host
import test_minres_host

CHECKS = 1, 5, 16
MESSAGES = {'flagged': 'cg: matrix is not positive definite', 'breakdown': '{}: breakdown', 'singular': 'fgmres: singular matrix', 'non-finite': '{}: non-finite residual'}
OUTCOMES = {'cg': {'converged', 'maxiter', 'flagged'}, 'cg+amg': {'converged', 'maxiter', 'flagged'}, 'bicgstab': {'converged', 'maxiter', 'breakdown', 'non-finite'},
            'minres': {'converged', 'maxiter', 'breakdown', 'non-finite'}, 'fgmres': {'converged', 'maxiter', 'singular', 'non-finite'}}
reached = set()  # the (solver, outcome) pairs the cases below produced


# ---- the numpy recurrences behind the interface of krylov.Recurrence ---------------------------------------------------------

class Host:
    '''`start`, `advance` and `solution` on a numpy recurrence `rec` with init(r), iterate(n, stop_rr), x, RR, FLAG and COUNT; what is read back is a Python
    float, as it is from the device'''

    def __init__(self, rec, A, b, free):
        self.rec, self.A, self.b, self.free = rec, A, b, free

    def start(self):
        self.rec.init(numpy.where(self.free, self.b - self.A @ self.rec.x, 0.))
        return float(self.rec.RR)

    def advance(self, steps, stop_rr):
        self.rec.iterate(steps, stop_rr)
        return float(self.rec.RR), float(self.rec.FLAG), float(self.rec.COUNT)

    def solution(self):
        return self.rec.x


class HostCg(Host, krylov.Cg):
    '''the three calls and the read-back of krylov.Cg.advance, which does the counting'''
    advance = krylov.Cg.advance

    def stop(self, stop_rr):
        self.rec.stop(stop_rr)

    def iterate(self, steps):
        self.rec.iterate(steps)

    def look(self):
        return float(self.rec.RR), float(self.rec.FLAG_B)


class HostBicgstab(Host, krylov.Bicgstab):
    pass


class HostMinres(Host, krylov.Minres):
    pass


class HostFgmres(Host, krylov.Fgmres):
    def __init__(self, rec, A, b, free):
        Host.__init__(self, rec, A, b, free)
        self.cycle = rec.m

    def update(self):
        self.rec.update()


class Pcg(test_cg_host.Recurrence):
    '''test_cg_host.Recurrence with z = M(r): iteration by iteration the arithmetic of test_amg_host.pcg_reference'''

    def z(self):
        return self.dinv(self.r)


# ---- a solve by the restated loop and by the real one --------------------------------------------------------------------------

def reference(solver, A, b, x0, free, dinv, stop_rr, maxiter, check, restart):
    '''(x, iterations, starts, outcome) of the loop the host test module of `solver` restates'''
    if solver == 'cg':
        return test_cg_host.cg_reference(A, b, x0, free, dinv, stop_rr, maxiter, check=check)
    if solver == 'cg+amg':  # (looks after every iteration: `check` is 1)
        return test_amg_host.pcg_reference(A, b, x0, free, dinv, stop_rr, maxiter)
    if solver == 'bicgstab':
        return test_bicgstab_host.bicgstab_solve_reference(A, b, x0, free, dinv, stop_rr, maxiter, check=check)
    if solver == 'minres':
        return test_minres_host.minres_solve_reference(A, b, x0, free, dinv, stop_rr, maxiter, check=check)
    x, it, outcome, cyc = test_gmres_host.gmres_reference(A, b, x0, free, dinv, stop_rr, restart, maxiter, check=check, full=True)
    return x, it, cyc.cycles, outcome


def recurrence(solver, A, b, x0, free, dinv, restart):
    x0, product = numpy.array(x0, dtype=float), lambda y: A @ y
    if solver == 'cg':
        return HostCg(test_cg_host.Recurrence(product, free, dinv, x0), A, b, free)
    if solver == 'cg+amg':
        return HostCg(Pcg(product, free, dinv, x0), A, b, free)
    if solver == 'bicgstab':
        return HostBicgstab(test_bicgstab_host.Recurrence(product, free, dinv, x0), A, b, free)
    if solver == 'minres':
        return HostMinres(test_minres_host.Recurrence(product, free, dinv, x0), A, b, free)
    return HostFgmres(test_gmres_host.Cycle(product, free, dinv, x0, max(1, min(int(restart), int(free.sum())))), A, b, free)


def real(solver, A, b, x0, free, dinv, atol, rtol, maxiter, check, restart):
    '''(x, iterations, starts, outcome, error) of krylov.solve'''
    rec = recurrence(solver, A, b, x0, free, dinv, restart)
    outcome = error = None
    try:
        x = krylov.solve(rec, atol, rtol, maxiter, check)
        outcome = 'converged'
    except matrix.ToleranceNotReached as e:
        x, outcome = e.best, 'maxiter'
    except matrix.MatrixError as e:
        x, error = rec.solution(), e
    return x, rec.iterations, getattr(rec.rec, 'starts', None) or rec.rec.cycles, outcome, error


def same_bytes(x, y):
    return x.dtype == y.dtype == float and x.tobytes() == y.tobytes()


def compare(solver, A, b, x0=None, free=None, dinv=None, atol=0., rtol=0., restart=30, maxiters=None, expect=None):
    '''The real loop against the restated one for `check` in CHECKS and `maxiters`: by default half of, two below, exactly and three above the iterations the
    case needs when it looks after every iteration.  `expect`: outcomes that must be among those of the case.'''
    n = len(b)
    b = numpy.asarray(b, dtype=float)
    x0 = numpy.zeros(n) if x0 is None else x0
    free = numpy.ones(n, dtype=bool) if free is None else free
    r0 = numpy.where(free, b - A @ x0, 0.)
    stop_rr = max(atol, rtol * float(r0 @ r0) ** .5) ** 2  # the bound as HipMatrix.solve documents it; r0 . r0 is the first RR of every recurrence, bit for bit
    if maxiters is None:
        need = reference(solver, A, b, x0, free, dinv, stop_rr, 10 * n + 10, 1, restart)[1]
        maxiters = sorted({need // 2, max(need - 2, 0), need, need + 3})
    seen = set()
    for maxiter in maxiters:
        for check in CHECKS:
            x, it, starts, outcome = reference(solver, A, b, x0, free, dinv, stop_rr, maxiter, check, restart)
            y, it_real, starts_real, outcome_real, error = real(solver, A, b, x0, free, dinv, atol, rtol, maxiter, check, restart)
            where = f'{solver}, maxiter={maxiter}, check={check}: the restated loop has {outcome} after {it} iterations and {starts} starts'
            if outcome in ('converged', 'maxiter'):
                assert error is None and outcome_real == outcome, where
            else:
                assert outcome_real is None and type(error) is matrix.MatrixError and str(error) == MESSAGES[outcome].format(solver), (where, error)
            assert same_bytes(x, y) and starts_real == starts, where
            if solver == 'cg+amg':  # pcg_reference looks after every iteration and counts those that moved x; the host counts what it enqueued: whole looks, the
                flagged = outcome == 'flagged'  # flagged one among them, in every run of looks (a start that returns or raises has none)
                assert it + flagged <= it_real <= min(maxiter, it + flagged + (check - 1) * (starts - 1 + flagged)) and (it_real % check == 0 or it_real == maxiter), where
            else:
                assert it_real == it, where
            seen.add(outcome)
    assert seen >= set(expect or ()), (solver, seen, expect)
    reached.update((solver, outcome) for outcome in seen)
    return seen


# ---- the cases -------------------------------------------------------------------------------------------------------------

def scaled_laplace():
    '''the system of test_cg_host.test_reference_agrees_with_a_direct_solve: constrained dofs held at non-zero values, a diagonal Jacobi has to do with'''
    A = test_bicgstab_host.laplace2d(9, 7)
    n = A.shape[0]
    rng = numpy.random.default_rng(3)
    s = scipy.sparse.diags(rng.uniform(.5, 2., n))
    A = scipy.sparse.csr_matrix(s @ A @ s)
    b = rng.normal(size=n)
    free = rng.uniform(size=n) < .8
    return A, b, numpy.where(free, 0., rng.normal(size=n)), free


def test_cg():
    A, b, x0, w = test_cg_host.restart_case()
    x, it, starts, outcome = test_cg_host.cg_reference(A, b, x0, numpy.ones(len(b), dtype=bool), None, (1e-13 * numpy.linalg.norm(b - A @ x0)) ** 2, 10 * len(b), check=1)
    assert outcome == 'converged' and starts >= 3  # the case restarts
    compare('cg', A, b, x0, rtol=1e-13, expect=['converged', 'maxiter'])
    A, b, x0, free = scaled_laplace()
    for dinv in (numpy.where(free, 1 / A.diagonal(), 0.), None):
        compare('cg', A, b, x0, free, dinv, rtol=1e-11, expect=['converged', 'maxiter'])
        compare('cg', A, b, x0, free, dinv, atol=1e-6, rtol=1e-3, expect=['converged'])
    assert compare('cg', A, b, x0, free, atol=1e3, maxiters=(0, 5)) == {'converged'}  # within the bound at the first start: a return without an iteration, whatever maxiter is
    # the diagonal family with a negative entry, and the 2 x 2 systems of test_cg_host.test_reference_on_the_small_cases
    d, b = (v.copy() for v in test_cg_host.diagonal_family(None, 1e12, 37))
    j = numpy.abs(b).argmax()
    d[j], b[j] = -d[j], 10 * b[j]  # (the negative entry outweighs the others in r . z and in p . q at the first iteration, with Jacobi and without)
    for dinv in (1 / d, None):
        assert compare('cg', scipy.sparse.diags(d, format='csr'), b, dinv=dinv, rtol=1e-10, maxiters=(1, 37, 40)) == {'flagged'}
    for rhs in ([1., 1.], [1., 2.]):
        assert compare('cg', numpy.diag([1., -1.]), rhs, dinv=numpy.array([1., -1.]), rtol=1e-8, maxiters=(2,)) == {'flagged'}


def test_cg_amg():
    '''test_amg_host.pcg_reference, which looks after every iteration, against krylov.Cg around test_cg_host.Recurrence with the cycle for z = M r'''
    A, free = test_amg_host.problem('laplace')
    n = A.shape[0]
    levels = test_amg_host.reference('laplace', 16)
    M = lambda r: test_amg_host.cycle(levels, r)
    b = numpy.random.default_rng(4).normal(size=n)
    x0 = numpy.where(free, 0., 1 + .1 * numpy.arange(n))
    compare('cg+amg', A, b, x0, free, M, rtol=1e-10, expect=['converged', 'maxiter'])
    assert compare('cg+amg', -A, b, x0, free, M, rtol=1e-10, maxiters=(1, 20)) == {'flagged'}  # (p . A p < 0 at the first iteration)
    assert compare('cg+amg', A, b, x0, free, M, atol=1e9, maxiters=(0, 5)) == {'converged'}


def test_bicgstab():
    for jacobi in (True, False):
        N, b, x0, free, dinv, stop_rr = test_bicgstab_host.agreement_case(jacobi)
        compare('bicgstab', N, b, x0, free, dinv, rtol=1e-11, expect=['converged', 'maxiter'])
    for name in test_bicgstab_host.BREAKDOWNS:  # a flag after progress: a restart, the iterations counting on
        K, bN, xN, rN = test_bicgstab_host.tiled(name, 40)
        free = numpy.ones(len(bN), dtype=bool)
        assert test_bicgstab_host.bicgstab_solve_reference(K, bN, numpy.zeros(len(bN)), free, None, (1e-10 * numpy.linalg.norm(bN)) ** 2, len(bN))[2] >= 3
        compare('bicgstab', K, bN, rtol=1e-10, expect=['converged', 'maxiter'])
    D = numpy.diag([1., -1.])
    assert compare('bicgstab', D, [1., 1.], atol=1e-12, maxiters=(2,)) == {'breakdown'}  # rhat . v = 0 at the first step
    assert compare('bicgstab', numpy.array([[0., 1.], [1., 0.]]), [1., 0.], atol=1e-12, maxiters=(2,)) == {'breakdown'}
    assert compare('bicgstab', D, [1., numpy.inf], atol=1e-12, maxiters=(0, 2)) == {'non-finite'}
    assert compare('bicgstab', D, [1., 2.], atol=10., maxiters=(0, 2)) == {'converged'}
    assert compare('bicgstab', D, [1., 2.], atol=1e-12, maxiters=(0, 1, 2, 3)) == {'converged', 'maxiter'}


def test_minres():
    K, cons, rhs, free, start, r0, Kff, sv = test_minres_host.small()
    for dinv in (None, numpy.where(free, 1 / numpy.abs(K.diagonal()), 0.)):
        compare('minres', K, rhs, start, free, dinv, rtol=1e-10, expect=['converged', 'maxiter'])
    A, b, x0, w = test_cg_host.restart_case()  # (the drift of the carried residual from the true one: a restart that iterates)
    compare('minres', A, b, x0, rtol=1e-13, expect=['converged', 'maxiter'])
    N = test_bicgstab_host.skewed(test_bicgstab_host.laplace2d(9, 7), 2.)  # not symmetric: the restarts get nowhere
    assert compare('minres', N, numpy.random.default_rng(3).normal(size=N.shape[0]), rtol=1e-10, maxiters=(40,)) == {'maxiter'}
    D = numpy.diag([1., -1.])
    assert compare('minres', numpy.zeros((2, 2)), [1., 1.], atol=1e-12, maxiters=(2,)) == {'breakdown'}  # the zero matrix: gamma = 0
    assert compare('minres', D, [1., 2.], dinv=numpy.array([1., -1.]), atol=1e-12, maxiters=(2,)) == {'breakdown'}  # a preconditioner that is not positive
    assert compare('minres', D, [1., numpy.inf], atol=1e-12, maxiters=(0, 2)) == {'non-finite'}
    assert compare('minres', D, [1., 2.], atol=10., maxiters=(0, 2)) == {'converged'}
    assert compare('minres', D, [1., 1.], atol=1e-12, maxiters=(0, 1, 2, 3)) == {'converged', 'maxiter'}


def test_fgmres():
    for jacobi in (True, False):
        A, b, free, x0, dinv = test_gmres_host.dense_case(12, 32, jacobi, True)
        for restart in (3, 5, 30):  # (30: clipped to the free dofs)
            compare('fgmres', A, b, x0, free, dinv, rtol=1e-10, restart=restart, expect=['converged', 'maxiter'])
        N, b, x0, free, dinv, stop_rr = test_bicgstab_host.agreement_case(jacobi)
        compare('fgmres', N, b, x0, free, dinv, rtol=1e-11, restart=5, maxiters=(13, 20, 2000), expect=['converged', 'maxiter'])
    one = numpy.ones(2)
    compare('fgmres', numpy.diag([1., 0.]), one, atol=1e-12, maxiters=(1, 2, 5), expect=['singular'])  # the first cycle removes what can be removed, the second finds nothing
    assert compare('fgmres', numpy.zeros((2, 2)), one, atol=1e-12, maxiters=(2,)) == {'singular'}
    assert compare('fgmres', numpy.eye(2), [1., numpy.inf], atol=1e-12, maxiters=(0, 2)) == {'non-finite'}
    assert compare('fgmres', numpy.eye(2), [3., -4.], atol=1e-12, maxiters=(0, 1, 2)) == {'converged', 'maxiter'}  # the lucky breakdown: a flag, and a solution
    D = numpy.diag([1., -1.])
    assert compare('fgmres', D, [1., 2.], numpy.array([5., 6.]), numpy.zeros(2, dtype=bool), maxiters=(0,)) == {'converged'}  # nothing free
    assert compare('fgmres', D, [1., 2.], atol=10., maxiters=(0, 2)) == {'converged'}


@pytest.mark.parametrize('solver', ['cg', 'cg+amg', 'bicgstab', 'minres', 'fgmres'])
def test_non_finite_residual_at_a_start(solver):
    '''cg_reference and pcg_reference assert a finite residual where the real loop raises: the message of the other three is that of 'cg' too'''
    D = numpy.diag([1., 2.])
    x, it, starts, outcome, error = real(solver, D, numpy.array([1., numpy.inf]), numpy.zeros(2), numpy.ones(2, dtype=bool), (lambda r: r) if solver == 'cg+amg' else None,
                                         1e-12, 0., 2, 16, 30)
    name = solver.split('+')[0]
    assert type(error) is matrix.MatrixError and str(error) == f'{name}: non-finite residual' and (it, starts) == (0, 1) and not x.any()


def test_every_outcome_of_every_loop_is_reached():
    '''the tests above fill `reached`; a case function that has not run yet (this test selected alone) runs here'''
    for solver, cases in (('cg', test_cg), ('cg+amg', test_cg_amg), ('bicgstab', test_bicgstab), ('minres', test_minres), ('fgmres', test_fgmres)):
        if not any(name == solver for name, outcome in reached):
            cases()
    assert reached == {(solver, outcome) for solver, outcomes in OUTCOMES.items() for outcome in outcomes}
