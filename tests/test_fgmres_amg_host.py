'''CPU-side checks of flexible GMRES preconditioned by the AMG cycle (matrix.HipMatrix.getprecon, solve(solver='fgmres', precon=M), nh_fgmres_iterate): a
numpy restatement of the flexible iteration (`FlexCycle`: test_gmres_host.Cycle with a preconditioner callable and the stored Z) pinned to the definition of
flexible GMRES; the host loop of nutils_amd.krylov around it; the step counts of the restated cycle (test_amg_host.level with the general pseudo-inverse on
the dense level) on nonsymmetric and on symmetric positive definite matrices; the errors raised before any device work; what the C ABI refuses.  `FlexCycle`,
`fgmres_reference` and the problems are the CPU reference of tests/test_gpu_fgmres_amg.py.'''
import ctypes
import functools
import types
import numpy
import pytest
import scipy.sparse

from nutils_amd import _lib, amg, krylov, matrix
import test_amg_host
from test_bicgstab_host import refused, csr, skewed, P
from test_gmres_host import Cycle, gmres_reference, U, ST_DONE

RTOL = 1e-10


# ---- the algorithm, restated ---------------------------------------------------------------------------------------------

class FlexCycle(Cycle):
    '''What lives on the device between nh_gmres_init (without a diagonal) and nh_gmres_update on Z: the cells and the basis V of `Cycle`, the columns
    Z[j] = M_j(v_j) and the scratch vector t.  `precon(v, j)`: what the preconditioner returns for v in step j of the cycle -- it may depend on j, or on
    anything else: that is what the method is flexible about.  Step j (nh_fgmres_iterate): t = precon(z), Z[j] = t, then the step of `Cycle` with t as the
    input of the product; `update` is x += sum_k y[k] Z[k].  A step that finds a status moves nothing (on the device its V-cycle still runs into t, which
    nothing reads afterwards).'''

    def __init__(self, product, free, precon, x, restart, passes=2):
        super().__init__(product, free, None, x, restart, passes)
        self.precon = precon

    def init(self, r):
        self.Z = numpy.zeros((self.m, len(r)), dtype=r.dtype)
        self.t = numpy.zeros_like(r)
        super().init(r)

    def step(self, stop_rr):
        if self.ST != 0:
            return
        z = self.z
        self.t = self.Z[self.COUNT] = self.precon(z, self.COUNT)
        self.z = self.t  # the product of `Cycle.step` reads z
        super().step(stop_rr)
        if self.ST != 0:  # (no v_(j+1) was made: z stays what it was)
            self.z = z

    def update(self):
        V, self.V = self.V, self.Z
        try:
            super().update()
        finally:
            self.V = V


def fgmres_reference(A, b, x, free, precon, stop_rr, restart, maxiter, check=16):
    '''The host loop of krylov.solve around a `FlexCycle`, a look enqueuing no more steps than the cycle has left: (x, Arnoldi steps, outcome, cycle), outcome
    'converged', 'maxiter', 'singular' or 'non-finite'.  `precon(v)` or `precon(v, j)`.'''
    mask = lambda y: numpy.where(free, y, 0.)
    m = max(1, min(int(restart), int(free.sum())))
    try:
        precon(numpy.zeros(len(b)), 0)
        M = precon
    except TypeError:
        M = lambda v, j: precon(v)
    cyc = FlexCycle(lambda y: A @ y, free, M, numpy.array(x, dtype=float), m)
    cyc.looks = []  # steps enqueued per look
    it, since, rr_start, outcome = 0, None, None, None
    while outcome is None:
        cyc.init(mask(b - A @ cyc.x))
        rr = cyc.RR
        if not numpy.isfinite(rr):
            outcome = 'non-finite'
        elif rr <= stop_rr:
            outcome = 'converged'
        elif since in (0, 1) and not rr < rr_start:
            outcome = 'singular'
        elif it >= maxiter:
            outcome = 'maxiter'
        else:
            start, rr_start = it, rr
            while it < maxiter:
                steps = min(check, maxiter - it, m - cyc.COUNT)
                cyc.looks.append(steps)
                cyc.iterate(steps, stop_rr)
                it = start + cyc.COUNT
                if cyc.FLAG or cyc.RR <= stop_rr or cyc.COUNT >= m:
                    break
            since = 0 if cyc.FLAG else None if since is None else since + 1
            cyc.update()
    return cyc.x, it, outcome, cyc


# ---- problems ------------------------------------------------------------------------------------------------------------

def convection_diffusion(velocity, shape=(40, 37)):
    '''(A, free): the bilinear Galerkin matrix of -laplace u + velocity . grad u on shape nodes of [0, 1] x [0, 2], node (i, j) at dof i shape[1] + j, both
    x-sides held: the matrix function.as_matrix assembles for the form of test_gpu_bicgstab.test_convection_diffusion_through_the_front_end'''
    def line(n, h):
        K, M = test_amg_host.line(n, h)
        e = numpy.ones(n - 1)
        C = scipy.sparse.diags([-e / 2, numpy.r_[-.5, numpy.zeros(n - 2), .5], e / 2], [-1, 0, 1])  # int phi_i phi_j'
        return K, M, C
    (Kx, Mx, Cx), (Ky, My, Cy) = line(shape[0], 1 / (shape[0] - 1)), line(shape[1], 2 / (shape[1] - 1))
    kron = scipy.sparse.kron
    A = scipy.sparse.csr_matrix(kron(Kx, My) + kron(Mx, Ky) + velocity[0] * kron(Cx, My) + velocity[1] * kron(Mx, Cy))
    A.sort_indices()
    free = numpy.ones(shape, dtype=bool)
    free[0] = free[-1] = False
    return A, free.ravel()


@functools.lru_cache(maxsize=None)
def problem(name):
    '''(A, free, coarse): 'chain' and 'laplace' are test_amg_host's, skewed by 0.5 ('spd-chain', 'spd-laplace': as they are); 'convdiff', 'convdiff6': velocity
    (3, -2) and (6, -4); 'block' / 'scattered': the skewed Laplace matrix with 100 free dofs, a 10 x 10 block of nodes or scattered ones.  Made once, never written.'''
    if name.startswith('convdiff'):
        return convection_diffusion({'convdiff': (3., -2.), 'convdiff6': (6., -4.)}[name]) + (40,)
    if name in ('block', 'scattered'):
        A, _ = test_amg_host.problem('laplace')
        free = numpy.zeros((40, 37), dtype=bool)
        if name == 'block':
            free[12:22, 9:19] = True
        else:
            free.ravel()[numpy.random.default_rng(3).choice(1480, 100, replace=False)] = True
        return skewed(A), free.ravel(), 256
    base = name.split('-')[-1]
    A, free = test_amg_host.problem(base)
    A = A if name.startswith('spd') else skewed(A)
    A.sort_indices()
    return A, free, 256 if base == 'chain' else 40


def general_hierarchy(A, free, coarse, hermitian=False):
    '''test_amg_host.hierarchy with the inverse of the dense level taken as the device takes it with symmetric=False: numpy.linalg.pinv without hermitian=True'''
    levels = test_amg_host.hierarchy(A, free, coarse)
    last = levels[-1]
    if last.kind == 'dense' and not hermitian:
        last = types.SimpleNamespace(**vars(last))
        last.ainv = numpy.linalg.pinv(last.A.toarray()[numpy.ix_(last.idx, last.idx)])
        levels = levels[:-1] + [last]
    return levels


@functools.lru_cache(maxsize=None)
def levels_of(name, coarse=None):
    A, free, default = problem(name)
    return general_hierarchy(A, free, coarse or default)


def system(name):
    '''(A, free, b, x0, stop_rr) of a solve to RTOL: a random right-hand side, constrained dofs held at non-zero values'''
    A, free, _ = problem(name)
    n = A.shape[0]
    b = numpy.random.default_rng(4).normal(size=n)
    x0 = numpy.where(free, 0., 1 + .1 * numpy.arange(n) / n)
    r0 = numpy.linalg.norm((b - A @ x0)[free])
    return A, free, b, x0, (RTOL * r0) ** 2


@functools.lru_cache(maxsize=None)
def steps(name, precon, restart, coarse=None):
    '''Arnoldi steps of the restated solve to RTOL: precon 'amg' (the cycle of `levels_of`), 'amg-hermitian' (its dense level inverted with hermitian=True) or
    'diag' (Jacobi: test_gmres_host.gmres_reference)'''
    A, free, b, x0, stop_rr = system(name)
    n = A.shape[0]
    if precon == 'diag':
        x, it, outcome = gmres_reference(A, b, x0, free, numpy.where(free, 1 / A.diagonal(), 0.), stop_rr, restart, 10 * n, check=1)
    else:
        levels = levels_of(name, coarse) if precon == 'amg' else general_hierarchy(*problem(name)[:2], coarse or problem(name)[2], hermitian=True)
        x, it, outcome, _ = fgmres_reference(A, b, x0, free, lambda r: test_amg_host.cycle(levels, r), stop_rr, restart, 10 * n, check=1)
    assert outcome == 'converged', (name, precon, restart, outcome)
    assert numpy.linalg.norm((b - A @ x)[free]) <= stop_rr ** .5
    return it


# ---- the restatement is flexible GMRES -------------------------------------------------------------------------------------

def dense_case(n, seed, constrained):
    rng = numpy.random.default_rng(seed)
    A = 3 * numpy.eye(n) + rng.normal(size=(n, n)) / numpy.sqrt(n)  # nonsymmetric, well conditioned
    A = numpy.diag(rng.uniform(.5, 2., n)) @ A
    b = rng.normal(size=n)
    free = rng.uniform(size=n) < .75 if constrained else numpy.ones(n, dtype=bool)
    free[:2] = True
    x0 = numpy.where(free, 0., rng.normal(size=n))
    return A, b, free, x0


@pytest.mark.parametrize('constrained', [True, False], ids=['constrained', 'free'])
@pytest.mark.parametrize('n', [5, 9, 12])
def test_estimate_is_the_least_squares_minimum(n, constrained):
    '''With a preconditioner that changes from step to step, M_j = (1 + j / 10) D_j^-1 with D_j the diagonal of A rolled by j places: after j steps
    sqrt(RR) = min_y |r0 - A Z_j y| over the columns Z_j = [M_0 v_0, .., M_(j-1) v_(j-1)] the cycle kept, Z[k] has the bytes of M_k(V[k]), and after the
    update the true residual is that minimum.  An update with the last preconditioner applied to V y -- right-preconditioned GMRES, which is what the device
    did before it kept Z -- is not: its residual is far above the tolerance.

    The tolerance is that of test_gmres_host.test_estimate_is_the_least_squares_minimum with B = A Z_j: e |r0| (1 + cond(B)), e = 8 j (n + 2) u (lstsq is
    backward stable, the columns of B are j rounded products from the basis, the residual is formed in j + 1 terms, the restatement is a backward stable
    GMRES on A Z_j = V_(j+1) H_j).  Z_j is an orthonormal basis times j diagonal scalings of condition below 8, so cond(B) stays modest for every j.'''
    A, b, free, x0 = dense_case(n, 40 + n, constrained)
    nfree = int(free.sum())
    d = numpy.diag(A)
    precon = lambda v, j: numpy.where(free, (1 + j / 10) * v / numpy.roll(d, j), 0.)
    r0 = numpy.where(free, b - A @ x0, 0.)
    norm = numpy.linalg.norm(r0)
    cyc = FlexCycle(lambda y: A @ y, free, precon, x0, nfree)
    cyc.init(r0)
    for j in range(1, nfree + 1):
        cyc.step(0.)
        assert cyc.COUNT == j
        for k in range(j):
            assert numpy.array_equal(cyc.Z[k], precon(cyc.V[k], k))
        B = numpy.where(free[:, None], A @ cyc.Z[:j].T, 0.)
        y = numpy.linalg.lstsq(B, r0, rcond=None)[0]
        minimum = numpy.linalg.norm(r0 - B @ y)
        cond = numpy.linalg.cond(B)
        tol = 8 * j * (n + 2) * U * norm * (1 + cond)
        print(f'n={n} j={j}: estimate {numpy.sqrt(cyc.RR):.6e}, minimum {minimum:.6e}, difference {abs(numpy.sqrt(cyc.RR) - minimum):.1e}, tolerance {tol:.1e}, cond {cond:.1e}')
        assert tol <= 1e-10 * norm
        assert abs(numpy.sqrt(cyc.RR) - minimum) <= tol
        if j == nfree - 1:  # the update of a cycle that has not solved the system: the estimate is the true residual
            part = FlexCycle(lambda y: A @ y, free, precon, x0, nfree)
            part.init(r0)
            part.iterate(j, 0.)
            estimate = numpy.sqrt(part.RR)
            part.update()
            true = numpy.linalg.norm(numpy.where(free, b - A @ part.x, 0.))
            assert estimate > 1e-6 * norm and abs(true - estimate) <= tol
            # x0 + M V y for the last M: not flexible GMRES
            wrong = x0 + precon(part.Y[:j] @ part.V[:j], j - 1)
            assert numpy.linalg.norm(numpy.where(free, b - A @ wrong, 0.)) > estimate + 1e-3 * norm
    assert cyc.ST == ST_DONE and cyc.FLAG  # (the space of nfree dimensions is full: the lucky breakdown)
    cyc.update()
    assert numpy.array_equal(cyc.x[~free], x0[~free])
    assert numpy.linalg.norm(numpy.where(free, b - A @ cyc.x, 0.)) <= tol
    for y in (cyc.z, cyc.w, cyc.t, *cyc.V, *cyc.Z):
        assert not y[~free].any()


def test_a_fixed_preconditioner_gives_the_cycle_of_test_gmres_host():
    '''with M = dinv for every step the flexible cycle is the right-preconditioned one: the same estimates, bit for bit, and the same x to rounding'''
    A, b, free, x0 = dense_case(12, 7, True)
    dinv = numpy.where(free, 1 / numpy.diag(A), 0.)
    r0 = numpy.where(free, b - A @ x0, 0.)
    flex, fixed = FlexCycle(lambda y: A @ y, free, lambda v, j: dinv * v, x0, 6), Cycle(lambda y: A @ y, free, dinv, x0, 6)
    for cyc in (flex, fixed):
        cyc.init(r0)
        cyc.iterate(8, 0.)
        cyc.update()
    assert flex.COUNT == fixed.COUNT == 6 and flex.estimates == fixed.estimates
    assert numpy.array_equal(flex.V, fixed.V)
    assert numpy.abs(flex.x - fixed.x).max() <= 64 * U * numpy.abs(fixed.x).max()


# ---- the host loop of krylov.solve around the restatement ----------------------------------------------------------------------

class HostFlex(krylov.Fgmres):
    '''krylov.Fgmres with its 'amg' variant's rules (admit, flagged, finish, and `advance`, which clips a look to what the cycle has left) on a FlexCycle
    instead of the device: what is overridden is what touches it -- the residual of a start, the kernels, the read-back'''

    def __init__(self, cyc, A, b, free):
        self.rec, self.A_, self.b, self.free = cyc, A, b, free
        self.cycle = self.left = cyc.m
        self.looks = []

    work = property(lambda self: numpy.array([self.rec.RR, self.rec.FLAG, self.rec.COUNT], dtype=float))

    def start(self):
        self.rec.init(numpy.where(self.free, self.b - self.A_ @ self.rec.x, 0.))
        return float(self.rec.RR)

    def iterate(self, steps, stop_rr):
        assert 1 <= steps <= self.rec.m - self.rec.COUNT  # no more than the cycle has left: a step past its end would run a V-cycle for nothing
        self.looks.append(steps)
        self.rec.iterate(steps, stop_rr)

    def update(self):
        self.rec.update()

    def solution(self):
        return self.rec.x


def loop(A, b, x0, free, precon, rtol, restart, maxiter, check):
    '''(x, iterations, cycles, outcome, looks) of krylov.solve around a FlexCycle'''
    m = max(1, min(restart, int(free.sum())))
    rec = HostFlex(FlexCycle(lambda y: A @ y, free, precon, numpy.array(x0, dtype=float), m), A, b, free)
    try:
        x, outcome = krylov.solve(rec, 0., rtol, maxiter, check), 'converged'
    except matrix.ToleranceNotReached as e:
        x, outcome = e.best, 'maxiter'
    except matrix.MatrixError as e:
        x, outcome = rec.solution(), str(e)
    return x, rec.iterations, rec.rec.cycles, outcome, rec.looks


@pytest.mark.parametrize('restart', [1, 4, 30])
def test_host_loop(restart):
    '''krylov.solve against `fgmres_reference` on a small system with the step-dependent preconditioner: bytes of x, steps, cycles, outcome and the steps of
    every look, for `check` 1, 5 and 16 and maxiter below, at and above what the solve needs'''
    A, b, free, x0 = dense_case(12, 11, True)
    d = numpy.diag(A)
    precon = lambda v, j: numpy.where(free, (1 + j / 10) * v / d, 0.)
    r0 = numpy.where(free, b - A @ x0, 0.)
    rtol = 1e-12
    stop_rr = max(0., rtol * float(r0 @ r0) ** .5) ** 2
    need = fgmres_reference(A, b, x0, free, precon, stop_rr, restart, 1000, 1)[1]
    assert need >= 6  # (a look of 16 steps has something to clip or to idle through, looks of 5 come in runs)
    seen = set()
    for maxiter in (need // 2, need - 1, need, need + 3):
        for check in (1, 5, 16):
            x, it, outcome, cyc = fgmres_reference(A, b, x0, free, precon, stop_rr, restart, maxiter, check)
            y, it_real, cycles, outcome_real, looks = loop(A, b, x0, free, precon, rtol, restart, maxiter, check)
            assert (it_real, cycles, outcome_real, looks) == (it, cyc.cycles, outcome, cyc.looks), (restart, maxiter, check)
            assert x.tobytes() == y.tobytes()
            assert max(looks) <= min(check, restart)
            seen.add(outcome)
    assert seen == {'converged', 'maxiter'}


def test_host_loop_on_a_singular_matrix():
    '''the rule of 'fgmres' holds for the flexible variant: a direction that vanishes without progress is MatrixError('fgmres: singular matrix')'''
    free = numpy.ones(2, dtype=bool)
    identity = lambda v, j: v
    x, it, cycles, outcome, looks = loop(numpy.diag([1., 0.]), numpy.array([1., 1.]), numpy.zeros(2), free, identity, 1e-12, 30, 2, 16)
    assert outcome == 'fgmres: singular matrix' and it in (1, 2) and x[0] == 1
    assert fgmres_reference(numpy.diag([1., 0.]), numpy.array([1., 1.]), numpy.zeros(2), free, identity, 1e-24, 30, 2)[2] == 'singular'
    x, it, cycles, outcome, looks = loop(numpy.zeros((2, 2)), numpy.array([1., 1.]), numpy.zeros(2), free, identity, 1e-12, 30, 2, 16)
    assert (it, outcome) == (0, 'fgmres: singular matrix')
    x, it, cycles, outcome, looks = loop(numpy.eye(2), numpy.array([1., numpy.inf]), numpy.zeros(2), free, identity, 1e-12, 30, 2, 16)
    assert (it, outcome) == (0, 'fgmres: non-finite residual')


# ---- what the cycle buys: the counts the GPU tests rely on ---------------------------------------------------------------------

@pytest.mark.parametrize('name', ['chain', 'convdiff'])
def test_cycle_against_jacobi(name):
    '''at restart 30 the cycle needs at most a quarter of the steps of Jacobi (measured when this was written: 37 / 2156 on the chain, 37 / 292 on
    convection-diffusion)'''
    levels = levels_of(name)
    cycle_steps, jacobi_steps = steps(name, 'amg', 30), steps(name, 'diag', 30)
    print(f'{name}: levels {[lv.nfree for lv in levels]}, {cycle_steps} steps with the cycle, {jacobi_steps} with Jacobi')
    assert len(levels) == 3
    assert 4 * cycle_steps <= jacobi_steps


def test_skewed_laplace_and_restarts():
    '''the other counts of the table the feature was proposed with, printed; the cycle never needs more steps than Jacobi, at any restart'''
    for name, restart in (('laplace', 30), ('laplace', 5), ('chain', 5), ('convdiff', 10)):
        cycle_steps, jacobi_steps = steps(name, 'amg', restart), steps(name, 'diag', restart)
        print(f'{name}, restart {restart}: {cycle_steps} steps with the cycle, {jacobi_steps} with Jacobi')
        assert cycle_steps < jacobi_steps
    one = steps('chain', 'amg', 1)
    print(f'chain, restart 1: {one} steps')
    assert steps('chain', 'amg', 30) <= one <= 2 * steps('chain', 'amg', 30)


@pytest.mark.parametrize('name,coarse', [('spd-laplace', 40), ('spd-laplace', 256), ('spd-chain', 256)])
def test_no_worse_than_cg_on_spd_matrices(name, coarse):
    '''unrestarted flexible GMRES minimises the residual over the space CG searches: steps <= iterations of CG with the same cycle + 2 (measured: 39 / 39,
    36 / 36, 26 / 27)'''
    A, free, b, x0, stop_rr = system(name)
    levels = levels_of(name, coarse)
    _, cg_iterations, _, outcome = test_amg_host.pcg_reference(A, b, x0, free, lambda r: test_amg_host.cycle(levels, r), stop_rr, A.shape[0])
    assert outcome == 'converged'
    gmres_steps = steps(name, 'amg', 1000, coarse)
    print(f'{name}, coarse {coarse}: {gmres_steps} steps, CG {cg_iterations} iterations')
    assert gmres_steps <= cg_iterations + 2


@pytest.mark.parametrize('name', ['block', 'scattered'])
def test_dense_level_zero_needs_the_general_inverse(name):
    '''100 free dofs of 1480 are a dense level at once: its general inverse is the inverse of the free block, one step; numpy.linalg.pinv(hermitian=True) of a
    nonsymmetric block is the inverse of another matrix, several'''
    levels = levels_of(name)
    assert [lv.kind for lv in levels] == ['dense'] and levels[0].nfree == 100
    general, hermitian = steps(name, 'amg', 30), steps(name, 'amg-hermitian', 30)
    print(f'{name}: {general} step with the general inverse, {hermitian} with hermitian=True')
    assert general == 1 < hermitian


def test_lagged_cycle():
    '''the hierarchy of velocity (3, -2) on the matrix of velocity (6, -4): within 1.5 x + 2 of the steps with its own (measured: 40 against 37)'''
    A, free, b, x0, stop_rr = system('convdiff6')
    lagged = levels_of('convdiff')
    x, it, outcome, _ = fgmres_reference(A, b, x0, free, lambda r: test_amg_host.cycle(lagged, r), stop_rr, 30, A.shape[0], check=1)
    own = steps('convdiff6', 'amg', 30)
    print(f'lagged {it} steps, own {own}')
    assert outcome == 'converged' and it <= 1.5 * own + 2


# ---- errors before any device work ---------------------------------------------------------------------------------------------

def fake(kind='amg', shape=(2, 2), free=(True, True), symmetric=True):
    '''a preconditioner object as `getprecon` makes it, without what lives on a device: `solve` refuses before it looks there'''
    return amg.Preconditioner(kind, shape, numpy.array(free), symmetric, None, None)


def test_solve_errors_come_before_any_device_work():
    A = matrix.HipMatrix(numpy.array([2., -1., -3., 2.]), numpy.array([0, 2, 4]), numpy.array([0, 1, 0, 1]), 2)
    b = numpy.ones(2)
    with pytest.raises(matrix.MatrixError, match='preconargs'):
        A.solve(b, solver='fgmres', rtol=1e-8, precon=fake(), preconargs=dict(coarse=16))
    with pytest.raises(matrix.MatrixError, match='built for a 3x3 matrix'):
        A.solve(b, solver='fgmres', rtol=1e-8, precon=fake(shape=(3, 3), free=(True,) * 3))
    with pytest.raises(matrix.MatrixError, match='another set of free dofs'):
        A.solve(b, solver='fgmres', rtol=1e-8, precon=fake(), constrain=numpy.array([numpy.nan, 1.]))
    with pytest.raises(matrix.MatrixError, match='another set of free dofs'):
        A.solve(b, solver='cg', rtol=1e-8, precon=fake('diag', free=(True, False)), constrain=numpy.array([True, False]))
    for solver in ('bicgstab', 'minres'):
        with pytest.raises(matrix.MatrixError, match="'fgmres'"):
            A.solve(b, solver=solver, rtol=1e-8, precon=fake())
    with pytest.raises(matrix.MatrixError, match='symmetric=False'):
        A.solve(b, solver='cg', rtol=1e-8, precon=fake(symmetric=False))
    with pytest.raises(matrix.MatrixError, match='restart'):
        A.solve(b, solver='fgmres', rtol=1e-8, precon=fake(), restart=0)
    with pytest.raises(matrix.MatrixError, match='tolerance'):
        A.solve(b, solver='fgmres', precon=fake())
    for precon in (fake(), fake('diag')):
        with pytest.raises(matrix.MatrixError, match='takes one right-hand side at a time'):
            A.solve_columns(numpy.ones((2, 2)), rtol=1e-8, precon=precon)
    # neither a name, None nor such an object: today's error; a Python callable among them
    for precon in (lambda r: r, 3, object(), 'ilu', b'amg'):
        for solver in ('cg', 'fgmres', 'bicgstab', 'minres'):
            with pytest.raises(matrix.MatrixError, match='invalid preconditioner'):
                A.solve(b, solver=solver, rtol=1e-8, precon=precon)
    # the string keeps every refusal it had
    for solver in ('bicgstab', 'fgmres', 'minres'):
        with pytest.raises(matrix.MatrixError, match='invalid preconditioner'):
            A.solve(b, solver=solver, rtol=1e-8, precon='amg')
    with pytest.raises(matrix.MatrixError, match='preconargs are the arguments of'):
        A.solve(b, solver='fgmres', rtol=1e-8, precon='diag', preconargs=dict(coarse=16))
    assert A._dev is None and A.iterations is None  # nothing was uploaded


def test_getprecon_errors_come_before_any_device_work():
    A = matrix.HipMatrix(numpy.array([2., -1., -3., 2.]), numpy.array([0, 2, 4]), numpy.array([0, 1, 0, 1]), 2)
    for symmetric in (True, False):
        for bad, message in ((dict(coarse=0), 'coarse must be'), (dict(coarse=1025), 'coarse must be'), (dict(sweeps=0), 'sweeps must be'), (dict(sweeps=1.5), 'sweeps must be'),
                             (dict(levels=3), 'invalid arguments'), (dict(coarse=16, cycle='W'), 'invalid arguments'), (dict(setup='rows'), 'setup must be'),
                             (dict(setup='block'), "needs `nullspace`"), (dict(smoother='ssor'), 'smoother must be'), (dict(degree=2), "arguments of smoother='chebyshev'"),
                             (dict(smoother='chebyshev', sweeps=2), 'sweeps counts'), (dict(nullspace=numpy.ones((3, 1))), 'nullspace must have the shape'),
                             (dict(nullspace=numpy.ones((2, 7))), 'between 1 and 6')):
            with pytest.raises(matrix.MatrixError, match=message):
                A.getprecon('amg', symmetric=symmetric, **bad)
    with pytest.raises(matrix.MatrixError, match='Lanczos'):
        A.getprecon('amg', smoother='chebyshev', symmetric=False)
    with pytest.raises(matrix.MatrixError, match='Lanczos'):
        A.getprecon('amg', smoother='chebyshev', degree=3, symmetric=False, constrain=numpy.array([numpy.nan, 1.]))
    with pytest.raises(matrix.MatrixError, match='invalid arguments'):
        A.getprecon('diag', coarse=16)
    for precon in ('ilu', None, lambda r: r):
        with pytest.raises(matrix.MatrixError, match='invalid preconditioner'):
            A.getprecon(precon)
    with pytest.raises(matrix.MatrixError, match='constraints have shape'):
        A.getprecon('amg', constrain=numpy.zeros(3))
    B = matrix.HipMatrix(numpy.array([2., -1., -3.]), numpy.array([0, 2, 3]), numpy.array([0, 1, 0]), 3)
    with pytest.raises(matrix.MatrixError, match='not square'):
        B.getprecon('amg')
    assert A._dev is None and A._amg is None and B._dev is None


def test_preconditioner_object():
    M = fake(symmetric=False)
    assert (M.kind, M.shape, M.symmetric) == ('amg', (2, 2), False) and 'amg' in repr(M)
    with pytest.raises(matrix.MatrixError, match='vector of 2 entries'):
        M(numpy.ones(3))
    with pytest.raises(matrix.MatrixError, match='vector of 2 entries'):
        M(numpy.ones((2, 2)))


def test_system_hands_linargs_on_untouched():
    '''solver.System passes the objects of `linargs` to `solve` as they are: neither copied nor turned into text'''
    from nutils_amd import solver
    M, seen = fake(), []

    class Jac:
        def solve(self, res, **kwargs):
            seen.append(kwargs)
            return res
        solve_leniently = solve
    system = types.SimpleNamespace(linear_iterations=[])
    dx = solver.System._linear_solve(system, Jac(), numpy.ones(2), dict(solver='fgmres', precon=M, rtol=1e-10), constrain=numpy.zeros(2, dtype=bool))
    assert seen[0]['precon'] is M and seen[0]['solver'] == 'fgmres' and numpy.array_equal(dx, numpy.ones(2))
    solver.System._linear_solve(system, Jac(), numpy.ones(2), dict(dict(solver='fgmres', precon=M), rtol=1e-3), lenient=True)  # (what a Newton solve makes of them)
    assert seen[1]['precon'] is M and len(system.linear_iterations) == 2


# ---- C ABI ---------------------------------------------------------------------------------------------------------------

def handle(n=3):
    '''a hierarchy of one diagonal level of n rows on pointers that are never followed (nh_amg_create checks its description on the host)'''
    lib = _lib.load()
    level = _lib.AmgLevel()
    level.A = csr(nrows=n, ncols=n)
    level.kind, level.w_dev = _lib.AMG_KINDS['diagonal'], P
    out = ctypes.c_void_p()
    assert lib.nh_amg_create(ctypes.byref(level), 1, ctypes.byref(out)) == 0 and out
    return out


def iterate(A, amg_handle, vectors=(P, P, ctypes.c_void_p(128), ctypes.c_void_p(256), P), work=P, restart=30, stop_rr=1e-20, niter=1):
    return _lib.load().nh_fgmres_iterate(A, None, amg_handle, *vectors, work, restart, stop_rr, niter, None)


def test_abi_refusals():
    lib = _lib.load()
    A = ctypes.byref(csr())
    h, h4 = handle(3), handle(4)
    try:
        refused(iterate(None, h), 'nh_fgmres_iterate', 'NULL matrix')
        refused(iterate(A, None), 'nh_fgmres_iterate', 'NULL hierarchy')
        refused(iterate(A, h4), 'nh_fgmres_iterate', 'another size')
        for i in range(5):  # V, Z, z, t, w
            vectors = [P, P, ctypes.c_void_p(128), ctypes.c_void_p(256), P]
            vectors[i] = None
            refused(iterate(A, h, vectors), 'nh_fgmres_iterate', 'NULL vector')
        refused(iterate(A, h, [P] * 5), 'nh_fgmres_iterate', "result is its argument")  # z is t
        refused(iterate(A, h, work=None), 'nh_fgmres_iterate', 'NULL vector')
        refused(iterate(ctypes.byref(csr(ncols=4)), h), 'nh_fgmres_iterate', 'square')
        refused(iterate(A, h, niter=-1), 'nh_fgmres_iterate', 'negative iteration count')
        refused(iterate(A, h, restart=0), 'nh_fgmres_iterate', 'restart')
        refused(iterate(A, h, restart=-3), 'nh_fgmres_iterate', 'restart')
        refused(iterate(A, h, stop_rr=-1e-300), 'nh_fgmres_iterate', 'negative')
        refused(iterate(A, h, stop_rr=float('nan')), 'nh_fgmres_iterate', 'negative')
        for fields, word in ((dict(nrows=-1), 'negative size'), (dict(lanes=3), 'power of two'), (dict(rowptr=None), 'NULL row pointers'), (dict(values=None), 'NULL values')):
            refused(iterate(ctypes.byref(csr(**fields)), h), 'nh_fgmres_iterate', word)
        # nothing to do is no error, and no launch: no steps, or an empty matrix with an empty hierarchy
        assert iterate(A, h, niter=0) == 0
    finally:
        for each in (h, h4):
            lib.nh_amg_free(each)


def test_table_and_wrapper_know_the_entry():
    from nutils_amd import kernels
    assert 'nh_fgmres_iterate' in _lib.SIGNATURES and len(_lib.SIGNATURES['nh_fgmres_iterate'][1]) == 13
    assert callable(kernels.fgmres_iterate)
