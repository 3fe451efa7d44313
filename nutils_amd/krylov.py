'''The host side of the device Krylov solves of `HipMatrix.solve`: ONE loop, `solve`, that decides when a solve returns, restarts or raises, around a `Recurrence`
that owns the vectors and the work array of its solver and says what is particular to it.  Nothing here needs a device to be imported: a recurrence imports
`device` and `kernels` when it is built, and the loop runs as well around a recurrence in numpy (tests/test_krylov_host.py).'''
import numpy

from .matrix import MatrixError, ToleranceNotReached


def solve(rec, atol, rtol, maxiter, check):
    '''Iterate `rec` until the true residual has |r| <= max(atol, rtol |r0|); returns `rec.solution()` and keeps `rec.iterations`.  A start reads r . r back, a
    look enqueues up to `check` iterations and reads r . r, the flag and the count back; a run of looks that ends without raising is followed by a new start.'''
    stop_rr, it = None, 0
    while True:  # a start: from the true residual
        rec.iterations = it  # (of the last solve, for whoever wants to know)
        rr = rec.start()
        if stop_rr is None:
            stop_rr = max(atol, rtol * rr ** .5) ** 2  # (the device compares r . r with this number, and so does the host)
        if not numpy.isfinite(rr):
            raise MatrixError(f'{rec.name}: non-finite residual')
        if rr <= stop_rr:
            return rec.solution()
        rec.admit(rr)
        if it >= maxiter:
            raise ToleranceNotReached(rec.solution())
        start = it
        while it < maxiter:  # a look
            rr, flag, count = rec.advance(min(check, maxiter - it), stop_rr)
            rec.iterations = it = start + int(count)
            if flag:
                rec.flagged(count)  # raises, or the run ends here
                break
            if not numpy.isfinite(rr):  # (never 'fgmres': its estimate is written only when finite, and a step that is not raises the flag)
                raise MatrixError(f'{rec.name}: non-finite residual')
            if rr <= stop_rr or count >= rec.cycle:
                break
        rec.finish(flag)


def _ready(precon):
    from . import amg
    return isinstance(precon, amg.Preconditioner)


class Recurrence:
    '''What `solve` iterates.  `start()` puts the true residual mask(rhs - A x) into r, initialises the recurrence and returns r . r; `advance(steps, stop_rr)`
    enqueues `steps` iterations and returns (r . r, flag, count) from one small read-back, count the iterations since the start that count; `solution()` is x as
    the caller wants it.  The rules are those of 'bicgstab' and 'minres'; a subclass makes its vectors, its work array, `init()` and `iterate(steps, stop_rr)`.'''

    cycle = float('inf')  # a run of looks ends when the count reaches it
    admit = finish = lambda self, arg: None  # admit(rr), at a start above the bound, may refuse to go on; finish(flag) follows a run of looks, before the next start

    def flagged(self, count):
        '''at a look that finds the flag up: after progress the run ends there, and the recurrence restarts from where it got to'''
        if not count:
            raise MatrixError(f'{self.name}: breakdown')

    def __init__(self, A, rhs, free, lhs, precon, on_device):
        from . import device, kernels
        self.A, self.kernels, self.csr = A, kernels, (*A.triplet(), A._ncols)
        ready = precon if _ready(precon) else None  # (an object of `getprecon`, which `solve` has checked against the matrix and the mask)
        self.mask, self.x, self.b, self.dinv = A._krylov_setup(rhs, free, lhs, None if ready else precon, on_device)
        if ready and ready.kind == 'diag':
            self.dinv = ready.dinv
        self.opts = dict(rowmask=self.mask, col32=A._columns(), lanes=A.lanes)
        self.vectors = lambda count, size=A.shape[0]: (device.empty(size, 'float64') for _ in range(count))
        (self.r,), x = self.vectors(1), self.x  # (no closure here or in a subclass holds `self`: a solve leaves no cycle behind to keep its vectors)
        self.solution = (lambda: x) if on_device else (lambda: device.to_host(x))

    def start(self):
        self.A.spmv(self.x, alpha=-1., beta=1., b=self.b, rowmask=self.mask, y=self.r)  # the true residual, mask(rhs - A x)
        self.init()
        return self.work[:1].item()

    def advance(self, steps, stop_rr):
        self.iterate(steps, stop_rr)
        return self.work[:3].tolist()


class Cg(Recurrence):
    '''the host counts what it enqueues: `iterations` is a multiple of `check`, or maxiter; any flag is the matrix's fault'''

    name = 'cg'
    count = 0

    def __init__(self, A, rhs, free, lhs, precon, on_device, preconargs):
        cycle = precon == 'amg' if isinstance(precon, str) else _ready(precon) and precon.kind == 'amg'
        super().__init__(A, rhs, free, lhs, None if cycle else precon, on_device)
        k, csr, opts, dinv, x, r, (p, q) = self.kernels, self.csr, self.opts, self.dinv, self.x, self.r, self.vectors(2)
        if cycle:  # z = M r is a V-cycle (nh_amg.hip); the rules are the same.  An object brings its hierarchy along: no numeric setup here
            hierarchy = precon.hierarchy if _ready(precon) else A._amg_hierarchy(free, self.mask, *preconargs)
            (z,), work = self.vectors(1), k.pcg_work()
            self.init = lambda: k.pcg_init(hierarchy.handle, r, z, p, work)
            self.iterate = lambda steps: k.pcg_iterate(*csr, amg=hierarchy.handle, x=x, r=r, z=z, p=p, q=q, work=work, niter=steps, **opts)
        else:
            work = k.cg_work()
            self.init = lambda: k.cg_init(dinv, r, p, work)
            self.iterate = lambda steps: k.cg_iterate(*csr, dinv=dinv, x=x, r=r, p=p, q=q, work=work, niter=steps, **opts)
        self.work, self.look = work, lambda: work[:2].tolist()
        self.stop = lambda stop_rr: k.cg_stop(work, stop_rr)  # (the iterations enqueued past convergence idle: their r . z would underflow before r . r, a false breakdown)

    def advance(self, steps, stop_rr):
        if not self.count:  # after the checks of a start, whose `init` cleared the cell
            self.stop(stop_rr)
        self.iterate(steps)
        self.count += steps
        return (*self.look(), self.count)

    def flagged(self, count):
        raise MatrixError('cg: matrix is not positive definite')

    def finish(self, flag):
        self.count = 0


class Bicgstab(Recurrence):
    name = 'bicgstab'  # (a start takes a fresh shadow residual)

    def __init__(self, A, *args):
        super().__init__(A, *args)
        k, csr, opts, dinv, x, r, (rhat, p, v, s, t) = self.kernels, self.csr, self.opts, self.dinv, self.x, self.r, self.vectors(5)
        phat, shat = self.vectors(2) if dinv is not None else (None, None)
        work = self.work = k.bicgstab_work()
        self.init = lambda: k.bicgstab_init(dinv, r, rhat, p, phat, work)
        self.iterate = lambda steps, stop_rr: k.bicgstab_iterate(*csr, dinv=dinv, x=x, r=r, rhat=rhat, p=p, v=v, s=s, t=t, phat=phat, shat=shat, work=work, stop_rr=stop_rr, niter=steps, **opts)


class Minres(Recurrence):
    name = 'minres'

    def __init__(self, A, *args):
        super().__init__(A, *args)
        dinv = None if self.dinv is None else self.dinv.abs()  # (the preconditioner of MINRES is positive definite: 1 / |diag|)
        k, csr, opts, x, r, (r1, r2, v, q, w1, w2) = self.kernels, self.csr, self.opts, self.x, self.r, self.vectors(6)
        work = self.work = k.minres_work()
        self.init = lambda: k.minres_init(dinv, r, r1, r2, v, w1, w2, work)
        self.iterate = lambda steps, stop_rr: k.minres_iterate(*csr, dinv=dinv, x=x, r=r, r1=r1, r2=r2, v=v, q=q, w1=w1, w2=w2, work=work, stop_rr=stop_rr, niter=steps, **opts)


class Fgmres(Recurrence):
    '''a start begins a cycle of up to `cycle` Arnoldi steps, which ends with x += M^-1 V y.  With an 'amg' object the method is flexible in earnest: step j keeps
    Z_j = M v_j, what the V-cycle returned, and the cycle ends with x += Z y: `cycle` more vectors on the device, 2 cycle + 1 in all.  A step enqueued past a
    stop moves nothing but still runs its V-cycle, so a look of that variant enqueues no more steps than the cycle has left.  A 'schur' object (the block
    preconditioner of a saddle point) takes the same branch with its own entry point, nh_fgmres_iterate_schur.'''

    name = 'fgmres'
    since = rr_start = None  # since: cycles finished since one ended on a vanished direction (0: the last one did)
    left = None  # the 'amg' variant: the steps its cycle has left

    def __init__(self, A, rhs, free, lhs, precon, on_device, restart):
        cycle = _ready(precon) and precon.kind in ('amg', 'schur')
        super().__init__(A, rhs, free, lhs, None if cycle else precon, on_device)
        m = self.cycle = max(1, min(restart, int(free.sum())))  # (a Krylov space has no more dimensions than there are free dofs)
        k, csr, opts, dinv, x, r, (z, w) = self.kernels, self.csr, self.opts, self.dinv, self.x, self.r, self.vectors(2)
        V, = self.vectors(1, (m + 1) * A.shape[0])
        work = self.work = k.gmres_work(m)
        if cycle:
            (t,), (Z,), hierarchy = self.vectors(1), self.vectors(1, m * A.shape[0]), precon.hierarchy  # (the closure keeps the hierarchy alive, as Cg's does)
            self.left = m
            self.init = lambda: k.gmres_init(None, r, V, z, work, restart=m)
            if precon.kind == 'schur':  # the block solve of a saddle point in place of the cycle: the same vectors and rules
                schur = precon.schur
                self.iterate = lambda steps, stop_rr: k.fgmres_iterate_schur(*csr, schur=schur.handle, V=V, Z=Z, z=z, t=t, w=w, work=work, restart=m, stop_rr=stop_rr, niter=steps, **opts)
            else:
                self.iterate = lambda steps, stop_rr: k.fgmres_iterate(*csr, amg=hierarchy.handle, V=V, Z=Z, z=z, t=t, w=w, work=work, restart=m, stop_rr=stop_rr, niter=steps, **opts)
            self.update = lambda: k.gmres_update(None, Z, x, work, restart=m)
            return
        self.init = lambda: k.gmres_init(dinv, r, V, z, work, restart=m)
        self.iterate = lambda steps, stop_rr: k.gmres_iterate(*csr, dinv=dinv, V=V, z=z, w=w, work=work, restart=m, stop_rr=stop_rr, niter=steps, **opts)
        self.update = lambda: k.gmres_update(dinv, V, x, work, restart=m)

    def advance(self, steps, stop_rr):
        if self.left is None:
            return super().advance(steps, stop_rr)
        rr, flag, count = super().advance(min(steps, self.left), stop_rr)
        self.left = self.cycle - int(count)
        return rr, flag, count

    def admit(self, rr):
        if self.since in (0, 1) and not rr < self.rr_start:
            # A direction has vanished: the Krylov space of that start was exhausted, which for a nonsingular matrix means the update solved the system to
            # rounding.  If that cycle got nowhere, or the next one on what rounding left of the residual (on diag(1, 0) it finds a direction of the size of
            # a rounding in x, and no flag), the matrix is singular.  Later cycles that stagnate are restarted GMRES stagnating: they run to maxiter.
            raise MatrixError('fgmres: singular matrix')
        self.rr_start = rr

    flagged = lambda self, count: None  # (a new direction vanished or is not finite: the cycle ends there)

    def finish(self, flag):
        self.since = 0 if flag else None if self.since is None else self.since + 1
        self.update()
        if self.left is not None:
            self.left = self.cycle  # (the next start begins a new cycle)
