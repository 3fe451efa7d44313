'''Probe of solver.System on its two routes: the host route (the Jacobian's values travel to page-locked host memory, the free block goes to scipy's direct
solver) and the device route (`matrix.backend('hip')`: the Jacobian stays in HBM as a HipMatrix, constraints are the row mask of a Krylov solve on the device,
`linargs` name the solver).  One JSON line per workload with, per route, the two halves of one Newton step -- for a linear system that step is the solve --

  * assemble: System.assemble_jacobian_residual for the iterate (host route: reduced to the free dofs, as System.solve asks for it), wall clock around a
    synchronised device; `cold` is the first call (merge plan, index tensors, first hand-over: everything that happens once per system), `warm` the median of
    --reps later ones,
  * solve: the linear solve System.solve would do next, with the Krylov iteration count and the relative residual |res - J dx| / |res| on the free dofs,

and the lengths of what crossed PCIe towards the host during a warm step (device.to_host, and the entries the host mirror has the device write).

Workloads: `laplace` (the Laplace example, --laplace N elements per side, CG; also times solve_constraints), `elasticity96` (trilinear elasticity on 96^3
elements, one face clamped and the opposite one displaced, CG), `cahnhilliard512` (one Newton step of the implicit Cahn-Hilliard step on 512^2 quadratic spline
elements from a random state, Jacobi-BiCGStab; --newton-solver names the device solver of that step, and a list such as bicgstab,minres reports the step
once per solver, the first under `device`, the others under `device_<solver>`: the Jacobian is symmetric with a saddle).  The host route's direct solve is run up to --host-solve-dofs unknowns (3-D fill-in makes it a matter of hours
and of hundreds of GB beyond); its assembly half is always run.

Usage: python tools/system_probe.py [--workloads laplace,elasticity96,cahnhilliard512] [--scale 1.0] [--newton-solver bicgstab,minres] [--out FILE]
(--scale shrinks every mesh for a quick look).  Not run by any test; no time in here is a pass criterion.'''
import argparse
import contextlib
import json
import os
import sys
import time
import warnings

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def laplace(n):
    from nutils_amd import mesh, function
    domain, geom = mesh.unitsquare(n, 'square')
    u = domain.field('u', btype='std', degree=1)
    v = domain.field('v', btype='std', degree=1)
    dV = function.J(geom)
    grad = lambda w: function.grad(w, geom)
    res = domain.integral((grad(v) * grad(u)).sum(-1) * dV, degree=2)
    flux = function.PointFunc(lambda x: numpy.cos(1) * numpy.cosh(x[:, 1]), geom)
    res -= domain.boundary['right'].integral(v * flux * dV, degree=2)
    g = function.PointFunc(lambda x: numpy.cosh(1) * numpy.sin(x[:, 0]), geom)
    sqr = domain.boundary['left'].integral(u * u * dV, degree=2)
    top = domain.boundary['top']
    sqr += top.integral(u * u * dV, degree=2) - 2 * top.integral(u * g * dV, degree=2) + top.integral(g * g * dV, degree=2)
    return sqr, res


def elasticity(n):
    from nutils_amd import mesh, function
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1, n + 1)] * 3)
    u = domain.field('u', btype='std', degree=1, shape=[3])
    v = domain.field('v', btype='std', degree=1, shape=[3])
    eps = lambda w: function.symgrad(w, geom)
    res = domain.integral(function.inner(eps(v), function.div(u, geom) * function.eye(3) + 1.3 * eps(u)) * function.J(geom), degree=2)
    cons = numpy.full((n + 1, n + 1, n + 1, 3), numpy.nan)
    cons[0] = 0.
    cons[-1] = [0., .05, -.1]
    return res, cons.reshape(-1, 3)


def cahnhilliard(n):
    from nutils_amd import mesh, function
    size, eps, M, stens, wn, wp, dt = 10., 1., 1., 50., 30., 20., .5
    domain, geom = mesh.rectilinear([numpy.linspace(0, size, n + 1)] * 2)
    phi = domain.field('φ', btype='spline', degree=2)
    phi0 = domain.field('φ0', btype='spline', degree=2)
    eta = domain.field('η', btype='spline', degree=2) * (stens / eps)
    p, p0 = function.value(phi), function.value(phi0)
    dp = p - p0
    psi = .25 * (p ** 2 - 1) ** 2
    dpsi = .25 * dp ** 2 * (1 - p ** 2 + 2 * p * dp / 3 - dp ** 2 / 6)
    dV = function.J(geom)
    grad = lambda w: function.grad(w, geom)
    nrg = domain.integral((psi + dpsi) * (stens / eps) * dV, degree=8) \
        + domain.integral(.5 * stens * eps * (grad(phi) * grad(phi)).sum(-1) * dV, degree=8) \
        - domain.integral(eta * phi * dV, degree=8) + domain.integral(eta * phi0 * dV, degree=8) \
        - domain.integral(.5 * dt * M * (grad(eta) * grad(eta)).sum(-1) * dV, degree=8) \
        + domain.boundary.integral((wp + wn) / 2 * dV, degree=4) + domain.boundary.integral((wp - wn) / 2 * phi * dV, degree=4)
    nd = len(phi.arg.basis)
    start = numpy.random.default_rng(0).uniform(-1, 1, nd)  # (the example's random initial condition)
    return nrg, {'φ': start, 'φ0': start, 'η': numpy.zeros(nd)}


@contextlib.contextmanager
def pcie_log():
    '''lengths of what comes to the host: device.to_host, and the index_copy calls whose destination is page-locked host memory (the host mirror)'''
    from nutils_amd import device, kernels
    lengths, to_host, index_copy = [], device.to_host, kernels.index_copy

    def logged_to_host(tensor):
        lengths.append(tensor.numel())
        return to_host(tensor)

    def logged_index_copy(src, dst, src_index=None, dst_index=None):
        if not dst.is_cuda:
            lengths.append((src_index if src_index is not None else dst_index if dst_index is not None else src).numel())
        return index_copy(src, dst, src_index=src_index, dst_index=dst_index)
    device.to_host, kernels.index_copy = logged_to_host, logged_index_copy
    try:
        yield lengths
    finally:
        device.to_host, kernels.index_copy = to_host, index_copy


def clock(fn):
    from nutils_amd import device
    device.synchronize()
    t0 = time.perf_counter()
    out = fn()
    device.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def step(system, arguments, constrain, linargs, on_device, solve, lengths=None):
    '''the two halves of one iteration of System.solve, timed apart -> (assemble ms, solve record or None)'''
    from nutils_amd import matrix
    x, free = system._pack(dict(arguments), constrain)
    args = system._unpack(dict(arguments), x)
    sub = None if on_device or free.all() else free
    assemble_ms, (jac, res) = clock(lambda: system.assemble_jacobian_residual(args, sub, copy=False))
    if not solve:
        return assemble_ms, None
    system.linear_iterations = []
    rhs, kwargs = (res, dict(constrain=~free)) if on_device else (res if sub is None else res[free], {})
    record = dict(converged=True)

    def run():
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter('always')
                dx = system._linear_solve(jac, rhs, linargs if on_device else None, not system.is_linear, **kwargs)
            if caught:
                record['converged'] = False
            return dx
        except matrix.ToleranceNotReached as e:
            record['converged'] = False
            return e.best
    record['ms'], dx = clock(run)
    keep = free if on_device or sub is None else numpy.ones(len(rhs), dtype=bool)
    mark = len(lengths) if lengths is not None else 0  # (the product of the check below is the probe's own traffic)
    record['iterations'] = system.linear_iterations[-1] if system.linear_iterations else getattr(jac, 'iterations', None)
    record['relative_residual'] = float(numpy.linalg.norm((rhs - jac @ dx)[keep]) / numpy.linalg.norm(rhs[keep]))
    if lengths is not None:
        del lengths[mark:]
    return assemble_ms, record


def route(make, arguments, constrain, linargs, on_device, solve, reps):
    from nutils_amd import matrix
    out = {}
    with matrix.backend('hip') if on_device else contextlib.nullcontext():
        system = make()
        cold, _ = step(system, arguments, constrain, linargs, on_device, False)
        warm, solves = [], []
        with pcie_log() as lengths:
            for rep in range(reps):  # (the host route's direct solve once: it takes seconds to minutes)
                ms, record = step(system, arguments, constrain, linargs, on_device, solve and (on_device or rep == reps - 1), lengths)
                warm.append(ms)
                if record:
                    solves.append(record)
        out['assemble_ms'] = dict(cold=cold, warm=float(numpy.median(warm)))
        if solve:
            out['solve'] = dict(solves[-1], ms=float(numpy.median([s['ms'] for s in solves])))
        else:
            out['solve'] = 'not run: more unknowns than --host-solve-dofs'
        out['to_host_lengths_per_step'] = sorted(set(lengths), reverse=True)[:4]
        out['to_host_entries_per_step'] = int(sum(lengths) // reps)
        jac = system._device_jac[1] if on_device else None
        out['size'] = system.size
        if jac is not None:
            out['nnz'], out['lanes'] = jac.nnz, jac.lanes
    return out


def probe(name, args):
    from nutils_amd import matrix
    from nutils_amd.solver import System
    n = lambda full: max(2, int(round(full * args.scale)))
    info = dict(name=name)
    if name == 'laplace':
        info['elements'] = [n(args.laplace)] * 2
        sqr, res = laplace(n(args.laplace))
        linargs = dict(solver='cg', rtol=args.rtol, maxiter=args.maxiter)
        info['solve_constraints'] = {}
        for on_device in (False, True):
            with matrix.backend('hip') if on_device else contextlib.nullcontext():
                system = System(sqr, trial='u')
                kwargs = dict(linargs=linargs) if on_device else {}
                cold, cons = clock(lambda: system.solve_constraints(droptol=1e-15, **kwargs))
                warm = float(numpy.median([clock(lambda: system.solve_constraints(droptol=1e-15, **kwargs))[0] for _ in range(args.reps)]))
                info['solve_constraints']['device' if on_device else 'host'] = dict(cold_ms=cold, warm_ms=warm, iterations=system.linear_iterations[-1],
                                                                                    constrained=int((~numpy.isnan(cons['u'])).sum()))
        make, arguments, constrain = (lambda: System(res, trial='u', test='v')), {}, cons
    elif name == 'elasticity96':
        info['elements'] = [n(96)] * 3
        res, cons = elasticity(n(96))
        linargs = dict(solver='cg', rtol=args.rtol, maxiter=args.maxiter)
        make, arguments, constrain = (lambda: System(res, trial='u', test='v')), {}, {'u': cons}
    elif name == 'cahnhilliard512':
        info['elements'] = [n(512)] * 2
        nrg, arguments = cahnhilliard(n(512))
        solvers = args.newton_solver.split(',')
        linargs = dict(solver=solvers[0], rtol=args.newton_rtol, maxiter=args.maxiter)
        make, constrain = (lambda: System(nrg, trial='φ,η')), None
    else:
        raise SystemExit(f'unknown workload {name!r}')
    info['linargs'] = linargs
    info['device'] = route(make, arguments, constrain, linargs, True, True, args.reps)
    if name == 'laplace':  # the same solve under the multigrid preconditioner: the first repetition builds the plan, the later ones reuse it (the median is theirs)
        info['device_amg'] = route(make, arguments, constrain, dict(linargs, precon='amg'), True, True, args.reps)
    if name == 'cahnhilliard512':
        for other in solvers[1:]:
            info['device_' + other] = route(make, arguments, constrain, dict(linargs, solver=other), True, True, args.reps)
    info['host'] = route(make, arguments, constrain, linargs, False, info['device']['size'] <= args.host_solve_dofs, args.reps)
    return info


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--workloads', default='laplace,elasticity96,cahnhilliard512')
    ap.add_argument('--scale', type=float, default=1.)
    ap.add_argument('--laplace', type=int, default=1024, help='elements per side of the Laplace example')
    ap.add_argument('--rtol', type=float, default=1e-8, help='relative tolerance of the linear workloads')
    ap.add_argument('--newton-rtol', type=float, default=1e-3, help="relative tolerance of the Newton step's linear solve (the default of System.solve)")
    ap.add_argument('--newton-solver', default='bicgstab', help="device solver of the cahnhilliard512 step; a comma-separated list reports the step once per solver")
    ap.add_argument('--maxiter', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-solve-dofs', type=int, default=1200000, help="largest system the host route's direct solver is run on")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    out = open(args.out, 'a') if args.out else None
    for name in args.workloads.split(','):
        line = json.dumps(probe(name, args), ensure_ascii=False)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
