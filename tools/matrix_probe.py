'''Probe of the device-resident matrix backend (matrix.HipMatrix, nh_csr.hip): one JSON line per matrix with

  * the time of a CSR product for every lanes-per-row count, from HIP events over windows of at least --window seconds after a warm-up, three windows
    each (median, and the spread (max - min) / median the comparisons are read against),
  * algorithmic bytes nnz (8 + 4) + nrows (8 + 8) + ncols 8 over that time, as a fraction of 8 TB/s (peak) and of 6.3 TB/s (achievable),
  * torch's own CSR product (torch.sparse_csr_tensor(...) @ x) timed in the same process, its windows alternating with ours,
  * what a user could do before this backend: device.to_host of the triplet plus the scipy product,
  * the time of a CG iteration, the product's share of it, and iterations and wall time of a Jacobi-CG solve to rtol = 1e-8 with one side held,
  * for the nonsymmetric twin N = K + 0.5 (triu(K, 1) - tril(K, -1)), built on the device from the value tensor: the time of a BiCGStab iteration against
    two products of the same run and against its vector passes at the stream rate, iterations, wall time and true residual of a Jacobi-BiCGStab solve under
    the conditions of the CG solve, and (unless --no-host-solve) the route a user had before: device.to_host of the triplet, the free submatrix and
    scipy.sparse.linalg.bicgstab with the same tolerance and Jacobi as a LinearOperator, timed once,
  * for the same twin, restarted GMRES at restart 10, 30 and 100: the time of an Arnoldi step (the mean over a full cycle, whose step j reads j + 1 basis
    vectors four times), the product's share of it and the share of everything else (the Gram-Schmidt kernels, the scalar kernel, the normalisation), the
    model's bytes of that rest, (4 (j + 1) + c) 8 n per step with c = 2 ceil((j + 1) / 8) + 8 passes over w, z, dinv and the new basis vector, over its time as a
    fraction of 8 TB/s, and steps, wall time and true residual of a Jacobi-GMRES solve under the conditions of the BiCGStab solve,
  * for the symmetric indefinite twin S (section 'minres'; the off-diagonal entries of K, the diagonal +-sum_j |K_ij| with the sign alternating from row to row:
    by Gershgorin |lambda| >= K_ii, half of the spectrum negative), built on the device from the value tensor: the time of a MINRES iteration against one
    product of the same run, and of a BiCGStab iteration and of a GMRES(30) step on the same matrix in the same process, their windows alternating; and
    iterations, wall time and true residual of a solve to rtol = 1e-8 by each of the three, on S and on the Helmholtz-like twin K - 0.01 diag(K), whose
    Jacobi-scaled spectrum crosses zero at its low end (the same pattern and kernels: the iteration times are those of S),
  * for the smoothed-aggregation AMG preconditioner (precon='amg'): the time of the symbolic and of the numeric phase of its setup, level sizes and operator
    complexity, one cycle against one masked product, and iterations, wall time and true residual of an AMG-CG solve (with the symbolic phase, and with it
    cached) beside the Jacobi-CG solve of the same system in the same process; for the vector matrices (elasticity96, p2vector32) all of that once more with
    the rigid-body modes as the near-nullspace (preconargs=dict(nullspace=amg.rigid_body_modes(coords))); with --amg-setup entry,block that part once per kind of
    plan (preconargs' `setup`), each with the products of its plans, the peak of torch's allocator during its symbolic phase, and its own solve,
  * for the smoothers of that preconditioner (section 'smoother'; the rigid-body modes for the vector matrices), in one process and alternating: Jacobi with one
    (the default) and two sweeps and Chebyshev of degree 2 and 3 -- the numeric setup with the share of its Lanczos estimates, the bounds of every level, one
    cycle, and iterations and wall time of the solve to rtol = 1e-8 with the symbolic phase cached; with --eigratios 4,10,30 the Chebyshev degree-2 solve for
    each ratio, and with --eigsteps 5,10,20 for each number of Lanczos steps,
  * for the matrix algebra (section 'algebra'; nh_csr_ops.hip): the wall time of `T`, of `submatrix(free, free)` and of two sums of different patterns (K + D, D
    the diagonal as a matrix of its own, a shifted operator; K + K^T on the tensors of the transpose, the same pattern met again) -- first, on a matrix without
    plans (the median of five after a warm-up, the device synchronised: these calls wait for the host), and with the plan (HIP events over windows, as the
    product) -- beside the host path of the same matrix in the same process (`_transpose_host`, `_submatrix_host`, `_add_host` on a matrix without a host
    copy, so the export is in it, as it was before; timed once, it takes seconds), with the bytes each device operation has to move and what fraction of
    8 TB/s that is,
  * for blocks of vectors (section 'columns', not in the default; nh_csr_multi.hip): at k = 1, 2, 4, 8 columns the time of the block product `spmm` against k calls of
    `spmv` in the same process, their windows alternating, with the algorithmic bytes of each -- nnz (8 + 4) + nrows 8 + k (nrows + ncols) 8 for the block product,
    which reads every (value, column) pair once, k (nnz (8 + 4) + nrows 16 + ncols 8) for the k products -- and the time of a batched CG iteration against k
    single-vector iterations (each timed call restores the residuals, starts the recurrences and enqueues 20 iterations, so that no window runs into convergence;
    the time is that call over 20),
  * for flexible GMRES with the AMG cycle (section 'flexible', not in the default; nh_fgmres_iterate): on the nonsymmetric twin, the setup of a preconditioner
    object (`getprecon('amg', symmetric=False)`, with and without the symbolic phase: the second is what a reused object saves every later solve), at restart
    10 and 30 the time of a step against a Jacobi-GMRES step and one cycle of the same run, their windows alternating, and steps, wall time (the median of
    three) and true residual of the solve to rtol = 1e-8 against Jacobi-GMRES at the same restart and Jacobi-BiCGStab in the same process; and a solve of
    the matrix one perturbation of the values further (off-diagonal entries scaled by factors within 10 % of one) with the old object against its own,
  * for the block preconditioner of a saddle point (section 'saddle', not in the default and not tied to --matrices; nh_schur_*, nh_fgmres_iterate_schur): one
    line per size of --stokes, the lid-driven Stokes problem on n x n Taylor-Hood elements (u of degree 2, p of degree 1) from the front end through
    solver.System: the setup of the object (`getprecon('schur')` with the SIMPLE diagonal and the component indicators as near-nullspace; first, and again on
    the next matrix of the pattern, where the symbolic phase and the plan of the transpose are there), one application against one product, and steps, wall
    time (the median of three) and true residual of the solve to rtol = 1e-8 by flexible GMRES(30) with the object -- built beforehand -- against BiCGStab,
    GMRES(30) and MINRES without a preconditioner in the same process, each capped at --maxiter iterations, the same object at restart 100, and an object
    whose Schur diagonal is minus the diagonal of the pressure mass matrix (`schur=`) at restart 30; and a solve of the matrix whose first block is
    1.05 A + 0.03 diag(A) with the old object against its own.

Usage: python tools/matrix_probe.py [--matrices poisson128,elasticity96,elasticity64,elasticity48,bilinear2048,bilinear1024,p2vector32,p2vector16] [--scale 1.0]
[--sections spmv,cg,bicgstab,fgmres,minres,amg,smoother,algebra,columns,flexible,saddle] [--stokes 16,32,64] [--amg-setup entry,block] [--eigratios 4,10,30] [--eigsteps 5,10,20] [--out FILE]
(--scale shrinks every mesh for a quick look; --sections leaves parts out).  Not run by any test.'''
import argparse
import json
import os
import sys
import time

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LANES = (4, 8, 16, 32, 64)


def build(name, scale):
    from nutils_amd import mesh, function
    n = lambda full: max(2, int(round(full * scale)))
    if name == 'poisson128':
        shape, degree, vector = [n(128)] * 3, 1, False
    elif name in ('elasticity96', 'elasticity64', 'elasticity48'):
        shape, degree, vector = [n(int(name[10:]))] * 3, 1, True
    elif name == 'bilinear2048':
        shape, degree, vector = [n(2048)] * 2, 1, False
    elif name == 'bilinear1024':
        shape, degree, vector = [n(1024)] * 2, 1, False
    elif name in ('p2vector32', 'p2vector16'):
        shape, degree, vector = [n(int(name[8:]))] * 3, 2, True
    else:
        raise SystemExit(f'unknown matrix {name!r}')
    domain, geom = mesh.rectilinear([numpy.linspace(0, 1, m + 1) for m in shape])
    nd = len(shape)
    if vector:
        u = domain.field('u', btype='std', degree=degree, shape=[nd])
        v = domain.field('v', btype='std', degree=degree, shape=[nd])
        eps = lambda w: function.symgrad(w, geom)
        res = domain.integral(function.inner(eps(v), function.div(u, geom) * function.eye(nd) + 1.3 * eps(u)) * function.J(geom), degree=2 * degree)
        K = function.derivative(function.derivative(res, 'v'), 'u')
    else:
        basis = domain.basis('std', degree=degree)
        K = domain.integral(function.outer(function.grad(basis, geom)).sum(-1) * function.J(geom), degree=2 * degree)
    nodes = [degree * m + 1 for m in shape]
    held = numpy.zeros(nodes + [nd if vector else 1], dtype=bool)
    held[0] = True  # the side x_0 = 0
    return K, held.ravel(), dict(shape=shape, degree=degree, components=nd if vector else 1)


def windows(fns, window, count=3):
    '''per function: times per call [s] of `count` windows of at least `window` seconds; the windows of the functions alternate'''
    import torch
    reps = []
    for fn in fns:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = 0
        while time.perf_counter() - t0 < .05:  # pilot
            fn()
            k += 1
            torch.cuda.synchronize()
        reps.append(max(3, int(k * window / .05 * 1.5)))
    out = [[] for _ in fns]
    for _ in range(count):
        for i, fn in enumerate(fns):
            while True:
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(reps[i]):
                    fn()
                stop.record()
                stop.synchronize()
                seconds = start.elapsed_time(stop) * 1e-3
                if seconds >= window:
                    break
                reps[i] = int(reps[i] * max(1.5, 1.2 * window / max(seconds, 1e-6)))
            out[i].append(seconds / reps[i])
    return out


def stats(times):
    med = float(numpy.median(times))
    return dict(us=med * 1e6, spread=float((max(times) - min(times)) / med))


def probe(name, args):
    import torch
    import scipy.sparse
    from nutils_amd import function, device, kernels, matrix
    K, held, info = build(name, args.scale)
    t0 = time.perf_counter()
    A = function.eval(function.as_matrix(K))
    device.synchronize()
    info['assemble_first_ms'] = (time.perf_counter() - t0) * 1e3
    values, rowptr, colidx = A.triplet()
    nrows, ncols = A.shape
    nnz = A.nnz
    lengths = (rowptr[1:] - rowptr[:-1])
    info.update(name=name, nrows=nrows, nnz=nnz, mean_row=nnz / nrows, max_row=int(lengths.max()), rule_lanes=A.lanes)
    nbytes = nnz * 12 + nrows * 16 + ncols * 8
    info['algorithmic_bytes'] = nbytes
    x = torch.from_numpy(numpy.random.default_rng(0).normal(size=ncols)).cuda()
    y = torch.empty(nrows, dtype=torch.float64, device='cuda')
    A._columns()

    # torch's CSR product
    try:
        T = torch.sparse_csr_tensor(rowptr, colidx, values, size=(nrows, ncols))
        torch_fn = lambda: T @ x
        err = float((torch_fn() - A.spmv(x)).abs().max() / A.spmv(x).abs().max())
        info['torch_vs_ours_max_rel_diff'] = err
    except Exception as e:  # not available in this build: recorded, not hidden
        torch_fn = None
        info['torch_csr'] = f'unavailable: {type(e).__name__}: {e}'

    free = ~held
    mask = device.to_dev(free, 'uint8')
    rhs = numpy.random.default_rng(2).normal(size=nrows)
    rhs_dev = device.to_dev(rhs, 'float64')
    res0 = torch.where(mask != 0, rhs_dev, torch.zeros_like(rhs_dev))
    if 'spmv' in args.sections:
        probe_spmv(A, x, y, nbytes, torch_fn, info, args)
    if 'cg' in args.sections:
        probe_cg(A, free, mask, rhs_dev, res0, info, args)
    if 'bicgstab' in args.sections:
        info['bicgstab'] = probe_bicgstab(A, free, mask, rhs_dev, res0, args)
    if 'fgmres' in args.sections:
        info['fgmres'] = probe_fgmres(A, free, mask, rhs_dev, res0, args)
    if 'minres' in args.sections:
        info['minres'] = probe_minres(A, free, mask, rhs_dev, res0, args)
    if 'amg' in args.sections:
        info['amg'] = probe_amg(A, free, mask, rhs_dev, res0, info, args)
    if 'smoother' in args.sections:
        info['smoother'] = probe_smoother(A, free, mask, rhs_dev, res0, info, args)
    if 'algebra' in args.sections:
        info['algebra'] = probe_algebra(A, free, args)
    if 'columns' in args.sections:
        info['columns'] = probe_columns(A, free, mask, args)
    if 'flexible' in args.sections:
        info['flexible'] = probe_flexible(A, free, mask, rhs_dev, res0, info, args)
    return info


def probe_spmv(A, x, y, nbytes, torch_fn, info, args):
    '''the product for every lane count, torch's, the int64 columns, and the host's'''
    import scipy.sparse
    from nutils_amd import device, kernels
    values, rowptr, colidx = A.triplet()
    nrows, ncols = A.shape
    lanes = sorted(set(LANES) | {A.lanes})
    fns = [(lambda L=L: A.spmv(x, y=y, lanes=L)) for L in lanes]
    if torch_fn:
        fns.append(torch_fn)
    res = windows(fns, args.window)
    info['spmv'] = {}
    for L, t in zip(lanes, res):
        s = stats(t)
        s.update(frac_8TBs=nbytes / (s['us'] * 1e-6) / 8e12, frac_6p3TBs=nbytes / (s['us'] * 1e-6) / 6.3e12, GBs=nbytes / (s['us'] * 1e-6) / 1e9)
        info['spmv'][str(L)] = s
    best = min(info['spmv'], key=lambda L: info['spmv'][L]['us'])
    info['best_lanes'] = int(best)
    if torch_fn:
        info['torch_csr'] = stats(res[-1])
        ours = info['spmv'][str(A.lanes)]
        info['ours_over_torch'] = ours['us'] / info['torch_csr']['us']
    # int64 columns at the rule's lane count
    fn64 = lambda: kernels.csr_spmv(values, rowptr, colidx, ncols, x, y=y, col32=None, lanes=A.lanes)
    info['spmv_int64_columns'] = stats(windows([fn64], args.window)[0])

    # what a user can do without the backend: copy the triplet, multiply with scipy
    t0 = time.perf_counter()
    hv, hrp, hci = (device.to_host(a) for a in (values, rowptr, colidx))
    info['to_host_ms'] = (time.perf_counter() - t0) * 1e3
    S = scipy.sparse.csr_matrix((hv, hci, hrp), (nrows, ncols))
    xh = x.cpu().numpy()
    S @ xh
    t0 = time.perf_counter()
    for _ in range(3):
        S @ xh
    info['scipy_matvec_ms'] = (time.perf_counter() - t0) / 3 * 1e3
    del S, hv, hrp, hci


def probe_algebra(A, free, args):
    '''T, submatrix(free, free) and sums of different patterns: first, with the plan, and on the host path'''
    import torch
    from nutils_amd import device, matrix
    values, rowptr, colidx = A.triplet()
    nrows, ncols = A.shape
    nnz = A.nnz
    idx = 4 if A._col32 is not None else 8  # bytes of a column index as the kernels read it

    def plain():  # the matrix without plans and without a host copy
        B = matrix.HipMatrix(values, rowptr, colidx, ncols)
        B._col32 = A._col32
        return B

    def wall(fn, repeats=5):
        fn()
        times = []
        for _ in range(repeats):
            device.synchronize()
            t0 = time.perf_counter()
            fn()
            device.synchronize()
            times.append(time.perf_counter() - t0)
        return dict(ms=float(numpy.median(times)) * 1e3, spread=float((max(times) - min(times)) / numpy.median(times)))

    def once(fn):
        device.synchronize()
        t0 = time.perf_counter()
        fn()
        device.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def with_bytes(entry, nbytes):
        entry.update(bytes=int(nbytes), frac_8TBs=nbytes / (entry.get('ms', entry.get('us', 0) * 1e-3) * 1e-3) / 8e12)
        return entry

    out = {}
    gather = lambda n: 24 * n  # pos, the value it points at, the value written
    # transpose: the histogram reads the columns, the placement reads them again and writes a key, the sort reads the key and writes pos and the source row
    planned = plain()
    T = planned.T
    out['T'] = dict(first=with_bytes(wall(lambda: plain().T), nnz * (2 * idx + 8 + 24) + 24 * ncols + gather(nnz)),
                    plan=with_bytes(stats(windows([lambda: planned.T], args.window)[0]), gather(nnz)),
                    host_ms=once(lambda: plain()._transpose_host()))
    # submatrix: count and fill read the columns (and the mask bytes they point at), the fill writes a column and a position per kept entry
    S = planned.submatrix(free, free)
    out['submatrix'] = dict(kept=S.nnz, first=with_bytes(wall(lambda: plain().submatrix(free, free)), nnz * 2 * idx + 32 * nrows + 16 * S.nnz + gather(S.nnz)),
                            plan=with_bytes(stats(windows([lambda: planned.submatrix(free, free)], args.window)[0]), gather(S.nnz)),
                            host_ms=once(lambda: plain()._submatrix_host(free, free)))
    # sums: the union reads both column lists twice and writes the union and both position lists; the values are zeroed, placed and added; the pruning pass
    # counts over columns and values and, where something cancelled (the stored zeros of an assembled matrix do, as on the host), fills and gathers
    from nutils_amd import kernels
    n = min(nrows, ncols)
    D = matrix.HipMatrix(torch.full((n,), .5, dtype=torch.float64, device='cuda'), torch.arange(nrows + 1, device='cuda').clamp(max=n), torch.arange(n, device='cuda'), ncols)
    for key, B in (('K+D', D), ('K+KT', T)):
        if B.shape != A.shape:
            continue
        union = kernels.pattern_union([A.triplet()[1:], B.triplet()[1:]])[1].numel()
        kept = (plain() + B).nnz
        nbytes = 2 * 8 * (nnz + B.nnz) + 8 * union + 8 * (nnz + B.nnz) + 8 * union + 24 * nnz + 32 * B.nnz + 16 * union + 32 * nrows
        if kept < union:
            nbytes += 16 * union + 16 * kept + gather(kept)
        out[key] = dict(nnz_other=B.nnz, nnz_union=union, nnz_sum=kept, first=with_bytes(wall(lambda: plain() + B), nbytes),
                        host_ms=once(lambda: plain()._add_host(matrix.HipMatrix(*B.triplet(), ncols), 1.)))
    return out


def probe_cg(A, free, mask, rhs_dev, res0, info, args):
    '''CG: time per iteration, the product's share, a solve'''
    import torch
    from nutils_amd import device, kernels, matrix
    values, rowptr, colidx = A.triplet()
    nrows, ncols = A.shape
    held = ~free
    dinv = (1. / A._diagonal_dev()).masked_fill(mask == 0, 0.)
    r = torch.from_numpy(numpy.random.default_rng(1).normal(size=nrows) * free).cuda()
    xs, p, q = torch.zeros_like(r), torch.empty_like(r), torch.empty_like(r)
    work = kernels.cg_work()
    kernels.cg_init(dinv, r, p, work)
    step = lambda: kernels.cg_iterate(values, rowptr, colidx, ncols, rowmask=mask, dinv=dinv, x=xs, r=r, p=p, q=q, work=work, niter=10, col32=A._columns(), lanes=A.lanes)
    masked = lambda: A.spmv(p, y=q, rowmask=mask)
    it, mv = windows([step, masked], args.window)
    info['cg_iteration'] = stats([t / 10 for t in it])
    info['cg_spmv_share'] = float(numpy.median(mv)) / info['cg_iteration']['us'] * 1e6
    device.synchronize()
    t0 = time.perf_counter()
    try:
        sol = A.solve(rhs_dev, constrain=held, rtol=1e-8, maxiter=args.maxiter)
        info['solve'] = dict(converged=True)
    except matrix.ToleranceNotReached as e:
        sol = e.best
        info['solve'] = dict(converged=False)
    device.synchronize()
    info['solve'].update(wall_ms=(time.perf_counter() - t0) * 1e3, iterations=A.cg_iterations)
    info['solve']['true_relative_residual'] = float(A.spmv(sol, alpha=-1., beta=1., b=rhs_dev, rowmask=mask).norm() / res0.norm())


def probe_columns(A, free, mask, args):
    '''blocks of k = 1, 2, 4, 8 vectors: the block product against k single products, a batched CG iteration against k single ones'''
    import torch
    from nutils_amd import kernels
    values, rowptr, colidx = A.triplet()
    nrows, ncols = A.shape
    nnz = A.nnz
    col32 = A._columns()
    entry = 8 + (4 if col32 is not None else 8)  # bytes of a (value, column) pair as the kernels read it
    csr = dict(rowmask=mask, col32=col32, lanes=A.lanes)
    dinv = (1. / A._diagonal_dev()).masked_fill(mask == 0, 0.)
    rng = numpy.random.default_rng(3)
    steps = 20
    out = {}
    for k in (1, 2, 4, 8):
        X = torch.from_numpy(rng.normal(size=(ncols, k))).cuda()
        Y = torch.empty((nrows, k), dtype=torch.float64, device='cuda')
        xs, y = [X[:, j].contiguous() for j in range(k)], torch.empty(nrows, dtype=torch.float64, device='cuda')
        block = lambda: A.spmm(X, Y=Y)
        singles = lambda: [A.spmv(xj, y=y) for xj in xs]
        tb, ts = windows([block, singles], args.window)
        bytes_block, bytes_singles = nnz * entry + nrows * 8 + k * (nrows + ncols) * 8, k * (nnz * entry + nrows * 16 + ncols * 8)
        spmm, spmv = stats(tb), stats(ts)
        spmm.update(bytes=bytes_block, GBs=bytes_block / spmm['us'] / 1e3)
        spmv.update(bytes=bytes_singles, GBs=bytes_singles / spmv['us'] / 1e3)
        # CG: the same residuals as a block and as k vectors
        R0 = torch.from_numpy(rng.normal(size=(nrows, k)) * free[:, None]).cuda()
        xb, R, P, Q = torch.zeros_like(R0), torch.empty_like(R0), torch.empty_like(R0), torch.empty_like(R0)
        work = kernels.cgm_work(k)

        def batched():
            R.copy_(R0)
            kernels.cgm_init(dinv, R, P, work)
            kernels.cgm_iterate(values, rowptr, colidx, ncols, dinv=dinv, x=xb, r=R, p=P, q=Q, work=work, niter=steps, **csr)

        r0s = [R0[:, j].contiguous() for j in range(k)]
        state = [(r0, torch.zeros_like(r0), torch.empty_like(r0), torch.empty_like(r0), torch.empty_like(r0), kernels.cg_work()) for r0 in r0s]

        def one_by_one():
            for r0, x, r, p, q, w in state:
                r.copy_(r0)
                kernels.cg_init(dinv, r, p, w)
                kernels.cg_iterate(values, rowptr, colidx, ncols, dinv=dinv, x=x, r=r, p=p, q=q, work=w, niter=steps, **csr)

        cb, cs = windows([batched, one_by_one], args.window)
        cgm, cg = stats([t / steps for t in cb]), stats([t / steps for t in cs])
        out[str(k)] = dict(spmm=spmm, k_spmv=spmv, spmv_over_spmm=spmv['us'] / spmm['us'], bytes_ratio=bytes_singles / bytes_block,
                           cgm_iteration=cgm, k_cg_iterations=cg, cg_over_cgm=cg['us'] / cgm['us'])
        del X, Y, xs, R0, xb, R, P, Q, state, r0s
    return out


def nodes_of(info):
    '''the coordinates of the nodes of `build`'s mesh, in the order of its dofs'''
    grids = [numpy.linspace(0, 1, info['degree'] * m + 1) for m in info['shape']]
    return numpy.stack(numpy.meshgrid(*grids, indexing='ij'), -1).reshape(-1, len(grids))


def probe_amg(A, free, mask, rhs_dev, res0, info, args):
    '''precon='amg': the symbolic and the numeric phase of the setup (wall clock, synchronised; the numeric one a first and a second time), one cycle
    against one masked product, and AMG-CG and Jacobi-CG solves of the same system in the same process; for a vector matrix the setup and the solve once
    more with the rigid-body modes as the near-nullspace (on the device beforehand: the solve times hold no upload)'''
    import torch
    from nutils_amd import amg, device, kernels, matrix
    values, rowptr, colidx = A.triplet()
    out = {}

    def clocked(fn):
        device.synchronize()
        t0 = time.perf_counter()
        result = fn()
        device.synchronize()
        return result, (time.perf_counter() - t0) * 1e3

    try:
        levels, out['symbolic_ms'] = clocked(lambda: amg.symbolic(rowptr, colidx, mask != 0, 256))
    except (matrix.MatrixError, RuntimeError) as e:  # (a product beyond the int32 indices of its plan, or out of memory: recorded, not hidden)
        return dict(error=f'{type(e).__name__}: {e}')
    h, out['numeric_first_ms'] = clocked(lambda: amg.Hierarchy(levels, values))
    h, out['numeric_ms'] = clocked(lambda: amg.Hierarchy(levels, values))
    out['levels'] = [lv.nfree for lv in levels]
    out['kinds'] = [lv.kind for lv in levels]
    nnzs = [lv.colidx.numel() for lv in levels]
    out['operator_complexity'] = sum(nnzs) / nnzs[0]
    r = torch.where(mask != 0, torch.from_numpy(numpy.random.default_rng(1).normal(size=A.shape[0])).cuda(), torch.zeros_like(rhs_dev))
    z = torch.empty_like(r)
    masked = lambda: A.spmv(r, y=z, rowmask=mask)
    t_cycle, t_mv = windows([lambda: h.apply(r, z), masked], args.window)
    out['cycle'] = stats(t_cycle)
    out['masked_spmv'] = stats(t_mv)
    out['cycle_over_product'] = out['cycle']['us'] / out['masked_spmv']['us']
    out['launches_per_cycle'] = 5 * (len(levels) - 1) + 1
    del h, levels
    preconargs = {'amg': None, 'diag': None}
    if info['components'] > 1:
        B = device.to_dev(amg.rigid_body_modes(nodes_of(info)), 'float64')
        out['rigid_body_modes'] = dict(k=B.shape[1])
        # --amg-setup entry,block: the setup once per kind of plan, side by side in this process; without it the default kind, as before
        for setup in args.amg_setup or [None]:
            rbm = out['rigid_body_modes'] if setup is None else out['rigid_body_modes'].setdefault(setup, {})
            try:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                levels, rbm['symbolic_ms'] = clocked(lambda: amg.symbolic(rowptr, colidx, mask != 0, 256, B.shape[1], setup=setup))
                rbm['symbolic_peak_bytes'] = torch.cuda.max_memory_allocated() - before  # (torch's allocator statistic: what the phase held at its peak, above what was there)
                rbm['symbolic_kept_bytes'] = torch.cuda.memory_allocated() - before
                rbm['setup'] = levels[0].setup
                rbm['products_level0'] = {what: getattr(levels[0], what).nprod for what in ('at', 'ap', 'rap')} if levels[0].kind == 'coarsen' else None
                rbm['products'] = [[getattr(lv, what).nprod for what in ('at', 'ap', 'rap')] for lv in levels if lv.kind == 'coarsen']
                h, rbm['numeric_first_ms'] = clocked(lambda: amg.Hierarchy(levels, values, 1, B))
                h, rbm['numeric_ms'] = clocked(lambda: amg.Hierarchy(levels, values, 1, B))
                rbm['levels'] = [lv.nfree for lv in levels]
                rbm['kinds'] = [lv.kind for lv in levels]
                rbm['operator_complexity'] = sum(lv.colidx.numel() for lv in levels) / nnzs[0]
                rbm['dropped_columns'] = [int((d.dinv == 0).sum()) for lv, d in zip(levels[1:], h.data[1:])]
                t_cycle, = windows([lambda: h.apply(r, z)], args.window)
                rbm['cycle'] = stats(t_cycle)
                rbm['cycle_over_product'] = rbm['cycle']['us'] / out['masked_spmv']['us']
                del h, levels
                preconargs['amg_rbm' if setup is None else 'amg_rbm_' + setup] = dict(nullspace=B) if setup is None else dict(nullspace=B, setup=setup)
            except (matrix.MatrixError, RuntimeError) as e:  # (as above: recorded, not hidden)
                rbm['error'] = f'{type(e).__name__}: {e}'
                levels = h = None  # (what the failed phase held goes back to the allocator before the next kind starts)

    def solve(name):
        try:
            return A.solve(rhs_dev, constrain=~free, rtol=1e-8, maxiter=args.maxiter, precon=name.split('_')[0], preconargs=preconargs[name]), True
        except matrix.ToleranceNotReached as e:
            return e.best, False

    runs, cached = {}, {}
    for name in preconargs:  # the first solve of an 'amg' kind runs its symbolic phase; the matrix caches one, so each kind is handed its own back below
        A._amg = None
        runs[name] = [clocked(lambda: solve(name))]
        cached[name] = A._amg
    for _ in range(3):  # (alternating)
        for precon in runs:
            A._amg = cached[precon]
            runs[precon].append(clocked(lambda: solve(precon)))
    for precon, timed in runs.items():
        (sol, converged), first = timed[0]
        res = dict(converged=converged, first_ms=first, wall_ms=float(numpy.median([ms for _, ms in timed[1:]])), spread=(max(ms for _, ms in timed[1:]) - min(ms for _, ms in timed[1:])))
        A._amg = cached[precon]
        solve(precon)
        res['iterations'] = A.iterations
        res['true_relative_residual'] = float(A.spmv(sol, alpha=-1., beta=1., b=rhs_dev, rowmask=mask).norm() / res0.norm())
        out['solve_' + precon] = res
    return out


def probe_smoother(A, free, mask, rhs_dev, res0, info, args):
    '''the smoothers of precon='amg' side by side on one hierarchy: per configuration the numeric setup (wall clock, synchronised, the median of three after
    a first), for Chebyshev the part of it that is nh_csr_lanczos (HIP events around the calls of a setup's worth of levels) and the bounds, one cycle, and the
    solve (the symbolic phase cached; the median of three, the configurations alternating)'''
    import torch
    from nutils_amd import amg, device, kernels, matrix
    values, rowptr, colidx = A.triplet()
    B = device.to_dev(amg.rigid_body_modes(nodes_of(info)), 'float64') if info['components'] > 1 else None
    base = {} if B is None else dict(nullspace=B)
    cheb = lambda **kwargs: dict(base, smoother='chebyshev', **kwargs)
    configs = {'jacobi1': dict(base), 'jacobi2': dict(base, sweeps=2), 'chebyshev2': cheb(degree=2), 'chebyshev3': cheb(degree=3)}
    for ratio in args.eigratios:
        configs[f'chebyshev2_ratio{ratio:g}'] = cheb(degree=2, eigratio=ratio)
    for steps in args.eigsteps:
        configs[f'chebyshev2_steps{steps}'] = cheb(degree=2, eigsteps=steps)

    def clocked(fn):
        device.synchronize()
        t0 = time.perf_counter()
        result = fn()
        device.synchronize()
        return result, (time.perf_counter() - t0) * 1e3

    try:
        levels = amg.symbolic(rowptr, colidx, mask != 0, 256, None if B is None else B.shape[1])
    except (matrix.MatrixError, RuntimeError) as e:  # (recorded, not hidden)
        return dict(error=f'{type(e).__name__}: {e}')
    out = dict(levels=[lv.nfree for lv in levels], kinds=[lv.kind for lv in levels])
    r = torch.where(mask != 0, torch.from_numpy(numpy.random.default_rng(1).normal(size=A.shape[0])).cuda(), torch.zeros_like(rhs_dev))
    z = torch.empty_like(r)
    for name, preconargs in configs.items():
        rest, smoother = amg.split_smoother(preconargs)
        sweeps = amg.check_args(rest, A.shape[0])[1]
        make = lambda: amg.Hierarchy(levels, values, sweeps, B, smoother)
        h, first = clocked(make)
        res = out[name] = dict(numeric_first_ms=first, numeric_ms=float(numpy.median([clocked(make)[1] for _ in range(3)])))
        if smoother is not None:
            res.update(theta=[d.theta for d in h.data[:-1]], rho=[float(d.rho) for d in h.data[:-1]], ub=[d.ub for d in h.data[:-1]], eigsteps_taken=[d.eigsteps for d in h.data[:-1]])
            coarsened = [(lv, d, d.dinv.sqrt(), amg.start_vector(lv.n, values.device)) for lv, d in zip(levels[:-1], h.data[:-1])]
            estimate = lambda: [kernels.csr_lanczos(d.values, lv.rowptr, lv.colidx, lv.n, s, u, smoother['eigsteps'], rowmask=lv.mask, col32=lv.col32) for lv, d, s, u in coarsened]
            res['lanczos_ms'] = stats(windows([estimate], args.window)[0])['us'] * 1e-3
        res['cycle'] = stats(windows([lambda: h.apply(r, z)], args.window)[0])
        del h

    def solve(name):
        try:
            return A.solve(rhs_dev, constrain=~free, rtol=1e-8, maxiter=args.maxiter, precon='amg', preconargs=configs[name]), True
        except matrix.ToleranceNotReached as e:
            return e.best, False

    A._amg = None
    runs = {name: [clocked(lambda: solve(name))] for name in configs}  # (the first of them runs the symbolic phase, which the matrix then keeps)
    for _ in range(3):  # (alternating)
        for name in configs:
            runs[name].append(clocked(lambda: solve(name)))
    for name, timed in runs.items():
        (sol, converged), _ = timed[0]
        solve(name)
        ms = [t for _, t in timed[1:]]
        out[name]['solve'] = dict(converged=converged, iterations=A.iterations, wall_ms=float(numpy.median(ms)), spread=max(ms) - min(ms),
                                  true_relative_residual=float(A.spmv(sol, alpha=-1., beta=1., b=rhs_dev, rowmask=mask).norm() / res0.norm()))
    return out


BICGSTAB_STEPS = 20


def nonsymmetric_twin(A):
    '''N = K + 0.5 (triu(K, 1) - tril(K, -1)) on the index tensors of A (set-up, not timed)'''
    import torch
    values, rowptr, colidx = A.triplet()
    rows = torch.repeat_interleave(torch.arange(A.shape[0], device=values.device), rowptr[1:] - rowptr[:-1])
    return A._with_values(values * (1 + .5 * torch.sign(colidx - rows)))


def probe_bicgstab(A, free, mask, rhs_dev, res0, args):
    '''the nonsymmetric twin of A: iteration time, a solve, the host route'''
    import torch
    import scipy.sparse
    import scipy.sparse.linalg
    from nutils_amd import device, kernels, matrix
    values, rowptr, colidx = A.triplet()
    nrows, ncols = A.shape
    N = nonsymmetric_twin(A)
    nvalues = N.triplet()[0]
    out = {}
    dinv = (1. / N._diagonal_dev()).masked_fill(mask == 0, 0.)
    r0 = torch.from_numpy(numpy.random.default_rng(1).normal(size=nrows) * free).cuda()
    x, r, rhat, p, v, s, t, phat, shat = (torch.zeros_like(r0) for _ in range(9))
    work = kernels.bicgstab_work()

    def start():  # the same state before every timed call: the iteration must neither converge nor break down inside a window
        x.zero_()
        r.copy_(r0)
        kernels.bicgstab_init(dinv, r, rhat, p, phat, work)

    def steps():
        start()
        kernels.bicgstab_iterate(nvalues, rowptr, colidx, ncols, rowmask=mask, dinv=dinv, x=x, r=r, rhat=rhat, p=p, v=v, s=s, t=t, phat=phat, shat=shat, work=work, stop_rr=0.,
                                 niter=BICGSTAB_STEPS, col32=A._columns(), lanes=A.lanes)

    masked = lambda: N.spmv(phat, y=v, rowmask=mask)
    t_steps, t_start, t_mv = windows([steps, start, masked], args.window)
    steps()
    rr, flag, moved = work[:3].tolist()
    out['moved_per_call'], out['flag'] = moved, flag  # (BICGSTAB_STEPS and 0, or the time below is not that of an iteration)
    per_iteration = [(a - b) / BICGSTAB_STEPS for a, b in zip(t_steps, t_start)]
    out['iteration'] = stats(per_iteration)
    out['masked_spmv'] = stats(t_mv)
    out['iteration_over_two_products'] = out['iteration']['us'] / (2 * out['masked_spmv']['us'])
    # vector passes of 8 n bytes: half r, v, dinv -> s, shat (5); update x, phat, shat, s, t, rhat -> x, r (8); direction r, p, v, dinv -> p, phat (6)
    out['vector_passes'] = 19
    vector_us = out['iteration']['us'] - 2 * out['masked_spmv']['us']
    out['vector_part_us'] = vector_us
    out['vector_part_frac_6p3TBs'] = 19 * 8 * nrows / (vector_us * 1e-6) / 6.3e12 if vector_us > 0 else None
    del x, r, rhat, p, v, s, t, phat, shat

    device.synchronize()
    t0 = time.perf_counter()
    try:
        sol = N.solve(rhs_dev, constrain=~free, solver='bicgstab', rtol=1e-8, maxiter=args.maxiter)
        out['solve'] = dict(converged=True)
    except matrix.ToleranceNotReached as e:
        sol = e.best
        out['solve'] = dict(converged=False)
    device.synchronize()
    out['solve'].update(wall_ms=(time.perf_counter() - t0) * 1e3, iterations=N.iterations)
    out['solve']['true_relative_residual'] = float(N.spmv(sol, alpha=-1., beta=1., b=rhs_dev, rowmask=mask).norm() / res0.norm())
    del sol
    if args.no_host_solve:
        return out

    # the route a user has without the device solver
    t0 = time.perf_counter()
    hv, hrp, hci = (device.to_host(a) for a in (nvalues, rowptr, colidx))
    out['host'] = dict(to_host_ms=(time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    S = scipy.sparse.csr_matrix((hv, hci, hrp), (nrows, ncols))
    keep, = free.nonzero()
    F = S[keep][:, keep]
    b = rhs_dev.cpu().numpy()[keep]  # (the constrained values are zero: no lift)
    d = 1. / F.diagonal()
    jacobi = scipy.sparse.linalg.LinearOperator(F.shape, matvec=lambda y: d * y)
    out['host']['submatrix_ms'] = (time.perf_counter() - t0) * 1e3
    count = [0]
    t0 = time.perf_counter()
    try:
        y, code = scipy.sparse.linalg.bicgstab(F, b, rtol=1e-8, atol=0., maxiter=args.maxiter, M=jacobi, callback=lambda _: count.__setitem__(0, count[0] + 1))
    except TypeError:  # scipy before 1.12 calls the relative tolerance `tol`
        y, code = scipy.sparse.linalg.bicgstab(F, b, tol=1e-8, atol=0., maxiter=args.maxiter, M=jacobi, callback=lambda _: count.__setitem__(0, count[0] + 1))
    out['host'].update(bicgstab_ms=(time.perf_counter() - t0) * 1e3, iterations=count[0], converged=code == 0,
                       true_relative_residual=float(numpy.linalg.norm(b - F @ y) / numpy.linalg.norm(b)))
    return out


FLEX_RESTARTS = (10, 30)


def probe_flexible(A, free, mask, rhs_dev, res0, info, args):
    '''the nonsymmetric twin of A under flexible GMRES with the AMG cycle as its preconditioner (an object of `getprecon`, symmetric=False; the rigid-body modes
    for a vector matrix): setup, the time of a step against a Jacobi-GMRES step and a cycle of the same run, and the solve against Jacobi-GMRES and
    Jacobi-BiCGStab in the same process, alternating; what a reused object saves; a solve with the object of the matrix before a perturbation of the values'''
    import torch
    from nutils_amd import amg, device, kernels, matrix
    _, rowptr, colidx = A.triplet()
    nrows, ncols = A.shape
    N = nonsymmetric_twin(A)
    nvalues = N.triplet()[0]
    out = {}

    def clocked(fn):
        device.synchronize()
        t0 = time.perf_counter()
        result = fn()
        device.synchronize()
        return result, (time.perf_counter() - t0) * 1e3

    pargs = dict(constrain=~free, symmetric=False)
    if info['components'] > 1:
        pargs['nullspace'] = device.to_dev(amg.rigid_body_modes(nodes_of(info)), 'float64')
    try:
        M, out['getprecon_first_ms'] = clocked(lambda: N.getprecon('amg', **pargs))  # (with the symbolic phase)
        M, out['getprecon_ms'] = clocked(lambda: N.getprecon('amg', **pargs))  # (the numeric setup: what a reused object saves a solve)
    except (matrix.MatrixError, RuntimeError) as e:  # (a plan beyond its int32 indices, or out of memory: recorded, not hidden)
        return dict(error=f'{type(e).__name__}: {e}')
    out['levels'] = [lv.nfree for lv in M.hierarchy.levels]
    dinv = (1. / N._diagonal_dev()).masked_fill(mask == 0, 0.)
    r0 = torch.from_numpy(numpy.random.default_rng(1).normal(size=nrows) * free).cuda()
    z, t, w = torch.zeros_like(r0), torch.zeros_like(r0), torch.zeros_like(r0)
    csr = dict(rowmask=mask, col32=A._columns(), lanes=A.lanes)

    def timed_solve(**kwargs):
        def run():
            try:
                return N.solve(rhs_dev, constrain=~free, rtol=1e-8, maxiter=args.maxiter, **kwargs), True
            except matrix.ToleranceNotReached as e:
                return e.best, False
        runs = [clocked(run) for _ in range(3)]
        (sol, converged), _ = runs[0]
        times = [ms for _, ms in runs]
        return dict(converged=converged, wall_ms=float(numpy.median(times)), spread=(max(times) - min(times)) / float(numpy.median(times)), iterations=N.iterations,
                    true_relative_residual=float(N.spmv(sol, alpha=-1., beta=1., b=rhs_dev, rowmask=mask).norm() / res0.norm()))

    for m in FLEX_RESTARTS:
        V, Z = (torch.zeros(k * nrows, dtype=torch.float64, device='cuda') for k in (m + 1, m))
        work = kernels.gmres_work(m)
        start_j, start_f = (lambda: kernels.gmres_init(dinv, r0, V, z, work, restart=m)), (lambda: kernels.gmres_init(None, r0, V, z, work, restart=m))

        def jacobi():  # a whole cycle from the same residual, none of its steps stopped (the bound is zero)
            start_j()
            kernels.gmres_iterate(nvalues, rowptr, colidx, ncols, dinv=dinv, V=V, z=z, w=w, work=work, restart=m, stop_rr=0., niter=m, **csr)

        def flexible():
            start_f()
            kernels.fgmres_iterate(nvalues, rowptr, colidx, ncols, amg=M.hierarchy.handle, V=V, Z=Z, z=z, t=t, w=w, work=work, restart=m, stop_rr=0., niter=m, **csr)

        t_flex, t_jac, t_sf, t_sj, t_cycle = windows([flexible, jacobi, start_f, start_j, lambda: M.hierarchy.apply(z, t)], args.window)
        flexible()
        res = dict(steps_per_call=work[:3].tolist()[2], basis_vectors=2 * m + 1, basis_bytes=(2 * m + 1) * 8 * nrows)
        res['step'] = stats([(a - b) / m for a, b in zip(t_flex, t_sf)])
        res['jacobi_step'] = stats([(a - b) / m for a, b in zip(t_jac, t_sj)])
        res['cycle'] = stats(t_cycle)
        res['cycle_share'] = res['cycle']['us'] / res['step']['us']
        res['step_over_jacobi_step'] = res['step']['us'] / res['jacobi_step']['us']
        del V, Z, work
        res['solve'] = timed_solve(solver='fgmres', precon=M, restart=m)
        res['solve_jacobi'] = timed_solve(solver='fgmres', precon='diag', restart=m)
        res['solve_over_jacobi'] = res['solve']['wall_ms'] / res['solve_jacobi']['wall_ms']
        torch.cuda.empty_cache()
        out[str(m)] = res
    out['solve_bicgstab'] = timed_solve(solver='bicgstab', precon='diag')
    # lagged: the object of N on the matrix one perturbation of the values further (every entry scaled by a factor within 10 % of one; the diagonal kept, so
    # the matrix stays as dominant as it was), against that matrix's own object
    scale = 1 + .1 * torch.from_numpy(numpy.random.default_rng(3).uniform(-1, 1, nvalues.numel())).cuda()
    rows = torch.repeat_interleave(torch.arange(nrows, device=nvalues.device), rowptr[1:] - rowptr[:-1])
    N2 = N._with_values(torch.where(rows == colidx, nvalues, nvalues * scale))

    def lagged(precon):
        device.synchronize()
        t0 = time.perf_counter()
        try:
            sol, converged = N2.solve(rhs_dev, constrain=~free, solver='fgmres', precon=precon, restart=30, rtol=1e-8, maxiter=args.maxiter), True
        except matrix.ToleranceNotReached as e:
            sol, converged = e.best, False
        device.synchronize()
        return dict(converged=converged, wall_ms=(time.perf_counter() - t0) * 1e3, iterations=N2.iterations,
                    true_relative_residual=float(N2.spmv(sol, alpha=-1., beta=1., b=rhs_dev, rowmask=mask).norm() / res0.norm()))

    own, out['lagged_own_setup_ms'] = clocked(lambda: N2.getprecon('amg', **pargs))
    out['lagged'] = dict(own=lagged(own), lagged=lagged(M))
    return out


RESTARTS = (10, 30, 100)


def probe_fgmres(A, free, mask, rhs_dev, res0, args):
    '''the nonsymmetric twin of A under restarted GMRES: the time of an Arnoldi step and where it goes, and a solve, per restart'''
    import torch
    from nutils_amd import device, kernels, matrix
    _, rowptr, colidx = A.triplet()
    nrows, ncols = A.shape
    N = nonsymmetric_twin(A)
    nvalues = N.triplet()[0]
    dinv = (1. / N._diagonal_dev()).masked_fill(mask == 0, 0.)
    r0 = torch.from_numpy(numpy.random.default_rng(1).normal(size=nrows) * free).cuda()
    z, w = torch.zeros_like(r0), torch.zeros_like(r0)
    out = {}
    for m in RESTARTS:
        V = torch.zeros((m + 1) * nrows, dtype=torch.float64, device='cuda')
        work = kernels.gmres_work(m)
        start = lambda: kernels.gmres_init(dinv, r0, V, z, work, restart=m)

        def cycle():  # a whole cycle from the same residual: step j = 0 .. m - 1, none of them stopped (the bound is zero)
            start()
            kernels.gmres_iterate(nvalues, rowptr, colidx, ncols, rowmask=mask, dinv=dinv, V=V, z=z, w=w, work=work, restart=m, stop_rr=0., niter=m, col32=A._columns(),
                                  lanes=A.lanes)

        masked = lambda: N.spmv(z, y=w, rowmask=mask)
        t_cycle, t_start, t_mv = windows([cycle, start, masked], args.window)
        cycle()
        est, flag, count = work[:3].tolist()
        res = dict(steps_per_call=count, flag=flag)  # (m and 0, or the time below is not that of a step)
        res['step'] = stats([(a - b) / m for a, b in zip(t_cycle, t_start)])
        res['masked_spmv'] = stats(t_mv)
        res['spmv_share'] = res['masked_spmv']['us'] / res['step']['us']
        rest_us = res['step']['us'] - res['masked_spmv']['us']
        res['rest_share'] = rest_us / res['step']['us']  # the Gram-Schmidt kernels, with the scalar kernel, the normalisation and the gaps between nine launches
        passes = [4 * (j + 1) + 2 * -(-(j + 1) // kernels.GMRES_CHUNK) + 8 for j in range(m)]
        res['model_passes_per_step'] = sum(passes) / m
        res['rest_frac_8TBs'] = sum(passes) / m * 8 * nrows / (rest_us * 1e-6) / 8e12 if rest_us > 0 else None
        del V, work
        device.synchronize()
        t0 = time.perf_counter()
        try:
            sol = N.solve(rhs_dev, constrain=~free, solver='fgmres', restart=m, rtol=1e-8, maxiter=args.maxiter)
            res['solve'] = dict(converged=True)
        except matrix.ToleranceNotReached as e:
            sol = e.best
            res['solve'] = dict(converged=False)
        device.synchronize()
        res['solve'].update(wall_ms=(time.perf_counter() - t0) * 1e3, iterations=N.iterations)
        res['solve']['true_relative_residual'] = float(N.spmv(sol, alpha=-1., beta=1., b=rhs_dev, rowmask=mask).norm() / res0.norm())
        res['solve']['ms_per_step'] = res['solve']['wall_ms'] / max(1, N.iterations)
        del sol
        torch.cuda.empty_cache()
        out[str(m)] = res
    return out


def indefinite_twin(A):
    '''S: the off-diagonal entries of K, the diagonal +-sum_j |K_ij|, + on even rows and - on odd ones, on the index tensors of A (set-up, not timed).  Symmetric,
    and by Gershgorin every eigenvalue is at least K_ii from zero, on the side of its row's sign.'''
    import torch
    values, rowptr, colidx = A.triplet()
    n = A.shape[0]
    rows = torch.repeat_interleave(torch.arange(n, device=values.device), rowptr[1:] - rowptr[:-1])
    rowabs = torch.zeros(n, dtype=values.dtype, device=values.device).index_add_(0, rows, values.abs())
    sign = 1. - 2. * (torch.arange(n, device=values.device) % 2)
    return A._with_values(torch.where(colidx == rows, (sign * rowabs)[rows], values))


def shifted_twin(A, sigma):
    '''K - sigma diag(K) on the index tensors of A (set-up, not timed): the spectrum of the Jacobi-scaled matrix moved down by sigma, so that its low end is
    negative and the rest is not, as in a Helmholtz problem; the diagonal keeps its sign, and Jacobi is the same preconditioner for every solver'''
    import torch
    values, rowptr, colidx = A.triplet()
    rows = torch.repeat_interleave(torch.arange(A.shape[0], device=values.device), rowptr[1:] - rowptr[:-1])
    return A._with_values(torch.where(colidx == rows, (1. - sigma) * values, values))


MINRES_STEPS = 20
SHIFT = .01


def probe_minres(A, free, mask, rhs_dev, res0, args):
    '''the symmetric indefinite twin of A: the time of a MINRES iteration beside a BiCGStab iteration and a GMRES(30) step, and a solve by each'''
    import torch
    from nutils_amd import device, kernels, matrix
    _, rowptr, colidx = A.triplet()
    nrows, ncols = A.shape
    S = indefinite_twin(A)
    svalues = S.triplet()[0]
    csr = dict(rowmask=mask, col32=A._columns(), lanes=A.lanes)
    dinv = (1. / S._diagonal_dev()).masked_fill(mask == 0, 0.)
    dabs = dinv.abs()
    r0 = torch.from_numpy(numpy.random.default_rng(1).normal(size=nrows) * free).cuda()
    m = 30
    vec = {name: torch.zeros_like(r0) for name in ('x', 'r', 'r1', 'r2', 'v', 'q', 'w1', 'w2', 'rhat', 'p', 's', 't', 'phat', 'shat', 'z', 'w')}
    V = torch.zeros((m + 1) * nrows, dtype=torch.float64, device='cuda')
    mwork, bwork, gwork = kernels.minres_work(), kernels.bicgstab_work(), kernels.gmres_work(m)

    # the same state before every timed call: no iteration may converge or break down inside a window (the bound is zero)
    def minres_start():
        vec['x'].zero_()
        vec['r'].copy_(r0)
        kernels.minres_init(dabs, *(vec[name] for name in ('r', 'r1', 'r2', 'v', 'w1', 'w2')), mwork)

    def minres_steps():
        minres_start()
        kernels.minres_iterate(svalues, rowptr, colidx, ncols, dinv=dabs, work=mwork, stop_rr=0., niter=MINRES_STEPS, **csr,
                               **{name: vec[name] for name in ('x', 'r', 'r1', 'r2', 'v', 'q', 'w1', 'w2')})

    def bicgstab_start():
        vec['x'].zero_()
        vec['r'].copy_(r0)
        kernels.bicgstab_init(dinv, vec['r'], vec['rhat'], vec['p'], vec['phat'], bwork)

    def bicgstab_steps():
        bicgstab_start()
        kernels.bicgstab_iterate(svalues, rowptr, colidx, ncols, dinv=dinv, work=bwork, stop_rr=0., niter=MINRES_STEPS, **csr,
                                 **{name: vec[name] for name in ('x', 'r', 'rhat', 'p', 's', 't', 'phat', 'shat')}, v=vec['v'])

    gmres_start = lambda: kernels.gmres_init(dinv, r0, V, vec['z'], gwork, restart=m)

    def gmres_cycle():
        gmres_start()
        kernels.gmres_iterate(svalues, rowptr, colidx, ncols, dinv=dinv, V=V, z=vec['z'], w=vec['w'], work=gwork, restart=m, stop_rr=0., niter=m, **csr)

    masked = lambda: S.spmv(vec['v'], y=vec['q'], rowmask=mask)
    t = windows([minres_steps, minres_start, bicgstab_steps, bicgstab_start, gmres_cycle, gmres_start, masked], args.window)
    out = dict(masked_spmv=stats(t[6]))
    for name, steps, work, t_steps, t_start, n in (('minres', minres_steps, mwork, t[0], t[1], MINRES_STEPS), ('bicgstab', bicgstab_steps, bwork, t[2], t[3], MINRES_STEPS),
                                                   ('fgmres30', gmres_cycle, gwork, t[4], t[5], m)):
        steps()
        _, flag, moved = work[:3].tolist()
        out[name] = dict(moved_per_call=moved, flag=flag, iteration=stats([(a - b) / n for a, b in zip(t_steps, t_start)]))  # (n and 0, or the time is not that of an iteration)
        out[name]['iteration_over_product'] = out[name]['iteration']['us'] / out['masked_spmv']['us']
    # vector passes of 8 n bytes: lanczos q, r1, r2, dinv -> r1, r2 (6); update v, w1, w2, x, r, r2, dinv -> w1, w2, x, r, v (12)
    out['minres']['vector_passes'] = 18
    vector_us = out['minres']['iteration']['us'] - out['masked_spmv']['us']
    out['minres']['vector_part_us'] = vector_us
    out['minres']['vector_part_frac_6p3TBs'] = 18 * 8 * nrows / (vector_us * 1e-6) / 6.3e12 if vector_us > 0 else None
    del vec, V
    torch.cuda.empty_cache()

    def solves(T, repeats):
        '''a solve to rtol = 1e-8 by each of the three; the last of `repeats` is the timed one'''
        results = {}
        for name, kwargs in (('minres', dict(solver='minres')), ('bicgstab', dict(solver='bicgstab')), ('fgmres30', dict(solver='fgmres', restart=m))):
            for _ in range(repeats):
                device.synchronize()
                t0 = time.perf_counter()
                try:
                    sol = T.solve(rhs_dev, constrain=~free, rtol=1e-8, maxiter=args.maxiter, **kwargs)
                    res = dict(converged=True)
                except matrix.ToleranceNotReached as e:
                    sol = e.best
                    res = dict(converged=False)
                device.synchronize()
                res.update(wall_ms=(time.perf_counter() - t0) * 1e3, iterations=T.iterations)
            res['true_relative_residual'] = float(T.spmv(sol, alpha=-1., beta=1., b=rhs_dev, rowmask=mask).norm() / res0.norm())
            res['ms_per_iteration'] = res['wall_ms'] / max(1, T.iterations)
            results[name] = res
            del sol
        return results

    for name, res in solves(S, 2).items():  # (the first solve warms every shape)
        out[name]['solve'] = res
    # the Helmholtz-like twin: the pattern and the kernels of S, so the iteration times above are its own; every shape is warm by now
    out['shifted'] = dict(sigma=SHIFT, **solves(shifted_twin(A, SHIFT), 1))
    return out


def probe_saddle(ne, args):
    import torch
    from nutils_amd import device, function, matrix, mesh
    from nutils_amd.solver import System
    domain, geom = mesh.unitsquare(ne, 'square')
    u, v = (domain.field(name, btype='std', degree=2, shape=(2,)) for name in 'uv')
    p, q = (domain.field(name, btype='std', degree=1) for name in 'pq')
    grad = lambda w: function.grad(w, geom)
    res = domain.integral(((grad(v) * grad(u)).sum(-1).sum(-1) - function.div(v, geom) * p - q * function.div(u, geom)) * function.J(geom), degree=4)
    nn = 2 * ne + 1
    ucons = numpy.full((nn, nn, 2), numpy.nan)
    ucons[0] = ucons[-1] = ucons[:, 0] = ucons[:, -1] = 0.
    ucons[1:-1, -1, 0] = 1.  # the lid
    pcons = numpy.full((ne + 1) ** 2, numpy.nan)
    pcons[0] = 0.
    with matrix.backend('hip'):
        system = System(res, trial='u,p', test='v,q')
        t0 = time.perf_counter()
        A = system.assemble_jacobian({})
        device.synchronize()
        assemble_ms = (time.perf_counter() - t0) * 1e3
    start, free = system._pack({}, {'u': ucons.reshape(-1, 2), 'p': pcons})
    cons = numpy.where(free, numpy.nan, start)
    second = system.trialmask('p')
    n = system.size
    out = dict(name=f'stokes{ne}', elements=ne, nrows=n, nnz=A.nnz, velocity_dofs=int((~second).sum()), pressure_dofs=int(second.sum()), free=int(free.sum()),
               rule_lanes=A.lanes, assemble_first_ms=assemble_ms)
    B = numpy.zeros((n, 2))
    B[~second] = numpy.tile(numpy.eye(2), (nn * nn, 1))
    first = dict(nullspace=device.to_dev(B, 'float64'))
    mask = device.to_dev(free, 'uint8')
    start_dev = device.to_dev(start, 'float64')

    def setup(K):
        device.synchronize()
        t0 = time.perf_counter()
        M = K.getprecon('schur', constrain=cons, second=second, first=first)
        device.synchronize()
        return M, (time.perf_counter() - t0) * 1e3
    M, first_ms = setup(A)
    again = A._with_values(A.triplet()[0].clone())
    _, cached_ms = setup(again)
    levels = M.hierarchy.levels
    out['setup'] = dict(first_ms=first_ms, cached_symbolic_ms=cached_ms, levels=[lv.nfree for lv in levels],
                        operator_complexity=sum(lv.colidx.numel() for lv in levels) / A.nnz)
    r = device.to_dev(numpy.random.default_rng(3).normal(size=n), 'float64')
    y, z = torch.empty_like(r), torch.empty_like(r)
    apply_t, product_t = windows([lambda: M.schur.apply(r, z), lambda: A.spmv(r, y=y)], args.window)
    out['application'] = dict(apply=stats(apply_t), product=stats(product_t), products_per_application=float(numpy.median(apply_t) / numpy.median(product_t)))

    def solve(K, **kwargs):
        r0 = float(K.spmv(start_dev, alpha=-1., rowmask=mask).norm())
        times, reached = [], True
        for _ in range(3):
            device.synchronize()
            t0 = time.perf_counter()
            try:
                x = K.solve(None, constrain=cons, rtol=1e-8, maxiter=args.maxiter, **kwargs)
            except matrix.ToleranceNotReached as e:
                x, reached = e.best, False
            device.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            if not reached:  # (a solve that runs into the cap is timed once)
                break
        res = float(K.spmv(device.to_dev(x, 'float64'), alpha=-1., rowmask=mask).norm()) / r0
        return dict(iterations=K.iterations, reached=reached, wall_ms=float(numpy.median(times)), true_residual=res)
    out['schur_fgmres30'] = solve(A, solver='fgmres', precon=M, restart=30)
    out['schur_fgmres100'] = solve(A, solver='fgmres', precon=M, restart=100)
    # the other Schur diagonal: minus the diagonal of the pressure mass matrix (viscosity 1) instead of the SIMPLE choice
    pbasis = domain.basis('std', degree=1)
    shat = numpy.zeros(n)
    shat[second] = -function.eval(function.as_matrix(domain.integral(function.outer(pbasis) * function.J(geom), degree=2))).diagonal()
    mass = A.getprecon('schur', constrain=cons, second=second, first=first, schur=shat)
    out['schur_mass_fgmres30'] = solve(A, solver='fgmres', precon=mass, restart=30)
    for solver in ('bicgstab', 'fgmres', 'minres'):
        out[('gmres30' if solver == 'fgmres' else solver) + '_none'] = solve(A, solver=solver, precon=None, **(dict(restart=30) if solver == 'fgmres' else {}))
    # the next matrix of the pattern: the first block moved
    values, rowptr, colidx = A.triplet()
    rows = torch.repeat_interleave(torch.arange(n, device=rowptr.device), rowptr[1:] - rowptr[:-1])
    velocity = device.to_dev(~second, 'uint8') != 0
    one = torch.ones_like(values)
    factor = torch.where(velocity[rows] & velocity[colidx], torch.where(rows == colidx, 1.08 * one, 1.05 * one), one)
    moved = A._with_values(values * factor)
    own, own_ms = setup(moved)
    out['lagged'] = dict(own=solve(moved, solver='fgmres', precon=own, restart=30), own_setup_ms=own_ms, lagged=solve(moved, solver='fgmres', precon=M, restart=30))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--matrices', default='poisson128,elasticity96,bilinear2048,p2vector32')
    ap.add_argument('--scale', type=float, default=1.)
    ap.add_argument('--window', type=float, default=.3)
    ap.add_argument('--maxiter', type=int, default=20000)
    ap.add_argument('--no-host-solve', action='store_true', help='skip the host BiCGStab of the nonsymmetric twin (minutes for the large matrices)')
    ap.add_argument('--sections', default='spmv,cg,bicgstab,fgmres,minres,amg', help='the parts of the probe to run')
    ap.add_argument('--amg-setup', default='', help="section 'amg', vector matrices: the kinds of plan to build the rigid-body hierarchy with, side by side, e.g. entry,block")
    ap.add_argument('--eigratios', default='', help="section 'smoother': the eigratio values of further Chebyshev degree-2 rows, e.g. 4,10,30")
    ap.add_argument('--eigsteps', default='', help="section 'smoother': the eigsteps values of further Chebyshev degree-2 rows, e.g. 5,10,20")
    ap.add_argument('--stokes', default='32', help="section 'saddle': the elements per side of the Taylor-Hood Stokes problems, e.g. 16,32,64")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    args.sections = args.sections.split(',')
    args.amg_setup = [v for v in args.amg_setup.split(',') if v]
    if set(args.amg_setup) - {'entry', 'block'}:
        raise SystemExit(f"--amg-setup takes 'entry' and 'block', got {args.amg_setup}")
    args.eigratios = [float(v) for v in args.eigratios.split(',') if v]
    args.eigsteps = [int(v) for v in args.eigsteps.split(',') if v]
    import torch
    out = open(args.out, 'a') if args.out else None
    runs = [lambda name=name: probe(name, args) for name in args.matrices.split(',') if name and set(args.sections) - {'saddle'}]
    if 'saddle' in args.sections:
        runs += [lambda ne=int(ne): probe_saddle(ne, args) for ne in args.stokes.split(',')]
    for run in runs:
        line = json.dumps(run())
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
