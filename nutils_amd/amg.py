'''Smoothed-aggregation algebraic multigrid for ``HipMatrix.solve(solver='cg', precon='amg')``.

Two phases.  ``symbolic`` reads the pattern and the constraint mask only and is written with torch tensor operations that run wherever their inputs
live (on the device in a solve, on CPU tensors in the tests): the aggregates, the CSR patterns of the prolongator P, the restriction R = P^T and the
coarse matrix A_c = R A P, and for each of the products A T, A P and R (A P) an expand-sort-compress plan -- the products of the sparse product listed,
sorted stably by output entry and cut into segments.  ``numeric`` reads values, on the device: every sparse product is one nh_segment_dot over its
plan, the step from A T to P and to the smoother's weights is elementwise, and the only thing that visits the host is the coarsest matrix (at most
``coarse``^2 doubles over PCIe), whose pseudo-inverse is computed there by numpy and applied on the device as a dense product.

The algorithm, level by level (A_f: the matrix on the free rows and columns; never formed on the finest level, where the row mask and zero rows of P
do it; coarse levels have no mask).  The pattern must be structurally symmetric.

weights      dinv = 1 / diag on free rows, 0 elsewhere; rho = max_i sum_j |a_ij| dinv_i over the free rows and columns (the Gershgorin bound of
             D^-1 A_f); omega = 4 / (3 rho), for the prolongator smoother and for the Jacobi smoother alike.
aggregation  a distance-2 maximal independent set by Luby rounds on the graph of the structural off-diagonal entries between free dofs.  Every dof has
             the unique priority key(i) = (top 31 bits of hash(i)) << 32 | i, with hash the fixed mix of ``keys``.  A round: k = key on undecided dofs,
             -1 elsewhere; m1 = max(k, neighbour-max k) on all dofs; m2 = max(m1, neighbour-max m1); an undecided dof with k == m2 becomes a root, every
             undecided dof within two edges of a new root is covered.  Then a root owns itself, a dof next to roots joins the one with the largest key,
             every other free dof joins, among its neighbours assigned in that step, the one whose root has the largest key.  Aggregates are numbered by
             ascending root index.  All of it is max-reductions: a pure function of pattern and mask.
prolongator  T[i, agg(i)] = 1 on free dofs; P = T - omega diag(dinv) A_f T (zero rows on constrained dofs), R = P^T stored as a CSR of its own,
             A_c = P^T A_f P.  P is held on the pattern of A_f T, which contains that of T wherever a free row has its diagonal entry.
termination  a level with at most ``coarse`` free dofs is solved densely (numpy.linalg.pinv(A_c, hermitian=True)); a level whose graph has no edges is
             solved by z = dinv b; any other level is coarsened.
cycle        V(sweeps, sweeps): x = omega dinv b, further sweeps x += omega dinv (b - A x), r = b - A x, x += P cycle(R r), `sweeps` sweeps more.  Equal
             pre- and post-smoothing with omega < 2 / rho keeps the cycle symmetric positive definite, which CG needs.

The constant is the only near-nullspace vector: elasticity gets a valid preconditioner, not an optimal one.'''

import numpy

MAX_COARSE = 1024  # the dense kernel's limit (nh_amg.hip)
_M32 = 0xffffffff


def _torch():
    import torch
    return torch


def _error():
    from .matrix import MatrixError  # (matrix imports this module in its solve)
    return MatrixError


def keys(n, device=None):
    '''int64 priorities of n dofs: h = (i + 1) 0x9E3779B97F4A7C15; h ^= h >> 32; h *= 0xD6E8FEB86659FD93; h ^= h >> 32 in wrapping 64-bit arithmetic with
    logical shifts; key = (h >> 33) << 32 | i'''
    torch = _torch()
    i = torch.arange(n, dtype=torch.int64, device=device)
    h = (i + 1) * (0x9E3779B97F4A7C15 - (1 << 64))  # (the constants as signed numbers: int64 products wrap)
    h = h ^ ((h >> 32) & _M32)  # (>> is arithmetic on int64: the mask makes it logical)
    h = h * (0xD6E8FEB86659FD93 - (1 << 64))
    h = h ^ ((h >> 32) & _M32)
    return (((h >> 33) & 0x7fffffff) << 32) | i


def _rows(rowptr):
    torch = _torch()
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=rowptr.device), rowptr[1:] - rowptr[:-1])


def _rowptr(rows, nrows):
    '''row pointers of sorted row indices'''
    torch = _torch()
    return torch.searchsorted(rows, torch.arange(nrows + 1, dtype=torch.int64, device=rows.device))


def aggregate(rowptr, colidx, free=None):
    '''(agg, nagg, rounds): agg[i] the aggregate of dof i, -1 on constrained dofs (bool tensor `free`; None: all free)'''
    torch = _torch()
    n = rowptr.numel() - 1
    rows = _rows(rowptr)
    keep = rows != colidx
    if free is not None:
        keep &= free[rows] & free[colidx]
    er, ec = rows[keep], colidx[keep]
    isfree = torch.ones(n, dtype=torch.bool, device=rowptr.device) if free is None else free

    def spread(v, own=True):  # max(v, neighbour-max v); own=False: the neighbour-max alone, -1 without neighbours
        out = v.clone() if own else torch.full_like(v, -1)
        return out.scatter_reduce_(0, er, v[ec], 'amax', include_self=True)

    key = keys(n, rowptr.device)
    undecided = isfree.clone()
    root = torch.zeros_like(isfree)
    rounds = 0
    while bool(undecided.any()):
        k = torch.where(undecided, key, -1)
        new = undecided & (k == spread(spread(k)))
        root |= new
        undecided &= spread(spread(new.to(torch.int64))) == 0
        rounds += 1
    owner = torch.where(root, key, torch.where(isfree, spread(torch.where(root, key, -1), own=False), -1))  # the key of the root a dof joins, -1: none yet
    owner = torch.where(isfree & (owner < 0), spread(owner, own=False), owner)
    if bool((isfree & (owner < 0)).any()):
        raise _error()('aggregation left free dofs without a root within two edges: the pattern is not structurally symmetric')
    number = torch.cumsum(root.to(torch.int64), 0) - 1
    agg = torch.where(isfree, number[owner.clamp(min=0) & _M32], -1)
    return agg, int(root.sum()), rounds


class Plan:
    '''expand-sort-compress plan of a sparse product: segment s sums products ptr[s] .. ptr[s + 1] - 1, product k = a[ia[k]] * b[ib[k]] (ib None: a[ia[k]]);
    rows / cols: the output entry of each segment, sorted by (row, col)'''

    def __init__(self, out_rows, out_cols, ncols, ia, ib):
        torch = _torch()
        nprod = ia.numel()
        if nprod >= 1 << 31:
            raise _error()(f'a sparse product of {nprod} terms exceeds the int32 indices of its plan')
        key, order = torch.sort(out_rows * ncols + out_cols, stable=True)
        ukey, counts = torch.unique_consecutive(key, return_counts=True)
        self.ptr = torch.zeros(ukey.numel() + 1, dtype=torch.int64, device=ia.device)
        torch.cumsum(counts, 0, out=self.ptr[1:])
        self.ia = ia[order].to(torch.int32)
        self.ib = None if ib is None else ib[order].to(torch.int32)
        self.rows = torch.div(ukey, ncols, rounding_mode='floor')
        self.cols = ukey - self.rows * ncols
        self.nseg, self.nprod = ukey.numel(), nprod


def _expand(index, ptr):
    '''for every i and every position m of ptr[index[i]] .. ptr[index[i] + 1] - 1: (i, m), i ascending and m ascending within i'''
    torch = _torch()
    count = ptr[index + 1] - ptr[index]
    src = torch.repeat_interleave(torch.arange(index.numel(), dtype=torch.int64, device=index.device), count)
    start = torch.cumsum(count, 0) - count
    return src, ptr[index][src] + torch.arange(src.numel(), dtype=torch.int64, device=index.device) - start[src]


class Level:
    '''What the symbolic phase knows of a level: n dofs, nfree of them free (`free`: bool tensor, None: all), the CSR pattern (rowptr, colidx) and `kind`
    ('coarsen', 'dense' or 'diagonal').  Of a coarsened level also: agg, nc; the pattern of P (prowptr, prow, pcol) with tind = T on it; the permutation
    rperm that takes the values of P to those of R, and R's pattern (rrowptr, rcol); the plans at (A T), ap (A P) and rap (R (A P)), whose output entries
    are the patterns of P, A P and A_c.'''


def _coarsen(lv):
    torch = _torch()
    rowptr, colidx, free, n = lv.rowptr, lv.colidx, lv.free, lv.n
    lv.agg, lv.nc, lv.rounds = aggregate(rowptr, colidx, free)
    nc = lv.nc
    rows = _rows(rowptr)
    k = torch.arange(colidx.numel(), dtype=torch.int64, device=colidx.device)
    if free is not None:
        k = k[free[rows] & free[colidx]]  # the entries of A_f
    arow, acol = rows[k], colidx[k]
    lv.at = Plan(arow, lv.agg[acol], nc, k, None)
    lv.prow, lv.pcol = lv.at.rows, lv.at.cols
    lv.prowptr = _rowptr(lv.prow, n)
    lv.tind = (lv.pcol == lv.agg[lv.prow]).to(torch.float64)
    src, m = _expand(acol, lv.prowptr)
    lv.ap = Plan(arow[src], lv.pcol[m], nc, k[src], m)
    aprowptr = _rowptr(lv.ap.rows, n)
    _, lv.rperm = torch.sort(lv.pcol * n + lv.prow, stable=True)
    rrow, lv.rcol = lv.pcol[lv.rperm], lv.prow[lv.rperm]
    lv.rrowptr = _rowptr(rrow, nc)
    lv.pcol32, lv.rcol32 = lv.pcol.to(torch.int32), lv.rcol.to(torch.int32)  # (nc and n are within int32: the keys hold the index in 32 bits)
    src, m = _expand(lv.rcol, aprowptr)
    lv.rap = Plan(rrow[src], lv.ap.cols[m], nc, src, m)
    return _rowptr(lv.rap.rows, nc), lv.rap.cols


def _dense_block(lv):
    '''the free block of a dense level, selected where the pattern lies: dk the positions of its entries in the value array, (drow, dcol) their place in the
    nfree x nfree matrix (free dofs renumbered in ascending order), idx32 the free dofs (None: all).  At most nfree^2 entries: what of this level goes to the host.'''
    torch = _torch()
    rows = _rows(lv.rowptr)
    if lv.free is None:
        lv.dk, lv.drow, lv.dcol, lv.idx32 = torch.arange(lv.colidx.numel(), dtype=torch.int64, device=rows.device), rows, lv.colidx, None
    else:
        lv.dk = torch.nonzero(lv.free[rows] & lv.free[lv.colidx]).reshape(-1)
        number = torch.cumsum(lv.free.to(torch.int64), 0) - 1
        lv.drow, lv.dcol = number[rows[lv.dk]], number[lv.colidx[lv.dk]]
        lv.idx32 = torch.nonzero(lv.free).reshape(-1).to(torch.int32)


def symbolic(rowptr, colidx, free=None, coarse=256):
    '''The levels of the hierarchy of a pattern and a mask (`free`: bool tensor, True on free dofs; None: all): a list of `Level`, the last of which is
    'dense' or 'diagonal'.  No value is read.'''
    torch = _torch()
    levels = []
    while True:
        lv = Level()
        lv.rowptr, lv.colidx, lv.free = rowptr, colidx, free
        lv.n = rowptr.numel() - 1
        lv.nfree = lv.n if free is None else int(free.sum())
        if lv.n > 0x7fffffff:
            raise _error()(f'{lv.n} dofs exceed the 32 bits the priorities of the aggregation keep for the index')
        lv.col32 = colidx.to(torch.int32)  # what the products of the cycle read (12 instead of 16 bytes per entry)
        lv.mask = None if free is None else free.to(torch.uint8)
        levels.append(lv)
        if lv.nfree <= coarse:
            lv.kind = 'dense'
            _dense_block(lv)
            return levels
        rowptr, colidx = _coarsen(lv)
        if lv.nc == lv.nfree:  # no edges: a diagonal matrix
            lv.kind = 'diagonal'
            return levels
        lv.kind = 'coarsen'
        free = None


def check_args(preconargs):
    '''(coarse, sweeps) of `preconargs`, validated'''
    from .matrix import MatrixError
    args = dict(preconargs or {})
    coarse, sweeps = args.pop('coarse', 256), args.pop('sweeps', 1)
    if args:
        raise MatrixError(f"invalid arguments {sorted(args)} for the 'amg' preconditioner: 'coarse' and 'sweeps'")
    isint = lambda v: isinstance(v, (int, numpy.integer)) and not isinstance(v, bool)
    if not (isint(coarse) and 1 <= coarse <= MAX_COARSE):
        raise MatrixError(f'amg: coarse must be an integer between 1 and {MAX_COARSE}, got {coarse!r}')
    if not (isint(sweeps) and sweeps >= 1):
        raise MatrixError(f'amg: sweeps must be an integer of at least 1, got {sweeps!r}')
    return int(coarse), int(sweeps)


class Hierarchy:
    '''The numeric phase on the device: the values of every level from those of the finest (`values`, on the pattern of `levels[0]`), and the handle of the
    cycle.  `levels`: of `symbolic`, on device tensors.  Per level `self.data[l]` keeps what the cycle reads: values, dinv, and for a coarsened level rho,
    omega (0-dim device tensors), w = omega dinv, pvalues, rvalues; for a dense level ainv.'''

    def __init__(self, levels, values, sweeps=1):
        from . import device, kernels
        from .matrix import MatrixError, spmv_lanes
        torch = _torch()
        self.levels, self.data = levels, []
        descriptions = []
        for l, lv in enumerate(levels):
            d = Level()
            self.data.append(d)
            d.values = values
            lanes = spmv_lanes(lv.n, lv.colidx.numel())
            diag = kernels.csr_diagonal(values, lv.rowptr, lv.colidx, lv.n, col32=lv.col32)
            keep = torch.ones_like(diag, dtype=torch.bool) if lv.free is None else lv.free
            if bool(((diag == 0) & keep).any()):
                raise MatrixError("building 'amg' preconditioner: diagonal has zero entries")
            d.dinv = (1. / diag).masked_fill(~keep | (diag == 0), 0.)
            d.b, d.x = (None, None) if l == 0 else (device.empty(lv.n, 'float64'), device.empty(lv.n, 'float64'))
            desc = dict(A=(values, lv.rowptr, lv.colidx, lv.n, lv.col32, lanes), rowmask=lv.mask, b=d.b, x=d.x, sweeps=sweeps)
            descriptions.append(desc)
            if lv.kind == 'dense':
                # PCIe: the one small matrix that visits the host, its free block only (at most coarse^2 entries, whatever n is)
                dense = numpy.zeros((lv.nfree, lv.nfree))
                numpy.add.at(dense, (device.to_host(lv.drow), device.to_host(lv.dcol)), device.to_host(values[lv.dk]))
                d.idx = lv.idx32
                d.ainv = device.to_dev(numpy.linalg.pinv(dense, hermitian=True).ravel(), 'float64') if lv.nfree else None
                desc.update(kind='dense', ndense=lv.nfree, Ainv=d.ainv, idx=d.idx)
                break
            if lv.kind == 'diagonal':
                desc.update(kind='diagonal', w=d.dinv)
                break
            absrow = kernels.csr_spmv(values.abs(), lv.rowptr, lv.colidx, lv.n, keep.to(torch.float64), rowmask=lv.mask, col32=lv.col32, lanes=lanes)
            d.rho = (absrow * d.dinv).max()
            d.omega = 4. / (3. * d.rho)
            d.w = d.omega * d.dinv
            d.atvalues = kernels.segment_dot(lv.at, values)
            d.pvalues = lv.tind - d.w[lv.prow] * d.atvalues
            d.rvalues = d.pvalues[lv.rperm]
            d.apvalues = kernels.segment_dot(lv.ap, values, d.pvalues)
            d.t, d.r = device.empty(lv.n, 'float64'), device.empty(lv.n, 'float64')
            desc.update(kind='coarsen', w=d.w, t=d.t, r=d.r, P=(d.pvalues, lv.prowptr, lv.pcol, lv.nc, lv.pcol32, 0), R=(d.rvalues, lv.rrowptr, lv.rcol, lv.n, lv.rcol32, 0))
            values = kernels.segment_dot(lv.rap, d.rvalues, d.apvalues)
        self.handle = kernels.Amg(descriptions)

    def apply(self, r, z=None):
        '''z = M r, one cycle (nh_amg_apply)'''
        return self.handle.apply(r, z)
