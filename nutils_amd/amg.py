'''Smoothed-aggregation algebraic multigrid for ``HipMatrix.solve(solver='cg', precon='amg')`` and, as an object of ``HipMatrix.getprecon`` (``Preconditioner``),
for ``solve(solver='cg' | 'fgmres', precon=M)``; on a masked first block it is also half of the block preconditioner of a saddle point (``Schur``).

Two phases.  ``symbolic`` reads the pattern and the constraint mask only and is written with torch tensor operations that run wherever their inputs
live (on the device in a solve, on CPU tensors in the tests): the aggregates, the CSR patterns of the prolongator P, the restriction R = P^T and the
coarse matrix A_c = R A P, and for each of the products A T, A P and R (A P) an expand-sort-compress plan -- the products of the sparse product listed,
sorted stably by output entry and cut into segments.  ``numeric`` reads values, on the device: every sparse product is one nh_segment_dot over its
plan (one nh_block_segment_dot with the block plans at the end of this text), the step from A T to P and to the smoother's weights is elementwise, and the only matrix that visits the host is the coarsest (at most
``coarse``^2 doubles over PCIe), whose pseudo-inverse is computed there by numpy and applied on the device as a dense product.  With the Chebyshev
smoother a level also sends the host the coefficients of its Lanczos recurrence (2 eigsteps + 1 doubles) and its rho, and gets 2 degree doubles back.

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
termination  a level with at most ``coarse`` free dofs is solved densely (numpy.linalg.pinv(A_c, hermitian=True); for a hierarchy made with symmetric=False,
             whose matrix need not be symmetric, the general numpy.linalg.pinv(A_c)); a level whose graph has no edges is solved by z = dinv b; any other
             level is coarsened.
cycle        V(sweeps, sweeps): x = omega dinv b, further sweeps x += omega dinv (b - A x), r = b - A x, x += P cycle(R r), `sweeps` sweeps more.  Equal
             pre- and post-smoothing with omega < 2 / rho keeps the cycle symmetric positive definite, which CG needs.
chebyshev    ``smoother='chebyshev'`` (``degree=2, eigsteps=10, eigratio=10.``) replaces the Jacobi sweeps of every coarsened level by a Chebyshev polynomial in
             D^-1 A_f; P and the hierarchy stay as they are.  Estimate: `eigsteps` Lanczos steps on S A_f S, S = sqrt(dinv), from q_0 = u / |u|, u = the top 31
             bits of the hash of ``keys`` scaled to [-1, 1) (``start_vector``), 0 on masked rows and where dinv = 0 (nh_csr_lanczos; a vanishing or
             non-finite beta ends it early); theta = the largest eigenvalue of the tridiagonal matrix, by numpy on the host.  Bounds: ub = min(1.1 theta, rho)
             (theta approaches the largest eigenvalue from below, rho is a true bound), lb = ub / eigratio.  Smoother: with tc = (ub + lb) / 2,
             delta = (ub - lb) / 2, rho_0 = delta / tc, rho_k = 1 / (2 tc / delta - rho_(k-1)): d = dinv (b - A x) / tc, x += d, then
             d = rho_k rho_(k-1) d + (2 rho_k / delta) dinv (b - A x), x += d for k = 1 .. degree - 1.  Before the coarse correction it starts from x = 0 (no
             product in the first step), after it the same `degree` steps run on the corrected x: equal polynomials keep the cycle symmetric, ub at or
             above the largest eigenvalue keeps it positive definite.  A cycle of degree d costs what a Jacobi cycle with sweeps = d costs.

Without further arguments the constant is the only near-nullspace vector, which is right for scalar problems; elasticity then gets a valid preconditioner,
not an optimal one.  A vector problem hands its near-nullspace B [n x k], k <= 6, to the setup (``preconargs=dict(nullspace=B)``; for elasticity the
rigid-body modes, ``rigid_body_modes``), and the algorithm becomes:

nodes        on level 0 every dof is a node, on a coarse level node = dof // k; the aggregation runs on the graph of nodes (I next to J where an entry of A_f
             joins a dof of one to a dof of the other), and a dof is in the aggregate of its node.
prolongator  T has k columns per aggregate: on the rows of aggregate a, the columns a k .. a k + k - 1 hold the Q of the thin QR of B on those rows
             (nh_aggregate_qr: Gram-Schmidt in two passes, a column that vanishes against the earlier ones is dropped: zero in Q, a zero diagonal entry in R).
             The triangles R, stacked, are the B of the coarse level, which has k dofs per aggregate and no mask.  P, R = P^T and A_c as above.
dropped      the coarse dof of a dropped column has a zero column of P, a zero row and column of A_c: dinv = 0 there, the smoother leaves it alone and the
             pseudo-inverse of the dense level ignores it.
termination  at most ``coarse`` free dofs: dense; as many aggregates as free nodes: z = dinv b, exact for k = 1 and symmetric positive semidefinite always.
block plans  ``preconargs=dict(nullspace=B, setup='block')``.  With k vectors the patterns are blocks by construction: the columns of every row of P and A P come in
             full groups a k .. a k + k - 1, A_c and every level matrix below the finest are made of full k x k blocks.  'entry' (the default, the plans above) lists
             every scalar product; 'block' runs the symbolic phase on the quotient (rows grouped by node, the columns of T, P and A P by aggregate) and lists one
             product per pair of blocks (``BlockPlan``): k (A T, A P) and k^2 (R (A P)) times fewer on level 0, k^3 times fewer below.  From the block patterns it
             derives the same integers 'entry' makes (the patterns of P, R, A P and A_c, tmap, rperm), and for every block its first entry and its row stride in
             the scalar CSR value array, which is where nh_block_segment_dot reads and writes: the cycle reads scalar CSR either way.  That rests on the rows of a
             node having one length and one set of columns, in full groups: ``node_blocks`` checks it on every level and raises MatrixError otherwise.  Without
             `setup`, a near-nullspace and an entry plan whose product count reaches MAX_NPROD make the whole hierarchy again as 'block'.'''

import functools
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


MAX_NPROD = 1 << 31  # what the int32 indices of a plan can count


@functools.lru_cache(maxsize=None)
def _overflow():
    '''the MatrixError of a plan that outgrows its indices: what ``symbolic(..., setup=None)`` answers with block plans, and nothing else'''
    return type('PlanOverflow', (_error(),), {})


def _check_nprod(nprod, blocks=False):
    if nprod >= MAX_NPROD:
        if blocks:
            raise _error()(f'a sparse product of {nprod} block terms, or an offset of {nprod} into its value arrays, exceeds the int32 indices of its plan')
        raise _overflow()(f"a sparse product of {nprod} terms exceeds the int32 indices of its plan; with a near-nullspace, preconargs=dict(setup='block') states "
                          'the plans over blocks, k to k^3 times fewer terms')


class Plan:
    '''expand-sort-compress plan of a sparse product: segment s sums products ptr[s] .. ptr[s + 1] - 1, product k = a[ia[k]] * b[ib[k]] (ib None: a[ia[k]]);
    rows / cols: the output entry of each segment, sorted by (row, col)'''

    def __init__(self, out_rows, out_cols, ncols, ia, ib):
        torch = _torch()
        nprod = ia.numel()
        _check_nprod(nprod)
        key, order = torch.sort(out_rows * ncols + out_cols, stable=True)
        ukey, counts = torch.unique_consecutive(key, return_counts=True)
        self.ptr = torch.zeros(ukey.numel() + 1, dtype=torch.int64, device=ia.device)
        torch.cumsum(counts, 0, out=self.ptr[1:])
        self.ia = ia[order].to(torch.int32)
        self.ib = None if ib is None else ib[order].to(torch.int32)
        self.rows = torch.div(ukey, ncols, rounding_mode='floor')
        self.cols = ukey - self.rows * ncols
        self.nseg, self.nprod = ukey.numel(), nprod


def _expand(index, ptr, blocks=False):
    '''for every i and every position m of ptr[index[i]] .. ptr[index[i] + 1] - 1: (i, m), i ascending and m ascending within i'''
    torch = _torch()
    count = ptr[index + 1] - ptr[index]
    _check_nprod(int(count.sum()), blocks)  # (before the lists are made, not after: they are what runs out of memory)
    src = torch.repeat_interleave(torch.arange(index.numel(), dtype=torch.int64, device=index.device), count)
    start = torch.cumsum(count, 0) - count
    return src, ptr[index][src] + torch.arange(src.numel(), dtype=torch.int64, device=index.device) - start[src]


class Level:
    '''What the symbolic phase knows of a level: n dofs, nfree of them free (`free`: bool tensor, None: all), the CSR pattern (rowptr, colidx) and `kind`
    ('coarsen', 'dense' or 'diagonal').  Of a coarsened level also: agg, nc; the pattern of P (prowptr, prow, pcol) with tind = T on it; the permutation
    rperm that takes the values of P to those of R, and R's pattern (rrowptr, rcol); the plans at (A T), ap (A P) and rap (R (A P)), whose output entries
    are the patterns of P, A P and A_c.  With a near-nullspace of k vectors (`k`; None without): nodesize (1 on level 0, k below: the dofs of a node), nagg,
    nc = nagg k, the free dofs aggregate by aggregate (mptr, midx), the plan `at` with two factors, a[e] T[acol[e], j] on T's value array [n x k], and
    instead of tind the map tmap from the entries of P into that array (-1: none).  `setup`: 'entry' or 'block', the kind of plans the hierarchy was made
    with; of a 'block' level at, ap and rap are `BlockPlan`s, every other integer is what 'entry' makes.'''


def _node_graph(rowptr, colidx, size):
    '''the CSR pattern of the graph whose node I is the dofs I size .. I size + size - 1: I next to J where an entry joins a dof of one to a dof of the other'''
    torch = _torch()
    nnodes = (rowptr.numel() - 1) // size
    key = torch.unique(torch.div(_rows(rowptr), size, rounding_mode='floor') * nnodes + torch.div(colidx, size, rounding_mode='floor'))  # (sorted)
    rows = torch.div(key, nnodes, rounding_mode='floor')
    return _rowptr(rows, nnodes), key - rows * nnodes


def _aggregate_nodes(lv):
    '''agg, nagg, rounds and nc of a level; returns the aggregate of every node'''
    torch = _torch()
    if lv.k is None or lv.nodesize == 1:
        lv.agg, lv.nagg, lv.rounds = aggregate(lv.rowptr, lv.colidx, lv.free)
        nodeagg = lv.agg
    else:  # a coarse level of a hierarchy with a near-nullspace: the k dofs of a node stay together
        nodeagg, lv.nagg, lv.rounds = aggregate(*_node_graph(lv.rowptr, lv.colidx, lv.nodesize))
        lv.agg = nodeagg[torch.div(torch.arange(lv.n, dtype=torch.int64, device=lv.rowptr.device), lv.nodesize, rounding_mode='floor')]
    lv.nc = lv.nagg * (lv.k or 1)
    return nodeagg


def _members(lv):
    '''mptr, midx: the free dofs aggregate by aggregate, ascending within one: what nh_aggregate_qr walks'''
    torch = _torch()
    dofs = torch.arange(lv.n, dtype=torch.int64, device=lv.rowptr.device) if lv.free is None else torch.nonzero(lv.free).reshape(-1)
    sagg, order = torch.sort(lv.agg[dofs], stable=True)
    lv.mptr, lv.midx = _rowptr(sagg, lv.nagg), dofs[order].to(torch.int32)


def _coarsen(lv):
    if lv.setup == 'block':
        return _coarsen_blocks(lv)
    torch = _torch()
    rowptr, colidx, free, n, nk = lv.rowptr, lv.colidx, lv.free, lv.n, lv.k
    _aggregate_nodes(lv)
    nc = lv.nc
    rows = _rows(rowptr)
    k = torch.arange(colidx.numel(), dtype=torch.int64, device=colidx.device)
    if free is not None:
        k = k[free[rows] & free[colidx]]  # the entries of A_f
    arow, acol = rows[k], colidx[k]
    if nk is None:
        lv.at = Plan(arow, lv.agg[acol], nc, k, None)
    else:
        if n * nk >= 1 << 31:
            raise _error()(f'{n} dofs times {nk} near-nullspace vectors exceed the int32 indices of the plans')
        _check_nprod(k.numel() * nk)
        _members(lv)
        j = torch.arange(nk, dtype=torch.int64, device=rowptr.device).repeat(k.numel())
        ke, re, ce = (t.repeat_interleave(nk) for t in (k, arow, acol))
        lv.at = Plan(re, lv.agg[ce] * nk + j, nc, ke, ce * nk + j)  # (A T)[i, agg(c) k + j] = sum over the entries (i, c) of a[e] T[c, j], T = Q [n x k]
    lv.prow, lv.pcol = lv.at.rows, lv.at.cols
    lv.prowptr = _rowptr(lv.prow, n)
    if nk is None:
        lv.tind = (lv.pcol == lv.agg[lv.prow]).to(torch.float64)
    else:  # where an entry of P finds its T in the value array Q, -1: T has none there
        block = torch.div(lv.pcol, nk, rounding_mode='floor')
        lv.tmap = torch.where(block == lv.agg[lv.prow], lv.prow * nk + (lv.pcol - block * nk), -1)
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


# ---- the same three products stated over blocks (setup='block') ------------------------------------------------------------

class BlockPlan:
    '''expand-sort-compress plan of a sparse product over blocks that lie in scalar CSR value arrays (nh_block_segment_dot): segment s is the output block
    (p x k) at out[of[s] + r os[s] + c], the sum over the products m = ptr[s] .. ptr[s + 1] - 1 of the block (p x q) at a[ia[m] + r sa[s] + t] times the block
    (q x k) at b[ib[m] + t sb[m] + c]; sb None: the stride `bstride` for all of them.  p and q are 1 or k.  brows / bcols: the output block of each segment,
    sorted by (row, column); of, os and sa are the caller's to fill in once the output's layout is known (`_layout`), nout being its scalar size.'''

    def __init__(self, k, p, q, out_brows, out_bcols, nbcols, ia, ib, sb=None, bstride=0):
        torch = _torch()
        nprod = ia.numel()
        _check_nprod(nprod, True)
        key, order = torch.sort(out_brows * nbcols + out_bcols, stable=True)
        ukey, counts = torch.unique_consecutive(key, return_counts=True)
        self.ptr = torch.zeros(ukey.numel() + 1, dtype=torch.int64, device=ia.device)
        torch.cumsum(counts, 0, out=self.ptr[1:])
        self.ia, self.ib = ia[order].to(torch.int32), ib[order].to(torch.int32)
        self.sb = None if sb is None else sb[order].to(torch.int32)
        self.brows = torch.div(ukey, nbcols, rounding_mode='floor')
        self.bcols = ukey - self.brows * nbcols
        self.k, self.p, self.q, self.bstride = k, p, q, bstride
        self.nseg, self.nprod, self.nout = ukey.numel(), nprod, ukey.numel() * p * k
        self.sa = self.of = self.os = None

    def scalar_pattern(self):
        '''(rows, cols) of the output's scalar entries, in the order of its value array'''
        return _scalar_pattern(self.brows, self.bcols, self.of, self.os, self.p, self.k)


def _layout(brows, nbrows, p, s):
    '''where the blocks (p x s) of a block pattern sorted by (row, column) lie in the scalar CSR of the same matrix: (first, stride, bptr, rowptr) -- the
    first entry of every block, the row stride of every block ROW (the length of its scalar rows), the block row pointers and the scalar ones'''
    torch = _torch()
    bptr = _rowptr(brows, nbrows)
    cnt = bptr[1:] - bptr[:-1]
    _check_nprod(brows.numel() * p * s, True)
    first = (bptr[brows] * (p - 1) + torch.arange(brows.numel(), dtype=torch.int64, device=brows.device)) * s  # ((bptr[I] p + position in the row) s)
    stride = cnt * s
    rowptr = torch.empty(nbrows * p + 1, dtype=torch.int64, device=brows.device)
    rowptr[:-1] = ((bptr[:-1] * (p * s)).reshape(-1, 1) + torch.arange(p, dtype=torch.int64, device=brows.device) * stride.reshape(-1, 1)).reshape(-1)
    rowptr[-1] = brows.numel() * p * s
    return first, stride, bptr, rowptr


def _block_entries(first, stride, p, s):
    '''the index of entry (r, c) of every block in the scalar value array: [blocks, p, s]'''
    torch = _torch()
    r, c = (torch.arange(m, dtype=torch.int64, device=first.device) for m in (p, s))
    return first.reshape(-1, 1, 1) + r.reshape(1, -1, 1) * stride.reshape(-1, 1, 1) + c.reshape(1, 1, -1)


def _scalar_pattern(brows, bcols, first, stride, p, s):
    '''(rows, cols): the scalar entries of the blocks (p x s), in the order of the value array; stride: of every block'''
    torch = _torch()
    idx = _block_entries(first.to(torch.int64), stride.to(torch.int64), p, s)
    rows, cols = torch.empty(idx.numel(), dtype=torch.int64, device=idx.device), torch.empty(idx.numel(), dtype=torch.int64, device=idx.device)
    r, c = (torch.arange(m, dtype=torch.int64, device=idx.device) for m in (p, s))
    rows[idx.reshape(-1)] = (brows.reshape(-1, 1, 1) * p + r.reshape(1, -1, 1)).expand(idx.shape).reshape(-1)
    cols[idx.reshape(-1)] = (bcols.reshape(-1, 1, 1) * s + c.reshape(1, 1, -1)).expand(idx.shape).reshape(-1)
    return rows, cols


def node_blocks(rowptr, colidx, size):
    '''(brows, bcols, first, length): the blocks (size x size) of a level matrix whose node I is the dofs I size .. I size + size - 1, sorted by (row, column),
    the position `first` of the first entry of each in the scalar value array, and the length of every scalar row (the row stride of the blocks of its node).
    This CHECKS what the block kernel relies on, since it writes where these integers point: the rows of a node have one length and one set of columns, and
    the columns come in full groups J size .. J size + size - 1.  MatrixError otherwise.'''
    torch = _torch()
    n = rowptr.numel() - 1
    length = rowptr[1:] - rowptr[:-1]
    rows = _rows(rowptr)
    e = torch.arange(colidx.numel(), dtype=torch.int64, device=colidx.device)
    t = e - rowptr[rows]  # the position in the row
    head = rows - rows % size  # the first dof of the node
    ok = n % size == 0 and bool((length == length[torch.arange(n, dtype=torch.int64, device=rowptr.device) // size * size]).all()) and bool((length % size == 0).all())
    if ok:
        j = t % size
        ok = bool((colidx == colidx[rowptr[head] + t]).all()) and bool((colidx % size == j).all()) and bool((colidx - j == colidx[e - j]).all())
    if not ok:
        raise _error()(f"amg: setup='block' needs a level matrix made of full {size} x {size} blocks, rows of a node with one length and one set of columns; "
                       "this one is not (setup='entry' makes no such assumption)")
    lead = (rows % size == 0) & (t % size == 0)
    first = e[lead]
    return rows[first] // size, colidx[first] // size, first, length


def _coarsen_blocks(lv):
    '''`_coarsen` on the quotient: rows grouped by node, the columns of T, P and A P by aggregate, one product per pair of blocks; from the block patterns the
    integers of the scalar CSRs that `_coarsen` makes, the same'''
    torch = _torch()
    rowptr, colidx, free, n, nk, ns = lv.rowptr, lv.colidx, lv.free, lv.n, lv.k, lv.nodesize
    i64 = dict(dtype=torch.int64, device=rowptr.device)
    nodeagg = _aggregate_nodes(lv)
    nagg, nn = lv.nagg, n // ns
    if n * nk >= MAX_NPROD:
        raise _error()(f'{n} dofs times {nk} near-nullspace vectors exceed the int32 indices of the plans')
    _check_nprod(colidx.numel(), True)
    _members(lv)
    if ns == 1:  # the entries of A_f, blocks of one entry
        rows = _rows(rowptr)
        first = torch.arange(colidx.numel(), **i64)
        if free is not None:
            first = first[free[rows] & free[colidx]]
        brows, bcols, length = rows[first], colidx[first], None
    else:
        if free is not None:
            raise _error()('amg: a level with nodes of several dofs has no mask')
        brows, bcols, first, length = node_blocks(rowptr, colidx, ns)
        length = length[::ns]  # of every node
    sa = lambda plan: None if ns == 1 else length[plan.brows].to(torch.int32)
    # A T: the block (I, J) of A times the rows of node J of Q [n x k]
    at = lv.at = BlockPlan(nk, ns, ns, brows, nodeagg[bcols], nagg, first, bcols * (ns * nk), None, nk)
    pfirst, pstride, pbptr, lv.prowptr = _layout(at.brows, nn, ns, nk)
    pbrows, pbcols = at.brows, at.bcols
    at.sa, at.of, at.os = sa(at), pfirst.to(torch.int32), pstride[pbrows].to(torch.int32)
    lv.prow, lv.pcol = at.scalar_pattern()
    block = torch.div(lv.pcol, nk, rounding_mode='floor')
    lv.tmap = torch.where(block == lv.agg[lv.prow], lv.prow * nk + (lv.pcol - block * nk), -1)
    # A P: the block (I, J) of A times every block of the block row J of P
    src, m = _expand(bcols, pbptr, True)
    ap = lv.ap = BlockPlan(nk, ns, ns, brows[src], pbcols[m], nagg, first[src], pfirst[m], None if ns == 1 else pstride[pbrows[m]])
    apfirst, apstride, apbptr, _ = _layout(ap.brows, nn, ns, nk)
    ap.sa, ap.of, ap.os = sa(ap), apfirst.to(torch.int32), apstride[ap.brows].to(torch.int32)
    # R = P^T: its blocks (k x nodesize) sorted by (aggregate, node), each entry from its twin in P
    _, bperm = torch.sort(pbcols * nn + pbrows, stable=True)
    rbrows, rbcols = pbcols[bperm], pbrows[bperm]
    rfirst, rstride, _, lv.rrowptr = _layout(rbrows, nagg, nk, ns)
    twin = _block_entries(pfirst[bperm], pstride[rbcols], ns, nk).transpose(1, 2)  # [blocks, k, nodesize]: the entry (r, j) of P's block at (j, r)
    lv.rperm = torch.empty(twin.numel(), **i64)
    lv.rperm[_block_entries(rfirst, rstride[rbrows], nk, ns).reshape(-1)] = twin.reshape(-1)
    rrow, lv.rcol = _scalar_pattern(rbrows, rbcols, rfirst, rstride[rbrows], nk, ns)
    lv.pcol32, lv.rcol32 = lv.pcol.to(torch.int32), lv.rcol.to(torch.int32)
    # R (A P): the block (a, I) of R times every block of the block row I of A P
    src, m = _expand(rbcols, apbptr, True)
    rap = lv.rap = BlockPlan(nk, nk, ns, rbrows[src], ap.bcols[m], nagg, rfirst[src], apfirst[m], None if ns == 1 else apstride[ap.brows[m]])
    acfirst, acstride, _, acrowptr = _layout(rap.brows, nagg, nk, nk)
    rap.sa, rap.of, rap.os = (None if nk == 1 else rstride[rap.brows].to(torch.int32)), acfirst.to(torch.int32), acstride[rap.brows].to(torch.int32)
    return acrowptr, rap.scalar_pattern()[1]


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


SETUPS = None, 'entry', 'block'


def check_setup(setup, nullspace):
    '''`setup` validated against the near-nullspace (anything that is None without one)'''
    if not (setup is None or isinstance(setup, str)) or setup not in SETUPS:
        raise _error()(f"amg: setup must be 'entry', 'block' or None, got {setup!r}")
    if setup == 'block' and nullspace is None:
        raise _error()("amg: setup='block' states the plans over the k x k blocks of a near-nullspace and needs `nullspace`; with the constant the entry plans "
                       'are the block plans')
    return setup


def split_setup(preconargs):
    '''(rest, setup): the key 'setup' of `preconargs` taken out and validated, the others left for `check_args`'''
    rest = dict(preconargs or {})
    setup = rest.pop('setup', None)
    return rest, check_setup(setup, rest.get('nullspace'))


def symbolic(rowptr, colidx, free=None, coarse=256, nullspace=None, *, setup=None):
    '''The levels of the hierarchy of a pattern and a mask (`free`: bool tensor, True on free dofs; None: all): a list of `Level`, the last of which is
    'dense' or 'diagonal'.  `nullspace`: the number k of near-nullspace vectors the numeric phase will be given (None: the constant, on every level).  No
    value is read.  `setup`: 'entry' (plans over scalar products), 'block' (over block products; needs `nullspace`) or None: 'entry', unless there is a
    near-nullspace and a product count of the entry plans reaches MAX_NPROD -- then the whole hierarchy is made again as 'block'.'''
    check_setup(setup, nullspace)
    if setup is None and nullspace is not None:
        try:
            return _symbolic(rowptr, colidx, free, coarse, nullspace, 'entry')
        except _overflow():  # (the count of a plan, known before its lists exist; no other MatrixError)
            return _symbolic(rowptr, colidx, free, coarse, nullspace, 'block')
    return _symbolic(rowptr, colidx, free, coarse, nullspace, setup or 'entry')


def _symbolic(rowptr, colidx, free, coarse, nullspace, setup):
    torch = _torch()
    levels = []
    while True:
        lv = Level()
        lv.setup = setup
        lv.rowptr, lv.colidx, lv.free = rowptr, colidx, free
        lv.n = rowptr.numel() - 1
        lv.nfree = lv.n if free is None else int(free.sum())
        lv.k, lv.nodesize = nullspace, 1 if nullspace is None or not levels else nullspace
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
        if lv.nagg * lv.nodesize == lv.nfree:  # as many aggregates as free nodes, no edges: a diagonal matrix (with a near-nullspace of k > 1: diagonal blocks)
            lv.kind = 'diagonal'
            return levels
        lv.kind = 'coarsen'
        free = None


MAX_NULLSPACE = 6  # the QR kernel's limit (nh_amg.hip): the rigid-body modes in 3-D


def check_args(preconargs, n=None):
    '''(coarse, sweeps, nullspace) of `preconargs`, validated; nullspace: None, or a float64 host array or device tensor of shape (n, k), n the size of the
    matrix when given'''
    from .matrix import MatrixError
    args = dict(preconargs or {})
    coarse, sweeps, B = args.pop('coarse', 256), args.pop('sweeps', 1), args.pop('nullspace', None)
    if args:
        raise MatrixError(f"invalid arguments {sorted(args)} for the 'amg' preconditioner: 'coarse', 'sweeps' and 'nullspace'")
    isint = lambda v: isinstance(v, (int, numpy.integer)) and not isinstance(v, bool)
    if not (isint(coarse) and 1 <= coarse <= MAX_COARSE):
        raise MatrixError(f'amg: coarse must be an integer between 1 and {MAX_COARSE}, got {coarse!r}')
    if not (isint(sweeps) and sweeps >= 1):
        raise MatrixError(f'amg: sweeps must be an integer of at least 1, got {sweeps!r}')
    if B is not None:
        tensor = type(B).__module__.split('.')[0] == 'torch'
        if not tensor:
            try:
                B = numpy.asarray(B)
            except Exception:
                raise MatrixError(f'amg: nullspace must be an array of shape (n, k), got {type(B).__name__}') from None
        if str(B.dtype).split('.')[-1] != 'float64':
            raise MatrixError(f'amg: nullspace must be float64, got {B.dtype}')
        if B.ndim == 1:
            B = B.reshape(-1, 1)
        if B.ndim != 2 or (n is not None and B.shape[0] != n):
            raise MatrixError(f'amg: nullspace must have the shape (n, k) or (n,)' + ('' if n is None else f' with n = {n}') + f', got {tuple(B.shape)}')
        if not 1 <= B.shape[1] <= MAX_NULLSPACE:
            raise MatrixError(f'amg: nullspace must have between 1 and {MAX_NULLSPACE} vectors, got k = {B.shape[1]}')
        if not bool(_torch().isfinite(B).all() if tensor else numpy.isfinite(B).all()):
            raise MatrixError('amg: nullspace has non-finite entries')
    return int(coarse), int(sweeps), B


SMOOTHER_KEYS = 'smoother', 'degree', 'eigsteps', 'eigratio'


def split_smoother(preconargs):
    '''(rest, smoother): the smoother keys of `preconargs` taken out and validated, the others left for `check_args`.  smoother: None for 'jacobi' (the
    default), or dict(degree=2, eigsteps=10, eigratio=10.) for 'chebyshev' with the values given filled in.'''
    from .matrix import MatrixError
    rest = dict(preconargs or {})
    given = {key: rest.pop(key) for key in SMOOTHER_KEYS if key in rest}
    kind = given.pop('smoother', 'jacobi')
    if not (isinstance(kind, str) and kind in ('jacobi', 'chebyshev')):
        raise MatrixError(f"amg: smoother must be 'jacobi' or 'chebyshev', got {kind!r}")
    if kind == 'jacobi':
        if given:
            raise MatrixError(f"amg: {sorted(given)} are arguments of smoother='chebyshev'; the 'jacobi' smoother takes 'sweeps'")
        return rest, None
    isint = lambda v: isinstance(v, (int, numpy.integer)) and not isinstance(v, bool)
    degree, eigsteps, eigratio = given.get('degree', 2), given.get('eigsteps', 10), given.get('eigratio', 10.)
    if not (isint(degree) and 1 <= degree <= 8):
        raise MatrixError(f'amg: degree must be an integer between 1 and 8, got {degree!r}')
    if not (isint(eigsteps) and 1 <= eigsteps <= 64):
        raise MatrixError(f'amg: eigsteps must be an integer between 1 and 64, got {eigsteps!r}')
    if not (isinstance(eigratio, (int, float, numpy.integer, numpy.floating)) and not isinstance(eigratio, bool) and numpy.isfinite(eigratio) and eigratio > 1):
        raise MatrixError(f'amg: eigratio must be a finite number greater than 1, got {eigratio!r}')
    if rest.get('sweeps', 1) != 1 or isinstance(rest.get('sweeps', 1), bool):
        raise MatrixError("amg: sweeps counts the sweeps of the 'jacobi' smoother; with smoother='chebyshev' it is `degree` that says how much smoothing is done")
    return rest, dict(degree=int(degree), eigsteps=int(eigsteps), eigratio=float(eigratio))


def start_vector(n, device=None):
    '''the start vector of the Lanczos recurrence: the top 31 bits of the hash of `keys`, as a number in [-1, 1)'''
    return (keys(n, device) >> 32).to(_torch().float64) * 2. ** -30 - 1.


def chebyshev_coefficients(ub, lb, degree):
    '''the pairs (c1, c2) of the steps d = c1 d + c2 dinv (b - A x), x += d of the Chebyshev polynomial of the interval [lb, ub], as a flat host array of
    2 degree numbers: theta = (ub + lb) / 2, delta = (ub - lb) / 2, rho_0 = delta / theta, rho_k = 1 / (2 theta / delta - rho_(k-1)); step 0 has (0, 1 / theta),
    step k (rho_k rho_(k-1), 2 rho_k / delta)'''
    theta, delta = (ub + lb) / 2., (ub - lb) / 2.
    coef, rho = [0., 1. / theta], delta / theta
    for _ in range(1, degree):
        new = 1. / (2. * theta / delta - rho)
        coef += [new * rho, 2. * new / delta]
        rho = new
    return numpy.array(coef)


def lanczos_theta(out):
    '''(theta, steps): the largest eigenvalue of the tridiagonal matrix of the alpha_j, beta_(j+1) that nh_csr_lanczos left in `out` (a host array), and the number
    of steps it took; theta is nan when there is none'''
    steps = int(out[-1])
    if not steps:
        return numpy.nan, 0
    alpha, beta = out[0:2 * steps:2], out[1:2 * steps - 1:2]
    T = numpy.diag(alpha) + numpy.diag(beta, 1) + numpy.diag(beta, -1)
    return (float(numpy.linalg.eigvalsh(T)[-1]) if numpy.isfinite(T).all() else numpy.nan), steps


def rigid_body_modes(coords):
    '''The near-nullspace of linear elasticity from the node coordinates `coords` [nnodes x d], d = 2 or 3: a host array [nnodes d x d (d + 1) / 2] whose
    columns are the d translations and then the rotations ((-y, x) in 2-D; about the x, y and z axis in 3-D), in the dof layout of a vector field
    (`function.field`: dof = node d + component).'''
    coords = numpy.asarray(coords, dtype=float)
    if coords.ndim != 2 or coords.shape[1] not in (2, 3):
        raise _error()(f'rigid_body_modes: coords must have the shape (nnodes, 2) or (nnodes, 3), got {coords.shape}')
    nnodes, d = coords.shape
    B = numpy.zeros((nnodes, d, d * (d + 1) // 2))
    for c in range(d):
        B[:, c, c] = 1.
    if d == 2:
        B[:, 0, 2], B[:, 1, 2] = -coords[:, 1], coords[:, 0]
    else:
        for axis in range(3):  # e_axis x r
            p, q = (axis + 1) % 3, (axis + 2) % 3
            B[:, q, 3 + axis], B[:, p, 3 + axis] = coords[:, p], -coords[:, q]
    return B.reshape(nnodes * d, -1)


class Hierarchy:
    '''The numeric phase on the device: the values of every level from those of the finest (`values`, on the pattern of `levels[0]`), and the handle of the
    cycle.  `levels`: of `symbolic`, on device tensors.  Per level `self.data[l]` keeps what the cycle reads: values, dinv, and for a coarsened level rho,
    omega (0-dim device tensors), w = omega dinv, pvalues, rvalues; for a dense level ainv.  `nullspace`: the near-nullspace of level 0, a float64 device
    tensor [n x k], for levels of ``symbolic(..., nullspace=k)``; a coarsened level then keeps its own as B, the values of T as q [n x k], and hands the
    triangles of the aggregates' QR on as the B of the next.  `smoother`: None (Jacobi) or the dict of `split_smoother`; a coarsened level then also keeps the
    Lanczos estimate theta of the largest eigenvalue of D^-1 A_f with the steps it took (eigsteps), ub, lb (host numbers), the coefficients of its polynomial
    (coef: 2 degree doubles on the device) and the vector d of the recurrence.  The estimate costs one look at the device per level: 2 eigsteps + 1 doubles.
    `symmetric=False`: the matrix need not be symmetric (its pattern must be, structurally): the dense level's inverse is then the general pseudo-inverse, and
    a Chebyshev smoother, whose bound is a Lanczos estimate, is refused; every other step of the setup reads no symmetry.'''

    def __init__(self, levels, values, sweeps=1, nullspace=None, smoother=None, symmetric=True):
        from . import device, kernels
        from .matrix import MatrixError, spmv_lanes
        torch = _torch()
        self.levels, self.data = levels, []
        if smoother is not None and not symmetric:
            raise MatrixError("amg: smoother='chebyshev' takes its bound from a Lanczos estimate, which needs a symmetric matrix; with symmetric=False the smoother is 'jacobi'")
        descriptions = []
        B, nk = nullspace, levels[0].k
        if (nk is None) != (B is None) or (B is not None and tuple(B.shape) != (levels[0].n, nk)):
            raise MatrixError(f'amg: the levels were made for a near-nullspace of {nk} vectors, the one given has the shape {None if B is None else tuple(B.shape)}')
        for l, lv in enumerate(levels):
            d = Level()
            self.data.append(d)
            d.values, d.B = values, B
            lanes = spmv_lanes(lv.n, lv.colidx.numel())
            diag = kernels.csr_diagonal(values, lv.rowptr, lv.colidx, lv.n, col32=lv.col32)
            keep = torch.ones_like(diag, dtype=torch.bool) if lv.free is None else lv.free
            # (below level 0 of a hierarchy with a near-nullspace a zero diagonal entry is the coarse dof of a dropped column, a zero row and column: dinv = 0 there)
            if (nk is None or l == 0) and bool(((diag == 0) & keep).any()):
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
                # (a symmetric matrix takes the pseudo-inverse from its eigenvalues, as ever; that of a matrix that need not be comes from its singular values)
                d.ainv = device.to_dev(numpy.linalg.pinv(dense, hermitian=bool(symmetric)).ravel(), 'float64') if lv.nfree else None
                desc.update(kind='dense', ndense=lv.nfree, Ainv=d.ainv, idx=d.idx)
                break
            if lv.kind == 'diagonal':
                desc.update(kind='diagonal', w=d.dinv)
                break
            absrow = kernels.csr_spmv(values.abs(), lv.rowptr, lv.colidx, lv.n, keep.to(torch.float64), rowmask=lv.mask, col32=lv.col32, lanes=lanes)
            d.rho = (absrow * d.dinv).max()
            d.omega = 4. / (3. * d.rho)
            d.w = d.omega * d.dinv
            product = kernels.block_segment_dot if lv.setup == 'block' else kernels.segment_dot  # (the plans of a level are of one kind)
            if nk is None:
                d.atvalues = kernels.segment_dot(lv.at, values)
                d.pvalues = lv.tind - d.w[lv.prow] * d.atvalues
            else:
                d.q, B = kernels.aggregate_qr(lv.mptr, lv.midx, nk, B)
                flat = d.q.reshape(-1)
                d.atvalues = product(lv.at, values, flat)
                d.pvalues = flat[lv.tmap.clamp(min=0)].masked_fill(lv.tmap < 0, 0.) - d.w[lv.prow] * d.atvalues
            d.rvalues = d.pvalues[lv.rperm]
            d.apvalues = product(lv.ap, values, d.pvalues)
            d.t, d.r = device.empty(lv.n, 'float64'), device.empty(lv.n, 'float64')
            if smoother is not None:
                # PCIe: the alpha and beta of the recurrence and its step count visit the host, and so does rho, one number
                out = kernels.csr_lanczos(values, lv.rowptr, lv.colidx, lv.n, d.dinv.sqrt(), start_vector(lv.n, values.device), smoother['eigsteps'], rowmask=lv.mask,
                                          col32=lv.col32, lanes=lanes)
                d.theta, d.eigsteps = lanczos_theta(device.to_host(out))
                if not (d.theta > 0 and numpy.isfinite(d.theta)):
                    raise MatrixError('amg: matrix is not positive definite')
                d.ub = min(1.1 * d.theta, float(d.rho))  # (theta comes from below, rho is a true bound)
                d.lb = d.ub / smoother['eigratio']
                d.coef = device.to_dev(chebyshev_coefficients(d.ub, d.lb, smoother['degree']), 'float64')
                d.d = device.empty(lv.n, 'float64')
                desc.update(smoother='chebyshev', degree=smoother['degree'], coef=d.coef, d=d.d)
            desc.update(kind='coarsen', w=d.w if smoother is None else d.dinv, t=d.t, r=d.r, P=(d.pvalues, lv.prowptr, lv.pcol, lv.nc, lv.pcol32, 0), R=(d.rvalues, lv.rrowptr, lv.rcol, lv.n, lv.rcol32, 0))
            values = product(lv.rap, d.rvalues, d.apvalues)
        self.handle = kernels.Amg(descriptions)

    def apply(self, r, z=None):
        '''z = M r, one cycle (nh_amg_apply)'''
        return self.handle.apply(r, z)


class Schur:
    '''The block upper-triangular preconditioner of a saddle point K = [[A, Bt], [B, C]] on the device (``HipMatrix.getprecon('schur')``; nh_schur_*): `first`, the
    ``Hierarchy`` built on K itself with the first field's free dofs `mask1` as its row mask (no submatrix is formed), and `sinv`, 1 / shat on the second field's
    free dofs and 0 elsewhere, shat the diagonal approximation of the Schur complement.  z = M r is z2 = sinv r, t = mask1(r - K z2), z1 = cycle(t), z = z1 + z2 on
    full-length vectors; r is not read on held dofs and z is zero there.  `csr`: the matrix as (values, rowptr, colidx, ncols, col32, lanes).'''

    def __init__(self, first, csr, mask1, sinv):
        from . import kernels
        self.first, self.mask1, self.sinv = first, mask1, sinv
        self.handle = kernels.Schur(first.handle, csr, mask1, sinv)

    def apply(self, r, z=None):
        '''z = M r, one application (nh_schur_apply)'''
        return self.handle.apply(r, z)


class Preconditioner:
    '''What ``HipMatrix.getprecon`` returns (the reference's Matrix.getprecon, matrix/_base.py): a preconditioner built once, applied by `M(r)` and taken by
    ``HipMatrix.solve(precon=M)`` in place of a name, on the matrix it was built on or on any other of the same shape, pattern and free mask -- the next Newton
    step's, say.  `kind`: 'amg' (`hierarchy`: the ``Hierarchy``, whose handle, level values and scratch vectors live as long as this object), 'diag' (`dinv`:
    the inverse diagonal, 0 on constrained rows) or 'schur' (`schur`: the ``Schur`` operator of a saddle point, whose first block's hierarchy is also `hierarchy`);
    `shape`: of the matrix; `free`: the host bool mask of the free dofs it was built for; `mask`: the same on
    the device (None: all free); `values`: the value tensor it was built on; `symmetric`: whether the operator may precondition conjugate gradients.'''

    def __init__(self, kind, shape, free, symmetric, values, mask, *, hierarchy=None, dinv=None, schur=None):
        self.kind, self.shape, self.free, self.symmetric, self.values, self.mask = kind, tuple(shape), free, bool(symmetric), values, mask
        self.hierarchy, self.dinv, self.schur = hierarchy, dinv, schur

    def __repr__(self):
        return f'<{self.kind!r} preconditioner of a {self.shape[0]}x{self.shape[1]} HipMatrix, {int(self.free.sum())} free dofs, symmetric={self.symmetric}>'

    def __call__(self, r):
        '''z = M r, one application: a numpy vector gives a numpy vector, a float64 device tensor a device tensor.  'amg': one V-cycle (``Hierarchy.apply``) on r
        as it is given; 'diag': dinv r; 'schur': the block solve (``Schur.apply``).'''
        from . import device
        tensor = type(r).__module__.split('.')[0] == 'torch'
        if not tensor:
            r = numpy.asarray(r, dtype=float)
        if r.ndim != 1 or r.shape[0] != self.shape[0] or (tensor and str(r.dtype) != 'torch.float64'):
            raise _error()(f'a preconditioner of a {self.shape[0]}x{self.shape[1]} matrix takes a float64 vector of {self.shape[0]} entries, got {tuple(r.shape)} {r.dtype}')
        rdev = r.contiguous() if tensor else device.to_dev(r, 'float64')
        z = self.hierarchy.apply(rdev) if self.kind == 'amg' else self.schur.apply(rdev) if self.kind == 'schur' else self.dinv * rdev
        return z if tensor else device.to_host(z)
