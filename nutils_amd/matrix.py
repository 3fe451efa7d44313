'''Matrix hand-off (boundary C of the reference): the GPU-built CSR triplet goes
back to the host solver exactly the way the reference's evaluator hands it over
(/root/reference/src/nutils/matrix/__init__.py:20-151): ``assemble_csr(values,
rowptr, colidx, ncols)`` validates the triplet and calls
``backend.current.assemble``.  The validation is vectorised here (the reference
uses Python ``all()`` over numpy arrays); the error behaviour (MatrixError, same
conditions) is the reference's.

Two backends.  'scipy' (the default; 'auto' means the same) wraps the host copy
of the triplet in a ``ScipyMatrix`` with a direct solver.  'hip' keeps the
triplet in HBM as a ``HipMatrix``: products, the diagonal and four Jacobi-
preconditioned Krylov solves -- conjugate gradients ('cg') for symmetric
positive definite systems, MINRES ('minres') for symmetric indefinite ones,
BiCGStab ('bicgstab') and restarted GMRES ('fgmres') for any square matrix --
run on the device (nh_csr.hip), 'cg' and 'fgmres' also with a multigrid
cycle as preconditioner (``getprecon``: objects built once and used for
several solves); ``function.eval(function.as_matrix(K))`` builds
one without the triplet ever visiting the host, and so does ``solver.System``
under this backend (``assemble_device``).  The matrix algebra runs there too
(nh_csr_ops.hip): ``T``, ``submatrix`` by masks or strictly increasing indices,
and sums of matrices with different patterns.  Blocks of vectors have names of
their own: ``matmat`` multiplies with an (ncols, k) block and
``solve_columns`` solves for an (n, k) block of right-hand sides by batched
conjugate gradients (nh_csr_multi.hip), reading the matrix once per eight
columns.  What a ``HipMatrix`` does
through scipy and a re-upload -- every solver other than 'cg', 'minres',
'bicgstab' and 'fgmres', ``export``, ``submatrix`` by unordered or repeated
integer indices -- says so in its docstring.
'''

import contextlib
import weakref
import numpy


class MatrixError(Exception):
    '''General error message for matrix-related failure (matrix/_base.py:9-12).'''


class ToleranceNotReached(MatrixError):
    '''The iterative solver stopped above the requested tolerance (matrix/_base.py:22-30); ``.best`` is the vector it had reached,
    constrained values included.'''

    def __init__(self, best):
        super().__init__('solver failed to reach tolerance')
        self.best = best


class ScipyMatrix:
    '''scipy.sparse.csr_matrix wrapper with the subset of the reference's Matrix
    interface (matrix/_base.py, _scipy.py:11-12) that the assembly path touches.'''

    def __init__(self, core):
        self.core = core
        self.shape = core.shape

    def export(self, form):
        if form == 'csr':
            return self.core.data, self.core.indices, self.core.indptr
        if form == 'coo':
            coo = self.core.tocoo()
            return coo.data, (coo.row, coo.col)
        if form == 'dense':
            return self.core.toarray()
        raise NotImplementedError(f'cannot export ScipyMatrix to {form!r}')

    def __matmul__(self, other):
        return self.core @ other

    def submatrix(self, rows, cols):
        rows = numpy.asarray(rows)
        cols = numpy.asarray(cols)
        if rows.dtype == bool:
            rows, = rows.nonzero()
        if cols.dtype == bool:
            cols, = cols.nonzero()
        return ScipyMatrix(self.core[rows, :][:, cols])

    def solve(self, rhs=None, *, lhs0=None, constrain=None, **solverargs):
        '''Direct solve with constraints in the reference's convention: `constrain`
        is an array with NaN for free dofs (matrix/_base.py:100-190).'''
        import scipy.sparse.linalg
        n = self.shape[0]
        x = numpy.zeros(n) if lhs0 is None else numpy.array(lhs0, dtype=float)
        rhs = numpy.zeros(n) if rhs is None else numpy.asarray(rhs, dtype=float)
        if constrain is None:
            free = numpy.ones(n, dtype=bool)
        else:
            constrain = numpy.asarray(constrain)
            if constrain.dtype == bool:
                free = ~constrain.ravel()
            else:
                free = numpy.isnan(constrain)
                x[~free] = constrain[~free]
        if free.all():
            return x + scipy.sparse.linalg.spsolve(self.core.tocsc(), rhs - self.core @ x)
        b = (rhs - self.core @ x)[free]
        A = self.core[free, :][:, free].tocsc()
        x[free] += scipy.sparse.linalg.spsolve(A, b)
        return x


class _ScipyBackend:
    @staticmethod
    def assemble(values, rowptr, colidx, ncols):
        import scipy.sparse
        return ScipyMatrix(scipy.sparse.csr_matrix((values, colidx, rowptr), (len(rowptr) - 1, ncols)))

    @staticmethod
    def assemble_trusted(values, rowptr, colidx, ncols):
        '''Same matrix for an index pair that has been through `assemble_csr` before (re-assembly of a Newton step: only the values
        are new): skips scipy's O(nnz) index scans and the copy it makes of the index arrays.'''
        import scipy.sparse
        core = scipy.sparse.csr_matrix((len(rowptr) - 1, ncols), dtype=values.dtype)
        core.data, core.indices, core.indptr = values, colidx, rowptr
        core.has_sorted_indices = True
        core.has_canonical_format = True
        return ScipyMatrix(core)


def spmv_lanes(nrows, nnz):
    '''Lanes of a wave that share a row in the device product: two thirds of the mean row length rounded down to a power of two, between 1 and 32
    (the rule of nh_csr_lanes; profiles/matrix_backend.md has the sweep it comes from: 4 lanes were fastest for 9 entries per row, 16 for 27, 32 for 81 and
    for P2 vector rows of 185 on average).  The kernel itself takes any power of two up to 64.  Rows shorter than the lane count leave lanes idle, longer ones
    are walked in strides.'''
    nrows, nnz = int(nrows), int(nnz)
    if nrows <= 0 or nnz <= 0:
        return 1
    target = 2 * nnz // (3 * nrows)
    lanes = 1
    while lanes < 32 and 2 * lanes <= target:
        lanes *= 2
    return lanes


def constraints(ncols, constrain=None, lhs0=None):
    '''(free, lhs) of a constrained solve in the reference's convention (matrix/_base.py:100-176): `constrain` is None (all dofs free), a float array
    in which NaN marks a free dof and a number the value the dof is held at, or a bool array in which True holds the dof at its value in `lhs0`
    (zero without one).  `free` is a bool vector, `lhs` a fresh float vector: `lhs0` with the constrained values written in.'''
    ncols = int(ncols)
    if lhs0 is None:
        lhs = numpy.zeros(ncols)
    else:
        lhs = numpy.array(lhs0, dtype=float)
        if lhs.shape != (ncols,):
            raise MatrixError(f'initial vector has shape {lhs.shape}, expected ({ncols},)')
    if constrain is None:
        return numpy.ones(ncols, dtype=bool), lhs
    constrain = numpy.asarray(constrain)
    if constrain.shape != (ncols,):
        raise MatrixError(f'constraints have shape {constrain.shape}, expected ({ncols},)')
    if constrain.dtype == bool:
        return ~constrain, lhs
    if constrain.dtype.kind not in 'fiu':
        raise MatrixError(f'constraints must be a float or bool array, got {constrain.dtype}')
    constrain = constrain.astype(float)
    free = numpy.isnan(constrain)
    lhs[~free] = constrain[~free]
    return free, lhs


def _is_tensor(a):
    return type(a).__module__.split('.')[0] == 'torch'


def _host(a):
    if a is None or not _is_tensor(a):
        return a
    from . import device
    return device.to_host(a)


def _row_major(t):
    '''a 2-D device tensor as a block of vectors: itself if its columns are one double apart and its rows do not overlap, else a contiguous copy'''
    return t if t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]) else t.contiguous()


def _selector(sel, n, what):
    '''A selector of `submatrix` as a bool mask of length n: a bool array, or integers that rise strictly (numeric.asboolean of the reference, numeric.py:494).
    None for any other integer array in range (unordered, repeated, negative indices): those keep the host path.  Raises MatrixError for a wrong length, an
    index out of range, more than one axis or a dtype that is neither bool nor integer.  Host arrays only: nothing is uploaded here.'''
    sel = numpy.asarray(sel)
    if sel.ndim != 1:
        raise MatrixError(f'{what} selection must be a vector, got {sel.ndim} axes')
    if sel.dtype == bool:
        if len(sel) != n:
            raise MatrixError(f'{what} mask has length {len(sel)}, expected {n}')
        return sel
    if not sel.size:
        return numpy.zeros(n, dtype=bool)
    if sel.dtype.kind not in 'iu':
        raise MatrixError(f'{what} selection must be a bool mask or an integer array, got {sel.dtype}')
    if int(sel.max()) >= n or int(sel.min()) < -n:
        raise MatrixError(f'{what} index out of range for {n} {what}s')
    if int(sel.min()) < 0 or (sel.size > 1 and not (sel[1:] > sel[:-1]).all()):
        return None
    mask = numpy.zeros(n, dtype=bool)
    mask[sel] = True
    return mask


class _Plan:
    '''The index side of a transpose or a submatrix: the result's (rowptr, colidx), its column count, and `pos`, where each of its entries lies in the operand.
    `apply(values)` is the matrix for the operand's current values: one gather.  The plan remembers the last matrix it made, weakly: while that one lives the
    next is made from it by `_with_values`, so its int32 columns, its AMG symbolic phase and its own plans carry over in turn.'''

    def __init__(self, key, rowptr, colidx, pos, ncols):
        self.key, self.rowptr, self.colidx, self.pos, self.ncols = key, rowptr, colidx, pos, ncols
        self._last = None

    def apply(self, values):
        from . import kernels
        values = kernels.csr_gather(values, self.pos)
        last = self._last and self._last()
        new = HipMatrix(values, self.rowptr, self.colidx, self.ncols) if last is None else last._with_values(values)
        self._last = weakref.ref(new)
        return new


class HipMatrix:
    '''CSR matrix that lives in HBM, with the interface of the reference's Matrix (matrix/_base.py): `shape`, `size`, `@`, `diagonal`, `export`, scalar
    multiples, sums, `submatrix`, `T`, `solve`, `solve_leniently`.

    `values` (f64), `rowptr`, `colidx` (int64) are device tensors as `_MatrixPlan.run` returns them, or host arrays, which are validated and uploaded at the
    first use on the device.  The matrix keeps references and never writes into them.  At the first product the column indices are narrowed to int32 once
    (12 instead of 16 bytes per entry; matrices with more than 2^31 - 1 columns keep the int64 indices).

    On the device: products (nh_csr_spmv), the diagonal, `rowsupp` / `colsupp` (nh_csr_support), scalar multiples, sums (of matrices that share their index tensors: values only, zeros kept; of different
    patterns: the union by nh_pattern_union_*, the values by nh_csr_add_values, the entries that cancel exactly dropped as scipy drops them, by nh_csr_select_*), `T`
    (nh_csr_transpose) and `submatrix` by bool masks or strictly increasing indices (nh_csr_select_*) -- the index side of a transpose or a submatrix is a plan kept on
    the matrix and handed on by `_with_values`, so the next matrix on the same pattern pays one gather (nh_index_copy) -- `solve(solver='cg')`, a
    conjugate-gradient iteration for SYMMETRIC POSITIVE DEFINITE systems preconditioned by Jacobi or by a smoothed-aggregation multigrid cycle (`precon='amg'`, amg.py), for SYMMETRIC systems that are indefinite (saddle points, Helmholtz) `solve(solver='minres')`, a MINRES iteration
    preconditioned by 1 / |diag|: one product a step, a residual that never rises in the norm it minimises, no breakdown short of the exhausted Krylov space;
    and for ANY square system (nonsymmetric, indefinite)
    `solve(solver='bicgstab')`, a Jacobi-preconditioned BiCGStab iteration, and `solve(solver='fgmres')`, Jacobi-preconditioned restarted GMRES, whose residual
    norm never rises within a cycle; all with ONE right-hand side per `solve`.  A block of vectors goes through names of its own, since `@` and `solve` refuse
    2-D arguments: `matmat(X)` multiplies with an (ncols, k) block and `solve_columns(rhs)` solves for an (n, k) block of right-hand sides by k conjugate-gradient
    recurrences (Jacobi or none) that share every pass over the matrix (nh_csr_spmm, nh_cgm_*: the values and column indices are read once per eight columns).
    `iterations` is the iteration count of the last device solve, `column_iterations` the per-column counts of the last `solve_columns`.  Through scipy and PCIe (export, host operation, re-upload): every other solver, `submatrix` by
    integer indices that are not strictly increasing, and the algebra of a matrix made from host arrays in which a row repeats a column.'''

    def __init__(self, values, rowptr, colidx, ncols, *, validate=True):
        self._ncols = int(ncols)
        if _is_tensor(values):
            self._dev = (values, rowptr, colidx)
            self._hostcsr = None
            nrows, nnz = rowptr.numel() - 1, values.numel()
        else:
            values, rowptr, colidx = numpy.asarray(values, dtype=float), numpy.asarray(rowptr), numpy.asarray(colidx)
            if validate:  # (the product trusts the column indices)
                _check_triplet(values, rowptr, colidx, self._ncols)
            self._dev = None
            self._hostcsr = (values, rowptr, colidx)
            nrows, nnz = len(rowptr) - 1, len(values)
        self.shape = (nrows, self._ncols)
        self.nnz = nnz
        self.lanes = spmv_lanes(nrows, nnz)
        self.cg_iterations = None
        self.iterations = None
        self.column_iterations = None  # of the last `solve_columns`: the iterations that moved each column
        self._col32 = None
        self._canonical = True if self._hostcsr is None else None  # (`_unique`: None until a host triplet has been looked at)
        self._amg = None  # (free mask, coarse, k, levels, setup) of the last 'amg' setup: the symbolic phase, reused while pattern and mask stay
        self._tplan = None  # the index side of `T` (_Plan), made at the first transpose
        self._subplan = None  # the index side of the last `submatrix` (_Plan; its key: the two masks)

    @property
    def size(self):
        return self.shape[0] * self.shape[1]

    # -- device side

    def triplet(self):
        '''(values, rowptr, colidx) as device tensors'''
        if self._dev is None:
            from . import device
            values, rowptr, colidx = self._hostcsr
            self._dev = device.to_dev(values, 'float64'), device.to_dev(rowptr, 'int64'), device.to_dev(colidx, 'int64')
        return self._dev

    def _columns(self):
        '''the int32 column indices, made at the first product; None for matrices too wide for them'''
        if self._col32 is None and self._ncols <= 0x7fffffff and self.nnz:
            from . import kernels
            self._col32 = kernels.csr_compact(self.triplet()[2], self._ncols)
        return self._col32

    def _with_values(self, values):
        '''a matrix on the same index tensors (and their int32 copy, the symbolic phase of an 'amg' preconditioner with the mask it was made for, and the plans of
        its transpose and of its last submatrix)'''
        _, rowptr, colidx = self.triplet()
        new = HipMatrix(values, rowptr, colidx, self._ncols)
        new._col32 = self._col32
        new._canonical = self._unique()
        new._amg = self._amg
        new._tplan = self._tplan
        new._subplan = self._subplan
        return new

    def _unique(self):
        '''whether no row repeats a column, which the algebra on the device takes for granted.  True of what the assembly leaves in HBM; host arrays, whose
        validation lets equal neighbours pass as the reference's does, are looked at once.'''
        if self._canonical is None:
            self._canonical = True
            if self._hostcsr is not None:
                _, rowptr, colidx = self._hostcsr
                same = numpy.flatnonzero(colidx[1:] == colidx[:-1]) + 1  # allowed only where a new row starts
                self._canonical = not (same.size and not numpy.isin(same, rowptr).all())
        return self._canonical

    def spmv(self, x, *, alpha=1., beta=0., b=None, rowmask=None, y=None, lanes=None):
        '''y = mask(alpha A x + beta b) on device tensors (nh_csr_spmv); `b` may be `y`'''
        from . import kernels
        values, rowptr, colidx = self.triplet()
        return kernels.csr_spmv(values, rowptr, colidx, self._ncols, x, y=y, alpha=alpha, beta=beta, b=b, rowmask=rowmask, col32=self._columns(),
                                lanes=self.lanes if lanes is None else lanes)

    def __matmul__(self, other):
        '''A @ x for one vector: a numpy vector gives a numpy vector, a device tensor a device tensor'''
        on_device = _is_tensor(other)
        if not on_device:
            other = numpy.asarray(other, dtype=float)
        if other.ndim != 1 or other.shape[0] != self.shape[1]:
            raise MatrixError(f'cannot multiply a {self.shape[0]}x{self.shape[1]} matrix with an array of shape {tuple(other.shape)}')
        from . import device
        y = self.spmv(other.contiguous() if on_device else device.to_dev(other, 'float64'))
        return y if on_device else device.to_host(y)

    def spmm(self, X, *, alpha=1., beta=0., B=None, rowmask=None, Y=None, lanes=None):
        '''Y = mask(alpha A X + beta B) on blocks of vectors, the device-level twin of `spmv` (nh_csr_spmm): 2-D float64 device tensors with unit column stride and
        any row stride, so a column slice of a wider tensor will do; `B` may be `Y`.  Column j is, bit for bit, `spmv` of column j.'''
        from . import kernels
        values, rowptr, colidx = self.triplet()
        return kernels.csr_spmm(values, rowptr, colidx, self._ncols, X, Y=Y, alpha=alpha, beta=beta, B=B, rowmask=rowmask, col32=self._columns(),
                                lanes=self.lanes if lanes is None else lanes)

    def _block_argument(self, X, nrows, what):
        '''a block of columns as the caller gave it, checked before anything is uploaded: (on_device, X) with X a float host array or a float64 device tensor of
        shape (nrows, k), k >= 1'''
        on_device = _is_tensor(X)
        if X is None:
            raise MatrixError(f'{what} is missing: a block of shape ({nrows}, k) is needed, the number of columns has to come from somewhere')
        if not on_device:
            X = numpy.asarray(X, dtype=float)
        if X.ndim != 2 or X.shape[1] < 1:
            raise MatrixError(f'{what} has shape {tuple(X.shape)}, expected ({nrows}, k) with k >= 1: a block of columns (one vector goes to `solve` or `@`)')
        if X.shape[0] != nrows:
            raise MatrixError(f'{what} shape {tuple(X.shape)} does not match matrix shape {self.shape[0]}x{self.shape[1]}')
        if on_device and 'float64' not in str(X.dtype):
            raise MatrixError(f'{what} must be a float64 tensor, got {X.dtype}')
        return on_device, X

    def matmat(self, X):
        '''A @ X for a block X of shape (ncols, k), k >= 1 (the reference's Matrix.__matmul__ with a 2-D array; `@` itself takes one vector): the matrix is read
        once per eight columns instead of once per column.  A numpy array gives a numpy array, a device tensor a device tensor.  A wrong shape or rank is a
        MatrixError before anything is uploaded.'''
        from . import device
        on_device, X = self._block_argument(X, self.shape[1], 'the right operand')
        Y = self.spmm(_row_major(X) if on_device else device.to_dev(X, 'float64'))
        return Y if on_device else device.to_host(Y)

    def _diagonal_dev(self):
        from . import kernels
        if self.shape[0] != self.shape[1]:
            raise MatrixError('failed to extract diagonal: matrix is not square')
        values, rowptr, colidx = self.triplet()
        return kernels.csr_diagonal(values, rowptr, colidx, self._ncols, col32=self._col32)

    def diagonal(self):
        '''A_ii as a host vector, 0 where a row has no diagonal entry (Matrix.diagonal)'''
        from . import device
        return device.to_host(self._diagonal_dev())

    def _support(self, tol, rows):
        from . import device, kernels
        tol = float(tol)
        if not tol >= 0:
            raise MatrixError(f'the tolerance of a support must not be negative, got {tol}')
        values, rowptr, colidx = self.triplet()
        supp = kernels.csr_support(values, rowptr, colidx, self._ncols, tol, rows=rows, cols=not rows, col32=self._columns(), lanes=self.lanes)[0 if rows else 1]
        return device.to_host(supp).astype(bool)

    def rowsupp(self, tol=0):
        '''host bool vector: the rows that hold an entry with |a| > tol (Matrix.rowsupp, matrix/_base.py:92-98), found on the device (nh_csr_support)'''
        return self._support(tol, True)

    def colsupp(self, tol=0):
        '''host bool vector: the columns that hold an entry with |a| > tol (nh_csr_support); what `System.solve_constraints` asks of its matrix'''
        return self._support(tol, False)

    # -- host side (PCIe)

    def export(self, form):
        '''host arrays: 'csr' (data, indices, indptr), 'coo' (data, (row, col)), 'dense'.  Copies the triplet over PCIe.'''
        if form not in ('csr', 'coo', 'dense'):
            raise NotImplementedError(f'cannot export HipMatrix to {form!r}')
        if self._hostcsr is None:
            from . import device
            self._hostcsr = tuple(device.to_host(a) for a in self.triplet())  # (kept: the matrix is immutable)
        values, rowptr, colidx = self._hostcsr
        if form == 'csr':
            return values, colidx, rowptr
        if form == 'coo':
            return values, (numpy.repeat(numpy.arange(self.shape[0], dtype=numpy.int64), numpy.diff(rowptr)), colidx)
        return self._scipy().export('dense')

    def _scipy(self):
        data, indices, indptr = self.export('csr')
        return _ScipyBackend.assemble(data, indptr, indices, self._ncols)

    @staticmethod
    def _from_scipy(core):
        core = core.tocsr()
        core.sum_duplicates()
        core.sort_indices()
        return HipMatrix(core.data, core.indptr.astype(numpy.int64), core.indices.astype(numpy.int64), core.shape[1])

    def _submatrix_host(self, rows, cols):
        '''PCIe path: selected on the host by scipy and uploaded again'''
        return self._from_scipy(self._scipy().submatrix(rows, cols).core)

    def _transpose_host(self):
        '''PCIe path: transposed on the host by scipy and uploaded again'''
        return self._from_scipy(self._scipy().core.T)

    def _add_host(self, other, sign):
        '''PCIe path: different patterns are merged on the host by scipy and the sum is uploaded'''
        return self._from_scipy(self._scipy().core + sign * other._scipy().core)

    # -- algebra: new index tensors, made on the device (nh_csr_ops.hip)

    def submatrix(self, rows, cols):
        '''The rows and columns selected by bool masks or by strictly increasing integer arrays (Matrix.submatrix with the reference's numeric.asboolean), made
        on the device (nh_csr_select_*); stored zeros stay.  The selectors are checked on the host before anything is uploaded: a wrong length, an index out of
        range or a dtype that is neither bool nor integer is a MatrixError.  All rows and all columns: the matrix itself.  The index side is kept (`_subplan`,
        one entry, keyed by the two masks), so the same selection of the next matrix on these index tensors is one gather.  Integer arrays that are not strictly
        increasing (unordered, repeated, negative) take the PCIe path: selected on the host by scipy and uploaded again.  A constrained `solve(solver='cg')` does
        not come here: it masks rows instead.'''
        rmask, cmask = _selector(rows, self.shape[0], 'row'), _selector(cols, self.shape[1], 'column')
        if rmask is not None and cmask is not None and rmask.all() and cmask.all():
            return self
        if rmask is None or cmask is None or not self._unique():
            return self._submatrix_host(rows, cols)
        plan = self._subplan
        if plan is None or not (numpy.array_equal(plan.key[0], rmask) and numpy.array_equal(plan.key[1], cmask)):
            from . import device, kernels
            values, rowptr, colidx = self.triplet()
            rowptr_s, colidx_s, pos = kernels.csr_select(values, rowptr, colidx, self._ncols, rowkeep=None if rmask.all() else device.to_dev(rmask, 'uint8'),
                                                         colkeep=None if cmask.all() else device.to_dev(cmask, 'uint8'), nrows_s=int(rmask.sum()),
                                                         ncols_s=int(cmask.sum()), col32=self._col32, lanes=self.lanes)
            plan = self._subplan = _Plan((rmask.copy(), cmask.copy()), rowptr_s, colidx_s, pos, int(cmask.sum()))
        return plan.apply(self.triplet()[0])

    @property
    def T(self):
        '''the transpose, made on the device (nh_csr_transpose); the index side is kept (`_tplan`), so the transpose of the next matrix on these index tensors is
        one gather'''
        if not self._unique():
            return self._transpose_host()
        if self._tplan is None:
            from . import kernels
            _, rowptr, colidx = self.triplet()
            self._tplan = _Plan(None, *kernels.csr_transpose(rowptr, colidx, self._ncols, col32=self._col32), self.shape[0])
        return self._tplan.apply(self.triplet()[0])

    # -- algebra: new values, shared indices

    def __mul__(self, other):
        if not numpy.isscalar(other):
            return NotImplemented
        return self._with_values(self.triplet()[0] * float(other))

    __rmul__ = __mul__

    def __truediv__(self, other):
        return self.__mul__(1 / other)

    def __neg__(self):
        return self.__mul__(-1.)

    def __add__(self, other, sign=1.):
        if not isinstance(other, HipMatrix):
            return NotImplemented
        if self.shape != other.shape:
            raise MatrixError(f'cannot add a {other.shape[0]}x{other.shape[1]} matrix to a {self.shape[0]}x{self.shape[1]} matrix')
        a, b = self.triplet(), other.triplet()
        if a[1] is b[1] and a[2] is b[2]:  # one pattern (scalar multiples, re-assemblies on the plan's index tensors): values only, on the device
            return self._with_values(a[0] + b[0] if sign > 0 else a[0] - b[0])
        if not (self._unique() and other._unique()):
            return self._add_host(other, sign)
        # different patterns: their union (nh_pattern_union_*), the values a + sign b written into it (nh_csr_add_values), and the entries that cancelled exactly
        # dropped as scipy's sparse sum drops them (nh_csr_select_*; NaN stays).  No plan: the pattern of a sum depends on the values.
        from . import kernels
        rowptr, colidx, (pa, pb) = kernels.pattern_union([a[1:], b[1:]])
        values = kernels.csr_add(a[0], pa, b[0], pb, sign, colidx.numel())
        pruned = kernels.csr_select(values, rowptr, colidx, self._ncols, drop_zeros=True, lanes=spmv_lanes(self.shape[0], colidx.numel()), lazy=True)
        if pruned is not None:  # (None: nothing cancelled, the union is the result)
            rowptr, colidx, pos = pruned
            values = kernels.csr_gather(values, pos)
        return HipMatrix(values, rowptr, colidx, self._ncols)

    def __sub__(self, other):
        return self.__add__(other, sign=-1.)

    # -- solve

    def solve(self, rhs=None, *, lhs0=None, constrain=None, solver='cg', atol=0., rtol=0., precon='diag', maxiter=None, check=16, restart=30, preconargs=None, **solverargs):
        '''Solve A x = rhs with constraints in the reference's convention (`constraints`; Matrix.solve, matrix/_base.py:100-176).

        solver='cg': conjugate gradients on the device for a SYMMETRIC POSITIVE DEFINITE matrix and ONE right-hand side.  No submatrix is formed: the free
        dofs are a row mask, the residual mask(rhs - A lhs) is one masked product, and since residual and search direction vanish on the constrained dofs the
        product ignores constrained columns by itself -- the iteration is that of the reference's submatrix(free, free).  It stops when the recurrence has
        |r| <= max(atol, rtol |r0|), and the iterations enqueued after that one do nothing; the true residual is then recomputed, and the iteration restarts from
        it should rounding have left it above the bound.
        An iterative solve has no "machine precision" mode: atol = rtol = 0 is an error, not a request for it.  `precon`: 'diag' (Jacobi), None, or -- for this
        solver alone -- 'amg': a smoothed-aggregation multigrid V-cycle (the `amg` module has the algorithm), `preconargs=dict(coarse=256, sweeps=1)`: the
        coarsest level has at most `coarse` (1 .. 1024) dofs and is solved densely, its matrix the only thing that visits the host; `sweeps` Jacobi sweeps before
        and after each coarse correction.  The near-nullspace is the constant unless `preconargs` has `nullspace=B`: a float64 host array or device tensor of
        shape (n, k), or (n,) for k = 1, with 1 <= k <= 6 finite vectors that the smoother reduces slowly -- for elasticity the rigid-body modes
        (`amg.rigid_body_modes(coords)`), without which a vector problem gets a valid preconditioner, not an optimal one.  Rows of constrained dofs are ignored;
        a host array crosses PCIe once per solve, as n k doubles.  The symbolic phase runs once per pattern, mask, `coarse`, k and `setup` and is handed on by
        `_with_values`.  With a near-nullspace `preconargs` may name how the sparse products of the setup are planned: `setup='entry'` (one int32 pair per scalar
        product; a plan of 2^31 products or more is a MatrixError) or `setup='block'` (one per product of k x k blocks, k to k^3 times fewer: what the large vector
        problems need); without `setup` it is 'entry' unless a plan outgrows its indices, and then 'block' for the whole hierarchy.
        `preconargs` may name the smoother: `smoother='jacobi'` (the default: the `sweeps` above) or `smoother='chebyshev'` with
        `degree=2` (1 .. 8: the steps of the polynomial before and after each coarse correction, a cycle costing what `sweeps=degree` costs), `eigsteps=10`
        (1 .. 64: the Lanczos steps that estimate the largest eigenvalue of D^-1 A on every level, run on the device at each numeric setup) and
        `eigratio=10.` (> 1: the polynomial damps the eigenvalues between the upper bound and its `eigratio`-th part).  `sweeps` other than 1 with 'chebyshev',
        or one of these three keys with 'jacobi', is an error.
        `maxiter` defaults to the number of free dofs; `check`: iterations enqueued between two looks at the device's residual norm and breakdown flag (one
        16-byte copy).  Raises ToleranceNotReached(best) when the bound is not met, MatrixError when the matrix turns out not to be positive definite.

        solver='bicgstab': right-preconditioned BiCGStab on the device for ANY square matrix and ONE right-hand side, with the keywords, the row mask, the
        stopping rule and the true-residual restart of 'cg'.  The iteration stops itself on the device, so `iterations` is exact whatever `check` is.  A
        breakdown of the recurrence (a vanishing rhat . r, rhat . v, t . t or omega) after progress restarts it from the true residual with a fresh shadow
        residual, the iterations counting on; a breakdown at the first step after a start raises MatrixError('bicgstab: breakdown').

        solver='fgmres': right-preconditioned restarted GMRES on the device for ANY square matrix and ONE right-hand side (with the fixed Jacobi preconditioner
        flexible and right-preconditioned GMRES are the same iteration; the reference's name for it is matrix/_mkl.py's), with the keywords, the row mask and
        the bound of 'cg'.  A cycle starts from the true residual, takes up to `restart` Arnoldi steps (a keyword of this solver alone, the others ignore it; an integer of at least 1, clipped to the number of
        free dofs; one product and two passes of classical Gram-Schmidt each) and ends with x += M^-1 V y; its residual norm, which the device knows from the
        rotated right-hand side, never rises.  The cycle stops itself on the device, so `iterations`, the Arnoldi steps over all cycles, is exact whatever
        `check` is, and `maxiter` counts the same.  When a new direction vanishes or is not finite the cycle ends there; if the true residual is then above the
        bound without having fallen in that cycle (or in the
        one after it, which may get a direction of the size of a rounding and no further) the solve raises MatrixError('fgmres: singular matrix').

        `precon` may also be an object that `getprecon` has built: `M = A.getprecon('amg', constrain=cons, symmetric=False)`, `A.solve(rhs, constrain=cons,
        solver='fgmres', precon=M)`.  The object must have the shape of the matrix and the free mask of the solve (MatrixError otherwise, before any device work);
        the values may differ: a preconditioner built on another matrix of the same pattern -- last step's Jacobian -- is the intended use, and a second solve
        with it repeats no setup.  `preconargs` beside an object is a MatrixError.  A 'diag' object goes wherever precon='diag' goes, with the same bytes; an 'amg'
        object goes to 'cg' if it was built with symmetric=True (the bytes of precon='amg') and to 'fgmres' always; 'bicgstab' and 'minres' refuse it.  With an
        'amg' object 'fgmres' is flexible GMRES (nh_fgmres_iterate): step j keeps Z_j = M v_j, what the V-cycle returned, and the cycle ends with x += Z y, which
        is right whatever the cycle is -- not symmetric, not convergent on its own, built from other values.  That is `restart` more vectors of n doubles on the
        device, 2 restart + 1 in all; a step is ten launches and a V-cycle, and a look enqueues no more steps than the cycle has left, since a step past a stop
        would still run its V-cycle.  A 'schur' object (`getprecon`: the block preconditioner of a saddle point, which has no usable 'diag' or 'amg') goes to
        'fgmres' alone, by the same flexible iteration with the block solve in place of the cycle (nh_fgmres_iterate_schur); 'cg', 'bicgstab' and 'minres'
        refuse it as they refuse an 'amg' object built with symmetric=False.  Anything that is neither 'diag', 'amg', None nor such an object is an invalid preconditioner: Python callables are not
        accepted, a host callback per step would undo the enqueued loop.

        solver='minres': MINRES of Paige and Saunders on the device for a SYMMETRIC matrix, definite or not, and ONE right-hand side, with the keywords, the row
        mask, the stopping rule and the true-residual restart of 'cg'.  One product and three launches an iteration, a three-term recurrence on a fixed handful
        of vectors.  `precon='diag'` is M^-1 = 1 / |A_ii| (MINRES needs a positive definite preconditioner; a zero on the diagonal of a free row is the
        MatrixError of the others: a saddle point with a zero block takes `precon=None`); 'amg' and `preconargs` are refused.  With a preconditioner the
        iteration minimises the residual in the M^-1-norm; the 2-norm residual that the bound is about is carried beside it.  The iteration stops itself on
        the device, so `iterations` is exact whatever `check` is.  The only failures of the recurrence are a scalar that is not finite and a rotation that
        vanishes (the zero matrix): after progress the recurrence restarts from the true residual, at the first step after a start that is
        MatrixError('minres: breakdown').  The matrix is NOT checked for symmetry: on a nonsymmetric matrix the recurrence converges to something the true
        residual rejects, the restarts get nowhere, and the solve ends in ToleranceNotReached, not in a wrong answer.

        Any other `solver` is a PCIe path: the matrix is exported to a ScipyMatrix and solved there.

        Returns a numpy vector, or a device tensor if `rhs` was one.'''
        nrows, ncols = self.shape
        on_device = _is_tensor(rhs)
        if rhs is not None:
            if not on_device:
                rhs = numpy.asarray(rhs, dtype=float)
            if rhs.ndim != 1:
                raise MatrixError(f'right-hand side has {rhs.ndim} axes: HipMatrix solves for one vector at a time')
            if rhs.shape[0] != nrows:
                raise MatrixError('right-hand side shape does not match matrix shape')
        if nrows != ncols:
            raise MatrixError(f'constrained matrix is not square: {nrows}x{ncols}')
        if solver not in ('cg', 'minres', 'bicgstab', 'fgmres'):
            x = self._scipy().solve(_host(rhs), lhs0=_host(lhs0), constrain=_host(constrain), **solverargs)
            if on_device:
                from . import device
                x = device.to_dev(x, 'float64')
            return x
        if not (atol > 0 or rtol > 0):
            raise MatrixError(f"solver {solver!r} needs a tolerance: pass atol or rtol (an iterative solve has no machine-precision mode)")
        from . import amg
        ready = isinstance(precon, amg.Preconditioner)  # (built by `getprecon`: everything about it is checked here and below, before any device work)
        if ready:
            if preconargs is not None:
                raise MatrixError('preconargs are the arguments of a preconditioner that `solve` builds; one that `getprecon` has built took them there')
            if precon.shape != self.shape:
                raise MatrixError(f'the preconditioner was built for a {precon.shape[0]}x{precon.shape[1]} matrix, this one is {nrows}x{ncols}')
            if precon.kind in ('amg', 'schur') and solver in ('bicgstab', 'minres'):
                raise MatrixError(f"HipMatrix solver {solver!r} takes a 'diag' preconditioner or None; an 'amg' preconditioner goes to 'fgmres' (any matrix) or, built with symmetric=True, to 'cg'")
            if solver == 'cg' and not precon.symmetric:
                raise MatrixError("solver 'cg' needs a symmetric preconditioner, this one was built with symmetric=False: it goes to 'fgmres'")
        elif precon == 'amg' and solver == 'cg':
            preconargs, setup = amg.split_setup(preconargs)
            preconargs, smoother = amg.split_smoother(preconargs)
            preconargs = amg.check_args(preconargs, ncols) + (smoother, setup)
        elif precon not in ('diag', None):
            raise MatrixError(f"invalid preconditioner {precon!r} for HipMatrix solver {solver!r}: 'diag' or None" + (", or 'amg'" if solver == 'cg' else ''))
        elif preconargs is not None:
            raise MatrixError(f"preconargs are the arguments of precon='amg'; the preconditioner {precon!r} takes none")
        if solver == 'fgmres' and not (isinstance(restart, (int, numpy.integer)) and not isinstance(restart, bool) and restart >= 1):
            raise MatrixError(f'fgmres: restart must be an integer of at least 1, got {restart!r}')
        free, lhs = constraints(ncols, _host(constrain), _host(lhs0))
        if ready and not numpy.array_equal(precon.free, free):
            raise MatrixError(f'the preconditioner was built for another set of free dofs ({int(precon.free.sum())} of them; this solve has {int(free.sum())}): build it with the constraints of the solve')
        from . import krylov
        maxiter, check = int(free.sum()) if maxiter is None else int(maxiter), max(1, int(check))
        args = self, rhs, free, lhs, precon, on_device
        rec = (krylov.Cg(*args, preconargs) if solver == 'cg' else krylov.Fgmres(*args, int(restart)) if solver == 'fgmres'
               else krylov.Bicgstab(*args) if solver == 'bicgstab' else krylov.Minres(*args))
        try:
            return krylov.solve(rec, atol, rtol, maxiter, check)
        finally:
            self.iterations = rec.iterations
            if solver == 'cg':
                self.cg_iterations = rec.iterations

    def solve_leniently(self, *args, **kwargs):
        '''`solve` that returns the vector reached instead of raising ToleranceNotReached'''
        try:
            return self.solve(*args, **kwargs)
        except ToleranceNotReached as e:
            import warnings
            warnings.warn(str(e))
            return e.best

    def solve_columns(self, rhs, *, lhs0=None, constrain=None, solver='cg', atol=0., rtol=0., precon='diag', maxiter=None, check=16, preconargs=None):
        '''Solve A X = rhs for a block of right-hand sides, rhs of shape (n, k) with k >= 1 (the reference's Matrix.solve with trailing axes, matrix/_base.py:100-224;
        `solve` itself takes one vector): several load cases on one matrix, solved by k independent conjugate-gradient recurrences that share every pass over
        the matrix (nh_cgm_*, nh_csr_spmm), so the matrix is read once per iteration and eight columns instead of once per iteration and column.

        `rhs`: a host array or a device tensor; None is not accepted.  `lhs0`: (n,), broadcast over the columns as the reference does, or (n, k).  `constrain`:
        (n,) in the two conventions of `constraints`, one mask for all columns; float constraints set every column to the constrained values.  On offer:
        solver='cg' with precon 'diag' (Jacobi) or None, for a SYMMETRIC POSITIVE DEFINITE matrix; every other solver, 'amg' and `preconargs` are a MatrixError
        (they solve one right-hand side at a time, through `solve`), and so are a missing tolerance and a matrix that is not square -- all before any device work.

        The stopping rule is the reference's: ONE bound for all columns of the call, max(atol, rtol max_j |r0_j|) with r0 = mask(rhs - A lhs), and every column
        must meet it.  Columns go in groups of at most eight; a group is one batched solve by the host loop of solver='cg': the true residuals by one block
        product, `check` iterations between two looks (one copy of 3k doubles), and once every column is within the bound by its recurrence the true residuals
        again, from which the columns that are above it restart while the others idle.  A column within the bound does no arithmetic, so column j of the result is,
        bit for bit, what `solve(rhs[:, j], atol=bound)` returns.  A block wider than eight columns is solved group by group on contiguous copies of its groups.
        `maxiter` (default: the free dofs) bounds the iterations of a group.  Raises MatrixError('cg: matrix is not positive definite') or ('cg: non-finite
        residual') for any column, ToleranceNotReached(best) with `best` of shape (n, k) when a column is above the bound after `maxiter` iterations.

        Sets `iterations` (the iterations enqueued for the group that took most; they are shared by the columns of a group) and `column_iterations` (a list: the
        iterations that moved each column, counted on the device, exact whatever `check` is).  Returns (n, k): a numpy array, or a device tensor if `rhs` was one.'''
        nrows, ncols = self.shape
        on_device, rhs = self._block_argument(rhs, nrows, 'right-hand side')
        k = rhs.shape[1]
        if nrows != ncols:
            raise MatrixError(f'constrained matrix is not square: {nrows}x{ncols}')
        offer = "solve_columns offers solver='cg' with precon='diag' or None"
        if solver != 'cg':
            raise MatrixError(f'{offer}; solver {solver!r} takes one right-hand side at a time (solve)')
        if precon not in ('diag', None):
            raise MatrixError(f'{offer}; the preconditioner {precon!r} takes one right-hand side at a time (solve)')
        if preconargs is not None:
            raise MatrixError(f"{offer}; preconargs are the arguments of precon='amg', which takes one right-hand side at a time (solve)")
        if not (atol > 0 or rtol > 0):
            raise MatrixError("solver 'cg' needs a tolerance: pass atol or rtol (an iterative solve has no machine-precision mode)")
        lhs0 = _host(lhs0)
        if lhs0 is not None:
            lhs0 = numpy.asarray(lhs0, dtype=float)
            if lhs0.shape not in ((ncols,), (ncols, k)):
                raise MatrixError(f'initial block has shape {lhs0.shape}, expected ({ncols},) or ({ncols}, {k})')
        constrain = _host(constrain)
        free, held = constraints(ncols, constrain)  # (one mask for all columns; `held`: zero with the values of float constraints written in)
        lhs = numpy.zeros((ncols, k))
        if lhs0 is not None:
            lhs[:] = lhs0 if lhs0.ndim == 2 else lhs0[:, None]
        if constrain is not None and numpy.asarray(constrain).dtype != bool:
            lhs[~free] = held[~free, None]
        return self._cg_columns(rhs, free, lhs, atol, rtol, precon, int(free.sum()) if maxiter is None else int(maxiter), max(1, int(check)), on_device)

    def _cg_columns(self, rhs, free, lhs, atol, rtol, precon, maxiter, check, on_device):
        from . import device, kernels
        n, k = lhs.shape
        values, rowptr, colidx = self.triplet()
        mask, x, b, dinv = self._krylov_setup(rhs if on_device else device.to_dev(rhs, 'float64'), free, lhs, precon, True)
        csr = dict(rowmask=mask, dinv=dinv, col32=self._columns(), lanes=self.lanes)
        groups = []
        for k0 in range(0, k, kernels.MULTI_MAX):  # a group: contiguous blocks of its own (the whole block if there is one group), the right-hand side a view
            cols = slice(k0, min(k0 + kernels.MULTI_MAX, k))
            xg = x if k <= kernels.MULTI_MAX else x[:, cols].contiguous()
            r, p, q = (device.torch().empty_like(xg) for _ in range(3))
            groups.append(dict(cols=cols, k=xg.shape[1], x=xg, b=b[:, cols], r=r, p=p, q=q, work=kernels.cgm_work(xg.shape[1])))

        def start(g):
            '''the true residuals mask(rhs - A x) of a group and fresh recurrences from them; returns r . r per column'''
            self.spmm(g['x'], alpha=-1., beta=1., B=g['b'], rowmask=mask, Y=g['r'])
            kernels.cgm_init(dinv, g['r'], g['p'], g['work'])
            rr = g['work'][:g['k']].tolist()
            if not numpy.isfinite(rr).all():
                raise MatrixError('cg: non-finite residual')
            return rr

        self.iterations, self.column_iterations = 0, [0] * k
        first = [start(g) for g in groups]
        stop_rr = max(atol, rtol * max(max(rr) for rr in first) ** .5) ** 2  # one bound for all columns (the device compares r . r with this number, and so does the host)
        reached = True
        for g, rr in zip(groups, first):
            kg, it = g['k'], 0
            while any(v > stop_rr for v in rr) and it < maxiter:
                kernels.cgm_stop(g['work'], kg, stop_rr)  # (a column within the bound idles: iterated past convergence its r . z would underflow, a false breakdown)
                while it < maxiter:
                    steps = min(check, maxiter - it)
                    kernels.cgm_iterate(values, rowptr, colidx, self._ncols, x=g['x'], r=g['r'], p=g['p'], q=g['q'], work=g['work'], niter=steps, **csr)
                    it += steps
                    head = g['work'][:3 * kg].tolist()
                    rr, flags, moved = head[:kg], head[kg:2 * kg], head[2 * kg:]
                    if any(flags):
                        raise MatrixError('cg: matrix is not positive definite')
                    if not numpy.isfinite(rr).all():
                        raise MatrixError('cg: non-finite residual')
                    if all(v <= stop_rr for v in rr):
                        break
                for j, m in enumerate(moved):  # (a start clears the device's counts)
                    self.column_iterations[g['cols'].start + j] += int(m)
                self.iterations = max(self.iterations, it)
                rr = start(g)
            reached = reached and all(v <= stop_rr for v in rr)
            if g['x'] is not x:
                x[:, g['cols']] = g['x']
        result = x if on_device else device.to_host(x)
        if not reached:
            raise ToleranceNotReached(result)
        return result

    def _krylov_setup(self, rhs, free, lhs, precon, on_device):
        '''(mask, x, b, dinv) of a device solve: the row mask of the free dofs (None: all), the start vector, the right-hand side, the inverse diagonal'''
        from . import device
        n = self.shape[0]
        mask = None if free.all() else device.to_dev(free, 'uint8')
        x = device.to_dev(lhs, 'float64')
        b = device.zeros(n, 'float64') if rhs is None else rhs.contiguous() if on_device else device.to_dev(rhs, 'float64')
        return mask, x, b, self._dinv(mask) if precon == 'diag' else None

    def _dinv(self, mask):
        '''the inverse diagonal on the rows the mask keeps, 0 elsewhere; a zero on a kept row is a MatrixError'''
        diag = self._diagonal_dev()
        keep = diag.new_ones(self.shape[0], dtype=bool) if mask is None else mask != 0
        if bool(((diag == 0) & keep).any()):
            raise MatrixError("building 'diag' preconditioner: diagonal has zero entries")
        return (1. / diag).masked_fill(~keep | (diag == 0), 0.)  # (constrained rows: any finite number, their residual is zero)

    def getprecon(self, precon, *, constrain=None, symmetric=True, **args):
        '''A preconditioner object (Matrix.getprecon of the reference, matrix/_base.py): built once, applied by `M(r)` (numpy in, numpy out; device tensor in,
        device tensor out) and taken by `solve(precon=M)` in place of a name, as often as wanted.  `constrain`: what `solve` takes (float with NaN on free dofs, or
        bool); it fixes the row mask of the preconditioner, and a solve that uses it must select the same dofs.

        'amg': the smoothed-aggregation V-cycle of `solve(solver='cg', precon='amg')`; `**args` are that solve's `preconargs` as keywords (coarse, sweeps,
        nullspace, setup, smoother, degree, eigsteps, eigratio), checked by the same functions with the same messages.  The symbolic phase comes from and goes
        to the matrix's cache as there, whatever `symmetric` is.  `symmetric=True` is exactly that hierarchy: `solve(solver='cg', precon=M)` returns the bytes of
        the solve that builds its own, without the numeric setup.  `symmetric=False` is for a matrix that need not be symmetric (its pattern must be,
        structurally: the aggregation says so otherwise): the dense level is inverted by the general pseudo-inverse, smoother='chebyshev' is a MatrixError (its
        bound is a Lanczos estimate), everything else is the same; such an object goes to `solve(solver='fgmres')` alone.
        'diag': the inverse diagonal, for every solver that takes precon='diag', with the same bytes on the same matrix; no arguments.
        'schur': the block preconditioner of a saddle point K = [[A, Bt], [B, C]] with C zero or small, where 'diag' finds zeros on the diagonal and 'amg' no
        elliptic operator: ``getprecon('schur', constrain=cons, second=pmask, schur=None, first=dict(coarse=256, sweeps=1, nullspace=None, setup=None))``.
        `second` (required): a bool mask of shape (n,) or strictly increasing indices, the dofs of the second field (the pressure); the first field is the
        rest, and both must have free dofs.  `first`: the arguments of the 'amg' cycle on the first block, checked as above (smoother='chebyshev' is refused as
        with symmetric=False; a `nullspace` has the shape (n, k) and is read on the first field's free dofs only); the hierarchy is built on K itself with
        those dofs as its row mask -- no submatrix is formed, the symbolic phase goes through the cache.  `schur`: the diagonal shat of an approximate Schur
        complement as a float vector of shape (n,), host array or device tensor, read on the second field's free dofs (for Stokes -diag(Mp) / nu); None is the
        SIMPLE choice shat_i = K_ii - sum_j K_ij K_ji / K_jj over the first field's free dofs j, computed on the device (nh_csr_schur_diagonal) with K_ji
        from the transpose, for which the pattern must be structurally symmetric.  A zero or non-finite shat_i is a MatrixError.  z = M r is the block
        upper-triangular solve z2 = r / shat, z1 = cycle(r - K z2), z = z1 + z2; r is not read on held dofs and z is zero there.  The object has
        symmetric=False whatever `symmetric` says and goes to `solve(solver='fgmres')` alone (nh_fgmres_iterate_schur).

        The object keeps alive what it reads: the hierarchy with its handle and level values, the value tensor it was built on, the masks.  It may be used on
        another matrix of the same shape and pattern (a matrix made by `_with_values`: the next Newton step, K + c M): that is a lagged preconditioner, which
        flexible GMRES tolerates by construction and CG as long as the object stays symmetric positive definite.  Argument errors are a MatrixError before any
        device work.'''
        from . import amg, device
        nrows, ncols = self.shape
        if nrows != ncols:
            raise MatrixError(f'constrained matrix is not square: {nrows}x{ncols}')
        if precon == 'amg':
            rest, setup = amg.split_setup(args)
            rest, smoother = amg.split_smoother(rest)
            if smoother is not None and not symmetric:
                raise MatrixError("amg: smoother='chebyshev' takes its bound from a Lanczos estimate, which needs a symmetric matrix; with symmetric=False the smoother is 'jacobi'")
            coarse, sweeps, nullspace = amg.check_args(rest, ncols)
        elif precon == 'diag':
            if args:
                raise MatrixError(f"invalid arguments {sorted(args)} for the 'diag' preconditioner: it takes none")
        elif precon == 'schur':
            second, shat, first = self._schur_args(args)
            rest, setup = amg.split_setup(first)
            rest, smoother = amg.split_smoother(rest)
            if smoother is not None:
                raise MatrixError("amg: smoother='chebyshev' takes its bound from a Lanczos estimate, which needs a symmetric matrix; with symmetric=False the smoother is 'jacobi'")
            coarse, sweeps, nullspace = amg.check_args(rest, ncols)
        else:
            raise MatrixError(f"invalid preconditioner {precon!r} for HipMatrix.getprecon: 'diag', 'amg' or 'schur'")
        free, _ = constraints(ncols, _host(constrain))
        if precon == 'schur':
            return self._schur(free, second, shat, coarse, sweeps, nullspace, setup)
        mask = None if free.all() else device.to_dev(free, 'uint8')
        if precon == 'diag':
            return amg.Preconditioner('diag', self.shape, free, True, self.triplet()[0], mask, dinv=self._dinv(mask))
        hierarchy = self._amg_hierarchy(free, mask, coarse, sweeps, nullspace, smoother, setup, symmetric=bool(symmetric))
        return amg.Preconditioner('amg', self.shape, free, symmetric, self.triplet()[0], mask, hierarchy=hierarchy)

    def _schur_args(self, args):
        '''(second, schur, first) of ``getprecon('schur', ...)``, validated on the host: `second` as a bool mask, `schur` None, a float host array or a device tensor
        of shape (n,), `first` a dict'''
        n = self.shape[1]
        args = dict(args)
        second, shat, first = args.pop('second', None), args.pop('schur', None), args.pop('first', None)
        if args:
            raise MatrixError(f"invalid arguments {sorted(args)} for the 'schur' preconditioner: 'second', 'schur' and 'first'")
        if second is None:
            raise MatrixError("schur: `second` is required: a bool mask of shape (n,) or strictly increasing indices that name the dofs of the second field (the pressure)")
        try:
            second = numpy.asarray(_host(second))
        except Exception:
            raise MatrixError(f'schur: second must be a bool mask or an integer array, got {type(second).__name__}') from None
        if second.ndim != 1 or second.dtype != bool and second.dtype.kind not in 'iu' or second.dtype == bool and len(second) != n:
            raise MatrixError(f'schur: second must be a bool mask of shape ({n},) or a vector of integer indices, got shape {second.shape} and dtype {second.dtype}')
        if second.dtype != bool:
            if second.size and (int(second.min()) < 0 or int(second.max()) >= n):
                raise MatrixError(f'schur: second has an index outside 0 .. {n - 1}')
            if second.size > 1 and not (second[1:] > second[:-1]).all():
                raise MatrixError('schur: the indices of second must be strictly increasing')
            index, second = second, numpy.zeros(n, dtype=bool)
            second[index] = True
        if first is not None and not isinstance(first, dict):
            raise MatrixError(f"schur: first must be a dict of the arguments of the 'amg' cycle on the first block, got {type(first).__name__}")
        if shat is not None:
            tensor = _is_tensor(shat)
            if not tensor:
                try:
                    shat = numpy.asarray(shat)
                except Exception:
                    raise MatrixError(f'schur: schur must be a float vector of shape ({n},), got {type(shat).__name__}') from None
            if tuple(shat.shape) != (n,) or 'float' not in str(shat.dtype):
                raise MatrixError(f'schur: schur must be a float vector of shape ({n},), got shape {tuple(shat.shape)} and dtype {shat.dtype}')
            if not tensor:
                shat = shat.astype(float)
        return second, shat, first

    @staticmethod
    def _schur_bad(shat, f2):
        '''whether shat, a host array or a device tensor, has a zero or non-finite entry where the mask f2 (of the same kind) is set'''
        finite = shat.isfinite() if _is_tensor(shat) else numpy.isfinite(shat)
        return bool(((shat == 0) | ~finite)[f2].any())

    def _schur(self, free, second, shat, coarse, sweeps, nullspace, setup):
        '''the 'schur' object of `getprecon`: the hierarchy of the first block on this matrix with the mask f1, the Schur diagonal (given, or the SIMPLE choice
        by nh_csr_schur_diagonal), and the handle that applies the two'''
        from . import amg, device, kernels
        torch = device.torch()
        f1, f2 = free & ~second, free & second
        if not f1.any() or not f2.any():
            raise MatrixError(f'schur: both fields need free dofs: the first has {int(f1.sum())}, the second {int(f2.sum())} (of {int(free.sum())} free dofs, {int(second.sum())} in `second`)')
        message = 'schur: the diagonal of the approximate Schur complement has zero or non-finite entries on the free dofs of the second field'
        if shat is not None and not _is_tensor(shat) and self._schur_bad(shat, f2):
            raise MatrixError(message)
        # -- the device from here on
        mask = None if free.all() else device.to_dev(free, 'uint8')
        mask1, f2_dev = device.to_dev(f1, 'uint8'), device.to_dev(f2, 'uint8') != 0
        values, rowptr, colidx = self.triplet()
        vt = None
        if shat is None:
            vt, rowptr_t, colidx_t = self.T.triplet()  # (the plan of the transpose stays on the matrix: the next one on this pattern pays one gather)
            if not (rowptr_t.shape == rowptr.shape and colidx_t.shape == colidx.shape and torch.equal(rowptr_t, rowptr) and torch.equal(colidx_t, colidx)):
                raise MatrixError('schur: the SIMPLE diagonal K_ii - sum_j K_ij K_ji / K_jj reads K_ji where K_ij lies, and the pattern of this matrix is not structurally '
                                  'symmetric: pass the diagonal of an approximate Schur complement as schur=')
        hierarchy = self._amg_hierarchy(f1, mask1, coarse, sweeps, nullspace, None, setup, symmetric=False)
        if vt is not None:
            shat = kernels.csr_schur_diagonal(values, rowptr, colidx, self._ncols, vt, mask1, hierarchy.data[0].dinv, col32=self._columns(), lanes=self.lanes)
        elif _is_tensor(shat):
            shat = shat.to(torch.float64).contiguous()
        else:
            shat = device.to_dev(shat, 'float64')
        if self._schur_bad(shat, f2_dev):
            raise MatrixError(message)
        sinv = (1. / shat).masked_fill(~f2_dev, 0.)
        schur = amg.Schur(hierarchy, (values, rowptr, colidx, self._ncols, self._columns(), self.lanes), mask1, sinv)
        return amg.Preconditioner('schur', self.shape, free, False, values, mask, hierarchy=hierarchy, schur=schur)

    def _amg_hierarchy(self, free, mask, coarse, sweeps, nullspace=None, smoother=None, setup=None, *, symmetric=True):
        '''the hierarchy of an 'amg' preconditioner (amg.Hierarchy): the symbolic phase is taken from the cache if it was made for this mask, this `coarse`,
        this number of near-nullspace vectors and this `setup`, the numeric phase runs on the values of this matrix (the smoother belongs to it: the cache
        does not know it)'''
        from . import amg, device
        _, rowptr, colidx = self.triplet()
        k = None if nullspace is None else nullspace.shape[1]
        if self._amg is None or self._amg[1] != coarse or self._amg[2] != k or self._amg[4] != setup or not numpy.array_equal(self._amg[0], free):
            self._amg = free.copy(), coarse, k, amg.symbolic(rowptr, colidx, None if mask is None else mask != 0, coarse, k, setup=setup), setup
        if nullspace is not None:  # PCIe: a host array goes up once, n k doubles
            nullspace = nullspace.contiguous() if _is_tensor(nullspace) else device.to_dev(nullspace, 'float64')
        return amg.Hierarchy(self._amg[3], self.triplet()[0], sweeps, nullspace, smoother, symmetric)


class _HipBackend:
    '''`matrix.backend('hip')`: host triplets (the hand-off of `function.eval(function.as_csr(K))`) become device matrices -- the round trip that
    `function.as_matrix` avoids.'''

    @staticmethod
    def assemble(values, rowptr, colidx, ncols):
        return HipMatrix(values, rowptr, colidx, ncols, validate=False)  # (`assemble_csr` has checked the triplet)

    assemble_trusted = assemble

    @staticmethod
    def assemble_device(values_dev, rowptr_dev, colidx_dev, ncols):
        '''The device hand-over: a matrix on the tensors the assembly left in HBM, nothing copied.  `solver.System` looks for this attribute; a backend
        that has it receives device tensors and solves where they lie.'''
        return HipMatrix(values_dev, rowptr_dev, colidx_dev, ncols)


class _Backend:
    '''``matrix.backend`` selector: any object with ``.assemble(values, rowptr,
    colidx, ncols)`` is accepted (matrix/__init__.py:20-27; fake-backend precedent
    /root/reference/tests/test_matrix.py:6-23).'''

    current = _ScipyBackend

    @contextlib.contextmanager
    def __call__(self, matrix):
        if isinstance(matrix, str):
            if matrix.lower() not in ('scipy', 'auto', 'hip'):
                raise ValueError(f'matrix backend {matrix!r} is not available in nutils_amd')
            matrix = _HipBackend if matrix.lower() == 'hip' else _ScipyBackend
        if not hasattr(matrix, 'assemble'):
            raise ValueError('matrix backend does not have an assemble function')
        previous, _Backend.current = _Backend.current, matrix
        try:
            yield matrix
        finally:
            _Backend.current = previous


backend = _Backend()


def _check_triplet(values, rowptr, colidx, ncols):
    '''The contract a backend may rely on (the conditions of matrix/__init__.py:47-69, each raising MatrixError): values a vector with
    one entry per column index; rowptr an integer vector that starts at 0, never decreases and ends at nnz; column indices integers
    below ncols that do not decrease inside a row.  One pass of numpy per condition.'''
    nnz = values.shape[0] if values.ndim == 1 else -1
    if nnz < 0:
        raise MatrixError(f'values must be a vector, got {values.ndim} axes')
    if rowptr.ndim != 1 or rowptr.dtype.kind not in 'ui' or not rowptr.size:
        raise MatrixError('row pointers must be a non-empty integer vector')
    if rowptr[0] != 0 or rowptr[-1] != nnz or numpy.any(numpy.diff(rowptr) < 0):
        raise MatrixError(f'row pointers must rise from 0 to the number of values ({nnz})')
    if colidx.ndim != 1 or colidx.dtype.kind not in 'ui' or colidx.size != nnz:
        raise MatrixError(f'column indices must be an integer vector of length {nnz}')
    if nnz and int(colidx.max()) >= ncols:
        raise MatrixError(f'column index {int(colidx.max())} outside the {ncols} columns')
    if nnz > 1:
        drops = numpy.flatnonzero(colidx[1:] < colidx[:-1]) + 1  # allowed only where a new row starts
        if drops.size and not numpy.isin(drops, rowptr).all():
            raise MatrixError('column indices decrease inside a row')


def assemble_csr(values, rowptr, colidx, ncols):
    '''Create sparse matrix from CSR sparse data (matrix/__init__.py:30-70): validate, then hand over to the current backend.'''
    values, rowptr, colidx = numpy.asarray(values), numpy.asarray(rowptr), numpy.asarray(colidx)
    ncols = ncols.__index__()
    _check_triplet(values, rowptr, colidx, ncols)
    return backend.current.assemble(values, rowptr, colidx, ncols)


def reassemble_csr(values, rowptr, colidx, ncols):
    '''`assemble_csr` for a (rowptr, colidx) pair that a previous `assemble_csr` call has validated -- the situation of every
    re-assembly inside a Newton or time loop, where the reference repeats the O(nnz) checks (matrix/__init__.py:47-69).
    Only the values are checked; backends without a trusted entry point get the ordinary one.'''
    values = numpy.asarray(values)
    if not (values.ndim == 1 and len(values) == len(colidx)):
        raise MatrixError('assemble received invalid values')
    trusted = getattr(backend.current, 'assemble_trusted', None)
    return trusted(values, rowptr, colidx, ncols) if trusted else backend.current.assemble(values, rowptr, colidx, ncols)


def compress_indices(indices, length):
    '''rowidx -> rowptr (numeric.py:687-711), vectorised.'''
    indices = numpy.asarray(indices)
    if len(indices) and (indices[0] < 0 or indices[-1] >= length):
        raise ValueError('indices are out of bounds')
    if len(indices) > 1 and (numpy.diff(indices) < 0).any():
        raise ValueError('indices are not monotomically increasing')
    return numpy.searchsorted(indices, numpy.arange(length + 1)).astype(numpy.int64)


def assemble_coo(values, rowidx, nrows, colidx, ncols):
    '''Create sparse matrix from COO sparse data (matrix/__init__.py:73-93).'''
    return assemble_csr(values, compress_indices(rowidx, nrows), colidx, ncols)


def assemble_block_csr(blocks):
    '''Create sparse block matrix from stacked CSR sparse data
    (matrix/__init__.py:103-151).  The reference merges multi-block rows with a
    Python loop over matrix rows; here the merge is one stable sort of the
    concatenated (row, block, position) keys.'''
    ncols = sum(n for *_, n in blocks[0])
    all_values, all_rows, all_cols, nrows_total = [], [], [], 0
    for row in blocks:
        nrows = len(row[0][1]) - 1
        col_offset = 0
        for block_values, block_rowptr, block_colidx, block_ncols in row:
            block_rowptr = numpy.asarray(block_rowptr)
            if len(block_rowptr) - 1 != nrows:
                raise MatrixError('sparse blocks have inconsistent row sizes')
            all_values.append(numpy.asarray(block_values))
            all_rows.append(numpy.repeat(numpy.arange(nrows) + nrows_total, numpy.diff(block_rowptr)))
            all_cols.append(numpy.asarray(block_colidx) + col_offset)
            col_offset += block_ncols
        if col_offset != ncols:
            raise MatrixError('sparse blocks have inconsistent column sizes')
        nrows_total += nrows
    values = numpy.concatenate(all_values)
    rows = numpy.concatenate(all_rows)
    cols = numpy.concatenate(all_cols)
    order = numpy.argsort(rows, kind='stable')  # blocks were appended in column order, so columns stay sorted per row
    return assemble_csr(values[order], compress_indices(rows[order], nrows_total), cols[order], ncols)
