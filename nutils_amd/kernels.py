'''Python faces of the C-ABI entry points (one function per kernel family).
Arguments are device tensors (see device.py); nothing here computes.'''

import ctypes
import os
import numpy

from . import _lib, device


def tabulate(coeffs_dev, nfn, ncoeffs, points_dev, nq, ndims):
    '''K2 (nh_poly_tabulate): T[nfn][nq][1+ndims].'''
    T = device.empty(nfn * nq * (1 + ndims), 'float64')
    _lib.call('nh_poly_tabulate', device.ptr(coeffs_dev), nfn, ncoeffs, device.ptr(points_dev), nq, ndims, device.ptr(T), device.stream())
    return T


def structured_dofs(shape, nloc, ndofs_axis, start_concat_dev, elem_begin, nelems):
    '''K1 (nh_structured_dofs).'''
    nd = len(shape)
    arr = ctypes.c_int * nd
    nb = int(numpy.prod(nloc))
    out = device.empty(nelems * nb, 'int32')
    _lib.call('nh_structured_dofs', nd, arr(*shape), arr(*nloc), arr(*ndofs_axis), device.ptr(start_concat_dev), elem_begin, nelems,
              device.ptr(out), device.stream())
    return out


GATHER_SCRATCH_LIMIT = 8 << 30
VECTOR_THREAD_PASS = {(3, 8, 3), (2, 4, 2), (2, 9, 2)}  # (ndims, functions per element, components) of nh_local_vector (nh_gather.hip)


class Pattern:
    '''K6 (nh_pattern_*): scalar sparsity pattern + element map, device resident.'''

    def __init__(self, nelems, nrows, ncols, tdofs, rdofs, nbt=0, nbr=0, toff=None, roff=None):
        args = _lib.PatternArgs(nelems, nrows, ncols, nbt, nbr, device.ptr(tdofs), device.ptr(rdofs), device.ptr(toff), device.ptr(roff))
        handle = ctypes.c_void_p()
        _lib.call('nh_pattern_build', ctypes.byref(args), ctypes.byref(handle), device.stream())
        self._handle = handle
        self._keep = (tdofs, rdofs, toff, roff)
        nnz = ctypes.c_int64()
        emap_len = ctypes.c_int64()
        srowptr, scol, emap, eoff = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.call('nh_pattern_info', handle, ctypes.byref(nnz), ctypes.byref(srowptr), ctypes.byref(scol), ctypes.byref(emap),
                  ctypes.byref(emap_len), ctypes.byref(eoff))
        self.nrows, self.ncols, self.nelems = nrows, ncols, nelems
        self.nnz_scalar = nnz.value
        self.srowptr_ptr, self.scol_ptr, self.emap_ptr, self.eoff_ptr = srowptr, scol, emap, eoff
        self.emap_len = emap_len.value

    def fused_info(self):
        '''(row blocks, rows per block, element visits) of the owner blocks built for NH_MATRIX_FUSED so far; (0, 0, 0): none'''
        nb, rpb, nv, rt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int()
        _lib.call('nh_pattern_fused_info', self._handle, ctypes.byref(nb), ctypes.byref(rpb), ctypes.byref(nv), ctypes.byref(rt))
        self.fused_routine = rt.value  # -1 none yet, 0 tabulated any-element routine, 1 / 2 sum-factorised trilinear routine (2: with a mass term)
        return nb.value, rpb.value, nv.value

    def owner_info(self):
        '''(row blocks, node rows per block, element visits, chunks of 64 contributions) of the row tasks built for vector-valued NH_MATRIX_FUSED so far; zeros: none'''
        nb, rpb, nv, nc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
        _lib.call('nh_pattern_owner_info', self._handle, ctypes.byref(nb), ctypes.byref(rpb), ctypes.byref(nv), ctypes.byref(nc))
        return nb.value, rpb.value, nv.value, nc.value

    def expanded_nnz(self, nct, ncr, mask=None):
        nnz = ctypes.c_int64()
        m = None if mask is None else numpy.ascontiguousarray(mask, dtype=numpy.uint8)
        _lib.call('nh_pattern_expanded_nnz', self._handle, nct, ncr, device.host_ptr(m), ctypes.byref(nnz))
        return nnz.value

    def expand(self, nct=1, ncr=1, mask=None):
        '''(rowptr, colidx) int64 device tensors of the component-expanded CSR (cached: re-assemblies reuse them).'''
        m = None if mask is None else numpy.ascontiguousarray(mask, dtype=numpy.uint8)
        key = nct, ncr, None if m is None else m.tobytes()
        cache = self.__dict__.setdefault('_expanded', {})
        if key in cache:
            return cache[key]
        cache[key] = self._expand(nct, ncr, m)
        return cache[key]

    def _expand(self, nct, ncr, m):
        nnz = self.expanded_nnz(nct, ncr, m)
        rowptr = device.empty(self.nrows * nct + 1, 'int64')
        colidx = device.empty(nnz, 'int64')
        _lib.call('nh_pattern_expand', self._handle, nct, ncr, device.host_ptr(m), device.ptr(rowptr), device.ptr(colidx), device.stream())
        return rowptr, colidx

    def __del__(self):
        h = getattr(self, '_handle', None)
        if h:
            try:
                _lib.load().nh_pattern_free(h)
            except Exception:
                pass
            self._handle = None


UNION_MAX = 8  # NH_UNION_MAX of nh_pattern.hip


def pattern_union(parts):
    '''Union of sorted-unique CSR patterns [(rowptr, colidx)] with equal row counts (nh_pattern_union_*): (rowptr, colidx, [position of every entry of part i in
    the union]).  Row-wise merge of sorted lists on the device; replaces the sort-based unique of the reference (evaluable.py:5560-5682).'''
    n = len(parts)
    nrows = parts[0][0].numel() - 1
    if any(rp.numel() - 1 != nrows for rp, _ in parts):
        raise ValueError('pattern_union: parts with different numbers of rows')
    if n > UNION_MAX:
        # more parts than one merge takes (NH_UNION_MAX): fold -- the union of the first UNION_MAX parts, then that union with the next UNION_MAX - 1, ...; the positions of a
        # part in an intermediate union are carried through the later ones
        rowptr, colidx, pos = pattern_union(parts[:UNION_MAX])
        at = UNION_MAX
        while at < n:
            more = parts[at:at + UNION_MAX - 1]
            rowptr2, colidx2, pos2 = pattern_union([(rowptr, colidx)] + more)
            pos = [pos2[0][q] for q in pos] + pos2[1:]
            rowptr, colidx = rowptr2, colidx2
            at += len(more)
        return rowptr, colidx, pos
    RP = (ctypes.c_void_p * n)(*[rp.data_ptr() for rp, _ in parts])
    CI = (ctypes.c_void_p * n)(*[ci.data_ptr() for _, ci in parts])
    rowptr = device.empty(nrows + 1, 'int64')
    nnz = ctypes.c_int64()
    _lib.call('nh_pattern_union_count', n, nrows, RP, CI, device.ptr(rowptr), ctypes.byref(nnz), device.stream())
    colidx = device.empty(nnz.value, 'int64')
    pos = [device.empty(ci.numel(), 'int64') for _, ci in parts]
    PP = (ctypes.c_void_p * n)(*[p.data_ptr() for p in pos])
    _lib.call('nh_pattern_union_fill', n, nrows, RP, CI, device.ptr(rowptr), device.ptr(colidx), PP, device.stream())
    return rowptr, colidx, pos


def geometry_iso(ngb, gT, gdofs, verts, bnd_axis=-1):
    g = _lib.Geometry(_lib.GEOM_ISO, ngb, device.ptr(gT), device.ptr(gdofs), device.ptr(verts), None, None, None, None, bnd_axis)
    g._keep = (gT, gdofs, verts)
    return g


def geometry_box(origin, size, bnd_axis=-1):
    g = _lib.Geometry(_lib.GEOM_BOX, 0, None, None, None, device.ptr(origin), device.ptr(size), None, None, bnd_axis)
    g._keep = (origin, size)
    return g


def geometry_tab(jac, x=None, bnd_axis=-1):
    g = _lib.Geometry(_lib.GEOM_TAB, 0, None, None, None, None, None, device.ptr(jac), device.ptr(x), bnd_axis)
    g._keep = (jac, x)
    return g


def factor_tensor(*, nelems, ndims, nq, rank, weights, geom, basis, ndofs, coeff=1., scale=None, elist=None):
    '''Taylor coefficient tensor of rank 3 or 4 of  coeff int scale u^rank dV  built on the device (nh_factor_tensor / nh_factor_fetch): (values[nnz],
    indices[rank][nnz]) as the reference's Monomial holds them (evaluable.py:5693-5751, 5785-5874).'''
    args = _lib.FactorArgs(nelems, device.ptr(elist), ndims, nq, rank, device.ptr(weights), geom, basis, device.ptr(scale), float(coeff), int(ndofs))
    nnz = ctypes.c_int64(0)
    _lib.call('nh_factor_tensor', ctypes.byref(args), ctypes.byref(nnz), device.stream())
    values = device.empty(nnz.value, 'float64')
    indices = device.empty(rank * nnz.value, 'int64')
    _lib.call('nh_factor_fetch', device.ptr(values), device.ptr(indices), device.stream())
    return values, indices.reshape(rank, nnz.value)


def rationalize(T, nelems, nb, dofs, weights, nq, ndims, W=None, dW=None, off=None):
    '''N_i = w_i B_i / W in place on per-element tables (nh_rationalize).'''
    _lib.call('nh_rationalize', device.ptr(T), nelems, nb, device.ptr(off), device.ptr(dofs), device.ptr(weights), device.ptr(W), device.ptr(dW), nq, ndims,
              device.stream())


def basis(T, dofs, nb=0, off=None, tab=None):
    b = _lib.Basis(nb, device.ptr(T), device.ptr(dofs), device.ptr(off), device.ptr(tab))
    b._keep = (T, dofs, off, tab)
    return b


# (dimension, functions per element) for which the owner-block kernels (NH_MATRIX_FUSED; they cover (1, 2), (1, 3), (2, 3), (2, 4), (2, 9), (3, 4), (3, 8) with fused=True)
# are the DEFAULT: measured faster than the gather with the ordered sums (tools/generic_probe.py, round 5, ordered rounds: 128^3 trilinear
# 0.55 against 0.90 ms; 2048^2 bilinear 0.43 against 0.45, 1024^2 quadratic splines 0.43 against 0.59, but 1024^2 biquadratic 0.88 against 0.69 ms -- the 2-D sizes stay
# with the gather)
FUSED_DEFAULT = {(3, 8)}
# (dimension, functions per element, components) of the owner kernel for vector-valued blocks (nh_owner.hip: Gram sums per scalar entry from D tables in LDS, one pass)
OWNER_VECTOR = {(3, 8, 3), (2, 4, 2), (2, 9, 2), (3, 27, 3)}


def _follow_connectivity(pattern, geom):
    '''The owner plan of vector-valued blocks keeps the vertex numbers of its visiting elements, made from the connectivity of an isoparametric geometry and
    keyed on its address (nh_pattern_forget_connectivity).  A tensor refilled in place keeps its address and bumps its version: then they are remade.'''
    gdofs = getattr(geom, '_keep', (None, None))[1] if geom.kind == _lib.GEOM_ISO else None
    key = None if gdofs is None else (gdofs.data_ptr(), gdofs._version)
    if getattr(pattern, '_connectivity', key) != key:
        _lib.call('nh_pattern_forget_connectivity', pattern._handle)
    pattern._connectivity = key


def assemble_matrix(*, nelems, ndims, nq, weights, geom, test, trial, nct, ncr, C, mask, pattern, values, elist=None, emap_offset=0, scale=None, flags=0,
                    cq=None, first_touch=None, gather=None, store=False, fused=False, fresh=False):
    '''K3+K4+K5 (nh_assemble_matrix); accumulates into `values`.  `first_touch=(grid_shape, nodes_per_axis)`: NH_MATRIX_FIRST_TOUCH.
    gather: NH_MATRIX_GATHER (deterministic owner-side reduction instead of atomics); None = from the second assembly on a pattern on (the gather
    map costs one device sort of the element map, which a one-off assembly does not earn back).  fused: NH_MATRIX_FUSED (owner blocks: one pass
    without scratch or global atomics for scalar blocks on small uniform bases, contributions added in visit order: bit-reproducible, bit-identical to the gather; excludes gather;
    the default for those blocks -- NUTILS_AMD_NO_FUSED=1 restores the gather / atomics choice).  fresh: `values` is uninitialised -- the gather and
    owner-block paths STORE their sums (no zero fill, no read of the old values), every other path gets the array zero-filled first.'''
    C = numpy.ascontiguousarray(C, dtype=float)
    if C.shape != (nct, 1 + ndims, ncr, 1 + ndims):
        raise ValueError(f'coefficient tensor has shape {C.shape}, expected {(nct, 1 + ndims, ncr, 1 + ndims)}')
    _follow_connectivity(pattern, geom)
    m = None if mask is None else numpy.ascontiguousarray(mask, dtype=numpy.uint8)
    if cq is not None and cq.numel() != nelems * nq * C.size:
        raise ValueError('per-point coefficient tensor must have shape [nelems][nq] + C.shape')
    args = _lib.MatrixArgs(nelems, device.ptr(elist), ndims, nq, device.ptr(weights), geom, test, trial, nct, ncr, device.host_ptr(C),
                           device.host_ptr(m), pattern.srowptr_ptr, ctypes.c_void_p(pattern.emap_ptr.value + 4 * emap_offset), pattern.eoff_ptr,
                           device.ptr(values), device.ptr(scale), int(flags) | (32 if first_touch else 0), device.ptr(cq))
    if first_touch:
        args.grid_shape[:] = list(first_touch[0]) + [1] * (3 - len(first_touch[0]))
        args.nodes_per_axis = int(first_touch[1])
    if elist is None and emap_offset == 0 and not os.environ.get('NUTILS_AMD_NO_BUCKETS'):
        args.pattern = pattern._handle  # ragged bases: launches per size class of the pattern
    whole = emap_offset == 0 and not flags and not first_touch and nelems == pattern.nelems
    if (not fused and gather is None and not os.environ.get('NUTILS_AMD_NO_FUSED') and whole and elist is None and nct == ncr == 1 and cq is None and (ndims, test.nb) in FUSED_DEFAULT
            and test.nb == trial.nb and test.dofs_dev == trial.dofs_dev and not test.off_dev):
        # (default since round 4 for the blocks the owner-block kernels cover: one pass, 1.5 x instead of 4.6 x the algorithmic traffic, and -- with the
        # turns of the block plan -- bit-reproducible like the gather)
        fused = True
    if (not fused and gather is None and not os.environ.get('NUTILS_AMD_NO_FUSED') and whole and elist is None and nct == ncr and cq is None and (ndims, test.nb, nct) in OWNER_VECTOR
            and test.nb == trial.nb and test.T_dev == trial.T_dev and test.dofs_dev == trial.dofs_dev and test.tab_dev == trial.tab_dev and not test.off_dev):
        fused = True  # (vector-valued blocks on small uniform bases: one pass instead of the thread pass + gather, 2.3 x the algorithmic bytes)
    if fused:
        if not whole:
            raise ValueError('fused needs all elements of the pattern in one call')
        if gather:
            raise ValueError('fused excludes gather')
        gather = False
    if gather is None:
        # (automatic only while the scratch of the local matrices stays below GATHER_SCRATCH_LIMIT bytes: 1.07 GB for the 128^3 trilinear mesh)
        # and for blocks with a thread pass (scalar blocks; the vector-valued sizes of VECTOR_THREAD_PASS): the local matrices of other vector-valued
        # blocks go through the one-wave-per-element kernel either way, and writing + gathering them costs more than its atomics -- 96^3 trilinear
        # elasticity 15.7 against 7.9 ms, 32^3 triquadratic 14.5 against 3.9 ms, tools/generic_probe.py)
        thread_pass = nct == ncr == 1 or ((ndims, test.nb, nct) in VECTOR_THREAD_PASS and nct == ncr and cq is None and test.nb == trial.nb
                                          and test.T_dev == trial.T_dev and test.dofs_dev == trial.dofs_dev and test.tab_dev == trial.tab_dev and not test.off_dev)
        # ... and blocks on ragged bases with a constant form.  Vector-valued: the element kernel sums Gram matrices per node pair (nh_assemble_generic.hip), which leaves
        # the global atomics as its bound -- 63 488 rational hierarchical elements 2.36 ms with atomics, 1.76 ms through the gather.  Scalar: 1.20 against 1.22 ms -- the
        # same time, and the sums become bit-reproducible (tools/ragged_probe.py, RAGGED_PROBE_SCALAR=1)
        thread_pass = thread_pass or bool(test.off_dev and cq is None)
        gather = (whole and thread_pass and getattr(pattern, '_assemblies', 0) >= 1 and not os.environ.get('NUTILS_AMD_NO_GATHER')
                  and 8 * pattern.emap_len * nct * ncr <= GATHER_SCRATCH_LIMIT and pattern.emap_len < 2 ** 32 and pattern.nnz_scalar < 2 ** 32)
    if whole:
        pattern._assemblies = getattr(pattern, '_assemblies', 0) + 1
    if fresh:
        if gather or fused:
            store = True
        else:
            values.zero_()
    if gather:
        if not whole:
            raise ValueError('gather needs all elements of the pattern in one call')
        args.pattern = pattern._handle
        args.flags |= 64 | (128 if store else 0)
    elif fused:
        args.pattern = pattern._handle
        args.flags |= 256 | (128 if store else 0)
    elif store:
        raise ValueError('store is an option of the gather and fused paths')
    _lib.call('nh_assemble_matrix', ctypes.byref(args), device.stream())


class ScatterPlan:
    '''Map of the deterministic vector scatter (nh_scatter_plan_build): for every dof the positions of its contributions in an element-major
    array of local vectors, in the order of the reference's loop.  One per (basis tables, element list).'''

    def __init__(self, *, nelems, nrows, nb, dofs, off=None, elist=None, nlist=None):
        handle = ctypes.c_void_p()
        _lib.call('nh_scatter_plan_build', int(nelems), int(nrows), int(nb), device.ptr(dofs), device.ptr(off), device.ptr(elist),
                  int(nelems if elist is None else nlist), ctypes.byref(handle), device.stream())
        self._handle, self._keep = handle, (dofs, off, elist)
        self.npositions = int(dofs.numel())  # length of a local array per component

    def __del__(self):
        h = getattr(self, '_handle', None)
        if h:
            try:
                _lib.load().nh_scatter_plan_free(h)
            except Exception:
                pass
            self._handle = None


def scatter_gather(pairs, ncomp, out, accumulate=True):
    '''out[dof][c] (+)= sum over the (plan, local array) pairs, in order, of the contributions of dof (nh_scatter_gather).'''
    n = len(pairs)
    P = (ctypes.c_void_p * n)(*[p._handle.value for p, _ in pairs])
    L = (ctypes.c_void_p * n)(*[loc.data_ptr() for _, loc in pairs])
    _lib.call('nh_scatter_gather', n, P, L, int(ncomp), device.ptr(out), int(bool(accumulate)), device.stream())


def assemble_vector(*, nelems, ndims, nq, weights, geom, test, trial, nct, ncr, C=None, f=None, u=None, out=None, f0=0., out_scalar=None,
                    elist=None, scale=None, local=None):
    C = None if C is None else numpy.ascontiguousarray(C, dtype=float)
    f = None if f is None else numpy.ascontiguousarray(f, dtype=float)
    if C is not None and C.shape != (nct, 1 + ndims, ncr, 1 + ndims):
        raise ValueError(f'coefficient tensor has shape {C.shape}')
    if f is not None and f.shape != (nct, 1 + ndims):
        raise ValueError(f'source tensor has shape {f.shape}')
    args = _lib.VectorArgs(nelems, device.ptr(elist), ndims, nq, device.ptr(weights), geom, test, trial, nct, ncr, device.host_ptr(C),
                           device.host_ptr(f), device.ptr(u), device.ptr(out), float(f0), device.ptr(out_scalar), device.ptr(scale), device.ptr(local))
    _lib.call('nh_assemble_vector', ctypes.byref(args), device.stream())


def _terms_args(keep, *, nelems, ndims, nq, weights, geom, fields, blocks, terms, polys=(), elist=None):
    S = 1 + ndims
    F, P = _fields_polys(fields, polys, keep)
    B = (_lib.Block * len(blocks))()
    for i, blk in enumerate(blocks):  # (test struct, nct, out[, local array of the deterministic scatter])
        B[i] = _lib.Block(blk[0], int(blk[1]), device.ptr(blk[2]), device.ptr(blk[3]) if len(blk) > 3 else None)
    T = (_lib.Term * len(terms))()
    for i, t in enumerate(terms):
        blk, fld = int(t['block']), int(t.get('field', -1))
        nct = blocks[blk][1]
        C, f = t.get('C'), t.get('f')
        if C is not None:
            C = numpy.ascontiguousarray(C, dtype=float)
            if fld < 0 or C.shape != (nct, S, fields[fld][2], S):
                raise ValueError(f'term {i}: coefficient tensor has shape {C.shape}')
        if f is not None:
            f = numpy.ascontiguousarray(f, dtype=float)
            if f.shape != (nct, S):
                raise ValueError(f'term {i}: source tensor has shape {f.shape}')
        qB, qt, qr = _qs(t.get('qs'), S)
        keep += [C, f, qB]
        T[i] = _lib.Term(blk, fld, int(t.get('poly', -1)), device.host_ptr(C), device.host_ptr(f), device.ptr(t.get('scale')), qt, qr, device.host_ptr(qB))
    keep += [F, P, B, T]
    return _lib.TermsArgs(nelems, device.ptr(elist), ndims, nq, device.ptr(weights), geom, len(fields), F, len(blocks), B, len(terms), T, len(polys), P)


def assemble_terms(**kwargs):
    '''All linear-form terms of a residual on one sample in ONE element loop (nh_assemble_terms).  Keywords: nelems, ndims, nq, weights, geom, elist=None,
    fields: [(basis struct, u, ncomp)], blocks: [(test struct, nct, out)], polys: [(vars [(field, comp)], coeffs, powers [nterms][nvars])],
    terms: [dict(block, field=-1, poly=-1, C=None, f=None, scale=None)].'''
    keep = []
    args = _terms_args(keep, **kwargs)
    _lib.call('nh_assemble_terms', ctypes.byref(args), device.stream())


def assemble_terms_multi(lists):
    '''The term lists of several samples (`lists`: keyword dicts of assemble_terms) in one launch (nh_assemble_terms_multi).'''
    if not lists:
        return
    keep = []
    args = [_terms_args(keep, **kw) for kw in lists]
    ptrs = (ctypes.POINTER(_lib.TermsArgs) * len(args))(*[ctypes.pointer(a) for a in args])
    _lib.call('nh_assemble_terms_multi', len(args), ptrs, device.stream())


TERMS_FAMILIES = ('k_terms', 'k_terms_multi', 'k_local_vterms2', 'k_mterms', 'k_local_terms', 'k_local_terms2')


def terms_launch_counts():
    '''{kernel family: launches since the library was loaded} of the term-list entries (nh_terms_launch_counts).'''
    counts = (ctypes.c_int64 * len(TERMS_FAMILIES))()
    _lib.call('nh_terms_launch_counts', counts)
    return dict(zip(TERMS_FAMILIES, counts))


GENERIC_FAMILIES = {'k_matrix_mfma': ('ND', 'MT', 'nt', 'kt', 'nas'), 'k_matrix_generic': ('branch', 'waves', 'use_w', 'qchunk', 'sym'),
                    'k_gram_sym': ('E', 'W', 'NC', 'USE0', 'TRI'), 'k_vector_generic': ('qchunk',)}
GENERIC_BRANCHES = ('entries', 'scalar_symmetric', 'gram', 'gram_symmetric')


def generic_launch_record():
    '''({kernel family: launches since the library was loaded}, {family: the launcher's choice for its last launch}) of the element kernels of
    nh_assemble_matrix / nh_assemble_vector (nh_generic_launch_record); the branch of k_matrix_generic by its name in GENERIC_BRANCHES.'''
    counts, last = (ctypes.c_int64 * len(GENERIC_FAMILIES))(), (ctypes.c_int32 * 16)()
    _lib.call('nh_generic_launch_record', counts, last)
    choice, at = {}, 0
    for family, names in GENERIC_FAMILIES.items():
        choice[family] = dict(zip(names, last[at:at + len(names)]))
        at += 5
    choice['k_matrix_generic']['branch'] = GENERIC_BRANCHES[choice['k_matrix_generic']['branch']]
    return dict(zip(GENERIC_FAMILIES, counts)), choice


def _qs(qs, S):
    '''term option qs = (B [S][S], field_t, field_r): point factor U_t . B . U_r'''
    if qs is None:
        return None, -1, -1
    B = numpy.ascontiguousarray(qs[0], dtype=float)
    if B.shape != (S, S):
        raise ValueError(f'point factor tensor has shape {B.shape}')
    return B, int(qs[1]), int(qs[2])


def _fields_polys(fields, polys, keep):
    F = (_lib.Field * max(len(fields), 1))()
    for i, (b, u, nc) in enumerate(fields):
        F[i] = _lib.Field(b, device.ptr(u), int(nc))
    P = (_lib.PointPoly * max(len(polys), 1))()
    for i, (vars_, coeffs, powers) in enumerate(polys):
        cf = numpy.ascontiguousarray(coeffs, dtype=float)
        pw = numpy.ascontiguousarray(powers, dtype=numpy.int32).reshape(len(cf), len(vars_))
        keep += [cf, pw]
        fld = (ctypes.c_int * 4)(*([v[0] for v in vars_] + [0] * (4 - len(vars_))))
        cmp_ = (ctypes.c_int * 4)(*([v[1] for v in vars_] + [0] * (4 - len(vars_))))
        P[i] = _lib.PointPoly(len(vars_), len(cf), fld, cmp_, device.host_ptr(cf), pw.ctypes.data if pw.size else None)
    return F, P


def assemble_matrix_terms(*, nelems, ndims, nq, weights, geom, test, trial, nct, ncr, mask, pattern, values, terms, fields=(), polys=(), elist=None, flags=0,
                          gather=None):
    '''All bilinear-form terms of a matrix block in ONE element loop, several elements per workgroup (nh_assemble_matrix_terms); accumulates
    into `values`.  terms: [dict(C, kind=0, field=-1, poly=-1, L=None, scale=None)], fields / polys as in assemble_terms.'''
    S = 1 + ndims
    keep = []
    F, P = _fields_polys(fields, polys, keep)
    m = None if mask is None else numpy.ascontiguousarray(mask, dtype=numpy.uint8)
    T = (_lib.MatrixTerm * len(terms))()
    for i, t in enumerate(terms):
        C = numpy.ascontiguousarray(t['C'], dtype=float)
        if C.shape != (nct, S, ncr, S):
            raise ValueError(f'term {i}: coefficient tensor has shape {C.shape}, expected {(nct, S, ncr, S)}')
        L = t.get('L')
        if L is not None:
            L = numpy.ascontiguousarray(L, dtype=float)
            if L.shape != (nct, S):
                raise ValueError(f'term {i}: L has shape {L.shape}')
        qB, qt, qr = _qs(t.get('qs'), S)
        keep += [C, L, qB]
        T[i] = _lib.MatrixTerm(int(t.get('kind', 0)), int(t.get('field', -1)), int(t.get('poly', -1)), device.host_ptr(C), device.host_ptr(L), device.ptr(t.get('scale')),
                               qt, qr, device.host_ptr(qB))
    whole = not flags and nelems == pattern.nelems
    if gather is None:  # (as in assemble_matrix: the owner-side reduction from the second assembly on a pattern on; blocks that do not qualify ignore it)
        gather = (whole and getattr(pattern, '_assemblies', 0) >= 1 and not os.environ.get('NUTILS_AMD_NO_GATHER')
                  and 8 * pattern.emap_len <= GATHER_SCRATCH_LIMIT and pattern.emap_len < 2 ** 32 and pattern.nnz_scalar < 2 ** 32)
    if whole:
        pattern._assemblies = getattr(pattern, '_assemblies', 0) + 1
    args = _lib.MatrixTermsArgs(nelems, device.ptr(elist), ndims, nq, device.ptr(weights), geom, test, trial, nct, ncr, device.host_ptr(m), pattern.srowptr_ptr,
                                pattern.emap_ptr, pattern.eoff_ptr, device.ptr(values), int(flags) | (64 if gather and whole else 0), len(fields), F, len(terms), T,
                                len(polys), P, pattern._handle)
    _lib.call('nh_assemble_matrix_terms', ctypes.byref(args), device.stream())


def sample_eval(*, nelems, ndims, nq, geom, trial=None, ncr=1, points=None, u=None, x=None, detj=None, U=None, elist=None):
    if trial is None:
        trial = _lib.Basis(0, None, None, None, None)
    args = _lib.EvalArgs(nelems, device.ptr(elist), ndims, nq, geom, trial, ncr, device.ptr(points), device.ptr(u), device.ptr(x), device.ptr(detj), device.ptr(U))
    _lib.call('nh_sample_eval', ctypes.byref(args), device.stream())


def p1hex_pattern(shape, row_begin=0, row_end=None):
    '''Closed-form CSR index arrays of the trilinear basis on a structured hex mesh (nh_p1hex_pattern).'''
    n0, n1, n2 = (int(n) for n in shape)
    nrows = (n0 + 1) * (n1 + 1) * (n2 + 1)
    if row_end is None:
        row_end = nrows

    def cum(X, N):
        return 0 if X == 0 else (3 * N - 2 if X >= N else 3 * X - 1)

    def rp(r):
        if r >= nrows:
            return (3 * n0 + 1) * (3 * n1 + 1) * (3 * n2 + 1)
        K, J, I = r % (n2 + 1), (r // (n2 + 1)) % (n1 + 1), r // ((n2 + 1) * (n1 + 1))
        ln = lambda X, N: (X > 0) + 1 + (X < N - 1)
        return cum(I, n0 + 1) * (3 * n1 + 1) * (3 * n2 + 1) + ln(I, n0 + 1) * (cum(J, n1 + 1) * (3 * n2 + 1) + ln(J, n1 + 1) * cum(K, n2 + 1))

    nnz = rp(row_end) - rp(row_begin)
    rowptr = device.empty(row_end - row_begin + 1, 'int64')
    colidx = device.empty(nnz, 'int64')
    arr = (ctypes.c_int * 3)(n0, n1, n2)
    _lib.call('nh_p1hex_pattern', arr, row_begin, row_end, device.ptr(rowptr), device.ptr(colidx), device.stream())
    return rowptr, colidx


def _p1hex_args(shape, values, gauss_x, gauss_w, verts, origin, scale, kappa, layers, planes, unit_matrix=None, qscale=None, max_workgroups=0, mass=0.,
                qmass=None):
    n0 = int(shape[0])
    layers = (0, n0) if layers is None else layers
    planes = (0, n0 + 1) if planes is None else planes
    a = _lib.P1HexArgs()
    a.shape[:] = [int(n) for n in shape]
    a.layer_begin, a.layer_end = layers
    a.plane_begin, a.plane_end = planes
    a.verts_dev = device.ptr(verts)
    a.origin[:] = [float(x) for x in origin]
    a.scale[:] = [float(x) for x in scale]
    a.gauss_x[:] = [float(x) for x in gauss_x]
    a.gauss_w[:] = [float(x) for x in gauss_w]
    a.kappa = float(kappa)
    a.values_dev = device.ptr(values)
    a.unit_matrix_dev = device.ptr(unit_matrix)
    if qscale is not None and qscale.numel() != 8 * int(shape[0]) * int(shape[1]) * int(shape[2]):
        raise ValueError('qscale must hold 8 values per element')
    a.qscale_dev = device.ptr(qscale)
    a.max_workgroups = int(max_workgroups)
    if qmass is not None and qmass.numel() != 8 * int(shape[0]) * int(shape[1]) * int(shape[2]):
        raise ValueError('qmass must hold 8 values per element')
    a.mass = float(mass) if qmass is None or mass else 1.
    a.qmass_dev = device.ptr(qmass)
    return a


def p1hex_unit_matrix(*, shape, gauss_x, gauss_w, origin=(0., 0., 0.), scale=(1., 1., 1.), kappa=1., mass=0.):
    '''8x8 element matrix of the uniform cell (nh_p1hex_unit_matrix): computed once per mesh.'''
    ke = device.empty(64, 'float64')
    a = _p1hex_args(shape, None, gauss_x, gauss_w, None, origin, scale, kappa, None, None, mass=mass)
    _lib.call('nh_p1hex_unit_matrix', ctypes.byref(a), device.ptr(ke), device.stream())
    return ke


def p1hex_laplace(*, shape, values, gauss_x, gauss_w, verts=None, origin=(0., 0., 0.), scale=(1., 1., 1.), kappa=1., layers=None, planes=None,
                  unit_matrix=None, qscale=None, max_workgroups=0, mass=0., qmass=None):
    '''Write-once structured P1-hex assembly of kappa grad.grad + mass phi phi (nh_p1hex_laplace).'''
    a = _p1hex_args(shape, values, gauss_x, gauss_w, verts, origin, scale, kappa, layers, planes, unit_matrix, qscale, max_workgroups, mass, qmass)
    _lib.call('nh_p1hex_laplace', ctypes.byref(a), device.stream())


class P1HexLaplace:
    '''nh_p1hex_laplace with the argument block filled ONCE: a re-assembly is one ctypes call (the per-step path of a Newton loop or of
    bench.py; building the block costs more host time than the launch).  Call with the value array of the step.'''

    def __init__(self, **kwargs):
        self._keep = kwargs  # the tensors whose addresses the block holds
        values = kwargs.pop('values', None)
        self._args = _p1hex_args(kwargs['shape'], values, kwargs['gauss_x'], kwargs['gauss_w'], kwargs.get('verts'), kwargs.get('origin', (0., 0., 0.)),
                                 kwargs.get('scale', (1., 1., 1.)), kwargs.get('kappa', 1.), kwargs.get('layers'), kwargs.get('planes'), kwargs.get('unit_matrix'),
                                 kwargs.get('qscale'), kwargs.get('max_workgroups', 0), kwargs.get('mass', 0.), kwargs.get('qmass'))
        self._ref = ctypes.byref(self._args)
        self._name = 'nh_p1hex_laplace'
        self._fn = getattr(_lib.load(), self._name)

    def __call__(self, values):
        self._args.values_dev = values.data_ptr()
        if _lib.TRACE is not None:
            _lib.TRACE.append(self._name)
        _lib.check(self._fn(self._ref, device.stream()))


def p1hex_apply(*, shape, u, out, gauss_x, gauss_w, verts, kappa=1., layers=None, planes=None, qscale=None, accumulate=True, max_workgroups=0, mass=0.,
                qmass=None):
    '''out (+)= K u for the P1-hex Laplace form without forming K (nh_p1hex_apply).'''
    n = (int(shape[0]) + 1) * (int(shape[1]) + 1) * (int(shape[2]) + 1)
    if u.numel() != n or out.numel() != n:
        raise ValueError('u and out must hold one value per vertex')
    a = _p1hex_args(shape, None, gauss_x, gauss_w, verts, (0., 0., 0.), (1., 1., 1.), kappa, layers, planes, None, qscale, max_workgroups, mass, qmass)
    _lib.call('nh_p1hex_apply', ctypes.byref(a), device.ptr(u), device.ptr(out), int(bool(accumulate)), device.stream())


def p2hex_rowptr(shape, node):
    '''Scalar row pointer of a node of the structured C0 quadratic basis (closed form, nh_p2hex_rowptr).'''
    out = ctypes.c_int64()
    _lib.call('nh_p2hex_rowptr', (ctypes.c_int * 3)(*[int(n) for n in shape]), int(node), ctypes.byref(out))
    return out.value


def p2hex_pattern(shape, ncomp):
    '''Closed-form CSR index arrays of the structured C0 quadratic hex basis with ncomp fully coupled components (nh_p2hex_pattern).'''
    n0, n1, n2 = (int(n) for n in shape)
    nnodes = (2 * n0 + 1) * (2 * n1 + 1) * (2 * n2 + 1)
    nnz = p2hex_rowptr(shape, nnodes) * ncomp * ncomp
    rowptr = device.empty(nnodes * ncomp + 1, 'int64')
    colidx = device.empty(nnz, 'int64')
    _lib.call('nh_p2hex_pattern', (ctypes.c_int * 3)(n0, n1, n2), int(ncomp), device.ptr(rowptr), device.ptr(colidx), device.stream())
    return rowptr, colidx


class P2HexMatrix:
    '''Write-once assembly of a constant-coefficient form on the structured C0 quadratic hex basis (nh_p2hex_matrix), argument block
    filled once: a re-assembly is one ctypes call.  Call with the value array of the step.'''

    def __init__(self, *, shape, nq, weights, geom, T, ncomp, C, scale=None, layers=None, owners=None, max_workgroups=0):
        C = numpy.ascontiguousarray(C, dtype=float)
        if C.shape != (ncomp, 4, ncomp, 4):
            raise ValueError(f'coefficient tensor has shape {C.shape}, expected {(ncomp, 4, ncomp, 4)}')
        n0 = int(shape[0])
        a = _lib.P2HexArgs()
        a.shape[:] = [int(n) for n in shape]
        a.nq = int(nq)
        a.weights_dev = device.ptr(weights)
        a.geom = geom
        a.T_dev = device.ptr(T)
        a.ncomp = int(ncomp)
        a.C_host = device.host_ptr(C)
        a.scale_dev = device.ptr(scale)
        a.layer_begin, a.layer_end = (0, n0) if layers is None else layers
        a.owner_begin, a.owner_end = (0, n0) if owners is None else owners
        a.max_workgroups = int(max_workgroups)
        a.weights_positive = int(bool((weights > 0).all().item()))  # (once per plan: the object lives as long as the weight array it keeps)
        self._keep = (weights, geom, T, C, scale)
        self._args = a
        self._ref = ctypes.byref(a)
        self._name = 'nh_p2hex_matrix'
        self._fn = getattr(_lib.load(), self._name)

    def __call__(self, values):
        self._args.values_dev = values.data_ptr()
        if _lib.TRACE is not None:
            _lib.TRACE.append(self._name)
        _lib.check(self._fn(self._ref, device.stream()))


class P2HexUniform:
    '''The same matrix on a mesh of UNIFORM cells (`cell`: the three edge lengths; constant form, no pointwise factor): the mesh of 2 x 2 x 2 such cells is assembled once by
    nh_p2hex_matrix, a (re-)assembly replicates its rows (nh_p2hex_rows_uniform: one write stream).  `owners` as for P2HexMatrix (slabs: owner io holds the node planes
    2 io and 2 io + 1).'''

    def __init__(self, *, shape, nq, weights, T, ncomp, C, cell, owners=None):
        idx = numpy.stack(numpy.meshgrid(*[numpy.arange(2.)] * 3, indexing='ij'), -1).reshape(-1, 3)
        cell = numpy.asarray(cell, dtype=float).reshape(3)
        small = (2, 2, 2)
        rp = ctypes.c_int64()
        _lib.call('nh_p2hex_rowptr', (ctypes.c_int * 3)(*small), 125, ctypes.byref(rp))
        self.table = device.empty(rp.value * ncomp * ncomp, 'float64')
        geom = geometry_box(device.to_dev(idx * cell, 'float64'), device.to_dev(numpy.broadcast_to(cell, idx.shape), 'float64'))
        P2HexMatrix(shape=small, nq=nq, weights=weights, geom=geom, T=T, ncomp=ncomp, C=C)(self.table)
        n0 = int(shape[0])
        ob, oe = (0, n0) if owners is None else owners
        self._shape = (ctypes.c_int * 3)(*[int(n) for n in shape])
        self._planes = 2 * int(ob), min(2 * int(oe) + 2, 2 * n0 + 1)
        self._nc = int(ncomp)
        self._name = 'nh_p2hex_rows_uniform'
        self._fn = getattr(_lib.load(), self._name)

    def __call__(self, values):
        if _lib.TRACE is not None:
            _lib.TRACE.append(self._name)
        _lib.check(self._fn(self._shape, self._nc, self.table.data_ptr(), values.data_ptr(), self._planes[0], self._planes[1], device.stream()))


def p2hex_matrix(*, values, **kwargs):
    P2HexMatrix(**kwargs)(values)


def monomial_csr(rowptr, colidx, values, x, y, alpha=1.):
    '''y[r] += alpha * sum_k values[k] x[colidx[k]] (nh_monomial_csr).'''
    if rowptr.numel() <= 1:  # (no rows: nothing to add to; tensors without elements have no allocation and the C ABI refuses their NULL pointers)
        return
    _lib.call('nh_monomial_csr', rowptr.numel() - 1, device.ptr(rowptr), device.ptr(colidx), device.ptr(values), device.ptr(x), float(alpha), device.ptr(y),
              device.stream())


def monomial(values, args, indices, out, out_index=None, alpha=1.):
    '''out[out_index[i]] += alpha values[i] prod_k args[k][indices[k][i]] (nh_monomial).'''
    n = len(args)
    if not values.numel():  # (no entries: as in monomial_csr)
        return
    A = (ctypes.c_void_p * max(n, 1))(*[a.data_ptr() for a in args])
    I = (ctypes.c_void_p * max(n, 1))(*[i.data_ptr() for i in indices])
    _lib.call('nh_monomial', values.numel(), device.ptr(values), n, A, I, device.ptr(out_index), float(alpha), device.ptr(out), device.stream())


def index_copy(src, dst, src_index=None, dst_index=None):
    '''dst[dst_index[i]] = src[src_index[i]] (nh_index_copy); `dst` is a device tensor or a PINNED host tensor (device-mapped).'''
    if not (dst.is_cuda or dst.is_pinned()):
        raise ValueError('index_copy: the destination must be device memory or page-locked host memory')
    n = (src_index if src_index is not None else dst_index if dst_index is not None else src).numel()
    if not n:
        return
    _lib.call('nh_index_copy', n, device.ptr(src), device.ptr(src_index), device.ptr(dst_index), device.ptr(dst), device.stream())


def pointwise_poly(xs, strides, coeffs, powers, n):
    '''out[i] = sum_t coeffs[t] prod_v xs[v][i*strides[v]]^powers[t][v] (nh_pointwise_poly).'''
    nv, nt = len(xs), len(coeffs)
    out = device.empty(n, 'float64')
    X = (ctypes.c_void_p * max(nv, 1))(*[x.data_ptr() for x in xs])
    S = (ctypes.c_int * max(nv, 1))(*[int(s) for s in strides])
    C = (ctypes.c_double * max(nt, 1))(*[float(c) for c in coeffs])
    P = (ctypes.c_int * max(nt * nv, 1))(*[int(p) for row in powers for p in row])
    _lib.call('nh_pointwise_poly', n, nv, X, S, nt, C, P, device.ptr(out), device.stream())
    return out


def point_expr(xs, strides, out_index, offsets, coef, n, nout, scale=None, out=None):
    '''out[i][f] (+)= scale_i sum_{t: out_index[t] == f} coef[t] prod_v xs[v][i*strides[v] + offsets[t][v]] (nh_point_expr): the contraction of field values at
    the points of a sample with a sparse constant tensor.  out_index (int32, ascending), offsets (int32 [nentries][nvars]), coef: device tables; `out`: added to if given.'''
    nv = len(xs)
    fresh = out is None
    if fresh:
        out = device.empty(n * nout, 'float64')
    X = (ctypes.c_void_p * max(nv, 1))(*[x.data_ptr() for x in xs])
    S = (ctypes.c_int64 * max(nv, 1))(*[int(s) for s in strides])
    _lib.call('nh_point_expr', n, nv, X, S, int(coef.numel()), device.ptr(out_index), device.ptr(offsets) if nv else None, device.ptr(coef),
              device.ptr(scale) if scale is not None else None, nout, device.ptr(out), 0 if fresh else 1, device.stream())
    return out


def point_forms(kind, Ut, B, Ur=None, L=None, scale=None):
    '''Per-point forms of field values (nh_point_forms): kind 0 -> [npoints] point factor Ut.B.Ur; kind 1 / 2 -> [npoints][S][S] coefficient
    tensors of the product-rule terms (sample._MatrixPlan.run).  Ut, Ur: [npoints][S] on the device; B [S][S], L [S] on the host.'''
    n, S = int(Ut.shape[0]), int(Ut.shape[1])
    B = numpy.ascontiguousarray(B, dtype=float).reshape(S, S)
    out = device.empty(n if kind == 0 else n * S * S, 'float64')
    Bc = (ctypes.c_double * (S * S))(*B.ravel())
    Lc = (ctypes.c_double * S)(*numpy.asarray(L, dtype=float).ravel()) if L is not None else None
    _lib.call('nh_point_forms', kind, n, S, device.ptr(Ut), device.ptr(Ur) if Ur is not None else None, Bc, Lc,
              device.ptr(scale) if scale is not None else None, device.ptr(out), device.stream())
    return out


QUAD_BTYPES = {'std': 0, 'spline': 1}


def quad_nnz(shape, btype, degree, ncomp):
    '''Entries of the closed-form CSR of a structured 2-D basis with ncomp fully coupled components (nh_quad_nnz: host only, no device).'''
    out = ctypes.c_int64()
    _lib.call('nh_quad_nnz', (ctypes.c_int * 2)(*[int(n) for n in shape]), QUAD_BTYPES[btype], int(degree), int(ncomp), ctypes.byref(out))
    return out.value


def quad_pattern(shape, btype, degree, ncomp):
    '''Closed-form CSR index arrays of the structured 2-D 'std' / 'spline' basis with ncomp fully coupled components (nh_quad_pattern).'''
    n0, n1 = (int(n) for n in shape)
    ndofs = (n0 + degree, n1 + degree) if btype == 'spline' else (n0 * degree + 1, n1 * degree + 1)
    rowptr = device.empty(ndofs[0] * ndofs[1] * ncomp + 1, 'int64')
    colidx = device.empty(quad_nnz(shape, btype, degree, ncomp), 'int64')
    _lib.call('nh_quad_pattern', (ctypes.c_int * 2)(n0, n1), QUAD_BTYPES[btype], int(degree), int(ncomp), device.ptr(rowptr), device.ptr(colidx), device.stream())
    return rowptr, colidx


class QuadMatrix:
    '''Write-once assembly of a constant-coefficient form on a structured 2-D basis (nh_quad_matrix), argument block filled once: a re-assembly is one
    ctypes call.  T: the class tables [nclass][nb][nq][3]; classes: the per-axis class arrays (StructuredBasis.axis_class), host.  Call with the value
    array of the step.'''

    def __init__(self, *, shape, btype, degree, nq, weights, geom, T, classes, ncomp, C, max_workgroups=0):
        C = numpy.ascontiguousarray(C, dtype=float)
        if C.shape != (ncomp, 3, ncomp, 3):
            raise ValueError(f'coefficient tensor has shape {C.shape}, expected {(ncomp, 3, ncomp, 3)}')
        a = _lib.QuadArgs()
        a.shape[:] = [int(n) for n in shape]
        a.btype, a.degree, a.nq = QUAD_BTYPES[btype], int(degree), int(nq)
        a.weights_dev = device.ptr(weights)
        a.geom = geom
        a.T_dev = device.ptr(T)
        ncls = [int(numpy.max(c)) + 1 for c in classes]
        cls = [device.to_dev(numpy.asarray(c, dtype=numpy.int32), 'int32') if n > 1 else None for c, n in zip(classes, ncls)]
        a.nclass[:] = ncls
        a.class0_dev, a.class1_dev = device.ptr(cls[0]), device.ptr(cls[1])
        a.ncomp = int(ncomp)
        a.C_host = device.host_ptr(C)
        a.max_workgroups = int(max_workgroups)
        self._keep = (weights, geom, T, C, cls)
        self._args = a
        self._ref = ctypes.byref(a)
        self._name = 'nh_quad_matrix'
        self._fn = getattr(_lib.load(), self._name)

    def __call__(self, values):
        self._args.values_dev = values.data_ptr()
        if _lib.TRACE is not None:
            _lib.TRACE.append(self._name)
        _lib.check(self._fn(self._ref, device.stream()))


class QuadUniform:
    '''The same matrix on a mesh of UNIFORM cells (`cell`: the two edge lengths): the small mesh of nh_quad_uniform_shape of such cells is assembled once by
    nh_quad_matrix (its first and last elements per axis take the classes of the big mesh's), a (re-)assembly replicates its rows (nh_quad_rows_uniform).'''

    def __init__(self, *, shape, btype, degree, nq, weights, T, classes, ncomp, C, cell):
        small = (ctypes.c_int * 2)()
        self._shape = (ctypes.c_int * 2)(*[int(n) for n in shape])
        _lib.call('nh_quad_uniform_shape', self._shape, QUAD_BTYPES[btype], int(degree), small)
        small = tuple(small)
        cls = []
        for n, ns, c in zip(shape, small, classes):
            es = numpy.arange(ns)
            cls.append(numpy.asarray(c)[numpy.where(es <= ns // 2, es, es - ns + int(n))])
        idx = numpy.stack(numpy.meshgrid(*[numpy.arange(float(n)) for n in small], indexing='ij'), -1).reshape(-1, 2)
        cell = numpy.asarray(cell, dtype=float).reshape(2)
        geom = geometry_box(device.to_dev(idx * cell, 'float64'), device.to_dev(numpy.broadcast_to(cell, idx.shape), 'float64'))
        self.table = device.empty(quad_nnz(small, btype, degree, ncomp), 'float64')
        QuadMatrix(shape=small, btype=btype, degree=degree, nq=nq, weights=weights, geom=geom, T=T, classes=cls, ncomp=ncomp, C=C)(self.table)
        self._bt, self._deg, self._nc = QUAD_BTYPES[btype], int(degree), int(ncomp)
        self._name = 'nh_quad_rows_uniform'
        self._fn = getattr(_lib.load(), self._name)

    def __call__(self, values):
        if _lib.TRACE is not None:
            _lib.TRACE.append(self._name)
        _lib.check(self._fn(self._shape, self._bt, self._deg, self._nc, self.table.data_ptr(), values.data_ptr(), device.stream()))


def hex1_nnz(shape, ncomp):
    '''Entries of the closed-form CSR of the trilinear 'std' basis of a 3-D structured mesh with ncomp fully coupled components (nh_hex1_nnz: host only,
    no device).'''
    out = ctypes.c_int64()
    _lib.call('nh_hex1_nnz', (ctypes.c_int * 3)(*[int(n) for n in shape]), int(ncomp), ctypes.byref(out))
    return out.value


def hex1_pattern(shape, ncomp):
    '''Closed-form CSR index arrays of the trilinear 'std' basis of a 3-D structured mesh with ncomp fully coupled components (nh_hex1_pattern).'''
    shape = [int(n) for n in shape]
    rowptr = device.empty(int(numpy.prod([n + 1 for n in shape])) * ncomp + 1, 'int64')
    colidx = device.empty(hex1_nnz(shape, ncomp), 'int64')
    _lib.call('nh_hex1_pattern', (ctypes.c_int * 3)(*shape), int(ncomp), device.ptr(rowptr), device.ptr(colidx), device.stream())
    return rowptr, colidx


class Hex1Matrix:
    '''Write-once assembly of a constant-coefficient form on the trilinear 'std' basis of a 3-D structured mesh (nh_hex1_matrix), argument block filled
    once: a re-assembly is one ctypes call.  T: the basis table [8][nq][4]; geom: an ISO (vertices, lexicographic) or BOX geometry.  Call with the
    value array of the step.'''

    def __init__(self, *, shape, nq, weights, geom, T, ncomp, C):
        C = numpy.ascontiguousarray(C, dtype=float)
        if C.shape != (ncomp, 4, ncomp, 4):
            raise ValueError(f'coefficient tensor has shape {C.shape}, expected {(ncomp, 4, ncomp, 4)}')
        a = _lib.Hex1Args()
        a.shape[:] = [int(n) for n in shape]
        a.nq = int(nq)
        a.weights_dev = device.ptr(weights)
        a.geom = geom
        a.T_dev = device.ptr(T)
        a.ncomp = int(ncomp)
        a.C_host = device.host_ptr(C)
        self._keep = (weights, geom, T, C)
        self._args = a
        self._ref = ctypes.byref(a)
        self._name = 'nh_hex1_matrix'
        self._fn = getattr(_lib.load(), self._name)

    def __call__(self, values):
        self._args.values_dev = values.data_ptr()
        if _lib.TRACE is not None:
            _lib.TRACE.append(self._name)
        _lib.check(self._fn(self._ref, device.stream()))


class Hex1Uniform:
    '''The same matrix on a mesh of UNIFORM cells (`cell`: the three edge lengths): the mesh of min(n, 2) such cells per axis is assembled once by
    nh_hex1_matrix, a (re-)assembly replicates its rows (nh_hex1_rows_uniform).'''

    def __init__(self, *, shape, nq, weights, T, ncomp, C, cell):
        small = tuple(min(int(n), 2) for n in shape)
        self._shape = (ctypes.c_int * 3)(*[int(n) for n in shape])
        idx = numpy.stack(numpy.meshgrid(*[numpy.arange(float(n)) for n in small], indexing='ij'), -1).reshape(-1, 3)
        cell = numpy.asarray(cell, dtype=float).reshape(3)
        geom = geometry_box(device.to_dev(idx * cell, 'float64'), device.to_dev(numpy.broadcast_to(cell, idx.shape), 'float64'))
        self.table = device.empty(hex1_nnz(small, ncomp), 'float64')
        Hex1Matrix(shape=small, nq=nq, weights=weights, geom=geom, T=T, ncomp=ncomp, C=C)(self.table)
        self._nc = int(ncomp)
        self._name = 'nh_hex1_rows_uniform'
        self._fn = getattr(_lib.load(), self._name)

    def __call__(self, values):
        if _lib.TRACE is not None:
            _lib.TRACE.append(self._name)
        _lib.check(self._fn(self._shape, self._nc, self.table.data_ptr(), values.data_ptr(), device.stream()))


# ---- device-resident CSR matrix (nh_csr.hip) ---------------------------------------------------------

def _csr(values, rowptr, colidx, ncols, col32, lanes):
    return _lib.Csr(rowptr.numel() - 1, int(ncols), values.numel(), device.ptr(values), device.ptr(rowptr), device.ptr(colidx), device.ptr(col32), int(lanes))


def csr_lanes(nrows, nnz):
    '''lanes per row the library takes for `lanes=0` (nh_csr_lanes; a host computation)'''
    return _lib.load().nh_csr_lanes(int(nrows), int(nnz))


def csr_compact(colidx, ncols):
    '''int32 copy of the int64 column indices (nh_csr_compact)'''
    col32 = device.empty(colidx.numel(), 'int32')
    _lib.call('nh_csr_compact', colidx.numel(), int(ncols), device.ptr(colidx), device.ptr(col32), device.stream())
    return col32


def csr_spmv(values, rowptr, colidx, ncols, x, *, y=None, alpha=1., beta=0., b=None, rowmask=None, col32=None, lanes=0):
    '''y = mask(alpha A x + beta b) (nh_csr_spmv).  col32: the narrowed column indices of `csr_compact`; None: the kernel reads the int64 `colidx`.
    lanes: lanes per row (0: the library's rule).  `b` may be `y`.'''
    if y is None:
        y = device.empty(rowptr.numel() - 1, 'float64')
    _lib.call('nh_csr_spmv', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), float(alpha), device.ptr(x), float(beta), device.ptr(b),
              device.ptr(rowmask), device.ptr(y), device.stream())
    return y


def csr_diagonal(values, rowptr, colidx, ncols, *, col32=None):
    '''diag[i] = A_ii or 0 (nh_csr_diagonal)'''
    diag = device.empty(rowptr.numel() - 1, 'float64')
    _lib.call('nh_csr_diagonal', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, 0)), device.ptr(diag), device.stream())
    return diag


def csr_support(values, rowptr, colidx, ncols, tol=0., *, rows=True, cols=True, col32=None, lanes=0):
    '''(rowsupp, colsupp): uint8 device vectors, 1 where a row / a column holds an entry with |a| > tol (nh_csr_support); None for the one not asked for'''
    rowsupp = device.empty(rowptr.numel() - 1, 'uint8') if rows else None
    colsupp = device.empty(int(ncols), 'uint8') if cols else None
    _lib.call('nh_csr_support', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), float(tol), device.ptr(rowsupp), device.ptr(colsupp), device.stream())
    return rowsupp, colsupp


def csr_transpose(rowptr, colidx, ncols, *, col32=None):
    '''(rowptr_t, colidx_t, pos): the pattern of the transpose and the position in the operand of every entry of it (nh_csr_transpose); the values of the
    transpose are `csr_gather(values, pos)`.  Rows sorted, the same tensors at every call.'''
    nnz = colidx.numel()
    rowptr_t, colidx_t, pos = device.empty(int(ncols) + 1, 'int64'), device.empty(nnz, 'int64'), device.empty(nnz, 'int64')
    A = _lib.Csr(rowptr.numel() - 1, int(ncols), nnz, None, device.ptr(rowptr), device.ptr(colidx), device.ptr(col32), 0)
    _lib.call('nh_csr_transpose', ctypes.byref(A), device.ptr(rowptr_t), device.ptr(colidx_t), device.ptr(pos), device.stream())
    return rowptr_t, colidx_t, pos


def csr_select(values, rowptr, colidx, ncols, *, rowkeep=None, colkeep=None, nrows_s=None, ncols_s=None, drop_zeros=False, col32=None, lanes=0, lazy=False):
    '''(rowptr_s, colidx_s, pos): the entries of the rows that the uint8 device vector `rowkeep` keeps and of the columns that `colkeep` keeps (None: all),
    without the exact zeros if `drop_zeros`; rows and columns numbered anew in ascending order, `pos` the position in the operand of every kept entry
    (nh_csr_select_count, nh_csr_select_fill).  `nrows_s`, `ncols_s`: how many rows and columns the masks keep; the library checks them.  `lazy`: None
    if every entry is kept and there are no masks -- the operand's own index tensors will do, the fill is skipped.'''
    nrows = rowptr.numel() - 1
    nrows_s = nrows if rowkeep is None else int(nrows_s)
    ncols_s = int(ncols) if colkeep is None else int(ncols_s)
    A = _csr(values, rowptr, colidx, ncols, col32, lanes)
    newrow = None if rowkeep is None else device.empty(nrows + 1, 'int64')
    newcol = None if colkeep is None else device.empty(int(ncols) + 1, 'int64')
    rowptr_s = device.empty(nrows_s + 1, 'int64')
    nnz = ctypes.c_int64()
    masks = device.ptr(rowkeep), device.ptr(colkeep), int(bool(drop_zeros))
    _lib.call('nh_csr_select_count', ctypes.byref(A), *masks, nrows_s, ncols_s, device.ptr(newrow), device.ptr(newcol), device.ptr(rowptr_s), ctypes.byref(nnz),
              device.stream())
    if lazy and rowkeep is None and colkeep is None and nnz.value == values.numel():
        return None
    colidx_s, pos = device.empty(nnz.value, 'int64'), device.empty(nnz.value, 'int64')
    if nnz.value:
        _lib.call('nh_csr_select_fill', ctypes.byref(A), *masks, device.ptr(newrow), device.ptr(newcol), device.ptr(rowptr_s), device.ptr(colidx_s), device.ptr(pos),
                  device.stream())
    return rowptr_s, colidx_s, pos


def csr_gather(values, pos):
    '''values[pos] as a new device vector (nh_index_copy): the values of a transpose or a selection from its plan'''
    out = device.empty(pos.numel(), 'float64')
    index_copy(values, out, src_index=pos)
    return out


def csr_add(a, pos_a, b, pos_b, sign, nnz_u):
    '''the values of a + sign b on the union of two patterns, `pos_a` and `pos_b` the positions of the parts' entries in it (`pattern_union`): zero, a
    placed, sign b added (nh_csr_add_values); sign is 1 or -1'''
    out = device.empty(nnz_u, 'float64')
    _lib.call('nh_csr_add_values', a.numel(), device.ptr(a), device.ptr(pos_a), b.numel(), device.ptr(b), device.ptr(pos_b), float(sign), int(nnz_u), device.ptr(out),
              device.stream())
    return out


def cg_work():
    '''the work array of a CG solve (nh_cg_work_doubles): [0] = r . r of the recurrence, [1] = breakdown flag, [2] = the bound of `cg_stop`'''
    return device.empty(_lib.load().nh_cg_work_doubles(), 'float64')


def cg_init(dinv, r, p, work):
    '''p = z = dinv r, first r . z and r . r, flag and bound cleared (nh_cg_init)'''
    _lib.call('nh_cg_init', r.numel(), device.ptr(dinv), device.ptr(r), device.ptr(p), device.ptr(work), device.stream())


def cg_stop(work, stop_rr):
    '''after `cg_init`: iterations that find r . r <= stop_rr do nothing (work[2] of nh_cg_iterate)'''
    work[2:3].fill_(float(stop_rr))


def cg_iterate(values, rowptr, colidx, ncols, *, rowmask, dinv, x, r, p, q, work, niter, col32=None, lanes=0):
    '''enqueue `niter` CG iterations (nh_cg_iterate): three launches each, nothing read back; they stop moving once r . r is within the bound of `cg_stop`'''
    _lib.call('nh_cg_iterate', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(rowmask), device.ptr(dinv), device.ptr(x), device.ptr(r),
              device.ptr(p), device.ptr(q), device.ptr(work), int(niter), device.stream())


MULTI_MAX = 8  # NH_MULTI_MAX: columns per group of the block product, and the most a batched CG takes at once


def _block(name, t, nrows):
    '''(k, ld) of a block of vectors: a 2-D float64 device tensor of `nrows` rows with unit column stride; its row stride is the leading dimension'''
    if not (hasattr(t, 'data_ptr') and t.is_cuda and t.dtype == device.torch().float64 and t.dim() == 2):
        raise ValueError(f'{name} must be a 2-D float64 device tensor')
    n, k = t.shape
    if n != nrows or k < 1:
        raise ValueError(f'{name} has shape {tuple(t.shape)}, expected ({nrows}, k) with k >= 1')
    if t.stride(1) != 1:
        raise ValueError(f'{name} must have unit column stride (got strides {tuple(t.stride())}): a block of vectors is row-major')
    if n > 1 and t.stride(0) < k:
        raise ValueError(f'{name} has row stride {t.stride(0)} for {k} columns: rows must not overlap')
    return k, (t.stride(0) if n > 1 else k)


def csr_spmm(values, rowptr, colidx, ncols, X, *, Y=None, alpha=1., beta=0., B=None, rowmask=None, col32=None, lanes=0):
    '''Y = mask(alpha A X + beta B) for a block of k >= 1 vectors (nh_csr_spmm): the matrix is read once per group of `MULTI_MAX` columns.  `X` (ncols, k), `B`
    and `Y` (nrows, k) are 2-D float64 device tensors with unit column stride and any row stride (a column slice of a wider tensor is fine); anything else
    is a ValueError.  `B` may be `Y`.  Column j of the result is, bit for bit, `csr_spmv` of column j.'''
    nrows = rowptr.numel() - 1
    k, ldx = _block('X', X, int(ncols))
    if Y is None:
        Y = device.torch().empty((nrows, k), dtype=X.dtype, device=X.device)
    ky, ldy = _block('Y', Y, nrows)
    kb, ldb = (k, 0) if B is None else _block('B', B, nrows)
    if ky != k or kb != k:
        raise ValueError(f'X has {k} columns, Y {ky}' + ('' if B is None else f', B {kb}'))
    _lib.call('nh_csr_spmm', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), k, float(alpha), device.ptr(X), ldx, float(beta), device.ptr(B), ldb,
              device.ptr(rowmask), device.ptr(Y), ldy, device.stream())
    return Y


def cgm_work(k):
    '''the work array of a batched CG on k <= `MULTI_MAX` columns (nh_cgm_work_doubles): [0:k] = r . r of the recurrences, [k:2k] = breakdown flags, [2k:3k] = the
    iterations since `cgm_init` that moved each column, [3k:4k] = the bounds of `cgm_stop`'''
    size = _lib.load().nh_cgm_work_doubles(int(k))
    if size < 0:
        _lib.check(-1)
    return device.empty(size, 'float64')


def cgm_init(dinv, r, p, work):
    '''per column of the contiguous (n, k) blocks: p = z = dinv r, first r . z and r . r; flags, counts and bounds cleared (nh_cgm_init)'''
    n, k = r.shape
    _lib.call('nh_cgm_init', n, k, device.ptr(dinv), device.ptr(r), device.ptr(p), device.ptr(work), device.stream())


def cgm_stop(work, k, stop_rr):
    '''after `cgm_init`: a column whose r . r <= stop_rr idles (work[3k:4k] of nh_cgm_iterate); `stop_rr` is one number for all columns or one each'''
    work[3 * k:4 * k] = device.torch().as_tensor(stop_rr, dtype=work.dtype, device=work.device)


def cgm_iterate(values, rowptr, colidx, ncols, *, rowmask, dinv, x, r, p, q, work, niter, col32=None, lanes=0):
    '''enqueue `niter` iterations of the batched CG on the contiguous (n, k) blocks x, r, p, q (nh_cgm_iterate): three launches each for all columns, nothing
    read back; a column stops moving once its r . r is within the bound of `cgm_stop`'''
    n, k = x.shape
    for name, t in (('x', x), ('r', r), ('p', p), ('q', q)):
        if tuple(t.shape) != (n, k) or not t.is_contiguous():
            raise ValueError(f'{name} must be a contiguous ({n}, {k}) block')
    _lib.call('nh_cgm_iterate', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), k, device.ptr(rowmask), device.ptr(dinv), device.ptr(x), device.ptr(r),
              device.ptr(p), device.ptr(q), device.ptr(work), int(niter), device.stream())


def bicgstab_work():
    '''the work array of a BiCGStab solve (nh_bicgstab_work_doubles): [0] = r . r of the recurrence, [1] = breakdown flag, [2] = iterations since
    `bicgstab_init` that moved x'''
    return device.empty(_lib.load().nh_bicgstab_work_doubles(), 'float64')


def csr_spmv_dots(values, rowptr, colidx, ncols, x, w, *, y=None, rowmask=None, col32=None, lanes=0, work=None):
    '''the product of a BiCGStab iteration on its own (nh_csr_spmv_dots): y = mask(A x); returns (y, dots) with dots[0] = w . y and dots[1] = y . y, a view of
    the first cells of `work`'''
    if y is None:
        y = device.empty(rowptr.numel() - 1, 'float64')
    if work is None:
        work = bicgstab_work()
    _lib.call('nh_csr_spmv_dots', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(x), device.ptr(w), device.ptr(rowmask), device.ptr(y),
              device.ptr(work), device.stream())
    return y, work[:2]


def bicgstab_init(dinv, r, rhat, p, phat, work):
    '''rhat = p = r, phat = dinv r, first r . r, flag and count cleared (nh_bicgstab_init); `phat` is None without a preconditioner'''
    _lib.call('nh_bicgstab_init', r.numel(), device.ptr(dinv), device.ptr(r), device.ptr(rhat), device.ptr(p), device.ptr(phat), device.ptr(work), device.stream())


def bicgstab_iterate(values, rowptr, colidx, ncols, *, rowmask, dinv, x, r, rhat, p, v, s, t, phat, shat, work, stop_rr, niter, col32=None, lanes=0):
    '''enqueue `niter` BiCGStab iterations (nh_bicgstab_iterate): five launches each, nothing read back; they stop moving once r . r <= stop_rr'''
    _lib.call('nh_bicgstab_iterate', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(rowmask), device.ptr(dinv), device.ptr(x), device.ptr(r),
              device.ptr(rhat), device.ptr(p), device.ptr(v), device.ptr(s), device.ptr(t), device.ptr(phat), device.ptr(shat), device.ptr(work), float(stop_rr), int(niter),
              device.stream())


def minres_work():
    '''the work array of a MINRES solve (nh_minres_work_doubles): [0] = r . r of the recurrence, [1] = flag, [2] = iterations since `minres_init` that moved x'''
    return device.empty(_lib.load().nh_minres_work_doubles(), 'float64')


def minres_init(dinv, r, r1, r2, v, w1, w2, work):
    '''r1 = r2 = r, w1 = w2 = 0, v = dinv r / sqrt(r . dinv r), first r . r, flag and count cleared (nh_minres_init); `dinv` is positive, or None'''
    _lib.call('nh_minres_init', r.numel(), device.ptr(dinv), device.ptr(r), device.ptr(r1), device.ptr(r2), device.ptr(v), device.ptr(w1), device.ptr(w2), device.ptr(work),
              device.stream())


def minres_iterate(values, rowptr, colidx, ncols, *, rowmask, dinv, x, r, r1, r2, v, q, w1, w2, work, stop_rr, niter, col32=None, lanes=0):
    '''enqueue `niter` MINRES iterations (nh_minres_iterate): three launches each and one at the end, nothing read back; they stop moving once r . r <= stop_rr'''
    _lib.call('nh_minres_iterate', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(rowmask), device.ptr(dinv), device.ptr(x), device.ptr(r),
              device.ptr(r1), device.ptr(r2), device.ptr(v), device.ptr(q), device.ptr(w1), device.ptr(w2), device.ptr(work), float(stop_rr), int(niter), device.stream())


GMRES_CHUNK = 8  # GS_CHUNK of nh_csr.hip: basis vectors the Gram-Schmidt kernels take per pass over w


def gmres_work(restart):
    '''the work array of a GMRES cycle of up to `restart` steps (nh_gmres_work_doubles): [0] = the squared residual norm of the least-squares problem (after
    `gmres_init`: r . r), [1] = 1. once a direction vanished or was not finite, [2] = Arnoldi steps since `gmres_init`'''
    size = _lib.load().nh_gmres_work_doubles(int(restart))
    if size < 0:
        _lib.check(-1)
    return device.empty(size, 'float64')


def gmres_init(dinv, r, V, z, work, *, restart):
    '''start a cycle from the residual r: v_0 = r / |r|, z = dinv v_0, the cells cleared (nh_gmres_init); `V` holds restart + 1 vectors'''
    _lib.call('nh_gmres_init', r.numel(), int(restart), device.ptr(dinv), device.ptr(r), device.ptr(V), device.ptr(z), device.ptr(work), device.stream())


def gmres_iterate(values, rowptr, colidx, ncols, *, rowmask, dinv, V, z, w, work, restart, stop_rr, niter, col32=None, lanes=0):
    '''enqueue `niter` Arnoldi steps (nh_gmres_iterate): nine launches each, nothing read back; they stop moving once the estimate is within stop_rr, the
    cycle is full or a direction has vanished'''
    _lib.call('nh_gmres_iterate', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(rowmask), device.ptr(dinv), device.ptr(V), device.ptr(z),
              device.ptr(w), device.ptr(work), int(restart), float(stop_rr), int(niter), device.stream())


def gmres_update(dinv, V, x, work, *, restart):
    '''x += dinv V y for the columns the cycle has taken (nh_gmres_update)'''
    _lib.call('nh_gmres_update', x.numel(), int(restart), device.ptr(dinv), device.ptr(V), device.ptr(x), device.ptr(work), device.stream())


# ---- smoothed-aggregation AMG and the CG it preconditions (nh_amg.hip) --------------------------------

def segment_dot(plan, a, b=None, out=None):
    '''out[s] = sum of a[ia[k]] * b[ib[k]] over the products of segment s of an expand-sort-compress plan (`amg.Plan`; nh_segment_dot); without `b` the
    segment sum of a[ia[k]]'''
    if out is None:
        out = device.empty(plan.nseg, 'float64')
    _lib.call('nh_segment_dot', plan.nseg, device.ptr(plan.ptr), device.ptr(plan.ia), device.ptr(plan.ib if b is not None else None), device.ptr(a), device.ptr(b),
              plan.nprod, device.ptr(out), device.stream())
    return out


def block_segment_dot(plan, a, b, out=None):
    '''the sparse product of a plan over blocks (`amg.BlockPlan`; nh_block_segment_dot): the output block (p x k) of segment s, at out[of[s] + r os[s] + c], is
    the sum over its products m of the block (p x q) at a[ia[m] + r sa[s] + t] times the block (q x k) at b[ib[m] + t sb[m] + c] (sb None: the stride
    plan.bstride).  `out`: plan.nout doubles when not given, zero where no block lies.  The indices are checked against the lengths of a, b and out here (one
    look at the device, the first time a plan meets arrays of these lengths): the kernel reads and writes where they point.'''
    import torch
    k, p, q, nseg, nprod = int(plan.k), int(plan.p), int(plan.q), int(plan.nseg), int(plan.nprod)
    if out is None:
        out = device.zeros(int(plan.nout), 'float64')
    for name, t in (('a', a), ('b', b), ('out', out)):
        if t.dim() != 1 or not t.is_contiguous() or str(t.dtype) != 'torch.float64':
            raise ValueError(f'block_segment_dot: {name} must be a contiguous float64 vector, got {tuple(t.shape)} {t.dtype}')
    i32 = lambda t, size: t is not None and str(t.dtype) == 'torch.int32' and t.numel() == size
    if str(plan.ptr.dtype) != 'torch.int64' or plan.ptr.numel() != nseg + 1 or not (i32(plan.ia, nprod) and i32(plan.ib, nprod) and i32(plan.of, nseg)):
        raise ValueError('block_segment_dot: ptr must be int64 [nseg + 1], ia and ib int32 [nprod], of int32 [nseg]')
    if p > 1 and not (i32(plan.sa, nseg) and i32(plan.os, nseg)):
        raise ValueError('block_segment_dot: blocks of several rows need sa and os, int32 [nseg]')
    if plan.sb is not None and not i32(plan.sb, nprod):
        raise ValueError('block_segment_dot: sb must be int32 [nprod]')
    lengths = a.numel(), b.numel(), out.numel()
    if 1 <= k <= 6 and p in (1, k) and q in (1, k) and nseg and nprod and getattr(plan, 'checked', None) != lengths:  # (the rest is the C entry's to refuse)
        i64 = lambda t: t.to(torch.int64)
        alast = i64(plan.ia) + (q - 1)
        if p > 1:  # the segment of every product, for the row stride of its first factor (clamped: a wrong ptr is found below, not followed)
            seg = torch.searchsorted(plan.ptr[1:].clamp(0, nprod).to(torch.int32), torch.arange(nprod, dtype=torch.int32, device=a.device), right=True, out_int32=True)
            alast += i64(plan.sa)[seg.clamp(max=nseg - 1).to(torch.int64)] * (p - 1)
        blast = i64(plan.ib) + (i64(plan.sb) if plan.sb is not None else int(plan.bstride)) * (q - 1) + (k - 1)
        olast = i64(plan.of) + (i64(plan.os) * (p - 1) if p > 1 else 0) + (k - 1)
        lowest = [plan.ia, plan.ib, plan.of, plan.ptr[1:] - plan.ptr[:-1]] + ([plan.sa, plan.os] if p > 1 else []) + ([plan.sb] if plan.sb is not None else [])
        first, last, lowest, *reach = torch.stack([plan.ptr[0], plan.ptr[-1], torch.stack([i64(t.min()) for t in lowest]).min(), alast.max(), blast.max(), olast.max()]).tolist()
        if first != 0 or last != nprod or lowest < 0:
            raise ValueError('block_segment_dot: ptr must rise from 0 to the number of products, and no index or stride may be negative')
        for name, entry, length in zip(('a', 'b', 'out'), reach, lengths):
            if entry >= length:
                raise ValueError(f'block_segment_dot: a block reaches entry {entry} of {name}, which has {length}')
        plan.checked = lengths  # (a plan is not written after it is made: the next numeric setup of these sizes does not look again)
    _lib.call('nh_block_segment_dot', k, p, q, nseg, device.ptr(plan.ptr), nprod, device.ptr(plan.ia), device.ptr(plan.ib), device.ptr(plan.sa if p > 1 else None),
              device.ptr(plan.sb), int(plan.bstride), device.ptr(plan.of), device.ptr(plan.os if p > 1 else None), device.ptr(a), device.ptr(b), device.ptr(out),
              device.stream())
    return out


def aggregate_qr(mptr, midx, k, B):
    '''(Q, Rc): the thin QR of the near-nullspace `B` [n x k] on the rows of every aggregate (nh_aggregate_qr).  Aggregate a has the rows
    midx[mptr[a] : mptr[a + 1]] (int64 pointers, int32 rows, every row in at most one aggregate); Q [n x k] is 0 on rows in none, Rc [nagg k x k] holds the
    triangles, the near-nullspace of the next level.  The member list is checked against n here (one look at the device): the kernel writes where it points.'''
    n, nagg, nmem = B.shape[0], mptr.numel() - 1, midx.numel()
    if B.dim() != 2 or B.shape[1] != k or not B.is_contiguous() or str(B.dtype) != 'torch.float64':
        raise ValueError(f'aggregate_qr: B must be a contiguous float64 tensor of shape (n, {k}), got {tuple(B.shape)} {B.dtype}')
    if str(mptr.dtype) != 'torch.int64' or str(midx.dtype) != 'torch.int32' or nagg < 0:
        raise ValueError('aggregate_qr: mptr must be int64 [nagg + 1] and midx int32')
    if nagg and not (int(mptr[0]) == 0 and int(mptr[-1]) == nmem and bool((mptr[1:] >= mptr[:-1]).all())):
        raise ValueError('aggregate_qr: mptr must rise from 0 to the number of members')
    if nmem and not (0 <= int(midx.min()) and int(midx.max()) < n):
        raise ValueError(f'aggregate_qr: member rows must lie in 0 .. {n - 1}')
    Q, Rc = device.empty(n * k, 'float64').reshape(n, k), device.empty(nagg * k * k, 'float64').reshape(nagg * k, k)
    _lib.call('nh_aggregate_qr', nagg, device.ptr(mptr), device.ptr(midx), nmem, int(k), n, device.ptr(B), device.ptr(Q), device.ptr(Rc), device.stream())
    return Q, Rc


def csr_jacobi(values, rowptr, colidx, ncols, x, w, b, *, y=None, rowmask=None, col32=None, lanes=0):
    '''y = x + w (b - A x) on the rows the mask keeps, 0 elsewhere, in one launch (nh_csr_jacobi)'''
    if y is None:
        y = device.empty(rowptr.numel() - 1, 'float64')
    _lib.call('nh_csr_jacobi', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(x), device.ptr(w), device.ptr(b), device.ptr(rowmask),
              device.ptr(y), device.stream())
    return y


def csr_chebyshev(values, rowptr, colidx, ncols, x, d, dinv, b, coef, *, y=None, dout=None, rowmask=None, col32=None, lanes=0):
    '''(y, dout): one step of the Chebyshev smoother in one launch (nh_csr_chebyshev): dout = c1 d + c2 dinv (b - A x), y = x + dout on the rows the mask keeps,
    0 elsewhere; `coef`: the device tensor (c1, c2).  d None: the first step of a polynomial, which reads neither d nor c1.  `dout` may be `d`.'''
    n = rowptr.numel() - 1
    if y is None:
        y = device.empty(n, 'float64')
    if dout is None:
        dout = device.empty(n, 'float64')
    _lib.call('nh_csr_chebyshev', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(x), device.ptr(d), device.ptr(dinv), device.ptr(b),
              device.ptr(coef), device.ptr(rowmask), device.ptr(y), device.ptr(dout), device.stream())
    return y, dout


def csr_lanczos(values, rowptr, colidx, ncols, s, u, steps, *, rowmask=None, col32=None, lanes=0):
    '''enqueue `steps` steps of the Lanczos recurrence on S A_f S, S = diag(s), from the start vector u (nh_csr_lanczos); returns the device tensor of
    2 steps + 1 doubles: alpha_j, beta_(j+1) in pairs, then the number of steps taken'''
    n = rowptr.numel() - 1
    out = device.empty(2 * int(steps) + 1, 'float64')
    work = device.empty(4 * n + _lib.LANCZOS_CELLS, 'float64')
    _lib.call('nh_csr_lanczos', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(s), device.ptr(rowmask), device.ptr(u), int(steps),
              device.ptr(work), device.ptr(out), device.stream())
    return out


class Amg:
    '''The handle of a hierarchy (nh_amg_create / nh_amg_free).  `levels`: one dict per level with A, and P, R for a coarsened level, as (values, rowptr,
    colidx, ncols, col32, lanes); rowmask, w, b, x, t, r, Ainv, idx: device tensors or None; kind: 'coarsen', 'dense' or 'diagonal'; sweeps; ndense.  A
    coarsened level with smoother='chebyshev' (default 'jacobi') also has degree, coef (2 degree doubles) and d, and w = 1 / diag.  The handle holds views:
    this object keeps the tensors alive.'''

    def __init__(self, levels):
        self._keep = levels
        self.n = levels[0]['A'][1].numel() - 1
        array = (_lib.AmgLevel * len(levels))()
        for lv, d in zip(array, levels):
            lv.A = _csr(*d['A'])
            for name in ('P', 'R'):
                if d.get(name) is not None:
                    setattr(lv, name, _csr(*d[name]))
            for name in ('rowmask', 'w', 'b', 'x', 't', 'r', 'Ainv', 'idx', 'coef', 'd'):
                setattr(lv, name + '_dev', device.ptr(d.get(name)))
            lv.kind, lv.sweeps, lv.ndense = _lib.AMG_KINDS[d['kind']], int(d.get('sweeps', 1)), int(d.get('ndense', 0))
            lv.smoother, lv.degree = _lib.AMG_SMOOTHERS[d.get('smoother', 'jacobi')], int(d.get('degree', 0))
            if lv.smoother and d['kind'] == 'coarsen' and (d['coef'].numel() != 2 * lv.degree or d['d'].numel() != d['A'][1].numel() - 1):
                raise ValueError(f'Amg: a Chebyshev level of degree {lv.degree} needs {2 * lv.degree} coefficients and a vector d of its size')  # (the cycle reads them unchecked)
        self._handle = ctypes.c_void_p()
        _lib.call('nh_amg_create', array, len(levels), ctypes.byref(self._handle))

    def __del__(self):
        handle, self._handle = getattr(self, '_handle', None), None
        if handle:
            _lib.load().nh_amg_free(handle)

    def apply(self, r, z=None):
        '''z = M r: one V-cycle, enqueued (nh_amg_apply)'''
        if z is None:
            z = device.empty(self.n, 'float64')
        _lib.call('nh_amg_apply', self._handle, device.ptr(r), device.ptr(z), device.stream())
        return z


def pcg_work():
    '''the work array of a CG solve with a cycle as its preconditioner (nh_pcg_work_doubles): [0] = r . r of the recurrence, [1] = breakdown flag, [2] = the
    bound of `cg_stop`'''
    return device.empty(_lib.load().nh_pcg_work_doubles(), 'float64')


def pcg_init(amg, r, z, p, work):
    '''z = M r, p = z, first r . z and r . r, flag and bound cleared (nh_pcg_init)'''
    _lib.call('nh_pcg_init', r.numel(), amg._handle, device.ptr(r), device.ptr(z), device.ptr(p), device.ptr(work), device.stream())


def pcg_iterate(values, rowptr, colidx, ncols, *, rowmask, amg, x, r, z, p, q, work, niter, col32=None, lanes=0):
    '''enqueue `niter` CG iterations preconditioned by the cycle of `amg` (nh_pcg_iterate): four launches and a cycle each, nothing read back; they stop
    moving once r . r is within the bound of `cg_stop`'''
    _lib.call('nh_pcg_iterate', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(rowmask), amg._handle, device.ptr(x), device.ptr(r),
              device.ptr(z), device.ptr(p), device.ptr(q), device.ptr(work), int(niter), device.stream())


def fgmres_iterate(values, rowptr, colidx, ncols, *, rowmask, amg, V, Z, z, t, w, work, restart, stop_rr, niter, col32=None, lanes=0):
    '''enqueue `niter` steps of flexible GMRES preconditioned by the cycle of `amg` (nh_fgmres_iterate): t = M z, Z[count] = t, then the Arnoldi step of
    `gmres_iterate` on A t; ten launches and a cycle each, nothing read back.  `V`: restart + 1 vectors, `Z`: restart; the cycle is started by
    `gmres_init(None, ...)` and ended by `gmres_update(None, Z, ...)`.  A step past a stop moves nothing but still runs its cycle into `t`.'''
    _lib.call('nh_fgmres_iterate', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(rowmask), amg._handle, device.ptr(V), device.ptr(Z),
              device.ptr(z), device.ptr(t), device.ptr(w), device.ptr(work), int(restart), float(stop_rr), int(niter), device.stream())


# ---- the block preconditioner of a saddle point (nh_amg.hip) -------------------------------------------

def csr_schur_diagonal(values, rowptr, colidx, ncols, vt, first, dinv, *, out=None, col32=None, lanes=0):
    '''out[i] = A_ii - sum over the entries k of row i with first[col[k]] of values[k] vt[k] dinv[col[k]] (nh_csr_schur_diagonal).  `vt`: the values of the
    transpose on the same pattern, `first`: a uint8 device vector, `dinv`: float64; all of the matrix's size, which the kernel takes for granted: checked here.'''
    n = rowptr.numel() - 1
    if n != int(ncols) or vt.numel() != values.numel() or first.numel() != n or dinv.numel() != n or str(first.dtype) != 'torch.uint8':
        raise ValueError(f'csr_schur_diagonal: a square matrix, transposed values of its length, a uint8 mask and an inverse diagonal of {n} entries are needed')
    if out is None:
        out = device.empty(n, 'float64')
    _lib.call('nh_csr_schur_diagonal', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(vt), device.ptr(first), device.ptr(dinv),
              device.ptr(out), device.stream())
    return out


class Schur:
    '''The handle of a block preconditioner (nh_schur_create / nh_schur_free).  `amg`: the `Amg` handle of the first block; `K`: (values, rowptr, colidx, ncols,
    col32, lanes); `mask1`: uint8, the first field's free dofs; `sinv`: float64, 1 / shat on the second field's free dofs and 0 elsewhere.  The handle holds
    views: this object keeps the tensors, the hierarchy's handle and its two scratch vectors alive.'''

    def __init__(self, amg, K, mask1, sinv):
        self.n = K[1].numel() - 1
        if amg.n != self.n or int(K[3]) != self.n or mask1.numel() != self.n or sinv.numel() != self.n or str(mask1.dtype) != 'torch.uint8' or str(sinv.dtype) != 'torch.float64':
            raise ValueError(f'Schur: a square matrix of {self.n} rows needs a hierarchy, a uint8 mask and a float64 vector of that size')
        self._keep = amg, K, mask1, sinv, device.empty(self.n, 'float64'), device.empty(self.n, 'float64')
        self._handle = ctypes.c_void_p()
        _lib.call('nh_schur_create', amg._handle, ctypes.byref(_csr(*K)), device.ptr(mask1), device.ptr(sinv), device.ptr(self._keep[4]), device.ptr(self._keep[5]),
                  ctypes.byref(self._handle))

    def __del__(self):
        handle, self._handle = getattr(self, '_handle', None), None
        if handle:
            _lib.load().nh_schur_free(handle)

    def apply(self, r, z=None):
        '''z = M r: sinv r, the masked product, the cycle of the first block, the sum; enqueued (nh_schur_apply)'''
        if z is None:
            z = device.empty(self.n, 'float64')
        _lib.call('nh_schur_apply', self._handle, device.ptr(r), device.ptr(z), device.stream())
        return z


def fgmres_iterate_schur(values, rowptr, colidx, ncols, *, rowmask, schur, V, Z, z, t, w, work, restart, stop_rr, niter, col32=None, lanes=0):
    '''`fgmres_iterate` with the application of a `Schur` handle in place of the cycle (nh_fgmres_iterate_schur): t = M z, Z[count] = t, then the Arnoldi step
    on A t; twelve launches, a product and a cycle each.  The matrix is that of the solve; the handle keeps the one it was built on.'''
    _lib.call('nh_fgmres_iterate_schur', ctypes.byref(_csr(values, rowptr, colidx, ncols, col32, lanes)), device.ptr(rowmask), schur._handle, device.ptr(V),
              device.ptr(Z), device.ptr(z), device.ptr(t), device.ptr(w), device.ptr(work), int(restart), float(stop_rr), int(niter), device.stream())
