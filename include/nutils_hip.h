/* nutils_hip.h -- C ABI of libnutils_hip.so, the MI355X (gfx950) element-integration
 * and sparse-assembly backend for Nutils.
 *
 * The reference (/root/reference, pure Python) has no FFI for this path: the work is
 * done by a generated numpy-per-element Python loop.  Each entry point below names the
 * reference code it replaces (paths relative to /root/reference/src/nutils).  The
 * boundary is plain C: opaque handles, device/host pointers, sizes, an int status
 * (0 = ok, negative = error, message via nh_last_error) -- the convention the reference
 * itself uses for its only native binding (matrix/_mkl.py:29-42,76-82), loaded with
 * ctypes like _util.py:195-237 (loadlib).
 *
 * Conventions
 *   - all "dev" pointers are HIP device pointers (hipMalloc / torch.cuda allocations);
 *     "host" pointers are ordinary memory.  `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream).  Calls are asynchronous on `stream` unless stated.
 *   - floating point data is IEEE f64 throughout (the reference computes in float64);
 *     index OUTPUTS are int64 (the reference's CSR index arrays are int64 and are
 *     compared bit-exactly); connectivity INPUTS are int32 on the device.
 *   - tabulated basis layout  T[fn][q][S], S = 1 + ndims: value, then d/dxi_j.
 *   - element-local ordering, dof numbering and CSR ordering follow the reference:
 *     CSR rows/cols sorted lexicographically, structural zeros retained, flat vector
 *     dof = scalar_dof * ncomp + comp (function.py:2598-2627).
 *   - thread model: one host thread per device context (the reference never threads;
 *     under NUTILS_NPROCS>1 it forks -- do not initialise before a fork).
 *   - library-owned state is per PROCESS, not per stream: the scratch of local matrices of NH_MATRIX_GATHER (grows to
 *     the largest pattern seen, 1.07 GB for the 128^3 trilinear mesh; nh_release_scratch() returns it), the staged
 *     basis tables of the thread-per-element passes and the parameter ring of nh_assemble_terms_multi are shared
 *     by all calls and carry no locks or events.  REQUIREMENT: all assembly entry points (nh_assemble_*, nh_p1hex_*,
 *     nh_p2hex_*) are issued from ONE host thread onto ONE stream at a time; only nh_index_copy, nh_memcpy_* and
 *     nh_monomial* (no library state) may run on a second stream beside them -- which is how nutils_amd/solver.py
 *     overlaps the copy of the Jacobian entries with the residual of the same step.
 */
#ifndef NUTILS_HIP_H
#define NUTILS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NH_OK 0
#define NH_EINVAL (-1)  /* invalid argument */
#define NH_EHIP (-2)    /* HIP runtime error (message has the HIP error string) */
#define NH_ELIMIT (-3)  /* problem exceeds a compiled-in limit of the kernel */
#define NH_ENOMEM (-4)

#define NH_ABI_VERSION 1

/* ---- runtime ------------------------------------------------------------------- */
int nh_abi_version(void);
const char *nh_last_error(void);
int nh_device_count(int *count);
int nh_set_device(int device);
/* name: caller buffer of namelen bytes; cus, lds_bytes, hbm_bytes may be NULL */
int nh_device_info(int device, char *name, size_t namelen, int *cus, int64_t *lds_bytes, int64_t *hbm_bytes);
int nh_malloc(void **dev, size_t bytes);
int nh_free(void *dev);
int nh_memcpy_h2d(void *dev, const void *host, size_t bytes, void *stream);
int nh_memcpy_d2h(void *host, const void *dev, size_t bytes, void *stream);
int nh_memset(void *dev, int byte, size_t bytes, void *stream);
int nh_stream_sync(void *stream);
int nh_release_scratch(void);  /* frees the library-owned scratch buffers (synchronises the device) */

/* ---- K2: basis tabulation -------------------------------------------------------
 * replaces nutils_poly eval_outer / GradPlan as called from generated code
 * (evaluable.py:4366-4374 Polyval, :4584-4653 PolyGrad).
 * coeffs[nfn][ncoeffs] in the reference coefficient order (evaluable.py:4331-4340),
 * points[nq][ndims]  ->  T[nfn][nq][1+ndims]. */
int nh_poly_tabulate(const double *coeffs_dev, int64_t nfn, int ncoeffs, const double *points_dev, int nq, int ndims,
                     double *T_dev, void *stream);

/* ---- K1: structured dof maps ----------------------------------------------------
 * replaces StructuredBasis.f_dofs_coeffs' integer part (function.py:3080-3093:
 * divmod unravel, Range + offsets, RavelIndex/Ravel).  shape[ndims] elements per axis
 * (element index: last axis fastest), start_dev[axis][shape[axis]] first dof per element
 * (concatenated over axes), per-axis dofs-per-element nloc[axis], per-axis dof counts
 * ndofs_axis[axis] (dofs wrap modulo ndofs_axis).  Output dofs[nelems][prod nloc] int32. */
int nh_structured_dofs(int ndims, const int *shape, const int *nloc, const int *ndofs_axis, const int *start_dev,
                       int64_t elem_begin, int64_t nelems, int32_t *dofs_dev, void *stream);

/* ---- K6: sparsity pattern --------------------------------------------------------
 * replaces Array.assparse's unique(flatindex) = ArgSort(stable)+UniqueMask+UniqueInverse
 * and as_csr's CompressIndices (evaluable.py:588-616, 5560-5682; numeric.py:687-711).
 * Builds the SCALAR pattern (rows = test dofs, cols = trial dofs) row-wise on the
 * device, plus the element map emap[e][m][n] = position of trial dof n of element e in
 * the sorted scalar row of test dof m.  Ragged bases pass offsets (prefix sums of dofs
 * per element, int64[nelems+1], host... see fields). */
typedef struct nh_pattern nh_pattern; /* opaque, owns device memory */

typedef struct {
  int64_t nelems;
  int64_t nrows, ncols;        /* scalar dof counts of test / trial basis */
  int nbt, nbr;                /* dofs per element if uniform; 0 if ragged (use offsets) */
  const int32_t *tdofs_dev;    /* test dofs, concatenated per element */
  const int32_t *rdofs_dev;    /* trial dofs (may alias tdofs_dev) */
  const int64_t *toff_dev;     /* ragged: int64[nelems+1] prefix sums, else NULL */
  const int64_t *roff_dev;
} nh_pattern_args;

int nh_pattern_build(const nh_pattern_args *args, nh_pattern **out, void *stream);
int nh_pattern_free(nh_pattern *p);
/* scalar nnz, and device pointers owned by the pattern (valid until nh_pattern_free);
 * eoff (ragged bases only, else NULL): int64[nelems+1] prefix sums of nbt_e*nbr_e indexing emap */
int nh_pattern_info(const nh_pattern *p, int64_t *nnz_scalar, const int64_t **srowptr_dev, const int32_t **scolidx_dev,
                    const int32_t **emap_dev, int64_t *emap_len, const int64_t **eoff_dev);
/* Expanded CSR index arrays for nct x ncr components with block mask[nct][ncr] (host,
 * nonzero = block present; NULL = all): rowptr_dev int64[nrows*nct+1], colidx_dev
 * int64[nnz]; nnz returned by nh_pattern_expanded_nnz.  Hand-back format of
 * matrix/__init__.py:30-70 (assemble_csr) -- indices int64, rows sorted, cols strictly
 * increasing within a row. */
/* owner blocks of NH_MATRIX_FUSED built for this pattern so far: number of row blocks (0: none yet, or the plan does not apply), rows of the largest
 * block, element visits over all blocks (>= nelems: elements on block borders are recomputed), and the element routine of the last fused
 * launch: -1 none yet, 0 the tabulated any-element routine, 1 / 2 the sum-factorised routine for trilinear hexahedra at the 2 x 2 x 2 Gauss
 * points (recognised from the tables of the launch; 2: with a mass term) */
int nh_pattern_fused_info(const nh_pattern *p, int *nblocks, int *rows_per_block, int64_t *nvisits, int *routine);
/* kernel launches of the term-list entries (nh_assemble_terms, nh_assemble_terms_multi, nh_assemble_matrix_terms) since the library was loaded, per
 * process and per kernel family: [0] k_terms, [1] k_terms_multi, [2] k_local_vterms2 (lane per element, residuals), [3] k_mterms, [4] k_local_terms,
 * [5] k_local_terms2 (thread-per-element passes in front of the owner-side reduction).  Read only: nothing in the library depends on the counts; a test
 * takes the difference around a call to see which family served it. */
int nh_terms_launch_counts(int64_t counts[6]);
/* the same for the element kernels of nh_assemble_matrix / nh_assemble_vector (the thread passes, owner blocks and write-once kernels these entries may route
 * to are not counted): counts [0] k_matrix_mfma, [1] k_matrix_generic, [2] k_gram_sym, [3] k_vector_generic, and what the launcher chose for the LAST launch
 * of each family: last[0..4] k_matrix_mfma ND, MT (M tiles), nt (N tiles), kt (k-steps), nas (active test slots); last[5..9] k_matrix_generic branch of the
 * element loop (0 entries, 1 scalar symmetric, 2 Gram, 3 Gram symmetric), waves per element, use_w, qchunk (< nq: the points are taken in chunks), sym;
 * last[10..14] k_gram_sym E (elements per workgroup), W (waves), NC, USE0, TRI; last[15] k_vector_generic qchunk.  Read only. */
int nh_generic_launch_record(int64_t counts[4], int32_t last[16]);
/* row tasks of NH_MATRIX_FUSED for vector-valued blocks built for this pattern so far (nh_owner.hip): row blocks (0: none yet, or the plan does not
 * apply), node rows per block, element visits of all blocks, chunks of 64 contributions */
int nh_pattern_owner_info(const nh_pattern *p, int *nblocks, int *rows_per_block, int64_t *nvisits, int64_t *nchunks);
/* The owner plan of vector-valued blocks keeps the vertex numbers of its visiting elements, made from the connectivity of an isoparametric geometry and
 * keyed on the address of that array.  After the array was refilled at the same address, this marks them stale: the next NH_MATRIX_FUSED launch remakes
 * them (one kernel on the stream of that launch, no synchronisation). */
int nh_pattern_forget_connectivity(nh_pattern *p);
int nh_pattern_expanded_nnz(const nh_pattern *p, int nct, int ncr, const unsigned char *mask, int64_t *nnz);
int nh_pattern_expand(const nh_pattern *p, int nct, int ncr, const unsigned char *mask, int64_t *rowptr_dev,
                      int64_t *colidx_dev, void *stream);

/* Union of up to 8 sorted-unique CSR patterns with the same number of rows (the per-sample matrices of one integral: volume + Nitsche / Robin
 * boundary terms; replaces the unique of evaluable.py:5560-5682 over the concatenated keys): a row of the union is the merge of the parts' sorted
 * column lists -- no sort.  nh_pattern_union_count fills rowptr_u_dev [nrows + 1] and returns the union's nnz (host, synchronises the stream);
 * nh_pattern_union_fill writes colidx_u_dev [nnz] and, for every entry k of part i, its position pos_dev[i][k] in the union. */
int nh_pattern_union_count(int nparts, int64_t nrows, const int64_t *const *rowptr_dev, const int64_t *const *colidx_dev, int64_t *rowptr_u_dev, int64_t *nnz, void *stream);
int nh_pattern_union_fill(int nparts, int64_t nrows, const int64_t *const *rowptr_dev, const int64_t *const *colidx_dev, const int64_t *rowptr_u_dev, int64_t *colidx_u_dev,
                          int64_t *const *pos_dev, void *stream);

/* ---- geometry descriptor ---------------------------------------------------------
 * replaces _TransformsCoords/_Jacobian lowering + numeric.inv + linalg.det
 * (function.py:1162-1181,1284-1295; evaluable.py:1403-1490; numeric.py:221-241). */
#define NH_GEOM_ISO 1    /* x = sum_a N_a(xi) X[gdofs[e][a]]; gT = tabulated geometry basis [ngb][nq][S] */
#define NH_GEOM_BOX 2    /* x = origin[e] + size[e] * xi  (axis aligned; rectilinear + hierarchical refinements) */
#define NH_GEOM_TAB 3    /* Jacobian (and coordinates) tabulated per element and point by the producer of the mesh: geometries
                            the kernels do not evaluate themselves (NURBS maps through transform chains, trimmed cells ...) */

typedef struct {
  int kind;
  int ngb;                   /* ISO: geometry basis functions per element (uniform) */
  const double *gT_dev;      /* ISO: [ngb][nq][S] */
  const int32_t *gdofs_dev;  /* ISO: [nelems][ngb] */
  const double *verts_dev;   /* ISO: [nverts][ndims] */
  const double *origin_dev;  /* BOX: [nelems][ndims] */
  const double *size_dev;    /* BOX: [nelems][ndims] */
  const double *jac_dev;     /* TAB: [nelems][nq][ndims][ndims]  d x_i / d xi_j */
  const double *x_dev;       /* TAB: [nelems][nq][ndims] or NULL (only needed by nh_sample_eval) */
  int bnd_axis;              /* -1: volume measure |det J|.  a >= 0: the points lie on the reference face xi_a = const and the
                                measure is the surface measure |det J| |J^-T e_a| (boundary integrals, topology.boundary) */
} nh_geometry;

/* ---- basis-on-elements descriptor ------------------------------------------------ */
typedef struct {
  int nb;                    /* functions per element if uniform, 0 if ragged */
  const double *T_dev;       /* tabulated functions [nfn][nq][S] */
  const int32_t *dofs_dev;   /* concatenated element dofs */
  const int64_t *off_dev;    /* ragged: int64[nelems+1] (dofs AND first-function offsets), else NULL */
  const int32_t *tab_dev;    /* uniform nb, several tables: table index per element (first fn = tab*nb); NULL = table 0.
                                Ragged: ignored (first function of element e = off[e]). */
} nh_basis;

/* ---- K3+K4+K5: matrix assembly ---------------------------------------------------
 * replaces the generated element loop (evaluable.py:6773-6786) for a bilinear integrand
 *   A[(m,c),(n,d)] = sum_q w_q |det J_q| sum_{a,b} Dt[q,m,a] C[c,a,d,b] Dr[q,n,b]
 * (D[.,.,0] = value, D[.,.,1+i] = d/dx_i: Basis.lower function.py:2758-2762, _Gradient
 * :1221-1231; einsum contraction evaluable.py:1885-1886, 6414-6505; sample.py:951-956)
 * and the scatter/accumulate of its sparse dedup (evaluable.py:603-605; numeric.accumulate
 * numeric.py:434-460) into `values_dev` laid out by the pattern. values are ACCUMULATED:
 * zero them first (nh_memset) for a fresh assembly. */
typedef struct {
  int64_t nelems;
  const int32_t *elist_dev;  /* optional element subset (bucket), NULL = 0..nelems-1; nelems counts the list */
  int ndims, nq;
  const double *weights_dev; /* [nq] */
  nh_geometry geom;
  nh_basis test, trial;
  int nct, ncr;              /* components of test / trial field */
  const double *C_host;      /* [nct][S][ncr][S] constant coefficient tensor (host memory) */
  const unsigned char *mask_host; /* [nct][ncr] block mask used for the pattern, NULL = all */
  const int64_t *srowptr_dev;/* scalar pattern */
  const int32_t *emap_dev;   /* element map from nh_pattern_info */
  const int64_t *eoff_dev;   /* ragged: int64[nelems+1] prefix sums of nbt_e*nbr_e, else NULL */
  double *values_dev;        /* [nnz of the expanded pattern] */
  const double *scale_dev;   /* optional pointwise factor of the integrand [nelems][nq] (a coefficient function evaluated at
                                the quadrature points), NULL = 1.  With elist_dev, scale and emap are indexed by LIST position. */
  int flags;                 /* NH_MATRIX_* bits */
  const double *cq_dev;      /* optional coefficient tensor PER QUADRATURE POINT, [nelems][nq][nct][S][ncr][S] (indexed like scale_dev),
                                replacing C_host (which then only provides the block mask): forms whose coefficients depend on a
                                field and its gradient at the point -- the product-rule term kappa'(u) phi_n grad u . grad phi_m
                                of a Newton Jacobian, advection with a computed velocity.  NULL = constant form. */
  int grid_shape[3];         /* NH_MATRIX_FIRST_TOUCH: elements per axis of the structured mesh (element id = last axis fastest) */
  int nodes_per_axis;        /* NH_MATRIX_FIRST_TOUCH: p + 1 local nodes per axis of the C0 ('std') basis, local order first axis slowest */
  const nh_pattern *pattern; /* optional: the handle the pattern pointers above come from.  With ragged bases (hierarchical / imported:
                                PlainBasis function.py:2881-2913) and no elist_dev the elements are launched per SIZE CLASS of the pattern
                                (functions per element <= 8, 16, 24, 32, 48, 64 ...), each class with the LDS footprint of its own largest
                                element; scale_dev / cq_dev stay indexed by element.  NULL: one launch sized by the largest element. */
} nh_matrix_args;

#define NH_MATRIX_EXCLUSIVE 1        /* no two elements of this launch touch the same CSR entry (one colour of an element
                                        colouring): entries are added with plain loads/stores -- deterministic -- not atomics */
#define NH_MATRIX_EMAP_BY_ELEMENT 2  /* with elist_dev: emap (and the pattern) cover ALL elements, index it by element id */
#define NH_MATRIX_NO_MFMA 4          /* force the generic one-wave-per-element VALU kernel */
#define NH_MATRIX_FIRST_TOUCH 32     /* with EXCLUSIVE | EMAP_BY_ELEMENT, colours = element index parities launched in lexicographic order
                                        (last axis fastest) on a FRESH value array of a structured C0 basis (grid_shape, nodes_per_axis):
                                        an entry whose two nodes do not both lie on a face shared with an element of an earlier colour is
                                        STORED, not added -- the caller does not zero-fill the values, and the ~70 % of the entries that
                                        receive a single contribution are not read */

#define NH_MATRIX_GATHER 64          /* deterministic owner-side reduction instead of atomics (needs `pattern`, all elements of the pattern in one
                                        call): the local matrices go to a scratch array, element by element, and every CSR entry is then
                                        summed ONCE over its contributions in ascending (element, m, n) order -- the order in which the
                                        reference's numpy.add.at / numeric.accumulate adds them (numeric.py:434-460, evaluable.py:603-605),
                                        so repeated assemblies are bit-identical.  The gather map is built on the first such call and cached
                                        in the pattern handle (one device sort of the element map). */

#define NH_MATRIX_STORE 128          /* with NH_MATRIX_GATHER or NH_MATRIX_FUSED: the sums are STORED, values_dev is not read (first term on a
                                        fresh array: no zero fill, no read-modify-write) */

#define NH_MATRIX_FUSED 256          /* owner blocks: ONE pass without scratch array or global atomics (needs `pattern`, all of its elements in
                                        one call, no elist, test and trial on one dof array).  The dofs are clustered by the Morton code of the
                                        centroid of the first element that contains them; Morton boxes of at most R rows form a block, and a
                                        block recomputes what it needs of every element touching one of its rows and writes each of its CSR rows
                                        once.  SCALAR blocks on small uniform bases (2 .. 9 functions per element): the rows of a block are ONE
                                        set of accumulators in LDS; the visiting elements add their local matrices in TURNS -- turn t holds the
                                        t-th visitor of every row in ascending (element, m) order, so no two threads meet in a row, a workgroup
                                        barrier separates the turns -- which is the order of NH_MATRIX_GATHER, i.e. of the reference's
                                        numpy.add.at: bit-identical to the gather path, 1.4 x the algorithmic bytes instead of 4.6 x.  Trilinear hexahedra at
                                        the 2 x 2 x 2 Gauss points with a form kappa grad.grad + mass phi phi (recognised from the tables passed)
                                        take the sum-factorised element routine of nh_p1hex_laplace (an exactly singular element then gives inf /
                                        NaN instead of numeric.inv's all-NaN inverse).  VECTOR-VALUED blocks (nct = ncr = 2 or 3 on trilinear
                                        hexahedra, bilinear or biquadratic quadrilaterals, one table set for test and trial): LDS holds the
                                        physical gradients of the visiting elements, a lane sums the Gram matrix of one contribution (element,
                                        m, n), a segmented sum over the lanes of a scalar entry forms it once and the form tensor is applied per
                                        entry (nh_owner.hip).  Every sum is formed in an order fixed by the plan: repeated assemblies are
                                        bit-identical.  The plan is built on the first such call and cached in the pattern handle.  Launches the
                                        flag does not apply to take the default path (atomics; with NH_MATRIX_STORE after a zero fill of the
                                        block's values). */

int nh_assemble_matrix(const nh_matrix_args *args, void *stream);

/* ---- vector / functional assembly, point evaluation --------------------------------
 * r[(m,c)] += sum_q w_q |det J_q| sum_a Dt[q,m,a] F[q,c,a],
 * F[q,c,a] = f[c][a] + sum_{d,b} C[c,a,d,b] U[q,d,b],  U[q,d,b] = sum_n Dr[q,n,b] u[rdofs[n]][d]
 * replaces Inflate/Assemble scatter (evaluable.py:3341-3495, 3552-3645; numpy.add.at /
 * numeric.accumulate) of a linear-form element loop.  With out_scalar_dev != NULL also
 * accumulates the functional  sum_q w|J| (f0 + 1/2 sum U[q,c,a] (C U)[q,c,a])  there
 * (Sample.integrate of a scalar, sample.py:160-175).  u_dev / C_host may be NULL. */
typedef struct {
  int64_t nelems;
  const int32_t *elist_dev;
  int ndims, nq;
  const double *weights_dev;
  nh_geometry geom;
  nh_basis test, trial;
  int nct, ncr;
  const double *C_host;      /* [nct][S][ncr][S] or NULL */
  const double *f_host;      /* [nct][S] constant source or NULL */
  const double *u_dev;       /* [ncols][ncr] trial coefficients or NULL */
  double *out_dev;           /* [nrows][nct] accumulated, or NULL */
  double f0;                 /* constant integrand of the functional */
  double *out_scalar_dev;    /* [1] accumulated, or NULL */
  const double *scale_dev;   /* optional pointwise factor [nelems][nq] (list position with elist_dev), NULL = 1 */
  double *local_dev;         /* NULL, or: local vectors stored element-major instead of atomics into out_dev (see nh_block.local_dev) */
} nh_vector_args;

int nh_assemble_vector(const nh_vector_args *args, void *stream);

/* ---- fused linear-form assembly: all terms of a residual in ONE element loop ----------
 * The reference evaluates the derivative of a functional as ONE generated element loop per
 * block (evaluable.py:6773-6786 with the Inflate/Assemble scatter :3341-3495; solver.py:334-386
 * assembles the residual of every trial block per Newton step): every term of the integrand
 * is evaluated at the same points inside that loop.  nh_assemble_terms is that loop:
 *   r_blk[(m,c)] += sum_q w_q |det J_q| sum_a Dt_blk[q,m,a] sum_{terms t of blk} g_t(q) F_t[q,c,a],
 *   F_t[q,c,a] = f_t[c][a] + sum_{d,b} C_t[c,a,d,b] U_{field(t)}[q,d,b],
 *   g_t(q)     = scale_t[e][q] * poly_t(values of up to 4 scalar fields at q)      (each factor optional)
 * for up to 2 output blocks (test spaces with their own out vector: the residual blocks of a
 * multi-field system), 6 fields and 32 terms sharing one sample (element list, points,
 * geometry).  Several elements are processed per workgroup (lanes over (element, point), then
 * over (element, test function)), so bases with few functions per element do not leave lanes idle
 * the way the one-wave-per-element kernel of nh_assemble_vector does.  Replaces one
 * nh_assemble_vector launch per term plus the nh_sample_eval / nh_pointwise_poly passes that
 * produced their scale arrays. */
typedef struct {
  nh_basis basis;
  const double *u_dev;       /* [ndofs][ncomp] coefficients */
  int ncomp;
} nh_field;

typedef struct {
  nh_basis test;
  int nct;                   /* components of the test space */
  double *out_dev;           /* [nrows][nct], accumulated */
  double *local_dev;         /* NULL, or: the local vectors are STORED here, element-major ([position of (e, m) in test.dofs_dev][nct]), instead of
                                being added into out_dev with atomics -- the first half of the deterministic scatter, see nh_scatter_plan_build */
} nh_block;

typedef struct {
  int nvars, nterms;         /* value = sum_t coeffs[t] prod_v x_v^powers[t][v], x_v = value of component comp[v] of fields[field[v]] at the point */
  int field[4], comp[4];
  const double *coeffs_host; /* [nterms] */
  const int *powers_host;    /* [nterms][nvars] */
} nh_point_poly;

typedef struct {
  int block;                 /* output block */
  int field;                 /* field the form is applied to, -1: source term (f only) */
  int poly;                  /* pointwise polynomial factor, -1: none */
  const double *C_host;      /* [nct][S][ncr][S] or NULL */
  const double *f_host;      /* [nct][S] or NULL */
  const double *scale_dev;   /* [nelems][nq] (list position with elist_dev) or NULL */
  int qs_field_t, qs_field_r; /* with qs_B_host: the term is also multiplied by s_q = sum_ab B[a][b] U_t[q,a] U_r[q,b] of two scalar fields */
  const double *qs_B_host;   /* [S][S] or NULL (the point factor of energy Hessians: d2/du2 of kappa(u) |grad u|^2 / 2 and the like) */
} nh_term;

typedef struct {
  int64_t nelems;
  const int32_t *elist_dev;
  int ndims, nq;
  const double *weights_dev;
  nh_geometry geom;
  int nfields;
  const nh_field *fields;
  int nblocks;
  const nh_block *blocks;
  int nterms;
  const nh_term *terms;
  int npolys;
  const nh_point_poly *polys;
} nh_terms_args;

int nh_assemble_terms(const nh_terms_args *args, void *stream);
/* The term lists of several samples (the volume sample and the sides of the boundary of one residual: the reference fuses all loops of
 * equal length under one id, evaluable.py:6841-6895, but still runs one loop per sample) in ONE launch: every list gets a range of
 * workgroups.  Same result as `count` nh_assemble_terms calls (the outputs are accumulated either way); lists of another dimension than
 * the first, lists of 2^14 elements and more (which may take the lane-per-element kernel) and lists beyond the eighth are launched on their own. */
int nh_assemble_terms_multi(int count, const nh_terms_args *const *lists, void *stream);

/* ---- fused bilinear-form assembly: all matrix terms of a block in ONE element loop ----------
 * Counterpart of nh_assemble_terms for the Jacobian blocks of a Newton step (solver.py:334-386;
 * derivative of the residual, evaluable.py:5693-5751): all terms share test / trial basis and the
 * pattern, their coefficient tensors are summed PER POINT inside the kernel,
 *   A[(m,c),(n,d)] += sum_q w_q |det J_q| sum_{a,b} Dt[q,m,a] Cq[q][c,a,d,b] Dr[q,n,b],  Cq = sum_t g_t(q) C_t(q),
 * with g_t as in nh_assemble_terms (scale array, pointwise polynomial of field values) and C_t(q)
 *   kind 0: the constant tensor C_host,
 *   kind 1: scalar fields, Cq[a][0] += sum_b B[a][b] U_field[q][b]         (product-rule term on the value slot of the trial function)
 *   kind 2: scalar fields, Cq[a][b] += L[a] sum_x B[x][b] U_field[q][x]    (product-rule term on the test side)
 * (kinds 1, 2: the per-point tensors that nh_matrix_args.cq_dev takes from the caller, here evaluated in the kernel: the terms
 * kappa'(u) phi_n grad u . grad phi_m of a quasi-linear Jacobian.)  Several elements per workgroup: lanes over (element, point) for the
 * pointwise part, over (element, m, n) for the contraction.  values are ACCUMULATED with the layout of nh_assemble_matrix. */
typedef struct {
  int kind;                  /* 0, 1, 2 (above) */
  int field;                 /* kinds 1, 2: the field U; else -1 */
  int poly;                  /* pointwise polynomial factor, -1: none */
  const double *C_host;      /* [nct][S][ncr][S]: C (kind 0) or B (kinds 1, 2) */
  const double *L_host;      /* kind 2: [nct][S] */
  const double *scale_dev;   /* [nelems][nq] or NULL; indexed like emap: by list position, with NH_MATRIX_EMAP_BY_ELEMENT by element */
  int qs_field_t, qs_field_r; /* as in nh_term */
  const double *qs_B_host;
} nh_matrix_term;

typedef struct {
  int64_t nelems;
  const int32_t *elist_dev;
  int ndims, nq;
  const double *weights_dev;
  nh_geometry geom;
  nh_basis test, trial;
  int nct, ncr;
  const unsigned char *mask_host; /* [nct][ncr] block mask used for the pattern, NULL = all */
  const int64_t *srowptr_dev;
  const int32_t *emap_dev;
  const int64_t *eoff_dev;
  double *values_dev;
  int flags;                 /* NH_MATRIX_EMAP_BY_ELEMENT, NH_MATRIX_GATHER, NH_MATRIX_STORE */
  int nfields;
  const nh_field *fields;
  int nterms;
  const nh_matrix_term *terms;
  int npolys;
  const nh_point_poly *polys;
  const nh_pattern *pattern; /* optional pattern handle: with NH_MATRIX_GATHER (| NH_MATRIX_STORE) in flags, scalar blocks on small uniform bases
                                (2 x 2 ... 9 x 9 local matrices, at most two scalar fields on the test basis: its tables AND its dof array) are assembled by a thread-per-element
                                pass + the owner-side reduction of nh_assemble_matrix; other blocks ignore NH_MATRIX_GATHER */
} nh_matrix_terms_args;

int nh_assemble_matrix_terms(const nh_matrix_terms_args *args, void *stream);

/* Sample.eval / bind (sample.py:192-232, _ConcatenatePoints.lower :966-975;
 * LoopConcatenate evaluable.py:5383-5508): values at all quadrature points, element
 * major.  Any output may be NULL.  x[e][q][ndims], detj[e][q],
 * U[e][q][ncr][S] (value and physical gradient of the field u). */
typedef struct {
  int64_t nelems;
  const int32_t *elist_dev;  /* optional element subset, NULL = 0..nelems-1; outputs are indexed by list position */
  int ndims, nq;
  nh_geometry geom;
  nh_basis trial;
  int ncr;
  const double *points_dev;  /* [nq][ndims] reference coordinates (needed for BOX geometry x) */
  const double *u_dev;
  double *x_dev, *detj_dev, *U_dev;
} nh_eval_args;

int nh_sample_eval(const nh_eval_args *args, void *stream);

/* ---- fast path: structured P1 hexahedra, scalar Laplace ----------------------------
 * Same result as nh_pattern_* + nh_assemble_matrix for the 3-D trilinear 'std' basis on
 * mesh.rectilinear (mesh.py:34-60; StructuredBasis function.py:3080-3100) with 2-point
 * Gauss per axis and isoparametric P1 (or uniform) geometry, but WRITE-ONCE: each
 * workgroup owns a column tile of dof rows, recomputes the element matrices that touch it,
 * reduces them in LDS and streams the finished CSR rows to HBM -- no global atomics, no
 * zero-fill, no element map.  The pattern is the reference's (sorted unique, structural
 * zeros kept; (3n+1)^3 law) in closed form: nh_p1hex_pattern writes rowptr (re-based to
 * row_begin, row_end-row_begin+1 entries) and colidx for rows [row_begin, row_end).
 * layer_*: element layers along axis 0 that contribute values; plane_*: dof planes along
 * axis 0 whose rows are written (multi-GPU slabs, nutils_amd/partition.py); values_dev
 * is indexed with the offsets of the FULL local mesh pattern. */
typedef struct {
  int shape[3];
  int layer_begin, layer_end;
  int plane_begin, plane_end;
  const double *verts_dev;   /* [(n0+1)(n1+1)(n2+1)][3]; NULL: x = origin + scale * vertex index */
  double origin[3], scale[3];
  double gauss_x[2], gauss_w[2]; /* 1-D Gauss points / weights on [0,1].  The points must be symmetric about 1/2 (gauss_x[0] +
                                    gauss_x[1] = 1 to 1e-14, as those of the 2-point Gauss rule are): the element routine uses it,
                                    and every entry that takes this struct returns NH_EINVAL for any other rule */
  double kappa;                  /* constant diffusivity */
  double *values_dev;
  const double *unit_matrix_dev; /* uniform geometry only: the 8x8 element matrix from nh_p1hex_unit_matrix (computed once per
                                    mesh, like the reference hoists it out of the loop); NULL: evaluated inside the call */
  const double *qscale_dev;      /* NULL, or [nelems][8]: coefficient at the Gauss points of every element (element index last
                                    axis fastest, points first coordinate slowest) multiplying kappa -- a scale_dev array of
                                    nh_assemble_matrix (variable or field-dependent diffusivity).  Needs verts_dev. */
  double mass;                   /* constant coefficient of an additional mass term mass * phi_m phi_n (0: stiffness only) */
  const double *qmass_dev;       /* NULL, or [nelems][8] like qscale_dev: mass coefficient at the Gauss points (multiplies `mass`,
                                    which must then be nonzero, e.g. 1) */
  int max_workgroups;            /* 0: one persistent workgroup per CU.  > 0: upper bound -- a multi-GPU caller leaves a few CUs to
                                    the RCCL send/recv kernels that run concurrently (a workgroup here takes a whole CU's LDS,
                                    so nothing else can start on a CU it occupies) */
} nh_p1hex_args;

int nh_p1hex_pattern(const int *shape, int64_t row_begin, int64_t row_end, int64_t *rowptr_dev, int64_t *colidx_dev, void *stream);
int nh_p1hex_laplace(const nh_p1hex_args *args, void *stream);
/* out (+)= K u for the same form, without the matrix: the element matrices are applied to the nodal values u_dev[ndofs] on the fly
 * and reduced row-wise (residual / matrix-free product; replaces the Inflate + numpy.add.at scatter of a vector-valued LoopSum,
 * evaluable.py:3405-3411).  Rows of the planes [plane_begin, plane_end) are written (accumulate = 0) or added to (1); needs
 * verts_dev; values_dev and unit_matrix_dev are ignored. */
int nh_p1hex_apply(const nh_p1hex_args *args, const double *u_dev, double *out_dev, int accumulate, void *stream);
/* element matrix (64 doubles, row major) of the uniform cell scale[0] x scale[1] x scale[2] (verts_dev ignored) */
int nh_p1hex_unit_matrix(const nh_p1hex_args *args, double *ke_dev, void *stream);

/* ---- fast path: structured C0 quadratic hexahedra, constant-coefficient forms, scalar or vector valued ------------------
 * Same result as nh_pattern_* + nh_assemble_matrix for the 3-D 'std' degree-2 basis (27 nodes per element, local order first axis
 * slowest: StructuredBasis function.py:3080-3100, mesh.py:34-60) of a full structured mesh, test = trial basis with ncomp
 * components, constant tensor C (BASELINE.json configs[2]: examples/elasticity.py stiffness scaled to 3-D), but WRITE-ONCE: a
 * workgroup owns K-lines of nodes, recomputes for every touching element only the rows it owns -- as (4 nodes x slots) x
 * (16 nodes) x (quadrature points) products on v_mfma_f64_16x16x4_f64, the form tensor applied to the 3x3 / 4x4 slot blocks
 * afterwards --, reduces in LDS row buffers laid out like the CSR rows and streams finished node planes to HBM.  No global
 * atomics, no zero-fill, no element map; the sorted-unique pattern of this basis is closed form (nh_p2hex_rowptr: scalar row
 * pointer of a node; per axis node X couples to [X-2, X+2] (X even) or [X-1, X+1] (X odd), clipped).  values_dev is laid out as
 * by nh_pattern_expand with all ncomp x ncomp blocks present.
 * owner_begin..owner_end (inclusive): lines of owner cells along axis 0 whose rows are written (owner io holds the node planes
 * 2 io and 2 io + 1; io = shape[0] holds the last plane); layer_begin..layer_end: element layers along axis 0 that contribute
 * (multi-GPU slabs, nutils_amd/partition.py).  Returns NH_ELIMIT when the tables do not fit the LDS (nq too large): use
 * nh_assemble_matrix. */
typedef struct {
  int shape[3];
  int nq;
  const double *weights_dev; /* [nq] */
  nh_geometry geom;
  const double *T_dev;       /* tabulated basis [27][nq][4] (one table: all elements of a 'std' basis share it) */
  int ncomp;                 /* components of the test = trial field, 1..3 */
  const double *C_host;      /* [ncomp][4][ncomp][4] (host memory) */
  double *values_dev;
  const double *scale_dev;   /* optional pointwise factor [nelems][nq], NULL = 1 */
  int layer_begin, layer_end;
  int owner_begin, owner_end;
  int max_workgroups;        /* 0: one persistent workgroup per CU */
  int weights_positive;      /* nonzero: every quadrature weight is > 0 (the caller owns the array and knows): the kernel that forms its operands in registers
                                carries sqrt(w |J|) on both of them; 0: signed weights, the table kernels */
} nh_p2hex_args;

int nh_p2hex_matrix(const nh_p2hex_args *args, void *stream);
int nh_p2hex_rowptr(const int *shape, int64_t node, int64_t *rowptr_out);
/* Meshes of UNIFORM cells (mesh.rectilinear with equidistant vertices: x = offset + scale * (multi-index + xi), mesh.py:45-52) with a constant form and no pointwise
 * factor: all element matrices are equal (the reference evaluates the same numbers for every element), so the rows of a node depend only on its class per axis (first,
 * odd, even, last) and equal the rows of the node of that class in a mesh of 2 x 2 x 2 such cells.  cell_values_dev: the values of nh_p2hex_matrix for shape {2, 2, 2}
 * on those cells (nh_p2hex_rowptr({2,2,2}, 125) * ncomp^2 doubles); this call replicates them into values_dev for the node planes [plane_begin, plane_end) of axis 0
 * (all of them: 0 .. 2 shape[0] + 1): a pure write stream.  Same layout and result as nh_p2hex_matrix on the box geometry of the same cells. */
int nh_p2hex_rows_uniform(const int *shape, int ncomp, const double *cell_values_dev, double *values_dev, int plane_begin, int plane_end, void *stream);
/* closed-form CSR index arrays of the component-expanded pattern (all ncomp x ncomp blocks): rowptr_dev int64[nnodes*ncomp+1],
 * colidx_dev int64[nh_p2hex_rowptr(shape, nnodes) * ncomp^2]; equal to nh_pattern_build + nh_pattern_expand for this basis */
int nh_p2hex_pattern(const int *shape, int ncomp, int64_t *rowptr_dev, int64_t *colidx_dev, void *stream);

/* ---- fast path: structured 2-D tensor-product bases on quadrilaterals, constant-coefficient forms, scalar or vector valued ---------
 * Same result (within rounding) as nh_pattern_* + nh_assemble_matrix for the 'std' basis of degree 1 or 2 and the 'spline' basis of degree 2
 * (StructuredBasis function.py:3030-3100, no periodic axis) of a full 2-D structured topology, test = trial basis with ncomp components and
 * all ncomp x ncomp blocks present, a constant tensor C (examples/laplace.py, poisson.py, elasticity.py), but WRITE-ONCE: a workgroup owns a
 * tile of node lines x nodes, evaluates the geometry of every element touching it into LDS, forms each of its rows in the registers of one
 * lane, and streams the tile's rows -- contiguous in the value array, one segment per line -- with coalesced stores.  No global atomics, no
 * zero-fill, no element map; repeated calls are bit-identical.
 * Pattern (closed form): per axis with n elements, 'std' degree p: dof X couples to [X-p, X+p] if X % p == 0, else to [p (X/p), p (X/p) + p],
 * clipped to [0, n p]; 'spline': to [max(0, X-p), min(n+p-1, X+p)]; a row is the Kronecker product of the two ranges (axis 0 slowest),
 * components as in nh_pattern_expand.  btype: 0 = 'std', 1 = 'spline'.  nh_quad_nnz is a host computation (no device). */
typedef struct {
  int shape[2];
  int btype, degree;         /* ('std', 1), ('std', 2), ('spline', 2) */
  int nq;
  const double *weights_dev; /* [nq] */
  nh_geometry geom;          /* ISO: gT_dev = the bilinear 'std' table [4][nq][3], verts_dev [(n0+1)(n1+1)][2] (vertex (i, j) at i (n1+1) + j; gdofs_dev
                                unused); BOX: size_dev [nelems][2] (element index last axis fastest).  bnd_axis must be -1. */
  const double *T_dev;       /* [nclass0 * nclass1][(p+1)^2][nq][3]: tabulated functions of every element class (class = c0 * nclass1 + c1) */
  int nclass[2];             /* classes per axis (StructuredBasis.nclasses_axis) */
  const int32_t *class0_dev, *class1_dev; /* per-axis class of every element (StructuredBasis.axis_class); may be NULL for an axis of one class */
  int ncomp;                 /* 1 or 2 */
  const double *C_host;      /* [ncomp][3][ncomp][3] (host memory) */
  double *values_dev;        /* [nh_quad_nnz] */
  int max_workgroups;        /* 0: one workgroup per tile; > 0: at most that many (they stride over the tiles) */
} nh_quad_args;

int nh_quad_nnz(const int *shape, int btype, int degree, int ncomp, int64_t *nnz);
/* rowptr_dev int64[ndofs * ncomp + 1], colidx_dev int64[nh_quad_nnz]; equal to nh_pattern_build + nh_pattern_expand (all blocks) */
int nh_quad_pattern(const int *shape, int btype, int degree, int ncomp, int64_t *rowptr_dev, int64_t *colidx_dev, void *stream);
/* values of the form; NH_ELIMIT when the geometric factors of a tile do not fit the LDS (too many quadrature points): use nh_assemble_matrix */
int nh_quad_matrix(const nh_quad_args *args, void *stream);
/* Meshes of UNIFORM cells (equidistant rectilinear vertices), constant form: the rows of a dof depend only on its place per axis (head, one
 * period of the interior, tail), all of which a small mesh holds -- 2 elements per axis for 'std', 3p-1 for splines (fewer when the mesh is
 * smaller: then it is the mesh).  nh_quad_uniform_shape gives that shape; small_values_dev: nh_quad_matrix on the small mesh of the same cells
 * (classes of the first / last elements per axis as in the big mesh); nh_quad_rows_uniform replicates its rows into values_dev: a pure write
 * stream with the layout of nh_quad_matrix. */
int nh_quad_uniform_shape(const int *shape, int btype, int degree, int *small_shape);
int nh_quad_rows_uniform(const int *shape, int btype, int degree, int ncomp, const double *small_values_dev, double *values_dev, void *stream);

/* ---- fast path: the trilinear 'std' basis of a full 3-D structured topology, constant-coefficient forms, 1-3 components -------------------
 * Same result (within rounding) as nh_pattern_* + nh_assemble_matrix for the 'std' basis of degree 1 (no periodic axis), test = trial basis
 * with ncomp components and all ncomp x ncomp blocks present, a constant tensor C (3-D linear elasticity, anisotropic diffusion), but
 * WRITE-ONCE: a workgroup owns a column of 2 x 2 nodes over a chunk of node planes, forms the Gram G_mn = sum_q w|J| D_m D_n^T of every element
 * under it (one element layer at a time, in LDS), sums the Grams of the elements that share a node pair in a fixed order, applies C and streams
 * the rows out with coalesced stores.  No global atomics, no zero-fill, no element map; repeated calls are bit-identical.
 * Pattern (closed form): node X of an axis with N = n + 1 nodes couples to [max(0, X-1), min(N-1, X+1)]; a row is the Kronecker product of the
 * three ranges (axis 0 slowest), components as in nh_pattern_expand.  nh_hex1_nnz is a host computation (no device). */
typedef struct {
  int shape[3];
  int nq;
  const double *weights_dev; /* [nq] */
  nh_geometry geom;          /* ISO: verts_dev [(n0+1)(n1+1)(n2+1)][3] (lexicographic; the map is the basis itself, T_dev serves as its table: gT_dev,
                                gdofs_dev unused);
                                BOX: size_dev [nelems][3] (element index last axis fastest).  bnd_axis must be -1. */
  const double *T_dev;       /* [8][nq][4]: tabulated functions of the basis */
  int ncomp;                 /* 1, 2 or 3 */
  const double *C_host;      /* [ncomp][4][ncomp][4] (host memory) */
  double *values_dev;        /* [nh_hex1_nnz] */
} nh_hex1_args;

int nh_hex1_nnz(const int *shape, int ncomp, int64_t *nnz);
/* rowptr_dev int64[(n0+1)(n1+1)(n2+1) ncomp + 1], colidx_dev int64[nh_hex1_nnz]; equal to nh_pattern_build + nh_pattern_expand (all blocks) */
int nh_hex1_pattern(const int *shape, int ncomp, int64_t *rowptr_dev, int64_t *colidx_dev, void *stream);
/* values of the form; NH_ELIMIT when the tables of the quadrature do not fit the LDS: use nh_assemble_matrix */
int nh_hex1_matrix(const nh_hex1_args *args, void *stream);
/* Meshes of UNIFORM cells (equidistant rectilinear vertices), constant form: the rows of a node depend only on its class per axis (first,
 * interior, last), all of which the mesh of min(n, 2) elements per axis holds.  small_values_dev: nh_hex1_matrix on that mesh of the same
 * cells; nh_hex1_rows_uniform replicates its rows into values_dev: a pure write stream with the layout of nh_hex1_matrix. */
int nh_hex1_rows_uniform(const int *shape, int ncomp, const double *small_values_dev, double *values_dev, void *stream);

/* ---- Monomial: evaluation of factored (pre-integrated) polynomial functionals -------------
 * replaces evaluable.Monomial (evaluable.py:5693-5751; `out = values.copy(); out *= arg[index]`
 * + Inflate/add.at), the per-Newton-step work after evaluable.factor (evaluable.py:5785-5874)
 * has evaluated the sparse Taylor coefficient tensors once with the element loop above.
 * nh_monomial_csr: y[r] += alpha * sum_k values[k] x[colidx[k]] over CSR row r (rank-2 tensor,
 *   deterministic, no atomics).
 * nh_monomial: out[out_index[i]] += alpha values[i] prod_k args[k][indices[k][i]], nargs <= 4;
 *   out_index NULL: scalar result accumulated in out[0].  args_dev / indices_dev are HOST arrays
 *   of device pointers. */
int nh_monomial_csr(int64_t nrows, const int64_t *rowptr_dev, const int64_t *colidx_dev, const double *values_dev, const double *x_dev,
                    double alpha, double *y_dev, void *stream);
int nh_monomial(int64_t n, const double *values_dev, int nargs, const double *const *args_dev, const int64_t *const *indices_dev,
                const int64_t *out_index_dev, double alpha, double *out_dev, void *stream);

/* ---- building the Taylor coefficient tensors of rank 3 and 4 ---------------------------------
 * replaces the one-time element loop + sparse dedup of evaluable.factor (evaluable.py:5785-5874: `zeroed.assparse`, zeros pruned) for value
 * polynomials of ONE scalar field, c int s(x) u^k dV -> C_k[i1..ik] = coeff int s N_i1 .. N_ik dV: every permutation stored, entries sorted by
 * (i1, .., ik) lexicographically, exact zeros dropped -- the arrays evaluable.Monomial holds (evaluable.py:5693-5751) and nh_monomial consumes.
 * nh_factor_tensor builds the tensor and reports its length; nh_factor_fetch copies it into caller-owned buffers (values[nnz], indices[rank][nnz])
 * and releases the library's copy.  One build at a time (the single-stream contract of the scratch buffers): a second build replaces the first, a fetch
 * without a build fails.  A build without elements, or one whose entries all cancel, leaves a tensor of length 0: its fetch takes NULL buffers. */
typedef struct {
  int64_t nelems;
  const int32_t *elist_dev;  /* optional element subset; scale_dev is indexed by list position */
  int ndims, nq, rank;       /* rank 3 or 4 */
  const double *weights_dev; /* [nq] */
  nh_geometry geom;
  nh_basis basis;            /* uniform nb */
  const double *scale_dev;   /* [nelems][nq] coefficient function at the points, or NULL */
  double coeff;              /* constant factor */
  int64_t ndofs;             /* length of the field's coefficient vector; ndofs^rank must fit 63 bits */
} nh_factor_args;
int nh_factor_tensor(const nh_factor_args *args, int64_t *nnz, void *stream);
int nh_factor_fetch(double *values_dev, int64_t *indices_dev, void *stream);

/* ---- block merge / submatrix: indexed copy of CSR values -----------------------------------
 * dst[dst_index[i]] = src[src_index[i]] (an index array may be NULL: i), plain stores, no accumulation.  The value half of
 * matrix.assemble_block_csr (matrix/__init__.py:103-151: the positions of every block entry in the merged matrix are fixed once
 * per system) and of Matrix.submatrix(free, free) (solver.py:332,386).  `dst` is device memory OR page-locked host memory that is
 * mapped into the device (hipHostMalloc / a pinned torch tensor): a Newton step then sends only the entries of the field-dependent
 * blocks over PCIe, straight into their places of the host CSR value array. */
int nh_index_copy(int64_t n, const double *src_dev, const int64_t *src_index_dev, const int64_t *dst_index_dev, double *dst, void *stream);

/* ---- pointwise coefficient functions ------------------------------------------------------
 * out[i] = sum_t coeffs[t] prod_v x_v[i*strides[v]]^powers[t*nvars+v]  (nvars <= 4, nterms <= 32;
 * x_dev is a HOST array of device pointers).  Evaluates polynomial coefficient functions of field
 * values at the quadrature points (from nh_sample_eval), e.g. psi'(phi), psi''(phi) of
 * examples/cahnhilliard.py:175-176, once per Newton step; the result is a scale_dev array.  The
 * reference represents such terms as rank-3/4 sparse tensors (evaluable.factor); here the
 * integrand is re-integrated with the pointwise coefficient. */
int nh_pointwise_poly(int64_t n, int nvars, const double *const *x_dev, const int *strides, int nterms, const double *coeffs,
                      const int *powers, double *out_dev, void *stream);

/* ---- deterministic vector scatter (owner-side reduction) ------------------------------------------
 * The reference scatters local vectors with numpy.add.at(out, dofs_e, values_e) element by element (Inflate._compile_with_out,
 * evaluable.py:3405-3411; numeric.accumulate, numeric.py:434-460): every dof receives its contributions in ascending (element, local
 * index) order.  Global atomics give the same sum in an arbitrary order, i.e. results that differ in the last bits from run to run.
 * Two-pass form with the reference's order: (1) the element kernels STORE their local vectors (nh_block.local_dev /
 * nh_vector_args.local_dev); (2) nh_scatter_gather sums, for every dof, its contributions through a map built once per (basis, element
 * list): positions of the (e, m) pairs in the local array, grouped by dof, within a dof ascending in (list position, m).
 * nelems / nb / off_dev / dofs_dev: the connectivity as in nh_basis (nb = 0: ragged with off_dev); elist_dev / nlist: the elements of the
 * sample in evaluation order (NULL: all nelems).  Several (plan, local) pairs -- the samples of one residual -- are summed in the order
 * given; accumulate = 0 stores, 1 adds to out_dev[nrows][ncomp]. */
typedef struct nh_scatter_plan nh_scatter_plan;
int nh_scatter_plan_build(int64_t nelems, int64_t nrows, int nb, const int32_t *dofs_dev, const int64_t *off_dev, const int32_t *elist_dev,
                          int64_t nlist, nh_scatter_plan **plan_out, void *stream);
int nh_scatter_plan_free(nh_scatter_plan *plan);
int nh_scatter_gather(int count, const nh_scatter_plan *const *plans, const double *const *locals_dev, int ncomp, double *out_dev,
                      int accumulate, void *stream);

/* ---- per-point forms of field values ------------------------------------------------------------
 * The product-rule coefficients of quasi-linear problems at every quadrature point, from U = (value, gradient w.r.t. x) of
 * the bound scalar field(s) there (nh_sample_eval; U[npoints][S], S = 1 + ndims):
 *   kind 0: out[i]       = sc_i sum_ab B[a][b] Ut[i][a] Ur[i][b]         (point factor of an energy: a scale_dev array)
 *   kind 1: out[i][a][b] = sc_i (b == 0 ? sum_x B[a][x] Ut[i][x] : 0)    (cq_dev of nh_assemble_matrix: g'(u) phi_n B(v, u))
 *   kind 2: out[i][a][b] = sc_i L[a] sum_x B[x][b] Ut[i][x]              (cq_dev: both one-sided tensors of an energy Hessian)
 * sc_i = scale_dev[i] or 1.  B_host [S][S], L_host [S] (kind 2).  Replaces what the reference obtains by differentiating the
 * evaluable graph (evaluable.py: `_derivative` of Multiply / Einsum nodes under function.derivative, function.py:1184-1196)
 * and evaluating the product inside the generated element loop. */
int nh_point_forms(int kind, int64_t npoints, int S, const double *Ut_dev, const double *Ur_dev, const double *B_host, const double *L_host,
                   const double *scale_dev, double *out_dev, void *stream);

/* ---- array-valued expressions of field values at the points of a sample ----------------------------
 * Sample.eval / Sample.bind (sample.py:192-232; _ConcatenatePoints.lower :966-975, _ReorderPoints :978-989) of a function that is a sum of
 * (constant coefficient tensor) x (product of values / gradients of bound fields and of coordinates) x (coefficient function of the point):
 *   out[i][f] (+)= sc_i sum_{t : out_index[t] == f} coef[t] prod_v x_v[i*strides[v] + offsets[t*nvars+v]],   f < nout, nvars <= 6.
 * x_dev: HOST array of nvars device pointers (U arrays of nh_sample_eval: stride ncomp*(1+ndims), offset comp*(1+ndims)+slot; coordinate
 * arrays: stride ndims, offset = axis); strides: HOST array.  out_index / offsets / coef: DEVICE tables of the nentries non-zeros of the
 * coefficient tensor, out_index ascending (an output that is met again later is added to).  scale_dev [npoints] or NULL.
 * accumulate = 0 stores (outputs without an entry become 0), 1 adds to out_dev[npoints][nout].  Replaces the reference's per-element
 * evaluation of the lowered function inside loop_concatenate (evaluable.py:5383-5508). */
int nh_point_expr(int64_t npoints, int nvars, const double *const *x_dev, const int64_t *strides, int64_t nentries, const int32_t *out_index_dev,
                  const int32_t *offsets_dev, const double *coef_dev, const double *scale_dev, int nout, double *out_dev, int accumulate, void *stream);

/* ---- rational bases (NURBS) ------------------------------------------------------------------
 * In-place transform of per-element tabulated functions T[(e, i)][q][S] (function (e,i) = e*nb+i, or off[e]+i for ragged bases)
 * into N_i = w_i B_i / W,  dN_i = w_i (dB_i W - B_i dW) / W^2  with the dof weights w[dofs[e][i]] and the weight function W
 * either tabulated (W_dev [nelems][nq], dW_dev [nelems][nq][ndims], derivatives w.r.t. the element coordinates) or, if
 * W_dev is NULL, W = sum_j w_j B_j of the element itself.  Replaces the symbolic quotient
 * `bsplinebasis * controlweights / weightfunc` (examples/platewithhole.py:71-72,85) evaluated inside the generated loop. */
int nh_rationalize(double *T_dev, int64_t nelems, int nb, const int64_t *off_dev, const int32_t *dofs_dev, const double *weights_dev,
                   const double *W_dev, const double *dW_dev, int nq, int ndims, void *stream);

/* ---- device-resident matrix: CSR product, diagonal, conjugate gradients ------------------------------
 * The matrix backend that fits the data of this library (the slot matrix/_mkl.py fills for the vendor library of the host): the
 * CSR triplet stays where the assembly left it, is multiplied there (Matrix.__matmul__, matrix/_base.py) and symmetric positive
 * definite systems are solved there (Matrix.solve with solver='cg'; constraints as a row mask instead of a submatrix).
 * nh_csr is a plain view: sizes and device pointers, nothing owned.  values f64, rowptr int64 [nrows + 1].  Column indices: col32_dev
 * (int32 [nnz], made once per matrix by nh_csr_compact; needs ncols <= INT32_MAX) if not NULL, else colidx_dev (the int64 [nnz] of the
 * assembly) -- 12 against 16 bytes per entry.  lanes: lanes of a wave that share a row, a power of two 1 .. 64; 0 = nh_csr_lanes(nrows,
 * nnz), two thirds of the mean row length rounded down to a power of two, at most 32.
 * Argument errors (NULL pointers, negative sizes, a bad `lanes`, int32 columns with ncols > INT32_MAX) return NH_EINVAL before
 * anything touches the device.  nrows == 0 succeeds without a launch; so does nnz == 0 where the result is known without one. */
typedef struct {
  int64_t nrows, ncols, nnz;
  const double *values_dev;
  const int64_t *rowptr_dev;
  const int64_t *colidx_dev;
  const int32_t *col32_dev;
  int lanes;
} nh_csr;

int nh_csr_lanes(int64_t nrows, int64_t nnz);  /* the rule behind lanes = 0 (host computation, returns the lane count) */
int nh_csr_compact(int64_t nnz, int64_t ncols, const int64_t *colidx_dev, int32_t *col32_dev, void *stream);
/* y = mask(alpha A x + beta b): rowmask_dev uint8 [nrows] or NULL, rows with mask 0 get y = 0 (their entries are not read); b_dev may be
 * NULL (no second term) and may be y_dev; x_dev must not overlap y_dev.  No atomics, and the launch geometry depends on (nrows, lanes)
 * only: repeated calls are bit-identical. */
int nh_csr_spmv(const nh_csr *A, double alpha, const double *x_dev, double beta, const double *b_dev, const unsigned char *rowmask_dev, double *y_dev, void *stream);
/* diag[i] = A_ii, 0 for a row without a diagonal entry (Matrix.diagonal) */
int nh_csr_diagonal(const nh_csr *A, double *diag_dev, void *stream);
/* The support of A above a tolerance (Matrix.rowsupp, matrix/_base.py): rowsupp[i] = 1 when row i holds an entry with |a| > tol (strictly; tol >= 0), else 0;
 * colsupp[j] likewise for column j.  uint8 [nrows] and [ncols]; either may be NULL.  The entry point zero-fills what it is given; a matrix without entries
 * is no launch.  Column indices int32 or int64 as for the product, and its rows-to-lanes mapping.  Several lanes may store the byte 1 to one address: plain
 * byte stores, no atomics, and the result, a set, is the same at every call. */
int nh_csr_support(const nh_csr *A, double tol, unsigned char *rowsupp_dev, unsigned char *colsupp_dev, void *stream);
/* ---- matrix algebra on the device (nh_csr_ops.hip): Matrix.T, Matrix.submatrix and sums of different patterns (matrix/_base.py) ----
 * Every operation returns index arrays and `pos`, the position in the operand of every entry of the result; the values are then
 * nh_index_copy(nnz, values, pos, NULL, values_result), and a later matrix on the same pattern needs only that copy.  All outputs are pure
 * functions of the inputs: repeated calls give identical arrays.  The rows of A hold their columns in ascending order (the triplet contract).
 *
 * nh_csr_transpose: the pattern of A^T.  rowptr_t_dev int64 [ncols + 1], colidx_t_dev and pos_dev int64 [nnz]; A->values_dev is not read and
 * may be NULL, A->lanes is not used.  Rows of A^T come out sorted by column (the source row) and, where a row of A repeats a column, in the
 * order of A.  pos is a permutation of 0 .. nnz - 1.  Phases: an int32 histogram of the columns (atomicAdd of ones; nrows <= INT32_MAX),
 * nh_scan_exclusive, one slot of its output row claimed per entry (int32 atomicAdd), every output row sorted by its unique keys -- the two
 * atomics cannot reach the result.  No floating point.  nnz is the caller's, so nothing is read back; the host waits only where
 * nh_scan_exclusive does, and once more when ncols > 2 nnz (the histogram then has a buffer of its own instead of living in pos_dev).
 * Output rows of up to 64 entries are sorted by one wave in registers, of 65 .. 2048 entries by a workgroup in LDS; a longer row takes a slow
 * path that is quadratic in its length over 2048 (pieces of 2048 sorted in LDS, ranks by binary search in the other pieces).
 *
 * nh_csr_select_count / nh_csr_select_fill: compaction by a predicate.  Entry k of row i is kept iff rowkeep_dev[i] != 0, colkeep_dev[col[k]] != 0
 * (uint8 [nrows] / [ncols]; NULL keeps all) and, if drop_zeros, values[k] != 0. (NaN is kept, -0. is not).  Kept rows and columns are numbered
 * densely in ascending order; entries keep their order in a row.  `count` writes newrow_dev int64 [nrows + 1] and newcol_dev int64 [ncols + 1], the
 * exclusive scans of the masks (NULL exactly where the mask is NULL), checks that the masks keep nrows_s rows and ncols_s columns -- what the
 * caller sized its arrays for; NH_EINVAL otherwise, before anything is written through them -- writes rowptr_s_dev int64 [nrows_s + 1] and
 * returns the number of kept entries in *nnz (host; synchronises the stream, the convention of nh_pattern_union_count).  `fill`, with the
 * same arguments and the arrays `count` wrote, writes colidx_s_dev and pos_dev, int64 [*nnz].  Lanes per row as in the product (A->lanes);
 * ranks within a row come from a wave vote per stride (__ballot, 64 bits).  No atomics.
 *
 * nh_csr_add_values: the values of a + sign b (sign 1. or -1.) on the union of two patterns, pos_a_dev / pos_b_dev being the positions of the
 * parts' entries in the union (nh_pattern_union_fill): out = 0, out[pos_a[k]] = a[k], out[pos_b[k]] += sign b[k].  Positions are unique within a
 * part: plain stores, no atomics.  out_dev double [nnz_u]. */
int nh_csr_transpose(const nh_csr *A, int64_t *rowptr_t_dev, int64_t *colidx_t_dev, int64_t *pos_dev, void *stream);
int nh_csr_select_count(const nh_csr *A, const unsigned char *rowkeep_dev, const unsigned char *colkeep_dev, int drop_zeros, int64_t nrows_s, int64_t ncols_s,
                        int64_t *newrow_dev, int64_t *newcol_dev, int64_t *rowptr_s_dev, int64_t *nnz, void *stream);
int nh_csr_select_fill(const nh_csr *A, const unsigned char *rowkeep_dev, const unsigned char *colkeep_dev, int drop_zeros, const int64_t *newrow_dev,
                       const int64_t *newcol_dev, const int64_t *rowptr_s_dev, int64_t *colidx_s_dev, int64_t *pos_dev, void *stream);
int nh_csr_add_values(int64_t nnz_a, const double *a_dev, const int64_t *pos_a_dev, int64_t nnz_b, const double *b_dev, const int64_t *pos_b_dev, double sign, int64_t nnz_u,
                      double *out_dev, void *stream);
/* Preconditioned conjugate gradients for square A, symmetric positive definite on the rows / columns the mask keeps, entirely on the
 * device: an iteration is three launches -- q = mask(A p) with partial sums of p . q per workgroup; alpha from the partials (summed by
 * every workgroup in the same order), x += alpha p, r -= alpha q, partials of r . z and r . r with z = dinv r; beta from those and
 * p = z + beta p -- and nothing is read back.  work_dev: nh_cg_work_doubles() doubles; after every iteration work[0] = r . r of the
 * recurrence and work[1] = the breakdown flag (0. / 1.): one 16-byte copy tells the host where the iteration stands.  work[2] is the
 * caller's to write after nh_cg_init (which sets it to 0.): the bound on r . r at or below which an iteration does no arithmetic and
 * raises no flag.  A caller that enqueues several iterations between two looks at work[0] sets it to its stopping bound: iterated past
 * convergence r . r falls through the subnormal range, where r . z or p . q is 0 before r . r is, a false breakdown.  The flag is raised
 * when r . r > work[2] and p . q or r . z is not a positive finite number (A or the preconditioner is not positive definite); from then
 * on the iterations leave x, r and p as they are.  dinv_dev: inverse diagonal (Jacobi) or NULL (none); it must be finite, and r and p
 * zero, on masked rows.  nh_cg_init forms p = z = dinv r and the first r . z, r . r from a given r and clears the flag and the bound;
 * nh_cg_iterate enqueues niter iterations. */
int64_t nh_cg_work_doubles(void);
int nh_cg_init(int64_t n, const double *dinv_dev, const double *r_dev, double *p_dev, double *work_dev, void *stream);
int nh_cg_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const double *dinv_dev, double *x_dev, double *r_dev, double *p_dev, double *q_dev,
                  double *work_dev, int niter, void *stream);
/* ---- several vectors at once (nh_csr_multi.hip): the product with a block of vectors, a batched CG ----
 * A block of vectors is row-major [n][k] with a leading dimension ld >= k in doubles: numpy's C order of an (n, k) array, a column slice of a wider block
 * being a view (its pointer and the wider block's ld).
 * nh_csr_spmm: Y = mask(alpha A X + beta B) for any k >= 1, by the rules of nh_csr_spmv (b_dev may be NULL and may be y_dev, x_dev must not overlap y_dev,
 * masked rows get zeros and their entries are not read, nothing atomic, repeated calls bit-identical).  Every (value, column) pair of the matrix is read once
 * per group of NH_MULTI_MAX columns and used for each of them; a remnant group neither reads nor writes past column k.  Rows of X are read two doubles at
 * a time where ldx is even and x_dev lies on a 16-byte boundary.  For every column the sums are formed in the order of nh_csr_spmv: column j of Y is, bit
 * for bit, the single-vector product of column j at the same lanes and index width.  nnz == 0 without b_dev zero-fills the k columns of every row (ldy
 * respected) without a launch.
 * nh_cgm_*: k <= NH_MULTI_MAX independent conjugate-gradient recurrences on one matrix, Jacobi-preconditioned (dinv_dev) or plain (NULL), by the rules of
 * nh_cg_* per column; x, r, p, q are blocks with ld = k, dinv and the row mask are shared.  An iteration is three launches that cover all columns: Q =
 * mask(A P) with the partials of p_j . q_j, the update, the direction.  work_dev: nh_cgm_work_doubles(k) doubles (-1 and an error for a k out of range).  The
 * head of the work array is the caller's:
 *   work[0 .. k)      r . r of each recurrence                                 (read)
 *   work[k .. 2k)     breakdown flags, 0. / 1.                                 (read)
 *   work[2k .. 3k)    iterations since nh_cgm_init that moved the column       (read; exact, whatever niter was)
 *   work[3k .. 4k)    the bounds on r . r, cleared by nh_cgm_init              (written by the caller after nh_cgm_init)
 * so one copy of 3k doubles tells the host where every column stands.  A column with r . r <= its bound idles as nh_cg_iterate does: no arithmetic, no flag,
 * p . q = 0 is no breakdown; a flagged column does no arithmetic on x, r, p either.  Idle columns still take part in the product: their p does not move, so
 * their q does not.  Column j of x, r, p after any number of iterations is, bit for bit, what nh_cg_* make of column j alone with the same bound.
 * Argument errors are NH_EINVAL (k < 1, ld < k, NULL vectors, a matrix that is not square, a negative niter) or NH_ELIMIT (k > NH_MULTI_MAX in nh_cgm_*). */
#define NH_MULTI_MAX 8
int nh_csr_spmm(const nh_csr *A, int k, double alpha, const double *x_dev, int64_t ldx, double beta, const double *b_dev, int64_t ldb,
                const unsigned char *rowmask_dev, double *y_dev, int64_t ldy, void *stream);
int64_t nh_cgm_work_doubles(int k);
int nh_cgm_init(int64_t n, int k, const double *dinv_dev, const double *r_dev, double *p_dev, double *work_dev, void *stream);
int nh_cgm_iterate(const nh_csr *A, int k, const unsigned char *rowmask_dev, const double *dinv_dev, double *x_dev, double *r_dev, double *p_dev, double *q_dev,
                   double *work_dev, int niter, void *stream);
/* Right-preconditioned BiCGStab for ANY square A (nonsymmetric, indefinite), M^-1 = dinv (Jacobi) or the identity (dinv_dev NULL), entirely on the
 * device and by the rules of the CG above: constraints are a row mask on which every vector vanishes, nothing is atomic, no scalar visits the host,
 * repeated solves are bit-identical.  An iteration is five launches: v = mask(A phat) with partial sums of rhat . v; alpha = rho / rhat . v, s = r - alpha v,
 * shat = dinv s, partials of s . s; t = mask(A shat) with partials of t . s and t . t; omega = t . s / t . t, x += alpha phat + omega shat, r = s - omega t,
 * partials of rhat . r and r . r; rho' = rhat . r, beta = (rho' / rho) (alpha / omega), p = r + beta (p - omega v), phat = dinv p.
 * nh_bicgstab_init takes a given r and sets rhat = p = r (the first direction), phat = dinv r, the scalars, work[0 .. 2]; it marks the iteration as finished if
 * r = 0.  nh_bicgstab_iterate enqueues niter iterations.  Once the recurrence has r . r <= stop_rr every remaining iteration, its products included, leaves all
 * vectors as they are (iterated past convergence BiCGStab drives rho to 0, a false breakdown).  work_dev: nh_bicgstab_work_doubles() doubles, of which the
 * host reads work[0] = r . r of the recurrence, work[1] = breakdown flag (0. / 1.), work[2] = iterations since nh_bicgstab_init that moved x (exact, whatever
 * niter was).  The flag is raised, with r != 0, when rho' is 0 or not finite, rhat . v is 0 or not finite, t . t = 0 or omega is 0 or not finite while s . s > stop_rr,
 * or alpha / beta overflow; x and r are then those of the last complete iteration and later iterations do no arithmetic (no 0 * inf).  No omega with
 * s . s <= stop_rr (t = 0, say) is convergence at the half step: omega = 0, x += alpha phat, r = s.  Vectors: x, r in/out; rhat, p, v, s, t, phat, shat belong to the
 * iteration between init and the last iterate; phat_dev / shat_dev are not used (and may be NULL) when dinv_dev is NULL; dinv must be finite on masked rows.
 * nh_csr_spmv_dots is the product of the iteration on its own: y = mask(A x), then work[0] = w . y and work[1] = y . y from the per-workgroup partials, summed
 * in the solver's order (work_dev: nh_bicgstab_work_doubles() doubles). */
int64_t nh_bicgstab_work_doubles(void);
int nh_csr_spmv_dots(const nh_csr *A, const double *x_dev, const double *w_dev, const unsigned char *rowmask_dev, double *y_dev, double *work_dev, void *stream);
int nh_bicgstab_init(int64_t n, const double *dinv_dev, const double *r_dev, double *rhat_dev, double *p_dev, double *phat_dev, double *work_dev, void *stream);
int nh_bicgstab_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const double *dinv_dev, double *x_dev, double *r_dev, const double *rhat_dev, double *p_dev,
                        double *v_dev, double *s_dev, double *t_dev, double *phat_dev, double *shat_dev, double *work_dev, double stop_rr, int niter, void *stream);
/* MINRES (Paige and Saunders) for SYMMETRIC square A, definite or not, preconditioned with M^-1 = dinv > 0 (the inverse of |diag|, say) or the identity (dinv_dev
 * NULL), entirely on the device and by the rules of the CG above: constraints are a row mask on which every vector vanishes, nothing is atomic, every sum in
 * a fixed order, no scalar visits the host, repeated solves are bit-identical.  One product and three launches an iteration, in the variable names of
 * scipy.sparse.linalg.minres: q = mask(A v) with the partials of v . q; alpha = v . q, r1 <- r2, r2 <- q - (beta / oldb) r1 - (alpha / beta) r2 (no r1 term in
 * the first step), partials of r2 . dinv r2; beta' = sqrt(r2 . dinv r2), the rotation, w1 <- w2, w2 <- (v - oldeps w1 - delta w2) / gamma, x += phi w2,
 * r <- sn^2 r - (phibar cs / beta') r2, v <- dinv r2 / beta', partials of r . r.  phibar is the norm of the residual in the M^-1-norm; r carries the residual itself,
 * since it is the 2-norm that stops the iteration.  Symmetry is not checked: on a nonsymmetric A the recurrence's r is not the residual of x.
 * nh_minres_init takes a given r (which stays the caller's: it becomes the carried residual) and sets r1 = r2 = r, w1 = w2 = 0, v = dinv r / sqrt(r . dinv r), the
 * scalars, work[0 .. 2]; it marks the iteration as finished if r = 0 and raises the flag if r . dinv r is not positive.  nh_minres_iterate enqueues niter
 * iterations and one small launch that sums r . r.  Once the recurrence has r . r <= stop_rr every remaining iteration leaves all vectors as they are, but for
 * the one product that follows the deciding step, which writes q and nothing else.  work_dev: nh_minres_work_doubles() doubles, of which the host reads
 * work[0] = r . r of the recurrence, work[1] = flag (0. / 1.), work[2] = iterations since nh_minres_init that moved x (exact, whatever niter was).  The flag is
 * raised, with r != 0, when a scalar is not finite, r2 . dinv r2 < 0 (dinv is not positive) or gamma = 0; x and r are then those of the last complete iteration
 * and later iterations do no arithmetic.  beta' = 0 with gamma > 0 is the Krylov space exhausted: the step is taken, r becomes 0, the iteration stops, no flag.
 * Vectors: x, r in/out; r1, r2, v, q, w1, w2 belong to the iteration between init and the last iterate; dinv must be finite on masked rows. */
int64_t nh_minres_work_doubles(void);
int nh_minres_init(int64_t n, const double *dinv_dev, const double *r_dev, double *r1_dev, double *r2_dev, double *v_dev, double *w1_dev, double *w2_dev, double *work_dev,
                   void *stream);
int nh_minres_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const double *dinv_dev, double *x_dev, double *r_dev, double *r1_dev, double *r2_dev, double *v_dev,
                      double *q_dev, double *w1_dev, double *w2_dev, double *work_dev, double stop_rr, int niter, void *stream);
/* Restarted GMRES for ANY square A, right-preconditioned with M^-1 = dinv (Jacobi) or the identity (dinv_dev NULL; with a fixed M this is also flexible GMRES),
 * entirely on the device and by the rules above: a row mask on which every vector vanishes, nothing atomic, every sum in a fixed order, no scalar visits the
 * host, repeated solves are bit-identical.  V_dev: restart + 1 basis vectors of n doubles, one after the other; z_dev, w_dev: n doubles; work_dev:
 * nh_gmres_work_doubles(restart) doubles (-1 and an error for restart < 1).  Of the work array the host reads work[0] = the squared residual norm of the
 * least-squares problem (after nh_gmres_init: r . r), work[1] = 1. once a new direction has vanished or was not finite, work[2] = the Arnoldi steps taken since
 * nh_gmres_init (exact, whatever niter was).
 * nh_gmres_init starts a cycle from a given r: v_0 = r / |r|, z = dinv v_0, g = |r| e_0; it marks the cycle as finished if r = 0.
 * nh_gmres_iterate enqueues niter Arnoldi steps of nine launches; the device knows which column it is at.  Step j: w = mask(A z); classical Gram-Schmidt
 * twice (the dots of w with v_0 .. v_j in one kernel that takes the basis vectors eight at a time, a small launch that sums the partials, w -= V h in one
 * kernel, the second time with the partials of w . w); one workgroup forms column j of the Hessenberg matrix from the two passes, applies the stored Givens
 * rotations, makes the new one, rotates g and writes work[0 .. 2]; v_(j+1) = w / h_(j+1,j), z = dinv v_(j+1).  The steps stop moving anything once
 * work[0] <= stop_rr, once restart columns are taken, or once a direction vanishes: |w| after the two passes within 2^-40 of |A z| before them.  With a pivot
 * left that is the lucky breakdown (the column is taken, work[0] = 0); with none (a zero column, say) or with a non-finite column the column is not taken.
 * nh_gmres_update forms x += dinv V y, y from the triangular system of the columns taken (one workgroup, then one kernel); whether the true residual is then
 * within the bound is the caller's to find out.  Vectors of even length on 16-byte boundaries are read and written two doubles at a time. */
int64_t nh_gmres_work_doubles(int restart);
int nh_gmres_init(int64_t n, int restart, const double *dinv_dev, const double *r_dev, double *V_dev, double *z_dev, double *work_dev, void *stream);
int nh_gmres_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const double *dinv_dev, double *V_dev, double *z_dev, double *w_dev, double *work_dev, int restart,
                     double stop_rr, int niter, void *stream);
int nh_gmres_update(int64_t n, int restart, const double *dinv_dev, const double *V_dev, double *x_dev, double *work_dev, void *stream);

/* ---- smoothed-aggregation AMG as the preconditioner of the CG solve (nh_amg.hip) ----------------------
 * The symbolic phase of the setup (aggregates, the patterns of P, R = P^T and A_c = R A P, and for each of the products A T, A P, R (A P) an
 * expand-sort-compress plan) is the caller's; these entries read value arrays.  By the rules above: nothing atomic, every sum in a fixed order, launch
 * geometry a function of sizes only, repeated calls bit-identical, argument errors NH_EINVAL before a launch, empty sizes no launch.
 * nh_segment_dot: out[s] = sum of a[ia[k]] * b[ib[k]] over k = ptr[s] .. ptr[s + 1] - 1, s < nseg; b_dev NULL: the plain segment sum of a[ia[k]].  ptr int64
 * [nseg + 1], ia / ib int32 [nprod], nprod = ptr[nseg].  Lanes per segment follow from the mean segment length by the rule of nh_csr_lanes.
 * nh_block_segment_dot: the same sum over blocks that lie in scalar value arrays, 1 <= k <= 6, p and q each 1 or k: segment s < nseg is the block (p x k) with
 * the entries out[of[s] + r os[s] + c], the sum over k' = ptr[s] .. ptr[s + 1] - 1, in that order and t ascending within, of a[ia[k'] + r sa[s] + t] *
 * b[ib[k'] + t sb[k'] + c], r < p, t < q, c < k.  ptr int64 [nseg + 1]; ia, ib, sb int32 [nprod]; sa, of, os int32 [nseg].  sa and os may be NULL for p = 1;
 * sb may be NULL for q = 1, and for q = k when every block of b has the row stride `bstride` >= k.  Every index must lie inside its array and the output
 * blocks must not overlap: that is the caller's to see to.  One lane per entry of an output block.
 * nh_aggregate_qr: the thin QR of a near-nullspace B_dev [n x k] row-major, 1 <= k <= 6, on the rows of every aggregate: aggregate a < nagg has the rows
 * midx[mptr[a]] .. midx[mptr[a + 1] - 1] (mptr int64 [nagg + 1], midx int32 [nmembers], nmembers = mptr[nagg]; every row below n, in at most one aggregate).
 * Q_dev [n x k] row-major gets the orthonormal columns on the rows of each aggregate and 0 on rows in none; Rc_dev [nagg k x k] row-major gets block a =
 * R of aggregate a, upper triangular with a non-negative diagonal, so that Q R = B on the aggregate's rows.  Columns left to right: n0 = |b_j|, two passes
 * of modified Gram-Schmidt against q_0 .. q_(j-1) with R[l][j] the sum of the two coefficients, n1 = |b_j| afterwards; n1 <= 2^-26 n0 drops the column
 * (q_j = 0 and R[j][j] = 0 exactly, R[l][j] kept), otherwise q_j /= n1 and R[j][j] = n1.  Lanes per aggregate follow from the mean size by the rule of
 * nh_csr_lanes.  Q_dev must not be B_dev.
 * nh_csr_jacobi: y = x + w (b - A x) on the rows the mask keeps, 0 on the others, in one launch; y must not be x.
 * nh_csr_chebyshev: one step of the Chebyshev smoother in one launch, on the mapping of nh_csr_jacobi: dout = c1 d + c2 dinv (b - A x), y = x + dout on the rows
 * the mask keeps, +0 in both on the others; coef_dev: the two doubles (c1, c2) on the device.  d_dev NULL is the first step of a polynomial, dout = c2 dinv
 * (b - A x): neither d nor c1 is read (there is no 0 * d).  y must not be x; dout may be d.
 * nh_csr_lanczos: `steps` >= 1 steps of the Lanczos recurrence on S A_f S, S = diag(s_dev) (s = sqrt(1 / diag), 0 where a row takes no part), enqueued: three
 * launches a step and two at the start, nothing read back.  q_0 = u0 / |u0| with u0 = u_dev on the rows the mask keeps and where s != 0, 0 elsewhere; step j:
 * w = s (mask(A (s q_j))) with the partials of q_j . w; alpha_j from them (summed by every workgroup in the same order), w -= alpha_j q_j + beta_j q_(j-1)
 * (beta_0 = 0: no q_(-1) is read) with the partials of w . w; beta_(j+1) = |w|, q_(j+1) = w / beta_(j+1) and s q_(j+1) for the next product.  out_dev: 2 steps
 * + 1 doubles, zero-filled first: out[2 j] = alpha_j, out[2 j + 1] = beta_(j+1), out[2 steps] = the number of steps taken.  A beta_(j+1) that is 0 or not
 * finite ends the recurrence with j + 1 steps taken (so does a start vector without a finite positive norm, with none); the launches after it idle.
 * work_dev: 4 n + NH_LANCZOS_CELLS doubles, the caller's, of no meaning afterwards.  n = 0: out is zero-filled, no launch.
 * nh_amg is a hierarchy made of level descriptions; like nh_csr it holds views and owns no device memory, and every vector of a description is the caller's
 * to allocate and to keep.  Level l < nlevels - 1 has kind NH_AMG_COARSEN: A (its matrix), rowmask_dev (level 0 only; NULL: all rows), w_dev = omega / diag
 * (0 on masked rows), P [n x n_c] and R = P^T [n_c x n] as CSR views of their own, sweeps >= 1, t_dev and r_dev: n doubles each; for l > 0 also b_dev and x_dev.
 * smoother = NH_AMG_CHEBYSHEV (NH_AMG_JACOBI = 0: a zero-filled tail is the Jacobi level above) makes the level's smoother the Chebyshev polynomial of
 * `degree` >= 1 steps: w_dev = 1 / diag (0 on masked rows, no omega), coef_dev: 2 degree doubles, (c1, c2) of step 0, 1, .. (c1 of step 0 is never read),
 * d_dev: n doubles, `sweeps` is not read.  Before the coarse correction x = d = c2 w b, then steps 1 .. degree - 1 of nh_csr_chebyshev; after it steps
 * 0 .. degree - 1, the first without d: the launches of a Jacobi level with sweeps = degree.
 * The last level is NH_AMG_DENSE -- Ainv_dev [ndense x ndense] row-major, ndense <= 1024; idx_dev int32 [ndense] lists the rows it acts on when ndense is
 * less than the rows of A (a masked level 0), whose other rows get 0 -- or NH_AMG_DIAGONAL, z = w b with w_dev = 1 / diag.
 * nh_amg_apply enqueues z = M r, one V(sweeps, sweeps) cycle from level 0, and returns: the first sweep x = w b, further ones x += w (b - A x), then
 * r = b - A x, b_c = R r, the cycle below, x += P x_c, and `sweeps` sweeps more.  With one sweep that is five launches a level.  r_dev and z_dev: n doubles, distinct.
 * nh_pcg_*: conjugate gradients with that cycle as the preconditioner.  An iteration: q = mask(A p) with the partials of p . q; alpha, x += alpha p,
 * r -= alpha q, partials of r . r; z = M r; partials of r . z; beta, p = z + beta p.  work_dev: nh_pcg_work_doubles() doubles; work[0 .. 2] are r . r, the
 * breakdown flag and the stopping bound with the meaning they have in nh_cg_*: once r . r <= work[2] no iteration moves x, r or p or raises the flag; a
 * p . q or r . z that is not a positive finite number while r . r > work[2] raises it and freezes the vectors.  nh_pcg_init forms z = M r, p = z and the
 * first r . z, r . r from a given r, and clears flag and bound.
 * nh_fgmres_iterate: flexible GMRES for ANY square A with that cycle as its preconditioner, on the vectors, the work array and the rules of nh_gmres_*: the
 * cycle is started by nh_gmres_init with dinv_dev NULL (v_0 = r / |r|, z a copy of it) and ended by nh_gmres_update(n, restart, NULL, Z_dev, x, work), which is
 * x += Z y.  Step j of the niter it enqueues: t = M z (the cycle of nh_amg_apply; the hierarchy may have been built on other values than A's: any linear or
 * nonlinear M will do, which is what "flexible" means); Z_j = t; w = mask(A t); the Gram-Schmidt passes, the scalars and v_(j+1) = w / h_(j+1,j), z = v_(j+1) of
 * nh_gmres_iterate: ten launches and a cycle.  V_dev: restart + 1 vectors of n doubles, Z_dev: restart; z_dev, t_dev, w_dev: n doubles, z_dev and t_dev distinct:
 * 2 restart + 1 basis vectors in all.  A step that finds the cycle stopped (work[0] <= stop_rr, restart columns taken, a direction vanished) leaves V, Z and the
 * work array alone; its V-cycle still runs, into t.  NULL hierarchy or vectors, a hierarchy of another size, restart < 1, negative niter or stop_rr and a
 * matrix that is not square are NH_EINVAL before a launch. */
typedef struct nh_amg nh_amg;
enum { NH_AMG_COARSEN = 0, NH_AMG_DENSE = 1, NH_AMG_DIAGONAL = 2 };
enum { NH_AMG_JACOBI = 0, NH_AMG_CHEBYSHEV = 1 };
enum { NH_LANCZOS_CELLS = 4096 };
typedef struct {
  nh_csr A;
  const unsigned char *rowmask_dev;
  const double *w_dev;
  nh_csr P, R;
  double *b_dev, *x_dev, *t_dev, *r_dev;
  int kind, sweeps;
  int64_t ndense;
  const double *Ainv_dev;
  const int32_t *idx_dev;
  int smoother, degree;
  const double *coef_dev;
  double *d_dev;
} nh_amg_level;

int nh_segment_dot(int64_t nseg, const int64_t *ptr_dev, const int32_t *ia_dev, const int32_t *ib_dev, const double *a_dev, const double *b_dev, int64_t nprod,
                   double *out_dev, void *stream);
int nh_block_segment_dot(int k, int p, int q, int64_t nseg, const int64_t *ptr_dev, int64_t nprod, const int32_t *ia_dev, const int32_t *ib_dev,
                         const int32_t *sa_dev, const int32_t *sb_dev, int bstride, const int32_t *of_dev, const int32_t *os_dev, const double *a_dev,
                         const double *b_dev, double *out_dev, void *stream);
int nh_aggregate_qr(int64_t nagg, const int64_t *mptr_dev, const int32_t *midx_dev, int64_t nmembers, int k, int64_t n, const double *B_dev, double *Q_dev,
                    double *Rc_dev, void *stream);
int nh_csr_jacobi(const nh_csr *A, const double *x_dev, const double *w_dev, const double *b_dev, const unsigned char *rowmask_dev, double *y_dev, void *stream);
int nh_csr_chebyshev(const nh_csr *A, const double *x_dev, const double *d_dev, const double *dinv_dev, const double *b_dev, const double *coef_dev,
                     const unsigned char *rowmask_dev, double *y_dev, double *dout_dev, void *stream);
int nh_csr_lanczos(const nh_csr *A, const double *s_dev, const unsigned char *rowmask_dev, const double *u_dev, int steps, double *work_dev, double *out_dev,
                   void *stream);
int nh_amg_create(const nh_amg_level *levels, int nlevels, nh_amg **out);
int nh_amg_free(nh_amg *amg);
int nh_amg_apply(const nh_amg *amg, const double *r_dev, double *z_dev, void *stream);
int64_t nh_pcg_work_doubles(void);
int nh_pcg_init(int64_t n, const nh_amg *amg, const double *r_dev, double *z_dev, double *p_dev, double *work_dev, void *stream);
int nh_pcg_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const nh_amg *amg, double *x_dev, double *r_dev, double *z_dev, double *p_dev, double *q_dev,
                   double *work_dev, int niter, void *stream);
int nh_fgmres_iterate(const nh_csr *A, const unsigned char *rowmask_dev, const nh_amg *amg, double *V_dev, double *Z_dev, double *z_dev, double *t_dev, double *w_dev,
                      double *work_dev, int restart, double stop_rr, int niter, void *stream);

/* ---- a block preconditioner for saddle-point systems K = [[A, Bt], [B, C]] (nh_amg.hip) ----------------------
 * The dofs are split into a first field (mask1) and a second; M is the block upper-triangular solve with the AMG cycle on the first block and a diagonal
 * approximation shat of the Schur complement on the second: z2 = sinv r, t = mask1(r - K z2), z1 = cycle(t), z = z1 + z2, all on vectors of n doubles.
 * nh_csr_schur_diagonal: out[i] = A_ii - sum over the entries k of row i with first[col[k]] != 0 of values[k] vt[k] dinv[col[k]], for every row of a square A;
 * vt_dev: the values of A^T on A's pattern (which must then be structurally symmetric: the caller's to see to), first_dev uint8 [n], dinv_dev double [n].  With
 * first the mask of the first field and dinv = 1 / diag there this is the SIMPLE diagonal of C - B diag(A)^-1 Bt on the rows of the second field.  The mapping
 * of nh_csr_spmv (A->lanes lanes per row, int32 or int64 columns), both sums folded in its order, nothing atomic: repeated calls are bit-identical.  A matrix
 * without entries is zero-filled without a launch.
 * nh_schur is a handle that holds views and owns no device memory: the hierarchy of the first block (built on K with the mask of the first field as its row
 * mask; it must outlive the handle), the view of K, mask1_dev uint8 [n], sinv_dev double [n] (1 / shat on the second field's free dofs, 0 elsewhere) and two
 * scratch vectors of n doubles, distinct.  nh_schur_apply enqueues z = M r: z2 = sinv r where sinv != 0 and +0 elsewhere (r is not read off the second field
 * there, nor on rows outside mask1 by the product), the masked product nh_csr_spmv(K, -1, z2, 1, r, mask1, t), the cycle of nh_amg_apply from t into z, and
 * z += z2: two launches, a product and a cycle.  r_dev and z_dev: n doubles, distinct, and neither a scratch vector of the handle.
 * nh_fgmres_iterate_schur is nh_fgmres_iterate with that application in place of the cycle: the same vectors, work array, rules and Arnoldi step; A is the
 * matrix of the solve, which may have other values than the K of the handle (a lagged preconditioner).  A NULL handle, matrix or vector, sizes that differ,
 * restart < 1, a negative niter or stop_rr and a matrix that is not square are NH_EINVAL before a launch. */
typedef struct nh_schur nh_schur;
int nh_csr_schur_diagonal(const nh_csr *A, const double *vt_dev, const unsigned char *first_dev, const double *dinv_dev, double *out_dev, void *stream);
int nh_schur_create(const nh_amg *first, const nh_csr *K, const unsigned char *mask1_dev, const double *sinv_dev, double *z2_dev, double *t_dev, nh_schur **out);
int nh_schur_free(nh_schur *schur);
int nh_schur_apply(const nh_schur *schur, const double *r_dev, double *z_dev, void *stream);
int nh_fgmres_iterate_schur(const nh_csr *A, const unsigned char *rowmask_dev, const nh_schur *schur, double *V_dev, double *Z_dev, double *z_dev, double *t_dev,
                            double *w_dev, double *work_dev, int restart, double stop_rr, int niter, void *stream);

#ifdef __cplusplus
}
#endif
#endif
