'''Symbolic side of the hot path, reduced to what the assembly kernels consume.

The reference lowers arbitrary ``function.Array`` expressions to an evaluable
graph and generates a Python loop (function.py:356-361, evaluable.py:6532-6838).
This backend accelerates the loop shapes named in SURVEY 8a -- integrals of
products of (derivatives of) basis functions / fields with constant coefficients
-- and represents exactly those: every operand is LINEAR in one argument (a basis
used as an array, or a named field, cf. ``function.field`` function.py:2598-2627)
and is stored as the constant tensor ``P[free..., comp, slot]`` that maps the
argument's value (slot 0) and physical gradient (slots 1..ndims) to the operand's
free axes.  Products of two operands give the coefficient tensor
``C[c, a, d, b]`` of nh_assemble_matrix.  Expressions outside this class raise
NotImplementedError (the reference path is the fallback for those, see
INTEGRATION.md) -- nothing is ever evaluated on the CPU here.
'''

import numpy


# ---- geometry ---------------------------------------------------------------------

class Geometry:
    '''A coordinate map usable as integration geometry / gradient reference.'''
    ndims: int


class RectilinearGeometry(Geometry):
    '''x = offset + scale * (element multi-index + xi): the geometry returned by
    mesh.rectilinear (mesh.py:45-52).'''

    def __init__(self, topo, offset, scale):
        self.topo = topo
        self.ndims = topo.ndims
        self.offset = numpy.asarray(offset, dtype=float)
        self.scale = numpy.asarray(scale, dtype=float)

    def element_boxes(self):
        idx = numpy.stack(numpy.meshgrid(*[numpy.arange(n, dtype=float) for n in self.topo.shape], indexing='ij'), -1).reshape(-1, self.ndims)
        origin = self.offset + self.scale * idx
        size = numpy.broadcast_to(self.scale, origin.shape)
        return origin, size


class BoxGeometry(Geometry):
    '''Axis-aligned box per element (hierarchically refined rectilinear meshes).'''

    def __init__(self, origin, size):
        self.origin = numpy.ascontiguousarray(origin, dtype=float)
        self.size = numpy.ascontiguousarray(size, dtype=float)
        self.ndims = self.origin.shape[1]

    def element_boxes(self):
        return self.origin, self.size


class GradedGeometry(BoxGeometry):
    '''mesh.rectilinear with non-uniform vertex arrays (mesh.py:34-60): boxes, plus the per-axis vertices for the structured kernels.'''

    def __init__(self, topo, axes):
        self.topo = topo
        self.axes = [numpy.asarray(v, dtype=float) for v in axes]
        idx = numpy.stack(numpy.meshgrid(*[numpy.arange(n) for n in topo.shape], indexing='ij'), -1).reshape(-1, topo.ndims)  # element order: last axis fastest
        super().__init__(numpy.stack([v[idx[:, i]] for i, v in enumerate(self.axes)], 1), numpy.stack([numpy.diff(v)[idx[:, i]] for i, v in enumerate(self.axes)], 1))

    def vertices(self):
        return numpy.stack(numpy.meshgrid(*self.axes, indexing='ij'), -1).reshape(-1, self.ndims)


class IsoGeometry(Geometry):
    '''x = sum_a N_a(xi) X_a  (``geom = gbasis @ verts`` in a Nutils script).'''

    def __init__(self, basis, verts):
        verts = numpy.asarray(verts, dtype=float)
        if verts.ndim != 2 or verts.shape[0] != basis.ndofs or verts.shape[1] != basis.ndims:
            raise ValueError(f'vertex array of shape {verts.shape} does not match basis ({basis.ndofs} dofs, {basis.ndims} dims)')
        if getattr(basis, 'nclasses', 1) != 1:
            raise NotImplementedError('isoparametric geometry needs a basis with one coefficient table for all elements (btype std)')
        self.basis = basis
        self.verts = numpy.ascontiguousarray(verts)
        self.ndims = basis.ndims


class TabulatedGeometry(Geometry):
    '''Geometry known at the points of ONE sample only: coordinates x[nelems][nq][ndims] and Jacobians
    J[nelems][nq][ndims][ndims] = d x_i / d xi_j w.r.t. the element coordinates, supplied by the mesh producer (NURBS maps
    seen through refinement transforms, examples/platewithhole.py:74-79; any map the kernels do not evaluate themselves).'''

    def __init__(self, x, J):
        self.x = numpy.ascontiguousarray(x, dtype=float)
        self.jac = numpy.ascontiguousarray(J, dtype=float)
        if self.jac.shape != self.x.shape + self.x.shape[-1:]:
            raise ValueError('J must have shape x.shape + (ndims,)')
        self.ndims = self.x.shape[-1]


def dot_basis(basis, values):
    '''``basis @ values``: geometry if values is (ndofs, ndims), else a scalar/vector field value.'''
    values = numpy.asarray(values, dtype=float)
    if values.ndim == 2 and values.shape == (basis.ndofs, basis.ndims):
        return IsoGeometry(basis, values)
    raise NotImplementedError('basis @ array is supported for geometry construction only; use fields with arguments otherwise')


def _same_geom(a, b):
    '''Geometry of a sum of gradient operands: mixing gradients with respect to different geometries in one operand is not representable.'''
    if a is not None and b is not None and a is not b:
        raise NotImplementedError('sum of gradients with respect to different geometries')
    return a if a is not None else b


class Measure:
    '''J(geom): the volume measure |det dx/dxi| (function.py:1266-1295).'''

    __array_ufunc__ = None

    def __init__(self, geom):
        if not isinstance(geom, Geometry):
            raise TypeError('J expects a geometry')
        self.geom = geom

    def __mul__(self, other):
        if isinstance(other, IntegrandSum):  # J(geom) * (a - b): distributes like (a - b) * J(geom)
            return other * self
        return _as_integrand(other).with_measure(self.geom)

    __rmul__ = __mul__


def J(geom):
    return Measure(geom)


class PointFunc:
    '''Scalar coefficient function of the physical coordinates (e.g. a Neumann flux
    ``cos(1) cosh(x_1)``, examples/laplace.py:68).  It is evaluated once per sample at the
    quadrature points -- coordinates come from the device (nh_sample_eval), the callable
    `func(x: (npoints, ndims)) -> (npoints,)` runs in numpy -- and enters the element
    kernels as a pointwise factor of the integrand (scale_dev).'''

    __array_ufunc__ = None

    def __init__(self, func, geom):
        if not isinstance(geom, Geometry):
            raise TypeError('PointFunc expects a geometry')
        self.func, self.geom = func, geom

    def __call__(self, x):
        v = numpy.asarray(self.func(x), dtype=float)
        if v.shape != (len(x),):
            v = numpy.broadcast_to(v, (len(x),)).copy()
        return v

    def __mul__(self, other):
        if isinstance(other, PointFunc):
            if other.geom is not self.geom:
                raise NotImplementedError('coefficient functions of different geometries')
            f, g = self.func, other.func
            return PointFunc(lambda x: numpy.asarray(f(x)) * numpy.asarray(g(x)), self.geom)
        if isinstance(other, (int, float)):
            f = self.func
            return PointFunc(lambda x: numpy.asarray(f(x)) * other, self.geom)
        if isinstance(other, IntegrandSum):
            return other * self
        return _as_integrand(other).with_scale(self)

    __rmul__ = __mul__

    def __neg__(self):
        return self * -1.


class PointTable(PointFunc):
    '''Scalar coefficient given by its VALUES at the points of one sample, [nelems-of-the-sample][nq] (a coefficient function that
    the producer of the integral has already evaluated there: nutils_amd/seam.py plans carry coefficient functions of the reference
    this way).  Enters the kernels as scale_dev like any PointFunc.'''

    def __init__(self, values):
        self.values = numpy.ascontiguousarray(values, dtype=float)
        self.func, self.geom = None, None

    def __call__(self, x=None):
        return self.values.reshape(-1)

    def __mul__(self, other):
        if isinstance(other, PointTable):
            return PointTable(self.values * other.values)
        if isinstance(other, (int, float)):
            return PointTable(self.values * other)
        if isinstance(other, PointFunc):
            raise NotImplementedError('tabulated coefficient times a coefficient function of x')
        return PointFunc.__mul__(self, other)

    __rmul__ = __mul__


class FieldPoly:
    '''Polynomial in the POINT VALUES of scalar fields, sum_t c_t prod_v field_v^p_tv: nonlinear coefficient functions such as
    the double-well potential psi(phi) = (phi^2-1)^2/4 of examples/cahnhilliard.py:175.  Evaluated on the device at the
    quadrature points (nh_sample_eval + nh_pointwise_poly) and applied as a pointwise factor of the integrand; derivatives
    with respect to a field differentiate the polynomial symbolically.'''

    __array_ufunc__ = None

    def __init__(self, args, terms):
        terms = {k: v for k, v in terms.items() if v != 0}
        used = [i for i in range(len(args)) if any(k[i] for k in terms)]  # (a variable no monomial uses is dropped: its field need not be bound at evaluation)
        self.args = tuple(args[i] for i in used)
        self.terms = {}
        for k, v in terms.items():
            kk = tuple(k[i] for i in used)
            self.terms[kk] = self.terms.get(kk, 0.) + v

    @staticmethod
    def _merge(a, b):
        args = list(a.args)
        for arg in b.args:
            if not any(arg.same(x) for x in args):
                args.append(arg)
        def lift(p):
            idx = [next(i for i, x in enumerate(args) if x.same(arg)) for arg in p.args]
            out = {}
            for k, v in p.terms.items():
                key = [0] * len(args)
                for i, pw in zip(idx, k):
                    key[i] = pw
                out[tuple(key)] = out.get(tuple(key), 0.) + v
            return out
        return args, lift(a), lift(b)

    @staticmethod
    def _const(c, like):
        return FieldPoly(like.args, {(0,) * len(like.args): float(c)})

    def _coerce(self, other):
        if isinstance(other, FieldPoly):
            return other
        if isinstance(other, (int, float)):
            return FieldPoly._const(other, self)
        return None

    def __add__(self, other):
        o = self._coerce(other)
        if o is None:
            return NotImplemented
        args, a, b = FieldPoly._merge(self, o)
        for k, v in b.items():
            a[k] = a.get(k, 0.) + v
        return FieldPoly(args, a)

    __radd__ = __add__

    def __neg__(self):
        return FieldPoly(self.args, {k: -v for k, v in self.terms.items()})

    def __sub__(self, other):
        o = self._coerce(other)
        return NotImplemented if o is None else self + (-o)

    def __rsub__(self, other):
        return (-self) + other

    def __mul__(self, other):
        o = self._coerce(other)
        if o is None:
            if isinstance(other, PointFunc):
                return NotImplemented
            if isinstance(other, IntegrandSum):
                return other * self
            return _as_integrand(other).with_fscale(self)
        args, a, b = FieldPoly._merge(self, o)
        out = {}
        for ka, va in a.items():
            for kb, vb in b.items():
                k = tuple(x + y for x, y in zip(ka, kb))
                out[k] = out.get(k, 0.) + va * vb
        return FieldPoly(args, out)

    __rmul__ = __mul__

    def __truediv__(self, other):
        return self * (1. / float(other))

    def __pow__(self, n):
        if not isinstance(n, int) or n < 0:
            raise NotImplementedError('integer powers only')
        out = FieldPoly._const(1., self)
        for _ in range(n):
            out = out * self
        return out

    def depends_on(self, name):
        return any(a.name == name and any(k[i] for k in self.terms) for i, a in enumerate(self.args))

    def arg_named(self, name):
        return next(a for a in self.args if a.name == name)

    def derivative(self, name):
        out = {}
        for i, a in enumerate(self.args):
            if a.name != name:
                continue
            for k, v in self.terms.items():
                if k[i]:
                    kk = k[:i] + (k[i] - 1,) + k[i + 1:]
                    out[kk] = out.get(kk, 0.) + v * k[i]
        return FieldPoly(self.args, out)


def value(field_operand):
    '''Point value of a scalar field as a FieldPoly variable (to build nonlinear coefficient functions).'''
    op = _as_operand(field_operand)
    if op.arg.name is None or op.arg.ncomp != 1 or op.P.shape != (1, op.P.shape[-1]) or numpy.abs(op.P[0, 1:]).sum() != 0:
        raise NotImplementedError('value() expects a plain scalar field')
    return FieldPoly((op.arg,), {(1,): float(op.P[0, 0])})


# ---- arguments and operands ----------------------------------------------------------

class Arg:
    '''The thing an operand is linear in: a basis with `ncomp` components.  `name` is
    None for a basis used directly as an array (its dof axis is an array axis).'''

    def __init__(self, basis, ncomp, name):
        self.basis, self.ncomp, self.name = basis, int(ncomp), name

    def same(self, other):
        return self is other or (self.name is not None and self.name == other.name and self.basis is other.basis and self.ncomp == other.ncomp)


class PointTerm:
    '''One term of a PointExpr: A[free..., (component, slot) per factor] x prod_k F_k[c_k][s_k] x scale(point).  Factors: ('field', Arg, geometry) -- value
    (slot 0) and gradient with respect to the geometry (slots 1 .. ndims) of a bound field; ('x', geometry) -- the coordinates (components = axes, one slot).'''

    def __init__(self, A, factors, scale=None):
        self.A = numpy.array(A, dtype=float, order='C')  # (ascontiguousarray would turn a scalar into a vector)
        self.factors = list(factors)
        self.scale = scale  # PointTable [nlist][nq] or None
        self._entries = {}

    def entries(self, ndims):
        '''The non-zeros of A as (output index, offset of (component, slot) in the point block of every factor, coefficient), outputs ascending.'''
        hit = self._entries.get(ndims)
        if hit is None:
            S = 1 + ndims
            nf = len(self.factors)
            slots = [S if f[0] == 'field' else 1 for f in self.factors]
            comps = [f[1].ncomp if f[0] == 'field' else ndims for f in self.factors]
            free = self.A.shape[:self.A.ndim - 2 * nf]
            if self.A.shape[len(free):] != tuple(n for c, sl in zip(comps, slots) for n in (c, sl)):
                raise ValueError(f'coefficient tensor {self.A.shape} does not match its factors')
            if self.A.ndim:
                idx = numpy.nonzero(self.A)
                out = numpy.ravel_multi_index(idx[:len(free)], free) if free else numpy.zeros(len(idx[0]), dtype=numpy.int64)
                coef = self.A[idx]
            else:  # a constant
                idx, out, coef = (), numpy.zeros(int(self.A != 0), dtype=numpy.int64), self.A.reshape(1)[:int(self.A != 0)]
            off = numpy.stack([idx[len(free) + 2 * k] * slots[k] + idx[len(free) + 2 * k + 1] for k in range(nf)], axis=1) if nf else numpy.zeros((len(out), 0), dtype=numpy.int64)
            hit = self._entries[ndims] = (out.astype(numpy.int32), off.astype(numpy.int32), numpy.asarray(coef, dtype=float), free)
        return hit


class PointExpr:
    '''Array-valued function of the point for Sample.eval / Sample.bind (sample.py:192-232 of the reference): a sum of PointTerms with the same free shape --
    displaced coordinates x + u, stresses C : grad(u), fluxes, products of fields.  Evaluated on the device: nh_sample_eval per (field, geometry), nh_point_expr per term.'''

    def __init__(self, shape, terms):
        self.shape = tuple(int(n) for n in shape)
        self.terms = list(terms)


def _bcast(a, b, keep):
    '''Broadcast the leading (free) axes of a and b numpy-style, keeping `keep` trailing axes of each aside.'''
    fa, fb = a.shape[:a.ndim - keep[0]], b.shape[:b.ndim - keep[1]]
    free = numpy.broadcast_shapes(fa, fb)
    a = numpy.broadcast_to(a.reshape((1,) * (len(free) - len(fa)) + a.shape), free + a.shape[len(fa):])
    b = numpy.broadcast_to(b.reshape((1,) * (len(free) - len(fb)) + b.shape), free + b.shape[len(fb):])
    return a, b, free


class Operand:
    '''Tensor-valued expression, linear in one argument: value[free...] =
    sum_{c,s} P[free..., c, s] D[c, s],  D[c,0] = arg_c, D[c,1+i] = d arg_c / d x_i.'''

    __array_ufunc__ = None

    def __init__(self, arg, P, geom=None):
        self.arg, self.P, self.geom = arg, numpy.asarray(P, dtype=float), geom

    @property
    def shape(self):
        free = self.P.shape[:-2]
        return ((self.arg.basis.ndofs,) if self.arg.name is None else ()) + free

    @property
    def ndim(self):
        return len(self.shape)

    def _free_axis(self, axis):
        nfree = self.P.ndim - 2
        lead = 1 if self.arg.name is None else 0
        if axis < 0:
            axis += nfree + lead
        axis -= lead
        if not 0 <= axis < nfree:
            raise ValueError('axis out of range (the dof axis of a basis cannot be reduced)')
        return axis

    def grad(self, geom):
        if not isinstance(geom, Geometry):
            raise TypeError('grad expects a geometry')
        if numpy.abs(self.P[..., 1:]).sum() != 0:
            raise NotImplementedError('second derivatives are outside the accelerated path')
        nd = geom.ndims
        if self.P.shape[-1] != 1 + nd:
            raise ValueError('geometry dimension does not match the argument')
        P = numpy.zeros(self.P.shape[:-2] + (nd,) + self.P.shape[-2:-1] + (1 + nd,))
        for j in range(nd):
            P[..., j, :, 1 + j] = self.P[..., :, 0]
        return Operand(self.arg, P, geom)

    def _const(self, other):
        other = numpy.asarray(other, dtype=float)
        a, b, free = _bcast(self.P, other, (2, 0))
        return Operand(self.arg, a * b[..., None, None], self.geom)

    def __mul__(self, other):
        if isinstance(other, (Measure, PointFunc, FieldPoly)):
            return other.__mul__(self)
        from .basis import Basis
        if isinstance(other, Basis):
            other = _as_operand(other)
        if isinstance(other, Operand):
            return _product(self, other)
        if isinstance(other, Integrand):
            return NotImplemented
        return self._const(other)

    def __rmul__(self, other):
        return self._const(other)

    def __truediv__(self, other):
        return self._const(1. / numpy.asarray(other, dtype=float))

    def __pow__(self, n):
        if n == 1:
            return self
        if n == 2:
            return self * self
        raise NotImplementedError('powers of a field beyond 2: use function.value(field) ** n (pointwise coefficient)')

    def __matmul__(self, other):
        '''Contraction over the last axis (`g @ g` of examples/poisson.py:32).'''
        return (self * other).sum(-1)

    def __neg__(self):
        return Operand(self.arg, -self.P, self.geom)

    def __add__(self, other):
        if not isinstance(other, Operand) or not other.arg.same(self.arg):
            raise NotImplementedError('operands can only be added to operands of the same argument')
        a, b, _ = _bcast(self.P, other.P, (2, 2))
        return Operand(self.arg, a + b, _same_geom(self.geom, other.geom))

    def __sub__(self, other):
        return self + (-other)

    def sum(self, axis=-1):
        return Operand(self.arg, self.P.sum(self._free_axis(axis)), self.geom)

    def transpose(self, a=-2, b=-1):
        return Operand(self.arg, numpy.swapaxes(self.P, self._free_axis(a), self._free_axis(b)), self.geom)

    @property
    def T(self):
        return self.transpose()

    def trace(self, a=-2, b=-1):
        return Operand(self.arg, numpy.trace(self.P, axis1=self._free_axis(a), axis2=self._free_axis(b)), self.geom)

    def __getitem__(self, item):
        if not isinstance(item, tuple):
            item = item,
        if self.arg.name is None:
            if item[0] != slice(None):
                raise NotImplementedError('the dof axis of a basis array cannot be indexed')
            item = item[1:]
        return Operand(self.arg, self.P[tuple(item) + (Ellipsis, slice(None), slice(None))], self.geom)


def trace(op, a=-2, b=-1):
    return op.trace(a, b)


def grad(op, geom):
    return _as_operand(op).grad(geom)


def symgrad(op, geom):
    g = _as_operand(op).grad(geom)
    return (g + g.T) * .5


def div(op, geom):
    return _as_operand(op).grad(geom).trace()


def eye(n):
    return numpy.eye(n)


def field(name, basis, shape=()):
    '''Named argument field (function.field, function.py:2598-2627): argument array of
    shape (ndofs, *shape); flat dof = scalar dof * ncomp + comp.'''
    shape = tuple(shape)
    if len(shape) > 1:
        raise NotImplementedError('fields of rank > 1')
    ncomp = shape[0] if shape else 1
    arg = Arg(basis, ncomp, name)
    S = 1 + basis.ndims
    if shape:
        P = numpy.zeros((ncomp, ncomp, S))
        P[numpy.arange(ncomp), numpy.arange(ncomp), 0] = 1
    else:
        P = numpy.zeros((1, S))
        P[0, 0] = 1
    return Operand(arg, P)


def dotarg(name, basis, shape=()):
    return field(name, basis, shape)


def _as_operand(obj):
    from .basis import Basis
    if isinstance(obj, Operand):
        return obj
    if isinstance(obj, Basis):
        if not hasattr(obj, '_as_operand'):
            P = numpy.zeros((1, 1 + obj.ndims))
            P[0, 0] = 1
            obj._as_operand = Operand(Arg(obj, 1, None), P)
        return obj._as_operand
    raise TypeError(f'cannot interpret {type(obj).__name__} as an operand')


# ---- integrands ------------------------------------------------------------------------

class Integrand:
    '''sum of: bilinear  B[c,a,d,b] Dtest[c,a] Dtrial[d,b]  (+ free axes until summed),
    linear  L[c,a] Dtest[c,a],  constant f0;  times the measure of `geom`.'''

    __array_ufunc__ = None

    def __init__(self, test=None, trial=None, B=None, L=None, f0=None, geom=None, measure=None, rows=False, cols=False, scale=None, fscale=None, qform=None, qscalar=None,
                 pvars=()):
        self.test, self.trial, self.B, self.L, self.f0 = test, trial, B, L, f0
        # point variables: the whole integrand is multiplied by prod_k U_arg_k[comp_k][slot_k] at the point -- components of values (slot 0) and gradients (slot 1 + i)
        # of bound, possibly vector-valued fields (the convection u_j d_j(u_i) v_i of Navier-Stokes, function.py:1207-1295 of the reference).  (Arg, comp, slot) triples;
        # evaluated on the device into the scale array of the term (sample._bind_pvars), differentiated by the product rule in `derivative` below.
        self.pvars = tuple(pvars)
        # product-rule terms of Newton Jacobians / Hessians of energies: forms whose coefficients depend on the point through the VALUES
        # (value and gradient) U of a field there.  With B the tensor of this integrand,
        #   qform = ('trial', arg):    C_q[c][a][0][0] = sum_db B[c][a][d][b] U_arg[d][b]     (result on the value slot of the trial function)
        #   qform = ('test', arg, L):  C_q[c][a][d][b] = L[c][a] sum_xy B[x][y][d][b] U_arg[x][y]
        #   qscalar = (Bs, arg_t, arg_r): the whole integrand is multiplied by s_q = sum Bs[c][a][d][b] U_t[c][a] U_r[d][b]
        # (scalar fields; assembled with per-point coefficient tensors / scale arrays built on the device)
        self.qform = qform
        self.qscalar = qscalar
        self.scale = scale      # PointFunc multiplying the whole integrand, or None
        self.fscale = fscale    # FieldPoly multiplying the whole integrand, or None
        self.geom = geom        # geometry the gradients refer to
        self.measure = measure  # geometry of the measure
        self.rows, self.cols = rows, cols  # dof axis of test / trial is an array axis (else: bound to an argument value)

    def _copy(self, **kw):
        d = dict(test=self.test, trial=self.trial, B=self.B, L=self.L, f0=self.f0, geom=self.geom, measure=self.measure, rows=self.rows, cols=self.cols,
                 scale=self.scale, fscale=self.fscale, qform=self.qform, qscalar=self.qscalar, pvars=self.pvars)
        d.update(kw)
        return Integrand(**d)

    @property
    def _tensor(self):
        return self.B if self.B is not None else self.L if self.L is not None else numpy.asarray(self.f0)

    @property
    def _keep(self):
        return 4 if self.B is not None else 2 if self.L is not None else 0

    @property
    def shape(self):
        t = self._tensor
        free = t.shape[:t.ndim - self._keep]
        lead = ((self.test.basis.ndofs,) if self.rows and self.test.name is None else ()) + ((self.trial.basis.ndofs,) if self.cols and self.trial.name is None else ())
        return lead + free

    def _set(self, t):
        return self._copy(**{'B' if self.B is not None else 'L' if self.L is not None else 'f0': t})

    def with_measure(self, geom):
        if self.measure is not None:
            raise NotImplementedError('integrand already carries a measure')
        if self.geom is not None and self.geom is not geom:
            raise NotImplementedError('gradient geometry and measure geometry differ')
        return self._copy(measure=geom)

    def with_scale(self, pf):
        return self._copy(scale=pf if self.scale is None else self.scale * pf)

    def with_fscale(self, fp):
        return self._copy(fscale=fp if self.fscale is None else self.fscale * fp)

    def __mul__(self, other):
        if isinstance(other, Measure):
            return self.with_measure(other.geom)
        if isinstance(other, PointFunc):
            return self.with_scale(other)
        if isinstance(other, FieldPoly):
            return self.with_fscale(other)
        if isinstance(other, (Operand, Integrand)):
            raise NotImplementedError('products of more than two argument-dependent factors are outside the accelerated path')
        other = numpy.asarray(other, dtype=float)
        t = self._tensor
        a, b, _ = _bcast(t, other, (self._keep, 0))
        return self._set(a * b.reshape(b.shape + (1,) * self._keep))

    __rmul__ = __mul__

    def __neg__(self):
        return self._set(-self._tensor)

    def sum(self, axis=-1):
        t = self._tensor
        nfree = t.ndim - self._keep
        lead = len(self.shape) - nfree
        if axis < 0:
            axis += nfree + lead
        axis -= lead
        if not 0 <= axis < nfree:
            raise ValueError('axis out of range')
        return self._set(t.sum(axis))

    def _compatible(self, other):
        def same(a, b):
            return (a is None and b is None) or (a is not None and b is not None and a.same(b))
        return same(self.test, other.test) and same(self.trial, other.trial) and self.rows == other.rows and self.cols == other.cols \
            and self.measure is other.measure and (self.B is None) == (other.B is None) and (self.L is None) == (other.L is None) \
            and self.scale is other.scale and self.fscale is other.fscale \
            and (self.geom is None or other.geom is None or self.geom is other.geom)  # gradients w.r.t. different geometries stay separate terms

    def __truediv__(self, other):
        return self * (1. / numpy.asarray(other, dtype=float))

    def __add__(self, other):
        if isinstance(other, IntegrandSum):
            return IntegrandSum([self] + other.terms)
        other = _as_integrand(other)
        if not self._compatible(other):  # e.g. (g @ g / 2 - u): a quadratic and a linear form -> kept apart, integrated term by term
            return IntegrandSum([self, other])
        a, b, _ = _bcast(self._tensor, other._tensor, (self._keep, other._keep))
        return self._set(a + b)._copy(geom=self.geom or other.geom)

    __radd__ = __add__

    def __sub__(self, other):
        return self + (-(other if isinstance(other, IntegrandSum) else _as_integrand(other)))

    def __rsub__(self, other):
        return (-self) + other


class IntegrandSum:
    '''Sum of integrands of different kinds (bilinear + linear + constant ...): distributes over multiplication with a measure or a
    coefficient and over integration, so that `topo.integral((g @ g / 2 - u) * J, degree)` reads as in the reference.'''

    __array_ufunc__ = None

    def __init__(self, terms):
        self.terms = list(terms)

    def __mul__(self, other):
        return IntegrandSum([t * other for t in self.terms])

    __rmul__ = __mul__

    def __truediv__(self, other):
        return IntegrandSum([t / other for t in self.terms])

    def __neg__(self):
        return IntegrandSum([-t for t in self.terms])

    def __add__(self, other):
        return IntegrandSum(self.terms + (other.terms if isinstance(other, IntegrandSum) else [_as_integrand(other)]))

    __radd__ = __add__

    def __sub__(self, other):
        return self + (-(other if isinstance(other, IntegrandSum) else _as_integrand(other)))


def _as_integrand(obj):
    if isinstance(obj, Integrand):
        return obj
    if isinstance(obj, Measure):
        return Integrand(f0=numpy.ones(()), measure=obj.geom)
    if isinstance(obj, PointFunc):
        return Integrand(f0=numpy.ones(()), scale=obj)
    if isinstance(obj, FieldPoly):
        return Integrand(f0=numpy.ones(()), fscale=obj)
    if isinstance(obj, (int, float, numpy.ndarray)):
        return Integrand(f0=numpy.asarray(obj, dtype=float))
    op = _as_operand(obj)
    return Integrand(test=op.arg, L=op.P, geom=op.geom, rows=op.arg.name is None)


def _product(a, b, outer=False):
    '''a * b for two operands: test side = a, trial side = b.'''
    if a.geom is not None and b.geom is not None and a.geom is not b.geom:
        raise NotImplementedError('factors differentiate with respect to different geometries')
    Pa, Pb, free = _bcast(a.P, b.P, (2, 2))
    B = Pa[..., :, :, None, None] * Pb[..., None, None, :, :]
    return Integrand(test=a.arg, trial=b.arg, B=B, geom=a.geom or b.geom, rows=a.arg.name is None, cols=b.arg.name is None)


def outer(a, b=None):
    '''Outer product over the dof axes of two basis arrays, elementwise over the
    remaining axes (function.outer in the reference): shape (ndofs_a, ndofs_b, ...).'''
    a = _as_operand(a)
    b = a if b is None else _as_operand(b)
    if a.arg.name is not None or b.arg.name is not None:
        raise TypeError('outer expects basis arrays; multiply fields directly')
    return _product(a, b)


def inner(a, b):
    '''Full contraction over all free axes of two operands.'''
    p = _product(_as_operand(a), _as_operand(b))
    while p.B.ndim > 4:
        p = p._set(p.B.sum(0))
    return p


# ---- integrals --------------------------------------------------------------------------

class Integral:
    '''Postponed integral: sum of (sample, integrand, factor) terms
    (sample.py:944-956 ``_Integral``); evaluated on the GPU by function.eval.'''

    def __init__(self, terms):
        self.terms = tuple(terms)

    def __add__(self, other):
        if not isinstance(other, Integral):
            return NotImplemented
        return Integral(self.terms + other.terms)

    def __neg__(self):
        return Integral((s, i, -f) for s, i, f in self.terms)

    def __sub__(self, other):
        return self + (-other)

    def __mul__(self, scalar):
        return Integral((s, i, f * float(scalar)) for s, i, f in self.terms)

    __rmul__ = __mul__

    @property
    def shape(self):
        return self.terms[0][1].shape

    def derivative(self, name):
        return derivative(self, name)

    def eval(self, **arguments):
        return eval(self, **arguments)


def _expand_fscale(itg, fac):
    '''the coefficient polynomial of a term written out: one term per monomial, its field values as point variables (value slot) -> [(integrand, factor)]'''
    out = []
    for powers, c in itg.fscale.terms.items():
        pv = tuple((a, 0, 0) for a, p in zip(itg.fscale.args, powers) for _ in range(p))
        out.append((itg._copy(fscale=None, pvars=itg.pvars + pv), fac * c))
    return out


def _pvar_derivative(itg, k):
    '''d/d(point variable k) of the integrand: the variable U[comp][slot] becomes the basis function phi_n of its argument at (comp, slot) -- a new test or trial slot.
    Slots that are bound to argument values (a trial field in a residual form, both fields of an energy) are moved into point variables first: B(v, u) with u bound is
    sum_db L_db(v) u[d][b], every summand a constant form times a point variable, so that the result is again (constant form) x (point variables) and nothing of
    the product rule needs per-point coefficient tensors.'''
    varg, comp, slot = itg.pvars[k]
    rest = itg.pvars[:k] + itg.pvars[k + 1:]
    if itg.qform is not None or itg.qscalar is not None:
        raise NotImplementedError('point variables together with the product-rule tensors of scalar coefficient functions')
    if (itg.B if itg.B is not None else itg.L if itg.L is not None else numpy.zeros(())).ndim > itg._keep:
        raise NotImplementedError('point variables on an integrand with free axes')
    S = 1 + varg.basis.ndims
    out = []
    if itg.test is None:  # f0 x variables -> linear form in the test function of varg
        L = numpy.zeros((varg.ncomp, S))
        L[comp, slot] = float(itg.f0)
        return [itg._copy(test=varg, L=L, f0=None, rows=True, pvars=rest)]
    if itg.B is None:
        if itg.rows:      # L(test) x variables -> bilinear form (test x varg)
            B = numpy.zeros(itg.L.shape + (varg.ncomp, S))
            B[..., comp, slot] = itg.L
            return [itg._copy(trial=varg, B=B, L=None, cols=True, pvars=rest)]
        for c, a in zip(*numpy.nonzero(itg.L)):  # L(u) with u bound: the slots of u become variables
            out += _pvar_derivative(itg._copy(test=None, L=None, f0=numpy.asarray(float(itg.L[c, a])), pvars=rest + ((itg.test, int(c), int(a)), itg.pvars[k])), len(rest) + 1)
        return out
    if itg.rows and itg.cols:
        raise NotImplementedError('derivative of a matrix with respect to a point variable (rank-3 tensor)')
    if itg.cols:
        raise NotImplementedError('point variables on a form whose trial slot is exposed before its test slot')
    if itg.rows:          # B(test, u) with u bound -> sum over the slots of u: L_db(test) u[d][b]
        for d, b in zip(*numpy.nonzero(numpy.abs(itg.B).sum(axis=(0, 1)))):
            out += _pvar_derivative(itg._copy(trial=None, B=None, L=numpy.ascontiguousarray(itg.B[:, :, d, b]), pvars=rest + ((itg.trial, int(d), int(b)), itg.pvars[k])), len(rest) + 1)
        return out
    for c, a, d, b in zip(*numpy.nonzero(itg.B)):  # energy density B(u, w) x variables: everything becomes a variable
        out += _pvar_derivative(itg._copy(test=None, trial=None, B=None, f0=numpy.asarray(float(itg.B[c, a, d, b])),
                                          pvars=rest + ((itg.test, int(c), int(a)), (itg.trial, int(d), int(b)), itg.pvars[k])), len(rest) + 2)
    return out


def derivative(integral, name):
    '''Derivative with respect to the named field argument (function.derivative):
    exposes that argument's dof axis.  Terms that do not depend on it vanish.'''
    out = []
    T = lambda B: numpy.moveaxis(B, (-4, -3, -2, -1), (-2, -1, -4, -3))
    for smp, itg, fac in integral.terms:
        mark = len(out)
        for k, (varg, comp, slot) in enumerate(itg.pvars):
            if varg.name == name:  # product rule on a point variable: the basis function of (varg, comp, slot) takes its place
                out += [(smp, t, fac) for t in _pvar_derivative(itg, k)]
        if itg.fscale is not None and itg.fscale.depends_on(name):
            g = itg.fscale.derivative(name)
            varg = itg.fscale.arg_named(name)
            S = 1 + varg.basis.ndims
            if g.terms:
                if itg.B is None and itg.L is None:        # g(phi) * const  ->  linear form in the test function of phi
                    L = numpy.zeros((1, S))
                    L[0, 0] = float(itg.f0)
                    out.append((smp, itg._copy(test=varg, L=L, f0=None, rows=True, fscale=g), fac))
                elif itg.B is None and itg.rows and not itg.cols:  # g(phi) * L(test)  ->  bilinear (test x phi)
                    B = numpy.zeros(itg.L.shape + (1, S))
                    B[..., 0, 0] = itg.L
                    out.append((smp, itg._copy(trial=varg, B=B, L=None, cols=True, fscale=g), fac))
                elif itg.B is not None and itg.rows and not itg.cols and itg.qform is None and itg.trial.ncomp == 1 and varg.ncomp == 1 and itg.B.ndim == 4:
                    # g(phi) * B(test, u)  ->  g'(phi) phi_n * B(test, u): bilinear (test x phi) with the coefficients B . U(u) of the point
                    out.append((smp, itg._copy(trial=varg, cols=True, fscale=g, qform=('trial', itg.trial)), fac))
                elif (itg.B is not None and not itg.rows and not itg.cols and itg.qform is None and itg.qscalar is None and itg.B.ndim == 4
                      and itg.test.ncomp == itg.trial.ncomp == varg.ncomp == 1):
                    # energy density g(phi) * B(u, w)  ->  g'(phi) phi_m * (U_u . B . U_w): linear form with a point factor
                    L = numpy.zeros((1, S))
                    L[0, 0] = 1.
                    out.append((smp, itg._copy(test=varg, trial=None, B=None, L=L, rows=True, fscale=g, qscalar=(itg.B, itg.test, itg.trial)), fac))
                elif itg.qform is None and itg.qscalar is None:
                    # any other position (a coefficient polynomial on a form with a bound trial field of several components, ...): the polynomial's monomials as point
                    # variables, differentiated by the product rule of _pvar_derivative -- again constant forms times point variables
                    # (the expanded terms carry the term's own point variables: their derivatives come out of the recursion, not of the loop above)
                    del out[mark:]
                    out += derivative(Integral([(smp, t, f) for t, f in _expand_fscale(itg, fac)]), name).terms
                    continue
                else:
                    raise NotImplementedError('derivative of a field-dependent coefficient in this position (rank-3 tensor)')
        if itg.qscalar is not None:
            Bs, at, ar = itg.qscalar
            hit_t, hit_r = at.name == name, ar.name == name
            if hit_t or hit_r:
                if not (itg.B is None and itg.L is not None and itg.rows and not itg.cols):
                    raise NotImplementedError('derivative of a point factor in this position')
                if hit_t and hit_r:
                    if at.basis is not ar.basis:
                        raise NotImplementedError
                    Bv, bound, targ = Bs + T(Bs), at, at   # d(U.B.U) = phi_n . (B + B^T) . U
                elif hit_r:
                    Bv, bound, targ = Bs, at, ar           # U_t . B . phi_n: contract the test side with U_t
                else:
                    Bv, bound, targ = T(Bs), ar, at        # phi_n . B . U_r
                out.append((smp, itg._copy(trial=targ, B=Bv, L=None, cols=True, qscalar=None, qform=('test', bound, itg.L)), fac))
        t_hit = itg.test is not None and itg.test.name == name and not itg.rows
        r_hit = itg.trial is not None and itg.trial.name == name and not itg.cols
        if itg.qform is not None and (t_hit or r_hit or itg.qform[1].name == name):
            raise NotImplementedError('third derivatives of field-dependent coefficients')
        if itg.B is not None and t_hit and r_hit:
            if itg.cols or itg.rows:
                raise NotImplementedError
            # quadratic in the field: d/du B(u,u) = B(du,u) + B(u,du)
            out.append((smp, itg._copy(B=itg.B + T(itg.B), rows=True), fac))
        elif t_hit:
            if itg.rows or (itg.cols and itg.B is None):
                raise NotImplementedError
            if itg.cols:  # keep the convention rows = first differentiated axis: transpose
                out.append((smp, itg._copy(B=T(itg.B), test=itg.trial, trial=itg.test, rows=True, cols=True), fac))
            else:
                out.append((smp, itg._copy(rows=True), fac))
        elif r_hit:
            if itg.rows:
                out.append((smp, itg._copy(cols=True), fac))
            else:  # derivative w.r.t. the trial-side field first: swap roles
                out.append((smp, itg._copy(B=T(itg.B), test=itg.trial, trial=itg.test, rows=True, cols=False), fac))
    return Integral(out)


class _AsCSR:
    def __init__(self, integral):
        self.integral = integral


def as_csr(integral):
    '''function.as_csr (function.py:2432-2437): evaluates to (values, rowptr, colidx);
    index arrays int64, rows/cols sorted, structural zeros retained.'''
    from . import factor as _factor
    if not isinstance(integral, (Integral, _factor.FactoredMatrix)):
        raise TypeError('as_csr expects an Integral')
    return _AsCSR(integral)


class _AsCOO:
    def __init__(self, integral):
        self.integral = integral


class _AsMatrix(_AsCSR):
    pass


def as_matrix(integral):
    '''Sibling of `as_csr` for the device-resident backend: evaluates to a `matrix.HipMatrix` on the CSR triplet the assembly left in HBM -- values and
    indices are not copied to the host.'''
    from . import factor as _factor
    if not isinstance(integral, (Integral, _factor.FactoredMatrix)):
        raise TypeError('as_matrix expects an Integral')
    return _AsMatrix(integral)


def as_coo(integral):
    '''function.as_coo (function.py:2440-2452): (values, rowidx, colidx).'''
    return _AsCOO(integral)


def eval(funcs, /, arguments=None, **kwargs):
    '''function.eval (function.py:2408-2429): evaluate one or several integrals
    (optionally wrapped in as_csr / as_coo) with the given arguments.'''
    from . import sample as _sample
    arguments = dict(arguments or {}, **kwargs)
    single = not isinstance(funcs, (tuple, list))
    items = (funcs,) if single else tuple(funcs)
    results = tuple(_sample.evaluate(f, arguments) for f in items)
    return results[0] if single else results


evaluate = eval


def factor(integral, name=None):
    '''function.factor (function.py:2630-2642): pre-integrated form of a polynomial functional.'''
    from . import factor as _factor
    return _factor.factor(integral, name)
