'''nh_block_segment_dot restated in numpy, for tests/test_amg_block_host.py and tests/test_gpu_amg_block.py: a helper module, no tests of its own.'''
import types
import numpy


def host_plan(plan):
    '''the integers of an `amg.BlockPlan` (or of a namespace like it) as numpy arrays; strides that the kernel does not read become zeros'''
    array = lambda t: None if t is None else (t.cpu().numpy() if hasattr(t, 'cpu') else numpy.asarray(t)).astype(numpy.int64)
    ptr, ia, ib = array(plan.ptr), array(plan.ia), array(plan.ib)
    nseg, nprod = len(ptr) - 1, len(ia)
    zeros = numpy.zeros(nseg, dtype=numpy.int64)
    sb = array(plan.sb) if plan.sb is not None else numpy.full(nprod, int(plan.bstride), dtype=numpy.int64)
    return types.SimpleNamespace(k=int(plan.k), p=int(plan.p), q=int(plan.q), ptr=ptr, ia=ia, ib=ib, sb=sb, nseg=nseg, nprod=nprod,
                                 sa=array(plan.sa) if plan.p > 1 else zeros, of=array(plan.of), os=array(plan.os) if plan.p > 1 else zeros)


def block_segment_dot(plan, a, b, nout):
    '''out [nout] in the arithmetic of a and b: the entry (r, c) of the output block of segment s, at of[s] + r os[s] + c, is the sum over the products m of
    the segment, in their order, and t ascending within a product, of a[ia[m] + r sa[s] + t] * b[ib[m] + t sb[m] + c]; 0 where no block lies'''
    h = host_plan(plan)
    seg = numpy.repeat(numpy.arange(h.nseg), numpy.diff(h.ptr))
    t = numpy.arange(h.q)
    out, written = numpy.zeros(nout, dtype=numpy.result_type(a, b)), numpy.zeros(nout, dtype=bool)
    for r in range(h.p):
        for c in range(h.k):
            terms = a[(h.ia + r * h.sa[seg])[:, None] + t] * b[h.ib[:, None] + t * h.sb[:, None] + c]  # [products, q]: the order of the kernel's sum
            block = numpy.zeros(h.nseg, dtype=out.dtype)
            numpy.add.at(block, numpy.repeat(seg, h.q), terms.ravel())
            where = h.of + r * h.os + c
            assert not written[where].any() and len(numpy.unique(where)) == len(where)  # (no two blocks share an entry)
            out[where], written[where] = block, True
    return out


def scalar_terms(plan):
    '''the number of scalar products in every entry of the output, entry by entry in the order of `block_segment_dot` with of = the blocks side by side'''
    h = host_plan(plan)
    return numpy.diff(h.ptr) * h.q
