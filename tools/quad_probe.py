#!/usr/bin/env python3
'''First and steady re-assembly times of the structured 2-D write-once path (nh_quad_matrix / nh_quad_rows_uniform) against the generic path
(NUTILS_AMD_NO_FAST_PATH=1) in the same process, on the forms of tools/generic_probe.py: python tools/quad_probe.py [case substrings].
One JSON line per case; algorithmic bytes = CSR values written once + the unique geometry vertices read once.'''
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy, torch
from nutils_amd import sample
from nutils_amd.workloads import quad_form as full_form

HBM = 8e12
DEFAULT = sample.QUAD_GEOMETRIC_BASES
CASES = [('2048^2 bilinear', [2048] * 2, 'std', 1, 1, False), ('1024^2 biquadratic', [1024] * 2, 'std', 2, 1, False),
         ('1024^2 spline2', [1024] * 2, 'spline', 2, 1, False), ('1024^2 bilinear elasticity', [1024] * 2, 'std', 1, 2, False),
         ('512^2 biquadratic elasticity', [512] * 2, 'std', 2, 2, False),
         ('2048^2 bilinear uniform', [2048] * 2, 'std', 1, 1, True), ('1024^2 spline2 uniform', [1024] * 2, 'spline', 2, 1, True)]


def timed(plan, window=0.2):
    '''steady re-assembly: HIP events around batches, warmed up, over at least `window` seconds'''
    for _ in range(3):
        plan.run({})
    torch.cuda.synchronize()
    n, total = 0, 0.
    while total < window:
        k = max(1, n or 5)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            plan.run({})
        b.record()
        b.synchronize()
        total += a.elapsed_time(b) / 1e3
        n += k
    return 1e3 * total / n


def first(f):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = sample._MatrixPlan(f.terms).run({})
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


only = sys.argv[1:]
for name, shape, btype, degree, nc, uniform in CASES:
    if only and not any(o in name for o in only):
        continue
    os.environ.pop('NUTILS_AMD_NO_FAST_PATH', None)
    default = uniform or (btype, degree) in DEFAULT
    # (a case the front end keeps on the generic path by default is measured on the kernel all the same: the routing rule is widened for this case only)
    sample.QUAD_GEOMETRIC_BASES = sample.QUAD_BASES
    f = full_form(shape, btype, degree, nc, uniform)
    plan = sample._MatrixPlan(f.terms)
    assert sample._quad_form(plan) is not None
    t_first, (v, rp, ci, _) = first(f)
    ms = timed(plan)
    os.environ['NUTILS_AMD_NO_FAST_PATH'] = '1'
    gplan = sample._MatrixPlan(f.terms)
    t_first_g, (v0, rp0, ci0, _) = first(f)
    ms_g = timed(gplan)
    os.environ.pop('NUTILS_AMD_NO_FAST_PATH')
    ms2 = timed(plan)  # (alternated: the fast path again after the generic one)
    same_idx = bool(torch.equal(rp, rp0) and torch.equal(ci, ci0))
    err = float((v - v0).abs().max() / v0.abs().max())
    nverts = 0 if uniform else (shape[0] + 1) * (shape[1] + 1)
    nbytes = 8 * v.numel() + 16 * nverts
    ms = min(ms, ms2)
    sample.QUAD_GEOMETRIC_BASES = DEFAULT
    print(json.dumps(dict(case=name, default=default, nnz=v.numel(), ms=round(ms, 4), ms_generic=round(ms_g, 4), speedup=round(ms_g / ms, 2), first_ms=round(t_first, 3),
                          first_ms_generic=round(t_first_g, 3), algorithmic_bytes=nbytes, hbm_frac=round(nbytes / (ms * 1e-3) / HBM, 3),
                          indices_equal=same_idx, max_rel_err=err)), flush=True)
    del plan, gplan, v, v0, rp, ci, rp0, ci0, f
    torch.cuda.empty_cache()
