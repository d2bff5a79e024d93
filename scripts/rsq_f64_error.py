"""Largest relative error of the hardware's f64 reciprocal square root
(__builtin_amdgcn_rsq, the start of acl_price's fast path, csrc/common.h) on
the fast path's range: 2^20 (--samples) log-uniform x in [1e-6, 1e60] and
every binade edge in that range (2^k and its two neighbours), against
1 / sqrt(x) in extended precision on the host (numpy longdouble, 64-bit
mantissa). Prints the figures and writes them to --out.

  python scripts/rsq_f64_error.py --out profiles/r10_prices/rsq_f64_error.txt
"""
import argparse
import ctypes as ct
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs(samples, seed=0):
    rng = np.random.RandomState(seed)
    x = 10.0 ** rng.uniform(-6.0, 60.0, samples)
    k = np.arange(int(np.floor(np.log2(1e-6))), int(np.ceil(np.log2(1e60))) + 1)
    e = np.ldexp(1.0, k)
    edges = np.concatenate([e, np.nextafter(e, 0.0), np.nextafter(e, np.inf)])
    edges = edges[(edges >= 1e-6) & (edges <= 1e60)]
    return np.concatenate([x, edges]), edges.size


def rsq_gpu(x):
    import torch
    from aclswarm_amd import _lib as L
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dev)
    r = torch.empty(len(x), dtype=torch.float64, device=dev)
    rc = L.lib().acl_internal_rsq_sweep(ct.c_void_p(xd.data_ptr()), ct.c_void_p(r.data_ptr()), len(x))
    assert rc == 0
    return r.cpu().numpy()


def rel_error(x, r):
    assert np.finfo(np.longdouble).nmant >= 63, "needs an extended-precision long double"
    ref = 1.0 / np.sqrt(x.astype(np.longdouble))
    return np.abs((r.astype(np.longdouble) - ref) / ref).astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    x, nedges = inputs(a.samples)
    err = rel_error(x, rsq_gpu(x))
    i = int(err.argmax())
    lines = [
        "v_rsq_f64 against 1/sqrt(x) in extended precision",
        "samples: %d log-uniform in [1e-6, 1e60] + %d binade edges" % (a.samples, nedges),
        "largest relative error e0 = %.6e = 2^%.3f at x = %r (%s)" % (
            err[i], np.log2(err[i]), float(x[i]), float(x[i]).hex()),
        "mean %.3e, 99.9th percentile %.3e" % (err.mean(), np.percentile(err, 99.9)),
        "largest on the binade edges: %.6e" % err[a.samples:].max(),
        "one Newton step leaves 1.5 e0^2 = %.3e relative = %.2f ulp of a double at most" % (
            1.5 * err[i] ** 2, 1.5 * err[i] ** 2 * 2.0 ** 53),
    ]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
