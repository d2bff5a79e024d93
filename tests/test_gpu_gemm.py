"""gemm80w4_f64_kernel (csrc/gemm_f64.h), launched directly through the
acl_internal_gemm_f64 hook on descriptors made here, against the longdouble
reference and the derived bound of tests/gemm_ref.py: shapes and transposes,
LDS-DMA staging and the boundaries of the rule that allows it, symmetric
products with the fused err2 / trp reductions, the operand transform, the
scaled Newton-Schulz update, the quintic band, the gate and the skip flag.

Every D has ldd = m + 5 and two extra columns, filled with a NaN pattern
before the call; every byte outside m x n must keep it. Operands are padded
with another NaN pattern, so a read outside an operand poisons the result.
Each test prints its largest error / bound.

The two stagings differ only in how a K step's operands reach LDS: the zero
fill, the transform's expression, the order of the K steps and the MFMA
sequence of every accumulator are the same code (the K loops' mm / dstep and
the shared epilogue), so the LDS-DMA results are asserted bit-equal to the
register-staged ones."""
import ctypes as ct

import numpy as np
import pytest

import gemm_ref as R

pytestmark = pytest.mark.gpu


def _nanfill(n, bits):
    return np.full(n, bits, np.uint64).view(np.float64)


class Launch:
    """One call of the hook on host jobs: builds the device operands and the
    records, runs, and reads the outputs back."""

    def __init__(self, jobs, sym=0, staging=0):
        import torch
        from aclswarm_amd import _lib as L
        self.L, self.torch = L, torch
        self.dev = torch.device("cuda:0")
        self.jobs, self.sym, self.staging = jobs, sym, staging
        self.keep = []
        self.recs = (L.GemmJobRec * len(jobs))()
        self.Dbuf, self.scal, self.trp = [], [], []
        ta, tb = jobs[0].ta, jobs[0].tb
        assert all(j.ta == ta and j.tb == tb for j in jobs)
        self.ta, self.tb = ta, tb
        for j, r in zip(jobs, self.recs):
            self._fill(j, r)

    def _up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.keep.append(t)
        return t

    def _matrix(self, x, pad, off=0):
        """x (r x c) column-major with leading dimension r + pad behind `off`
        doubles, everything else NaN; returns (address, ld)."""
        r, c = x.shape
        ld = r + pad
        buf = _nanfill(off + ld * c, R.PAD_BITS)
        buf[off:].reshape(c, ld)[:, :r] = x.T
        t = self._up(buf)
        return (t.data_ptr() + 8 * off if buf.size else 0), ld

    def _fill(self, j, r):
        r.m, r.n, r.k = j.m, j.n, j.k
        r.alpha, r.beta = j.alpha, j.beta
        r.A, r.lda = self._matrix(j.A, j.pad_a, j.off_a)
        r.B, r.ldb = self._matrix(j.B, j.pad_b, j.off_b)
        ldd = j.m + 5
        d = _nanfill(ldd * (j.n + 2), R.SENTINEL_BITS)
        if j.alias_c:
            d.reshape(j.n + 2, ldd)[:j.n, :j.m] = j.C.T
        D = self._up(d)
        self.Dbuf.append(D)
        r.D, r.ldd = D.data_ptr(), ldd
        if j.alias_c:
            r.C, r.ldc = r.D, ldd
        elif j.C is not None:
            r.C, r.ldc = self._matrix(j.C, j.pad_c)
        else:
            r.C, r.ldc = None, j.m + 3
        # scalars: [tnrm, nserr, gerr, err2], then the partials
        nsp = [] if j.nsp is None else list(j.nsp)
        s = self._up(np.array([j.tnrm or 0.0, j.nserr or 0.0, j.gerr or 0.0, 0.0] + nsp))
        self.scal.append(s)
        p = s.data_ptr()
        r.tmask, r.tdiag = j.tmask, j.tdiag
        r.tnrm = p if j.tnrm is not None else None
        r.nserr = p + 8 if j.nserr is not None else None
        r.gerr, r.glo, r.ghi = (p + 16 if j.gerr is not None else None), j.glo, j.ghi
        r.err2 = p + 24 if j.err2 else None
        r.nsp, r.nsn = (p + 32 if nsp else None), len(nsp)
        r.nscap, r.nstol = j.nscap, j.nstol
        if j.skip is not None:
            r.skip = self._up(np.array([j.skip], np.int32)).data_ptr()
        nt = (j.m + R.TILE - 1) // R.TILE
        if j.trp:
            t = self._up(_nanfill(nt + 2, R.SENTINEL_BITS))
            self.trp.append(t)
            r.trp = t.data_ptr()
        else:
            self.trp.append(None)
        if j.qB is not None:
            r.qB, ldq = self._matrix(j.qB, j.pad_b)
            assert ldq == r.ldb
            r.qlo, r.qhi, r.qalpha, r.qbeta = j.qlo, j.qhi, j.qalpha, j.qbeta

    def run(self, expect_rc=0):
        ran = ct.c_int(-1)
        rc = self.L.lib().acl_internal_gemm_f64(self.ta, self.tb, self.sym, self.staging,
                                                self.recs, len(self.jobs), ct.byref(ran))
        assert rc == expect_rc, rc
        self.dma_ran = ran.value
        return self

    def D(self, i):
        """(D as m x n, whether every byte outside it kept the sentinel)."""
        j = self.jobs[i]
        buf = self.Dbuf[i].cpu().numpy().reshape(j.n + 2, j.m + 5)
        out = np.ones(buf.shape, bool)
        out[:j.n, :j.m] = False
        border = (buf.view(np.uint64)[out] == np.uint64(R.SENTINEL_BITS)).all()
        return buf[:j.n, :j.m].T.copy(), bool(border)

    def untouched(self, i):
        buf = self.Dbuf[i].cpu().numpy()
        return bool((buf.view(np.uint64) == np.uint64(R.SENTINEL_BITS)).all())

    def err2(self, i):
        return float(self.scal[i].cpu().numpy()[3])

    def trps(self, i):
        return self.trp[i].cpu().numpy()


def _reference(job):
    if not hasattr(job, "_ref"):
        job._ref = R.reference(job)
    return job._ref


def _check(launch, sym=False):
    """Every job's D within its bound, its border untouched; the largest
    error / bound and the Ds."""
    worst, Ds = 0.0, []
    for i, j in enumerate(launch.jobs):
        D, border = launch.D(i)
        assert border, ("a write outside m x n", j.name)
        ref, bound = _reference(j)
        r = R.ratios(D, ref, bound, sym)
        rm = float(r.max()) if r.size else 0.0
        assert rm <= 1.0, (j.name, rm, np.unravel_index(r.argmax(), r.shape))
        if sym:
            assert R.mirror_equal(D), j.name
        worst = max(worst, rm)
        Ds.append(D)
    return worst, Ds


def _bits_equal(a, b):
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def test_record_mirrors_the_native_struct(cuda):
    from aclswarm_amd import _lib as L
    assert L.lib().acl_internal_gemm_job_size() == ct.sizeof(L.GemmJobRec)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_shapes_and_transposes(cuda, ta, tb):
    """Nine jobs in one launch (past one group of eight), register staging:
    with a separate C, with beta = 0 and C NULL, with C aliasing D."""
    worst = 0.0
    for variant in ("c", "noc", "alias"):
        la = Launch(R.shape_jobs(ta, tb, variant), staging=0).run()
        assert la.dma_ran == 0
        w, _ = _check(la)
        worst = max(worst, w)
    print("shapes ta=%d tb=%d: largest error / bound %.3f" % (ta, tb, worst))


def test_lds_dma_staging(cuda):
    jobs = R.dma_jobs()
    reg = Launch(jobs, staging=0).run()
    dma = Launch(jobs, staging=1).run()
    assert reg.dma_ran == 0 and dma.dma_ran == 1
    w0, D0 = _check(reg)
    w1, D1 = _check(dma)
    diff = max(float(np.abs(a - b).max()) for a, b in zip(D0, D1))
    print("LDS-DMA: largest error / bound %.3f (registers %.3f), largest difference between "
          "the stagings %.3e" % (w1, w0, diff))
    for j, a, b in zip(jobs, D0, D1):
        assert _bits_equal(a, b), j.name


@pytest.mark.parametrize("kind", R.INELIGIBLE)
def test_dma_eligibility_boundaries(cuda, kind):
    """A request for the host's staging decision on a job the rule refuses,
    alone and among jobs it allows: the LDS-DMA kernel does not run, and the
    results are right."""
    alone = Launch([R.eligibility_job(kind)], staging=1).run()
    assert alone.dma_ran == 0
    w0, _ = _check(alone)
    batch = [R.eligibility_job(None, 1), R.eligibility_job(kind), R.eligibility_job(None, 2)]
    mixed = Launch(batch, staging=1).run()
    assert mixed.dma_ran == 0
    w1, _ = _check(mixed)
    # (the batch without the refused job is staged by LDS-DMA)
    ok = Launch([batch[0], batch[2]], staging=1).run()
    assert ok.dma_ran == 1
    w2, _ = _check(ok)
    print("eligibility %s: largest error / bound %.3f" % (kind, max(w0, w1, w2)))


def _check_reductions(launch, Ds):
    worst_e = worst_t = 0.0
    for i, (j, D) in enumerate(zip(launch.jobs, Ds)):
        if not j.err2:
            continue
        e, g = R.err2_reference(D)
        got = R.hp(np.array(launch.err2(i)))[()]
        re = float(abs(got - e) / (g * e))
        assert re <= 1.0, (j.name, "err2", launch.err2(i), float(e), re)
        worst_e = max(worst_e, re)
        parts = R.trp_reference(D)
        t = launch.trps(i)
        assert (t[len(parts):].view(np.uint64) == np.uint64(R.SENTINEL_BITS)).all(), j.name
        for b, (s, tol) in enumerate(parts):
            rt = float(abs(R.hp(np.array(t[b]))[()] - s) / tol)
            assert rt <= 1.0, (j.name, "trp", b, t[b], float(s), rt)
            worst_t = max(worst_t, rt)
    return worst_e, worst_t


def test_symmetric_products(cuda):
    """Y = Z Z with err2 and trp, then U = -0.5 Z Y + 1.5 Z on the stored Y,
    both stagings, each twice: D and trp bit-equal over the runs and the
    stagings (err2 is accumulated atomically and need not be)."""
    ys = R.sym_y_jobs()
    runs = [Launch(ys, sym=1, staging=s).run() for s in (0, 1, 0, 1)]
    assert [la.dma_ran for la in runs] == [0, 1, 0, 1]
    res = [_check(la, sym=True) for la in runs]
    wy = max(w for w, _ in res)
    Y = res[0][1]
    we = wt = 0.0
    for la, (_, Ds) in zip(runs, res):
        e, t = _check_reductions(la, Ds)
        we, wt = max(we, e), max(wt, t)
        for i, j in enumerate(ys):
            assert _bits_equal(Ds[i], Y[i]), j.name
            assert _bits_equal(la.trps(i), runs[0].trps(i)), j.name
    us = R.sym_u_jobs(ys, Y)
    uruns = [Launch(us, sym=1, staging=s).run() for s in (0, 1, 0, 1)]
    assert [la.dma_ran for la in uruns] == [0, 1, 0, 1]
    ures = [_check(la, sym=True) for la in uruns]
    wu = max(w for w, _ in ures)
    for _, Ds in ures:
        for i, j in enumerate(us):
            assert _bits_equal(Ds[i], ures[0][1][i]), j.name
    print("symmetric: largest error / bound Y %.3f, U %.3f; err2 %.3f and trp %.3f of theirs"
          % (wy, wu, we, wt))


def test_operand_transform(cuda):
    worst = 0.0
    w, _ = _check(Launch(R.transform_jobs(81, False), staging=0).run())
    worst = max(worst, w)
    for jobs in (R.transform_jobs(82, True), R.transform_jobs(162, True),
                 R.transform_nonsquare_jobs()):
        reg = Launch(jobs, staging=0).run()
        dma = Launch(jobs, staging=1).run()
        assert reg.dma_ran == 0 and dma.dma_ran == 1
        w0, D0 = _check(reg)
        w1, D1 = _check(dma)
        worst = max(worst, w0, w1)
        for j, a, b in zip(jobs, D0, D1):
            assert _bits_equal(a, b), j.name
    print("transform: largest error / bound %.3f" % worst)


def test_scaled_update(cuda):
    jobs = R.scaled_jobs()
    reg = Launch(jobs, sym=1, staging=0).run()
    dma = Launch(jobs, sym=1, staging=1).run()
    assert reg.dma_ran == 0 and dma.dma_ran == 1
    w0, D0 = _check(reg, sym=True)
    w1, D1 = _check(dma, sym=True)
    for j, a, b in zip(jobs, D0, D1):
        assert _bits_equal(a, b), j.name
    print("scaled update: largest error / bound %.3f" % max(w0, w1))


def test_transformed_first_step_symmetric(cuda):
    """J_NSYF / J_NSUF as the ADMM issues them: the transform inside symmetric
    launches (the diagonal tiles' K loop), with err2, trp and the scaled
    update, under both stagings."""
    jobs = R.first_step_jobs()
    reg = Launch(jobs, sym=1, staging=0).run()
    dma = Launch(jobs, sym=1, staging=1).run()
    assert reg.dma_ran == 0 and dma.dma_ran == 1
    w0, D0 = _check(reg, sym=True)
    w1, D1 = _check(dma, sym=True)
    e0, t0 = _check_reductions(reg, D0)
    e1, t1 = _check_reductions(dma, D1)
    for i, (j, a, b) in enumerate(zip(jobs, D0, D1)):
        assert _bits_equal(a, b), j.name
        if j.trp:
            assert _bits_equal(reg.trps(i), dma.trps(i)), j.name
    print("transformed first step: largest error / bound %.3f; err2 %.3f and trp %.3f of theirs"
          % (max(w0, w1), max(e0, e1), max(t0, t1)))


def test_quintic_band(cuda):
    jobs = R.quintic_jobs()
    reg = Launch(jobs, staging=0).run()
    dma = Launch(jobs, staging=1).run()
    assert reg.dma_ran == 0 and dma.dma_ran == 1
    w0, D0 = _check(reg)
    w1, D1 = _check(dma)
    for j, a, b in zip(jobs, D0, D1):
        assert _bits_equal(a, b), j.name
    print("quintic band: largest error / bound %.3f" % max(w0, w1))


def test_gate_and_skip(cuda):
    jobs = R.gate_skip_jobs()
    worst = 0.0
    for staging in (0, 1):
        la = Launch(jobs, staging=staging).run()
        assert la.dma_ran == staging
        assert la.untouched(0) and la.untouched(1)
        D, border = la.D(2)
        assert border
        r = R.max_ratio(D, jobs[2])
        assert r <= 1.0, r
        worst = max(worst, r)
    print("gate and skip: largest error / bound %.3f" % worst)


def test_hook_refuses_bad_descriptors(cuda):
    """Nonzero, and nothing launched: D keeps its sentinel."""
    rng = np.random.RandomState(9)

    def job(**kw):
        return R.general(rng, 18, 18, 6, alpha=-0.5, beta=1.5, pad_a=2, pad_b=2, **kw)

    def refused(la):
        la.run(expect_rc=1)
        assert la.dma_ran == 0
        assert all(la.untouched(i) for i in range(len(la.jobs)))

    for field in ("m", "n", "k"):
        la = Launch([job(), job()], staging=1)
        setattr(la.recs[1], field, -1)
        refused(la)
    for field, rows in (("lda", 18), ("ldb", 6), ("ldc", 18), ("ldd", 18)):
        la = Launch([job()])
        setattr(la.recs[0], field, rows - 1)
        refused(la)
    la = Launch([job()], sym=1)
    la.recs[0].n = 17
    refused(la)
    la = Launch([job(nsp=np.array([9.0]), nserr=1e-3, nscap=1.7, nstol=1e-12)])
    la.recs[0].nserr = None
    refused(la)
    la = Launch([job(qB=rng.standard_normal((6, 18)), nserr=1e-3, qlo=0.0, qhi=1.0)])
    la.recs[0].nserr = None
    refused(la)
    # (the untouched descriptors run)
    _check(Launch([job(), job()], staging=1).run())
