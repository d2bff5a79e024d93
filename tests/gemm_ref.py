"""Reference, tolerance and cases for the direct tests of the fp64 MFMA GEMM
(csrc/gemm_f64.h: gemm80w4_f64_kernel through the acl_internal_gemm_f64 hook,
tests/test_gpu_gemm.py), and CPU tests that the checker itself would catch a
subtly wrong kernel (collected through tests/test_gemm_ref.py).

Reference: the job's operation, D = alpha op(A)' op(B)' + beta C', on the fp64
operands promoted to np.longdouble (63-bit mantissa; mpmath at 80 bits where
the platform's long double is narrower). X' is the operand as the kernel's
transform reads it, (x - [diagonal] tdiag) / *tnrm for the operands in tmask;
alpha, beta are the ones the kernel's epilogue takes (the scaled Newton-Schulz
update's a = sqrt(m / sum nsp), the quintic band's qalpha, qbeta and qB).

Tolerance (derived, for any summation order with or without FMAs): every
computed term of an element's sum is its exact value times at most c factors
(1 + d), |d| <= u = 2^-53, so

    |D - ref| <= gamma_c (|alpha| |A'| |B'| + |beta| |C'|),  gamma_c = c u / (1 - c u)

elementwise, with c counted from the kernel's expressions:
    k   the dot product (a term passes through at most k additions; the
        products are exact inside an FMA; zero padding adds exactly)
    3   the sum of block (4, 4)'s four per-wave partials
    3   the epilogue: alpha * acc, beta * c, their sum
    3   per operand in tmask: 1 / *tnrm, the subtraction, the product
    3 (nsn + 2) + 3   a scaled update's alpha: a^3 alpha with a from nsn - 1
        additions, a quotient and a square root (taken as two roundings)
    (the scaled beta, (nsn + 2) + 1, is covered by alpha's count)
Plain jobs: c = k + 9. The reference's own rounding, at most the same count
of factors with u = 2^-64, is added to the bound (a factor 1 + 2^-11).
"""
import numpy as np

LD = np.longdouble
HAVE_LD = np.finfo(LD).nmant >= 63
U = 2.0 ** -53
TILE = 80

# what D's border and the operands' padding are filled with: NaNs with a
# payload (a read of padding poisons the result, a stray write shows)
SENTINEL_BITS = 0x7FF8A5A55A5A0DD0
PAD_BITS = 0x7FF8BAD0BAD0BAD0


def _nan(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


def hp(x):
    """fp64 values promoted to the reference's precision."""
    x = np.asarray(x, np.float64)
    if HAVE_LD:
        return x.astype(LD)
    import mpmath
    mpmath.mp.prec = 80
    out = np.empty(x.shape, object)
    for i, v in np.ndenumerate(x):
        out[i] = mpmath.mpf(float(v))
    return out


def _hp_scalar(v):
    return hp(np.array(float(v)))[()]


def _hp_sqrt(v):
    if HAVE_LD:
        return np.sqrt(v)
    import mpmath
    return mpmath.sqrt(v)


def gamma(c):
    return c * U / (1.0 - c * U)


class Job:
    """One GEMM job on the host: the stored operands (A is m x k, or k x m
    under ta; B is k x n, or n x k under tb; C, qB as D), the scalars the
    descriptor's pointers point at as values, and how the GPU test lays the
    operands out (leading dimension = rows + pad, offsets in doubles)."""

    def __init__(self, m, n, k, A, B, C=None, alpha=1.0, beta=0.0, ta=0, tb=0, **kw):
        self.m, self.n, self.k, self.ta, self.tb = m, n, k, ta, tb
        self.A, self.B, self.C = A, B, C
        self.alpha, self.beta = float(alpha), float(beta)
        self.skip = None          # *skip, or None for a NULL pointer
        self.err2 = False         # accumulate |D - I|_F^2
        self.trp = False          # store the diagonal tiles' trace partials
        self.tmask, self.tdiag, self.tnrm = 0, 0.0, None
        self.nsp, self.nserr, self.nscap, self.nstol = None, None, 0.0, 0.0
        self.gerr, self.glo, self.ghi = None, 0.0, 0.0
        self.qB, self.qlo, self.qhi, self.qalpha, self.qbeta = None, 0.0, 0.0, 0.0, 0.0
        # layout on the device
        self.pad_a = self.pad_b = self.pad_c = 3
        self.off_a = self.off_b = 0
        self.alias_c = False      # C is D (D pre-filled with C)
        self.name = ""
        for key, v in kw.items():
            assert hasattr(self, key), key
            setattr(self, key, v)
        ra, ca = (k, m) if ta else (m, k)
        rb, cb = (n, k) if tb else (k, n)
        assert A.shape == (ra, ca) and B.shape == (rb, cb), (A.shape, B.shape, m, n, k)
        assert C is None or C.shape == (m, n)
        assert self.beta == 0.0 or C is not None

    @property
    def nsn(self):
        return 0 if self.nsp is None else len(self.nsp)

    def runs(self):
        if self.skip:
            return False
        if self.gerr is not None and not (self.glo <= self.gerr < self.ghi):
            return False
        return True

    def quintic(self):
        return self.qB is not None and self.qlo <= self.nserr < self.qhi

    def scale(self):
        """a of the scaled update in the reference's precision (None: the
        update is unscaled), as the kernel decides it."""
        if self.quintic() or self.nsp is None or self.nserr < self.nstol:
            return None
        tr = hp(np.asarray(self.nsp)).sum()
        # the decision on the fp64 partials summed in order, as the kernel sums them
        tr64 = 0.0
        for p in self.nsp:
            tr64 += float(p)
        if tr64 < 0.0 or tr64 != tr64:
            return None  # sqrt of a negative ratio: not a number, unscaled
        cap = _hp_scalar(self.nscap)
        if tr64 == 0.0:
            return cap  # m / 0 = inf, capped
        a = _hp_sqrt(_hp_scalar(self.m) / tr)
        return a if a < cap else cap

    def roundings(self):
        c = self.k + 9 + 3 * bin(self.tmask & 7).count("1")
        if self.nsp is not None:
            c += 3 * (self.nsn + 2) + 3
        return c


def _transform(x, on, job):
    """The operand as the kernel reads it, in the reference's precision: the
    diagonal is where the operand's own row and column indices are equal."""
    x = hp(x)
    if not on:
        return x
    r, c = x.shape
    d = np.zeros((r, c))
    np.fill_diagonal(d, job.tdiag)
    return (x - hp(d)) / _hp_scalar(job.tnrm)


def operands(job):
    """op(A)' (m x k), op(B)' (k x n), C' (m x n or None), alpha, beta in the
    reference's precision, as the kernel's job takes them."""
    quint = job.quintic()
    A = job.A.T if job.ta else job.A
    if quint:
        B, tB = job.qB, False
        assert not job.tb
    else:
        B, tB = (job.B.T if job.tb else job.B), bool(job.tmask & 2)
    Ap = _transform(A, job.tmask & 1, job)
    Bp = _transform(B, tB, job)
    alpha, beta = _hp_scalar(job.alpha), _hp_scalar(job.beta)
    if quint:
        alpha, beta = _hp_scalar(job.qalpha), _hp_scalar(job.qbeta)
    else:
        a = job.scale()
        if a is not None:
            alpha, beta = alpha * a * a * a, beta * a
    Cp = None
    if beta != 0:
        Cp = _transform(job.C, job.tmask & 4, job)
    return Ap, Bp, Cp, alpha, beta


def reference(job):
    """(ref, bound): the job's D in the reference's precision and the
    elementwise error bound of the module docstring."""
    Ap, Bp, Cp, alpha, beta = operands(job)
    m, n = job.m, job.n
    if job.k > 0:
        prod = Ap @ Bp
        mag = np.abs(Ap) @ np.abs(Bp)
    else:
        prod = hp(np.zeros((m, n)))
        mag = hp(np.zeros((m, n)))
    ref = alpha * prod
    mag = abs(alpha) * mag
    if Cp is not None:
        ref = ref + beta * Cp
        mag = mag + abs(beta) * np.abs(Cp)
    g = gamma(job.roundings()) * (1.0 + 2.0 ** -11)
    return ref, mag * _hp_scalar(g)


def ratios(D, ref, bound, sym=False):
    """|D - ref| / bound elementwise (0 where both vanish, inf where only the
    bound does; a NaN in D gives inf). sym: an element may instead be within
    ref[j, i]'s bound of ref[j, i] (the exact product of a symmetric launch
    need not be exactly symmetric, and the kernel stores one of the two)."""
    fin = np.isfinite(D)
    Dh = hp(np.where(fin, D, 0.0))

    def one(ref, bound):
        err = np.abs(Dh - ref)
        pos = bound > 0
        q = np.asarray(err / np.where(pos, bound, 1), dtype=np.float64)
        out = np.where(pos, q, np.where(err == 0, 0.0, np.inf))
        return np.where(fin, out, np.inf)
    r = one(ref, bound)
    if sym:
        r = np.minimum(r, one(ref.T, bound.T))
    return r


def max_ratio(D, job, sym=False):
    ref, bound = reference(job)
    return float(ratios(D, ref, bound, sym).max()) if D.size else 0.0


def mirror_equal(D):
    """Outside the diagonal 16-blocks D[j, i] has the bits of D[i, j]."""
    N = D.shape[0]
    b = np.arange(N) // 16
    off = b[:, None] != b[None, :]
    v = np.ascontiguousarray(D).view(np.uint64)
    return bool((v == v.T)[off].all())


def err2_reference(D):
    """sum (D - I)^2 over the stored D, and the relative bound gamma_(N N + 4)
    (every term is non-negative)."""
    N = D.shape[0]
    d = hp(D) - hp(np.eye(N))
    return (d * d).sum(), gamma(N * N + 4)


def trp_reference(D):
    """Per diagonal tile: the sum of the stored diagonal, and gamma_84 on the
    sum of its magnitudes."""
    N = D.shape[0]
    dg = hp(np.diag(D).copy())
    out = []
    for b in range((N + TILE - 1) // TILE):
        seg = dg[b * TILE:(b + 1) * TILE]
        out.append((seg.sum(), np.abs(seg).sum() * _hp_scalar(gamma(84))))
    return out


# ---------------------------------------------------------------------------
# a float64 model of the kernel (numpy's product: some summation order), with
# the mutations the checker must catch

MUTATIONS = ("drop_k", "drop_last_step", "a_transposed", "mirror_wrong_side", "diag_at_ij",
             "no_beta_c")


def model_f64(job, mutate=None):
    """The job in float64 with the kernel's own expressions around numpy's
    product. mutate: one of MUTATIONS --
    drop_k: one k term left out; drop_last_step: the last (partial) K step of
    16 left out; a_transposed: A (square) read with the other transpose flag;
    mirror_wrong_side: the triangle below the diagonal 16-blocks written from
    the one above, as a symmetric launch does, on a product that is not
    symmetric; diag_at_ij: the transform's diagonal judged by the output
    element's (gi == gj) instead of the operand's own (gi == gk, gj == gkb);
    no_beta_c: beta C left out."""
    assert mutate is None or mutate in MUTATIONS
    m, n, k = job.m, job.n, job.k
    quint = job.quintic()
    A = job.A
    ta = job.ta
    if mutate == "a_transposed":
        assert m == k
        ta = not ta
    A = A.T if ta else A
    if quint:
        B, tB = job.qB, False
    else:
        B, tB = (job.B.T if job.tb else job.B), bool(job.tmask & 2)
    tinv = 1.0 / job.tnrm if job.tmask else 1.0

    def tr(x, on, diag=True):
        if not on:
            return x
        d = np.zeros(x.shape)
        if diag:
            np.fill_diagonal(d, job.tdiag)
        return (x - d) * tinv

    alpha, beta = job.alpha, job.beta
    if quint:
        alpha, beta = job.qalpha, job.qbeta
    elif job.nsp is not None and not (job.nserr < job.nstol):
        t = 0.0
        for p in job.nsp:
            t += float(p)
        with np.errstate(all="ignore"):
            a = np.sqrt(np.float64(m) / np.float64(t))
        if a == a:
            ac = a if a < job.nscap else job.nscap
            alpha *= ac * ac * ac
            beta *= ac
    if mutate == "diag_at_ij" and (job.tmask & 3):
        # off the output's diagonal no operand diagonal is seen; on it every
        # k term of the transformed operands loses tdiag
        Ap, Bp = tr(A, job.tmask & 1, False), tr(B, tB, False)
        acc = Ap @ Bp
        for i in range(min(m, n)):
            ai = (A[i, :] - job.tdiag) * tinv if job.tmask & 1 else A[i, :]
            bi = (B[:, i] - job.tdiag) * tinv if tB else B[:, i]
            acc[i, i] = ai @ bi
    else:
        Ap, Bp = tr(A, job.tmask & 1), tr(B, tB)
        if mutate == "drop_k":
            keep = np.ones(k, bool)
            keep[k // 2] = False
            Ap, Bp = Ap[:, keep], Bp[keep, :]
        if mutate == "drop_last_step":
            last = 16 * ((k - 1) // 16)
            Ap, Bp = Ap[:, :last], Bp[:last, :]
        acc = Ap @ Bp if Ap.shape[1] else np.zeros((m, n))
    D = alpha * acc
    if beta != 0.0 and mutate != "no_beta_c":
        D = D + beta * tr(job.C, job.tmask & 4)
    if mutate == "mirror_wrong_side":
        assert m == n
        b = np.arange(m) // 16
        low = b[:, None] > b[None, :]
        D = np.where(low, D.T, D)
    return D


# ---------------------------------------------------------------------------
# cases (shared by the GPU tests and the checker's own tests)

SHAPES = ((1, 1, 1), (15, 17, 3), (16, 16, 4), (17, 33, 16), (79, 81, 17), (80, 80, 32),
          (81, 161, 33), (96, 100, 5), (40, 24, 0))
DMA_SHAPES = ((2, 2, 2), (16, 16, 16), (78, 83, 18), (80, 80, 80), (82, 161, 34),
              (160, 162, 50))
SYM_SIZES = (16, 80, 82, 96, 162, 242)


def _mat(rng, r, c):
    """Entries of either sign with magnitudes in [0.5, 1.5): no term of a
    product is negligible, so a lost term shows in every element."""
    return rng.uniform(0.5, 1.5, (r, c)) * rng.choice([-1.0, 1.0], (r, c))


def general(rng, m, n, k, ta=0, tb=0, with_c=True, **kw):
    A = _mat(rng, *((k, m) if ta else (m, k)))
    B = _mat(rng, *((n, k) if tb else (k, n)))
    C = _mat(rng, m, n) if with_c else None
    return Job(m, n, k, A, B, C, ta=ta, tb=tb, **kw)


def shape_jobs(ta, tb, variant):
    """The nine shapes in one launch. variant: 'c' alpha = -0.5, beta = 1.5
    with a separate C; 'noc' beta = 0 and C NULL; 'alias' C aliasing D."""
    rng = np.random.RandomState(100 + 2 * ta + tb)
    jobs = []
    for m, n, k in SHAPES:
        j = general(rng, m, n, k, ta, tb, alpha=-0.5, beta=1.5, name="%dx%dx%d" % (m, n, k))
        if variant == "noc":
            j.beta, j.C = 0.0, None
        j.alias_c = variant == "alias"
        jobs.append(j)
    return jobs


def dma_jobs():
    """Untransposed, even leading dimensions (rows + 2 or rows + 4), aligned."""
    rng = np.random.RandomState(200)
    jobs = []
    for i, (m, n, k) in enumerate(DMA_SHAPES):
        jobs.append(general(rng, m, n, k, alpha=-0.5, beta=1.5, pad_a=2 + 2 * (i & 1),
                            pad_b=4 - 2 * (i & 1), name="%dx%dx%d" % (m, n, k)))
    return jobs


INELIGIBLE = ("odd_m", "odd_k", "odd_lda", "odd_ldb", "a_off8", "b_off8", "tmask8")


def eligibility_job(kind, seed=0):
    """A two-tile-row product that LDS-DMA may stage (kind None), or the same
    with one property the rule refuses."""
    rng = np.random.RandomState(300 + seed)
    m, n, k = 82, 83, 34
    if kind == "odd_m":
        m = 81
    if kind == "odd_k":
        k = 33
    j = general(rng, m, n, k, alpha=-0.5, beta=1.5, pad_a=2, pad_b=2, name=str(kind))
    if kind == "odd_m":
        j.pad_a = 3  # (lda stays even: only m is odd)
    if kind == "odd_k":
        j.pad_b = 3
    if kind == "odd_lda":
        j.pad_a = 3
    if kind == "odd_ldb":
        j.pad_b = 3
    if kind == "a_off8":
        j.off_a = 1
    if kind == "b_off8":
        j.off_b = 1
    if kind == "tmask8":  # a bit the kernel does not know: nothing is transformed
        j.tmask, j.tdiag, j.tnrm = 8, 0.37, 2.7
    return j


def sym_matrix(rng, N):
    R = _mat(rng, N, N) / np.sqrt(N)
    return 0.5 * (R + R.T)


def sym_y_jobs():
    """Y = Z Z, Z symmetric, with err2 and trp, one job per size."""
    rng = np.random.RandomState(400)
    jobs = []
    for N in SYM_SIZES:
        Z = sym_matrix(rng, N)
        jobs.append(Job(N, N, N, Z, Z, None, 1.0, 0.0, err2=True, trp=True, pad_a=2, pad_b=2,
                        name="Y%d" % N))
    return jobs


def sym_u_jobs(y_jobs, Ys):
    """U = -0.5 Z Y + 1.5 Z on the stored Ys."""
    return [Job(j.m, j.m, j.m, j.A, Y, j.A, -0.5, 1.5, pad_a=2, pad_b=2, pad_c=2,
                name="U%d" % j.m) for j, Y in zip(y_jobs, Ys)]


TRANSFORM_MASKS = (1, 2, 3, 4, 5, 7)


def transform_jobs(N, staging_both):
    """One job per tmask on general N x N operands (and the non-square
    82 x 50 x 34 with the sizes that LDS-DMA may stage)."""
    rng = np.random.RandomState(500 + N)
    jobs = []
    for tm in TRANSFORM_MASKS:
        jobs.append(general(rng, N, N, N, alpha=-0.5, beta=1.5, tmask=tm, tdiag=0.37, tnrm=2.7,
                            pad_a=2 if staging_both else 3, pad_b=2 if staging_both else 3,
                            name="N%d tmask%d" % (N, tm)))
    return jobs


def transform_nonsquare_jobs():
    rng = np.random.RandomState(550)
    return [general(rng, 82, 50, 34, alpha=-0.5, beta=1.5, tmask=tm, tdiag=0.37, tnrm=2.7,
                    pad_a=2, pad_b=2, name="82x50x34 tmask%d" % tm) for tm in TRANSFORM_MASKS]


SCALED_KINDS = ("scaled", "capped", "converged", "zero", "negative")


def scaled_jobs():
    """U = -0.5 Z Y + 1.5 Z with the scaled update's fields, N = 82 (two
    partials) and 162 (three): a below the cap; above it; *nserr < nstol
    (unscaled); partials summing to 0 (a infinite, capped); to a negative
    number (a not a number, unscaled)."""
    rng = np.random.RandomState(600)
    jobs = []
    for N in (82, 162):
        nsn = (N + TILE - 1) // TILE
        Z = sym_matrix(rng, N)
        Y = Z @ Z
        Y = np.triu(Y) + np.triu(Y, 1).T
        for kind in SCALED_KINDS:
            part = rng.uniform(0.5, 1.5, nsn)
            part *= N / 1.44 / part.sum()  # a = sqrt(N / sum) ~ 1.2
            nscap, nserr = 1.7, 1e-3
            if kind == "capped":
                nscap = 1.1
            if kind == "converged":
                nserr = 1e-13 * N
            if kind == "zero":
                part = np.array([1.0, -1.0, 0.0][:nsn]) if nsn == 3 else np.array([1.0, -1.0])
            if kind == "negative":
                part = -part
            jobs.append(Job(N, N, N, Z, Y, Z, -0.5, 1.5, nsp=part, nserr=nserr, nscap=nscap,
                            nstol=1e-12 * N, pad_a=2, pad_b=2, pad_c=2,
                            name="N%d %s" % (N, kind)))
    return jobs


def first_step_jobs():
    """The sign iteration's first step as the ADMM issues it (J_NSYF, J_NSUF):
    symmetric launches that read Z0 = (W - tdiag I) / *tnrm through the
    transform -- Y = Z0 Z0 (tmask 3, with err2 and trp) and the scaled
    U = -0.5 Z0 Y + 1.5 Z0 (tmask 5) -- so that the diagonal tiles' K loop
    meets the transform too, under either staging."""
    rng = np.random.RandomState(650)
    jobs = []
    for N in (82, 162):
        nsn = (N + TILE - 1) // TILE
        W = 2.7 * sym_matrix(rng, N)
        kw = dict(tdiag=0.37, tnrm=2.7, pad_a=2, pad_b=2, pad_c=2)
        jobs.append(Job(N, N, N, W, W, None, 1.0, 0.0, tmask=3, err2=True, trp=True,
                        name="first Y %d" % N, **kw))
        Z0 = (W - 0.37 * np.eye(N)) / 2.7
        Y = Z0 @ Z0
        Y = np.triu(Y) + np.triu(Y, 1).T
        part = rng.uniform(0.5, 1.5, nsn)
        part *= N / 1.44 / part.sum()
        jobs.append(Job(N, N, N, W, Y, W, -0.5, 1.5, tmask=5, nsp=part, nserr=1e-3, nscap=1.7,
                        nstol=1e-12 * N, name="first U %d" % N, **kw))
    return jobs


def quintic_jobs():
    """tmask = 7 with qB set: *nserr inside [qlo, qhi) (B read from qB,
    untransformed, qalpha / qbeta, unscaled) and outside (the ordinary scaled
    product)."""
    rng = np.random.RandomState(700)
    jobs = []
    N = 82
    for inside in (True, False):
        j = general(rng, N, N, N, alpha=-0.5, beta=1.5, tmask=7, tdiag=0.37, tnrm=2.7,
                    pad_a=2, pad_b=2, name="quintic " + ("inside" if inside else "outside"))
        j.qB = _mat(rng, N, N)
        j.qlo, j.qhi, j.qalpha, j.qbeta = 1e-10, 1e-6, 1.0, 1.875
        j.nserr = 1e-8 if inside else 1e-3
        j.nsp, j.nscap, j.nstol = np.array([30.0, 27.0]), 1.7, 1e-10
        jobs.append(j)
    return jobs


def gate_skip_jobs():
    rng = np.random.RandomState(800)
    mk = lambda name, **kw: general(rng, 82, 82, 34, alpha=-0.5, beta=1.5, pad_a=2, pad_b=2,
                                    name=name, **kw)
    return [mk("gated out", gerr=1e-3, glo=1e-10, ghi=1e-6), mk("skipped", skip=1),
            mk("runs", gerr=1e-8, glo=1e-10, ghi=1e-6, skip=0)]


def all_case_groups():
    """{group: [(job, sym)]}: every job of every GPU case, for the checker's
    own tests (the symmetric U products on a float64 Y)."""
    g = {}
    g["shapes"] = [(j, False) for ta in (0, 1) for tb in (0, 1) for v in ("c", "noc", "alias")
                   for j in shape_jobs(ta, tb, v)]
    g["dma"] = [(j, False) for j in dma_jobs()]
    g["eligibility"] = [(eligibility_job(k), False) for k in (None,) + INELIGIBLE]
    ys = sym_y_jobs()
    Ys = [model_f64(j) for j in ys]
    g["sym"] = [(j, True) for j in ys + sym_u_jobs(ys, Ys)]
    g["transform"] = [(j, False) for N, both in ((81, False), (82, True), (162, True))
                      for j in transform_jobs(N, both)] + [
        (j, False) for j in transform_nonsquare_jobs()]
    g["scaled"] = [(j, True) for j in scaled_jobs()]
    g["first_step"] = [(j, True) for j in first_step_jobs()]
    g["quintic"] = [(j, False) for j in quintic_jobs()]
    g["gate_skip"] = [(j, False) for j in gate_skip_jobs() if j.runs()]
    return g


# ---------------------------------------------------------------------------
# the checker's own tests (no GPU)

def test_reference_precision():
    """np.longdouble with a 63-bit mantissa, or mpmath at 80 bits in its place."""
    if np.finfo(np.longdouble).nmant >= 63:
        assert HAVE_LD and hp(np.ones(1)).dtype == np.longdouble
    else:
        import mpmath
        assert not HAVE_LD and isinstance(hp(np.ones(1))[0], mpmath.mpf)
    one = hp(np.array([1.0]))[0]
    assert one + _hp_scalar(2.0 ** -60) != one  # more than fp64's 53 bits


def test_float64_product_passes_every_case():
    for group, jobs in all_case_groups().items():
        worst = 0.0
        for j, sym in jobs:
            r = max_ratio(model_f64(j), j, sym)
            assert r <= 1.0, (group, j.name, r)
            worst = max(worst, r)
        print("%-12s float64 numpy product: largest error / bound %.3f" % (group, worst))


def _fails(job, mutate, sym=False):
    ref, bound = reference(job)
    r = ratios(model_f64(job, mutate), ref, bound, sym)
    return float(r.max())


def test_dropped_k_term_fails_in_every_element():
    for ta in (0, 1):
        for tb in (0, 1):
            for j in shape_jobs(ta, tb, "c"):
                if j.k == 0:
                    continue
                ref, bound = reference(j)
                r = ratios(model_f64(j, "drop_k"), ref, bound)
                assert r.min() > 1e7, (j.name, r.min())
    for j in dma_jobs():
        ref, bound = reference(j)
        assert ratios(model_f64(j, "drop_k"), ref, bound).min() > 1e7, j.name


def test_dropped_last_k_step_fails():
    for j in shape_jobs(0, 0, "c") + dma_jobs() + transform_nonsquare_jobs():
        if j.k == 0:
            continue
        assert _fails(j, "drop_last_step") > 1e7, j.name


def test_a_read_transposed_fails():
    for N, both in ((81, False), (82, True)):
        for j in transform_jobs(N, both):
            assert _fails(j, "a_transposed") > 1e7, j.name


def test_mirror_from_the_wrong_side_fails():
    """On a product that is not symmetric the plain check refuses a mirrored
    triangle; on the symmetric cases the mirrored model passes the symmetric
    check and is bit-symmetric off the diagonal blocks."""
    for j in transform_jobs(82, True) + quintic_jobs():
        assert _fails(j, "mirror_wrong_side") > 1e7, j.name
    ys = sym_y_jobs()
    for j in ys:
        D = model_f64(j, "mirror_wrong_side")
        assert mirror_equal(D)
        assert max_ratio(D, j, sym=True) <= 1.0
    R = np.random.RandomState(1).standard_normal((40, 40))
    assert not mirror_equal(R)


def test_transform_diagonal_at_output_indices_fails():
    for j in transform_nonsquare_jobs():
        if j.tmask & 3:
            assert _fails(j, "diag_at_ij") > 1e7, j.name


def test_omitted_beta_c_fails():
    for group, jobs in all_case_groups().items():
        for j, sym in jobs:
            if j.beta != 0.0 and j.m > 0:
                assert _fails(j, "no_beta_c", sym) > 1e7, (group, j.name)


def test_scaled_reference_takes_the_kernels_branches():
    want = {"scaled": "a", "capped": "cap", "converged": None, "zero": "cap", "negative": None}
    for j in scaled_jobs():
        kind = j.name.split()[1]
        a = j.scale()
        if want[kind] is None:
            assert a is None
        elif want[kind] == "cap":
            assert float(a) == j.nscap
        else:
            assert 1.0 < float(a) < j.nscap
    inside, outside = quintic_jobs()
    assert inside.quintic() and inside.scale() is None
    assert not outside.quintic() and outside.scale() is not None


def test_err2_and_trp_references_on_the_float64_model():
    for j in sym_y_jobs():
        D = model_f64(j)
        e, g = err2_reference(D)
        e64 = ((D - np.eye(j.m)) ** 2).sum()
        assert abs(hp(np.array(e64))[()] - e) <= g * e
        parts = trp_reference(D)
        assert len(parts) == (j.m + TILE - 1) // TILE
        for b, (s, tol) in enumerate(parts):
            s64 = np.diag(D)[b * TILE:(b + 1) * TILE].sum()
            assert abs(hp(np.array(s64))[()] - s) <= tol
