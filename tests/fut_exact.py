"""Exact per-year probabilities of the future engine's model, and the
binomial test that holds the kernels' counts to them.

Every other reference of the future engine (oracle/spom_future_oracle.c, the
numpy checkers of test_future_wide_host.py and test_future_summary_host.py)
replays the simulation loop on the kernels' own random stream and asks for
equal counts.  An error they share with the kernels -- a draw used twice, a
pressure from the wrong occupancy, a source row off by one, a border weight --
is invisible to equality.  The three references here use no random stream:
they are matrices and closed forms of the model of
main_MIDASPOM_future.c:64-110 (one year) and :343-386 (the replicate loop),
and a count over N replicates is tested against them as a binomial variate.
Nothing here imports the oracle or the checkers.

    chain     the 2^n-state Markov chain, n <= 10, every year: P(all empty),
              the distribution of the number occupied, P(patch k occupied)
    year1     P(patch k occupied after the first year) for any n, where the
              clamp of pC cannot bind (the real dispersal coupling)
    isolated  d/m >= 100: the patches decouple, every patch its own two-state
              chain, any n, every year (Poisson-binomial for the number
              occupied)

The model.  Posterior cell (ie, ic) has e = 0.01 ie, c = 0.01 ic and is drawn
with probability w_ie w_ic post[ie, ic] / pscale, w = 1/2 on the border,
pscale = (s-1)^2.  E = min(1, e/K_D).  An occupied patch survives the year
with probability 1 - E, independently; then every patch k that is empty is
colonised with probability pC_k(z) = min(1, c s1_k(z)),
s1_k(z) = sum_{l in z, l != k} M[l][k] K_D + M[n][k] K_S, over the set z of
*survivors*.  A missing patch of the last survey is occupied or empty with
probability 1/2 each, all completions equally likely.

Full mass.  Every case uses a posterior whose weighted mass is pscale up to
rounding, so that (but for the one draw in 2^31 that equals RAND_MAX) no
replicate carries the previous one's (e, c) over: the replicates are then
independent and every count is binomial(N, p).  The carry-over under a smaller
mass makes replicates dependent; it stays the business of the equality tests.

Precision.  Ordinary doubles: the references are exact to about 1e-15 (they
agree with each other to 1e-12, test_future_exact.py), the statistical
resolution at 10^5 to 10^6 replicates is 1e-3 to 1e-4 in p.

Discreteness.  The kernels compare u = r / RAND_MAX, r uniform on [0, 2^31),
RAND_MAX = 2^31 - 1, with a threshold x in [0, 1].  P(u > x) =
1 - (floor(x RAND_MAX) + 1) / 2^31 for x < 1 and P(u < x) =
ceil(x RAND_MAX) / 2^31; since x RAND_MAX / 2^31 = x - x 2^-31, both lie within
2^-31 of 1 - x and x.  The posterior's inverse CDF moves both ends of a cell by
at most that, the cell's probability by at most 2^-30.  So any single
probability of the model is off by at most 2^-30 = 9.3e-10, and a cell of a
table that depends on D draws by at most D 2^-30.  No N here exceeds 10^6 (the
cases use 4 x 10^5): a tested cell with N p (1-p) >= 100 has a standard
deviation of at least 10 / N = 1e-5 in p, four orders above the shift of a
patch-year (two draws), two above that of the 12 000 draws of a 1024-patch
replicate over six years;
where p is so small that the count is 0 or a few, a relative shift of 1e-7
does not move the p-value either.  It is ignored.  (One consequence is kept in
mind when choosing cases: with e = 0 a patch still dies once in 2^31 draws, so
no case rests a probability of exactly 1 on e = 0.)
"""
from __future__ import annotations

import functools
import math

import numpy as np

MUTANTS = ("pre", "src0", "noclamp", "sameword", "noborder")


# ---------------------------------------------------------------------------
# the model's tables
# ---------------------------------------------------------------------------
def matrix(n, m, d, dS, src0=False):
    """The reference's M with the source row (:265-277), libm exp.  src0: the
    mutant source row exp(-a k dS) instead of exp(-a (k+1) dS)."""
    a = 1.0 / m
    M = np.zeros((n + 1, n))
    for i in range(n):
        for j in range(i + 1, n):
            M[i, j] = M[j, i] = math.exp(-a * (j - i) * d)
    for j in range(n):
        M[n, j] = math.exp(-a * (j + (0 if src0 else 1)) * dS)
    return M


def cells(post, border=True):
    """[(e, c, probability)] of the posterior cells with mass, as the scan of
    :361-375 draws them: cell i owns [pcum[i-1], pcum[i]) of [0, pscale).
    Raises unless the mass fills pscale (module docstring).  border=False is
    the mutant without the border weights: its cumulative sum passes pscale,
    and the scan never reaches the cells beyond."""
    post = np.asarray(post, dtype=np.float64)
    s = post.shape[0]
    assert post.shape == (s, s) and s >= 2 and np.all(post >= 0)
    pscale = float((s - 1) * (s - 1))
    out, acc = [], 0.0
    for ie in range(s):
        for ic in range(s):
            w = 1.0
            if border:
                w *= 0.5 if ie in (0, s - 1) else 1.0
                w *= 0.5 if ic in (0, s - 1) else 1.0
            lo = acc
            acc += w * float(post[ie, ic])
            p = (min(acc, pscale) - min(lo, pscale)) / pscale
            if p > 0:
                out.append((0.01 * ie, 0.01 * ic, p))
    if abs(min(acc, pscale) / pscale - 1.0) > 1e-12:
        raise ValueError(f"posterior mass {acc} does not fill pscale {pscale}: replicates would not be independent")
    return out


def start(row):
    """q_k: 1, 0 or 1/2 for an occupied, empty or missing patch."""
    row = np.asarray(row)
    return np.where(row == 1, 1.0, np.where(row == -1, 0.5, 0.0))


# ---------------------------------------------------------------------------
# (a) the 2^n-state chain
# ---------------------------------------------------------------------------
def _product(a1):
    """P[i, z'] = prod_k (a1[i, k] if bit k of z' else 1 - a1[i, k])."""
    P = np.ones((a1.shape[0], 1))
    for k in range(a1.shape[1]):
        P = np.concatenate([P * (1.0 - a1[:, k:k + 1]), P * a1[:, k:k + 1]], axis=1)
    return P


def _extinction(v, n, E):
    """Every occupied patch dies with probability E, independently."""
    v = v.copy()
    for k in range(n):
        u = v.reshape(-1, 2, 1 << k)
        u[:, 0, :] += E * u[:, 1, :]
        u[:, 1, :] *= 1.0 - E
    return v


def chain(row, post, tfut, m=400.0, d=200.0, KD=1.0, KS=0.0, dS=200.0, mutant=None):
    """(pext[tfut], hist[tfut, n+1], occ[tfut, n]): after year t + 1 the
    probability that every patch is empty, that exactly j patches are
    occupied, and that patch k is occupied, averaged over the posterior.

    mutant (test_future_exact.py, sensitivity): None, or the model with one
    error: "pre" pressure from the occupancy before extinction, "src0" the
    source row exp(-a k dS), "noclamp" E not clamped at 1 (the result is then
    no probability), "sameword" one draw for a patch's extinction and
    colonisation (a patch that just died is recolonised with probability
    min(pC, E) / E; n <= 8), "noborder" no border weights in the posterior."""
    assert mutant is None or mutant in MUTANTS
    row = np.asarray(row)
    n = row.size
    assert 1 <= n <= (8 if mutant == "sameword" else 10) and KD > 0
    S = 1 << n
    M = matrix(n, m, d, dS, src0=mutant == "src0")
    bits = ((np.arange(S)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.float64)
    s1 = bits @ (M[:n] * KD) + M[n] * KS            # s1[z, k]; M[k][k] = 0 leaves l = k out
    npop = bits.sum(axis=1).astype(np.int64)
    q = start(row)
    v0 = np.prod(np.where(bits == 1, q, 1.0 - q), axis=1)
    if mutant == "sameword":
        X = np.repeat(np.arange(S), S)
        Z = np.tile(np.arange(S), S)
        keep = (Z & ~X) == 0
        X, Z = X[keep], Z[keep]                      # the 3^n pairs (before, survivors)

    @functools.lru_cache(maxsize=None)
    def colonisation(c):                             # P[z, z'] from the survivor set z
        return _product(np.where(bits == 1, 1.0, np.minimum(1.0, c * s1)))

    pext, hist, occ = np.zeros(tfut), np.zeros((tfut, n + 1)), np.zeros((tfut, n))
    for e, c, w in cells(post, border=mutant != "noborder"):
        E = e / KD
        if mutant != "noclamp":
            E = min(1.0, E)
        pc = np.minimum(1.0, c * s1)
        if mutant == "pre":
            year = _product(bits * (1.0 - E) + (1.0 - bits * (1.0 - E)) * pc)
        elif mutant == "sameword":
            dead = bits[X] - bits[Z]
            again = np.minimum(pc[Z], E) / E if E > 0 else pc[Z]
            pair = _product(np.where(bits[Z] == 1, 1.0, np.where(dead == 1, again, pc[Z])))
            wpair = np.prod(np.where(bits[Z] == 1, 1.0 - E, np.where(dead == 1, E, 1.0)), axis=1)
        v = v0
        for t in range(tfut):
            if mutant == "pre":
                v = v @ year
            elif mutant == "sameword":
                v = (v[X] * wpair) @ pair
            else:
                v = _extinction(v, n, E) @ colonisation(c)
            pext[t] += w * v[0]
            hist[t] += w * np.bincount(npop, weights=v, minlength=n + 1)
            occ[t] += w * (v @ bits)
    return pext, hist, occ


# ---------------------------------------------------------------------------
# (b) the first year, any n
# ---------------------------------------------------------------------------
def year1(row, post, m=400.0, d=200.0, KD=1.0, KS=0.0, dS=200.0):
    """occ[n]: P(patch k occupied after year 1) = sigma_k + (1 - sigma_k) c sbar_k,
    sigma_k = q_k (1 - E), sbar_k = sum_{l != k} sigma_l M[l][k] K_D + M[n][k] K_S,
    averaged over the cells.  The expectation passes through pC only where the
    clamp cannot bind: raises otherwise."""
    row = np.asarray(row)
    n = row.size
    assert KD > 0
    M = matrix(n, m, d, dS)
    q = start(row)
    full = M[:n].sum(axis=0) * KD + M[n] * KS
    out = np.zeros(n)
    for e, c, w in cells(post):
        if c * full.max() > 1.0:
            raise ValueError(f"the clamp can bind: c = {c}, largest sum {full.max()}")
        sigma = q * (1.0 - min(1.0, e / KD))
        sbar = sigma @ M[:n] * KD + M[n] * KS
        out += w * (sigma + (1.0 - sigma) * c * sbar)
    return out


# ---------------------------------------------------------------------------
# (c) isolated patches, any n, every year
# ---------------------------------------------------------------------------
def poisson_binomial(p):
    """Distribution of the number of successes of independent trials p[k]."""
    dist = np.zeros(p.size + 1)
    dist[0] = 1.0
    for k, pk in enumerate(p):
        dist[1:k + 2] = dist[1:k + 2] * (1.0 - pk) + dist[:k + 1] * pk
        dist[0] *= 1.0 - pk
    return dist


def isolated(row, post, tfut, m=400.0, d=200.0, KD=1.0, KS=0.0, dS=200.0):
    """(pext, hist, occ) as chain(), for d/m >= 100: the coupling between
    patches is at most n K_D e^-100 c and is dropped; patch k survives with
    1 - E and is colonised with g_k = min(1, c K_S M[n][k])."""
    row = np.asarray(row)
    n = row.size
    assert KD > 0 and d / m >= 100.0
    M = matrix(n, m, d, dS)
    pext, hist, occ = np.zeros(tfut), np.zeros((tfut, n + 1)), np.zeros((tfut, n))
    for e, c, w in cells(post):
        assert KD * n * math.exp(-100.0) * c < 1e-30
        E = min(1.0, e / KD)
        g = np.minimum(1.0, c * KS * M[n])
        p = start(row)
        for t in range(tfut):
            p = p * (1.0 - E)
            p = p + (1.0 - p) * g
            occ[t] += w * p
            pext[t] += w * np.prod(1.0 - p)
            hist[t] += w * poisson_binomial(p)
    return pext, hist, occ


# ---------------------------------------------------------------------------
# the test: exact two-sided binomial p-values, Bonferroni over a call's cells
# ---------------------------------------------------------------------------
def _log_pmf(k, N, p):
    return (math.lgamma(N + 1) - math.lgamma(k + 1) - math.lgamma(N - k + 1)
            + k * math.log(p) + (N - k) * math.log1p(-p))


def binom_p(count, N, p):
    """2 min(P(X <= count), P(X >= count)), capped at 1, X ~ binomial(N, p):
    the pmf at `count` and from there the recurrence
    pmf(j-1) / pmf(j) = j (1-p) / ((N-j+1) p) in log space, summed over the
    tail on count's side of the mean until its terms fall below e^-45 of the
    first (they decrease at least as fast as a Gaussian's: 10 standard
    deviations and 50 terms); the other tail is 1 - that + pmf(count).  No
    normal approximation."""
    count, N, p = int(count), int(N), float(p)
    assert 0 <= count <= N and 0.0 <= p <= 1.0
    if p == 0.0:
        return 1.0 if count == 0 else 0.0
    if p == 1.0:
        return 1.0 if count == N else 0.0
    lp0 = _log_pmf(count, N, p)
    width = int(10.0 * math.sqrt(N * p * (1.0 - p))) + 50
    lr = math.log1p(-p) - math.log(p)
    if count <= N * p:                                 # the lower tail, downwards
        j = np.arange(count, max(count - width, 0), -1, dtype=np.float64)
        steps = np.log(j) - np.log(N - j + 1.0) + lr
    else:                                              # the upper tail, upwards
        j = np.arange(count, min(count + width, N), dtype=np.float64)
        steps = np.log(N - j) - np.log(j + 1.0) - lr
    terms = np.concatenate([[0.0], np.cumsum(steps)])
    log_tail = lp0 + math.log(float(np.exp(terms).sum()))
    tail = math.exp(log_tail) if log_tail > -740.0 else 0.0
    other = 1.0 - tail + math.exp(lp0) if lp0 > -740.0 else 1.0
    return min(1.0, 2.0 * min(tail, other))


def pvalues(counts, N, probs):
    """binom_p cell by cell; a `probability` outside [0, 1] (a mutant's) has
    p-value 0."""
    counts = np.asarray(counts).ravel()
    probs = np.asarray(probs, dtype=np.float64).ravel()
    assert counts.shape == probs.shape
    return np.array([binom_p(k, N, p) if 0.0 <= p <= 1.0 else 0.0 for k, p in zip(counts, probs)])


def check(counts, N, probs, alpha=1e-5, label=""):
    """Every cell's exact binomial p-value is at least alpha / cells
    (Bonferroni, once per call); a cell of probability exactly 0 counts 0 and
    one of exactly 1 counts N (their p-value is 0 otherwise).  No cell is left
    out.  Prints the smallest p-value and the largest |z| (over the cells with
    N p (1-p) >= 100, where z means something); returns both."""
    counts = np.asarray(counts).ravel().astype(np.int64)
    probs = np.asarray(probs, dtype=np.float64).ravel()
    pv = pvalues(counts, N, probs)
    var = N * probs * (1.0 - probs)
    z = np.where(var >= 100.0, np.abs(counts - N * probs) / np.sqrt(np.maximum(var, 100.0)), 0.0)
    worst = int(np.argmin(pv))
    print(f"{label}: {pv.size} cells, N {N}, smallest p-value {pv[worst]:.3g} (cell {worst}: count {counts[worst]}, "
          f"p {probs[worst]:.6g}), largest |z| {z.max():.2f} over the {int((var >= 100.0).sum())} cells with "
          f"N p (1-p) >= 100")
    bad = np.flatnonzero(pv < alpha / pv.size)
    assert bad.size == 0, (label, [(int(i), int(counts[i]), float(probs[i]), float(pv[i])) for i in bad[:8]])
    return float(pv[worst]), float(z.max())


def rejects(counts, N, probs, alpha=1e-5):
    """The smallest p-value if check() would fail on it, else None."""
    pv = pvalues(counts, N, probs)
    return float(pv.min()) if pv.min() < alpha / pv.size else None


def informative(N, probs, floor=100.0):
    """Cells whose count has a variance of at least `floor`."""
    probs = np.asarray(probs, dtype=np.float64)
    return N * probs * (1.0 - probs) >= floor


# ---------------------------------------------------------------------------
# the cases, shared by test_future_exact.py (CPU: the oracle against them,
# non-vacuity, sensitivity) and test_gpu_future_exact.py
# ---------------------------------------------------------------------------
TWO32 = 1 << 32


def make_row(n, nmiss, frac, seed):
    """n patches, about `frac` of them occupied, nmiss missing, reproducibly."""
    rng = np.random.default_rng(seed)
    row = (rng.random(n) < frac).astype(np.int32)
    if nmiss:
        row[rng.choice(n, size=min(nmiss, n), replace=False)] = -1
    return row


def posterior(s, mass):
    """An s x s posterior with probability mass[(ie, ic)] (relative) in its
    cells, the border weights undone, scaled to pscale."""
    post = np.zeros((s, s))
    total = float(sum(mass.values()))
    for (ie, ic), v in mass.items():
        w = (0.5 if ie in (0, s - 1) else 1.0) * (0.5 if ic in (0, s - 1) else 1.0)
        post[ie, ic] = v / total * (s - 1) * (s - 1) / w
    return post


def _chain_cases():
    grid = lambda ies, ics: {(ie, ic): 1.0 for ie in ies for ic in ics}
    return {
        # one missing patch under a source; the replicate indices pass 2^32
        "n1": dict(row=np.array([-1], dtype=np.int32), post=posterior(21, grid((5, 10), (5, 10, 15))),
                   kw=dict(m=400.0, d=100.0, KD=0.5, KS=2.0, dS=100.0), tfut=12, N=400000, seed=11,
                   rep0=TWO32 - 150000, options=""),
        # no source: all empty is absorbing
        "n2": dict(row=np.array([1, -1], dtype=np.int32), post=posterior(21, grid((10, 15), (10, 20))),
                   kw=dict(m=400.0, d=100.0, KD=1.0, KS=0.0, dS=200.0), tfut=12, N=400000, seed=12, rep0=0,
                   options=""),
        # a source that matters (its row is visible), E around 1/2, windows of 3 years
        "n8": dict(row=make_row(8, 2, 0.6, seed=8), post=posterior(21, grid((10, 15, 20), (5, 12, 20))),
                   kw=dict(m=400.0, d=100.0, KD=0.3, KS=1.0, dS=200.0), tfut=12, N=400000, seed=13, rep0=5,
                   options=";MDP_FUT_SUM_YEARS=3"),
        # mass on the border rows and columns (e = 0, c = 0, c = 0.2) and cells with e/K_D > 1 (ie = 15, 20)
        "n9": dict(row=make_row(9, 3, 0.6, seed=9),
                   post=posterior(21, {(0, 6): 1.0, (5, 0): 2.0, (5, 20): 2.0, (8, 10): 2.0, (15, 8): 1.5,
                                       (20, 12): 1.5, (20, 20): 1.0, (3, 4): 1.0}),
                   kw=dict(m=400.0, d=100.0, KD=0.1, KS=0.5, dS=100.0), tfut=10, N=400000, seed=14, rep0=77,
                   options=""),
        # c up to 0.4 at d = 50: c s1 > 1 where most patches survive (the clamp binds); no source
        "n10": dict(row=make_row(10, 2, 0.8, seed=10),
                    post=posterior(41, {(20, 40): 1.0, (40, 40): 1.0, (40, 20): 1.0, (30, 30): 1.0}),
                    kw=dict(m=400.0, d=50.0, KD=0.5, KS=0.0, dS=200.0), tfut=10, N=400000, seed=15, rep0=3,
                    options=""),
    }


CHAIN_CASES = _chain_cases()

LANE_SIZES = (17, 32, 33, 64)
WIDE_SIZES = (65, 128, 129, 256, 257, 512, 513, 1024)


def year1_case(n):
    """The real coupling (d/m = 1/4: the full column sum of M is about 7), a
    source row that spans (e^-2, 1) over the row, up to 12 missing patches.
    c (K_D 7.1 + K_S) <= 0.18 * 5.6: the clamp cannot bind."""
    mass = {(2, 6): 1.0, (3, 12): 2.0, (5, 18): 1.0, (4, 9): 1.0}
    return dict(row=make_row(n, min(12, n // 5), 0.3, seed=100 + n), post=posterior(21, mass),
                kw=dict(m=400.0, d=100.0, KD=0.5, KS=2.0, dS=800.0 / n), N=400000, seed=200 + n, rep0=n)


def isolated_case(n, absorbing=False):
    """d/m = 1000: M between patches underflows to exactly 0.  K_S = 4 with a
    source row spanning (e^-2, 1); or, absorbing, K_S = 0 with no empty patch
    in the row and cells at E = 1/4, 1/2, 1 and 5/4, so that whole replicates
    die from the first year on and the rest keep every patch informative."""
    if absorbing:
        mass = {(1, 3): 3.0, (2, 5): 3.0, (4, 2): 1.0, (5, 7): 1.0}
        row = make_row(n, 12, 1.0, seed=300 + n)
        kw = dict(m=1.0, d=1000.0, KD=0.04, KS=0.0, dS=2.0 / n)
    else:
        mass = {(2, 5): 1.0, (5, 10): 2.0, (10, 20): 1.0, (7, 3): 1.0}
        row = make_row(n, min(12, n // 5), 0.4, seed=300 + n)
        kw = dict(m=1.0, d=1000.0, KD=0.2, KS=4.0, dS=2.0 / n)
    return dict(row=row, post=posterior(21, mass), kw=kw, tfut=6, N=400000, seed=400 + n, rep0=2 * n)
