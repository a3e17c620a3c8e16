"""The future engine beyond 64 patches, the parts that need no GPU.

The CPU oracle (oracle/spom_future_oracle.c) holds `int pitmp[64]` and stops
at 64 patches.  The checker of the patch-parallel kernel beyond that is
`checker()` below: a numpy restatement of the reference loop
(main_MIDASPOM_future.c:64-110, :343-386) over the literal (n+1) x n matrix M
-- no Toeplitz table, a linear scan of the cumulative posterior with the
reference's carry-over, the colonisation sums by an explicit ascending loop
over the surviving patches (a numpy reduction sums pairwise: other bits).
It returns the per-year counts and every replicate's final state.  Here it is
pinned to the oracle, count for count, on five problems up to 64 patches; the
GPU tests (test_gpu_future_wide.py) import it.

Also here: the refusals of mdp_future_create_opts, which come before any
device call, and the host planner's stand-alone check program
(_build/future_plan_check) against a Python restatement of the layout.
"""
from __future__ import annotations

import functools
import math
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle

ROOT = Path(__file__).resolve().parents[1]
PLAN_CHECK = ROOT / "midaspom_amd" / "_build" / "future_plan_check"
RAND_MAX = 2147483647.0
U32 = np.uint64(0xffffffff)


# ---------------------------------------------------------------------------
# Philox4x32-10, vectorised in uint64 over the counter's last word
# ---------------------------------------------------------------------------
def philox_pairs(seed, rep, t, pairs):
    """words[4, len(pairs)] of philox(seed, {rep_lo, rep_hi, t, pair})."""
    pairs = np.asarray(pairs, dtype=np.uint64)
    k0, k1 = np.uint64(seed & 0xffffffff), np.uint64((seed >> 32) & 0xffffffff)
    c0 = np.full(pairs.shape, rep & 0xffffffff, dtype=np.uint64)
    c1 = np.full(pairs.shape, (rep >> 32) & 0xffffffff, dtype=np.uint64)
    c2 = np.full(pairs.shape, t & 0xffffffff, dtype=np.uint64)
    c3 = pairs & U32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & U32
        k0 = (k0 + np.uint64(0x9E3779B9)) & U32
        k1 = (k1 + np.uint64(0xBB67AE85)) & U32
    return np.stack([c0, c1, c2, c3])


def matrix(n, m, d, dS):
    """The reference's M with the source row (:265-277), libm exp."""
    a = 1.0 / m
    M = np.zeros((n + 1, n))
    for i in range(n):
        for j in range(i + 1, n):
            M[i, j] = M[j, i] = math.exp(-a * (j - i) * d)
    for j in range(n):
        M[n, j] = math.exp(-a * (j + 1) * dS)
    return M


def checker(row, post, nrep, tfut, seed=0, rep0=0, m=400.0, d=200.0, KD=1.0, KS=0.0, dS=200.0):
    """(counts[tfut], states[nrep, n]) of replicates [rep0, rep0 + nrep)."""
    row = np.asarray(row, dtype=np.int64)
    n = row.size
    post = np.asarray(post, dtype=np.float64)
    s = post.shape[0] if post.size else 0
    M = matrix(n, m, d, dS)
    # trapezoid-weighted cumulative posterior in scan order (:362-369)
    pcum = []
    acc = 0.0
    for ie in range(s):
        for ic in range(s):
            w = 1.0
            if ie in (0, s - 1):
                w *= 0.5
            if ic in (0, s - 1):
                w *= 0.5
            acc += w * float(post[ie, ic])
            pcum.append(acc)
    pscale = float((s - 1) * (s - 1))

    def scan(rep):
        r = int(philox_pairs(seed, rep, 0xffffffff, [0])[0, 0]) >> 1
        pec = pscale * float(r) / RAND_MAX
        for i, v in enumerate(pcum):
            if pec < v:
                return (i // s) * 0.01, (i % s) * 0.01
        return None

    missing = np.flatnonzero(row == -1)
    nmiss = missing.size
    pairs = np.arange((n + 1) // 2)
    k = np.arange(n)
    counts = np.zeros(tfut, dtype=np.uint64)
    states = np.zeros((nrep, n), dtype=bool)
    ec = (0.0, 0.0)
    q = rep0
    while q > 0:  # carry-in: the (e, c) the sequential loop holds at rep0
        q -= 1
        found = scan(q)
        if found:
            ec = found
            break
    for i in range(nrep):
        rep = rep0 + i
        found = scan(rep)
        if found:
            ec = found
        e, c = ec
        init = (int(philox_pairs(seed, rep, 0xffffffff, [0])[1, 0]) >> 1) % (1 << nmiss)
        occ = row == 1
        for qi, col in enumerate(missing):  # the first missing patch is the most significant bit
            occ[col] = (init >> (nmiss - 1 - qi)) & 1
        with np.errstate(divide="ignore", invalid="ignore"):
            E = np.float64(e) / np.float64(KD)  # as C divides: e/0 is inf, 0/0 is NaN (no patch survives)
        if E > 1:
            E = 1.0
        for t in range(tfut):
            w = philox_pairs(seed, rep, t, pairs)
            ext = (w[2 * (k & 1), k >> 1] >> np.uint64(1)).astype(np.float64) / RAND_MAX
            col = (w[2 * (k & 1) + 1, k >> 1] >> np.uint64(1)).astype(np.float64) / RAND_MAX
            surv = occ & (ext > E)
            s1 = np.zeros(n)
            for l in np.flatnonzero(surv):  # ascending l, one add per survivor: the reference's order
                s1 += M[l] * KD
            s1 += M[n] * KS
            pc = np.minimum(c * s1, 1.0)
            occ = surv | (~surv & (col < pc))
            if not occ.any():
                counts[t] += np.uint64(1)
        states[i] = occ
    return counts, states


def make_row(n, nmiss, frac, seed):
    """n patches, `frac` of them occupied, nmiss missing, reproducibly."""
    rng = np.random.default_rng(seed)
    row = (rng.random(n) < frac).astype(np.int32)
    if nmiss:
        row[rng.choice(n, size=min(nmiss, n), replace=False)] = -1
    return row


@functools.lru_cache(maxsize=None)
def posterior21():
    """A smooth 21-step posterior with its mass at small e and moderate c,
    scaled to the (necstep-1)^2 the sampler expects."""
    g = np.arange(21) * 0.01
    post = np.exp(-((g[:, None] - 0.04) / 0.03) ** 2 - ((g[None, :] - 0.12) / 0.05) ** 2)
    w = np.ones(21)
    w[0] = w[-1] = 0.5
    return post * (400.0 / float((np.outer(w, w) * post).sum()))


# ---------------------------------------------------------------------------
# 1. the checker against the reference-pinned oracle
# ---------------------------------------------------------------------------
def test_philox_matches_the_oracle():
    for seed, rep, t in [(0, 0, 0), ((1 << 35) + 8, (1 << 32) + 5, 7), (12345, 1234, 0xffffffff)]:
        got = philox_pairs(seed, rep, t, np.arange(6))
        for p in range(6):
            assert [int(x) for x in got[:, p]] == oracle.philox(seed, [rep & 0xffffffff, rep >> 32, t, p])


@pytest.mark.parametrize("n,KD,KS", [(1, 1.0, 0.0), (9, 0.3, 2.0), (17, 0.0, 1.0), (33, 1.0, 0.2), (64, 4.0, 0.7)])
def test_checker_equals_the_oracle(n, KD, KS):
    """300 replicates x 9 years from replicate 1234 (a carry-in look-back),
    missing data, at half the posterior mass so that draws carry over."""
    row = make_row(n, min(3, n), 0.5, seed=n)
    post = posterior21() * 0.5
    kw = dict(m=400.0, d=100.0, KD=KD, KS=KS, dS=150.0)
    ref = oracle.future_counts(row, post, tfut=9, nrep=300, seed=77, rep0=1234, **kw)
    got, states = checker(row, post, 300, 9, seed=77, rep0=1234, **kw)
    assert np.array_equal(got, ref), (got, ref)
    assert int((~states.any(axis=1)).sum()) == int(ref[-1])


# ---------------------------------------------------------------------------
# 2. refusals, all before the first device call
# ---------------------------------------------------------------------------
def _refused(row, options, match, post=None):
    with pytest.raises(mdp.MidaspomError, match=match):
        mdp.Future(np.asarray(row, dtype=np.int32), posterior21() if post is None else post, options=options)


@pytest.mark.parametrize("options", ["MDP_FUT_WIDE=auto", "MDP_FUT_WIDE=1", {"MDP_FUT_WIDE": "auto"}])
def test_1025_patches_are_refused(options):
    _refused(np.ones(1025), options, "UNSUPPORTED")


@pytest.mark.parametrize("options", ["MDP_FUT_WIDE=0", ""])
def test_65_patches_need_the_option(options):
    _refused(np.ones(65), options, "UNSUPPORTED")


@pytest.mark.parametrize("options", ["MDP_FUT_NARROW=1", "MDP_FUT_WIDE=2", "MDP_FUT_WIDE=", "MDP_WIDE=1"])
def test_unknown_option_or_value(options):
    _refused(np.ones(8), options, "EINVAL")
    _refused(np.ones(100), options, "EINVAL")


def test_survey_value_2_under_auto():
    row = np.ones(100, dtype=np.int32)
    row[70] = 2
    _refused(row, "MDP_FUT_WIDE=auto", "EINVAL")
    _refused(np.full(100, -1), "MDP_FUT_WIDE=auto", "UNSUPPORTED")  # 100 missing patches


def test_new_symbols_without_an_abi_bump():
    lib = mdp._lib.lib()
    assert lib.mdp_abi_version() == 9
    for name in ("mdp_future_create_opts", "mdp_future_kernel", "mdp_future_states"):
        assert hasattr(lib, name)


# ---------------------------------------------------------------------------
# 3. the host planner's check program against the layout restated here
# ---------------------------------------------------------------------------
def _fnv(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h


def layout(row, m, d, KD, KS, dS):
    """What future_plan_check prints for k_future_wide, from the definitions:
    lane lam owns pairs lam + 64 j, patch 2*pair + p in bit 2 j + p."""
    n = len(row)
    NP = 1 if n <= 128 else 2 if n <= 256 else 4 if n <= 512 else 8
    length = (n + 128 * NP + 1) & ~1
    occ0 = [0] * 64
    miss = []
    for k, v in enumerate(row):
        pair = k >> 1
        lane, bit = pair & 63, 2 * (pair >> 6) + (k & 1)
        if v == 1:
            occ0[lane] |= 1 << bit
        elif v == -1:
            miss.append((lane << 8) | bit)
    a = 1.0 / m
    G = [0.0] * (length + 1)
    for i in range(2 * n - 1):
        if i != n - 1:
            G[i] = math.exp(-a * abs(i - (n - 1)) * d) * KD
    image = G[:length] + G[1:length + 1]
    src = [math.exp(-a * (j + 1) * dS) * KS if j < n else 0.0 for j in range(128 * NP)]
    words = [0] * ((n + 63) // 64)
    for k, v in enumerate(row):
        if v != 0:
            words[k >> 6] |= 1 << (k & 63)
    return "\n".join([
        f"kernel k_future_wide<{NP}>",
        f"n {n} len {length} nmiss {len(miss)}",
        "occ0" + "".join(f" {v:x}" for v in occ0),
        "miss" + "".join(f" {v:x}" for v in miss),
        f"image {_fnv(struct.pack(f'<{len(image)}d', *image)):016x} src {_fnv(struct.pack(f'<{len(src)}d', *src)):016x}",
        "states" + "".join(f" {w:x}" for w in words),
        "check ok",
    ]) + "\n"


def _plan_check(exe, row, options, m=400.0, d=100.0, KD=0.7, KS=0.3, dS=150.0):
    text = "".join("m" if v == -1 else str(int(v)) for v in row)
    return subprocess.run([str(exe), text, str(m), str(d), str(KD), str(KS), str(dS), options], capture_output=True,
                          text=True, timeout=120)


@pytest.mark.parametrize("n", [1, 64, 65, 128, 129, 1024])
def test_plan_check_program(n):
    assert PLAN_CHECK.exists(), "future_plan_check is built by `make -C midaspom_amd/csrc`"
    row = make_row(n, min(5, n), 0.4, seed=1000 + n)
    r = _plan_check(PLAN_CHECK, row, "MDP_FUT_WIDE=1")
    assert r.returncode == 0, r.stderr
    assert r.stdout == layout(list(row), 400.0, 100.0, 0.7, 0.3, 150.0)
    r = _plan_check(PLAN_CHECK, row, "MDP_FUT_WIDE=auto")
    assert r.returncode == 0, r.stderr
    want = "k_future<" if n <= 64 else "k_future_wide<"
    assert r.stdout.splitlines()[0].startswith("kernel " + want)
    r = _plan_check(PLAN_CHECK, row, "")
    assert (r.returncode == 0) == (n <= 64), r.stderr


def lane_plan(row, m, d, KD, KS, dS):
    """What future_plan_check prints for a lane kernel, from the definitions:
    bit k of a mask is patch k, the missing bits in patch order, M*K_D padded
    with zeros to NM x NM and the source row M[n]*K_S to NM."""
    n = len(row)
    NM = 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64
    M = matrix(n, m, d, dS)
    MK = np.zeros((NM, NM))
    MK[:n, :n] = M[:n] * KD
    src = np.zeros(NM)
    src[:n] = M[n] * KS
    occ0 = sum(1 << k for k, v in enumerate(row) if v == 1)
    miss = np.array([1 << k for k, v in enumerate(row) if v == -1], dtype="<u8")
    return (f"kernel k_future<{NM}>\n"
            f"lane nmiss {miss.size} occ0 {occ0:x} miss {_fnv(miss.tobytes()):016x} "
            f"MK {_fnv(MK.astype('<f8').tobytes()):016x} src {_fnv(src.astype('<f8').tobytes()):016x}\n")


@pytest.mark.parametrize("n", [1, 7, 9, 17, 33, 64])
def test_plan_check_program_lane(n):
    """The lane kernels' plan (occupied mask, missing bits, M*K_D, source row)
    with two missing patches (one at n = 1), on every padded size."""
    assert PLAN_CHECK.exists(), "future_plan_check is built by `make -C midaspom_amd/csrc`"
    row = make_row(n, min(2, n), 0.4, seed=2000 + n)
    assert int((row == -1).sum()) == min(2, n)
    for options in ("", "MDP_FUT_WIDE=auto"):
        r = _plan_check(PLAN_CHECK, row, options)
        assert r.returncode == 0, r.stderr
        assert r.stdout == lane_plan(list(row), 400.0, 100.0, 0.7, 0.3, 150.0)


def test_plan_check_program_lane_refusals():
    """A lane row is refused as mdp_future_create refuses it."""
    r = _plan_check(PLAN_CHECK, [1, 0, 2, 1], "")
    assert r.returncode == 1 and "survey value 2 in column 2" in r.stderr
    r = _plan_check(PLAN_CHECK, [-1] * 31 + [1], "")
    assert r.returncode == 1 and "31 missing patches" in r.stderr
    assert _plan_check(PLAN_CHECK, [-1] * 30 + [1], "").returncode == 0
