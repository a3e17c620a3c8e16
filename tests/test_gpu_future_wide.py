"""The future engine's patch-parallel kernel k_future_wide<NP> on the GPU
(mdp_future_create_opts, MDP_FUT_WIDE): against the reference-pinned oracle
up to 64 patches (MDP_FUT_WIDE=1), against the numpy checker of
test_future_wide_host.py beyond (counts and every replicate's state, bit for
bit), the embedding of a 64-patch problem in a 200-patch row, the plumbing
(splits, device form, grid stride, look-back flag), both drop-ins and the
posterior -> forecast chain on a 256-patch survey.
"""
from __future__ import annotations

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle
from midaspom_amd import _lib, synth
from test_future_wide_host import checker, make_row, posterior21

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, D = 400.0, 100.0
TWO32 = 1 << 32
AUTO = "MDP_FUT_WIDE=auto"
WIDE = "MDP_FUT_WIDE=1"


def np_of(n):
    return 1 if n <= 128 else 2 if n <= 256 else 4 if n <= 512 else 8


# ---------------------------------------------------------------------------
# 1. MDP_FUT_WIDE=1 against the pinned oracle, n <= 64
# ---------------------------------------------------------------------------
NMISS = {1: 1, 2: 2, 9: 5, 33: 12, 64: 12}


def harsh21():
    """21 steps, the mass at e near 0.2 and c near 0.02: replicates of up to
    64 patches go extinct within ten years, and some are recolonised."""
    g = np.arange(21) * 0.01
    post = np.exp(-((g[:, None] - 0.2) / 0.03) ** 2 - ((g[None, :] - 0.02) / 0.02) ** 2)
    w = np.ones(21)
    w[0] = w[-1] = 0.5
    return post * (400.0 / float((np.outer(w, w) * post).sum()))


@pytest.mark.parametrize("KD,KS,dS", [(1.0, 0.0, 200.0), (0.3, 2.0, 50.0), (0.0, 1.0, 200.0)])
@pytest.mark.parametrize("n", [1, 2, 9, 33, 64])
def test_wide_kernel_equals_the_oracle(n, KD, KS, dS):
    """Missing data, the half-mass posterior (about half the draws carry the
    previous replicate's (e, c) over) and replicate indices across 2^32."""
    row = make_row(n, NMISS[n], 0.5 if n < 9 else 0.15, seed=40 + n)
    post = harsh21() * 0.5
    kw = dict(m=M, d=D, KD=KD, KS=KS, dS=dS)
    nrep, tfut, seed, rep0 = 3000, 10, (1 << 35) + 8, TWO32 - 1500
    ref = oracle.future_counts(row, post, tfut=tfut, nrep=nrep, seed=seed, rep0=rep0, **kw)
    with mdp.Future(row, post, options=WIDE, **kw) as f:
        assert f.kernel == "k_future_wide<1>"
        got = f.simulate(nrep, tfut, seed=seed, rep0=rep0)
    with mdp.Future(row, post, options=AUTO, **kw) as f:
        assert f.kernel.startswith("k_future<")
        lane = f.simulate(nrep, tfut, seed=seed, rep0=rep0)
    print(n, KD, KS, "counts", got, "oracle", ref)
    assert ref.max() > 0 and ref.min() < nrep  # the equality is not vacuous
    assert np.array_equal(got, ref)
    assert np.array_equal(lane, ref)


@pytest.mark.parametrize("n", [1, 2, 9, 33, 64])
def test_wide_kernel_nan_and_zero_posteriors(n):
    row = make_row(n, NMISS[n], 0.5, seed=40 + n)
    nan = posterior21().copy()
    nan[7, 3] = np.nan  # the scan matches nothing from this cell on
    for post in (nan, np.zeros((21, 21))):
        ref = oracle.future_counts(row, post, tfut=8, nrep=2000, seed=9, rep0=100, m=M, d=D, KD=0.5, KS=0.1)
        with mdp.Future(row, post, m=M, d=D, KD=0.5, KS=0.1, options=WIDE) as f:
            got = f.simulate(2000, 8, seed=9, rep0=100)
        assert np.array_equal(got, ref), (got, ref)


# ---------------------------------------------------------------------------
# 2. auto beyond 64 patches against the numpy checker: counts and states
# ---------------------------------------------------------------------------
def moderate_posterior():
    """s = 11, the mass at small e and moderate c: most patches stay occupied."""
    post = np.zeros((11, 11))
    post[1:3, 3:9] = 1.0
    post[2, 5] = 3.0
    w = np.ones(11)
    w[0] = w[-1] = 0.5
    return post * (100.0 / float((np.outer(w, w) * post).sum()))


def harsh_posterior():
    """s = 11, rows 0-2 and columns 6-10 zero (e >= 0.03, c <= 0.05), scaled
    to 0.8 (s-1)^2: a fifth of the draws carry over."""
    post = np.ones((11, 11))
    post[0:3, :] = 0.0
    post[:, 6:] = 0.0
    w = np.ones(11)
    w[0] = w[-1] = 0.5
    return post * (80.0 / float((np.outer(w, w) * post).sum()))


# regime (a): K_D = 1, many patches occupied, mid-range colonisation sums.
# regime (b): near extinction; K_D (and K_S) per size chosen with the checker
# on the CPU so that the final count lies strictly inside (0, nrep).
#            n: (nrep, tfut, K_D of (b), K_S of (b))
SIZES = {
    65: (60, 8, 0.08, 0.0),
    127: (60, 8, 0.06, 0.0),
    128: (60, 8, 0.06, 0.3),
    129: (60, 8, 0.06, 0.3),
    255: (40, 6, 0.05, 0.0),
    256: (40, 6, 0.05, 0.0),
    257: (40, 6, 0.05, 0.0),
    513: (30, 5, 0.045, 0.0),
    1024: (24, 5, 0.08, 0.0),  # 22/24 by the checker (K_D = 0.04 to 0.06: 24/24)
}


def wide_case(n, regime):
    nrep, tfut, KD, KS = SIZES[n]
    if regime == "a":
        return dict(row=make_row(n, 6, 0.5, seed=n), post=moderate_posterior(), nrep=nrep, tfut=tfut, seed=500 + n,
                    rep0=777, kw=dict(m=M, d=D, KD=1.0, KS=0.4, dS=150.0))
    return dict(row=make_row(n, 4, 0.2, seed=3 * n), post=harsh_posterior(), nrep=nrep, tfut=tfut, seed=900 + n,
                rep0=4321, kw=dict(m=M, d=100.0, KD=KD, KS=KS, dS=150.0))


@functools.lru_cache(maxsize=None)
def wide_reference(n, regime):
    c = wide_case(n, regime)
    counts, last = checker(c["row"], c["post"], c["nrep"], c["tfut"], seed=c["seed"], rep0=c["rep0"], **c["kw"])
    _, first = checker(c["row"], c["post"], c["nrep"], 0, seed=c["seed"], rep0=c["rep0"], **c["kw"])
    return counts, last, first


@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("n", sorted(SIZES))
def test_auto_equals_the_checker(n, regime):
    c = wide_case(n, regime)
    counts, last, first = wide_reference(n, regime)
    if regime == "a":
        assert last.mean() > 0.2  # many patches occupied: the state comparison is sensitive
    else:
        assert 0 < counts[-1] < c["nrep"], counts  # not trivially 0 or nrep
    with mdp.Future(c["row"], c["post"], options=AUTO, **c["kw"]) as f:
        assert f.kernel == f"k_future_wide<{np_of(n)}>"
        got = f.simulate(c["nrep"], c["tfut"], seed=c["seed"], rep0=c["rep0"])
        got_last = f.states(c["nrep"], c["tfut"], seed=c["seed"], rep0=c["rep0"])
        got_first = f.states(c["nrep"], 0, seed=c["seed"], rep0=c["rep0"])
    print(n, regime, "counts", got, "checker", counts, "occupied", int(got_last.sum()), int(last.sum()))
    assert got_first.shape == (c["nrep"], n) and got_first.dtype == bool
    assert np.array_equal(got_first, first)
    assert np.array_equal(got, counts)
    assert np.array_equal(got_last, last)


# ---------------------------------------------------------------------------
# 3. embedding: 64 patches inside a 200-patch row with c = 0
# ---------------------------------------------------------------------------
def test_embedded_64_patches():
    """Patches 64..199 empty, the posterior's mass in column ic = 0 (c = 0):
    c*s1 = 0 never colonises and the draws are addressed by patch index, so
    the counts are the oracle's on the first 64 patches alone."""
    row64 = make_row(64, 3, 0.12, seed=64)
    row = np.zeros(200, dtype=np.int32)
    row[:64] = row64
    post = np.zeros((21, 21))
    post[4:15, 0] = np.linspace(1.0, 3.0, 11)
    w = np.ones(21)
    w[0] = w[-1] = 0.5
    post *= 300.0 / float((np.outer(w, w) * post).sum())  # 3/4 of the mass: carry-over too
    kw = dict(m=M, d=D, KD=1.0, KS=0.5, dS=150.0)
    ref = oracle.future_counts(row64, post, tfut=12, nrep=20000, seed=17, rep0=5, **kw)
    assert ref[0] < 20000 and 0 < ref[-1] < 20000, ref
    with mdp.Future(row, post, options=AUTO, **kw) as f:
        assert f.kernel == "k_future_wide<2>"
        got = f.simulate(20000, 12, seed=17, rep0=5)
    assert np.array_equal(got, ref), (got, ref)


# ---------------------------------------------------------------------------
# 4. plumbing
# ---------------------------------------------------------------------------
def test_splits_and_device_form():
    import torch
    c = wide_case(129, "b")
    N, tfut = 5000, 9
    with mdp.Future(c["row"], c["post"], options=AUTO, **c["kw"]) as f:
        whole = f.simulate(N, tfut, seed=3, rep0=11)
        parts = sum(f.simulate(b - a, tfut, seed=3, rep0=11 + a) for a, b in [(0, 1), (1, 1234), (1234, 1237), (1237, N)])
        out = torch.zeros(tfut, dtype=torch.int64, device="cuda:0")
        st = torch.cuda.current_stream().cuda_stream
        f.simulate_device(out.data_ptr(), N, tfut, seed=3, rep0=11, stream=st)
        f.check(st)
        assert f.time_kernel(N, tfut, seed=3, reps=2) > 0
    assert 0 < whole[-1] < N
    assert np.array_equal(parts, whole)
    assert np.array_equal(out.cpu().numpy().astype(np.uint64), whole)


def test_grid_stride_second_trip():
    """One pass of the grid takes 4 replicates per workgroup x 4096
    workgroups; 7 more take the second trip (one full workgroup and 3 waves of
    another).  The whole run is the sum of its two trips run alone, and the
    tail equals the checker."""
    c = wide_case(65, "b")
    one_pass = 4 * 4096
    N, tfut = one_pass + 7, 3
    with mdp.Future(c["row"], c["post"], options=AUTO, **c["kw"]) as f:
        whole = f.simulate(N, tfut, seed=21)
        first = f.simulate(one_pass, tfut, seed=21)
        tail = f.simulate(7, tfut, seed=21, rep0=one_pass)
        tail_states = f.states(7, tfut, seed=21, rep0=one_pass)
    ref, ref_states = checker(c["row"], c["post"], 7, tfut, seed=21, rep0=one_pass, **c["kw"])
    assert np.array_equal(tail, ref) and np.array_equal(tail_states, ref_states)
    assert np.array_equal(first + tail, whole)
    assert 0 < whole[-1] < N


def test_lookback_flag():
    """A 1e-12-scaled posterior: replicates from 100000 on look back past the
    65536 the engine holds.  The device flag is sticky until check reads it."""
    import torch
    c = wide_case(65, "a")
    st = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    with mdp.Future(c["row"], c["post"] * 1e-12, options=AUTO, **c["kw"]) as bad:
        bad.simulate_device(out.data_ptr(), 8, 4, seed=1, rep0=100000, stream=st)  # overflows
        bad.simulate_device(out.data_ptr(), 8, 4, seed=1, stream=st)               # does not
        with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
            bad.check(st)
        bad.check(st)  # cleared by the previous check
        with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
            bad.simulate(8, 4, seed=1, rep0=100000)
        with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
            bad.states(8, 4, seed=1, rep0=100000)
        bad.check(st)  # the host forms' overflow does not leak into the device flag


def test_states_refusals():
    row = make_row(40, 3, 0.5, seed=1)
    for options in (None, AUTO):  # the lane kernels keep no state
        with mdp.Future(row, posterior21(), m=M, d=D, options=options) as f:
            assert f.kernel == "k_future<64>"
            with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
                f.states(10, 3)
    with mdp.Future(make_row(65, 3, 0.5, seed=1), posterior21(), m=M, d=D, options=AUTO) as f:
        with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
            f.states((1 << 19) + 1, 3)  # W = 2 words per replicate: past the 2^20-word cap
        with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
            f.states(10, 12289)
        assert f.states(0, 3).shape == (0, 65)


# ---------------------------------------------------------------------------
# 5. the drop-ins on a 100-patch occupancy file
# ---------------------------------------------------------------------------
def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def test_dropins_on_100_patches(tmp_path):
    n, nrep, tfut = 100, 60, 6
    rows = [make_row(n, 0, 0.5, seed=7), make_row(n, 3, 0.2, seed=8)]
    occ = tmp_path / "occ100.txt"
    occ.write_text("".join(" ".join(str(int(v)) for v in r) + "\n" for r in rows))
    post = harsh_posterior()
    pfile = tmp_path / "posterior.txt"
    pfile.write_text("".join("".join(f"{v:.17g}\t" for v in r) + "\n" for r in post))
    assert np.array_equal(mdp.read_posterior(pfile), post)
    kw = dict(m=M, d=D, KD=0.07, KS=0.3, dS=150.0)
    ref, _ = checker(rows[-1], post, nrep, tfut, seed=123, **kw)
    assert 0 < ref[-1] < nrep, ref
    want = "".join(f"{int(v)}\t" for v in ref)
    flags = ["-n", str(nrep), "-a", str(tfut), "-m", "400", "-d", "100", "-D", "0.07", "-S", "0.3", "-s", "150", "-i",
             str(occ), "-q", str(pfile), "-r", "123"]
    outs = {}
    for name, prog in (("c", [str(_lib.FUTURE_CLI_PATH)]), ("py", [sys.executable, "-m", "midaspom_amd.future"])):
        for g in ("1", "2"):
            out = tmp_path / f"pext_{name}_{g}.txt"
            r = subprocess.run(prog + flags + ["-g", g, "-o", str(out)], capture_output=True, text=True, timeout=180,
                               env=_env(), cwd=tmp_path)
            assert r.returncode == 0, r.stderr
            outs[name, g] = (out.read_text(), r.stdout)
            assert outs[name, g][0] == want, (name, g)
    # the reference's stdout, the full (n+1) x n migration matrix included
    lines = outs["c", "1"][1].splitlines()
    at = lines.index("Migration matrix:")
    assert all(len(ln.split()) == n for ln in lines[at + 1: at + 2 + n])
    assert lines[at + 2 + n] == "npstates = 8"
    assert outs["py", "1"][1].splitlines()[: at + 3 + n] == lines[: at + 3 + n]


# ---------------------------------------------------------------------------
# 6. the chain users run: posterior, then forecast, on 256 patches
# ---------------------------------------------------------------------------
def test_posterior_then_forecast_on_256_patches(tmp_path):
    occ = synth.write(tmp_path / "occ256.txt", **dict(synth.CONFIG3, T=20))
    pfile = tmp_path / "posterior.txt"
    mdp.run_file(occ, pfile, m=M, d=D, s=101)
    n, tmax, row = mdp.read_survey(occ)
    post = mdp.read_posterior(pfile)
    assert (n, tmax, post.shape) == (256, 20, (101, 101))
    kw = dict(m=M, d=D, KD=1.0, KS=0.0, dS=200.0)
    ref, ref_states = checker(row, post, 30, 5, seed=4, rep0=2, **kw)
    with mdp.Future(row, post, options=AUTO, **kw) as f:
        assert f.kernel == "k_future_wide<2>"
        got = f.simulate(30, 5, seed=4, rep0=2)
        states = f.states(30, 5, seed=4, rep0=2)
    assert np.array_equal(got, ref)
    assert np.array_equal(states, ref_states)
