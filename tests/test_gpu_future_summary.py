"""The future engine's summaries on the GPU (mdp_future_summary): hist[t][m],
the replicates with exactly m occupied patches after year t + 1, and
occ[t][k], those with patch k occupied -- from the lane kernels
(k_future_tab<NM>) and the patch-parallel ones (k_future_wide_tab<NP>),
against the reference-pinned oracle (hist[:, 0]) and the per-year numpy
checker of test_future_summary_host.py (both tables, cell for cell), across
window boundaries (MDP_FUT_SUM_YEARS), through the plumbing (splits,
accumulation, device form, one table alone, the grid stride's second trip),
the refusals and both drop-ins.
"""
from __future__ import annotations

import ctypes
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import midaspom_amd as mdp
import oracle
from midaspom_amd import _lib, rpost
from test_future_summary_host import identities, summary_checker
from test_future_wide_host import make_row, posterior21
from test_gpu_future_wide import AUTO, D, M, NMISS, TWO32, WIDE, harsh21, harsh_posterior, np_of, wide_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def years(cap):
    return f";MDP_FUT_SUM_YEARS={cap}" if cap else ""


# ---------------------------------------------------------------------------
# 1. the lane kernels and MDP_FUT_WIDE=1 up to 64 patches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("KD,KS,dS", [(1.0, 0.0, 200.0), (0.3, 2.0, 50.0)])
@pytest.mark.parametrize("n", [1, 2, 9, 33, 64])
def test_lane_and_wide_tables(n, KD, KS, dS):
    """hist[:, 0] equals the oracle's counts, the two kernels' tables equal
    each other, and at 300 replicates both equal the per-year checker."""
    row = make_row(n, NMISS[n], 0.5 if n < 9 else 0.15, seed=40 + n)
    post = harsh21() * 0.5
    kw = dict(m=M, d=D, KD=KD, KS=KS, dS=dS)
    nrep, tfut, seed, rep0 = 3000, 10, (1 << 35) + 8, TWO32 - 1500
    ref = oracle.future_counts(row, post, tfut=tfut, nrep=nrep, seed=seed, rep0=rep0, **kw)
    chk_hist, chk_occ, _ = summary_checker(row, post, 300, tfut, seed=seed, rep0=rep0, **kw)
    got = {}
    for opts in (AUTO, WIDE):
        with mdp.Future(row, post, options=opts, **kw) as f:
            nm = 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64
            assert f.kernel == ("k_future_wide<1>" if opts == WIDE else f"k_future<{nm}>")
            got[opts] = f.summary(nrep, tfut, seed=seed, rep0=rep0)
            small = f.summary(300, tfut, seed=seed, rep0=rep0)
        hist, occ = got[opts]
        assert hist.shape == (tfut, n + 1) and occ.shape == (tfut, n) and hist.dtype == occ.dtype == np.uint64
        print(n, KD, KS, opts, "hist[:,0]", hist[:, 0], "oracle", ref)
        assert np.array_equal(hist[:, 0], ref)
        identities(hist, occ, nrep)
        assert np.array_equal(small[0], chk_hist)
        assert np.array_equal(small[1], chk_occ)
    assert ref.max() > 0 and ref.min() < nrep
    assert np.array_equal(got[AUTO][0], got[WIDE][0])
    assert np.array_equal(got[AUTO][1], got[WIDE][1])


# ---------------------------------------------------------------------------
# 2. MDP_FUT_WIDE=auto beyond 64 patches against the per-year checker
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_tables(n, regime):
    c = wide_case(n, regime)
    hist, occ, _ = summary_checker(c["row"], c["post"], c["nrep"], c["tfut"], seed=c["seed"], rep0=c["rep0"], **c["kw"])
    hist.setflags(write=False)
    occ.setflags(write=False)
    return hist, occ


@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("n", [65, 128, 129, 257, 1024])
def test_auto_tables_equal_the_checker(n, regime):
    c = wide_case(n, regime)
    hist, occ = wide_tables(n, regime)
    # non-vacuity, on the reference tables
    if regime == "a":
        assert len(np.flatnonzero(hist[-1])) >= 5   # a spread of occupied counts in the last year
        assert occ[-1].min() > 0                    # every patch occupied in some replicate
    else:
        assert 0 < hist[-1][0] < c["nrep"]          # K_S = 0: through the shortcut; 0.3: past it
    with mdp.Future(c["row"], c["post"], options=AUTO, **c["kw"]) as f:
        assert f.kernel == f"k_future_wide<{np_of(n)}>"
        got_hist, got_occ = f.summary(c["nrep"], c["tfut"], seed=c["seed"], rep0=c["rep0"])
    print(n, regime, "hist[-1] cells", np.flatnonzero(got_hist[-1]), "occ[-1] range", got_occ[-1].min(),
          got_occ[-1].max())
    assert np.array_equal(got_hist, hist)
    assert np.array_equal(got_occ, occ)
    identities(got_hist, got_occ, c["nrep"])


# ---------------------------------------------------------------------------
# 3. window boundaries
# ---------------------------------------------------------------------------
def test_windows_lane():
    """8 years in windows of 1, 3 (a ragged last window) and the engine's own
    choice: the same tables, equal to the checker."""
    n = 33
    row = make_row(n, NMISS[n], 0.15, seed=40 + n)
    post = harsh21() * 0.5
    kw = dict(m=M, d=D, KD=0.3, KS=2.0, dS=50.0)
    ref_hist, ref_occ, _ = summary_checker(row, post, 300, 8, seed=5, rep0=TWO32 - 100, **kw)
    for cap in (1, 3, 0):
        with mdp.Future(row, post, options=AUTO + years(cap), **kw) as f:
            hist, occ = f.summary(300, 8, seed=5, rep0=TWO32 - 100)
        assert np.array_equal(hist, ref_hist), cap
        assert np.array_equal(occ, ref_occ), cap


def test_windows_wide_extinct_replicates_cross_boundaries():
    """Regime (b) at K_S = 0: extinct replicates keep adding to hist[.][0]
    in every later window."""
    c = wide_case(65, "b")
    assert c["kw"]["KS"] == 0.0 and c["tfut"] == 8
    ref_hist, ref_occ = wide_tables(65, "b")
    assert 0 < ref_hist[2][0] < ref_hist[-1][0]  # extinct before year 3's boundary, more later
    for cap in (1, 3, 0):
        with mdp.Future(c["row"], c["post"], options=AUTO + years(cap), **c["kw"]) as f:
            hist, occ = f.summary(c["nrep"], c["tfut"], seed=c["seed"], rep0=c["rep0"])
        assert np.array_equal(hist, ref_hist), cap
        assert np.array_equal(occ, ref_occ), cap


# ---------------------------------------------------------------------------
# 4. plumbing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lane", "wide"])
def test_splits_accumulation_device_form_and_single_tables(kind):
    import torch
    if kind == "lane":
        n = 9
        row, post = make_row(n, NMISS[n], 0.15, seed=49), harsh21() * 0.5
        kw, N, opts = dict(m=M, d=D, KD=0.3, KS=2.0, dS=50.0), 5000, AUTO + years(4)
    else:
        c = wide_case(129, "b")
        n, row, post, kw, N, opts = 129, c["row"], c["post"], c["kw"], 1500, AUTO + years(4)
    tfut = 9
    with mdp.Future(row, post, options=opts, **kw) as f:
        hist, occ = f.summary(N, tfut, seed=3, rep0=11)
        identities(hist, occ, N)
        assert np.array_equal(hist[:, 0], f.simulate(N, tfut, seed=3, rep0=11))
        # three uneven sub-ranges into the same arrays
        h2, o2 = np.zeros_like(hist), np.zeros_like(occ)
        for a, b in [(0, 1), (1, 1234), (1234, N)]:
            f.summary(b - a, tfut, seed=3, rep0=11 + a, hist=h2, occ=o2)
        assert np.array_equal(h2, hist) and np.array_equal(o2, occ)
        # the host form accumulates
        f.summary(N, tfut, seed=3, rep0=11, hist=h2, occ=o2)
        assert np.array_equal(h2, 2 * hist) and np.array_equal(o2, 2 * occ)
        # one table alone
        h_only, none = f.summary(N, tfut, seed=3, rep0=11, occ=False)
        assert none is None and np.array_equal(h_only, hist)
        none, o_only = f.summary(N, tfut, seed=3, rep0=11, hist=False)
        assert none is None and np.array_equal(o_only, occ)
        # the device form overwrites, and takes either table alone
        st = torch.cuda.current_stream().cuda_stream
        dh = torch.full((tfut, n + 1), 7, dtype=torch.int64, device="cuda:0")
        do = torch.full((tfut, n), 7, dtype=torch.int64, device="cuda:0")
        f.summary_device(dh.data_ptr(), do.data_ptr(), N, tfut, seed=3, rep0=11, stream=st)
        f.check(st)
        assert np.array_equal(dh.cpu().numpy().astype(np.uint64), hist)
        assert np.array_equal(do.cpu().numpy().astype(np.uint64), occ)
        dh.fill_(7)
        do.fill_(7)
        f.summary_device(dh.data_ptr(), 0, N, tfut, seed=3, rep0=11, stream=st)
        f.summary_device(0, do.data_ptr(), N, tfut, seed=3, rep0=11, stream=st)
        f.check(st)
        assert np.array_equal(dh.cpu().numpy().astype(np.uint64), hist)
        assert np.array_equal(do.cpu().numpy().astype(np.uint64), occ)
        assert f.time_summary(N, tfut, seed=3, reps=2) > 0
    assert 0 < hist[-1][0] < N


def test_grid_stride_second_trip_lane():
    """k_future_tab<8>: 2048 workgroups x 256 lanes per trip; 4096*256 + 777
    replicates take a second and a third trip, the last with a ragged wave."""
    n = 7
    row = make_row(n, 2, 0.5, seed=47)
    post = harsh21() * 0.5
    kw = dict(m=M, d=D, KD=1.0, KS=0.0, dS=200.0)
    N, tfut = 4096 * 256 + 777, 3
    ref = oracle.future_counts(row, post, tfut=tfut, nrep=N, seed=21, rep0=0, **kw)
    with mdp.Future(row, post, options=AUTO, **kw) as f:
        assert f.kernel == "k_future<8>"
        hist, occ = f.summary(N, tfut, seed=21)
    identities(hist, occ, N)
    assert np.array_equal(hist[:, 0], ref)


def test_grid_stride_second_trip_wide():
    """k_future_wide_tab<1> at 65 patches: 4096*4 + 5 replicates, several
    trips of the 2048-workgroup grid and a workgroup with one wave at work."""
    c = wide_case(65, "b")
    N, tfut = 4096 * 4 + 5, 3
    with mdp.Future(c["row"], c["post"], options=AUTO, **c["kw"]) as f:
        assert f.kernel == "k_future_wide<1>"
        hist, occ = f.summary(N, tfut, seed=21)
        counts = f.simulate(N, tfut, seed=21)
    identities(hist, occ, N)
    assert np.array_equal(hist[:, 0], counts)
    # beyond the oracle's 64 patches the plain kernel is the pinned reference
    # of hist[:, 0] (test_gpu_future_wide.py pins it to the checker)
    assert 0 < counts[-1] < N


# ---------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------
def test_refusals():
    with mdp.Future(make_row(1024, 4, 0.2, seed=1), posterior21(), m=M, d=D, options=AUTO) as f:
        with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
            f.summary(10, 1024)                      # 1024 * 2049 cells > 2^21
        hist, occ = f.summary(2, 2)
        identities(hist, occ, 2)
    with mdp.Future(make_row(9, 2, 0.5, seed=1), posterior21(), m=M, d=D) as f:
        for tfut in (0, 12289):
            with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
                f.summary(10, tfut)
        with pytest.raises(mdp.MidaspomError, match="EINVAL"):
            f.summary(10, 5, hist=False, occ=False)  # both tables NULL
        with pytest.raises(mdp.MidaspomError, match="EINVAL"):
            f.summary_device(0, 0, 10, 5)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        assert _lib.lib().mdp_future_summary(f._h, 0, 0, 10, 5, u64p(), u64p()) != 0
    for options in ("MDP_FUT_SUM_YEARS=many", "MDP_FUT_SUM_YEARS=12289", "MDP_FUT_SUM_YEARS=", "MDP_FUT_SUM_YEARS=-3"):
        with pytest.raises(mdp.MidaspomError, match="EINVAL"):
            mdp.Future(np.ones(9, dtype=np.int32), posterior21(), options=options)


@pytest.mark.parametrize("opts", [None, WIDE])
def test_lookback_flag(opts):
    """A 1e-12-scaled posterior: replicates from 100000 on look back past the
    65536 the engine holds (test_gpu_future_wide.test_lookback_flag's
    construction).  The host form refuses; the device form raises the sticky
    flag that check() reads."""
    import torch
    row = make_row(9, 2, 0.5, seed=1)
    st = torch.cuda.current_stream().cuda_stream
    dh = torch.zeros((4, 10), dtype=torch.int64, device="cuda:0")
    with mdp.Future(row, posterior21() * 1e-12, m=M, d=D, options=opts) as bad:
        bad.summary_device(dh.data_ptr(), 0, 8, 4, seed=1, rep0=100000, stream=st)  # overflows
        bad.summary_device(dh.data_ptr(), 0, 8, 4, seed=1, stream=st)               # does not
        with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
            bad.check(st)
        bad.check(st)  # cleared by the previous check
        with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
            bad.summary(8, 4, seed=1, rep0=100000)
        bad.check(st)  # the host form's overflow does not leak into the device flag


# ---------------------------------------------------------------------------
# 6. the drop-ins
# ---------------------------------------------------------------------------
def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _files(tmp_path, n):
    rows = [make_row(n, 0, 0.5, seed=7), make_row(n, 3, 0.2, seed=8)]
    occ = tmp_path / f"occ{n}.txt"
    occ.write_text("".join(" ".join(str(int(v)) for v in r) + "\n" for r in rows))
    post = harsh_posterior()
    pfile = tmp_path / f"posterior{n}.txt"
    pfile.write_text("".join("".join(f"{v:.17g}\t" for v in r) + "\n" for r in post))
    return rows[-1], post, occ, pfile


def _table(a):
    return "".join("".join(f"{int(v)}\t" for v in r) + "\n" for r in a)


@pytest.mark.parametrize("n", [9, 200])
def test_dropins_write_the_tables(tmp_path, n):
    nrep, tfut = 600, 6
    row, post, occ_file, pfile = _files(tmp_path, n)
    kw = dict(m=M, d=D, KD=0.07 if n > 64 else 0.5, KS=0.3, dS=150.0)
    with mdp.Future(row, post, options=AUTO, **kw) as f:
        hist, occ = f.summary(nrep, tfut, seed=123)
    flags = ["-n", str(nrep), "-a", str(tfut), "-m", "400", "-d", "100", "-D", str(kw["KD"]), "-S", "0.3", "-s", "150",
             "-i", str(occ_file), "-q", str(pfile), "-r", "123"]
    progs = (("c", [str(_lib.FUTURE_CLI_PATH)]), ("py", [sys.executable, "-m", "midaspom_amd.future"]))
    for name, prog in progs:
        plain = tmp_path / f"plain_{name}.txt"
        r0 = subprocess.run(prog + flags + ["-o", str(plain)], capture_output=True, text=True, timeout=180, env=_env(),
                            cwd=tmp_path)
        assert r0.returncode == 0, r0.stderr
        for g in ("1", "3"):
            o, h, k = (tmp_path / f"{x}_{name}_{g}.txt" for x in ("pext", "hist", "occ"))
            r = subprocess.run(prog + flags + ["-g", g, "-o", str(o), "-H", str(h), "-O", str(k)], capture_output=True,
                               text=True, timeout=180, env=_env(), cwd=tmp_path)
            assert r.returncode == 0, r.stderr
            assert o.read_bytes() == plain.read_bytes()
            assert h.read_text() == _table(hist) and k.read_text() == _table(occ), (name, g)
            got = rpost.read_future_summary(h, k, n=n, tfut=tfut)
            assert np.array_equal(got[0], hist) and np.array_equal(got[1], occ)
            # the new lines come after the existing one, and only with the flags
            tail = [ln for ln in r.stdout.splitlines() if ln.startswith("Writing on file")]
            assert tail == [f"Writing on file {x}... done" for x in (o, h, k)]
        assert r0.stdout.count("Writing on file") == 1
    assert len(np.flatnonzero(hist[-1])) >= 2


def test_torchrun_two_ranks_write_the_tables(tmp_path):
    n, nrep, tfut = 9, 601, 6
    row, post, occ_file, pfile = _files(tmp_path, n)
    flags = ["-n", str(nrep), "-a", str(tfut), "-m", "400", "-d", "100", "-D", "0.5", "-S", "0.3", "-s", "150", "-i",
             str(occ_file), "-q", str(pfile), "-r", "123"]
    names = {}
    for tag in ("single", "multi"):
        names[tag] = [str(tmp_path / f"{x}_{tag}.txt") for x in ("pext", "hist", "occ")]
    out = ["-o", names["single"][0], "-H", names["single"][1], "-O", names["single"][2]]
    r1 = subprocess.run([sys.executable, "-m", "midaspom_amd.future", *flags, *out], capture_output=True, text=True,
                        timeout=180, env=_env(), cwd=ROOT)
    assert r1.returncode == 0, r1.stderr
    out = ["-o", names["multi"][0], "-H", names["multi"][1], "-O", names["multi"][2]]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           "-m", "midaspom_amd.future", "--backend", "gloo", *flags, *out]
    r2 = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=_env(), cwd=ROOT)
    assert r2.returncode == 0, r2.stderr[-3000:]
    for a, b in zip(names["single"], names["multi"]):
        assert open(a, "rb").read() == open(b, "rb").read()
    hist, occ = rpost.read_future_summary(names["multi"][1], names["multi"][2], n=n, tfut=tfut)
    identities(hist, occ, nrep)
