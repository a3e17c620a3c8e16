"""The stream contract of every device-resident entry point, on a stream that
nothing orders for free.

Every other GPU test passes ``torch.cuda.current_stream().cuda_stream``, which
is 0, HIP's null stream: there every synchronous copy and memset inside the
library falls into line by itself.  Here the caller's stream is a torch side
stream -- non-blocking, a non-zero handle -- with a delay queued on it
(``torch.cuda._sleep``), so that whatever the library does on the null stream
or on a handle's private stream runs at once, DURING the delay, while what it
queues on the caller's stream runs after it.  A slip then gives wrong numbers
every time, not once in a while:

(a) ordering.  delay, a sentinel fill of the output (NaN, or 2^63 - 1 for
    counts), the device-form call, a non-blocking copy to pinned host memory,
    all on the side stream.  A launch or memset that went to another stream
    finishes during the delay and the fill then overwrites it.  After
    ``s.synchronize()`` the copy equals the reference bit for bit and holds no
    sentinel (the padding of an ``ld_out`` larger than needed still holds it).
(b) a new grid under a run in flight: grid A behind the delay, then from the
    host at once grid B (``set_grid`` and a second device-form call, or the
    host form, or -- the simulator -- a second side stream).  B has A's axis
    lengths and A's largest c (both axes reversed on an asymmetric grid): no
    buffer is reallocated and no c table rebuilt, and a run of A that reads
    B's axes gives B's numbers in A's places, never an out-of-range read.
(c) the future engine: the look-back overflow raised behind the delay is seen
    by ``check(s)``, and host forms issued while a device form is pending.

References are the host forms of a FRESH handle, compared with
``np.array_equal``: the rest of the suite ties the host forms to the oracle
and the long-double models, here only ordering is under test.  The only
synchronisation is ``s.synchronize()``; nothing synchronises the device.

The condition that makes a pass mean something: the event recorded behind the
delay has not completed (``query()`` is False) when the host has made its last
enqueue -- for a sequence that ends in a call which itself waits (``set_grid``
under a pending run, a host form, ``time_kernels``, ``check``), when the host
is about to make that call.  If the delay is over by then the test FAILS with
"delay too short"; it neither skips nor passes.

Measured on an MI355X.  ``torch.cuda._sleep`` stalls the stream; it counts the
shader clock: 5 000 000 ticks took 3.55 ms on an idle device (1.41 GHz) and
2.09 to 2.38 ms on a busy one, so the rate is probed once per session and the
delay carries a margin for a clock that rises after the probe
(CLOCK_MARGIN).  The host side of a sequence, from the first enqueue to the
condition, took at most (MEASURED_HOST_MS) 0.17 ms for the posterior engine,
0.07 ms for the scenario engine, 0.60 ms for the simulator (two uploads of a
grid) and 0.32 ms for the future engine; the first launch of a process took
2.8 ms once.  DELAY_MS = 15 is 25 times the longest and 5 times that
outlier; with the margin a test waits 15 to 30 ms, and each took 0.03 to
0.10 s.  On a side stream dealt to the null stream's hardware queue the
simulator's synchronous upload waited out the whole delay every time
(side_stream() explains, and avoids such a stream).

test_host_forms_while_a_device_form_is_pending is a guard, not a detector:
the host form runs at once on the engine's own stream and the device form
only after the delay, so the two cannot be made to overlap with a delay and
the test does not fail deterministically without the fix.
"""
from __future__ import annotations

import functools
import time

import numpy as np
import pytest

import midaspom_amd as mdp
import fwd_ld
from test_future_wide_host import make_row

pytestmark = pytest.mark.gpu

DELAY_MS = 15.0
# torch.cuda._sleep counts the shader clock, which the probe may catch idling
# (measured: 1.41 GHz) while a test runs at up to 2.38 GHz: a ratio of 1.7
CLOCK_MARGIN = 2.0
# the longest host side of each family's sequences in the run the docstring
# cites (ms, first enqueue to the condition)
MEASURED_HOST_MS = {"engine": 0.165, "scenario": 0.069, "simulator": 0.604, "future": 0.319, "first launch": 2.803}
I64_MAX = 2 ** 63 - 1


# ---------------------------------------------------------------------------
# the helper: a side stream, the delay, sentinel-filled outputs, pinned copies
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sleep_ticks_per_ms():
    """Ticks of ``torch.cuda._sleep`` per millisecond on this device, from one
    timed probe on a side stream (after one call that loads the kernel)."""
    import torch
    s = torch.cuda.Stream()
    probe = 5_000_000
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        torch.cuda._sleep(probe)
        b.record(s)
    s.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 1.0, f"torch.cuda._sleep({probe}) took {ms:.3f} ms: it does not stall the stream"
    print(f"\ntorch.cuda._sleep: {probe} ticks = {ms:.2f} ms")
    return probe / ms


@functools.lru_cache(maxsize=None)
def side_stream():
    """The side stream of every test: non-blocking, a non-zero handle, and on
    another hardware queue than the null stream.  HIP deals its streams over a
    few hardware queues (4 by default), and the packets of one queue run in
    order whatever the streams' flags.  A synchronous copy on the null stream
    -- the simulator uploads its grid so in every call -- then waits behind a
    delay on a side stream dealt to the same queue: a false dependency, which
    would order by accident what these tests want left unordered, and make the
    host wait out the delay.  So candidates are probed: a short delay on the
    stream, a synchronous pageable copy on the null stream, and the stream is
    taken if the delay is still running when the copy returns."""
    import torch
    torch.cuda.set_device(0)
    ticks = int(2.0 * CLOCK_MARGIN * sleep_ticks_per_ms())
    dev, host = torch.zeros(16, dtype=torch.float64, device="cuda:0"), torch.ones(16, dtype=torch.float64)
    tried = []  # (kept alive: torch deals its pooled streams round robin)
    for _ in range(16):
        s = torch.cuda.Stream()
        tried.append(s)
        with torch.cuda.stream(s):
            torch.cuda._sleep(ticks)
            ev = torch.cuda.Event()
            ev.record(s)
        dev.copy_(host)
        free = not ev.query()
        s.synchronize()
        if free and s.cuda_stream != 0:
            print(f"\nside stream: candidate {len(tried)} shares no queue with the null stream")
            return s
    pytest.fail("no side stream whose delay a synchronous copy on the null stream does not wait for")


def second_stream():
    """Another side stream than side_stream()."""
    import torch
    for _ in range(4):
        s = torch.cuda.Stream()
        if s.cuda_stream not in (0, side_stream().cuda_stream):
            return s
    pytest.fail("no second side stream")


class Side:
    """The side stream with a delay queued on it.  Outputs are allocated (and
    pinned host copies with them) BEFORE the delay is queued: an allocation
    may synchronise."""

    def __init__(self):
        import torch
        self.torch = torch
        torch.cuda.set_device(0)
        self.ticks = int(DELAY_MS * CLOCK_MARGIN * sleep_ticks_per_ms())
        self.s = side_stream()
        self.h = self.s.cuda_stream
        self.outs = []
        self.ev = None

    def out(self, shape, dtype="f8"):
        torch = self.torch
        dt = torch.float64 if dtype == "f8" else torch.int64
        dev = torch.empty(shape, dtype=dt, device="cuda:0")
        host = torch.empty(shape, dtype=dt).pin_memory()
        host.fill_(0)
        self.outs.append((dev, host))
        return dev

    def delay(self):
        """Queue the delay and, behind it, the sentinel fill of every output."""
        torch = self.torch
        self.t0 = time.perf_counter()
        with torch.cuda.stream(self.s):
            torch.cuda._sleep(self.ticks)
            self.ev = torch.cuda.Event()
            self.ev.record(self.s)
            for dev, _ in self.outs:
                dev.fill_(float("nan") if dev.dtype == torch.float64 else I64_MAX)

    def still_delayed(self, what):
        """The condition: the delay has not run out on the device."""
        host_ms = (time.perf_counter() - self.t0) * 1e3
        done = self.ev.query()
        print(f"\n{what}: host side {host_ms:.3f} ms of a delay of at least {DELAY_MS:.0f} ms")
        if done:
            pytest.fail(f"delay too short: {what} took the host {host_ms:.3f} ms, the delay ({DELAY_MS:.0f} ms or more) "
                        "was over before its last enqueue")

    def fetch(self, *streams):
        """Non-blocking copies to pinned memory on the side stream, then
        s.synchronize() -- of the side stream(s) alone."""
        torch = self.torch
        with torch.cuda.stream(self.s):
            for dev, host in self.outs:
                host.copy_(dev, non_blocking=True)
        for x in streams:
            x.synchronize()
        self.s.synchronize()
        return [host.numpy().copy() for _, host in self.outs]


def no_sentinel(a):
    return not (np.isnan(a).any() if a.dtype == np.float64 else (a == I64_MAX).any())


def u64(a):
    return a.astype(np.uint64)


# ---------------------------------------------------------------------------
# the posterior engine: fwd_ld's case a1 on a 9 x 5 grid
# ---------------------------------------------------------------------------
ENGINE_PATHS = {"fused": {"MDP_FUSED": "1"}, "reading": {"MDP_FUSED": "0"}, "generic": {"MDP_JIT": "0"},
                "wide": {"MDP_WIDE": "1"}}
# asymmetric, so that the reversed axes are another grid with the same largest c
E9 = np.array([0.03, 0.08, 0.15, 0.22, 0.34, 0.47, 0.55, 0.71, 0.9])
C5 = np.array([0.02, 0.11, 0.3, 0.52, 0.85])
GRID_A = (E9, C5)
GRID_B = (E9[::-1].copy(), C5[::-1].copy())


@functools.lru_cache(maxsize=None)
def a1_model():
    return mdp.Model.from_obs(np.ascontiguousarray(fwd_ld._obs_a1(), dtype=np.int32), m=400.0, p=0.5, d=100.0)


def engine(path):
    return mdp.Engine(a1_model(), devices=[0], options=dict(ENGINE_PATHS[path]))


def ran_path(eng, path):
    names, variant = " ".join(sorted(eng.launched())), eng.info()["variant"]
    if path == "fused":
        return "mdp_fwd_jit<fused" in names
    if path == "reading":
        return "mdp_fwd_jit<reading" in names and "k_qrows<" in names
    if path == "generic":
        return variant < 10000 and "k_forward" in names
    return variant >= 20000


@functools.lru_cache(maxsize=None)
def engine_reference(path, which):
    """[ne][nc] of a fresh engine's host form."""
    e, c = GRID_A if which == "A" else GRID_B
    with engine(path) as eng:
        ref = eng.loglik_grid(e, c)
        assert ran_path(eng, path), (path, eng.launched(), eng.info())
    assert np.isfinite(ref).all() and np.unique(ref).size == ref.size
    return ref


def test_the_two_grids_differ():
    """B is A with both axes reversed: the same lengths and largest c, other
    values in every place a run of A could read them."""
    a, b = engine_reference("fused", "A"), engine_reference("fused", "B")
    assert a.shape == b.shape and GRID_A[1].max() == GRID_B[1].max()
    assert (a != b).sum() >= a.size - 1  # (the centre point is its own mirror image)


def engine_view(flat, layout, ne, nc):
    """(the [ne][nc] values, the padding) of an output of leading dimension > needed."""
    if layout == "ec":
        return flat[:, :nc], flat[:, nc:]
    return flat[:, :ne].T, flat[:, ne:]


def engine_out(side, layout, ne, nc):
    return side.out((ne, nc + 3) if layout == "ec" else (nc, ne + 4))


@pytest.mark.parametrize("layout", ["ec", "ce"])
@pytest.mark.parametrize("path", list(ENGINE_PATHS))
def test_engine_run_is_ordered_on_the_stream(path, layout):
    ref = engine_reference(path, "A")
    e, c = GRID_A
    side = Side()
    with engine(path) as eng:
        eng.set_layout(layout)
        eng.set_grid(e, c)
        out = engine_out(side, layout, e.size, c.size)
        side.delay()
        eng.run(out.data_ptr(), out.shape[1], side.h)
        side.still_delayed(f"engine run {path} {layout}")
        got, = side.fetch()
        assert ran_path(eng, path), eng.launched()
    val, pad = engine_view(got, layout, e.size, c.size)
    assert no_sentinel(val)
    assert np.array_equal(val, ref)
    assert np.isnan(pad).all()  # nothing was written past the grid's columns


@pytest.mark.parametrize("layout", ["ec", "ce"])
@pytest.mark.parametrize("path", ["fused", "reading"])
def test_engine_time_kernels_is_ordered_on_the_stream(path, layout):
    """reps = 2 on the side stream: the output is what a plain run computes.
    (time_kernels waits for its own events, so the condition is taken just
    before it.)"""
    ref = engine_reference(path, "A")
    e, c = GRID_A
    side = Side()
    with engine(path) as eng:
        eng.set_layout(layout)
        eng.set_grid(e, c)
        out = engine_out(side, layout, e.size, c.size)
        side.delay()
        side.still_delayed(f"engine time_kernels {path} {layout}")
        ms = eng.time_kernels(out.data_ptr(), out.shape[1], side.h, reps=2)
        got, = side.fetch()
    assert ms and all(v >= 0 for v in ms.values())
    val, pad = engine_view(got, layout, e.size, c.size)
    assert no_sentinel(val) and np.array_equal(val, ref) and np.isnan(pad).all()


@pytest.mark.parametrize("second", ["set_grid", "host-form"])
@pytest.mark.parametrize("path", list(ENGINE_PATHS))
def test_engine_new_grid_under_a_run_in_flight(path, second):
    """Grid A behind the delay; from the host at once grid B, by set_grid and
    a second run on the same stream, or by the host form."""
    ref_a, ref_b = engine_reference(path, "A"), engine_reference(path, "B")
    (ea, ca), (eb, cb) = GRID_A, GRID_B
    side = Side()
    with engine(path) as eng:
        eng.set_grid(ea, ca)
        out_a, out_b = side.out(ref_a.shape), side.out(ref_b.shape)
        side.delay()
        eng.run(out_a.data_ptr(), ca.size, side.h)
        side.still_delayed(f"engine A in flight {path}")
        if second == "set_grid":
            eng.set_grid(eb, cb)
            eng.run(out_b.data_ptr(), cb.size, side.h)
            got_a, got_b = side.fetch()
        else:
            got_b = eng.loglik_grid(eb, cb)
            got_a, _ = side.fetch()
    assert no_sentinel(got_a) and no_sentinel(got_b)
    assert np.array_equal(got_b, ref_b)
    assert np.array_equal(got_a, ref_a), "the run in flight read the next grid"


# ---------------------------------------------------------------------------
# the exact scenario engine: k_scn (n = 6), k_scn_row (n = 9), k_scn_big (n = 3)
# ---------------------------------------------------------------------------
ROW = np.array([1, -1, 0, 1, 0, -1, 1, 1, 0, 1, -1, 0], dtype=np.int32)
SCN = {"k_scn": (6, {}), "k_scn_row": (9, {}), "k_scn_big": (3, {"MDP_SCN_BIG": 1, "MDP_SCN_LAUNCH_PTS": 4})}
SCN_KW = dict(m=400.0, p=0.5, d=100.0)
TS, TDIS = 3, 2
SCN_A = (np.array([0.1, 0.35, 0.6]), np.array([0.2, 0.6]), np.array([0.8, 2.0]), np.array([250.0, 1500.0]))
SCN_B = tuple(x[::-1].copy() for x in SCN_A)


def scn_args(kind, g):
    return (g[0], g[1], g[2], g[3] if kind == "loss" else None)


@functools.lru_cache(maxsize=None)
def scenario_reference(kernel, kind, which):
    n, opts = SCN[kernel]
    with mdp.Scenario(ROW[:n], kind, options=dict(opts), **SCN_KW) as sc:
        ref = sc.lik(*scn_args(kind, SCN_A if which == "A" else SCN_B), ts=TS, tdis=TDIS)
    assert 2 * int((ref > 0).sum()) >= ref.size
    return ref


@pytest.mark.parametrize("timed", [False, True], ids=["run", "time_kernels"])
@pytest.mark.parametrize("kind", ["dieoff", "loss"])
@pytest.mark.parametrize("kernel", list(SCN))
def test_scenario_run_is_ordered_on_the_stream(kernel, kind, timed):
    n, opts = SCN[kernel]
    ref = scenario_reference(kernel, kind, "A")
    side = Side()
    with mdp.Scenario(ROW[:n], kind, options=dict(opts), **SCN_KW) as sc:
        shape = sc.set_grid(*scn_args(kind, SCN_A), ts=TS, tdis=TDIS)
        out = side.out(shape)
        side.delay()
        if timed:  # (waits for its own events: the condition is taken just before)
            side.still_delayed(f"scenario time_kernels {kernel} {kind}")
            sc.time_kernels(out.data_ptr(), side.h, reps=2)
        else:
            sc.run(out.data_ptr(), side.h)
            side.still_delayed(f"scenario run {kernel} {kind}")
        got, = side.fetch()
    assert no_sentinel(got) and np.array_equal(got, ref)


@pytest.mark.parametrize("second", ["set_grid", "host-form"])
@pytest.mark.parametrize("kind", ["dieoff", "loss"])
@pytest.mark.parametrize("kernel", list(SCN))
def test_scenario_new_grid_under_a_run_in_flight(kernel, kind, second):
    n, opts = SCN[kernel]
    ref_a, ref_b = scenario_reference(kernel, kind, "A"), scenario_reference(kernel, kind, "B")
    assert not np.array_equal(ref_a, ref_b)
    side = Side()
    with mdp.Scenario(ROW[:n], kind, options=dict(opts), **SCN_KW) as sc:
        sc.set_grid(*scn_args(kind, SCN_A), ts=TS, tdis=TDIS)
        out_a, out_b = side.out(ref_a.shape), side.out(ref_b.shape)
        side.delay()
        sc.run(out_a.data_ptr(), side.h)
        side.still_delayed(f"scenario A in flight {kernel} {kind}")
        if second == "set_grid":
            sc.set_grid(*scn_args(kind, SCN_B), ts=TS, tdis=TDIS)
            sc.run(out_b.data_ptr(), side.h)
            got_a, got_b = side.fetch()
        else:
            got_b = sc.lik(*scn_args(kind, SCN_B), ts=TS, tdis=TDIS)
            got_a, _ = side.fetch()
    assert no_sentinel(got_a) and no_sentinel(got_b)
    assert np.array_equal(got_b, ref_b)
    assert np.array_equal(got_a, ref_a), "the run in flight read the next grid"


# ---------------------------------------------------------------------------
# the scenario simulator: k_scnsim (n = 9), k_scnsim_wave (n = 70)
# ---------------------------------------------------------------------------
SIM = {"k_scnsim": 9, "k_scnsim_wave": 70}
SIM_OPTS = {"MDP_SIM_WAVE": "auto", "MDP_SIM_LAUNCH_PTS": 3}
SIM_KW = dict(ts=4, tdis=3, nrep=300, seed=11, rep0=5)
SIM_A = (np.array([0.05, 0.4]), np.array([0.1, 0.7]), np.array([0.8, 2.5]), np.array([250.0, 1500.0]))
SIM_B = tuple(x[::-1].copy() for x in SIM_A)


def sim_row(kernel):
    return ROW[:9] if SIM[kernel] == 9 else make_row(70, 2, 0.5, seed=70)


def simulator(kernel, kind, warm=None):
    """warm: a grid for one host-form call of one replicate.  A simulator sets
    its device side up (allocations, a stream, events) in its first computing
    call, and an allocation may wait for the device: the tests make that call
    before they queue the delay, with the OTHER grid, so that the buffer the
    kernels read holds the wrong axes until the call under test uploads its own."""
    sim = mdp.ScenarioSim(sim_row(kernel), kind, options=dict(SIM_OPTS), **SCN_KW)
    assert sim.kernel.startswith(kernel + "<"), sim.kernel
    if warm is not None:
        sim.tables(*scn_args(kind, warm), **{**SIM_KW, "nrep": 1})
    return sim


@functools.lru_cache(maxsize=None)
def sim_reference(kernel, kind, which):
    with simulator(kernel, kind) as sim:
        hist, match = sim.tables(*scn_args(kind, SIM_A if which == "A" else SIM_B), **SIM_KW)
    assert (hist.sum(-1) == SIM_KW["nrep"]).all()
    return hist, match


def sim_outs(side, ref):
    return side.out(ref[0].shape, "i8"), side.out(ref[1].shape, "i8")


def sim_equal(got, ref, what):
    for g, r, name in zip(got, ref, ("hist", "match")):
        assert no_sentinel(g), (what, name)
        assert np.array_equal(u64(g), r), (what, name)


@pytest.mark.parametrize("kind", ["dieoff", "loss"])
@pytest.mark.parametrize("kernel", list(SIM))
def test_simulator_tables_device_is_ordered_on_the_stream(kernel, kind):
    ref = sim_reference(kernel, kind, "A")
    side = Side()
    with simulator(kernel, kind, warm=SIM_B) as sim:
        dh, dm = sim_outs(side, ref)
        side.delay()
        sim.tables_device(dh.data_ptr(), dm.data_ptr(), *scn_args(kind, SIM_A), stream=side.h, **SIM_KW)
        side.still_delayed(f"simulator tables_device {kernel} {kind}")
        got = side.fetch()
    sim_equal(got, ref, "A")


@pytest.mark.parametrize("second", ["same-stream", "host-form", "second-stream"])
@pytest.mark.parametrize("kind", ["dieoff", "loss"])
@pytest.mark.parametrize("kernel", list(SIM))
def test_simulator_new_grid_under_a_run_in_flight(kernel, kind, second):
    """Every call uploads its grid: A behind the delay, then B by a second
    tables_device on the same stream, by the host form, or by a
    tables_device on a second side stream with nothing queued on it."""
    ref_a, ref_b = sim_reference(kernel, kind, "A"), sim_reference(kernel, kind, "B")
    assert not np.array_equal(ref_a[0], ref_b[0])
    side = Side()
    other = second_stream()
    with simulator(kernel, kind, warm=SIM_B) as sim:
        a, b = sim_outs(side, ref_a), sim_outs(side, ref_b)
        side.delay()
        sim.tables_device(a[0].data_ptr(), a[1].data_ptr(), *scn_args(kind, SIM_A), stream=side.h, **SIM_KW)
        side.still_delayed(f"simulator A in flight {kernel} {kind}")
        if second == "host-form":
            got_b = sim.tables(*scn_args(kind, SIM_B), **SIM_KW)
            got_a = side.fetch()[:2]
        else:
            st = side.h if second == "same-stream" else other.cuda_stream
            sim.tables_device(b[0].data_ptr(), b[1].data_ptr(), *scn_args(kind, SIM_B), stream=st, **SIM_KW)
            if second == "second-stream":  # B's tables are read on the first stream: order it after the second
                side.s.wait_stream(other)
            got = side.fetch(other) if second == "second-stream" else side.fetch()
            got_a, got_b = got[:2], got[2:]
    sim_equal(got_b, ref_b, "B")
    sim_equal(got_a, ref_a, "A (the run in flight read the next grid)")


# ---------------------------------------------------------------------------
# the future engine: k_future<8> (n = 8), k_future_wide<1> (n = 70)
# ---------------------------------------------------------------------------
FUT = {"k_future": 8, "k_future_wide": 70}
FUT_KW = dict(m=400.0, d=100.0, KD=0.3, KS=0.2, dS=150.0)
NREP, TFUT = 4096, 6
FUT_RUN = dict(seed=7, rep0=3)


def harsh21():
    """21 steps, the mass at e near 0.2 and c near 0.02: replicates go extinct
    within a few years (tests/test_gpu_future_wide.py's posterior)."""
    g = np.arange(21) * 0.01
    post = np.exp(-((g[:, None] - 0.2) / 0.03) ** 2 - ((g[None, :] - 0.02) / 0.02) ** 2)
    w = np.ones(21)
    w[0] = w[-1] = 0.5
    return post * (400.0 / float((np.outer(w, w) * post).sum()))


def future(kernel, post=None, sum_years=False):
    n = FUT[kernel]
    opts = "MDP_FUT_WIDE=auto" + (";MDP_FUT_SUM_YEARS=2" if sum_years else "")
    f = mdp.Future(make_row(n, 2, 0.4, seed=300 + n), harsh21() if post is None else post, options=opts, **FUT_KW)
    assert f.kernel.startswith(kernel + "<"), f.kernel
    return f


@functools.lru_cache(maxsize=None)
def future_reference(kernel):
    with future(kernel, sum_years=True) as f:
        counts = f.simulate(NREP, TFUT, **FUT_RUN)
        hist, occ = f.summary(NREP, TFUT, **FUT_RUN)
    assert (hist.sum(-1) == NREP).all() and np.array_equal(hist[:, 0], counts) and occ.sum() > 0
    return counts, hist, occ


@pytest.mark.parametrize("kernel", list(FUT))
def test_future_simulate_device_is_ordered_on_the_stream(kernel):
    counts, _, _ = future_reference(kernel)
    side = Side()
    with future(kernel) as f:
        out = side.out((TFUT,), "i8")
        side.delay()
        f.simulate_device(out.data_ptr(), NREP, TFUT, stream=side.h, **FUT_RUN)
        side.still_delayed(f"future simulate_device {kernel}")
        got, = side.fetch()
        f.check(side.h)
    assert no_sentinel(got) and np.array_equal(u64(got), counts)


@pytest.mark.parametrize("kernel", list(FUT))
def test_future_summary_device_is_ordered_on_the_stream(kernel):
    """MDP_FUT_SUM_YEARS=2: three windows of years, the replicate records
    carried from one launch to the next."""
    _, hist, occ = future_reference(kernel)
    side = Side()
    with future(kernel, sum_years=True) as f:
        dh, do = side.out(hist.shape, "i8"), side.out(occ.shape, "i8")
        side.delay()
        f.summary_device(dh.data_ptr(), do.data_ptr(), NREP, TFUT, stream=side.h, **FUT_RUN)
        side.still_delayed(f"future summary_device {kernel}")
        got_h, got_o = side.fetch()
        f.check(side.h)
    assert no_sentinel(got_h) and no_sentinel(got_o)
    assert np.array_equal(u64(got_h), hist) and np.array_equal(u64(got_o), occ)


@pytest.mark.parametrize("kernel", list(FUT))
def test_future_check_waits_for_the_stream(kernel):
    """A posterior scaled by 1e-12: replicates from 100000 on look back past
    the 65536 the engine holds.  The overflow is raised by a launch behind
    the delay; check(s) waits for it, refuses and clears the flag."""
    side = Side()
    with future(kernel, post=harsh21() * 1e-12) as bad:
        out = side.out((4,), "i8")
        side.delay()
        bad.simulate_device(out.data_ptr(), 8, 4, seed=1, rep0=100000, stream=side.h)
        side.still_delayed(f"future overflow {kernel}")
        with pytest.raises(mdp.MidaspomError, match="UNSUPPORTED"):
            bad.check(side.h)
        assert side.ev.query()  # check waited for the stream
        bad.simulate_device(out.data_ptr(), 8, 4, seed=1, stream=side.h)  # no look-back past the limit
        bad.check(side.h)
        side.fetch()


@pytest.mark.parametrize("form", ["summary", "simulate"])
@pytest.mark.parametrize("kernel", list(FUT))
def test_host_forms_while_a_device_form_is_pending(kernel, form):
    """A guard (the module docstring): the host forms share dpartial, dtab
    and the replicate records with the device form pending behind the delay;
    each gives its fresh-handle result."""
    counts, hist, occ = future_reference(kernel)
    side = Side()
    with future(kernel, sum_years=True) as f:
        dc, dh, do = side.out((TFUT,), "i8"), side.out(hist.shape, "i8"), side.out(occ.shape, "i8")
        side.delay()
        f.simulate_device(dc.data_ptr(), NREP, TFUT, stream=side.h, **FUT_RUN)
        f.summary_device(dh.data_ptr(), do.data_ptr(), NREP, TFUT, stream=side.h, **FUT_RUN)
        side.still_delayed(f"future device forms pending {kernel}")
        if form == "summary":
            host_h, host_o = f.summary(NREP, TFUT, **FUT_RUN)
            assert np.array_equal(host_h, hist) and np.array_equal(host_o, occ)
        else:
            assert np.array_equal(f.simulate(NREP, TFUT, **FUT_RUN), counts)
        got_c, got_h, got_o = side.fetch()
        f.check(side.h)
    assert no_sentinel(got_c) and no_sentinel(got_h) and no_sentinel(got_o)
    assert np.array_equal(u64(got_c), counts) and np.array_equal(u64(got_h), hist) and np.array_equal(u64(got_o), occ)
