"""One context used the way the driver, the benchmark and a long-lived caller
use it: cocoa_init again on a used context, another method / H / solver,
cocoa_set_train / cocoa_set_test on a context that has run, the state setters
between rounds (hingeDriver.scala:84-109 runs its five methods one after
another on one SparkContext; bench.py re-initialises its engine for the
time-to-gap leg).

A *leg* is (method, H, lam, beta, gamma, seed, solver) run for T rounds.  The
checked engine runs a dirtying leg first and is left the way a caller that
stopped early leaves it: one more round enqueued (with its Gram prefetch for
the round after), and an evaluation begun (cocoa_eval_begin, or
cocoa_eval_async with no round behind it) that nobody collects.  Then leg B,
compared with a fresh oracle.Run of leg B alone and with a fresh engine that
ran leg B alone:

* strict: w, alpha and the hex of primal / gap equal both, bit for bit;
* fast: against the oracle w within 1e-9 max|w|, alpha within 1e-9, primal and
  gap within 1e-9 |P|, error counts exact (the north_star tolerance); against
  the fresh engine w within 1e-12 max|w| and alpha within 1e-12 (the bound
  test_gpu_mirror.py / test_gpu_compact.py use between two orders of the same
  sums);
* the cocoa_plan_info flags of the path the leg was meant to take, and the same
  flags as the fresh engine's.

State leaks these tests found (both fixed in engine.hip):

* cocoa_eval_async, then cocoa_set_solver, then cocoa_init: cocoa_init failed
  with "call cocoa_init first" -- eval_quiesce enqueued the never-fired
  evaluation only to drop it, and the enqueue needs an initialised context
  (test_solver_switches_on_one_engine).
* a multi-device context kept an uncollected cocoa_eval_begin across
  cocoa_init / cocoa_set_train / cocoa_set_test: every later cocoa_eval raised
  "an evaluation is pending" (test_multi_member_context_driver_order).
"""
import contextlib
import math
import multiprocessing as mp
import os
from collections import namedtuple

import numpy as np
import pytest

import cocoa_amd
from cocoa_amd import Engine, LabeledData, configs
from cocoa_amd._capi import E_STATE
from cocoa_amd.configs import shard_bounds
from cocoa_amd.engine import comm_unique_id
from oracle import oracle
from tests.test_gpu_gram import _edge

pytestmark = pytest.mark.gpu
REL, SAME = 1e-9, 1e-12
ORDER = ["cocoa+", "cocoa", "mbcd", "mbsgd", "localsgd"]  # hingeDriver.scala:84-109
FLAGS = ("solver", "gram_mirror", "xw_producer", "eval_split", "eval_test_split", "mbsgd_pull", "dw_compact",
         "dw_dbuf")
BIG = 1 << 30  # numRounds as bench.py passes it: every round prefetches the next one's Gram rows

Leg = namedtuple("Leg", "method H lam beta gamma seed solver", defaults=(200, 2e-3, 1.0, 1.0, 5, "auto"))


def odata(d):
    return oracle.Data(d.row_ptr, d.col, d.val, d.y, d.part_ptr, d.num_features)


class Data:
    def __init__(self, name, tr, te, env=None, dense=False):
        self.name, self.tr, self.te, self.env, self.dense = name, tr, te, env or {}, dense
        self.od, self.ot = odata(tr), odata(te)


def _dense_rows(rng, n, d, part):
    X = rng.standard_normal((n, d)) / np.sqrt(d)
    return LabeledData(np.arange(n + 1, dtype=np.int64) * d, np.tile(np.arange(d, dtype=np.int32), n), X.reshape(-1),
                       np.where(rng.random(n) < 0.5, 1.0, -1.0), np.asarray(part, np.int64), d)


_DATA, _REF, _FRESH = {}, {}, {}


def data(name):
    """The data sets of this module, built once: the C2-shaped share every test
    uses, the edge rows (duplicates, empty rows, 5,000-entry rows, a one-row
    partition; another d), a C4-shaped share on compact deltaW slices, dense rows."""
    if name not in _DATA:
        if name == "c2":
            sh = configs.share("c2", n=12000, parts=16, n_test=1000)
            _DATA[name] = Data(name, sh.train, sh.test)
        elif name == "edge":
            tr = _edge()
            _DATA[name] = Data(name, tr, tr.row_range(200, 900))
        elif name == "c4":
            sh = configs.share("c4", n=8000, d=100000, parts=8, n_test=500)
            _DATA[name] = Data(name, sh.train, sh.test, env={"COCOA_DW_COMPACT": "1"})
        elif name == "dense":
            rng = np.random.default_rng(17)
            _DATA[name] = Data(name, _dense_rows(rng, 2048, 64, configs.balanced(2048, 8)),
                               _dense_rows(rng, 256, 64, [0, 256]), dense=True)
    return _DATA[name]


@pytest.fixture(scope="module")
def c2():
    return data("c2")


@contextlib.contextmanager
def _env(monkeypatch, env):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        yield
    finally:
        for k in env or {}:
            monkeypatch.delenv(k)


def load(e, D, monkeypatch, test=True):
    with _env(monkeypatch, D.env):
        if D.dense:
            e.set_train_dense(D.tr.val.reshape(D.tr.n, D.tr.num_features), D.tr.y, D.tr.part_ptr)
        else:
            e.set_train(D.tr)
    if test:
        e.set_test(D.te)
    return e


def ref(D, leg, T):
    """The oracle's leg alone (computed once, never modified)."""
    key = (D.name, leg, T)
    if key not in _REF:
        run = oracle.Run(D.od, leg.method, D.tr.n, leg.H, leg.lam, leg.beta, leg.gamma, seed=leg.seed, nthreads=8)
        evs = []
        for t in range(1, T + 1):
            run.round(t)
            evs.append(run.eval(D.ot))
        _REF[key] = dict(w=run.w(), alpha=run.alpha(), evs=evs)
    return _REF[key]


def set_solver(e, kind):
    if getattr(e, "_solver", "auto") != kind:  # (cocoa_set_solver revokes the init: only when the leg changes it)
        e.set_solver(kind)
        e._solver = kind


def run_leg(e, D, leg, T, monkeypatch, flow="deferred", dirty="begin", env=None):
    """Leg on engine e: T rounds, each evaluated in `flow` (deferred: eval_begin
    behind round t, eval_end once round t+1 is queued; async: eval_async /
    eval_wait the same way; sync: eval after every round).  (w, alpha) are read
    after round T; then the leg ends dirty: round T+1 and an evaluation begun
    (dirty="begin") or snapshotted with no round behind it ("async"), never
    collected."""
    set_solver(e, leg.solver)
    with _env(monkeypatch, env):
        e.init(leg.method, D.tr.n, BIG, leg.H, leg.lam, leg.beta, leg.gamma, 1, leg.seed)
    plan = e.plan()
    begin, end = (e.eval_async, e.eval_wait) if flow == "async" else (e.eval_begin, e.eval_end)
    evs, pending = [], False
    for t in range(1, T + 1):
        e.round(t)
        if flow == "sync":
            evs.append(e.eval())
            continue
        if pending:
            evs.append(end())
        begin()
        pending = True
    w, alpha = e.w(), e.alpha()
    if dirty:
        e.round(T + 1)
    if pending:
        evs.append(end())
    if dirty:
        (e.eval_async if dirty == "async" else e.eval_begin)()
    return dict(w=w, alpha=alpha, evs=evs, plan=plan)


def fresh(D, leg, T, monkeypatch, strict, flow="deferred", env=None, devices=None):
    """Leg B alone on a new engine (once per distinct leg)."""
    key = (D.name, leg, T, strict, flow, tuple(sorted((env or {}).items())), tuple(devices or ()))
    if key not in _FRESH:
        e = load(Engine(strict=strict, devices=devices), D, monkeypatch)
        _FRESH[key] = run_leg(e, D, leg, T, monkeypatch, flow=flow, dirty=None, env=env)
        e.close()
    return _FRESH[key]


def check_evs(evs, revs, strict, tol=REL):
    assert len(evs) == len(revs)
    for t, (ev, rv) in enumerate(zip(evs, revs), 1):
        if strict:
            assert float(ev["primal"]).hex() == float(rv["primal"]).hex(), (t, ev["primal"], rv["primal"])
            assert float(ev["gap"]).hex() == float(rv["gap"]).hex(), (t, ev["gap"], rv["gap"])
        else:
            P = abs(rv["primal"])
            assert abs(ev["primal"] - rv["primal"]) <= tol * P, (t, ev["primal"], rv["primal"])
            assert abs(ev["gap"] - rv["gap"]) <= tol * P, (t, ev["gap"], rv["gap"])
        assert ev["test_err_count"] == (rv["test_err"] if "test_err" in rv else rv["test_err_count"]), t


def check(res, D, leg, T, strict, fr=None):
    """res against the oracle's leg, and against the fresh engine's (fr)."""
    r = ref(D, leg, T)
    wr = r["w"]
    wmax = np.max(np.abs(wr))
    if strict:
        assert np.array_equal(res["w"], wr) and np.array_equal(res["alpha"], r["alpha"]), leg
    else:
        assert np.max(np.abs(res["w"] - wr)) <= REL * wmax, (leg, np.max(np.abs(res["w"] - wr)) / wmax)
        assert np.max(np.abs(res["alpha"] - r["alpha"])) <= REL, leg
    check_evs(res["evs"], r["evs"], strict)
    if fr is not None:
        if strict:
            assert np.array_equal(res["w"], fr["w"]) and np.array_equal(res["alpha"], fr["alpha"]), leg
        else:
            assert np.max(np.abs(res["w"] - fr["w"])) <= SAME * wmax, (leg, np.max(np.abs(res["w"] - fr["w"])) / wmax)
            assert np.max(np.abs(res["alpha"] - fr["alpha"])) <= SAME, leg
        assert {k: res["plan"][k] for k in FLAGS} == {k: fr["plan"][k] for k in FLAGS}, leg


def expect_plan(plan, leg, strict, D=None):
    """The path flags a leg on sparse rows with dense deltaW slices (C2, the edge
    rows) must show: a run that fell back to a simpler path fails here."""
    m = leg.method
    gram = not strict and m != "mbsgd" and leg.solver in ("auto", "gram")
    want = {"solver": "gram" if gram else "chain",
            "gram_mirror": 1 if gram and leg.H > 48 else 0,
            "xw_producer": 1 if gram and m != "mbcd" else 0,
            "mbsgd_pull": 1 if m == "mbsgd" and not strict else 0,
            "dw_compact": 0, "dw_dbuf": 0}
    if D is not None and D.name == "c2":
        want["eval_split"] = want["eval_test_split"] = 0 if strict else 1
    got = {k: plan[k] for k in want}
    assert got == want, (leg, got, want)


def _dirt(i, strict):
    """How leg i ends and evaluates: both flows and both uncollected kinds in turn."""
    if strict:  # (the pipelined evaluation is fast mode's)
        return "deferred", "begin"
    return ("deferred", "async")[i % 2], ("begin", "async")[(i // 2 + i) % 2]


# 1 ---------------------------------------------------------------- driver order
@pytest.mark.parametrize("strict", [True, False])
def test_driver_order_on_one_engine(c2, strict, monkeypatch):
    """hingeDriver.scala:84-109: CoCoA+, CoCoA, MbCD, mb-SGD, local SGD one after
    another on one context, every leg left dirty; every collected evaluation
    and every leg's final state is the oracle's and a fresh engine's."""
    e = load(Engine(strict=strict), c2, monkeypatch)
    for i, m in enumerate(ORDER):
        leg = Leg(m)
        _, dirty = _dirt(i, strict)
        res = run_leg(e, c2, leg, 4, monkeypatch, flow="deferred", dirty=dirty)
        expect_plan(res["plan"], leg, strict, c2)
        check(res, c2, leg, 4, strict, fresh(c2, leg, 4, monkeypatch, strict))


# 2 ------------------------------------------------------------------ pair matrix
def _leg_b(a, b):
    return Leg(b) if a != b else Leg(b, H=177, lam=1e-3, gamma=0.5, seed=9)


@pytest.mark.parametrize("a,b", [(a, b) for a in ORDER for b in ORDER])
def test_every_ordered_pair_of_legs(c2, a, b, monkeypatch):
    """20 pairs of distinct methods and 5 same-method pairs whose second leg
    changes H (200 -> 177), seed, lambda and gamma (1.0 -> 0.5)."""
    i = ORDER.index(a) * 5 + ORDER.index(b)
    flow, dirty = _dirt(i, False)
    e = load(Engine(strict=False), c2, monkeypatch)
    la, lb = Leg(a), _leg_b(a, b)
    ra = run_leg(e, c2, la, 3, monkeypatch, flow=flow, dirty=dirty)
    expect_plan(ra["plan"], la, False, c2)
    res = run_leg(e, c2, lb, 3, monkeypatch)
    expect_plan(res["plan"], lb, False, c2)
    check(res, c2, lb, 3, False, fresh(c2, lb, 3, monkeypatch, False))


@pytest.mark.parametrize("method", ["cocoa+", "cocoa", "localsgd"])
def test_prefetch_of_the_last_leg_is_not_taken_for_the_same_round_number(c2, method, monkeypatch):
    """The Gram prefetch is keyed on the round number alone.  Leg A stops with
    round 3's rows (its seed's samples) prefetched; leg B, another seed, runs
    through round 3 and must form its own."""
    e = load(Engine(strict=False), c2, monkeypatch)
    la, lb = Leg(method, seed=11), Leg(method, seed=5)
    run_leg(e, c2, la, 1, monkeypatch, flow="async", dirty="async")
    res = run_leg(e, c2, lb, 4, monkeypatch)
    expect_plan(res["plan"], lb, False, c2)
    check(res, c2, lb, 4, False, fresh(c2, lb, 4, monkeypatch, False))


# 3 -------------------------------------------------------- H across the window
@pytest.mark.parametrize("method", ["cocoa+", "mbcd", "localsgd"])
def test_h_across_the_mirror_window_on_one_engine(c2, method, monkeypatch):
    """The mirrored solver takes only H > 48 (more than kGNB = 3 batches): nbatch,
    and with it xbase, xw_flag, gt and the plan buffers, shrink and grow."""
    e = load(Engine(strict=False), c2, monkeypatch)
    mirror = []
    for i, H in enumerate([200, 40, 49, 48, 193]):
        leg = Leg(method, H=H)
        flow, dirty = _dirt(i, False)
        res = run_leg(e, c2, leg, 2, monkeypatch, flow=flow, dirty=dirty)
        mirror.append(res["plan"]["gram_mirror"])
        expect_plan(res["plan"], leg, False, c2)
        check(res, c2, leg, 2, False)
    assert mirror == [1, 0, 1, 0, 1]


# 4 ------------------------------------------------------ the benchmark's sequence
def _steps(e, t, count, flow, stop=None):
    """bench.py steps(): count rounds from t, each evaluated behind the next."""
    begin, end = (e.eval_async, e.eval_wait) if flow == "async" else (e.eval_begin, e.eval_end)
    evs, rounds, pending = [], [], None
    for _ in range(count):
        e.round(t)
        if pending is not None:
            evs.append(end())
            rounds.append(pending)
            pending = None
            if stop and stop(evs[-1]["gap"]):
                return evs, rounds
        begin()
        pending = t
        t += 1
    if pending is not None:
        evs.append(end())
        rounds.append(pending)
    return evs, rounds


@pytest.fixture(scope="module")
def gap_target(c2):
    """From the oracle alone: the first round R >= 8 whose gap drops by more
    than 1e-6 |P_R|, and the target half-way down that drop -- the 1e-9
    tolerance cannot move the round at which gap <= target first holds."""
    leg = Leg("cocoa+", lam=1e-3, seed=0)
    r = ref(c2, leg, 30)
    g = [ev["gap"] for ev in r["evs"]]  # g[t - 1]: after round t
    P = [abs(ev["primal"]) for ev in r["evs"]]
    R = next((t for t in range(8, 31) if g[t - 2] - g[t - 1] > 1e-6 * P[t - 1]), None)
    assert R is not None and R <= 30
    target = (g[R - 2] + g[R - 1]) / 2
    assert all(g[t - 1] - target > 1e-6 * P[t - 1] / 4 for t in range(1, R))  # no earlier round within tolerance of it
    return leg, R, target


@pytest.mark.parametrize("flow", ["deferred", "async"])
def test_benchmark_sequence_reinit_reaches_the_gap_at_the_oracles_round(c2, gap_target, flow, monkeypatch):
    """bench.py: init, the timed rounds, five bare evaluations, init again with
    the same arguments, then rounds until gap <= target (flow async: --pipeline)."""
    leg, R, target = gap_target
    r = ref(c2, leg, 30)
    args = ("cocoa+", c2.tr.n, BIG, leg.H, leg.lam, 1.0, 1.0, 1, leg.seed)
    e = load(Engine(strict=False), c2, monkeypatch)
    e.init(*args)
    expect_plan(e.plan(), leg, False, c2)
    evs, rounds = _steps(e, 1, 12, flow)
    assert rounds == list(range(1, 13))
    check_evs(evs, r["evs"][:12], False)
    for _ in range(5):
        check_evs([e.eval()], r["evs"][11:12], False)
    e.init(*args)
    expect_plan(e.plan(), leg, False, c2)
    evs, rounds = _steps(e, 1, 30, flow, stop=lambda g: g <= target)
    assert rounds == list(range(1, R + 1)), (rounds, R)
    check_evs(evs, r["evs"][:R], False)
    f = load(Engine(strict=False), c2, monkeypatch)
    f.init(*args)
    fevs, frounds = _steps(f, 1, 30, flow, stop=lambda g: g <= target)
    assert frounds == rounds
    check_evs(evs, fevs, False, tol=SAME)


# 5 --------------------------------------------------------------- solver switches
def test_solver_switches_on_one_engine(c2, monkeypatch):
    """cocoa_set_solver takes effect at the next cocoa_init, and revokes the
    current one: cocoa_round before that init is a state error."""
    e = load(Engine(strict=False), c2, monkeypatch)
    seq = [("gram", "cocoa+"), ("chain", "cocoa+"), ("auto", "mbcd"), ("gram", "localsgd")]
    for i, (solver, m) in enumerate(seq):
        leg = Leg(m, solver=solver)
        e.set_solver(solver)
        e._solver = solver
        with pytest.raises(cocoa_amd.CocoaError) as ei:
            e.round(1)
        assert ei.value.code == E_STATE
        # (the first leg ends with an evaluation snapshotted and never enqueued, the next begun, ...)
        res = run_leg(e, c2, leg, 3, monkeypatch, flow=("async", "deferred")[i % 2], dirty=("async", "begin")[i % 2])
        expect_plan(res["plan"], leg, False, c2)
        check(res, c2, leg, 3, False, fresh(c2, leg, 3, monkeypatch, False, flow=("async", "deferred")[i % 2]))


# 6 ------------------------------------------------- state setters on a used engine
@pytest.mark.parametrize("solver", ["gram", "chain"])
def test_set_state_on_a_used_engine_then_reinit(c2, solver, monkeypatch):
    """(a) cocoa_set_w / cocoa_set_alpha (alpha partly outside [0, 1]) after a
    round and an evaluation whose x.w is cached: the next rounds start from the
    new state under the reference's skip rule (CoCoA.scala:166-172).
    (b) the init after it starts clean (the projection rule off again)."""
    leg = Leg("cocoa+", solver=solver)
    rng = np.random.default_rng(3)
    a0 = rng.uniform(-0.5, 1.5, c2.tr.n)
    a0[::7] = 0.0
    a0[3::7] = 1.0
    w0 = rng.standard_normal(c2.tr.num_features) * 1e-2
    e = load(Engine(strict=False), c2, monkeypatch)
    e.set_solver(solver)
    e._solver = solver
    e.init("cocoa+", c2.tr.n, BIG, leg.H, leg.lam, 1.0, 1.0, 1, leg.seed)
    expect_plan(e.plan(), leg, False, c2)
    e.round(1)
    e.eval()
    e.set_w(w0)
    e.set_alpha(a0)
    run = oracle.Run(c2.od, "cocoa+", c2.tr.n, leg.H, leg.lam, 1.0, 1.0, seed=leg.seed, nthreads=8)
    run.set_state(w0, a0)
    for t in (2, 3):
        e.round(t)
        run.round(t)
    wr = run.w()
    assert np.max(np.abs(e.w() - wr)) <= REL * np.max(np.abs(wr))
    assert np.max(np.abs(e.alpha() - run.alpha())) <= REL
    check_evs([e.eval()], [run.eval(c2.ot)], False)
    res = run_leg(e, c2, leg, 3, monkeypatch)
    expect_plan(res["plan"], leg, False, c2)
    check(res, c2, leg, 3, False, fresh(c2, leg, 3, monkeypatch, False))


@pytest.mark.parametrize("strict", [True, False])
def test_checkpoint_loaded_into_a_used_engine(c2, strict, tmp_path, monkeypatch):
    """(c) A round-3 checkpoint of a CoCoA+ leg, loaded after the engine has run
    an mb-SGD and a CoCoA leg: rounds 4-6 land on the uninterrupted run."""
    leg = Leg("cocoa+")
    path = str(tmp_path / "leg.ck")
    e = load(Engine(strict=strict), c2, monkeypatch)
    e.init("cocoa+", c2.tr.n, BIG, leg.H, leg.lam, 1.0, 1.0, 1, leg.seed)
    for t in range(1, 7):
        e.round(t)
        if t == 3:
            e.save_checkpoint(path, t)
    whole = dict(w=e.w(), alpha=e.alpha())
    for i, m in enumerate(["mbsgd", "cocoa"]):
        res = run_leg(e, c2, Leg(m), 2, monkeypatch, dirty=_dirt(i + 1, strict)[1])
        check(res, c2, Leg(m), 2, strict)
    e.init("cocoa+", c2.tr.n, BIG, leg.H, leg.lam, 1.0, 1.0, 1, leg.seed)
    expect_plan(e.plan(), leg, strict, c2)
    assert e.load_checkpoint(path) == 3
    for t in range(4, 7):
        e.round(t)
    got = dict(w=e.w(), alpha=e.alpha(), evs=[e.eval()], plan=e.plan())
    r = ref(c2, leg, 6)
    wmax = np.max(np.abs(r["w"]))
    if strict:
        for k in ("w", "alpha"):
            assert np.array_equal(got[k], whole[k]) and np.array_equal(got[k], r[k])
    else:
        assert np.max(np.abs(got["w"] - r["w"])) <= REL * wmax
        assert np.max(np.abs(got["alpha"] - r["alpha"])) <= REL
        assert np.max(np.abs(got["w"] - whole["w"])) <= SAME * wmax
        assert np.max(np.abs(got["alpha"] - whole["alpha"])) <= SAME
    check_evs(got["evs"], r["evs"][5:6], strict)


@pytest.mark.parametrize("strict", [True, False])
def test_unit_calls_between_rounds_leave_the_run_alone(c2, strict, monkeypatch):
    """(d) cocoa_local_sdca, cocoa_samples and cocoa_debug_gram_rows between
    rounds 2 and 3: the trajectory is the one of a twin that made no such call."""
    leg = Leg("cocoa+")
    twins = []
    for poke in (False, True):
        e = load(Engine(strict=strict), c2, monkeypatch)
        e.init("cocoa+", c2.tr.n, BIG, leg.H, leg.lam, 1.0, 1.0, 1, leg.seed)
        expect_plan(e.plan(), leg, strict, c2)
        evs = []
        for t in range(1, 5):
            e.round(t)
            evs.append(e.eval())
            if poke and t == 2:
                part = 3
                nl = int(c2.tr.part_ptr[part + 1] - c2.tr.part_ptr[part])
                da, dw = e.local_sdca(part, np.zeros(c2.tr.num_features), 120, 1e-3, c2.tr.n, np.zeros(nl), 11, True,
                                      16.0)
                assert np.any(da != 0) and np.any(dw != 0)
                assert np.array_equal(e.samples(part, leg.seed + 3, 64), oracle.samples(leg.seed + 3, nl, 64))
                if not strict:
                    assert e.gram_rows(3).shape == (16, 13 * 16, 48)
        twins.append(dict(w=e.w(), alpha=e.alpha(), evs=evs))
    a, b = twins
    wmax = np.max(np.abs(a["w"]))
    if strict:
        assert np.array_equal(a["w"], b["w"]) and np.array_equal(a["alpha"], b["alpha"])
    else:
        assert np.max(np.abs(a["w"] - b["w"])) <= SAME * wmax
        assert np.max(np.abs(a["alpha"] - b["alpha"])) <= SAME
    check_evs(b["evs"], a["evs"], strict, tol=SAME)
    check(dict(b, plan=None), c2, leg, 4, strict)


@pytest.mark.parametrize("strict", [True, False])
def test_cocoa_run_on_a_used_engine_equals_a_fresh_one(c2, strict, monkeypatch):
    """(e) cocoa_run (init + rounds + evaluations in one call) after a manual leg."""
    leg = Leg("cocoa+")
    out = []
    for used in (False, True):
        e = load(Engine(strict=strict), c2, monkeypatch)
        if used:
            run_leg(e, c2, Leg("mbsgd"), 2, monkeypatch, dirty=_dirt(1, strict)[1])
        evs = []
        e.run("cocoa+", c2.tr.n, 4, leg.H, leg.lam, 1.0, 1.0, debug_iter=1, seed=leg.seed,
              callback=lambda t, ev: evs.append(ev))
        expect_plan(e.plan(), leg, strict, c2)
        out.append(dict(w=e.w(), alpha=e.alpha(), evs=evs, plan=e.plan()))
    check(out[1], c2, leg, 4, strict, out[0])
    check_evs(out[1]["evs"], out[0]["evs"], strict, tol=SAME)


# 7 --------------------------------------------------------------- data replacement
def _expect_data_plan(plan, D, leg, strict):
    if D.name in ("c2", "edge"):
        return expect_plan(plan, leg, strict, D)
    if strict:
        want = {"solver": "chain", "gram_mirror": 0, "xw_producer": 0, "mbsgd_pull": 0, "eval_split": 0}
        want["dw_compact"] = 1 if D.name == "c4" and leg.method == "cocoa+" else 0
    elif D.name == "c4":  # compact slices (CoCoA+), double-buffered; mb-SGD on the dense ones, by the pull
        cp = leg.method == "cocoa+"
        want = {"solver": "gram" if cp else "chain", "gram_mirror": 0, "dw_compact": 1 if cp else 0,
                "dw_dbuf": 1 if cp else 0, "mbsgd_pull": 0 if cp else 1}
    else:  # dense rows: the dense solver; no CSR for the pull
        want = {"solver": "dense" if leg.method == "cocoa+" else "chain", "gram_mirror": 0, "xw_producer": 0,
                "mbsgd_pull": 0, "dw_compact": 0}
    got = {k: plan[k] for k in want}
    assert got == want, (D.name, leg, got, want)


_H = {"c2": 200, "edge": 150, "c4": 1000, "dense": 100}


@pytest.mark.parametrize("strict", [True, False])
def test_train_set_replaced_on_a_used_engine(strict, monkeypatch):
    """cocoa_set_train on a context that has run: another n, d, K and layout
    (CSR with dense slices, CSR with compact slices, dense rows) each time, and
    back.  The old test set is dropped with the old rows; the CSC copy of the
    mb-SGD pull is rebuilt."""
    e = Engine(strict=strict)
    for i, name in enumerate(["c2", "edge", "c4", "dense", "c2"]):
        D = data(name)
        H = _H[name]
        lp, ls = Leg("cocoa+", H=H, gamma=0.5), Leg("mbsgd", H=H)
        load(e, D, monkeypatch, test=False)
        f = load(Engine(strict=strict), D, monkeypatch, test=False)
        got = []
        for x in (e, f):  # no test rows until cocoa_set_test: the fresh engine's test fields
            x.init("cocoa+", D.tr.n, BIG, H, lp.lam, 1.0, 0.5, 1, lp.seed)
            got.append(x.eval())
        f.close()
        for k in ("test_err_count", "test_rows"):
            assert got[0][k] == got[1][k] == 0
        assert math.isnan(got[0]["test_error"]) and math.isnan(got[1]["test_error"])
        assert got[0]["primal"].hex() == got[1]["primal"].hex()
        e.set_test(D.te)
        for j, leg in enumerate((lp, ls)):
            flow, dirty = _dirt(i + j, strict)
            res = run_leg(e, D, leg, 3, monkeypatch, flow=flow, dirty=dirty)
            _expect_data_plan(res["plan"], D, leg, strict)
            check(res, D, leg, 3, strict, fresh(D, leg, 3, monkeypatch, strict, flow=flow))


@pytest.mark.parametrize("strict", [True, False])
def test_test_set_replaced_between_rounds(c2, strict, monkeypatch):
    """cocoa_set_test alone on an initialised context, an evaluation pending:
    smaller, larger, all rows empty, and whole in the cold pass
    (COCOA_EVAL_TEST_SPLIT=0); error counts exact, eval_test_split follows."""
    leg = Leg("cocoa+")
    te = c2.te
    empty = LabeledData(np.zeros(301, np.int64), np.zeros(0, np.int32), np.zeros(0), te.y[:300].copy(),
                        np.array([0, 300], np.int64), te.num_features)
    sets = [(te.row_range(100, 500), {}, 1), (te.row_range(0, 90), {}, 1), (te, {}, 1), (empty, {}, None),
            (te.row_range(300, 1000), {"COCOA_EVAL_TEST_SPLIT": "0"}, 0), (te.row_range(0, 700), {}, 1)]
    e = load(Engine(strict=strict), c2, monkeypatch, test=False)
    e.init("cocoa+", c2.tr.n, BIG, leg.H, leg.lam, 1.0, 1.0, 1, leg.seed)
    run = oracle.Run(c2.od, "cocoa+", c2.tr.n, leg.H, leg.lam, 1.0, 1.0, seed=leg.seed, nthreads=8)
    for t, (ts, env, split) in enumerate(sets, 1):
        e.round(t)
        run.round(t)
        e.eval_begin()  # (reads the test rows about to be replaced; dropped by cocoa_set_test)
        with _env(monkeypatch, env):
            e.set_test(ts)
        ev = e.eval()
        check_evs([ev], [run.eval(odata(ts))], strict)
        assert ev["test_rows"] == ts.n
        if split is not None:
            assert e.plan()["eval_test_split"] == (0 if strict else split), t
        else:
            f = load(Engine(strict=strict), c2, monkeypatch, test=False)
            f.set_test(ts)
            f.init("cocoa+", c2.tr.n, 1, leg.H, leg.lam)
            assert e.plan()["eval_test_split"] == f.plan()["eval_test_split"]
            f.close()
    expect_plan(e.plan(), leg, strict)
    wr = run.w()
    if strict:
        assert np.array_equal(e.w(), wr) and np.array_equal(e.alpha(), run.alpha())
    else:
        assert np.max(np.abs(e.w() - wr)) <= REL * np.max(np.abs(wr))
        assert np.max(np.abs(e.alpha() - run.alpha())) <= REL


# 8 -------------------------------------------------------- mb-SGD pull / scatter
@pytest.mark.parametrize("name", ["c2", "edge"])
def test_mbsgd_pull_and_scatter_toggled_across_inits(name, monkeypatch):
    """The pull leaves the round's sum in slice 0 and folds that slice alone; the
    scatter and the SDCA solvers use every slice.  Pull, scatter
    (COCOA_MBSGD_PULL=0 at that init), pull, CoCoA, pull on one engine."""
    D = data(name)
    H = 300 if name == "edge" else 200
    e = load(Engine(strict=False), D, monkeypatch)
    seq = [("mbsgd", 1), ("mbsgd", 0), ("mbsgd", 1), ("cocoa", None), ("mbsgd", 1)]
    for i, (m, pull) in enumerate(seq):
        leg = Leg(m, H=H, seed=3 + i)
        flow, dirty = _dirt(i, False)
        env = {"COCOA_MBSGD_PULL": "0"} if pull == 0 else None
        res = run_leg(e, D, leg, 3, monkeypatch, flow=flow, dirty=dirty, env=env)
        if pull is not None:
            assert res["plan"]["mbsgd_pull"] == pull and res["plan"]["solver"] == "chain"
        else:
            expect_plan(res["plan"], leg, False, D)
        check(res, D, leg, 3, False)


# 9 ----------------------------------------------------------- multi-member context
@pytest.mark.parametrize("strict", [True, False])
def test_multi_member_context_driver_order(c2, strict, monkeypatch):
    """cocoa_create_multi over [0, 0] (group_init's own reset): the driver's five
    methods on one context, every leg ending with an uncollected evaluation."""
    e = load(Engine(strict=strict, devices=[0, 0]), c2, monkeypatch)
    for m in ORDER:
        leg = Leg(m)
        res = run_leg(e, c2, leg, 2, monkeypatch)
        assert res["plan"]["gram_mirror"] == 0 and res["plan"]["n_devices"] == 2
        assert res["plan"]["solver"] == ("chain" if strict or m == "mbsgd" else "gram")
        check(res, c2, leg, 2, strict, fresh(c2, leg, 2, monkeypatch, strict, devices=[0, 0]))


# 10 ------------------------------------------------------------- two HOST ranks
_RANK_LEGS = [("cocoa+", None), ("mbsgd", "1"), ("mbsgd", "0"), ("cocoa+", None)]


def _rank_worker(rank, world, uid_q, out_q):
    try:
        D = data("c2")
        tr, te = D.tr, D.te
        k0, k1 = shard_bounds(tr.num_parts, world, rank)
        r0, r1 = shard_bounds(te.n, world, rank)
        if rank == 0:
            uid = comm_unique_id("host")
            for _ in range(world - 1):
                uid_q.put(uid)
        else:
            uid = uid_q.get(timeout=60)
        e = Engine(device=0, strict=False)
        e.set_train(tr.shard(k0, k1), part_begin=k0, num_parts_global=tr.num_parts)
        e.set_test(te.row_range(r0, r1))
        e.comm_init("host", rank, world, uid)
        out = []
        for i, (m, pull) in enumerate(_RANK_LEGS):
            if pull is not None:
                os.environ["COCOA_MBSGD_PULL"] = pull
            e.init(m, tr.n, BIG, 200, 2e-3, 1.0, 1.0, 1, 5 + i)
            os.environ.pop("COCOA_MBSGD_PULL", None)
            plan = e.plan()
            for t in (1, 2, 3):
                e.round(t)
            ev, w = e.eval(), e.w()
            e.round(4)
            e.eval_begin()  # left for the next init to drop (both ranks: its sums are exchanged)
            out.append((w, ev, {k: plan[k] for k in FLAGS}))
        out_q.put((rank, out))
    except Exception as ex:  # noqa: BLE001
        out_q.put((rank, repr(ex)))


def test_two_host_ranks_reuse_their_engines(c2):
    """Two processes over the HOST transport, each rank's one engine through
    CoCoA+, mb-SGD by the pull, mb-SGD by the scatter, CoCoA+: w byte-identical
    on the ranks and the single-process oracle's within tolerance."""
    world = 2
    ctx = mp.get_context("spawn")
    uid_q, out_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, uid_q, out_q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        out = dict(out_q.get(timeout=150) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert not isinstance(out[r], str), out[r]
    for i, (m, pull) in enumerate(_RANK_LEGS):
        leg = Leg(m, seed=5 + i)
        rf = ref(c2, leg, 3)
        (w0, ev0, p0), (w1, ev1, p1) = out[0][i], out[1][i]
        for p in (p0, p1):
            assert p["solver"] == ("gram" if m == "cocoa+" else "chain")
            assert p["mbsgd_pull"] == (int(pull) if pull is not None else 0)
        assert w0.tobytes() == w1.tobytes(), leg
        assert np.max(np.abs(w0 - rf["w"])) <= REL * np.max(np.abs(rf["w"])), leg
        for ev in (ev0, ev1):
            check_evs([ev], rf["evs"][2:3], False)
