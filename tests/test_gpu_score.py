"""Scoring on the GPU (cocoa_score*, Engine.decision_function / predict):
decision values f_r = sum_q val[q] * w[col[q]] of caller rows.

Reference: a Python float loop per row in stored order (product, then add).
Strict mode must equal it bitwise; fast mode within
REL * sum_q |val[q] * w[col[q]]| per row (REL = 1e-9, tests/test_gpu_parity.py),
and two identical fast calls must return identical bytes."""
import ctypes
import os

import numpy as np
import pytest

import cocoa_amd
from cocoa_amd import Engine
from cocoa_amd import _capi as C
from cocoa_amd.data import LabeledData

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
TRAIN = os.path.join(G, "data", "small_train.dat")
TEST = os.path.join(G, "data", "small_test.dat")
REL = 1e-9

# row lengths that bracket any plausible tile size; empty rows first, last and
# two in a row in the middle
LADDER = [0, 1, 15, 16, 17, 63, 64, 65, 0, 0, 2047, 2048, 2049, 4095, 4096, 4097, 8193, 20000, 0]


def ref_scores(row_ptr, col, val, w):
    """(f, sum |val * w|) per row by a plain float loop in stored order."""
    wl, cl, vl, rp = w.tolist(), col.tolist(), val.tolist(), row_ptr.tolist()
    f, a = [], []
    for r in range(len(rp) - 1):
        s, t = 0.0, 0.0
        for q in range(rp[r], rp[r + 1]):
            p = vl[q] * wl[cl[q]]
            s = s + p
            t = t + abs(p)
        f.append(s)
        a.append(t)
    return np.array(f, np.float64), np.array(a, np.float64)


def make_w(d, seed):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(d)
    w[w == 0.0] = 1.0
    return w


def make_csr(lens, d, seed):
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if d == 1:
        col = np.zeros(int(rp[-1]), np.int32)
    else:
        col = np.concatenate([rng.choice(d, n, replace=False) if d <= 100000 else rng.integers(0, d, n)
                              for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = rng.standard_normal(int(rp[-1]))
    n = len(lens)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    return LabeledData(rp, col, val, y, np.array([0, n], np.int64), d)


class Case:
    def __init__(self, lens, d, seed):
        self.data = make_csr(lens, d, seed)
        self.w = make_w(d, seed + 1000)
        self.f, self.a = ref_scores(self.data.row_ptr, self.data.col, self.data.val, self.w)


@pytest.fixture(scope="module")
def ladder():
    return Case(LADDER, 20011, 11)


@pytest.fixture(scope="module")
def ladder_d1():
    return Case(LADDER, 1, 12)


@pytest.fixture(scope="module")
def engines():
    return {True: Engine(strict=True), False: Engine(strict=False)}


def check(got, case, strict):
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == case.f.shape
    if strict:
        assert np.array_equal(got.view(np.uint64), case.f.view(np.uint64))
    else:
        err = np.abs(got - case.f)
        print("fast: max |f - f_ref| / sum|val w| = %r" % float(np.max(err / np.maximum(case.a, 1e-300), initial=0.0)))
        assert np.all(err <= REL * case.a)


# ------------------------------------------------------------- host rows --
@pytest.mark.parametrize("strict", [True, False])
def test_row_length_ladder(engines, ladder, strict):
    e = engines[strict]
    got = e.decision_function(ladder.data, ladder.w)
    check(got, ladder, strict)
    again = e.decision_function(ladder.data, ladder.w)
    assert got.tobytes() == again.tobytes()
    assert np.array_equal(e.predict(ladder.data, ladder.w), np.where(got > 0, 1.0, -1.0))


@pytest.mark.parametrize("strict", [True, False])
def test_ladder_with_one_feature(engines, ladder_d1, strict):
    check(engines[strict].decision_function(ladder_d1.data, ladder_d1.w), ladder_d1, strict)


@pytest.mark.parametrize("strict", [True, False])
def test_no_rows_and_all_rows_empty(engines, strict):
    e = engines[strict]
    w = make_w(7, 1)
    none = LabeledData(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0),
                       np.array([0, 0], np.int64), 7)
    assert e.decision_function(none, w).shape == (0,)
    assert e.decision_function(np.zeros((0, 7)), w).shape == (0,)
    empty = LabeledData(np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0), np.ones(5),
                        np.array([0, 5], np.int64), 7)
    got = e.decision_function(empty, w)
    assert got.tobytes() == np.zeros(5).tobytes()
    assert np.array_equal(e.predict(empty, w), -np.ones(5))


@pytest.mark.parametrize("strict", [True, False])
def test_three_million_features(engines, strict):
    # int32 columns up to d - 1, w (24 MB) beyond L2
    rng = np.random.default_rng(3)
    d = 3_000_000
    lens = rng.integers(1, 40, 50).tolist()
    case = Case(lens, d, 5)
    case.data.col[-1] = d - 1
    case.data.col[0] = 0
    case.f, case.a = ref_scores(case.data.row_ptr, case.data.col, case.data.val, case.w)
    check(engines[strict].decision_function(case.data, case.w), case, strict)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("n", [1, 130])
@pytest.mark.parametrize("d", [1, 3, 64, 4097])
def test_dense_rows(engines, strict, n, d):
    rng = np.random.default_rng(100 * d + n)
    X = rng.standard_normal((n, d))
    w = make_w(d, d)
    rp = np.arange(n + 1, dtype=np.int64) * d
    col = np.tile(np.arange(d, dtype=np.int32), n)
    f, a = ref_scores(rp, col, X.reshape(-1), w)
    got = engines[strict].decision_function(X, w)
    if strict:
        assert np.array_equal(got.view(np.uint64), f.view(np.uint64))
    else:
        assert np.all(np.abs(got - f) <= REL * a)
        assert got.tobytes() == engines[strict].decision_function(X, w).tobytes()


@pytest.mark.parametrize("strict", [True, False])
def test_chunked_upload(ladder, strict):
    # 64-entry chunks: the 20000-entry row (and every row longer than 64) is a chunk of its own
    e = Engine(strict=strict)
    e.score_set_chunk(64)
    check(e.decision_function(ladder.data, ladder.w), ladder, strict)
    e.score_set_chunk(0)
    check(e.decision_function(ladder.data, ladder.w), ladder, strict)
    X = np.random.default_rng(4).standard_normal((130, 9))
    w = make_w(9, 9)
    one = e.decision_function(X, w)
    e.score_set_chunk(64)  # 7 dense rows per chunk
    many = e.decision_function(X, w)
    assert many.tobytes() == one.tobytes()


def test_host_argument_errors(engines, ladder):
    e = engines[True]
    d = ladder.data
    bad = LabeledData(d.row_ptr, d.col.copy(), d.val, d.y, d.part_ptr, d.num_features)
    bad.col[5] = d.num_features
    with pytest.raises(cocoa_amd.IndexOutOfBoundsError):
        e.decision_function(bad, ladder.w)
    bad.col[5] = -1
    with pytest.raises(cocoa_amd.IndexOutOfBoundsError):
        e.decision_function(bad, ladder.w)
    rp = d.row_ptr.copy()
    rp[3] = rp[4] + 1
    with pytest.raises(cocoa_amd.IllegalArgumentError):
        e.decision_function(LabeledData(rp, d.col, d.val, d.y, d.part_ptr, d.num_features), ladder.w)
    rp = d.row_ptr.copy()
    rp[0] = 1
    with pytest.raises(cocoa_amd.IllegalArgumentError):
        e.decision_function(LabeledData(rp, d.col, d.val, d.y, d.part_ptr, d.num_features), ladder.w)
    with pytest.raises(cocoa_amd.IllegalArgumentError):
        e.decision_function(d, ladder.w[:-1])


# ----------------------------------------------------------- device rows --
def score_device(e, w_t, crow, col, val, n, d):
    import torch
    out = torch.empty(n, dtype=torch.float64, device=crow.device)
    torch.cuda.synchronize()
    C.check(C.lib().cocoa_score_device(e.h, ctypes.c_void_p(w_t.data_ptr()), ctypes.c_void_p(crow.data_ptr()),
                                       ctypes.c_void_p(col.data_ptr()), ctypes.c_void_p(val.data_ptr()), n,
                                       int(val.shape[0]), d, ctypes.c_void_p(out.data_ptr())), e.h)
    e.sync()
    return out


@pytest.mark.parametrize("strict", [True, False])
def test_device_csr_matches_host(engines, ladder, strict):
    import torch
    e = engines[strict]
    dat = ladder.data
    n, d = dat.n, dat.num_features
    host = e.decision_function(dat, ladder.w)
    dev = torch.device("cuda", 0)
    crow = torch.from_numpy(dat.row_ptr).to(dev)
    col64 = torch.from_numpy(dat.col.astype(np.int64)).to(dev)
    val = torch.from_numpy(dat.val).to(dev)
    # torch CSR with int64 column indices (converted to int32 on the device), numpy w and torch w
    X = torch.sparse_csr_tensor(crow, col64, val, size=(n, d))
    for w in (ladder.w, torch.from_numpy(ladder.w).to(dev)):
        got = e.decision_function(X, w)
        assert isinstance(got, torch.Tensor) and got.device == X.device and got.dtype == torch.float64
        check(got.cpu().numpy(), ladder, strict)
        if strict:
            assert got.cpu().numpy().tobytes() == host.tobytes()
    pred = e.predict(X, ladder.w)
    assert pred.device == X.device
    assert np.array_equal(pred.cpu().numpy(), np.where(got.cpu().numpy() > 0, 1.0, -1.0))
    # col / val views that start at odd element offsets into larger tensors
    # (12 and 8 bytes past a 16-byte boundary)
    nnz = dat.nnz
    colbuf = torch.zeros(nnz + 8, dtype=torch.int32, device=dev)
    valbuf = torch.zeros(nnz + 8, dtype=torch.float64, device=dev)
    rpbuf = torch.zeros(n + 1 + 8, dtype=torch.int64, device=dev)
    wbuf = torch.zeros(d + 8, dtype=torch.float64, device=dev)
    colv, valv, rpv, wv = colbuf[3:3 + nnz], valbuf[1:1 + nnz], rpbuf[1:n + 2], wbuf[1:d + 1]
    colv.copy_(torch.from_numpy(dat.col))
    valv.copy_(val)
    rpv.copy_(crow)
    wv.copy_(torch.from_numpy(ladder.w))
    assert colv.data_ptr() % 16 == 12 and valv.data_ptr() % 16 == 8
    odd = score_device(e, wv, rpv, colv, valv, n, d)
    check(odd.cpu().numpy(), ladder, strict)
    odd2 = score_device(e, wv, rpv, colv, valv, n, d)
    assert odd.cpu().numpy().tobytes() == odd2.cpu().numpy().tobytes()


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("d", [3, 4097])
def test_device_dense_matches_host(engines, strict, d):
    import torch
    e = engines[strict]
    n = 130
    X = np.random.default_rng(d).standard_normal((n, d))
    w = make_w(d, d + 1)
    host = e.decision_function(X, w)
    big = torch.zeros(n * d + 3, dtype=torch.float64, device="cuda")
    Xt = big[1:1 + n * d].view(n, d)  # starts 8 bytes past a 16-byte boundary
    Xt.copy_(torch.from_numpy(X))
    got = e.decision_function(Xt, torch.from_numpy(w).to("cuda"))
    assert got.device == Xt.device and got.shape == (n,)
    assert got.cpu().numpy().tobytes() == host.tobytes()


def test_device_variants_refused_on_a_multi_device_context():
    import torch
    g = Engine(devices=[0, 0], strict=True)
    X = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(cocoa_amd.CocoaError) as ei:
        g.decision_function(X, np.ones(3))
    assert ei.value.code == C.E_STATE
    with pytest.raises(cocoa_amd.CocoaError) as ei:
        g.decision_function(X.to_sparse_csr(), np.ones(3))
    assert ei.value.code == C.E_STATE


# ------------------------------------------------------------- context w --
@pytest.fixture(scope="module")
def c1():
    return cocoa_amd.load_libsvm(TRAIN, 4, 9947), cocoa_amd.load_libsvm(TEST, 4, 9947)


def trained(c1, strict, rounds=4):
    tr, te = c1
    e = Engine(strict=strict)
    e.set_train(tr)
    e.set_test(te)
    e.init("cocoa+", tr.n, rounds, 50, 1e-3)
    for t in range(1, rounds + 1):
        e.round(t)
    return e


def test_context_w_strict(c1):
    tr, te = c1
    e = trained(c1, True)
    f_ctx = e.decision_function(te)
    w = e.w()
    f_w = e.decision_function(te, w)
    assert f_ctx.tobytes() == f_w.tobytes()
    f_ref, _ = ref_scores(te.row_ptr, te.col, te.val, w)
    assert f_ctx.tobytes() == f_ref.tobytes()
    assert e.score_errors(f_ctx, te.y) == e.eval()["test_err_count"]
    # dense rows of the context's width, w = None
    X = np.random.default_rng(1).standard_normal((3, tr.num_features))
    assert e.decision_function(X).tobytes() == e.decision_function(X, w).tobytes()
    # rows of another width are refused on a context that holds a training set
    with pytest.raises(cocoa_amd.IllegalArgumentError):
        e.decision_function(np.zeros((2, 5)), np.ones(5))


def test_context_w_fast_error_count(c1):
    tr, te = c1
    e = trained(c1, False)
    w = e.w()
    f_ref, a = ref_scores(te.row_ptr, te.col, te.val, w)
    nz = f_ref != 0.0
    print("min |f_ref| / sum|val w| over nonzero rows = %r" % float(np.min(np.abs(f_ref[nz]) / a[nz])))
    assert np.all(np.abs(f_ref[nz]) > 1e-6 * a[nz])  # the precondition of an exact error count
    f = e.decision_function(te)
    assert np.all(np.abs(f - f_ref) <= REL * a)
    assert e.score_errors(f, te.y) == e.score_errors(f_ref, te.y) == e.eval()["test_err_count"]
    import torch
    Xt = torch.sparse_csr_tensor(torch.from_numpy(te.row_ptr), torch.from_numpy(te.col), torch.from_numpy(te.val),
                                 size=(te.n, te.num_features)).to("cuda")
    f_dev = e.decision_function(Xt)  # the context's w, device rows
    assert np.all(np.abs(f_dev.cpu().numpy() - f_ref) <= REL * a)
    assert e.score_errors(f_dev, te.y) == e.eval()["test_err_count"]


def test_fast_error_count_on_seeded_rows(engines):
    case = Case([37] * 300 + [0] + [2100] * 3, 5000, 21)
    nz = case.f != 0.0
    assert np.all(np.abs(case.f[nz]) > 1e-6 * case.a[nz])
    f = engines[False].decision_function(case.data, case.w)
    check(f, case, False)
    assert Engine.score_errors(f, case.data.y) == Engine.score_errors(case.f, case.data.y)
    assert Engine.score_errors(f, case.data.y) == int(np.sum(~(case.f * case.data.y > 0)))


@pytest.mark.parametrize("strict", [True, False])
def test_context_without_training_set(ladder, strict):
    e = Engine(strict=strict)
    check(e.decision_function(ladder.data, ladder.w), ladder, strict)
    with pytest.raises(cocoa_amd.CocoaError) as ei:
        e.decision_function(ladder.data)
    assert ei.value.code == C.E_STATE
    with pytest.raises(cocoa_amd.CocoaError) as ei:
        e.decision_function(np.zeros((2, 3)))
    assert ei.value.code == C.E_STATE


@pytest.mark.parametrize("strict,solver", [(True, "auto"), (False, "chain"), (False, "gram")])
def test_scoring_does_not_disturb_training(c1, strict, solver):
    """Run A scores between rounds and while an evaluation is pending, run B
    does not: w, alpha and both evaluation records are bitwise equal, in strict
    mode and in fast mode on the chain solver.  Fast mode's Gram solver
    accumulates in LDS with floating-point atomics, so two identical runs
    WITHOUT any scoring already differ in the last bit (measured on C1: max
    |dw| 2.2e-16, alpha and the final evaluation differ too); on that path the
    twins are held to the 1e-12 bound the engine-reuse tests use between two
    orders of the same sums."""
    tr, te = c1

    def run(score):
        e = Engine(strict=strict)
        e.set_train(tr)
        e.set_test(te)
        e.set_solver(solver)
        e.init("cocoa+", tr.n, 6, 50, 1e-3)
        assert strict or e.plan()["solver"] == solver
        for t in (1, 2, 3):
            e.round(t)
        e.eval_begin()
        if score:
            f = e.decision_function(te)
            f2 = e.decision_function(te.row_range(0, 5), np.ones(tr.num_features))
            assert f.shape == (te.n,) and f2.shape == (5,)
        e.round(4)
        if score:
            e.score_set_chunk(1000)
            e.decision_function(te)
        ev1 = e.eval_end()
        for t in (5, 6):
            e.round(t)
            if score:
                e.decision_function(tr)
        return e.w(), e.alpha(), ev1, e.eval()

    wa, aa, e1a, e2a = run(True)
    wb, ab, e1b, e2b = run(False)
    if solver != "gram":
        assert wa.tobytes() == wb.tobytes() and aa.tobytes() == ab.tobytes()
        assert e1a == e1b and e2a == e2b
        return
    SAME = 1e-12
    assert np.max(np.abs(wa - wb)) <= SAME * np.max(np.abs(wb)) and np.max(np.abs(aa - ab)) <= SAME
    for x, y in ((e1a, e1b), (e2a, e2b)):
        assert abs(x["primal"] - y["primal"]) <= SAME * abs(y["primal"])
        assert abs(x["gap"] - y["gap"]) <= SAME * abs(y["primal"])
        assert x["test_err_count"] == y["test_err_count"] and x["test_rows"] == y["test_rows"]


def test_scoring_beside_a_pipelined_evaluation(c1):
    """cocoa_eval_async pending while rows are scored (fast mode, chain solver:
    the repeatable path): cocoa_eval_wait returns what the twin without scoring
    gets, and the run goes on the same."""
    tr, te = c1

    def run(score):
        e = Engine(strict=False)
        e.set_train(tr)
        e.set_test(te)
        e.set_solver("chain")
        e.init("cocoa+", tr.n, 5, 50, 1e-3)
        for t in (1, 2, 3):
            e.round(t)
        e.eval_async()
        if score:
            e.decision_function(te)
        e.round(4)
        if score:
            e.decision_function(te, np.ones(tr.num_features))
        ev = e.eval_wait()
        e.round(5)
        return e.w(), e.alpha(), ev, e.eval()

    wa, aa, e1a, e2a = run(True)
    wb, ab, e1b, e2b = run(False)
    assert wa.tobytes() == wb.tobytes() and aa.tobytes() == ab.tobytes()
    assert e1a == e1b and e2a == e2b


def test_init_after_scoring(c1):
    tr, te = c1
    a = trained(c1, True, rounds=3)
    a.decision_function(te)
    a.init("cocoa+", tr.n, 3, 50, 1e-3)
    for t in (1, 2, 3):
        a.round(t)
    b = trained(c1, True, rounds=3)
    assert a.w().tobytes() == b.w().tobytes() and a.eval() == b.eval()


def test_multi_device_host_scoring_strict(c1, ladder):
    tr, te = c1
    one = Engine(strict=True)
    g = Engine(devices=[0, 0], strict=True)
    assert g.decision_function(ladder.data, ladder.w).tobytes() == one.decision_function(ladder.data, ladder.w).tobytes()
    X = np.random.default_rng(8).standard_normal((31, 17))
    w = make_w(17, 2)
    assert g.decision_function(X, w).tobytes() == one.decision_function(X, w).tobytes()
    with pytest.raises(cocoa_amd.CocoaError) as ei:
        g.decision_function(X)
    assert ei.value.code == C.E_STATE
    # the group's own w after training, against a one-device engine's
    g.set_train(tr)
    g.init("cocoa+", tr.n, 2, 50, 1e-3)
    o = trained(c1, True, rounds=2)
    for t in (1, 2):
        g.round(t)
    assert g.decision_function(te).tobytes() == o.decision_function(te).tobytes()
