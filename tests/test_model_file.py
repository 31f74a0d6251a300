"""CPU tests of the scoring interface's host side: the text model file
(cocoa_model_save / cocoa_model_load) round-trips every double bitwise and
reports the documented error codes, and cocoa_score_errors applies
computeClassificationError's rule.  No GPU."""
import ctypes

import numpy as np
import pytest

import cocoa_amd
from cocoa_amd import _capi as C
from cocoa_amd.jdouble import java_double_tostring as jstr

SPECIAL = [0.0, -0.0, 1.0, -1.5, 5e-324, -5e-324, 2.2250738585072014e-308, 2.225073858507201e-308,
           1.7976931348623157e308, -1.7976931348623157e308, 2.0e23, 1.0e23, 9007199254740993.0, 0.1, 1e-3, 1e7,
           123456.789e-20, float("nan"), float("inf"), float("-inf"), np.pi, 4.35, 1.0e-5]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_round_trip_special_values_bitwise(tmp_path):
    w = np.array(SPECIAL, np.float64)
    p = str(tmp_path / "special.model")
    cocoa_amd.save_model(p, w, method="cocoa_plus", lam=1e-3, rounds=7)
    back = cocoa_amd.load_model(p)
    assert back.dtype == np.float64 and back.shape == w.shape
    assert np.array_equal(bits(back), bits(w))
    lines = open(p).read().split("\n")
    assert lines[:5] == ["COCOA-MODEL 1", "numFeatures %d" % len(w), "method cocoa_plus", "lambda 0.001", "rounds 7"]
    assert lines[-1] == "" and len(lines) == 5 + len(w) + 1
    # the weights are spelled as java.lang.Double.toString spells them
    assert lines[5:-1] == [jstr(float(x)) for x in w]
    assert lines[5 + SPECIAL.index(2.0e23)] == "1.9999999999999998E23"
    assert lines[5 + 1] == "-0.0" and lines[5 + 4] == "4.9E-324"


@pytest.mark.parametrize("d", [1, 9947])
def test_round_trip_sizes(tmp_path, d):
    rng = np.random.default_rng(d)
    w = rng.standard_normal(d) * np.exp(rng.uniform(-40, 40, d))
    # random bit patterns too (finite ones: a NaN payload has no text form)
    raw = rng.integers(0, 2 ** 63, d, dtype=np.int64).view(np.float64)
    w[::3] = np.where(np.isfinite(raw), raw, 1.0)[::3]
    p = str(tmp_path / "m.model")
    cocoa_amd.save_model(p, w, method="cocoa", lam=0.01, rounds=200)
    assert np.array_equal(bits(cocoa_amd.load_model(p)), bits(w))


def write(tmp_path, text, name="bad.model"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


GOOD = "COCOA-MODEL 1\nnumFeatures 2\nmethod cocoa\nlambda 0.001\nrounds 3\n1.0\n-2.5E-4\n"


def test_numpy_reads_the_weight_lines(tmp_path):
    p = write(tmp_path, GOOD, "good.model")
    assert cocoa_amd.load_model(p).tolist() == [1.0, -2.5e-4]
    assert np.loadtxt(p, skiprows=5).tolist() == [1.0, -2.5e-4]


@pytest.mark.parametrize("text", [
    "COCOA-MODEL 2\nnumFeatures 2\nmethod cocoa\nlambda 0.001\nrounds 3\n1.0\n2.0\n",   # wrong magic
    "COCOACK1\n",                                                                       # another format
    "",                                                                                 # empty file
    "COCOA-MODEL 1\nnumFeatures 2\nmethod cocoa\nlambda 0.001\nrounds 3\n1.0\n",        # a line short
    "COCOA-MODEL 1\nnumFeatures 2\nmethod cocoa\nlambda 0.001\nrounds 3\n1.0\n2.0\n3.0\n",  # a line long
    "COCOA-MODEL 1\nnumFeatures 2\nmethod cocoa\nlambda 0.001\nrounds 3\n1.0\n2.0x\n",  # unparsable number
    "COCOA-MODEL 1\nnumFeatures 2\nmethod cocoa\nlambda 0.001\nrounds 3\n1.0\n\n",      # empty number
    "COCOA-MODEL 1\nnumFeatures 2\nmethod cocoa\nlambda 0.001\nrounds 3\n1.0\n 2.0\n",  # leading blank
    "COCOA-MODEL 1\nnumFeatures 2\nmethod cocoa\nlambda 0.001\nrounds 3\n1.0\nnan\n",   # not Java's spelling
    "COCOA-MODEL 1\nnumFeatures two\nmethod cocoa\nlambda 0.001\nrounds 3\n1.0\n2.0\n",  # bad header number
    "COCOA-MODEL 1\nnumFeatures 0\nmethod cocoa\nlambda 0.001\nrounds 3\n",             # d < 1
    "COCOA-MODEL 1\nnumFeatures 2\nlambda 0.001\nmethod cocoa\nrounds 3\n1.0\n2.0\n",   # header order
])
def test_load_parse_errors(tmp_path, text):
    p = write(tmp_path, text)
    with pytest.raises(cocoa_amd.NumberFormatError) as ei:
        cocoa_amd.load_model(p)
    assert ei.value.code == C.E_PARSE


def test_load_missing_file_is_io_error(tmp_path):
    with pytest.raises(cocoa_amd.CocoaError) as ei:
        cocoa_amd.load_model(str(tmp_path / "nope.model"))
    assert ei.value.code == C.E_IO


def test_save_errors(tmp_path):
    w = np.ones(3)
    with pytest.raises(cocoa_amd.CocoaError) as ei:
        cocoa_amd.save_model(str(tmp_path / "no_such_dir" / "m.model"), w)
    assert ei.value.code == C.E_IO
    with pytest.raises(cocoa_amd.IllegalArgumentError):
        cocoa_amd.save_model(str(tmp_path / "m.model"), np.zeros(0))
    lib = C.lib()
    assert lib.cocoa_model_save(None, C.f64p(w), 3, b"x", 0.0, 0) == C.E_ARG
    assert lib.cocoa_model_save(str(tmp_path / "m.model").encode(), None, 3, b"x", 0.0, 0) == C.E_ARG
    assert lib.cocoa_model_load(None, None, None) == C.E_ARG


def test_score_errors_rule():
    nan = float("nan")
    f = np.array([0.5, -0.5, 0.5, -0.5, 0.0, 0.0, -0.0, nan, nan, 1e-320, -1e-320, np.inf, -np.inf])
    y = np.array([1.0, -1.0, -1.0, 1.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0])
    # errors: rows 2, 3 (wrong sign), 4, 5, 6 (f = 0 under either label), 7, 8 (NaN), 10, 12
    assert cocoa_amd.Engine.score_errors(f, y) == 9
    assert cocoa_amd.Engine.score_errors(f, y) == int(np.sum(~(f * y > 0)))
    assert cocoa_amd.Engine.score_errors(np.zeros(0), np.zeros(0)) == 0
    n = ctypes.c_int64(-1)
    assert C.lib().cocoa_score_errors(None, None, 3, ctypes.byref(n)) == C.E_ARG
    assert C.lib().cocoa_score_errors(C.f64p(f), C.f64p(y), -1, ctypes.byref(n)) == C.E_ARG
    assert C.lib().cocoa_score_errors(C.f64p(f), C.f64p(y), 2, None) == C.E_ARG
