"""cocoa_driver --modelDir and cocoa_predict on the reference demo (config C1),
strict mode: writing the models changes nothing on the driver's stdout, and
cocoa_predict on the CoCoA+ model prints the test error the driver printed and
writes the decision values of the loaded model, bitwise."""
import os
import subprocess

import numpy as np
import pytest

import cocoa_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DRIVER = os.path.join(ROOT, "cocoa_amd", "cocoa_driver")
PREDICT = os.path.join(ROOT, "cocoa_amd", "cocoa_predict")
TRAIN = os.path.join(GOLD, "data", "small_train.dat")
TEST = os.path.join(GOLD, "data", "small_test.dat")


def run(cmd, cwd):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(cwd))


def test_model_dir_and_predict(tmp_path):
    assert os.path.exists(DRIVER) and os.path.exists(PREDICT), "build cocoa_driver and cocoa_predict first (make)"
    cmd = [DRIVER, "--trainFile=" + TRAIN, "--testFile=" + TEST, "--numFeatures=9947", "--numRounds=5",
           "--localIterFrac=0.1", "--numSplits=4", "--lambda=.001", "--justCoCoA=false", "--strict=true",
           "--debugIter=5"]
    plain = run(cmd, tmp_path)
    mdir = tmp_path / "models"
    mdir.mkdir()
    saved = run(cmd + ["--modelDir=" + str(mdir)], tmp_path)
    assert plain.returncode == 1 and saved.returncode == 1 and "DistGD" in saved.stderr  # the DistGD exit, as before
    assert saved.stdout == plain.stdout
    assert sorted(os.listdir(mdir)) == ["cocoa.model", "cocoa_plus.model", "localsgd.model", "mbcd.model",
                                        "mbsgd.model"]
    lines = saved.stdout.splitlines()
    i = next(k for k, ln in enumerate(lines) if ln.startswith("CoCoA+ has finished running"))
    driver_err = next(ln for ln in lines[i:] if ln.startswith(" Test Error: ")).split(": ", 1)[1]

    model = str(mdir / "cocoa_plus.model")
    head = open(model).read().split("\n")[:5]
    assert head == ["COCOA-MODEL 1", "numFeatures 9947", "method cocoa_plus", "lambda 0.001", "rounds 5"]
    out = tmp_path / "scores.txt"
    p = run([PREDICT, "--modelFile=" + model, "--testFile=" + TEST, "--numFeatures=9947", "--numSplits=4",
             "--outFile=" + str(out), "--strict=true"], tmp_path)
    assert p.returncode == 0, p.stderr
    got = dict(ln.split(": ", 1) for ln in p.stdout.splitlines())
    assert got["rows"] == "600"
    assert got["test error"] == driver_err

    # the --outFile lines are the strict scores of the loaded model
    w = cocoa_amd.load_model(model)
    te = cocoa_amd.load_libsvm(TEST, 4, 9947)
    wl, cl, vl, rp = w.tolist(), te.col.tolist(), te.val.tolist(), te.row_ptr.tolist()
    ref = []
    for r in range(te.n):
        s = 0.0
        for q in range(rp[r], rp[r + 1]):
            s = s + vl[q] * wl[cl[q]]
        ref.append(s)
    scores = [float(ln) for ln in open(out).read().splitlines()]
    assert np.array(scores).tobytes() == np.array(ref).tobytes()
    assert scores == [float(cocoa_amd.jstr(s)) for s in ref]

    # without --numFeatures the model's width is used; a missing model is an error
    q = run([PREDICT, "--modelFile=" + model, "--testFile=" + TEST, "--strict=true"], tmp_path)
    assert q.returncode == 0 and q.stdout == p.stdout
    bad = run([PREDICT, "--modelFile=" + str(mdir / "none.model"), "--testFile=" + TEST], tmp_path)
    assert bad.returncode == 1 and bad.stdout == ""
