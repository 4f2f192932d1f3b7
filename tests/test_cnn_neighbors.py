"""``embed`` / ``neighbors`` of fitted Genetic-CNN models on the CPU (torch executor) against the plain-loop oracle
of tests/neighbors_ref.py. The fits are those of tests/test_cnn_tta.py (shared inside one pytest process, left
unchanged)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import neighbors_ref as R
import test_cnn_tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, NB = 7, 40               # queries x[:NQ], bank x[NQ:NQ + NB]


def _same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("case,ens", [("mnist", False), ("rgb", False), ("rgb", True)])
def test_neighbors_equal_the_oracle(case, ens, metric, k):
    fitted, x = T._ensemble(case)
    obj = fitted if ens else fitted.members[0]
    q, bank = x[:NQ], x[NQ:NQ + NB]
    eb = obj.embed(bank)
    assert eb.dtype == np.float32 and eb.shape == (NB, (3 if ens else 1) * 16) and eb.min() >= 0 and eb.max() > 0
    want = R.neighbors_ref(obj.embed(q), eb, k, metric)
    _same(obj.neighbors(q, bank, k=k, metric=metric), want)                 # a bank of images
    _same(obj.neighbors(q, eb, k=k, metric=metric, batch=32), want)         # the same bank, embedded before


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_duplicates_tie_and_a_bank_row_finds_itself(metric):
    """Bank rows 3 and 11 are one image: side by side, 3 first, equal distance. Query 0 is bank row 5: first, l2 0."""
    _, clf, x = T._fit("mnist")
    bank = x[NQ:NQ + NB].copy()
    bank[11] = bank[3]
    q = np.concatenate([bank[5:6], bank[3:4], x[:3]])
    idx, dist = clf.neighbors(q, bank, k=16, metric=metric)
    _same((idx, dist), R.neighbors_ref(clf.embed(q), clf.embed(bank), 16, metric))
    if metric == "l2":           # (a cosine distance of 0 is shared by every bank row of the query's direction)
        assert idx[0, 0] == 5 and idx[1, 0] == 3 and idx[1, 1] == 11
        assert dist[0, 0] == 0.0 and dist[1, 0] == 0.0 and dist[1, 1] == 0.0
    for row_i, row_d in zip(idx, dist):
        at = {int(j): p for p, j in enumerate(row_i)}
        assert 11 not in at or at[11] == at[3] + 1
        assert at.get(3, 15) == 15 or (at[11] == at[3] + 1 and row_d[at[3]] == row_d[at[11]])


def test_batch_does_not_change_a_row_and_the_ensemble_concatenates():
    fitted, x = T._ensemble("rgb_bn")
    a, b = fitted.embed(x[:70], batch=32), fitted.embed(x[:70], batch=256)
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() == np.concatenate([m.embed(x[:70]) for m in fitted.members], axis=1).tobytes()
    _same(fitted.neighbors(x[:70], x[20:90], k=5, batch=32), fitted.neighbors(x[:70], x[20:90], k=5, batch=256))
    assert fitted.embed(x[0]).shape == (1, 48)
    m, clf, x = T._fit("mnist")                                             # the model forwards to its classifier
    assert m.embed(x[:5]).tobytes() == clf.embed(x[:5]).tobytes()
    _same(m.neighbors(x[:5], x[5:30], k=3, metric="cosine"), clf.neighbors(x[:5], x[5:30], k=3, metric="cosine"))


BAD = [
    (dict(k=0), "k must be"), (dict(k=17), "k must be"), (dict(k=2.0), "k must be"), (dict(k=True), "k must be"),
    (dict(k=9), "exceeds the bank"), (dict(metric="l1"), "metric"), (dict(bank="D15"), "features"),
    (dict(bank="nan"), "finite"), (dict(bank="3d"), "bank must be"), (dict(bank="shape"), "bank of images"),
    (dict(batch=0), "batch"), (dict(batch=1.5), "batch"), (dict(backend="triton"), "backend"),
]


@pytest.mark.parametrize("ens", [False, True])
@pytest.mark.parametrize("kw,msg", BAD, ids=[str(i) for i in range(len(BAD))])
def test_refusals_come_before_any_forward(kw, msg, ens, monkeypatch):
    from gentun_amd.models.cnn_fitted import CnnClassifier
    fitted, x = T._ensemble("mnist")
    obj = fitted if ens else fitted.members[0]
    D = 48 if ens else 16

    def no_forward(*a, **k):
        raise AssertionError("a forward ran before the refusal")
    monkeypatch.setattr(CnnClassifier, "_torch_features", no_forward)
    banks = {"D15": np.zeros((8, D - 1), np.float32), "nan": np.full((8, D), np.nan, np.float32),
             "3d": np.zeros((8, 4, D), np.float32), "shape": np.zeros((8, 28, 27, 1), np.float32)}
    kw = dict(kw)
    bank = banks[kw.pop("bank")] if "bank" in kw else x[:8]
    with pytest.raises(ValueError, match=msg):
        obj.neighbors(x[:2], bank, **kw)
    if "batch" in kw or "backend" in kw:
        with pytest.raises(ValueError, match=msg):
            obj.embed(x[:2], **kw)


def test_example_runs():
    env = dict(os.environ, GENTUN_EXAMPLE_SMALL="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cnn_neighbors.py"), "--device", "cpu"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["k"] == 5 and out["bank_rows"] == 224 - out["held_out_rows"]
    assert 0.0 <= out["accuracy_vote"] <= 1.0 and out["kth_distance_held_out"] >= 0.0
