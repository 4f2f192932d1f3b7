"""The fitted GBDT model on MI355X: ``gbdt.train(device='cuda:0')`` against the engine's own stage trace, and the
forest predictor (csrc/hip/gbdt_predict.hip) against the CPU predictor, bit for bit. Shapes come from
tests/gbdt_stage_cases.py; the predictor's shapes are the smallest that reach each kernel path."""

import numpy as np
import pytest

import gbdt_stage_cases as cases
from gentun_amd.models import gbdt

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TRAIN_CASES = ("B3", "C", "E", "F1", "G0", "H12")
_GPU_FIT, _CPU_FIT = {}, {}


def _gpu_fit(name):
    if name not in _GPU_FIT:
        c = cases.load(name)
        _GPU_FIT[name] = gbdt.train(c["params"], c["x"], c["y"], num_boost_round=c["rounds"], seed=c["seed"], device=DEV)
    return _GPU_FIT[name]


def _cpu_fit(key, params, x, y, rounds):
    if key not in _CPU_FIT:
        _CPU_FIT[key] = gbdt.train(params, x, y, num_boost_round=rounds, seed=0)
    return _CPU_FIT[key]


def _fresh(F, seed, n=700):
    """Rows no model saw: NaN, +-inf and values beyond the training range."""
    rng = np.random.default_rng(seed)
    z = (3.0 * rng.standard_normal((n, F))).astype(np.float32)
    for p, v in ((0.05, np.nan), (0.02, np.inf), (0.02, -np.inf), (0.02, 1e30), (0.02, -1e30)):
        z[rng.random(z.shape) < p] = v
    return z


def _compact(tree_xy, leaf, max_depth):
    """Heap tables of the trace -> level-order (feature, split_bin, left, value), written independently of the
    package's compaction: recursive depths first, then numbering by (depth, heap index)."""
    reach = []

    def visit(h, d):
        reach.append((d, h))
        if tree_xy[h][0] >= 0 and d < max_depth:
            visit(2 * h + 1, d + 1)
            visit(2 * h + 2, d + 1)

    visit(0, 0)
    reach.sort()
    index = {h: i for i, (_d, h) in enumerate(reach)}
    feature, split_bin, left, value = [], [], [], []
    for d, h in reach:
        split = tree_xy[h][0] >= 0 and d < max_depth
        feature.append(int(tree_xy[h][0]) if split else -1)
        split_bin.append(int(tree_xy[h][1]) if split else -1)
        left.append(index[2 * h + 1] if split else -1)
        value.append(float(leaf[h]))
    return feature, split_bin, left, value


_TRACE = {}


def _trace(name):
    """One-fold trace of the case (fold_of == -1 everywhere): {(round, class): (TREE, LEAF)}, final MARGIN, history."""
    if name not in _TRACE:
        from gentun_amd.models import gbdt_hip as H
        c = cases.load(name)
        n = c["x"].shape[0]
        hist = np.zeros((c["rounds"], len(c["marr"]), 4))
        kept, T = H.cv_trace(c["x"], c["y"], np.full(n, -1, np.int32), 1, c["parr"], c["obj"], c["num_class"], c["marr"],
                             c["rounds"], 0, c["seed"], hist, trace_rounds=c["rounds"], tags=["TREE", "LEAF", "MARGIN"])
        assert kept == c["rounds"]
        _TRACE[name] = (T, hist)
    return _TRACE[name]


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_trained_trees_equal_the_trace(name):
    c = cases.load(name)
    bst = _gpu_fit(name)
    T, hist = _trace(name)
    D = max(0, min(int(c["params"]["max_depth"]), 12))
    tsz = (2 << D) - 1
    assert bst.num_trees == c["rounds"] * bst.K
    for t in range(bst.num_trees):
        rnd, cl = divmod(t, bst.K)
        tree = T[(rnd, cl, -1, "TREE")]
        leaf = T[(rnd, cl, -1, "LEAF")]
        assert len(tree) == tsz and len(leaf) == tsz                      # one fold
        txy = np.stack([tree["x"], tree["y"]], axis=1)
        feature, split_bin, left, value = _compact(txy, leaf, D)
        o, e = int(bst.tree_offsets[t]), int(bst.tree_offsets[t + 1])
        assert bst.feature[o:e].tolist() == feature, t
        assert bst.split_bin[o:e].tolist() == split_bin, t
        assert bst.left[o:e].tolist() == left, t
        assert bst.value[o:e].tobytes() == np.asarray(value, np.float64).tobytes(), t
        assert np.array_equal(bst.value[o:e].astype(np.float32).astype(np.float64), bst.value[o:e])
    if name == "G0":
        assert np.all(np.diff(bst.tree_offsets) == 1)
    else:
        assert np.any(bst.feature >= 0)
    metrics = c["params"].get("eval_metric") or gbdt.DEFAULT_METRIC[c["obj"]]
    for j, m in enumerate([metrics] if isinstance(metrics, str) else metrics):
        assert bst.history["train-" + m] == hist[:, j, 0].tolist()
    # thresholds are the device cuts at the split bins, and the device cuts are the CPU quantiser's
    cuts = gbdt.cuts(c["x"])
    inner = np.flatnonzero(bst.feature >= 0)
    want = np.array([cuts[bst.feature[i]][bst.split_bin[i]] for i in inner], np.float32)
    assert bst.threshold[inner].tobytes() == want.tobytes()


def _same_on_both(bst, x, **kw):
    for mode in ({"output_margin": True}, {"pred_leaf": True}):
        cpu = bst.predict(x, **mode, **kw)
        gpu = bst.predict(x, device=DEV, **mode, **kw)
        assert cpu.dtype == gpu.dtype and cpu.shape == gpu.shape
        assert cpu.tobytes() == gpu.tobytes(), (mode, kw, x.shape)


def test_predict_chunk_and_block_tails_three_classes(monkeypatch):
    """n = 5003 with 1000-row uploads (a chunk tail of 3 rows, block tails), K = 3, ntree_limit, n = 1."""
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("E")
    monkeypatch.setattr(H, "PREDICT_CHUNK_ROWS", 1000)
    cpu_bst = _cpu_fit("E", c["params"], c["x"], c["y"], 3)
    for bst in (_gpu_fit("E"), cpu_bst):
        assert bst.K == 3
        _same_on_both(bst, c["x"])
        _same_on_both(bst, _fresh(c["x"].shape[1], 1))
        _same_on_both(bst, c["x"], ntree_limit=2)
        _same_on_both(bst, c["x"][:1])
        for kw in ({}, {"ntree_limit": 1}):
            assert bst.predict(c["x"], device=DEV, **kw).tobytes() == bst.predict(c["x"], **kw).tobytes()


def test_predict_five_features():
    from gentun_amd.models import gbdt_hip as H
    x, y = cases._reg(1000, 5, 11)
    x = np.ascontiguousarray(x, np.float32)
    assert x.shape[1] == 5 and H.predict_rows(5) == 256
    bst = _cpu_fit("F5", {"objective": "reg:linear", "max_depth": 3}, x, y, 3)
    _same_on_both(bst, x)
    _same_on_both(bst, _fresh(5, 2, n=257))


def test_predict_256_features_rows_in_lds():
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("A")
    assert c["x"].shape[1] == 256 and 64 <= H.predict_rows(256) < 256
    bst = _cpu_fit("A", c["params"], c["x"], c["y"], 2)
    _same_on_both(bst, c["x"][:1500])
    _same_on_both(bst, _fresh(256, 3, n=300))


def test_predict_wide_rows_from_global_memory():
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("I")
    assert c["x"].shape == (200, 8200) and H.predict_rows(8200) == 0
    bst = _cpu_fit("I", c["params"], c["x"], c["y"], 2)
    assert np.any(bst.feature >= 0)
    _same_on_both(bst, c["x"])
    _same_on_both(bst, _fresh(8200, 4, n=70))


def test_predict_tree_beyond_the_chunk_budget():
    c = cases.load("H12")
    bst = _gpu_fit("H12")
    assert int(np.diff(bst.tree_offsets).max()) > 1228                    # PF_NODES: walked from global memory
    _same_on_both(bst, c["x"][:3000])
    _same_on_both(bst, _fresh(c["x"].shape[1], 5))


def test_predict_several_tree_chunks():
    c = cases.load("B3")
    bst = _cpu_fit("B3x40", {"objective": "reg:linear", "max_depth": 6, "eta": 0.1}, c["x"], c["y"], 40)
    assert bst.num_trees == 40 and len(bst.feature) > 3 * 1228           # more than three LDS tree chunks
    _same_on_both(bst, c["x"])
    _same_on_both(bst, _fresh(c["x"].shape[1], 6))
    _same_on_both(bst, c["x"], ntree_limit=17)


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_predict_of_training_rows_follows_the_fp32_training_margins(name):
    """The engine sums a row's leaves in fp32, the Booster in fp64: T additions plus the base margin's rounding,
    each within 2^-24 of the partial margin it produces."""
    c = cases.load(name)
    bst = _gpu_fit(name)
    n, K, rounds = c["x"].shape[0], bst.K, c["rounds"]
    traced = _trace(name)[0][(rounds - 1, K - 1, -1, "MARGIN")].reshape(n, K).astype(np.float64)
    got = bst.predict(c["x"], output_margin=True, device=DEV).reshape(n, K)
    leaves = bst.predict(c["x"], pred_leaf=True)
    partial = np.full((n, K), bst.base_margin, np.float64)
    biggest = np.abs(partial).max()
    for t in range(bst.num_trees):
        partial[:, t % K] += bst.value[int(bst.tree_offsets[t]) + leaves[:, t]]
        biggest = max(biggest, np.abs(partial).max())
    assert partial.tobytes() == got.tobytes()
    bound = (rounds + 1) * 2.0 ** -24 * biggest
    err = float(np.abs(got - traced).max())
    print("case", name, "max |fp64 predict - fp32 training margin|", err, "bound", bound)
    assert err <= bound


@pytest.mark.parametrize("name", ["F1", "B3"])
def test_device_cuts_equal_cpu_cuts(name):
    from gentun_amd.models import gbdt_hip as H
    c = cases.load(name)
    nb, key, _fs = H.quantize_device(c["x"])
    dev, cpu = H.device_cuts(key, nb), gbdt.cuts(c["x"])
    assert len(dev) == len(cpu) == c["x"].shape[1]
    for a, b in zip(dev, cpu):
        assert a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes()


def test_cv_is_unchanged_by_train():
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("C")
    kw = dict(num_boost_round=2, nfold=3, seed=0, device=DEV)
    before = gbdt.cv(c["params"], c["x"], c["y"], **kw)
    key = H.quantize_device(c["x"])[1]
    gbdt.train(c["params"], c["x"], c["y"], num_boost_round=2, seed=0, device=DEV)
    assert H.quantize_device(c["x"])[1] == key                              # the bins cache survived
    assert gbdt.cv(c["params"], c["x"], c["y"], **kw) == before
    assert H.quantize_device(c["x"])[1] == key                              # and cv found them on the device


def test_train_refuses_trees_deeper_than_the_engine():
    c = cases.load("G0")
    with pytest.raises(ValueError):
        gbdt.train({"objective": "reg:linear", "max_depth": 13}, c["x"], c["y"], num_boost_round=1, device=DEV)
