"""Node statistics and SHAP contributions on MI355X: the GPU-trained cover / gain against the engine's own
stage trace, and the SHAP kernel (csrc/hip/gbdt_shap.hip) against the CPU predictor, bit for bit, on the
smallest shapes that reach each of its paths: rows in LDS or from global memory x tables in LDS chunks or from
global memory, chunk and block tails, K > 1, merged elements, depth 0."""

import numpy as np
import pytest

import gbdt_stage_cases as cases
import gbdt_stage_ref as ref
from gentun_amd.models import gbdt
from gentun_amd.models.booster import Booster
from test_gbdt_explain import fit as small_fit, leaf_scale, mixed_rows, odd_rows, oracle_contribs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TABLE_BYTES = 32 * 1024          # SH_TABLE_BYTES of gbdt_shap.hip
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


def _reach(tree_xy, max_depth):
    """Heap ids of the nodes a walk from the root reaches, in the Booster's order: by (depth, heap id)."""
    reach = []

    def visit(h, d):
        reach.append((d, h))
        if tree_xy[h][0] >= 0 and d < max_depth:
            visit(2 * h + 1, d + 1)
            visit(2 * h + 2, d + 1)

    visit(0, 0)
    reach.sort()
    return reach


@pytest.mark.parametrize("name", ["B3", "C", "E", "G0", "H12"])
def test_trained_statistics_equal_the_trace(name):
    from gentun_amd.models import gbdt_hip as H
    c = cases.load(name)
    bst = _gpu_fit(name)
    assert bst.cover is not None and bst.cover.dtype == np.float64 and len(bst.cover) == len(bst.feature)
    n = c["x"].shape[0]
    hist = np.zeros((c["rounds"], len(c["marr"]), 4))
    kept, T = H.cv_trace(c["x"], c["y"], np.full(n, -1, np.int32), 1, c["parr"], c["obj"], c["num_class"], c["marr"],
                         c["rounds"], 0, c["seed"], hist, trace_rounds=c["rounds"],
                         tags=["TREE", "MX", "LNODES", "BEST"])
    assert kept == c["rounds"]
    D = max(0, min(int(c["params"]["max_depth"]), 12))
    tsz = (2 << D) - 1
    lgn = ref.lg_n(n, c["obj"] == 0)
    for t in range(bst.num_trees):
        rnd, cl = divmod(t, bst.K)
        tree = T[(rnd, cl, -1, "TREE")]
        txy = np.stack([tree["x"], tree["y"]], axis=1)
        mx = T[(rnd, cl, -1, "MX")].view(np.float32)
        ih = 2.0 ** -ref.fx_exp(mx[1], lgn)
        cover_h, gain_h = np.zeros(tsz), np.zeros(tsz)
        for d in range(D + 1):
            L = 1 << d
            cover_h[L - 1:2 * L - 1] = T[(rnd, cl, d, "LNODES")]["H"][:L].astype(np.float64) * ih
            if d < D:
                gain_h[L - 1:2 * L - 1] = T[(rnd, cl, d, "BEST")]["gain"][:L]
        reach = _reach(txy, D)
        o, e = int(bst.tree_offsets[t]), int(bst.tree_offsets[t + 1])
        assert e - o == len(reach)
        want_cover = np.array([cover_h[h] for _d, h in reach])
        want_gain = np.array([gain_h[h] if txy[h][0] >= 0 and d < D else 0.0 for d, h in reach])
        assert bst.cover[o:e].tobytes() == want_cover.tobytes(), t
        assert bst.gain[o:e].tobytes() == want_gain.tobytes(), t
    if name == "B3":                             # reg:linear, subsample 1: the covers are row counts
        for t in range(bst.num_trees):
            o, e = int(bst.tree_offsets[t]), int(bst.tree_offsets[t + 1])
            counts = np.zeros(e - o)
            leaves = bst.predict(c["x"], pred_leaf=True)[:, t]
            for j in range(e - o - 1, -1, -1):   # children come after their parent
                counts[j] = np.sum(leaves == j) if bst.feature[o + j] < 0 else (
                    counts[bst.left[o + j]] + counts[bst.left[o + j] + 1])
            assert bst.cover[o:e].tolist() == counts.tolist()


def test_cv_is_unchanged_by_a_train_with_statistics():
    c = cases.load("C")
    kw = dict(num_boost_round=2, nfold=3, seed=0, device=DEV)
    before = gbdt.cv(c["params"], c["x"], c["y"], **kw)
    bst = gbdt.train(c["params"], c["x"], c["y"], num_boost_round=2, seed=0, device=DEV)
    assert bst.cover is not None
    assert gbdt.cv(c["params"], c["x"], c["y"], **kw) == before


# ---- GPU against CPU, bit for bit ---------------------------------------------------------------------------
def _same_on_both(bst, x, **kw):
    cpu = bst.predict(x, pred_contribs=True, **kw)
    gpu = bst.predict(x, pred_contribs=True, device=DEV, **kw)
    assert cpu.dtype == gpu.dtype == np.float64 and cpu.shape == gpu.shape
    assert cpu.shape == ((len(x), x.shape[1] + 1) if bst.K == 1 else (len(x), bst.K, x.shape[1] + 1))
    assert cpu.tobytes() == gpu.tobytes(), (kw, x.shape)
    return gpu


def _fresh(F, seed, n=700):
    return odd_rows(F, seed, n)


def _table_bytes(bst, t):
    """Bytes of tree t's leaf and element records in gbdt_shap.hip: 16 per leaf, 32 per unique feature of a path."""
    o, e = int(bst.tree_offsets[t]), int(bst.tree_offsets[t + 1])
    feats = {0: frozenset()}
    total = 0
    for j in range(e - o):
        if bst.feature[o + j] >= 0:
            s = feats[j] | {int(bst.feature[o + j])}
            feats[int(bst.left[o + j])] = feats[int(bst.left[o + j]) + 1] = s
        else:
            total += 16 + 32 * len(feats[j])
    return total


def _longest_path(bst):
    best = 0
    for t in range(bst.num_trees):
        o, e = int(bst.tree_offsets[t]), int(bst.tree_offsets[t + 1])
        feats = {0: frozenset()}
        for j in range(e - o):
            if bst.feature[o + j] >= 0:
                s = feats[j] | {int(bst.feature[o + j])}
                feats[int(bst.left[o + j])] = feats[int(bst.left[o + j]) + 1] = s
            else:
                best = max(best, len(feats[j]))
    return best


def test_contribs_chunk_and_block_tails_three_classes(monkeypatch):
    """n = 5003 with 1000-row uploads (a chunk tail of 3 rows, block tails), K = 3, ntree_limit, n = 1."""
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("E")
    monkeypatch.setattr(H, "PREDICT_CHUNK_ROWS", 1000)
    cpu_bst = _cpu_fit("E", c["params"], c["x"], c["y"], 3)
    for bst in (_gpu_fit("E"), cpu_bst):
        assert bst.K == 3 and len(c["x"]) == 5003
        _same_on_both(bst, c["x"])
        _same_on_both(bst, _fresh(c["x"].shape[1], 1))
        _same_on_both(bst, c["x"][:1200], ntree_limit=2)
        _same_on_both(bst, c["x"][:1])


def test_contribs_five_features():
    from gentun_amd.models import gbdt_hip as H
    x, y = cases._reg(1000, 5, 11)
    x = np.ascontiguousarray(x, np.float32)
    assert x.shape[1] == 5 and H.shap_rows(5) == 256
    bst = _cpu_fit("F5", {"objective": "reg:linear", "max_depth": 3}, x, y, 3)
    _same_on_both(bst, x)
    _same_on_both(bst, _fresh(5, 2, n=257))


def test_contribs_256_features():
    """Bench width. Its rows are read from global memory: staged rows would leave one wave per CU (see the
    kernel's header); the staged-rows path is what the narrow cases (F = 5, 6, 8, 9) run."""
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("A")
    assert c["x"].shape[1] == 256 and H.shap_rows(256) == 0 and H.shap_rows(13) == 256 and H.shap_rows(14) == 0
    bst = _cpu_fit("A", c["params"], c["x"], c["y"], 2)
    _same_on_both(bst, c["x"][:1500])
    _same_on_both(bst, _fresh(256, 3, n=300))


def test_contribs_wide_rows_from_global_memory():
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("I")
    assert c["x"].shape == (200, 8200) and H.shap_rows(8200) == 0
    bst = _cpu_fit("I", c["params"], c["x"], c["y"], 2)
    assert np.any(bst.feature >= 0)
    _same_on_both(bst, c["x"])
    _same_on_both(bst, _fresh(8200, 4, n=70))


def test_contribs_wide_rows_and_a_tree_beyond_the_table_budget():
    """The one kernel path no trained case reaches: rows from global memory AND tables from global memory. A
    synthetic full tree of depth 8 over 8200 features, with random positive covers."""
    from gentun_amd.models import gbdt_hip as H
    F, depth = 8200, 8
    assert H.shap_rows(F) == 0
    rng = np.random.default_rng(12)
    nn, inner = (2 << depth) - 1, (1 << depth) - 1
    feature = np.full(nn, -1, np.int32)
    feature[:inner] = rng.integers(0, F, inner)
    left = np.full(nn, -1, np.int32)
    left[:inner] = 2 * np.arange(inner) + 1
    threshold = np.zeros(nn, np.float32)
    threshold[:inner] = rng.standard_normal(inner)
    bst = Booster(tree_offsets=[0, nn], feature=feature, threshold=threshold, split_bin=np.where(feature >= 0, 0, -1),
                  left=left, value=0.1 * rng.standard_normal(nn), objective=0, num_class=1, base_margin=0.5,
                  n_features=F, params={}, history={}, cover=rng.uniform(0.5, 9.0, nn), gain=np.zeros(nn))
    assert _table_bytes(bst, 0) > TABLE_BYTES
    got = _same_on_both(bst, _fresh(F, 13, n=70))
    margin = bst.predict(_fresh(F, 13, n=70), output_margin=True, device=DEV)
    assert np.abs(got.sum(axis=1) - margin).max() <= 1e-12 * leaf_scale(bst)


def test_contribs_tree_beyond_the_table_budget():
    c = cases.load("H12")
    bst = _gpu_fit("H12")
    from gentun_amd.models import gbdt_hip as H
    assert _table_bytes(bst, 0) > TABLE_BYTES                             # read from global memory
    assert _longest_path(bst) == 6 and H.shap_rows(6) == 256              # beside rows staged in LDS
    _same_on_both(bst, c["x"][:1000])
    _same_on_both(bst, _fresh(c["x"].shape[1], 5, n=300))


def test_contribs_paths_of_twelve_unique_features():
    """33 features, depth 16: paths with 12 or more unique features, still inside the kernel's limit; the tree's
    tables also exceed the chunk budget."""
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("B3")
    bst = _cpu_fit("deep16", {"objective": "reg:linear", "max_depth": 16, "min_child_weight": 0, "lambda": 0.0},
                   c["x"], c["y"], 1)
    assert 12 <= _longest_path(bst) <= H.shap_limit()
    _same_on_both(bst, c["x"][:600])
    _same_on_both(bst, _fresh(c["x"].shape[1], 8, n=300))


def test_contribs_several_table_chunks():
    c = cases.load("B3")
    bst = _cpu_fit("B3x40", {"objective": "reg:linear", "max_depth": 6, "eta": 0.1}, c["x"], c["y"], 40)
    sizes = [_table_bytes(bst, t) for t in range(bst.num_trees)]
    assert max(sizes) <= TABLE_BYTES and sum(sizes) > 3 * TABLE_BYTES      # more than three LDS table chunks
    _same_on_both(bst, c["x"][:1500])
    _same_on_both(bst, _fresh(c["x"].shape[1], 6))
    _same_on_both(bst, c["x"][:700], ntree_limit=17)


def test_contribs_depth_zero():
    c = cases.load("G0")
    bst = _gpu_fit("G0")
    assert np.all(np.diff(bst.tree_offsets) == 1)
    got = _same_on_both(bst, c["x"][:300])
    assert np.all(got[:, :-1] == 0.0)


def test_contribs_merged_elements_oracle_and_additivity():
    """The 2-feature depth-5 model (paths repeat a feature), F = 8: GPU == CPU, the GPU output against the
    brute-force oracle with the CPU test's bound, and additivity against the GPU margins."""
    from gentun_amd.models import gbdt_hip as H
    x, _y, bst = small_fit("two")
    assert H.shap_rows(8) == 256
    rows = mixed_rows(x, 5)
    got = _same_on_both(bst, rows)
    want = oracle_contribs(bst, rows)[:, 0, :]
    bound = 1e-12 * leaf_scale(bst)
    err = float(np.abs(got - want).max())
    print("max |GPU phi - oracle|", err, "bound", bound)
    assert err <= bound
    big = np.concatenate([x, _fresh(8, 7)])
    phi = _same_on_both(bst, big)
    margin = bst.predict(big, output_margin=True, device=DEV)
    err = float(np.abs(phi.sum(axis=1) - margin).max())
    print("max |sum GPU phi - GPU margin|", err, "bound", bound)
    assert err <= bound


def test_a_path_beyond_the_kernel_limit_raises():
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("B3")
    bst = _cpu_fit("deep", {"objective": "reg:linear", "max_depth": 30, "min_child_weight": 0, "lambda": 0.0},
                   c["x"], c["y"], 1)
    assert H.shap_limit() >= 12 and _longest_path(bst) > H.shap_limit()
    with pytest.raises(ValueError, match=str(H.shap_limit())):
        bst.predict(c["x"][:10], pred_contribs=True, device=DEV)
    assert bst.predict(c["x"][:10], pred_contribs=True).shape == (10, c["x"].shape[1] + 1)   # the CPU has no such limit
