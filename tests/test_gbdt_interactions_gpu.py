"""SHAP interaction values on MI355X: the kernel of csrc/hip/gbdt_shap_inter.hip against the CPU predictor, bit
for bit, on the smallest shapes that reach each of its paths: chunk and block tails, K > 1, feature-axis splits
from one owner of all features to one owner per feature, tables in LDS chunks or from global memory, merged
elements, depth 0, and the two refusals. The boosters are those of test_gbdt_explain_gpu.py (trained once per session)."""

import numpy as np
import pytest

import gbdt_stage_cases as cases
from test_gbdt_explain import fit as small_fit, leaf_scale, mixed_rows
from test_gbdt_explain_gpu import _cpu_fit, _fresh, _gpu_fit, _longest_path, _table_bytes
from test_gbdt_interactions import check_structure, oracle_interactions, twelve_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TABLE_BYTES = 16 * 1024          # SI_TABLE_BYTES of gbdt_shap_inter.hip


def _same_on_both(bst, x, **kw):
    cpu = bst.predict(x, pred_interactions=True, **kw)
    gpu = bst.predict(x, pred_interactions=True, device=DEV, **kw)
    F1 = x.shape[1] + 1
    assert cpu.dtype == gpu.dtype == np.float64 and cpu.shape == gpu.shape
    assert cpu.shape == ((len(x), F1, F1) if bst.K == 1 else (len(x), bst.K, F1, F1))
    assert cpu.tobytes() == gpu.tobytes(), (kw, x.shape)
    return gpu


def test_interactions_chunk_and_block_tails_three_classes(monkeypatch):
    """n = 703 with 300-row uploads (a chunk tail of 103 rows, block tails of 44 and 103), K = 3, ntree_limit,
    n = 1; a GPU-trained and a CPU-trained booster."""
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("E")
    monkeypatch.setattr(H, "PREDICT_CHUNK_ROWS", 300)
    assert H.shap_inter_plan(703, 9, 3) == (300, 8)
    for bst in (_gpu_fit("E"), _cpu_fit("E", c["params"], c["x"], c["y"], 3)):
        assert bst.K == 3
        _same_on_both(bst, c["x"][:703])
        _same_on_both(bst, c["x"][:703], ntree_limit=2)
        _same_on_both(bst, c["x"][:1])


def test_interactions_five_features():
    """F = 5: fewer features than the split would otherwise take (S = 4, owners of unequal size)."""
    from gentun_amd.models import gbdt_hip as H
    x, y = cases._reg(1000, 5, 11)
    x = np.ascontiguousarray(x, np.float32)
    bst = _cpu_fit("F5", {"objective": "reg:linear", "max_depth": 3}, x, y, 3)
    assert bst.num_rounds == 3 and H.shap_inter_plan(257, 5) == (257, 4)
    rows = _fresh(5, 2, n=257)
    check_structure(bst, rows, _same_on_both(bst, rows), device=DEV)


def test_interactions_several_table_chunks():
    c = cases.load("B3")
    bst = _cpu_fit("B3x40", {"objective": "reg:linear", "max_depth": 6, "eta": 0.1}, c["x"], c["y"], 40)
    sizes = [_table_bytes(bst, t) for t in range(bst.num_trees)]
    assert c["x"].shape[1] == 33 and max(sizes) <= TABLE_BYTES and sum(sizes) > 3 * TABLE_BYTES
    _same_on_both(bst, c["x"][:600])
    _same_on_both(bst, c["x"][:600], ntree_limit=17)


@pytest.mark.parametrize("split", [1, 2, 16])
def test_interactions_do_not_depend_on_the_split(split):
    """The splits the small cases do not choose by themselves, forced: one owner of everything (what a launch with
    enough rows runs), two, sixteen."""
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("B3")
    bst = _cpu_fit("B3x40", {"objective": "reg:linear", "max_depth": 6, "eta": 0.1}, c["x"], c["y"], 40)
    rows = np.ascontiguousarray(np.concatenate([c["x"][:200], _fresh(33, 9, n=57)]))
    want = bst.predict(rows, pred_interactions=True, ntree_limit=5)
    got = np.empty((len(rows), 1, 34, 34), np.float64)
    H.predict_interactions(bst, rows, 5, got, split=split)
    assert got.tobytes() == want.tobytes()


def test_interactions_paths_of_twelve_unique_features():
    """33 features, depth 16: paths with 12 or more unique features, inside the kernel's limit; the tree's tables
    also exceed the chunk budget."""
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("B3")
    bst = _cpu_fit("deep16", {"objective": "reg:linear", "max_depth": 16, "min_child_weight": 0, "lambda": 0.0},
                   c["x"], c["y"], 1)
    assert 12 <= _longest_path(bst) <= H.shap_inter_limit() and _table_bytes(bst, 0) > TABLE_BYTES
    _same_on_both(bst, c["x"][:300])


def test_interactions_256_features():
    """Bench width, 150 rows = 79 MB per output: two row blocks only, so the widest feature-axis split; the whole
    input is one device chunk until 508 rows."""
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("A")
    assert c["x"].shape[1] == 256
    assert H.shap_inter_plan(150, 256) == (150, 256) and H.shap_inter_plan(600, 256) == (508, 256)
    assert H.shap_inter_plan(20000, 32) == (20000, 8) and H.shap_inter_plan(1 << 17, 8) == (1 << 17, 1)
    bst = _cpu_fit("A", c["params"], c["x"], c["y"], 2)
    _same_on_both(bst, c["x"][:150])


def test_interactions_tree_beyond_the_table_budget():
    c = cases.load("H12")
    bst = _gpu_fit("H12")
    assert _table_bytes(bst, 0) > TABLE_BYTES and _longest_path(bst) == 6      # read from global memory
    _same_on_both(bst, c["x"][:300])


def test_interactions_depth_zero():
    c = cases.load("G0")
    bst = _gpu_fit("G0")
    assert np.all(np.diff(bst.tree_offsets) == 1)
    got = _same_on_both(bst, c["x"][:300])
    F = c["x"].shape[1]
    assert np.all(got[:, F, F] == bst.predict(c["x"][:300], pred_contribs=True, device=DEV)[:, F])
    got[:, F, F] = 0.0
    assert np.all(got == 0.0)


def test_interactions_merged_elements_oracle_and_additivity():
    """The 2-feature depth-5 model (paths repeat a feature), F = 8: the GPU output against the brute-force oracle
    with the CPU test's bound; row sums against the GPU contributions, the total against the GPU margins."""
    x, _y, bst = small_fit("two")
    rows = twelve_rows(x, 5)
    got = _same_on_both(bst, rows)
    want = oracle_interactions(bst, rows)[:, 0]
    bound = 1e-12 * leaf_scale(bst)
    err = float(np.abs(got - want).max())
    print("max |GPU Phi - oracle|", err, "bound", bound)
    assert err <= bound
    big = np.concatenate([x[:400], mixed_rows(x, 7)])
    check_structure(bst, big, _same_on_both(bst, big), device=DEV)


def test_a_path_beyond_the_kernel_limit_raises():
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("B3")
    bst = _cpu_fit("deep", {"objective": "reg:linear", "max_depth": 30, "min_child_weight": 0, "lambda": 0.0},
                   c["x"], c["y"], 1)
    assert H.shap_inter_limit() >= 12 and _longest_path(bst) > H.shap_inter_limit()
    with pytest.raises(ValueError, match="more than {} unique".format(H.shap_inter_limit())):
        bst.predict(c["x"][:10], pred_interactions=True, device=DEV)


def test_a_row_beyond_the_buffer_bound_raises():
    from gentun_amd.models import gbdt_hip as H
    c = cases.load("I")
    assert c["x"].shape[1] == 8200 and H.shap_inter_plan(1, 8200) is None
    bst = _cpu_fit("I", c["params"], c["x"], c["y"], 2)
    with pytest.raises(ValueError, match="CPU predictor"):
        bst.predict(c["x"][:2], pred_interactions=True, device=DEV)
    cpu = bst.predict(c["x"][:2], pred_contribs=True)
    assert bst.predict(c["x"][:2], pred_contribs=True, device=DEV).tobytes() == cpu.tobytes()


def test_existing_outputs_are_unchanged_by_an_interactions_call():
    c = cases.load("E")
    bst = _gpu_fit("E")
    x = c["x"][:500]
    before = (bst.predict(x, pred_contribs=True, device=DEV), bst.predict(x, output_margin=True, device=DEV))
    bst.predict(x, pred_interactions=True, device=DEV)
    after = (bst.predict(x, pred_contribs=True, device=DEV), bst.predict(x, output_margin=True, device=DEV))
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
