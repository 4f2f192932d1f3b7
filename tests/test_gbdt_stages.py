"""Stage-by-stage oracle of the GPU GBDT engine (csrc/hip/gbdt_hist.hip) through its trace hook
(gbdt_cv_hip_trace, gentun_amd.models.gbdt_hip.cv_trace): after every stage of the traced rounds the
engine's buffers are compared with the plain numpy reference tests/gbdt_stage_ref.py evaluated on that
stage's *traced input*. Integers (fixed-point gradients, histograms, prefix sums, children totals, row
sets, chunk lists, rank sums) and fp32 results with one rounding (squared-error gradients, leaves,
margins) are compared for equality; fp32 transcendental code (logistic / softmax gradients, metric
terms) against fp64 within a bound pinned at 4x the error measured on MI355X
(profiles/gbdt_stage_oracle.txt). Cases: tests/gbdt_stage_cases.py."""

import math

import numpy as np
import pytest

import gbdt_stage_cases as cases
import gbdt_stage_ref as ref

pytestmark = pytest.mark.gpu

GB_R = 16384
# 4x the largest error measured on MI355X per case (profiles/gbdt_stage_oracle.txt), ceilings 1e-6 (gradients,
# absolute: g, h lie in [-spw, spw]) and 1e-5 (metric sums, relative)
GRAD_BOUND = {"C": 4.3e-7, "E": 3.4e-7, "J3": 2.3e-7, "J32": 0.0}       # J32: one round from margin 0, p = 0.5 exactly
METRIC_BOUND = {"A": 5.1e-8, "B4": 9.4e-8, "B3": 3.2e-8, "C": 3.4e-7, "D": 8.5e-8, "E": 1.6e-7, "F1": 2.3e-8,
                "F2": 5.8e-8, "G0": 9.1e-8, "Gz": 0.0, "H10": 2.4e-8, "H12": 1.6e-8, "I": 7.1e-8}
MEASURED = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_lists(k, d, LN, CH, RD, nch, nrd, expect_lists):
    """Every built node is covered exactly once by chunks of <= GB_R rows; partial slots are disjoint and
    numbered in node order; reductions name their node's slot range."""
    built = [j for j in range(len(LN)) if LN["exists"][j] and LN["built"][j]] if expect_lists else []
    want_ch, want_rd, nslot = [], [], 0
    for j in built:
        s, cnt = int(LN["start"][j]), int(LN["count"][j])
        if cnt <= GB_R:
            want_ch.append((j, s, cnt, -1))
            continue
        first = nslot
        for o in range(0, cnt, GB_R):
            want_ch.append((j, s + o, min(GB_R, cnt - o), nslot))
            nslot += 1
        want_rd.append((j, first, nslot - first))
    assert nch == len(want_ch) and nrd == len(want_rd), (k, d, nch, nrd, len(want_ch), len(want_rd))
    got_ch = [tuple(int(v) for v in CH[i]) for i in range(nch)]
    got_rd = [tuple(int(RD[f][i]) for f in ("node", "first", "nslots")) for i in range(nrd)]
    assert got_ch == want_ch, (k, d, got_ch[:4], want_ch[:4])
    assert got_rd == want_rd, (k, d, got_rd, want_rd)
    for (_j, _s, cnt, _slot) in got_ch:
        assert cnt <= GB_R
    return nslot


def _run(name):
    from gentun_amd.models import gbdt_hip as H
    c = cases.load(name)
    x, y, fold_of, nf, parr = c["x"], c["y"], c["fold_of"], c["nfold"], c["parr"]
    p = ref.pdict(parr)
    n, F = x.shape
    obj = c["obj"]
    K = max(2, c["num_class"]) if obj >= 4 else 1
    kind = 3 if obj >= 4 else (0 if obj == 0 else (1 if obj == 1 else 2))
    hconst = kind == 0
    D = max(0, min(int(p["max_depth"]), 12))
    Lmax, Lh, tsz = 1 << D, 1 << max(0, D - 1), (2 << D) - 1
    maxch = (n + GB_R - 1) // GB_R + Lh + 2
    nm = len(c["marr"])
    tags = [t for t in H.TRACE_TAGS if c["heavy"] or t not in H.TRACE_HEAVY]
    hist_t = np.zeros((c["rounds"], nm, 4))
    kept_t, T = H.cv_trace(x, y, fold_of, nf, parr, obj, c["num_class"], c["marr"], c["rounds"], 0, c["seed"], hist_t,
                           trace_rounds=c["traced"], tags=tags)
    assert kept_t == c["rounds"]
    # untraced equals traced: same history, same return value, bit for bit
    hist_u = np.zeros_like(hist_t)
    kept_u = H.cv(x, y, fold_of, nf, parr, obj, c["num_class"], c["marr"], c["rounds"], 0, c["seed"], hist_u)
    assert kept_u == kept_t and hist_u.tobytes() == hist_t.tobytes()
    nb, key, fs = H.quantize_device(x)
    bins = np.ascontiguousarray(H.device_bins(x, key, fs)[:, :F])
    base = p["base_score"]
    if obj in (1, 2):
        b = min(1 - 1e-7, max(1e-7, base))
        base = math.log(b / (1 - b))
    meas = {"grad": 0.0, "metric": 0.0, "split_nodes": 0, "ambiguous": 0, "grid": c["grid"]}
    prev_after = np.full((nf, n, K), np.float32(base), np.float32)
    for rnd in range(c["traced"]):
        for cl in range(K):
            g = lambda tag, d=-1: T[(rnd, cl, d, tag)]          # noqa: E731
            before = g("MARGIN", -2).reshape(nf, n, K)
            after = g("MARGIN").reshape(nf, n, K)
            assert np.array_equal(_bits(before), _bits(prev_after))
            prev_after = after
            GH = g("GH").reshape(nf, n, 2)
            MX = g("MX").reshape(nf, 2).view(np.float32)
            KEYS, ORDER = g("KEYS"), g("ORDER").reshape(nf, D + 1, F)
            root = g("ROOT")
            nroot, rows0 = root[:nf], root[nf:].reshape(nf, n)
            TREE = np.stack([g("TREE")["x"], g("TREE")["y"]], axis=1).reshape(nf, tsz, 2).astype(np.int64)
            LEAF = g("LEAF").reshape(nf, tsz)
            for k in range(nf):
                # ---- draws, gradients, scale, root rows
                key_ref, levels_ref = ref.tree_draws(c["seed"], k, rnd, cl, F, D, p)
                assert int(KEYS[k]) == key_ref
                feats = [ref.order_to_feats(ORDER[k, d]) for d in range(D + 1)]
                assert feats == levels_ref
                g32, h32 = GH[k, :, 0], GH[k, :, 1]
                if kind == 0:
                    assert np.array_equal(_bits(g32), _bits(before[k, :, 0] - y)) and np.all(h32 == 1.0)
                else:
                    gr, hr = ref.grad(before[k], y, kind, cl, p["scale_pos_weight"])
                    err = max(float(np.max(np.abs(g32 - gr))), float(np.max(np.abs(h32 - hr))))
                    meas["grad"] = max(meas["grad"], err)
                    assert err <= GRAD_BOUND[name], (k, err)
                mg, mh, se_g, se_h = ref.scale(g32, h32, n, hconst)
                assert _bits(MX[k]).tolist() == _bits([mg, mh]).tolist()
                ig, ih = 2.0 ** -se_g, 2.0 ** -se_h
                qg, qh = ref.quantise(g32, se_g), ref.quantise(h32, se_h)
                rr = ref.root_rows(fold_of, k, key_ref, p["subsample"])
                assert int(nroot[k]) == len(rr)
                assert np.array_equal(np.sort(rows0[k, :len(rr)]), rr)
                # ---- levels
                rows_d = rows0[k]
                for d in range(D + 1):
                    L = 1 << d
                    LN = g("LNODES", d).reshape(nf, Lmax)[k][:L]
                    if d == 0:
                        assert (LN["start"][0], LN["count"][0], LN["exists"][0], LN["built"][0]) == (0, len(rr), 1, 1)
                        assert int(LN["G"][0]) == int(qg[rr].sum()) and int(LN["H"][0]) == int(qh[rr].sum())
                    else:
                        assert LN.tobytes() == g("NXT", d - 1).reshape(nf, Lmax)[k][:L].tobytes()
                    cnts = g("COUNTS", d).reshape(nf, 2)[k]
                    _check_lists(k, d, LN, g("CHUNKS", d).reshape(nf, maxch)[k], g("REDS", d).reshape(nf, maxch)[k],
                                 int(cnts[0]), int(cnts[1]), d == 0 or d < D)
                    has_hist = d < D or d == 0
                    Hd = g("HIST", d).reshape(nf, Lh, F, 256, 2)[k] if (c["heavy"] and has_hist) else None
                    if d < D:
                        BEST = g("BEST", d).reshape(nf, Lh)[k]
                        CAND = g("CAND", d).reshape(nf, Lh, F)[k] if c["heavy"] else None
                        NX = g("NXT", d).reshape(nf, Lmax)[k][:2 * L]
                        out = g("ROWS", d).reshape(nf, n)[k]
                        ends = NX["start"].astype(np.int64) + NX["count"]
                        assert np.all(np.diff(ends) >= 0)
                    SP = g("SPLITV", d).reshape(nf, Lmax)[k][:L]
                    for j in range(L):
                        nd = LN[j]
                        nid = L - 1 + j
                        if not nd["exists"]:
                            assert nd["count"] == 0 and (SP["x"][j], SP["y"][j]) == (-1, 0)
                            if d < D:
                                for ch in (NX[2 * j], NX[2 * j + 1]):
                                    assert (ch["exists"], ch["count"], ch["start"]) == (0, 0, nd["start"])
                            continue
                        seg = rows_d[nd["start"]:nd["start"] + nd["count"]]
                        G, Hh = int(nd["G"]), int(nd["H"])
                        assert _bits(LEAF[k, nid]) == _bits(ref.leaf_value(p, G, Hh, ig, ih)), (k, d, j)
                        href = None
                        if has_hist and (Hd is not None or (d < D and nd["count"] >= 2)):
                            href = ref.hist(bins, seg, qg, qh)
                        if Hd is not None and (nd["built"] or d + 1 < D):
                            assert np.array_equal(Hd[j], href), (k, d, j)        # built nodes, subtracted siblings
                        split = False
                        if d < D and nd["count"] >= 2:
                            s = ref.scan(href, G, Hh, feats[d], nb, p, ig, ih)
                            B = BEST[j]
                            bf, bb = int(B["feature"]), int(B["bin"])
                            if s is None:
                                assert bf < 0, (k, d, j, B)
                            else:
                                assert bf >= 0 and bb >= 0, (k, d, j, s["feature"], s["bin"], s["gain"])
                                pre = np.cumsum(href[bf, :bb + 1], axis=0)[-1]
                                assert (int(B["GL"]), int(B["HL"])) == (int(pre[0]), int(pre[1])), (k, d, j)
                                gref = s["gains"][bf][bb]
                                assert abs(float(B["gain"]) - gref) <= s["tol"], (k, d, j, B["gain"], gref)
                                if s["gap"] >= s["tol"]:
                                    assert (bf, bb) == (s["feature"], s["bin"]), (k, d, j, bf, bb, s["feature"],
                                                                                  s["bin"], s["gap"], s["tol"])
                                else:
                                    meas["ambiguous"] += 1
                                    assert abs(gref - s["gain"]) <= s["tol"]
                                if CAND is not None:
                                    cb = CAND[j][bf]
                                    assert (cb["gain"], cb["GL"], cb["HL"], cb["bin"]) == (B["gain"], B["GL"], B["HL"], bb)
                                    assert np.array_equal(CAND[j]["order"], ORDER[k, d] - 1)
                                    assert np.all(CAND[j]["bin"][ORDER[k, d] == 0] == -1)
                                    for f in (feats[d] if F <= 64 else ()):   # every feature's own scan
                                        sf, cf = ref.scan(href, G, Hh, [f], nb, p, ig, ih), CAND[j][f]
                                        if sf is None:
                                            assert cf["bin"] == -1, (k, d, j, f)
                                        elif sf["gap"] >= sf["tol"]:
                                            assert (cf["bin"], int(cf["GL"]), int(cf["HL"])) == \
                                                (sf["bin"], int(sf["GL"]), int(sf["HL"])), (k, d, j, f)
                            split = ref.keeps_split(p, bf, bb, float(B["gain"]))
                        want_sp = (bf, bb) if split else (-1, 0)
                        assert (int(SP["x"][j]), int(SP["y"][j])) == want_sp, (k, d, j)
                        assert tuple(TREE[k, nid]) == want_sp, (k, d, j)
                        if d == D:
                            continue
                        l, r = NX[2 * j], NX[2 * j + 1]
                        if not split:
                            end = nd["start"] + nd["count"]
                            for ch in (l, r):
                                assert (ch["exists"], ch["count"], ch["start"]) == (0, 0, end)
                            continue
                        meas["split_nodes"] += 1
                        lrows, rrows = ref.partition(bins, seg, bf, bb)
                        lc, rc = len(lrows), len(rrows)
                        assert (l["exists"], r["exists"], l["parent"], r["parent"]) == (1, 1, j, j)
                        assert (l["start"], l["count"], r["start"], r["count"]) == (nd["start"], lc, nd["start"] + lc, rc), \
                            (rnd, cl, k, d, j, l, r)
                        assert (int(l["G"]), int(l["H"])) == (int(B["GL"]), int(B["HL"]))
                        assert (int(r["G"]), int(r["H"])) == (G - int(B["GL"]), Hh - int(B["HL"]))
                        assert (int(l["G"]), int(l["H"])) == (int(qg[lrows].sum()), int(qh[lrows].sum()))
                        assert (l["built"], r["built"]) == ((1, 0) if lc <= rc else (0, 1)), (k, d, j, lc, rc)
                        assert np.array_equal(np.sort(out[l["start"]:l["start"] + lc]), np.sort(lrows)), (k, d, j)
                        assert np.array_equal(np.sort(out[r["start"]:r["start"] + rc]), np.sort(rrows)), (k, d, j)
                    if d < D:
                        rows_d = out
                # ---- predict: every row of the fold (test and unsampled rows too), only class cl's column
                leaf_of = ref.walk(bins, TREE[k], D)
                want = before[k].copy()
                want[:, cl] = before[k][:, cl] + LEAF[k][leaf_of]
                assert np.array_equal(_bits(after[k]), _bits(want)), (k, rnd, cl)
                if name == "Gz":
                    assert tuple(TREE[k, 0]) == (-1, 0) and LEAF[k, 0] == 0          # -0.0: -(0) / (H + lambda)
                    assert np.array_equal(_bits(after[k]), _bits(before[k]))
        # ---- metrics on the round's traced margins
        mblocks = min((n + 255) // 256, 256)
        MET = T[(rnd, -1, -1, "MET")].reshape(nm, nf, mblocks, 4).sum(axis=2)
        for mi, met in enumerate(int(m) for m in c["marr"]):
            for k in range(nf):
                for q, rows in enumerate((np.nonzero(fold_of != k)[0], np.nonzero(fold_of == k)[0])):
                    if met == 4:
                        a = T[(rnd, -1, -1, "AUC")].reshape(nf, 4)[k]
                        rs, npos, _nneg = ref.auc_sums(prev_after[k][rows, 0], y[rows])
                        assert (float(a[2 * q]), float(a[2 * q + 1])) == (rs, float(npos)), (k, q)
                        continue
                    terms = ref.metric_terms(met, obj, prev_after[k][rows], y[rows])
                    got, cnt = float(MET[mi, k, 2 * q]), float(MET[mi, k, 2 * q + 1])
                    assert cnt == len(rows)
                    want = float(np.sum(terms))
                    if met in (3, 5):
                        assert got == want, (met, k, q)
                    else:
                        err = abs(got - want) / max(abs(want), 1e-300) if want != 0 else abs(got)
                        meas["metric"] = max(meas["metric"], err)
                        assert err <= METRIC_BOUND[name], (met, k, q, got, want)
    MEASURED[name] = meas
    print("case {}: grid {} ({}a multiple of 8); max |grad error| {:.3e}; max metric rel. error {:.3e}; "
          "{} split nodes, {} ambiguous".format(name, c["grid"], "" if c["grid"] % 8 == 0 else "not ", meas["grad"],
                                                meas["metric"], meas["split_nodes"], meas["ambiguous"]))
    assert meas["ambiguous"] <= 0.01 * meas["split_nodes"]


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_stage_oracle(name):
    _run(name)
