"""The kernels away from nct_params_default: eps, nonlocal_weight, local_weight, wls_lambda_init, wls_alpha and cluster_num go straight into kernel arguments and
kernel dispatch, and every other GPU test leaves them at their defaults. The sets, inputs and bars are those of tests/test_params_oracle.py, which holds the CPU
oracle to tests/ref64.py on them without a device; here the kernels meet the oracle bit for bit and ref64 at the project's bars (2 ulp for T1, S1_CAP_RATIO, the
1e-12 / 1e-10 / 1e-7 short-run bars, rtol 2e-5 / atol 2e-6 for S2, KM_MARGIN, 4e-16 for the kNN weights), and the entry points that copy or forward nct_params are
held to nct_process_pair byte for byte. Each test prints its figures (fraction of each bar in use) before it asserts."""
import numpy as np
import pytest
import ref64
import synth
from test_gpu_color import _level_case
from test_gpu_vs_ref64 import _chan, _check_after_s1, _lab2bgr_of
from test_params_oracle import KM_INPUTS, KM_KS, KNN_LABELS, KNN_SIZES, LEVEL_CASES, PARAM_SETS, SET_NAMES, km_expect, knn_case
from test_ref64_oracle import S1_CAP_RATIO, _ulp_close, check_kmeans, check_knn

pytestmark = pytest.mark.gpu

# 136 896 pixels at the level: the shared-gather S1 operator and the 32 x 14 S2 tiles exist only from 100 000 pixels
BIG_CASE = (372, 368, 372, 368, (23, 23), 16, 4, "flat")
STAGE_KEYS = ("ab_local", "ab_nonlocal", "ab_up", "roughness", "ab_wls")


def _prm(name=None, **fields):
    """nct_params_default with a set of PARAM_SETS (None: none) and single fields on top"""
    import nct
    p = nct.Params.default()
    for k, v in dict(PARAM_SETS[name] if name else {}, **fields).items():
        setattr(p, k, v)
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def vgg():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


# ---------------------------------------------------------------- a. the colour stage seam
_inputs, _default_wls = {}, {}


def _level_inputs(oracle, case):
    """tests/test_gpu_color.py's level inputs (the oracle's resize, Lab conversion and kNN graph), built once per case and left unchanged"""
    if case not in _inputs:
        H, W, h, w, grid, samples, layer = case[:7]
        _inputs[case] = _level_case(20 + layer, H, W, h, w, grid, samples, oracle, len(case) > 7)
    return _inputs[case]


def _default_ab_wls(ctx, oracle, case):
    if case not in _default_wls:
        err, s, g, full, ids, ws = _level_inputs(oracle, case)
        _default_wls[case] = ctx.local_color_transfer(err, s, g, full, ids, ws, case[6], want_stages=True)[1]["ab_wls"]
    return _default_wls[case]


@pytest.mark.parametrize("name,case", [(n, c) for c in LEVEL_CASES for n in SET_NAMES] + [(n, BIG_CASE) for n in ("strong", "soft")])
def test_color_stages_with_params(ctx, oracle, name, case):
    """nct_local_color_transfer with a parameter set: every stage bit for bit the oracle's with the same set (as test_local_color_transfer_stages asserts it), another
    result than the default parameters give, and — on the four small cases — T1, S1's energy, U1, roughness, S2 and A1 against ref64 with the set's values"""
    H, W, h, w, grid, samples, layer = case[:7]
    prm = PARAM_SETS[name]
    err, s, g, full, ids, ws = _level_inputs(oracle, case)
    go, gs = ctx.local_color_transfer(err, s, g, full, ids, ws, layer, params=_prm(name), want_stages=True)
    oo, os_ = oracle.local_color_transfer(err, s, g, full, ids, ws, layer, params=dict(prm, k_num=8.0), want_stages=True)
    cap = 50 if layer == 4 else 100
    assert gs["cg_iters"].tolist() == os_["cg_iters"].tolist() == [cap] * 3
    assert gs["wls_iters"].tolist() == os_["wls_iters"].tolist() and 0 < max(gs["wls_iters"]) < 5000
    for k in STAGE_KEYS:
        assert np.array_equal(_bits(gs[k]), _bits(os_[k])), k
    assert np.array_equal(go, oo)
    assert not np.array_equal(gs["ab_wls"], _default_ab_wls(ctx, oracle, case)), "the set is meant to change S2's result on this case"
    if case is BIG_CASE:
        print("color", name, case[:4], "wls_iters", max(gs["wls_iters"]))
        return
    slab, glab, flab = (oracle.bgr2lab(x).reshape(-1, 3) / 255.0 for x in (s, g, full))
    ea, eb = ref64.local_stats(oracle.bgr2lab(s), oracle.bgr2lab(g), prm["eps"])
    assert _ulp_close(gs["ab_local"][0], ea, 2) and _ulp_close(gs["ab_local"][1], eb, 2)
    system = ref64.s1_system(slab, glab, ref64.err_weight(err), ids, ws, h, w, prm["local_weight"], prm["wls_alpha"], H * W / (h * w), nonlocal_weight=prm["nonlocal_weight"])
    ratios = []
    for c in range(3):
        A, rhs = system[c]
        x0 = _chan(gs["ab_local"], c)
        xr, _ = ref64.s1_cg(A, rhs, x0, cap)
        f0, fg, fr = (ref64.s1_objective(A, rhs, v) for v in (x0, _chan(gs["ab_nonlocal"], c), xr))
        ratios.append(fg / fr)
        assert fg <= f0, c
    stats = {}
    try:
        _check_after_s1(_lab2bgr_of(ctx), gs, go, H, W, h, w, flab, prm=prm, stats=stats)
    finally:
        print("color", name, case[:4], "S1 ratio %.4f .. %.4f" % (min(ratios), max(ratios)), "S2 worst / allowed %.3g" % stats.get("s2_frac", np.nan), "wls_iters", max(gs["wls_iters"]))
    assert S1_CAP_RATIO[0] <= min(ratios) and max(ratios) <= S1_CAP_RATIO[1], ratios


# ---------------------------------------------------------------- b. S1 short runs
@pytest.mark.parametrize("name", ["help", "soft"])
@pytest.mark.parametrize("case", [LEVEL_CASES[1], LEVEL_CASES[3]])
def test_s1_short_runs_with_params(oracle, case, name, monkeypatch):
    """NCT_S1_MAXIT = 1, 2, 5 as in test_s1_short_runs_vs_literal_cg: the GPU's S1 iterate vs ref64's literal CGNR from the GPU's own T1 guess. local_weight (0.001,
    0.03) and wls_alpha (0.8) of these sets are not floats: S1 takes both as float (ColorTransfer.cpp:548-550), and a kernel that took the double would miss the bars"""
    import nct
    H, W, h, w, grid, samples, layer = case[:7]
    prm = PARAM_SETS[name]
    err, s, g, full, ids, ws = _level_inputs(oracle, case)
    slab, glab = (oracle.bgr2lab(x).reshape(-1, 3) / 255.0 for x in (s, g))
    system = ref64.s1_system(slab, glab, ref64.err_weight(err), ids, ws, h, w, prm["local_weight"], prm["wls_alpha"], H * W / (h * w), nonlocal_weight=prm["nonlocal_weight"])
    for maxit, tol in ((1, 1e-12), (2, 1e-10), (5, 1e-7)):
        monkeypatch.setenv("NCT_S1_MAXIT", str(maxit))
        with nct.Context(0) as c:
            _, gs = c.local_color_transfer(err, s, g, full, ids, ws, layer, params=_prm(name), want_stages=True)
        assert gs["cg_iters"].tolist() == [maxit] * 3
        worst = 0.0
        for ch in range(3):
            A, rhs = system[ch]
            x, k = ref64.s1_cg(A, rhs, _chan(gs["ab_local"], ch), maxit)
            assert k == maxit
            worst = max(worst, float((np.abs(_chan(gs["ab_nonlocal"], ch) - x) / (tol + tol * np.abs(x))).max()))
        print("s1-short", name, case[:4], maxit, "worst / bar %.3g" % worst)
        assert worst <= 1.0, (maxit, worst)          # np.allclose(got, x, rtol=tol, atol=tol)


# ---------------------------------------------------------------- c. the finish alone
@pytest.mark.parametrize("name", ["strong", "soft"])
def test_color_finish_with_params(ctx, oracle, name):
    """nct_color_finish on an upsampled grid (tests/test_gpu_fullres.py's 31 x 24 level of a 61 x 47 working size onto 250 x 171) reads wls_lambda_init and wls_alpha"""
    from fullres_ref import oracle_finish, smooth_ab
    (h, w), (wh, ww), (H, W) = (31, 24), (61, 47), (250, 171)
    ab, s_full = smooth_ab(102, h, w), synth.image(202, H, W)
    prm = PARAM_SETS[name]
    bgr, exp = oracle_finish(oracle, ab, h, w, wh, ww, s_full, wls_lambda_init=prm["wls_lambda_init"], wls_alpha=prm["wls_alpha"])
    got, st = ctx.color_finish(ab, h, w, wh, ww, s_full, _prm(name), want_stages=True)
    assert list(st["wls_iters"]) == list(exp["wls_iters"]) and 0 < max(st["wls_iters"]) < 5000
    for k in ("ab_up", "roughness", "ab_wls"):
        assert np.array_equal(_bits(st[k]), _bits(exp[k])), k
    assert np.array_equal(got, bgr)
    assert not np.array_equal(st["ab_wls"], ctx.color_finish(ab, h, w, wh, ww, s_full, want_stages=True)[1]["ab_wls"])


# ---------------------------------------------------------------- d. k-means
@pytest.mark.parametrize("K", KM_KS)
@pytest.mark.parametrize("name", sorted(KM_INPUTS))
def test_kmeans_labels_with_k(ctx, oracle, name, K):
    """K on both sides of the K <= 10 dispatch edges of k_cluster.hip (k_km_init's staged rows, k_km_dist512), and K = 1: ref64's labels (check_kmeans), the oracle's
    bit for bit, a donor move on the blobs at K = 11 and 16, the one-label exit of 12 distinct vectors at K = 16"""
    f = KM_INPUTS[name]()
    m = check_kmeans(ctx.cluster_features, ctx.feat_normalize, f, 1, km_expect(name, K), K=K)
    print("kmeans", name, K, "margin %.3g" % m)
    gl, gn = ctx.cluster_features(f, K, 11, 1)
    ol, on = oracle.cluster_features(f, K, 11, 1)
    assert gn == on and np.array_equal(gl, ol)
    assert gn == (1 if km_expect(name, K) == "one" else K)


@pytest.mark.parametrize("K", [11, 16])
def test_kmeans_beyond_the_lds_list_with_k(ctx, oracle, K):
    """70 x 70 points: beyond k_km_init's LDS permutation list, with the general centre kernel. The labels are ref64's on the library's own normalised map (exact: no
    margin needed) and the oracle's; this map's margin against ref64's own normalisation (2.4e-7, 7.5e-7) lies below KM_MARGIN, so that comparison is not made"""
    f = synth.features(3, 512, 70, 70) * np.float32(5.0)
    gl, gn = ctx.cluster_features(f, K, 11, 1)
    el, en, _ = ref64.kmeans_labels(ctx.feat_normalize(f), K, 11, 1, normalized=True)
    assert gn == en == K and np.array_equal(gl, el)
    ol, on = oracle.cluster_features(f, K, 11, 1)
    assert gn == on and np.array_equal(gl, ol)


# ---------------------------------------------------------------- e. kNN graph
@pytest.mark.parametrize("nl", KNN_LABELS)
@pytest.mark.parametrize("size", KNN_SIZES)
def test_knn_graph_with_many_labels(ctx, size, nl, monkeypatch):
    """1, 11 and 16 labels against ref64: labels 10 .. 15 fill the four cluster bits of the sort key. The 120 x 110 case under both search forms (NCT_KNN_RUNS)"""
    import nct
    img, labels = knn_case(size, nl)
    lab = ctx.bgr2lab(img)
    exp = ref64.knn_graph(lab, labels, nl, size[4])
    pad, dev = check_knn(*ctx.knn_graph(lab, labels, nl, size[4]), *exp, f"{size} {nl} labels")
    print("knn", size, nl, "padded", pad, "max rel dev %.3g" % dev)
    if size[0] == 120:
        for runs in ("0", "1"):
            monkeypatch.setenv("NCT_KNN_RUNS", runs)
            with nct.Context(0) as c:
                check_knn(*c.knn_graph(lab, labels, nl, size[4]), *exp, f"{size} {nl} labels runs {runs}")


def test_knn_graph_label_15_fine_cells(ctx):
    """103 680 pixels: the 2-unit cells and the two-stage start table, whose last sixteenth belongs to cluster 15; every inner cell of the label grid is in 5 clusters"""
    size, nl = (320, 324, 20, 21, 16), 16
    img, labels = knn_case(size, nl)
    member = ref64.cluster_members(labels, nl)
    assert member.sum(0).max() == 5 and member[15].any()
    lab = ctx.bgr2lab(img)
    pad, dev = check_knn(*ctx.knn_graph(lab, labels, nl, size[4]), *ref64.knn_graph(lab, labels, nl, size[4]), str(size))
    print("knn", size, nl, "cells of cluster 15:", int(member[15].sum()), "padded", pad, "max rel dev %.3g" % dev)


# ---------------------------------------------------------------- f. the whole pair
PAIR_SRC, PAIR_REF = (1000, 64, 72), (1001, 72, 64)          # the coarsest grid is 4 x 5 = 20 points, at least 16
PAIR_PARAMS = [("help", {}), ("soft", dict(cluster_num=13)), (None, dict(cluster_num=1)), (None, dict(cluster_num=3)), (None, dict(cluster_num=16))]


@pytest.mark.parametrize("name,fields", PAIR_PARAMS, ids=["help", "soft-13", "K1", "K3", "K16"])
def test_pair_levels_with_params(ctx, oracle, vgg, name, fields):
    """nct_pair_run_levels: every level's result and the k-means labels are the oracle's with the same parameters (orc_process_pair_levels) — no parameter is dropped
    between nct_params and the level loop's kernels"""
    src, ref = synth.image_flat(*PAIR_SRC), synth.image_flat(*PAIR_REF)
    ctx.vgg19_load_raw(*vgg)
    ctx.pair_upload(src, ref)
    lv = ctx.pair_run_levels(src.shape, ref.shape, _prm(name, **fields), want_color=True)
    K = fields.get("cluster_num", 10)
    _, olv = oracle.process_pair(src, ref, *vgg, dict(PARAM_SETS[name] if name else {}, **fields), want_levels=True)
    for l in range(5):
        assert np.array_equal(lv["result"][l], olv[l]), f"level {l}"
    assert np.array_equal(ctx.pair_download(), olv[4])
    ol, on = oracle.cluster_features(oracle.vgg19_features(src, *vgg, 5)[4], K, 11, 1)
    assert lv["labels"].shape == (4, 5) and np.array_equal(lv["labels"], ol) and int(lv["labels"].max()) + 1 == on


# ---------------------------------------------------------------- g. plumbing identities
def test_every_entry_point_forwards_the_params(ctx, vgg):
    """soft with cluster_num 13 through the entry points that copy or forward nct_params — frame 0 of a sequence (nct_seq_begin keeps a copy), nct_process_multi with one
    reference, nct_process_pair_fullres on a source that needs no shrinking: the bytes of nct_process_pair with the same parameters, not those of the defaults"""
    src, ref = synth.image_flat(*PAIR_SRC), synth.image_flat(*PAIR_REF)
    ctx.vgg19_load_raw(*vgg)
    prm = _prm("soft", cluster_num=13)
    base, exp = ctx.process_pair(src, ref), ctx.process_pair(src, ref, prm)
    assert not np.array_equal(exp, base), "the parameters are meant to change this pair's result"
    ctx.seq_begin(ref, src.shape, prm)
    try:
        frame0 = ctx.seq_frame(src)
    finally:
        ctx.seq_end()
    for what, got in (("seq frame 0", frame0), ("process_multi", ctx.process_multi(src, [ref], prm)), ("process_pair_fullres", ctx.process_pair_fullres(src, ref, 1000, prm))):
        assert np.array_equal(got, exp), what
