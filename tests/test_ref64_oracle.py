"""The CPU oracle vs tests/ref64.py, the float64 restatements written from the reference's text: whole maps, odd and elongated sizes, A != B, flat images, NaN
and constant error maps, hub-heavy kNN graphs. The GPU parity tests compare the kernels with the oracle bit for bit, so what these pin, the kernels inherit;
tests/test_gpu_vs_ref64.py checks the kernels against ref64 directly."""
import numpy as np
import pytest
import ref64
import synth
from test_gpu_color import _level_case

SIZES = [(17, 17), (17, 400), (31, 23), (113, 170)]
# (A size, B size): A != B in both directions, elongated, and the odd ratios of the pyramid
AB_SIZES = [((17, 17), (31, 23)), ((31, 23), (17, 17)), ((17, 400), (23, 31)), ((113, 170), (57, 85))]


def _nnf(kind, seed, ah, aw, bh, bw):
    """random: uniform matches; collapsed: every pixel matches one of two B pixels (many-source completeness targets); border: matches on B's outer ring,
    where most patch taps fall outside B."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return synth.random_nnf(seed, ah, aw, bh, bw)
    if kind == "collapsed":
        pts = np.array([[bh // 2, bw // 3], [0, bw - 1]])
        p = pts[rng.integers(0, 2, (ah, aw))]
        return ((p[..., 0].astype(np.uint32) << 12) | p[..., 1].astype(np.uint32))
    side = rng.integers(0, 4, (ah, aw))
    t = rng.random((ah, aw))
    y = np.where(side == 0, 0, np.where(side == 1, bh - 1, (t * bh).astype(int)))
    x = np.where(side == 2, 0, np.where(side == 3, bw - 1, (t * bw).astype(int)))
    return (y.astype(np.uint32) << 12) | x.astype(np.uint32)


def _ulp_close(got, exp, ulps):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    return np.all(np.abs(got - exp) <= ulps * np.spacing(np.maximum(np.abs(exp), np.abs(got))))


# ---------------------------------------------------------------- N2, P1, B2, B1
@pytest.mark.parametrize("dims", [(17, 17, 31, 23, 9, 9), (17, 400, 23, 31, 9, 200), (31, 23, 17, 17, 16, 12), (113, 170, 57, 85, 57, 85), (35, 47, 29, 61, 17, 23)])
def test_nnf_upsample(oracle, dims):
    ah, aw, bh, bw, hh, hw = dims
    half = synth.random_nnf(dims[0] + dims[1], hh, hw, (bh + 1) // 2, (bw + 1) // 2)
    assert np.array_equal(oracle.nnf_upsample(half, ah, aw, bh, bw), ref64.nnf_upsample(half, ah, aw, bh, bw))


@pytest.mark.parametrize("C", [3, 64, 512])
@pytest.mark.parametrize("kind", ["random", "collapsed", "border"])
def test_patch_distance(oracle, C, kind):
    """PatchMatch with no iterations returns the distance of the initial NNF at every pixel: minus the mean over the taps inside both maps of the dot product."""
    for i, ((ah, aw), (bh, bw)) in enumerate(AB_SIZES[:3] if C == 512 else AB_SIZES):
        a = oracle.feat_normalize(synth.features(2 + i, C, ah, aw))
        b = oracle.feat_normalize(synth.features(3 + i, C, bh, bw))
        nnf = _nnf(kind, 4 + i, ah, aw, bh, bw)
        _, d = oracle.patchmatch(a, b, nnf, iters=0, rs_max=4, seed=1)
        assert np.abs(d - ref64.patch_distance(a, b, nnf)).max() <= 1e-5, (ah, aw, bh, bw)
        if (ah, aw) == (bh, bw) or i == 0:
            bb = b if (ah, aw) == (bh, bw) else a[::-1].copy()
            assert np.abs(oracle.feature_distance(a, bb) - ref64.feature_distance(a, bb)).max() <= 1e-5


@pytest.mark.parametrize("C", [3, 64, 512])
@pytest.mark.parametrize("weights", [(1.0, 2.0), (2.0, 1.0)])
def test_vote_features(oracle, C, weights):
    wc, wp = weights
    for i, ((ah, aw), (bh, bw)) in enumerate(AB_SIZES[:2] if C == 512 else AB_SIZES):
        pin = synth.features(7 + i, C, bh, bw)
        for kind in ("random", "collapsed", "border"):
            ann = _nnf(kind, 10 + i, ah, aw, bh, bw)
            bnn = _nnf("random" if kind == "collapsed" else kind, 20 + i, bh, bw, ah, aw)
            got, gpw = oracle.bds_vote_features(ann, bnn, pin, wc, wp, want_pw=True)
            exp, epw = ref64.vote_features(ann, bnn, pin, wc, wp)
            assert np.allclose(got, exp, rtol=1e-5, atol=1e-6), (kind, ah, aw, bh, bw)
            assert np.allclose(gpw, epw, rtol=1e-5, atol=1e-9), (kind, ah, aw, bh, bw)


def _vote_image_agrees(got, exp, v):
    """exact, except where the float64 value lies within 1e-4 of an integer (where the sum order can decide the truncation)"""
    near = np.abs(v - np.round(v)) < 1e-4
    return not np.any((got != exp) & ~near)


@pytest.mark.parametrize("weights", [(1.0, 2.0), (2.0, 1.0)])
def test_vote_image(oracle, weights):
    wc, wp = weights
    for i, ((ah, aw), (bh, bw)) in enumerate(AB_SIZES):
        a, b = synth.image(30 + i, ah, aw), synth.image(40 + i, bh, bw)
        for kind in ("random", "collapsed", "border"):
            ann = _nnf(kind, 50 + i, ah, aw, bh, bw)
            bnn = _nnf("random" if kind == "collapsed" else kind, 60 + i, bh, bw, ah, aw)
            got = oracle.bds_vote_image(a, b, ann, bnn, wc, wp)
            exp, v = ref64.vote_image(a, b, ann, bnn, wc, wp, want_float=True)
            assert _vote_image_agrees(got, exp, v), (kind, ah, aw, bh, bw)


# ---------------------------------------------------------------- T1, T2
@pytest.mark.parametrize("hw", SIZES)
def test_local_stats(oracle, hw):
    h, w = hw
    for mk in (synth.image, synth.image_flat):
        s, g = oracle.bgr2lab(mk(1, h, w)), oracle.bgr2lab(mk(2, h, w))
        for eps in (0.6, 0.01):
            ga, gb = oracle.local_stats(s, g, eps)
            ea, eb = ref64.local_stats(s, g, eps)
            assert _ulp_close(ga, ea, 2) and _ulp_close(gb, eb, 2), (mk.__name__, eps)
    flat = np.full((h, w, 3), (120, 40, 200), np.uint8)                      # variance 0 everywhere: a = sigma_g / eps
    g = oracle.bgr2lab(synth.image(3, h, w))
    for (s1, g1) in ((flat, g), (g, flat), (flat, flat)):
        ga, gb = oracle.local_stats(s1, g1, 0.6)
        ea, eb = ref64.local_stats(s1, g1, 0.6)
        assert _ulp_close(ga, ea, 2) and _ulp_close(gb, eb, 2)


def test_err_weight(oracle):
    rng = np.random.default_rng(4)
    e = -rng.random((31, 23)).astype(np.float32)
    maps = [e, np.full((17, 17), -0.25, np.float32)]                       # a constant map: 0 / 0 -> NaN -> 1e-6 everywhere
    en = e.copy(); en[3:6, 4:9] = np.nan; en[0, 0] = np.nan; en[-1, -1] = np.nan
    maps.append(en)
    for m in maps:
        assert np.array_equal(oracle.err_weight(m), ref64.err_weight(m))
    assert np.all(ref64.err_weight(maps[1]) == 1e-6)
    assert np.all(ref64.err_weight(en)[np.isnan(en).reshape(-1)] == 1e-6)


# ---------------------------------------------------------------- S1
# (H, W, h, w, label grid, samples, layer, flat)
S1_CASES = [(48, 48, 12, 12, (3, 3), 4, 2, False), (34, 800, 17, 400, (2, 20), 4, 3, False), (62, 46, 31, 23, (3, 3), 4, 1, False),
            (96, 96, 48, 48, (3, 3), 16, 3, True), (64, 64, 64, 64, (4, 4), 16, 4, True)]


def _s1_case(oracle, case, seed=21):
    H, W, h, w, grid, samples, layer, flat = case
    err, s, g, full, ids, ws = _level_case(seed, H, W, h, w, grid, samples, oracle, flat)
    slab = oracle.bgr2lab(s).reshape(-1, 3) / 255.0
    glab = oracle.bgr2lab(g).reshape(-1, 3) / 255.0
    return err, s, g, full, ids, ws, slab, glab


@pytest.mark.parametrize("case", S1_CASES)
def test_s1_short_iterations(oracle, case):
    """maxit 1, 2, 5: the oracle's canonical recurrence (what the kernels reproduce) vs the literal CGNR on ref64's assembled A, from the same x0. Before the
    truncated CG's chaos sets in they agree to rounding (test_canonical_cg_matches_explicit_for_few_iterations shows the same for the oracle's two forms)."""
    H, W, h, w, grid, samples, layer, flat = case
    err, s, g, full, ids, ws, slab, glab = _s1_case(oracle, case)
    if flat:
        assert np.bincount(ids.reshape(-1)).max() > 64
    wgt = ref64.err_weight(err)
    nf = H * W / (h * w)
    x0 = np.stack(oracle.local_stats(oracle.bgr2lab(s), oracle.bgr2lab(g), 0.6))
    system = ref64.s1_system(slab, glab, wgt, ids, ws, h, w, 0.125, 1.2, nf)
    for maxit, tol in ((1, 1e-12), (2, 1e-10), (5, 1e-7)):
        ab, it = oracle.nonlocal_solve(x0, slab, glab, wgt, ids, ws, h, w, layer, 0.125, 1.2, nf, maxit=maxit)
        assert it.tolist() == [maxit] * 3
        for c in range(3):
            A, rhs = system[c]
            x, k = ref64.s1_cg(A, rhs, np.r_[x0[0][:, c], x0[1][:, c]], maxit)
            assert k == maxit
            assert np.allclose(np.r_[ab[0][:, c], ab[1][:, c]], x, rtol=tol, atol=tol), (maxit, c)


# f(oracle's iterate at the cap) / f(ref64's literal iterate at the cap), f = |A x - rhs|^2 per channel. Measured with this file's case generator on 8 seeds x
# {48x48 -> 24x24 layer 2, 40x56 -> 20x28 layer 3, 64x64 flat layer 4, 96x96 -> 48x48 flat layer 3} x 3 channels: 0.992 .. 1.018 (the two recurrences part after
# a few iterations but descend the same energy). The bar [0.9, 1.1] leaves about five times that spread.
S1_CAP_RATIO = (0.9, 1.1)


@pytest.mark.parametrize("case", [(48, 48, 24, 24, (3, 3), 4, 2, False), (40, 56, 20, 28, (5, 7), 4, 3, False), (64, 64, 64, 64, (4, 4), 16, 4, True)])
def test_s1_at_the_cap_descends_like_the_literal_cg(oracle, case):
    H, W, h, w, grid, samples, layer, flat = case
    err, s, g, full, ids, ws, slab, glab = _s1_case(oracle, case, seed=5)
    _, st = oracle.local_color_transfer(err, s, g, full, ids, ws, layer, want_stages=True)
    system = ref64.s1_system(slab, glab, ref64.err_weight(err), ids, ws, h, w, 0.125, 1.2, H * W / (h * w))
    cap = 50 if layer == 4 else 100
    for c in range(3):
        A, rhs = system[c]
        x0 = np.r_[st["ab_local"][0][:, c], st["ab_local"][1][:, c]]
        xo = np.r_[st["ab_nonlocal"][0][:, c], st["ab_nonlocal"][1][:, c]]
        xr, _ = ref64.s1_cg(A, rhs, x0, cap)
        f0, fo, fr = (ref64.s1_objective(A, rhs, v) for v in (x0, xo, xr))
        assert fo <= f0
        assert S1_CAP_RATIO[0] <= fo / fr <= S1_CAP_RATIO[1], (c, fo, fr)


# ---------------------------------------------------------------- U1
@pytest.mark.parametrize("dims", [(9, 9, 17, 17), (9, 200, 17, 400), (16, 12, 31, 23), (57, 85, 113, 170), (12, 17, 100, 90), (5, 3, 5, 3)])
def test_resize_linear(oracle, dims):
    """cv::resize INTER_LINEAR of a 64FC3 map: <= 4 ulp from ref64's float-coefficient form. The pure float64 mapping differs by the float rounding of the
    source coordinate fx (OpenCV keeps its interpolation table in float): at most half a float ulp of the largest coordinate times the largest step between
    neighbours."""
    sh, sw, dh, dw = dims
    src = np.random.default_rng(sh * sw).random((sh, sw, 3)) - 0.3
    got = oracle.resize_f64c3(src, dh, dw)
    assert _ulp_close(got, ref64.resize_linear_f64(src, dh, dw), 4)
    step = max(np.abs(np.diff(src, axis=0)).max(initial=0), np.abs(np.diff(src, axis=1)).max(initial=0))
    bound = 2 * np.spacing(np.float32(max(sh, sw))) * step + 1e-15
    assert np.abs(got - ref64.resize_linear_f64(src, dh, dw, float_coeffs=False)).max() <= bound


def test_roughness_last_channel_decides(oracle):
    rng = np.random.default_rng(8)
    N = 4000
    lab = rng.random((N, 3))
    ab = np.stack([rng.random((N, 3)) * 2.0, rng.random((N, 3)) * 0.8 - 0.4])
    nc = lab * ab[0] + ab[1]
    out = (nc < 0) | (nc > 1)
    assert (out[:, :2].any(1) & ~out[:, 2]).sum() > 100 and (~out[:, :2].any(1) & out[:, 2]).sum() > 100
    assert np.array_equal(oracle.roughness(ab, lab), ref64.roughness(ab, lab))


# ---------------------------------------------------------------- S2, A1 and the composed level
LEVEL_CASES = [(48, 48, 12, 12, (3, 3), 4, 2, False), (40, 56, 20, 28, (5, 7), 4, 3, False), (34, 800, 17, 400, (2, 20), 4, 3, False),
               (113, 170, 113, 170, (5, 7), 8, 4, False), (96, 96, 48, 48, (3, 3), 16, 3, True)]


@pytest.mark.parametrize("case", LEVEL_CASES)
def test_level_stages_vs_ref64(oracle, case):
    """The oracle's composed level, stage by stage, against ref64 applied to the oracle's own previous stage: T1, U1 (resize + roughness), the S2 system and
    its exact solve, A1."""
    H, W, h, w, grid, samples, layer, flat = case
    err, s, g, full, ids, ws, slab, glab = _s1_case(oracle, case, seed=40 + layer)
    out, st = oracle.local_color_transfer(err, s, g, full, ids, ws, layer, want_stages=True)
    flab = oracle.bgr2lab(full).reshape(-1, 3) / 255.0
    ea, eb = ref64.local_stats(oracle.bgr2lab(s), oracle.bgr2lab(g), 0.60)
    assert _ulp_close(st["ab_local"][0], ea, 2) and _ulp_close(st["ab_local"][1], eb, 2)
    if (h, w) != (H, W):
        up = np.stack([ref64.resize_linear_f64(st["ab_nonlocal"][p].reshape(h, w, 3), H, W).reshape(-1, 3) for p in range(2)])
        assert _ulp_close(st["ab_up"], up, 4)
    else:
        assert np.array_equal(st["ab_up"], st["ab_nonlocal"])
    assert np.array_equal(st["roughness"], ref64.roughness(st["ab_up"], flab))
    lam = 0.024 * (H * W) / (h * w) * (4 if (h, w) == (H, W) else 1)
    for o_, r_ in zip(oracle.wls_system(flab, H, W, lam, 1.2, st["roughness"]), ref64.wls_system(flab, H, W, lam, 1.2, st["roughness"])):
        assert np.allclose(o_, r_, rtol=1e-14, atol=0)
    exact = ref64.wls_solve_exact(st["ab_up"], flab, H, W, lam, 1.2, st["roughness"])
    assert np.allclose(st["ab_wls"], exact, rtol=2e-5, atol=2e-6)
    lab_out = ref64.apply_coeffs(st["ab_wls"], flab)
    assert np.array_equal(oracle.apply_coeffs(st["ab_wls"], flab), lab_out)
    assert np.array_equal(out, oracle.lab2bgr(lab_out.reshape(H, W, 3)))


def test_wls_zero_rhs_is_skipped(oracle):
    """A coefficient channel that is zero everywhere has a zero right-hand side: the reference does not solve it and its result stays 0 — the same as
    ref64's skip — while the other channels are solved."""
    oracle._decl_color()
    H, W = 17, 23
    rng = np.random.default_rng(6)
    lab = oracle.bgr2lab(synth.image_flat(4, H, W)).reshape(-1, 3) / 255.0
    rough = np.where(rng.random(H * W) < 0.2, 1e-6, 1.0)
    ab = np.stack([rng.random((H * W, 3)), rng.random((H * W, 3)) - 0.5])
    ab[0][:, 1] = 0.0
    ab[1][:, 2] = 0.0
    exp = ref64.wls_solve_exact(ab, lab, H, W, 0.37, 1.2, rough)
    a, b = ab[0].copy(), ab[1].copy()
    oracle.l.orc_wls_solve(a.reshape(-1), b.reshape(-1), np.ascontiguousarray(lab).reshape(-1), H, W, 0.37, 1.2, rough, 0)
    assert np.all(exp[0][:, 1] == 0) and np.all(exp[1][:, 2] == 0) and np.all(a[:, 1] == 0) and np.all(b[:, 2] == 0)
    assert np.allclose(np.stack([a, b]), exp, rtol=1e-8, atol=1e-10)


# ---------------------------------------------------------------- the chained loop (main.cu:47-454)
# (source size, reference size, bds_weight, image kind): the pyramid ratios of the second and third pairs are odd at every level (17 -> 9 -> 5 -> 3 -> 2,
# 400 -> 200 -> 100 -> 50 -> 25, 23 -> 12 -> 6 -> 3 -> 2); the second's coarsest level is 2x2 against 2x2 (the smallest the pipeline accepts)
PAIR_CASES = [((96, 80), (72, 104), 2.0, "flat"), ((17, 17), (23, 31), 2.0, "cos"), ((17, 400), (40, 23), 0.0, "cos")]


def pair_images(case):
    (sh, sw), (rh, rw), _, kind = case
    mk = synth.image_flat if kind == "flat" else synth.image
    return mk(1000, sh, sw), mk(1001, rh, rw)


@pytest.mark.parametrize("case", PAIR_CASES)
def test_pair_levels_vs_ref64(oracle, case):
    """Every level of the oracle's whole pair against ref64 recomputed from the two input images: pyramid, features (R from the reference image, S from the
    source and then from the previous level's result), distances at the dumped matches, seed bound, guidance image and matching error (tests/levels_ref64.py)."""
    import levels_ref64
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    src, ref = pair_images(case)
    bds = case[2]
    _, lv = oracle.process_pair(src, ref, ws, bs, dict(bds_weight=bds), want_nnf=True)
    geo = ref64.level_geometry(*src.shape[:2], *ref.shape[:2])
    assert geo[0]["ah"] >= 2 and geo[0]["aw"] >= 2
    # the colour stage's inputs: each level's result must be the oracle's composed colour level run on that level's S image, guidance image and matching
    # error, with the kNN graph of samples = 2^l (main.cu:351-359) over the k-means labels and layer l; then its stages against ref64 as for the GPU
    labels, _ = oracle.cluster_features(oracle.vgg19_features(src, ws, bs, 5)[4], 10, 11, 1)
    spyr, _ = levels_ref64.chain_pyramid(src, [(g["ah"], g["aw"]) for g in geo], oracle.resize_u8c3)
    lv["labels"], lv["color"] = labels, []
    for l in range(5):
        ids, kw = oracle.knn_graph(oracle.bgr2lab(spyr[l]), labels, int(labels.max()) + 1, geo[l]["knn_samples"])
        out, st = oracle.local_color_transfer(lv["err"][l], spyr[l], lv["guide"][l], src, ids, kw, l, want_stages=True)
        assert np.array_equal(out, lv["result"][l]), f"level {l}: the result is not the colour stage of the level's inputs"
        lv["color"].append(st)
    stats = levels_ref64.check_levels(lv, src, ref, ws, bs, bds, oracle.resize_u8c3, oracle=oracle)
    print("pair", case, {k: float("%.3g" % v) for k, v in stats.items()})
