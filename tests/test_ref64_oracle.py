"""The CPU oracle vs tests/ref64.py, the float64 restatements written from the reference's text: whole maps, odd and elongated sizes, A != B, flat images, NaN
and constant error maps, hub-heavy kNN graphs. The GPU parity tests compare the kernels with the oracle bit for bit, so what these pin, the kernels inherit;
tests/test_gpu_vs_ref64.py checks the kernels against ref64 directly."""
import numpy as np
import pytest
import ref64
import synth
from test_gpu_color import _level_case

SIZES = [(17, 17), (17, 400), (31, 23), (113, 170)]
# the colour stage's parameters as nct_params_default sets them (Config.h:58-72): what every check below assumes unless it is handed another set
COLOR_DEFAULTS = dict(eps=0.60, nonlocal_weight=2.0, local_weight=0.125, wls_lambda_init=0.024, wls_alpha=1.2)
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


def _nnf_pair(kind, seed_a, seed_b, ah, aw, bh, bw):
    """(ann, bnn) of a vote case. random / border: both fields of that kind; collapsed: ann collapsed, bnn random; collapsed_b: ann random, bnn collapsed —
    half of R's pixels on each of two S pixels, the lists the vote kernels' hub pass sums (every block of 64 sources beyond a target's first)."""
    ka, kb = {"collapsed": ("collapsed", "random"), "collapsed_b": ("random", "collapsed")}.get(kind, (kind, kind))
    return _nnf(ka, seed_a, ah, aw, bh, bw), _nnf(kb, seed_b, bh, bw, ah, aw)


def max_in_degree(bnn, ah, aw):
    """the largest number of R pixels whose match is one S pixel"""
    bnn = np.asarray(bnn, np.uint32)
    return int(np.bincount(((bnn >> 12) * aw + (bnn & 0xFFF)).ravel().astype(np.int64), minlength=ah * aw).max())


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


# the vote cases of tests/test_gpu_dev_seams.py: (ah, aw, bh, bw); the second grid gives collapsed_b 486 / 2 sources per target, three hub blocks each
SEAM_VOTE_GRIDS = [(7, 5, 9, 11), (20, 24, 18, 27)]
SEAM_VOTE_C = (4, 64, 512)


@pytest.mark.parametrize("weights", [(1.0, 2.0), (2.0, 1.0)])
def test_votes_collapsed_b(oracle, weights):
    """collapsed_b (a collapsed R -> S field: the hub pass's long source lists) at the seam test's shapes: the oracle, whose summation order is the kernels',
    stays inside the tolerances test_gpu_vs_ref64.py::test_votes_vs_ref64 gives the other kinds, so that kind needs no bound of its own."""
    wc, wp = weights
    for (ah, aw, bh, bw) in SEAM_VOTE_GRIDS:
        ia, ib = synth.image(1, ah, aw), synth.image(2, bh, bw)
        ann, bnn = _nnf_pair("collapsed_b", 3, 4, ah, aw, bh, bw)
        if bh * bw >= 260:
            assert max_in_degree(bnn, ah, aw) >= 130
        for C in SEAM_VOTE_C:
            pin = synth.features(7, C, bh, bw)
            got, gpw = oracle.bds_vote_features(ann, bnn, pin, wc, wp, want_pw=True)
            exp, epw = ref64.vote_features(ann, bnn, pin, wc, wp)
            dev = np.abs(got - exp) / (1e-6 + 1e-5 * np.abs(exp))
            print("collapsed_b", (ah, aw, bh, bw), C, weights, "vote deviation / tolerance %.3g" % dev.max())
            assert np.allclose(got, exp, rtol=1e-5, atol=1e-6) and np.allclose(gpw, epw, rtol=1e-5, atol=1e-12)
        ei, v = ref64.vote_image(ia, ib, ann, bnn, wc, wp, want_float=True)
        assert _vote_image_agrees(oracle.bds_vote_image(ia, ib, ann, bnn, wc, wp), ei, v)


# collapsed_b at 350 x 350 (test_gpu_vs_ref64.py::test_votes_vs_ref64's largest case) puts 61 310 sources on one target: float sums of that length. There the
# oracle's vote and weight deviate 1.28 and 1.31 times the tolerance of the other kinds (rtol 1e-5; atol 1e-6, 1e-12) from ref64, with either pair of weights
# (test_votes_collapsed_b_long_lists prints it); up to 3 325 sources (88 x 88 from 70 x 95) it stays below a tenth of it. Four times the measured value, as for
# NORM_MAP_TOL below, for lists longer than VOTE_LONG_LIST.
VOTE_LONG_LIST = 10000
VOTE_LONG_LIST_SCALE = 5.3


def vote_tol_scale(bnn, ah, aw):
    return VOTE_LONG_LIST_SCALE if max_in_degree(bnn, ah, aw) > VOTE_LONG_LIST else 1.0


def test_votes_collapsed_b_long_lists(oracle):
    """the calibration of VOTE_LONG_LIST_SCALE"""
    C, (ah, aw, bh, bw) = 64, (350, 350, 350, 350)
    pin = synth.features(7, C, bh, bw)
    ann, bnn = _nnf_pair("collapsed_b", 3, 4, ah, aw, bh, bw)
    assert vote_tol_scale(bnn, ah, aw) == VOTE_LONG_LIST_SCALE
    worst = 0.0
    for wc, wp in ((1.0, 2.0), (2.0, 1.0)):
        got, gpw = oracle.bds_vote_features(ann, bnn, pin, wc, wp, want_pw=True)
        exp, epw = ref64.vote_features(ann, bnn, pin, wc, wp)
        worst = max(worst, float((np.abs(got - exp) / (1e-6 + 1e-5 * np.abs(exp))).max()), float((np.abs(gpw - epw) / (1e-12 + 1e-5 * np.abs(epw))).max()))
    print("collapsed_b 350 x 350: deviation / tolerance %.3g" % worst)
    assert 1.0 < worst and 4 * worst <= VOTE_LONG_LIST_SCALE


# ---------------------------------------------------------------- N1 and the matching error alone, at the widths of a 16-lane row
# C: one lane busy, a partial first round, a partial second round, one full round, a partial third round, eight rounds; HW: one pixel, a block with a dead row,
# a full block, a second block with one live row (its other rows read the last pixel, clamped), several blocks
NORM_C = (4, 8, 20, 64, 132, 512)
NORM_HW = (1, 15, 16, 17, 63)
# Largest |oracle - ref64| over that table (test_normalize_and_distance_alone prints it; synth.features maps, the dead-pixel map included): 8.11e-8 in the
# normalised map (values in [0, 1]: one rounding of the norm and one of the quotient) and 1.54e-6 in the response, where the rounding of the norms is divided
# by their spread (max - min). The bounds are four times that, the margin FEAT16_TOL leaves; the GPU tests import them.
NORM_MAP_TOL = 3.3e-7
NORM_RESP_TOL = 6.2e-6
# the project's bound for the matching error of unit vectors (test_patch_distance)
FEATURE_DISTANCE_TOL = 1e-5


def norm_hw(HW):
    return (7, 9) if HW == 63 else (1, HW)


def norm_map(C, HW, seed=0, dead=False):
    f = synth.features(100 + seed + C + HW, C, *norm_hw(HW))
    if dead:
        f.reshape(C, -1)[:, HW // 2] = 0
    return f


def check_normalize(normalize, C, HW, dead=False):
    """normalize(f, want_resp=True) against ref64 within NORM_MAP_TOL / NORM_RESP_TOL; NaN exactly over a dead pixel's channels (and, in the response, over the
    whole map where all norms are equal: HW = 1). Returns the two largest deviations."""
    f = norm_map(C, HW, dead=dead)
    got, resp = normalize(f, want_resp=True)
    exp, eresp = ref64.normalize(f), ref64.response(f)
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.isnan(exp).sum() == (C if dead else 0)
    assert np.array_equal(np.isnan(resp), np.isnan(eresp)) and np.isnan(eresp).all() == (HW == 1)
    dm = float(np.nanmax(np.abs(got - exp), initial=0.0))
    dr = 0.0 if HW == 1 else float(np.abs(resp - eresp).max())
    assert dm <= NORM_MAP_TOL and dr <= NORM_RESP_TOL, (C, HW, dead, dm, dr)
    if dead and HW > 1:
        assert resp.reshape(-1)[HW // 2] == 0
    return dm, dr


def check_feature_distance(normalize, distance, C, HW):
    a, b = normalize(norm_map(C, HW, 1)), normalize(norm_map(C, HW, 2))
    d = float(np.abs(distance(a, b) - ref64.feature_distance(a, b)).max())
    assert d <= FEATURE_DISTANCE_TOL, (C, HW, d)
    return d


def test_normalize_and_distance_alone(oracle):
    """The calibration of NORM_MAP_TOL and NORM_RESP_TOL: the oracle carries the kernels' summation order bit for bit, and its largest deviation from ref64
    over the C / HW table (dead-pixel maps from HW = 15 on) is what the constants above record."""
    worst = np.zeros(3)
    for C in NORM_C:
        for HW in NORM_HW:
            for dead in ((False, True) if HW > 1 else (False,)):
                worst[:2] = np.maximum(worst[:2], check_normalize(oracle.feat_normalize, C, HW, dead))
            worst[2] = max(worst[2], check_feature_distance(oracle.feat_normalize, oracle.feature_distance, C, HW))
    print("oracle vs ref64 alone: map %.3g response %.3g matching error %.3g" % tuple(worst))
    assert worst[0] * 4 <= NORM_MAP_TOL and worst[1] * 4 <= NORM_RESP_TOL, "the bounds no longer leave the margin of four over the oracle's deviation"


def test_response_of_equal_norms_is_nan(oracle):
    """max = min: the reference's text scales 0 by 1 / 0, so every pixel of the response is NaN (ref64.response); the normalised map is unaffected"""
    f = np.tile(synth.features(5, 20, 1, 1), (1, 3, 5)) * np.where(np.arange(15).reshape(1, 3, 5) % 2, -1, 1).astype(np.float32)
    got, resp = oracle.feat_normalize(f, want_resp=True)
    assert np.isnan(resp).all() and np.isnan(ref64.response(f)).all()
    assert np.abs(got - ref64.normalize(f)).max() <= NORM_MAP_TOL


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


def check_s1_short_iterations(oracle, case, prm=COLOR_DEFAULTS):
    """maxit 1, 2, 5: the oracle's canonical recurrence (what the kernels reproduce) vs the literal CGNR on ref64's assembled A, from the same x0. Before the
    truncated CG's chaos sets in they agree to rounding (test_canonical_cg_matches_explicit_for_few_iterations shows the same for the oracle's two forms).
    prm: the colour parameters handed to both sides. Returns the largest |oracle - ref64| / bar over the three runs."""
    H, W, h, w, grid, samples, layer, flat = case
    err, s, g, full, ids, ws, slab, glab = _s1_case(oracle, case)
    if flat:
        assert np.bincount(ids.reshape(-1)).max() > 64
    wgt = ref64.err_weight(err)
    nf = H * W / (h * w)
    x0 = np.stack(oracle.local_stats(oracle.bgr2lab(s), oracle.bgr2lab(g), prm["eps"]))
    system = ref64.s1_system(slab, glab, wgt, ids, ws, h, w, prm["local_weight"], prm["wls_alpha"], nf, nonlocal_weight=prm["nonlocal_weight"])
    worst = 0.0
    for maxit, tol in ((1, 1e-12), (2, 1e-10), (5, 1e-7)):
        ab, it = oracle.nonlocal_solve(x0, slab, glab, wgt, ids, ws, h, w, layer, prm["local_weight"], prm["wls_alpha"], nf, nl_weight=prm["nonlocal_weight"], maxit=maxit)
        assert it.tolist() == [maxit] * 3
        for c in range(3):
            A, rhs = system[c]
            x, k = ref64.s1_cg(A, rhs, np.r_[x0[0][:, c], x0[1][:, c]], maxit)
            assert k == maxit
            got = np.r_[ab[0][:, c], ab[1][:, c]]
            worst = max(worst, float((np.abs(got - x) / (tol + tol * np.abs(x))).max()))
            assert np.allclose(got, x, rtol=tol, atol=tol), (maxit, c)
    return worst


@pytest.mark.parametrize("case", S1_CASES)
def test_s1_short_iterations(oracle, case):
    check_s1_short_iterations(oracle, case)


# f(oracle's iterate at the cap) / f(ref64's literal iterate at the cap), f = |A x - rhs|^2 per channel. Measured with this file's case generator on 8 seeds x
# {48x48 -> 24x24 layer 2, 40x56 -> 20x28 layer 3, 64x64 flat layer 4, 96x96 -> 48x48 flat layer 3} x 3 channels: 0.992 .. 1.018 (the two recurrences part after
# a few iterations but descend the same energy). The bar [0.9, 1.1] leaves about five times that spread.
S1_CAP_RATIO = (0.9, 1.1)


@pytest.mark.parametrize("case", [(48, 48, 24, 24, (3, 3), 4, 2, False), (40, 56, 20, 28, (5, 7), 4, 3, False), (64, 64, 64, 64, (4, 4), 16, 4, True)])
def test_s1_at_the_cap_descends_like_the_literal_cg(oracle, case):
    check_s1_at_the_cap(oracle, case)


def check_s1_at_the_cap(oracle, case, prm=COLOR_DEFAULTS, seed=5):
    """-> the (smallest, largest) energy ratio over the three channels, each inside S1_CAP_RATIO"""
    H, W, h, w, grid, samples, layer, flat = case
    err, s, g, full, ids, ws, slab, glab = _s1_case(oracle, case, seed=seed)
    _, st = oracle.local_color_transfer(err, s, g, full, ids, ws, layer, params=dict(prm, k_num=8.0), want_stages=True)
    system = ref64.s1_system(slab, glab, ref64.err_weight(err), ids, ws, h, w, prm["local_weight"], prm["wls_alpha"], H * W / (h * w), nonlocal_weight=prm["nonlocal_weight"])
    cap = 50 if layer == 4 else 100
    ratios = []
    for c in range(3):
        A, rhs = system[c]
        x0 = np.r_[st["ab_local"][0][:, c], st["ab_local"][1][:, c]]
        xo = np.r_[st["ab_nonlocal"][0][:, c], st["ab_nonlocal"][1][:, c]]
        xr, _ = ref64.s1_cg(A, rhs, x0, cap)
        f0, fo, fr = (ref64.s1_objective(A, rhs, v) for v in (x0, xo, xr))
        assert fo <= f0
        assert S1_CAP_RATIO[0] <= fo / fr <= S1_CAP_RATIO[1], (c, fo, fr)
        ratios.append(fo / fr)
    return min(ratios), max(ratios)


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
    check_level_stages(oracle, case)


def check_level_stages(oracle, case, prm=COLOR_DEFAULTS):
    """The oracle's composed level, stage by stage, against ref64 applied to the oracle's own previous stage: T1, U1 (resize + roughness), the S2 system and
    its exact solve, A1. Returns (the stages, the largest |S2 - exact| / (atol + rtol |exact|): the fraction of S2's bar in use)."""
    H, W, h, w, grid, samples, layer, flat = case
    err, s, g, full, ids, ws, slab, glab = _s1_case(oracle, case, seed=40 + layer)
    out, st = oracle.local_color_transfer(err, s, g, full, ids, ws, layer, params=dict(prm, k_num=8.0), want_stages=True)
    flab = oracle.bgr2lab(full).reshape(-1, 3) / 255.0
    ea, eb = ref64.local_stats(oracle.bgr2lab(s), oracle.bgr2lab(g), prm["eps"])
    assert _ulp_close(st["ab_local"][0], ea, 2) and _ulp_close(st["ab_local"][1], eb, 2)
    if (h, w) != (H, W):
        up = np.stack([ref64.resize_linear_f64(st["ab_nonlocal"][p].reshape(h, w, 3), H, W).reshape(-1, 3) for p in range(2)])
        assert _ulp_close(st["ab_up"], up, 4)
    else:
        assert np.array_equal(st["ab_up"], st["ab_nonlocal"])
    assert np.array_equal(st["roughness"], ref64.roughness(st["ab_up"], flab))
    lam, alpha = prm["wls_lambda_init"] * (H * W) / (h * w) * (4 if (h, w) == (H, W) else 1), prm["wls_alpha"]
    for o_, r_ in zip(oracle.wls_system(flab, H, W, lam, alpha, st["roughness"]), ref64.wls_system(flab, H, W, lam, alpha, st["roughness"])):
        assert np.allclose(o_, r_, rtol=1e-14, atol=0)
    exact = ref64.wls_solve_exact(st["ab_up"], flab, H, W, lam, alpha, st["roughness"])
    assert np.allclose(st["ab_wls"], exact, rtol=2e-5, atol=2e-6)
    lab_out = ref64.apply_coeffs(st["ab_wls"], flab)
    assert np.array_equal(oracle.apply_coeffs(st["ab_wls"], flab), lab_out)
    assert np.array_equal(out, oracle.lab2bgr(lab_out.reshape(H, W, 3)))
    return st, float((np.abs(st["ab_wls"] - exact) / (2e-6 + 2e-5 * np.abs(exact))).max())


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
    stats = levels_ref64.check_levels(lv, src, ref, ws, bs, bds, oracle)
    print("pair", case, {k: float("%.3g" % v) for k, v in stats.items()})


# ---------------------------------------------------------------- A1: BGR <-> Lab over every 8-bit input
# bgr2lab: OpenCV's 8-bit path against the exact mapping (ref64.bgr2lab's unrounded value), per band of the exact L byte and per channel. The 8-bit path rounds
# its result (0.5), scales L by 296/2^15 instead of 295.8 (<= 0.2 at L = 255), quantises linear light to 1/2040 (sRGBGammaTab_b) and the cube root to 2^-15
# (LabCbrtTab_b) before the matrix and after it. The linear-light step moves f = Y^(1/3) by step / (3 Y^(2/3)): in dark colours (L byte < 64, Y < 0.043) up to
# a few tenths of an L unit, in a and b — differences of two such cube roots scaled by 500 and 200 — over a unit more; above, the step shrinks below half a
# unit. Measured maxima over all 2^24 inputs, (L, a, b): [0, 64) 1.55 / 2.67 / 1.70, [64, 128) 0.92 / 1.37 / 1.26, [128, 256) 0.75 / 0.84 / 0.94.
BGR2LAB_BANDS = [(0, 64, (2.0, 3.0, 2.0)), (64, 128, (1.25, 1.75, 1.5)), (128, 256, (1.0, 1.0, 1.0))]


def _lattice(b0, b1):
    g = np.arange(256)
    return np.stack(np.meshgrid(np.arange(b0, b1), g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.uint8)


def check_bgr2lab_all(bgr2lab):
    """bgr2lab (a library's) over all 2^24 BGR triples, in chunks, within BGR2LAB_BANDS of ref64.bgr2lab; on the grey axis a and b exactly 128 and L within
    1 LSB of the exact byte. Returns the largest deviation per band."""
    worst = np.zeros((len(BGR2LAB_BANDS), 3))
    for b0 in range(0, 256, 32):
        bgr = _lattice(b0, b0 + 32)
        got = np.asarray(bgr2lab(bgr)).astype(np.float64)
        _, val = ref64.bgr2lab(bgr)
        dev = np.abs(got - val)
        L = np.rint(val[:, 0])
        for bi, (lo, hi, bound) in enumerate(BGR2LAB_BANDS):
            sel = (L >= lo) & (L < hi)
            if sel.any():
                worst[bi] = np.maximum(worst[bi], dev[sel].max(0))
    for bi, (lo, hi, bound) in enumerate(BGR2LAB_BANDS):
        assert np.all(worst[bi] <= bound), (lo, hi, worst[bi].tolist(), bound)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    got, (eb, _) = np.asarray(bgr2lab(grey)).astype(int), ref64.bgr2lab(grey)
    assert np.all(got[:, 1:] == 128) and np.abs(got[:, 0] - eb[:, 0]).max() <= 1
    return worst


def check_lab2bgr_all(lab2bgr):
    """lab2bgr(lab, form) (a library's) over all 2^24 Lab triples, both forms, within 1 LSB of ref64.lab2bgr outside the cube form's far-out channels.
    Returns the largest deviation per form."""
    worst = []
    for form in (0, 1):
        dev = 0
        for b0 in range(0, 256, 32):
            lab = _lattice(b0, b0 + 32)
            got = np.asarray(lab2bgr(lab, form)).astype(np.float64)
            exp, far = ref64.lab2bgr(lab, form)
            dev = max(dev, float(np.abs(got - exp)[~far].max()))
        assert dev <= 1, (form, dev)
        worst.append(dev)
    return worst


def test_bgr2lab_all_inputs_vs_ref64(oracle):
    print("bgr2lab", check_bgr2lab_all(oracle.bgr2lab).round(3).tolist())


def test_lab2bgr_all_inputs_vs_ref64(oracle):
    print("lab2bgr", check_lab2bgr_all(lambda lab, form: oracle.lab2bgr(lab, form=form)))


# ---------------------------------------------------------------- C1: k-means labels
# A label comparison through two normalisations (the library's float one, ref64's float64 one rounded to float) is meaningful only where no point lies nearer
# than that to a tie: the two normalised maps differ by <= 1e-7 relative, which moved a float L2 distance by at most 5.1e-7 relative (measured on
# synth.features 44 x 44 x 512, 64-channel 9 x 11 maps and 63 x 63 blobs). Every case's margin (ref64.kmeans_labels) must exceed four times that.
KM_MARGIN = 2e-6


def _km_blobs(seed, C, h, w, nb, noise):
    rng = np.random.default_rng(seed)
    cen = rng.random((nb, C)).astype(np.float32)
    pts = np.abs(cen[rng.integers(0, nb, h * w)] + np.float32(noise) * rng.standard_normal((h * w, C)).astype(np.float32)) + np.float32(0.01)
    return np.ascontiguousarray(pts.T.reshape(C, h, w))


def _km_few(seed, C, h, w, distinct, skew):
    """few distinct vectors; skew: the first holds that fraction of the points, so centre selection rejects duplicates deep into the permutation"""
    rng = np.random.default_rng(seed)
    protos = (rng.random((distinct, C), dtype=np.float32) + np.float32(0.05)) * np.float32(3.0)
    which = np.where(rng.random(h * w) < skew, 0, rng.integers(1, distinct, h * w))
    return np.ascontiguousarray(protos[which].T.reshape(C, h, w))


def _km_donor():
    """33 points near 12 prototypes in 8 channels: seed 1 leaves a cluster empty after the first step (the donor rule moves the farthest point of the next
    cluster into it)"""
    rng = np.random.default_rng(67)
    n, C = int(rng.integers(10, 40)), 8
    pro = rng.random((12, C)).astype(np.float32) + 0.01
    return np.ascontiguousarray((pro[rng.integers(0, 12, n)] + 0.05 * rng.random((n, C))).T.reshape(C, 1, n)).astype(np.float32)


def _km_tie():
    """ten distinct unit vectors in 16 channels, 40 copies each, and the midpoints of the pairs (0, 1), (2, 3), (4, 5): after normalisation a midpoint is
    exactly as far from both ends (the two squares swap places inside one group of four), so its first assignment is an exact tie that the strict > gives to
    the lower centre id. No margin: the tie is the point."""
    C = 16
    v = np.zeros((10, C), np.float32)
    v[np.arange(10), np.arange(10)] = 1.0
    v[:, 12] = 0.25
    mids = np.stack([(v[2 * i] + v[2 * i + 1]) * np.float32(0.5) for i in range(3)])
    pts = np.concatenate([np.repeat(v, 40, 0), mids])
    return np.ascontiguousarray(pts.T.reshape(C, 1, -1))


# (name, features, seeds, what the case must reach: steps == 11 ("cap"), an early stop ("early"), a donor move, one label, duplicate rejections, an exact tie;
#  whether the margin above KM_MARGIN is required — where it is not, only the comparison on the library's own normalised map holds, which is exact)
KM_CASES = [("synth16", lambda: synth.features(3, 512, 16, 16) * np.float32(5.0), (1, 2, 3), "early"),
            ("synth44_cap", lambda: synth.features(3, 512, 44, 44) * np.float32(5.0), (2,), "cap"),
            ("c64_9x11", lambda: synth.features(1, 64, 9, 11), (1, 2, 3), "early"),
            ("blobs63", lambda: _km_blobs(1, 512, 63, 63, 10, 0.05), (2,), "donor"),
            ("blobs70", lambda: _km_blobs(1, 512, 70, 70, 10, 0.05), (1,), "cap"),
            ("few70", lambda: _km_few(4, 512, 70, 70, 12, 0.9), (1, 2, 3), "dups"),
            ("few30_one_label", lambda: _km_few(5, 512, 30, 30, 4, 0.5), (1,), "one"),
            ("n_below_K", lambda: synth.features(2, 512, 3, 3), (1,), "one"),
            ("n_equals_K", lambda: synth.features(2, 512, 2, 5), (1, 2), "early"),
            ("donor8", _km_donor, (1,), "donor"),
            ("tie16", _km_tie, (1, 2, 3), "tie", False),
            ("synth44_tight_cap", lambda: synth.features(3, 512, 44, 44) * np.float32(5.0), (1,), "cap", False),      # an exact tie in a Lloyd step
            ("synth63_tight_cap", lambda: synth.features(3, 512, 63, 63) * np.float32(5.0), (1,), "cap", False)]


def check_kmeans(cluster, normalize, f, seed, expect, need_margin=True, K=10):
    """cluster(f, K, iters, seed) -> (labels, n): bit for bit ref64.kmeans_labels of the library's own normalised map (no margin needed: ref64 emulates every
    float operation), and of ref64's normalisation of f with the margin above KM_MARGIN (need_margin False: only reported). Returns the margin."""
    gl, gn = cluster(f, K, 11, seed)
    el, en, _, info = ref64.kmeans_labels(normalize(f), K, 11, seed, normalized=True, want_info=True)
    assert gn == en and np.array_equal(gl, el), "labels differ from ref64 on the library's normalised map"
    rl, rn, margin = ref64.kmeans_labels(f, K, 11, seed)
    if need_margin:
        assert margin >= KM_MARGIN, f"margin {margin:.3g}: this case cannot tell a label error from the normalisation's rounding"
        assert gn == rn and np.array_equal(gl, rl)
    if expect == "cap":
        assert info["steps"] == 11 and not info["converged"], info
    elif expect == "early":
        assert info["converged"] and info["steps"] < 11, info
    elif expect == "donor":
        assert info["donors"] > 0, info
    elif expect == "one":
        assert gn == 1 and not gl.any()
    return margin


@pytest.mark.parametrize("case", KM_CASES, ids=[c[0] for c in KM_CASES])
def test_kmeans_labels_vs_ref64(oracle, case):
    name, mk, seeds, expect = case[:4]
    f = mk()
    if expect == "dups":
        perm = ref64._perm_splitmix(f.shape[1] * f.shape[2], 1)
        assert np.flatnonzero(f.reshape(f.shape[0], -1)[0][perm] != f.reshape(f.shape[0], -1)[0][perm[0]]).size > 0
    for seed in seeds:
        m = check_kmeans(oracle.cluster_features, oracle.feat_normalize, f, seed, expect, *case[4:])
        print(name, seed, "margin %.3g" % m)


@pytest.mark.parametrize("case", PAIR_CASES[:1] + PAIR_CASES[2:])
def test_kmeans_labels_of_conv5_vs_ref64(oracle, case):
    """the source's and the reference's float64 conv5_1 (ref64.vgg19_taps) at the pair sizes of test_pair_levels_vs_ref64"""
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    for img in pair_images(case):
        f = ref64.vgg19_taps(img, ws, bs, 5)[4]
        for seed in (1, 2, 3):
            check_kmeans(oracle.cluster_features, oracle.feat_normalize, f, seed, None)


# ---------------------------------------------------------------- K1: kNN graph
def knn_labels(kind, lh, lw, seed=0):
    """label grids: "checker" (x + 2y) mod 5 — every cell's four neighbours carry four other labels, so with dilation each cell is in 5 clusters; "single" —
    random labels 0..3 plus label 4 on one cell and label 5 on one corner cell (one-cell clusters); "bands" — vertical bands of 3 labels"""
    yy, xx = np.mgrid[0:lh, 0:lw]
    if kind == "checker":
        return ((xx + 2 * yy) % 5).astype(np.int32), 5
    if kind == "single":
        lb = np.random.default_rng(seed).integers(0, 4, (lh, lw)).astype(np.int32)
        lb[lh // 2, lw // 3] = 4
        lb[0, lw - 1] = 5
        return lb, 6
    return (xx * 3 // lw).astype(np.int32), 3


def knn_image(kind, h, w, seed=9):
    img = synth.image_flat(seed, h, w) if kind == "flat" else synth.image(seed, h, w)
    if kind == "flat":
        img[h // 2:h // 2 + 2, : w // 2] = (255, 0, 255)           # isolated far colours
        img[0, 0] = (0, 255, 0)
    return img


def check_knn(gi, gw, ei, ew, what):
    """ids exactly, weights within 4e-16 relative (orc_exp / the kernels' exp are within 1 ulp of libm). Returns (padded entries, max relative deviation)."""
    assert np.array_equal(gi, ei), f"{what}: ids differ from ref64 at {int((gi != ei).any(1).sum())} pixels"
    assert np.allclose(gw, ew, rtol=4e-16, atol=0), what
    nz = ew > 0
    dev = float((np.abs(gw - ew)[nz] / ew[nz]).max(initial=0.0))
    pad = int(((ew == 0) & (ei == np.arange(ei.shape[0])[:, None])).sum())
    return pad, dev


# (level h, w, label grid lh, lw, label kind, image kind, samples)
KNN_CASES = [(113, 170, 8, 11, "checker", "flat", 16), (113, 170, 8, 11, "single", "cos", 16), (60, 47, 12, 10, "checker", "flat", 5),
             (40, 44, 40, 44, "single", "flat", 1), (45, 61, 23, 31, "checker", "cos", 2), (70, 33, 10, 5, "single", "flat", 7),
             (64, 64, 8, 8, "bands", "flat", 8), (37, 53, 3, 4, "checker", "cos", 13), (30, 30, 30, 30, "checker", "flat", 1)]


@pytest.mark.parametrize("case", KNN_CASES)
def test_knn_graph_vs_ref64(oracle, case):
    h, w, lh, lw, lkind, ikind, samples = case
    labels, nl = knn_labels(lkind, lh, lw)
    lab = oracle.bgr2lab(knn_image(ikind, h, w))
    gi, gw = oracle.knn_graph(lab, labels, nl, samples)
    ei, ew = ref64.knn_graph(lab, labels, nl, samples)
    pad, dev = check_knn(gi, gw, ei, ew, str(case))
    print(case, "padded", pad, "max rel dev %.3g" % dev)


def test_knn_graph_flat_ties_and_padding(oracle):
    """a map of few colours (every distance tied many times) and a grid that leaves pixels uncovered (3 x 4 cells of 5 on a 17 x 23 level): the (distance, id)
    order and the zero-weight self padding"""
    rng = np.random.default_rng(2)
    pal = rng.integers(0, 256, (4, 3)).astype(np.uint8)
    lab = oracle.bgr2lab(pal[rng.integers(0, 4, (17, 23))])
    labels, nl = knn_labels("single", 3, 4, 1)
    gi, gw = oracle.knn_graph(lab, labels, nl, 5)
    ei, ew = ref64.knn_graph(lab, labels, nl, 5)
    pad, _ = check_knn(gi, gw, ei, ew, "flat")
    assert pad > 0 and np.all(ew.reshape(17, 23, 8)[15:, :, :] == 0)
    # one cluster of 2 x 4 covered pixels: each has 7 others, so the eighth entry is the zero-weight self edge
    labels = np.zeros((2, 4), np.int32)
    gi, gw = oracle.knn_graph(lab, labels, 1, 1)
    ei, ew = ref64.knn_graph(lab, labels, 1, 1)
    check_knn(gi, gw, ei, ew, "2x4")
    cov = (np.arange(17)[:, None] < 2) & (np.arange(23)[None, :] < 4)
    assert np.all(ew.reshape(17, 23, 8)[cov][:, 7] == 0) and np.all(ew.reshape(17, 23, 8)[cov][:, :7] > 0)
