"""The kernels vs tests/ref64.py, the float64 restatements written from the reference's text, at the production and edge shapes — a check that does not go
through the oracle, whose operator order the kernels mirror. Each colour stage is compared with ref64 applied to the GPU's own previous stage."""
import numpy as np
import pytest
import ref64
import synth
from test_gpu_color import _level_case
from test_ref64_oracle import S1_CAP_RATIO, _ulp_close, _vote_image_agrees, _nnf

pytestmark = pytest.mark.gpu

# the cases of test_gpu_color.py::test_local_color_transfer_stages (k_s1_hub, the shared-gather operator, the 48x8 V-cycle tiles) and one 17x400 level
COLOR_CASES = [(48, 48, 12, 12, (3, 3), 4, 2), (40, 56, 20, 28, (5, 7), 4, 3), (32, 32, 32, 32, (2, 2), 16, 4), (372, 368, 372, 368, (23, 23), 16, 4),
               (96, 96, 48, 48, (3, 3), 16, 3, "flat"), (160, 160, 80, 80, (5, 5), 16, 2, "flat"), (64, 64, 64, 64, (4, 4), 16, 4, "flat"),
               (372, 368, 372, 368, (23, 23), 16, 4, "flat"), (34, 800, 17, 400, (2, 20), 4, 3)]


def _case(oracle, case):
    H, W, h, w, grid, samples, layer = case[:7]
    err, s, g, full, ids, ws = _level_case(20 + layer, H, W, h, w, grid, samples, oracle, len(case) > 7)
    slab = oracle.bgr2lab(s).reshape(-1, 3) / 255.0
    glab = oracle.bgr2lab(g).reshape(-1, 3) / 255.0
    flab = oracle.bgr2lab(full).reshape(-1, 3) / 255.0
    return H, W, h, w, layer, err, s, g, full, ids, ws, slab, glab, flab


def _chan(ab, c):
    return np.r_[ab[0][:, c], ab[1][:, c]]


def _check_after_s1(oracle, gs, go, H, W, h, w, flab):
    """U1, roughness, S2 and A1, each against ref64 applied to the GPU's previous stage. Returns the number of pixels where channel 0 or 1 leaves [0, 1] and
    channel 2 does not (only the last channel decides the roughness)."""
    if (h, w) != (H, W):
        for p in range(2):
            src = gs["ab_nonlocal"][p].reshape(h, w, 3)
            up = ref64.resize_linear_f64(src, H, W).reshape(-1, 3)
            assert _ulp_close(gs["ab_up"][p], up, 4), p
            up64 = ref64.resize_linear_f64(src, H, W, float_coeffs=False).reshape(-1, 3)
            assert np.all(np.abs(gs["ab_up"][p] - up64) <= 1e-7 * np.abs(up64) + 1e-15), p
    else:
        assert np.array_equal(gs["ab_up"], gs["ab_nonlocal"])
    assert np.array_equal(gs["roughness"], ref64.roughness(gs["ab_up"], flab))
    lam = 0.024 * (H * W) / (h * w) * (4 if (h, w) == (H, W) else 1)
    exact = ref64.wls_solve_exact(gs["ab_up"], flab, H, W, lam, 1.2, gs["roughness"])
    assert np.allclose(gs["ab_wls"], exact, rtol=2e-5, atol=2e-6)
    assert np.array_equal(go, oracle.lab2bgr(ref64.apply_coeffs(gs["ab_wls"], flab).reshape(H, W, 3)))
    nc = flab * gs["ab_up"][0] + gs["ab_up"][1]
    out = (nc < 0) | (nc > 1)
    return int((out[:, :2].any(1) & ~out[:, 2]).sum())


@pytest.mark.parametrize("case", COLOR_CASES)
def test_color_stages_vs_ref64(ctx, oracle, case):
    """T1 within 2 ulp; S1 at the reference's cap: the energy |A x - rhs|^2 of ref64's system falls from the T1 guess and lands within S1_CAP_RATIO of the literal
    CGNR's (calibration: tests/test_ref64_oracle.py); U1, roughness, S2 (exact solve) and A1 as in _check_after_s1."""
    H, W, h, w, layer, err, s, g, full, ids, ws, slab, glab, flab = _case(oracle, case)
    go, gs = ctx.local_color_transfer(err, s, g, full, ids, ws, layer, want_stages=True)
    ea, eb = ref64.local_stats(oracle.bgr2lab(s), oracle.bgr2lab(g), 0.60)
    assert _ulp_close(gs["ab_local"][0], ea, 2) and _ulp_close(gs["ab_local"][1], eb, 2)
    cap = 50 if layer == 4 else 100
    assert gs["cg_iters"].tolist() == [cap] * 3
    system = ref64.s1_system(slab, glab, ref64.err_weight(err), ids, ws, h, w, 0.125, 1.2, H * W / (h * w))
    for c in range(3):
        A, rhs = system[c]
        x0 = _chan(gs["ab_local"], c)
        xr, _ = ref64.s1_cg(A, rhs, x0, cap)
        f0, fg, fr = (ref64.s1_objective(A, rhs, v) for v in (x0, _chan(gs["ab_nonlocal"], c), xr))
        assert fg <= f0, c
        assert S1_CAP_RATIO[0] <= fg / fr <= S1_CAP_RATIO[1], (c, fg, fr)
    mixed = _check_after_s1(oracle, gs, go, H, W, h, w, flab)
    if len(case) > 7 and case[0] == 372:
        assert mixed > 0, "this case is meant to hold pixels where only channel 0 or 1 leaves [0, 1]"


@pytest.mark.parametrize("case", [COLOR_CASES[i] for i in (0, 1, 3, 4, 7, 8)])
def test_s1_short_runs_vs_literal_cg(oracle, case, monkeypatch):
    """NCT_S1_MAXIT = 1, 2, 5: the GPU's S1 iterate vs ref64's literal CGNR from the GPU's own T1 guess, at the agreement the oracle's two forms show
    (test_canonical_cg_matches_explicit_for_few_iterations); the reported iteration counts follow the hook."""
    import nct
    H, W, h, w, layer, err, s, g, full, ids, ws, slab, glab, flab = _case(oracle, case)
    system = ref64.s1_system(slab, glab, ref64.err_weight(err), ids, ws, h, w, 0.125, 1.2, H * W / (h * w))
    for maxit, tol in ((1, 1e-12), (2, 1e-10), (5, 1e-7)):
        monkeypatch.setenv("NCT_S1_MAXIT", str(maxit))
        with nct.Context(0) as c:
            _, gs = c.local_color_transfer(err, s, g, full, ids, ws, layer, want_stages=True)
        assert gs["cg_iters"].tolist() == [maxit] * 3
        for ch in range(3):
            A, rhs = system[ch]
            x, k = ref64.s1_cg(A, rhs, _chan(gs["ab_local"], ch), maxit)
            assert k == maxit
            assert np.allclose(_chan(gs["ab_nonlocal"], ch), x, rtol=tol, atol=tol), (maxit, ch)


def test_flat_guide_skips_the_zero_rhs(ctx, oracle):
    """A guide of one colour: a = 0 everywhere after T1, the T1 guess already solves S1 (no iteration), and S2 skips the all-zero a right-hand sides
    (ColorTransfer.cpp:1000-1030 with solve_direct_cpu) — their result stays 0."""
    H, W, h, w, layer, err, s, g, full, ids, ws, slab, glab, flab = _case(oracle, COLOR_CASES[1])
    g = np.full_like(g, (90, 140, 60))
    go, gs = ctx.local_color_transfer(err, s, g, full, ids, ws, layer, want_stages=True)
    assert np.all(gs["ab_local"][0] == 0) and gs["cg_iters"].tolist() == [0, 0, 0]
    assert np.all(gs["ab_wls"][0] == 0)
    _check_after_s1(oracle, gs, go, H, W, h, w, flab)


# ---------------------------------------------------------------- correspondence
@pytest.mark.parametrize("dims", [(44, 44, 88, 88, 88, 88), (88, 88, 175, 175, 175, 175), (29, 43, 57, 85, 75, 120), (57, 85, 113, 170, 150, 240), (16, 16, 32, 32, 32, 32)])
def test_nnf_upsample_vs_ref64(ctx, dims):
    ahh, awh, ah, aw, bh, bw = dims
    half = synth.random_nnf(5, ahh, awh, (bh + 1) // 2, (bw + 1) // 2)
    assert np.array_equal(ctx.nnf_upsample(half, ah, aw, bh, bw), ref64.nnf_upsample(half, ah, aw, bh, bw))


def _check_pm(a, b, nnf0, nnf, d):
    bh, bw = b.shape[1:]
    x, y = nnf & 0xFFF, nnf >> 12
    assert np.all(x < bw) and np.all(y < bh)
    exp = ref64.patch_distance(a, b, nnf)
    fin = np.isfinite(exp)
    assert np.array_equal(np.isfinite(d), fin)
    assert np.abs(d[fin] - exp[fin]).max() <= 1e-5
    d0 = ref64.patch_distance(a, b, nnf0)
    both = fin & np.isfinite(d0)
    assert np.all(d[both] <= d0[both] + 1e-5)


# (C, ah, aw, bh, bw, dead feature pixels)
PM_CASES = [(512, 44, 44, 44, 44, True), (256, 175, 175, 175, 175, False), (128, 350, 350, 350, 350, False), (64, 700, 700, 700, 700, False),
            (64, 37, 300, 61, 45, True)]


@pytest.mark.parametrize("case", PM_CASES)
def test_patchmatch_distances_vs_ref64(ctx, case):
    """Both directions, every pixel: the returned distance is ref64's patch distance at the returned match (1e-5; NaN exactly where a tap of the patch is a
    dead — all-zero, hence NaN after normalisation — feature pixel), matches lie inside the other map, and no pixel ends worse than its initial match."""
    C, ah, aw, bh, bw, dead = case
    fa, fb = synth.features(31, C, ah, aw), synth.features(32, C, bh, bw)
    if dead:
        fa[:, 5:9, 7:12] = 0; fa[:, ah - 1, aw - 1] = 0; fb[:, 3:8, 2:6] = 0; fb[:, 0, 0] = 0
    a, b = ctx.feat_normalize(fa), ctx.feat_normalize(fb)
    for (p, q, seed) in ((a, b, 11), (b, a, 12)):
        nnf0 = synth.random_nnf(seed, p.shape[1], p.shape[2], q.shape[1], q.shape[2])
        nnf, d = ctx.patchmatch(p, q, nnf0, iters=5, rs_max=32, seed=seed)
        _check_pm(p, q, nnf0, nnf, d)


# ---------------------------------------------------------------- votes
# the feature vote takes C a multiple of 4 (VGG maps: 64..512), so the narrowest map is C = 4; three channels are the image vote's
@pytest.mark.parametrize("C,dims", [(4, (17, 400, 23, 31)), (64, (31, 23, 17, 17)), (512, (44, 44, 44, 44)), (256, (88, 88, 70, 95)), (64, (350, 350, 350, 350))])
@pytest.mark.parametrize("weights", [(1.0, 2.0), (2.0, 1.0)])
def test_votes_vs_ref64(ctx, C, dims, weights):
    ah, aw, bh, bw = dims
    wc, wp = weights
    pin = synth.features(7, C, bh, bw)
    ia, ib = synth.image(1, ah, aw), synth.image(2, bh, bw)
    for kind in ("random", "collapsed", "border"):
        ann = _nnf(kind, 3, ah, aw, bh, bw)
        bnn = _nnf("random" if kind == "collapsed" else kind, 4, bh, bw, ah, aw)
        got, gpw = ctx.bds_vote_features(ann, bnn, pin, wc, wp, want_pw=True)
        exp, epw = ref64.vote_features(ann, bnn, pin, wc, wp)
        assert np.allclose(got, exp, rtol=1e-5, atol=1e-6), kind
        assert np.allclose(gpw, epw, rtol=1e-5, atol=1e-12), kind
        gi = ctx.bds_vote_image(ia, ib, ann, bnn, wc, wp)
        ei, v = ref64.vote_image(ia, ib, ann, bnn, wc, wp, want_float=True)
        assert _vote_image_agrees(gi, ei, v), kind
