"""The kernels vs tests/ref64.py, the float64 restatements written from the reference's text, at the production and edge shapes — a check that does not go
through the oracle, whose operator order the kernels mirror. Each colour stage is compared with ref64 applied to the GPU's own previous stage."""
import numpy as np
import pytest
import ref64
import synth
from test_gpu_color import _level_case
from test_ref64_oracle import COLOR_DEFAULTS, S1_CAP_RATIO, _ulp_close, _vote_image_agrees, _nnf_pair, vote_tol_scale

pytestmark = pytest.mark.gpu

# the cases of test_gpu_color.py::test_local_color_transfer_stages (k_s1_hub, the shared-gather operator, the 48x8 V-cycle tiles) and one 17x400 level
COLOR_CASES = [(48, 48, 12, 12, (3, 3), 4, 2), (40, 56, 20, 28, (5, 7), 4, 3), (32, 32, 32, 32, (2, 2), 16, 4), (372, 368, 372, 368, (23, 23), 16, 4),
               (96, 96, 48, 48, (3, 3), 16, 3, "flat"), (160, 160, 80, 80, (5, 5), 16, 2, "flat"), (64, 64, 64, 64, (4, 4), 16, 4, "flat"),
               (372, 368, 372, 368, (23, 23), 16, 4, "flat"), (34, 800, 17, 400, (2, 20), 4, 3)]


def _case(ctx, case):
    """test_gpu_color._level_case's inputs built without the oracle: the GPU's resize and Lab conversion (each pinned to ref64: the pyramid check of
    tests/levels_ref64.py and test_lab_conversions_all_inputs_vs_ref64) and ref64's kNN graph over the same label grid"""
    H, W, h, w, grid, samples, layer = case[:7]
    seed, mk = 20 + layer, (synth.image_flat if len(case) > 7 else synth.image)
    full = mk(seed, H, W)
    s = ctx.resize_u8c3(full, h, w) if (h, w) != (H, W) else full
    g = ctx.resize_u8c3(mk(seed + 1, H, W), h, w)
    lh, lw = grid
    labels = (np.arange(lh * lw).reshape(lh, lw) % 3).astype(np.int32)
    ids, ws = ref64.knn_graph(ctx.bgr2lab(s), labels, 3, samples)
    err = -np.random.default_rng(seed).random((h, w)).astype(np.float32)
    slab = ctx.bgr2lab(s).reshape(-1, 3) / 255.0
    glab = ctx.bgr2lab(g).reshape(-1, 3) / 255.0
    flab = ctx.bgr2lab(full).reshape(-1, 3) / 255.0
    return H, W, h, w, layer, err, s, g, full, ids, ws, slab, glab, flab


def _lab2bgr_of(lib):
    return lambda lab, form: lib.lab2bgr(lab, form=0 if form is None else form)


def _chan(ab, c):
    return np.r_[ab[0][:, c], ab[1][:, c]]


def _check_after_s1(lab2bgr, gs, go, H, W, h, w, flab, form=None, step_bound=False, prm=COLOR_DEFAULTS, stats=None):
    """U1, roughness, S2 and A1, each against ref64 applied to the GPU's previous stage; form: the Lab -> BGR form of the run (None: the default, piecewise).
    The result image must be exactly lab2bgr(lab, form) — the library's own conversion, pinned over all 2^24 inputs by check_lab2bgr_all — of ref64's Lab
    bytes, and within 1 LSB of ref64.lab2bgr of them outside the cube form's far-out channels. The upsampled
    coefficients lie within 1e-7 relative of the pure float64 mapping, or — step_bound, for the large ratios of a whole pyramid (2x2 -> 17x17), where an
    interpolant near zero between large coefficients breaks a relative bound — within what OpenCV's float table allows in each of the two passes: the float
    source coordinate (half an ulp of the largest coordinate) times the largest step between neighbours, plus the float weights 1 - fx, fx (half an ulp of 1
    each) times the largest coefficient; plus the 4 ulp above. prm: the colour parameters of the run (S2 reads wls_lambda_init and wls_alpha); stats
    (a dict, optional) receives "s2_frac", the largest |S2 - exact| / (atol + rtol |exact|). Returns
    the number of pixels where channel 0 or 1 leaves [0, 1] and channel 2 does not (only the last channel decides the roughness)."""
    if (h, w) != (H, W):
        for p in range(2):
            src = gs["ab_nonlocal"][p].reshape(h, w, 3)
            up = ref64.resize_linear_f64(src, H, W).reshape(-1, 3)
            assert _ulp_close(gs["ab_up"][p], up, 4), p
            up64 = ref64.resize_linear_f64(src, H, W, float_coeffs=False).reshape(-1, 3)
            if step_bound:
                step = max(np.abs(np.diff(src, axis=0)).max(initial=0), np.abs(np.diff(src, axis=1)).max(initial=0))
                bound = 2 * (np.spacing(np.float32(max(h, w))) * step + np.spacing(np.float32(1)) * np.abs(src).max()) + 4 * np.spacing(np.abs(up64)) + 1e-15
                assert np.all(np.abs(gs["ab_up"][p] - up64) <= bound), p
            else:
                assert np.all(np.abs(gs["ab_up"][p] - up64) <= 1e-7 * np.abs(up64) + 1e-15), p
    else:
        assert np.array_equal(gs["ab_up"], gs["ab_nonlocal"])
    assert np.array_equal(gs["roughness"], ref64.roughness(gs["ab_up"], flab))
    lam = prm["wls_lambda_init"] * (H * W) / (h * w) * (4 if (h, w) == (H, W) else 1)
    exact = ref64.wls_solve_exact(gs["ab_up"], flab, H, W, lam, prm["wls_alpha"], gs["roughness"])
    if stats is not None:
        stats["s2_frac"] = max(stats.get("s2_frac", 0.0), float((np.abs(gs["ab_wls"] - exact) / (2e-6 + 2e-5 * np.abs(exact))).max()))
    assert np.allclose(gs["ab_wls"], exact, rtol=2e-5, atol=2e-6)
    lab_out = ref64.apply_coeffs(gs["ab_wls"], flab)
    assert np.array_equal(go, lab2bgr(lab_out.reshape(H, W, 3), form))
    exp, far = ref64.lab2bgr(lab_out, 1 if form == 1 else 0)
    assert np.abs(go.reshape(-1, 3).astype(np.float64) - exp)[~far].max() <= 1
    nc = flab * gs["ab_up"][0] + gs["ab_up"][1]
    out = (nc < 0) | (nc > 1)
    return int((out[:, :2].any(1) & ~out[:, 2]).sum())


@pytest.mark.parametrize("case", COLOR_CASES)
def test_color_stages_vs_ref64(ctx, case):
    """T1 within 2 ulp; S1 at the reference's cap: the energy |A x - rhs|^2 of ref64's system falls from the T1 guess and lands within S1_CAP_RATIO of the literal
    CGNR's (calibration: tests/test_ref64_oracle.py); U1, roughness, S2 (exact solve) and A1 as in _check_after_s1."""
    H, W, h, w, layer, err, s, g, full, ids, ws, slab, glab, flab = _case(ctx, case)
    go, gs = ctx.local_color_transfer(err, s, g, full, ids, ws, layer, want_stages=True)
    ea, eb = ref64.local_stats(ctx.bgr2lab(s), ctx.bgr2lab(g), 0.60)
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
    mixed = _check_after_s1(_lab2bgr_of(ctx), gs, go, H, W, h, w, flab)
    if len(case) > 7 and case[0] == 372:
        assert mixed > 0, "this case is meant to hold pixels where only channel 0 or 1 leaves [0, 1]"


@pytest.mark.parametrize("case", [COLOR_CASES[i] for i in (0, 1, 3, 4, 7, 8)])
def test_s1_short_runs_vs_literal_cg(ctx, case, monkeypatch):
    """NCT_S1_MAXIT = 1, 2, 5: the GPU's S1 iterate vs ref64's literal CGNR from the GPU's own T1 guess, at the agreement the oracle's two forms show
    (test_canonical_cg_matches_explicit_for_few_iterations); the reported iteration counts follow the hook."""
    import nct
    H, W, h, w, layer, err, s, g, full, ids, ws, slab, glab, flab = _case(ctx, case)
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


def test_flat_guide_skips_the_zero_rhs(ctx):
    """A guide of one colour: a = 0 everywhere after T1, the T1 guess already solves S1 (no iteration), and S2 skips the all-zero a right-hand sides
    (ColorTransfer.cpp:1000-1030 with solve_direct_cpu) — their result stays 0."""
    H, W, h, w, layer, err, s, g, full, ids, ws, slab, glab, flab = _case(ctx, COLOR_CASES[1])
    g = np.full_like(g, (90, 140, 60))
    go, gs = ctx.local_color_transfer(err, s, g, full, ids, ws, layer, want_stages=True)
    assert np.all(gs["ab_local"][0] == 0) and gs["cg_iters"].tolist() == [0, 0, 0]
    assert np.all(gs["ab_wls"][0] == 0)
    _check_after_s1(_lab2bgr_of(ctx), gs, go, H, W, h, w, flab)


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
    for kind in ("random", "collapsed", "border", "collapsed_b"):          # collapsed_b: the R -> S field collapsed, the hub pass's long source lists
        ann, bnn = _nnf_pair(kind, 3, 4, ah, aw, bh, bw)
        got, gpw = ctx.bds_vote_features(ann, bnn, pin, wc, wp, want_pw=True)
        exp, epw = ref64.vote_features(ann, bnn, pin, wc, wp)
        k = vote_tol_scale(bnn, ah, aw)                      # 1, but for collapsed_b at 350 x 350: the calibration stands at VOTE_LONG_LIST_SCALE
        assert np.allclose(got, exp, rtol=k * 1e-5, atol=k * 1e-6), kind
        assert np.allclose(gpw, epw, rtol=k * 1e-5, atol=k * 1e-12), kind
        gi = ctx.bds_vote_image(ia, ib, ann, bnn, wc, wp)
        ei, v = ref64.vote_image(ia, ib, ann, bnn, wc, wp, want_float=True)
        assert _vote_image_agrees(gi, ei, v), kind


# ---------------------------------------------------------------- the chained loop (main.cu:47-454)
# NCT_FLAG_FEAT16 bounds at the fp16-candidate levels (tests/levels_ref64.py): (vs the distance with the candidate map rounded to fp16, vs the exact distance).
# Measured on both FEAT16 pairs below: at most 5.2e-6 (distances and seed bound in the fp16 metric) and 8.9e-5 (vs exact); the bounds leave about four and
# five times that.
FEAT16_TOL = (2e-5, 5e-4)


@pytest.fixture(scope="module")
def vgg():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


def _pair_run(c, vgg, src, ref, bds=2.0, levels=5, flags=0):
    import nct
    c.vgg19_load_raw(*vgg)
    prm = nct.Params.default(); prm.bds_weight = bds; prm.levels = levels; prm.flags = flags
    c.pair_upload(src, ref)
    lv = c.pair_run_levels(src.shape, ref.shape, prm, want_color=True)
    assert np.array_equal(c.pair_download(), lv["result"][levels - 1]), "the final image is not the last level's result"
    return lv


def _check_pair(c, vgg, src, ref, bds, tag, levels=5, **kw):
    import levels_ref64
    lv = _pair_run(c, vgg, src, ref, bds, levels, kw.pop("flags", 0))
    stats = levels_ref64.check_levels(lv, src, ref, *vgg, bds, c, levels=levels, **kw)
    print("ref64-levels", tag, {k: float("%.3g" % v) for k, v in stats.items()})
    return lv, stats


def _standin_crop():
    """160x200 crops of the in4 / tar4 stand-ins: regions of one colour, i.e. kNN hubs, at full resolution"""
    import os
    import natural_inputs
    from PIL import Image
    d = natural_inputs.require()
    im = [np.asarray(Image.open(os.path.join(d, n + ".png")).convert("RGB"))[..., ::-1] for n in ("in4", "tar4")]
    return np.ascontiguousarray(im[0][4:164, 16:216]), np.ascontiguousarray(im[1][10:170, 30:230])


@pytest.mark.parametrize("case", __import__("test_ref64_oracle").PAIR_CASES)
def test_pair_levels_vs_ref64_gpu(ctx, vgg, case):
    """Every level of the GPU pair against ref64 recomputed from the two input images (tests/levels_ref64.py), colour stages included: T1, S1 at the cap on the
    kNN graph rebuilt from the dumped labels with samples = 2^l, resize, roughness, S2, the result."""
    from test_ref64_oracle import pair_images
    src, ref = pair_images(case)
    _check_pair(ctx, vgg, src, ref, case[2], case[:3])


def test_pair_levels_vs_ref64_standin_crop(ctx, vgg):
    import nct
    src, ref = _standin_crop()
    _check_pair(ctx, vgg, src, ref, 2.0, "standin")
    hub = ctx.counter(nct.CTR_S1_HUB_BLOCKS_L0 + 4)
    assert hub > 0 or hub == -1, f"the crop is meant to have kNN hubs at the finest level ({hub})"


def test_pair_levels_vs_ref64_dead_feature_pixels(ctx, vgg):
    """test_gpu_pipeline.py::test_pair_with_dead_feature_pixels_matches_oracle's pair: conv1_1 answers 0 in every channel inside a black rectangle of R, so the
    normalised map holds NaN there and the distances of patches touching it are NaN — at the same pixels as ref64's."""
    ws, bs = [w.copy() for w in vgg[0]], [b.copy() for b in vgg[1]]
    mean = np.asarray(ref64.VGG_MEAN_BGR, np.float32)
    bs[0] = (-(ws[0].sum(axis=(2, 3)) * (-mean)[None, :]).sum(1) - 1.0).astype(np.float32)
    src, ref = synth.image(1000, 96, 80), synth.image(1001, 72, 104)
    ref[20:30, 30:44] = 0
    lv, _ = _check_pair(ctx, (ws, bs), src, ref, 2.0, "dead")
    assert np.isnan(lv["bnnd"][4]).any(), "R -> S queries inside the dead region keep a NaN distance"


def test_pair_levels_vs_ref64_bds8_and_partial(ctx, vgg):
    """bds_weight 8 (completeness ahead of coherence), and a run of three levels (nct_params.levels) whose last result is the final image"""
    _check_pair(ctx, vgg, synth.image_flat(1000, 112, 96), synth.image_flat(1001, 80, 128), 8.0, "bds8")
    _check_pair(ctx, vgg, synth.image(11, 88, 72), synth.image(12, 64, 96), 2.0, "levels3", levels=3)


def test_pair_levels_vs_ref64_s1_short(vgg, monkeypatch):
    """NCT_S1_MAXIT=2: at every level S1's iterate equals ref64's literal CGNR over two iterations from the dumped T1 guess (1e-10, as in
    test_s1_short_runs_vs_literal_cg) — a tight check of the graph, weights and sizes the pipeline hands to S1."""
    import nct
    from test_ref64_oracle import PAIR_CASES, pair_images
    monkeypatch.setenv("NCT_S1_MAXIT", "2")
    src, ref = pair_images(PAIR_CASES[0])
    with nct.Context(0) as c:
        _check_pair(c, vgg, src, ref, PAIR_CASES[0][2], "s1_maxit2", s1_maxit=2)


def test_pair_levels_vs_ref64_feat16(ctx, vgg):
    """NCT_FLAG_FEAT16, which the oracle does not model: at the C >= 256 levels the distances are those of fp16 candidate tiles (FEAT16_TOL), elsewhere and in
    every other check the fp32 bounds hold"""
    import nct
    from test_ref64_oracle import PAIR_CASES, pair_images
    for tag, (src, ref) in (("feat16", pair_images(PAIR_CASES[0])), ("feat16_standin", _standin_crop())):
        _check_pair(ctx, vgg, src, ref, 2.0, tag, flags=nct.FLAG_FEAT16, feat16=FEAT16_TOL)


def test_pair_levels_vs_ref64_lab2bgr_cube(ctx, vgg):
    """NCT_FLAG_LAB2BGR_CUBE: every level's result is the plain-cube Lab -> BGR form of ref64's coefficients applied to the source"""
    import nct
    from test_ref64_oracle import PAIR_CASES, pair_images
    src, ref = pair_images(PAIR_CASES[0])
    lv, _ = _check_pair(ctx, vgg, src, ref, 2.0, "cube", flags=nct.FLAG_LAB2BGR_CUBE, lab2bgr_form=1)
    base = _pair_run(ctx, vgg, src, ref)
    assert not np.array_equal(lv["result"][4], base["result"][4]), "the cube form is meant to change some pixel of this pair"


# ---------------------------------------------------------------- A1, C1, K1 against ref64
def test_lab_conversions_all_inputs_vs_ref64(ctx):
    """every 8-bit BGR and Lab triple, both Lab -> BGR forms, within the bounds of test_ref64_oracle.py (BGR2LAB_BANDS, 1 LSB outside the far-out channels)"""
    from test_ref64_oracle import check_bgr2lab_all, check_lab2bgr_all
    print("bgr2lab", check_bgr2lab_all(ctx.bgr2lab).round(3).tolist())
    print("lab2bgr", check_lab2bgr_all(lambda lab, form: ctx.lab2bgr(lab, form=form)))


@pytest.mark.parametrize("case", __import__("test_ref64_oracle").KM_CASES, ids=[c[0] for c in __import__("test_ref64_oracle").KM_CASES])
def test_kmeans_labels_vs_ref64_gpu(ctx, case):
    """the CPU cases (n on both sides of KM_LDS_PERM = 4096, duplicate rejection deep into the permutation, donor, cap, early stop, one label)"""
    from test_ref64_oracle import check_kmeans
    name, mk, seeds, expect = case[:4]
    f = mk()
    for seed in seeds:
        print(name, seed, "margin %.3g" % check_kmeans(ctx.cluster_features, ctx.feat_normalize, f, seed, expect, *case[4:]))


@pytest.mark.parametrize("size", [700, 1000])
def test_kmeans_labels_of_gpu_conv5_vs_ref64(ctx, vgg, size):
    """conv5_1 of the GPU's own VGG at 44 x 44 (a 700^2 source) and 63 x 63: the labels are ref64's k-means of the GPU's normalised map bit for bit (every
    float operation emulated, so no margin is needed); the margin against ref64's normalisation is reported"""
    from test_ref64_oracle import check_kmeans
    ctx.vgg19_load_raw(*vgg)
    img = synth.image_flat(700 + size, size, size)
    f = ctx.vgg19_features(img, 5)[4]
    assert f.shape[1:] == ((44, 44) if size == 700 else (63, 63))
    for seed in (1, 2):
        print(size, seed, "margin %.3g" % check_kmeans(ctx.cluster_features, ctx.feat_normalize, f, seed, None, need_margin=False))


def _knn_pair_images(kind):
    if kind == "flat":
        img = synth.image_flat(9, 700, 700)
    elif kind == "standin":
        import os
        import natural_inputs
        from PIL import Image
        im = np.asarray(Image.open(os.path.join(natural_inputs.require(), "in4.png")).convert("RGB"))[..., ::-1]
        img = np.ascontiguousarray(np.repeat(np.repeat(im[:350, :350], 2, 0), 2, 1))      # upscaled: runs of equal colours
    else:
        img = synth.image_flat(10, 300, 1000)
    img = img.copy()
    h, w = img.shape[:2]
    img[h // 2:h // 2 + 3, : w // 3] = (255, 0, 255)                  # isolated far colours: the bounded-ring fallback
    img[0, 0] = (0, 255, 0)
    img[h - 1, w - 1] = (0, 0, 255)
    return img


@pytest.mark.parametrize("kind", ["flat", "standin", "elongated"])
def test_knn_graph_pyramid_vs_ref64(kind, monkeypatch):
    """K1 at every level of a pair's pyramid (700 x 700: 44 .. 700, samples 1 .. 16 over a 44 x 44 label grid; 300 x 1000 for the elongated one), under both
    search forms (NCT_KNN_RUNS = 0, 1): ids exactly, weights within 4e-16 relative of ref64.knn_graph. The fine levels reach the 8-unit and the 2-unit cells."""
    import nct
    img = _knn_pair_images(kind)
    H, W = img.shape[:2]
    geo = ref64.level_geometry(H, W, H, W)
    lh, lw = geo[0]["ah"], geo[0]["aw"]
    labels = ((np.arange(lh * lw).reshape(lh, lw) // 5 + np.arange(lh)[:, None] // 3) % 10).astype(np.int32)
    labels[lh // 2, lw // 2] = 9
    with nct.Context(0) as c:
        pyr = [None] * 5
        pyr[4] = img
        for l in range(3, -1, -1):
            pyr[l] = c.resize_u8c3(pyr[l + 1], geo[l]["ah"], geo[l]["aw"])
        labs = [c.bgr2lab(p) for p in pyr]
    exp = [ref64.knn_graph(labs[l], labels, 10, geo[l]["knn_samples"]) for l in range(5)]
    for runs in ("0", "1"):
        monkeypatch.setenv("NCT_KNN_RUNS", runs)
        with nct.Context(0) as c:
            for l in range(5):
                gi, gw = c.knn_graph(labs[l], labels, 10, geo[l]["knn_samples"])
                pad, dev = __import__("test_ref64_oracle").check_knn(gi, gw, *exp[l], f"{kind} level {l} runs {runs}")
                print(kind, l, runs, "padded", pad, "max rel dev %.3g" % dev)
