"""The chaining of the per-pair loop, transfer_color_single_bds (main.cu:47-454), checked level by level against tests/ref64.py.

check_levels() takes one pair's per-level dumps — the dict of oracle.process_pair(want_nnf=True) or of nct.Context.pair_run_levels(want_color=True), which have
the same keys — and recomputes from the two input images alone, in float64, what each level should have seen:
  1. pyramid    S and R chained down through the library's own resize_u8c3 (main.cu:104-108), each step < 1 LSB from ref64.resize_linear_u8_exact;
  2. features   R's taps from the full reference image (main.cu:102), S's from the source at level 0 (main.cu:94) and from the previous level's result after
                that (main.cu:424-427), normalised (main.cu:259-275): annd / bnnd are ref64.patch_distance at the dumped matches, A and B the right way round
                (main.cu:283-284), NaN exactly where ref64 gives NaN;
  3. seed bound no pixel ends worse than its seed: nnf_init at level 0 (main.cu:230-234), else the previous level's NNF upsampled with its own direction's
                geometry (main.cu:235-251);
  4. guide      ref64.vote_image on the chained level images with weights (1, bds_weight) (main.cu:291);
  5. error      minus the dot product of the normalised S features and the normalised BDS vote of R's raw features (main.cu:297-318);
  6. colour     (GPU dumps with the colour stages) T1 from the level's Lab images, S1 on the kNN graph rebuilt from the dumped labels with samples = 2^l
                (main.cu:351-359), then resize, roughness, S2 and the result (tests/test_gpu_vs_ref64.py::_check_after_s1).
Checks 2, 3 and 5 hold to TOL, absolute. Measured on the pairs of tests/test_ref64_oracle.py and tests/test_gpu_vs_ref64.py, oracle and GPU: at most 2.8e-7
(distances), 2.3e-7 (seed bound) and 2.8e-7 (matching error); TOL leaves about seven times that.

NCT_FLAG_FEAT16 (feat16=(tight, loose)): at the levels with C >= 256 PatchMatch reads its candidate tiles from fp16 copies of the normalised maps (the candidate
side is B for annd, A for bnnd). There annd / bnnd must be within `tight` of the distance with the candidate map rounded to fp16 — which a shadow map of the
wrong side (na_h for nb_h) or of the previous level would miss by the size of a feature difference, not of a rounding — and within `loose` of the exact fp32
distance, which only bounds how far fp16 tiles can move a distance. The seed bound then holds in the fp16 metric.
"""
import numpy as np
import ref64
from test_ref64_oracle import _ulp_close, _vote_image_agrees

TOL = 2e-6
# the float VGG's conv5_1 moved a float L2 distance between normalised features by at most 3.5e-6 relative from ref64's float64 taps (measured with
# synthetic_vgg19(19) on the sources of PAIR_CASES, the stand-in crop, and the bds8 / levels3 pairs, whose margins were 1.7e-3 .. 3.4e-2); the bar leaves 14x
KM_VGG_MARGIN = 5e-5
FP16_MIN_C = 256          # nct_pipeline.cpp: pm_mode = NCT_PM_FP16 for C >= 256 under NCT_FLAG_FEAT16


def _f16(x):
    """the fp16 shadow map of a normalised map: the fp32 map rounded to nearest (k_feat.hip, __floats2half2_rn)"""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def _max_dev(got, exp, what):
    """max |got - exp| over the finite pixels; NaN must sit at the same pixels in both"""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    ng, ne = np.isnan(got), np.isnan(exp)
    assert np.array_equal(ng, ne), f"{what}: NaN differs from ref64 at {int((ng != ne).sum())} pixels"
    assert np.isfinite(got[~ng]).all() and np.isfinite(exp[~ne]).all(), what
    return float(np.abs(got[~ng] - exp[~ne]).max(initial=0.0))


def _seed_margin(d, d0, what):
    """max (d - d0) where the seed's distance d0 is finite: PatchMatch keeps a candidate only when it is strictly better (GeneralizedPatchMatch.cu:520-525),
    so a finite seed never ends NaN and never ends worse"""
    d, d0 = np.asarray(d, np.float64), np.asarray(d0, np.float64)
    fin = np.isfinite(d0)
    assert np.isfinite(d[fin]).all(), f"{what}: a pixel with a finite seed distance ended NaN"
    return float((d[fin] - d0[fin]).max(initial=-np.inf))


def chain_pyramid(img, sizes, resize):
    """main.cu:104-108: level l is resize(level l + 1), down from the full image. sizes: [(h, w)] per level, coarse -> fine. Returns (pyramid, max |u8 - exact|)."""
    pyr = [None] * len(sizes)
    pyr[-1] = np.asarray(img, np.uint8)
    worst = 0.0
    for l in range(len(sizes) - 2, -1, -1):
        h, w = sizes[l]
        pyr[l] = np.asarray(resize(pyr[l + 1], h, w), np.uint8)
        d = float(np.abs(pyr[l] - ref64.resize_linear_u8_exact(pyr[l + 1], h, w)).max())
        assert d < 1.0, f"pyramid level {l}: {d} LSB from the exact bilinear value"
        worst = max(worst, d)
    return pyr, worst


def check_levels(dumps, src, ref, ws, bs, bds_weight, lib, levels=5, feat16=None, s1_maxit=None, lab2bgr_form=None, prm=None, cluster_num=10):
    """Runs checks 1-5 at every level that ran (and 6 when `dumps` holds "color"). lib: the library that made the dumps (the oracle or an nct.Context); its
    resize_u8c3 builds the pyramids (each step checked against the exact bilinear value), its bgr2lab the Lab bytes and its lab2bgr the expected result image —
    both conversions are pinned to ref64 over all 2^24 inputs (tests/test_ref64_oracle.py::check_bgr2lab_all, check_lab2bgr_all). The kNN graph is ref64's,
    over the dumped labels, which must be ref64.kmeans_labels of the source's float64 conv5_1 (with a margin of KM_VGG_MARGIN). s1_maxit: NCT_S1_MAXIT of the run — S1's iterate must then equal ref64's literal CGNR from the
    dumped T1 guess to 1e-10. lab2bgr_form: the Lab -> BGR form the run used (1 under NCT_FLAG_LAB2BGR_CUBE). prm, cluster_num: the colour parameters and the cluster
    count of the run (None: test_ref64_oracle.COLOR_DEFAULTS; 10). Returns {check: largest deviation}."""
    from test_gpu_vs_ref64 import _chan, _check_after_s1, _lab2bgr_of
    from test_ref64_oracle import COLOR_DEFAULTS, S1_CAP_RATIO
    prm = COLOR_DEFAULTS if prm is None else prm
    src, ref = np.asarray(src, np.uint8), np.asarray(ref, np.uint8)
    H, W = src.shape[:2]
    RH, RW = ref.shape[:2]
    geo = ref64.level_geometry(H, W, RH, RW)
    stats = {}

    def note(k, v):
        stats[k] = max(stats.get(k, -np.inf), v)

    resize = lib.resize_u8c3
    spyr, ds = chain_pyramid(src, [(g["ah"], g["aw"]) for g in geo], resize)
    rpyr, dr = chain_pyramid(ref, [(g["bh"], g["bw"]) for g in geo], resize)
    note("pyramid", max(ds, dr))
    rtaps = ref64.vgg19_taps(ref, ws, bs, 5)
    s_raw = ref64.vgg19_taps(src, ws, bs, 5)[4]
    flab = None
    if "color" in dumps:
        flab = lib.bgr2lab(src).reshape(-1, 3) / 255.0
        # C1: the labels the colour stages used are the k-means of the source's conv5_1, here computed in float64 from the image alone
        el, en, margin = ref64.kmeans_labels(s_raw, cluster_num, 11, 1)
        assert margin >= KM_VGG_MARGIN, f"k-means margin {margin:.3g}: the pair cannot tell a label error from the float VGG's rounding"
        assert int(dumps["labels"].max()) + 1 == en and np.array_equal(dumps["labels"], el), "labels differ from ref64.kmeans_labels"
        note("km_margin_min", -margin)
    for l in range(levels):
        g = geo[l]
        ah, aw, bh, bw, C = g["ah"], g["aw"], g["bh"], g["bw"], g["C"]
        ann, bnn = dumps["ann"][l], dumps["bnn"][l]
        assert ann.shape == (ah, aw) and bnn.shape == (bh, bw), l
        ax, ay = ann & 0xFFF, ann >> 12
        bx, by = bnn & 0xFFF, bnn >> 12
        assert ax.max() < bw and ay.max() < bh and bx.max() < aw and by.max() < ah, f"level {l}: a match outside the other map"
        if l > 0:
            s_raw = ref64.vgg19_taps(dumps["result"][l - 1], ws, bs, g["tap"])[-1]
        r_raw = rtaps[g["tap"] - 1]
        assert s_raw.shape == (C, ah, aw) and r_raw.shape == (C, bh, bw), l
        na, nb = ref64.normalize(s_raw), ref64.normalize(r_raw)
        # 2. distances at the dumped matches, 3. seed bound
        seed_a = ref64.nnf_init(ah, aw, bh, bw) if l == 0 else ref64.nnf_upsample(dumps["ann"][l - 1], ah, aw, bh, bw)
        seed_b = ref64.nnf_init(bh, bw, ah, aw) if l == 0 else ref64.nnf_upsample(dumps["bnn"][l - 1], bh, bw, ah, aw)
        for key, p, q, nnf, seed in (("annd", na, nb, ann, seed_a), ("bnnd", nb, na, bnn, seed_b)):
            d = dumps[key][l]
            exact = ref64.patch_distance(p, q, nnf)
            if feat16 is not None and C >= FP16_MIN_C:
                tight, loose = feat16
                q16 = _f16(q)
                dev = _max_dev(d, ref64.patch_distance(p, q16, nnf), f"level {l}: {key} vs the fp16-candidate distance")
                assert dev <= tight, f"level {l}: {key} is {dev:.3g} from the fp16-candidate distance (bound {tight:.3g})"
                note(key + "_fp16", dev)
                dev = _max_dev(d, exact, f"level {l}: {key} vs the exact distance")
                assert dev <= loose, f"level {l}: {key} is {dev:.3g} from the exact distance (bound {loose:.3g})"
                note(key + "_fp16_vs_exact", dev)
                m = _seed_margin(d, ref64.patch_distance(p, q16, seed), f"level {l}: {key}")
                assert m <= tight, f"level {l}: {key} ends {m:.3g} worse than its seed (fp16 metric)"
                note("seed_fp16", m)
            else:
                dev = _max_dev(d, exact, f"level {l}: {key}")
                assert dev <= TOL, f"level {l}: {key} is {dev:.3g} from ref64's patch distance"
                note(key, dev)
                m = _seed_margin(d, ref64.patch_distance(p, q, seed), f"level {l}: {key}")
                assert m <= TOL, f"level {l}: {key} ends {m:.3g} worse than its seed"
                note("seed", m)
        # 4. guidance image
        exp, v = ref64.vote_image(spyr[l], rpyr[l], ann, bnn, 1.0, bds_weight, want_float=True)
        assert _vote_image_agrees(dumps["guide"][l], exp, v), f"level {l}: the guidance image differs from ref64's vote"
        note("guide_px", float((dumps["guide"][l] != exp).any(-1).mean()))
        # 5. matching error
        voted, _ = ref64.vote_features(ann, bnn, r_raw, 1.0, bds_weight)
        dev = _max_dev(dumps["err"][l], ref64.feature_distance(na, ref64.normalize(voted)), f"level {l}: err")
        assert dev <= TOL, f"level {l}: err is {dev:.3g} from ref64's matching error"
        note("err", dev)
        # 6. colour stage
        if "color" in dumps:
            gs = dumps["color"][l]
            slab_u8, glab_u8 = lib.bgr2lab(spyr[l]), lib.bgr2lab(dumps["guide"][l])
            labels = dumps["labels"]
            ids, kw = ref64.knn_graph(slab_u8, labels, int(labels.max()) + 1, g["knn_samples"])
            ea, eb = ref64.local_stats(slab_u8, glab_u8, prm["eps"])
            assert _ulp_close(gs["ab_local"][0], ea, 2) and _ulp_close(gs["ab_local"][1], eb, 2), f"level {l}: T1"
            slab, glab = slab_u8.reshape(-1, 3) / 255.0, glab_u8.reshape(-1, 3) / 255.0
            system = ref64.s1_system(slab, glab, ref64.err_weight(dumps["err"][l]), ids, kw, ah, aw, prm["local_weight"], prm["wls_alpha"], H * W / (ah * aw),
                                     nonlocal_weight=prm["nonlocal_weight"])
            cap = s1_maxit if s1_maxit else (50 if l == 4 else 100)
            for c in range(3):
                A, rhs = system[c]
                x0, xg = _chan(gs["ab_local"], c), _chan(gs["ab_nonlocal"], c)
                xr, k = ref64.s1_cg(A, rhs, x0, cap)
                assert gs["cg_iters"][c] <= cap, f"level {l}: S1 ran {gs['cg_iters'][c]} iterations on channel {c}"
                if s1_maxit:
                    assert gs["cg_iters"][c] == k, f"level {l}: S1 ran {gs['cg_iters'][c]} iterations on channel {c}, ref64 {k}"
                    assert np.allclose(xg, xr, rtol=1e-10, atol=1e-10), f"level {l}: S1 after {s1_maxit} iterations, channel {c}"
                    note("s1_short", float(np.abs(xg - xr).max()))
                else:
                    f0, fg, fr = (ref64.s1_objective(A, rhs, x) for x in (x0, xg, xr))
                    assert fg <= f0, f"level {l}: S1 raised the energy on channel {c}"
                    # the energy check of test_color_stages_vs_ref64; on the few-pixel coarse levels of a small pair both iterates end within 1e-4 of
                    # the descent from the T1 guess of each other — near the minimum, where the ratio of two tiny energies says nothing (17x17 at 9x9: 1.15)
                    assert S1_CAP_RATIO[0] <= fg / fr <= S1_CAP_RATIO[1] or abs(fg - fr) <= 1e-4 * (f0 - fr), (l, c, f0, fg, fr)
                    note("s1_ratio_dev", abs(fg / fr - 1.0))
                    note("s1_rel_descent_dev", abs(fg - fr) / (f0 - fr))
            _check_after_s1(_lab2bgr_of(lib), gs, dumps["result"][l], H, W, ah, aw, flab, form=lab2bgr_form, step_bound=True, prm=prm)
    return stats
