"""Region selection from strokes (SPEC §6.16) without a GPU: the properties of the numpy rule (tests/region_select_ref.py) — the subsample keeps exactly max_seeds, the
int32 bound of rule 2, mixed cells, the copy at tap 1, the stamp — and what the rule is for: on two textures with the same grey values and the same mean the matte from
VGG19 features finds the object where a colour-only rule cannot. Features come from the oracle's VGG19 with the synthetic weights. The binding's surface is checked too."""
import numpy as np
import pytest

import nct
import region_select_ref as sel


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def texture():
    return sel.texture_fixture()


@pytest.fixture(scope="module")
def texture_taps(oracle, weights, texture):
    return oracle.vgg19_features(texture[0], *weights, deepest_tap=2)


def test_binding_has_the_calls():
    for name in ("nct_region_select_params_default", "nct_region_select", "nct_region_select_dev", "nct_feat_quantize", "nct_feat_quantize_dev", "nct_region_score",
                 "nct_region_score_dev", "nct_pair_select_region", "nct_seq_select_region"):
        assert name in nct.SIGNATURES and hasattr(nct.lib(), name), name
    for name in ("region_select", "feat_quantize", "region_score", "pair_select_region", "seq_select_region"):
        assert callable(getattr(nct.Context, name)), name
    p = nct.RegionSelectParams.default()
    assert (p.tap, p.sharpness, p.floor_permille, p.max_seeds, p.snap_iters) == (sel.TAP, sel.SHARPNESS, sel.FLOOR_PERMILLE, sel.MAX_SEEDS, sel.SNAP_ITERS) == (2, 1024, 700, 4096, 1)
    assert (p.snap.radius, p.snap.sigma, p.snap.binary) == sel.SNAP == (3, 10, 1)
    assert (nct.STROKE_IN, nct.STROKE_OUT) == (sel.IN, sel.OUT) == (255, 128)


@pytest.mark.parametrize("max_seeds", [1, 2, 7, 64, 4096])
def test_the_subsample_keeps_exactly_max_seeds(max_seeds):
    """n from max_seeds to 3 max_seeds (every n for the small ones, a stride and both ends for 4096); below it every seed is kept; the kept ranks are increasing and
    the slot a kept seed takes, floor(i max_seeds / n), counts the kept seeds in front of it"""
    ns = range(max_seeds, 3 * max_seeds + 1) if max_seeds <= 64 else [4096, 4097, 5000, 8191, 8192, 8193, 12287, 12288]
    for n in ns:
        k = sel.kept(n, max_seeds)
        assert k.sum() == max_seeds, (n, max_seeds)
        i = np.nonzero(k)[0].astype(np.int64)
        assert np.array_equal(i * max_seeds // n, np.arange(max_seeds)), (n, max_seeds)
    for n in range(0, max_seeds, max(1, max_seeds // 9)):
        assert sel.kept(n, max_seeds).all()


def test_the_int32_bound_holds(oracle, texture_taps):
    """rule 2: |q| < 32780 on the fixtures' rows, so by Cauchy-Schwarz every dot product and every partial sum of it is below 2^31; checked on the partial sums too"""
    for F in texture_taps:
        q = sel.quantize(oracle, F).astype(np.int64)
        assert np.sqrt((q * q).sum(axis=1).max()) < 32780
        assert 32780 ** 2 < 2 ** 31
        rows = q[:: max(1, len(q) // 97)]
        part = np.cumsum(rows[:, None, :] * rows[None, :, :], axis=-1)
        assert np.abs(part).max() < 2 ** 31
    import synth
    q = sel.quantize(oracle, synth.features(3, 512, 9, 11)).astype(np.int64)
    assert np.sqrt((q * q).sum(axis=1).max()) < 32780


def test_quantize_zero_pixel_and_unit_pixel(oracle):
    f = np.random.default_rng(2).random((64, 3, 5), dtype=np.float32)
    f[:, 1, 2] = 0
    f[:, 2, 4] = 0; f[17, 2, 4] = 3.5
    q = sel.quantize(oracle, f)
    assert not q[1 * 5 + 2].any()
    assert q[2 * 5 + 4][17] == 32767 and np.count_nonzero(q[2 * 5 + 4]) == 1


def test_a_mixed_cell_is_no_seed():
    T = sel.call_strokes(56, 64)
    for tap, mixed in ((1, 0), (2, 1), (3, 2), (5, 1)):
        code, i_in, i_out = sel.seed_cells(T, tap, 7)
        assert (code == sel.MIXED).sum() == mixed, tap
        wt = code.shape[1]
        if tap >= 2:
            c = (31 >> (tap - 1)) * wt + (37 >> (tap - 1))
            assert code.flat[c] == sel.MIXED and c not in i_in and c not in i_out
        kept_in, kept_out = (code == sel.IN_KEPT).sum(), (code == sel.OUT_KEPT).sum()
        assert kept_in == len(i_in) == min(7, kept_in + (code == sel.IN_DROPPED).sum())
        assert kept_out == len(i_out) == min(7, kept_out + (code == sel.OUT_DROPPED).sum())
        if tap <= 3:
            assert (code == sel.IN_DROPPED).any() and (code == sel.OUT_DROPPED).any(), tap
    # an inside stroke that lies only in mixed cells leaves no inside seed
    T = np.zeros((56, 64), np.uint8); T[20, 20] = sel.IN; T[21, 21] = sel.OUT
    assert len(sel.seed_cells(T, 1, 7)[1]) == 1 and len(sel.seed_cells(T, 2, 7)[1]) == 0


def test_tap_1_copies_and_stamped_pixels_survive(oracle, weights):
    src, T = sel.call_source(56, 64), sel.call_strokes(56, 64)
    taps = oracle.vgg19_features(src, *weights, deepest_tap=2)
    M0, st = sel.select(oracle, src, T, *weights, tap=1, max_seeds=7, snap_iters=0, feat=taps[0])
    assert np.array_equal(st["up"], st["score"])
    assert np.array_equal(M0, sel.stamp(st["score"], T))
    for tap in (1, 2):
        for iters in (0, 1, 2):
            M, _ = sel.select(oracle, src, T, *weights, tap=tap, max_seeds=7, snap_iters=iters, feat=taps[tap - 1])
            assert (M[T == sel.IN] == 255).all() and (M[T == sel.OUT] == 0).all(), (tap, iters)
    with pytest.raises(sel.NoInsideSeed):
        sel.select(oracle, src, np.where(T == sel.OUT, T, 0).astype(np.uint8), *weights, tap=1, feat=taps[0])


def test_texture_features_find_the_object_colour_does_not(oracle, weights, texture, texture_taps):
    """The two regions hold the same two grey values with the same mean: nearest-seed on colour is chance, on relu2_1 it is the object. Measured with the synthetic
    weights: IoU 0.974 (tap 2, no snap) against 0.12 (colour only); the bounds are the issue's"""
    img, T, obj = texture
    M, _ = sel.select(oracle, img, T, *weights, tap=2, snap_iters=0, feat=texture_taps[1])
    got = sel.iou(M >= 128, obj)
    colour = sel.iou(sel.colour_only(oracle, img, T) >= 128, obj)
    print("texture fixture: IoU tap 2 = %.4f, colour only = %.4f" % (got, colour))
    assert got >= 0.90
    assert colour < 0.5
