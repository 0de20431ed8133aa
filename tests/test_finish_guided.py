"""The guided finish (SPEC §6.10) without a GPU: the exports, the CLI's -upguide / -upsigma and their refusals, and what the rule itself promises, asserted on the numpy
reference the GPU tests compare against (tests/finish_guided_ref.py): equal sizes are the upsampling finish, the clamp case clamps, the tile bound of the kernel holds,
and on a slanted edge the guided stretch leaves less than half of the bilinear stretch's error."""
import os
import subprocess
import numpy as np
import pytest

import nct
import finish_guided_ref as gr
import synth
from finish_up_ref import oracle_finish_upsample
from fullres_ref import smooth_ab

BIN = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")


def test_library_exports_the_new_symbols_at_version_118():
    l = nct.lib()
    for name in ("nct_guided_params_default", "nct_color_finish_guided", "nct_color_finish_guided_dev", "nct_set_finish_guided"):
        assert name in nct.SIGNATURES and getattr(l, name) is not None
    assert l.nct_version() == nct.NCT_VERSION == 118
    assert nct.GuidedParams.default().sigma == 10.0 == gr.SIGMA
    assert (nct.FINISH_EXACT, nct.FINISH_UPSAMPLE) == (0, 1)                # the guided finish is a modifier, not a third finish


def test_help_shows_one_line_per_flag():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True)
    for flag, default in (("-upguide", "0"), ("-upsigma", "10")):
        lines = [l for l in r.stdout.splitlines() if l.startswith(flag + ": ")]
        assert len(lines) == 1 and lines[0].startswith("%s: (default=%s) [extension] " % (flag, default)), lines


@pytest.mark.parametrize("args,flag", [(("-fullres", "2", "-upguide", "2"), "-upguide"), (("-fullres", "2", "-upguide", "-1"), "-upguide"),
                                       (("-upguide", "1"), "-upguide 1"), (("-fullres", "1", "-upguide", "1"), "-upguide 1"),
                                       (("-seq", "1", "-seqfull", "1", "-upguide", "1"), "-upguide 1"), (("-seq", "1", "-upguide", "1"), "-upguide 1"),
                                       (("-fullres", "2", "-upguide", "1", "-upsigma", "0"), "-upsigma"), (("-fullres", "2", "-upguide", "1", "-upsigma", "-3"), "-upsigma"),
                                       (("-fullres", "2", "-upguide", "1", "-upsigma", "nan"), "-upsigma"), (("-fullres", "2", "-upguide", "1", "-upsigma", "inf"), "-upsigma"),
                                       (("-upsigma", "0"), "-upsigma")])
def test_cli_refuses_at_startup(tmp_path, args, flag):
    r = subprocess.run([BIN, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"), *args], capture_output=True, text=True)
    assert r.returncode != 0 and "Error:" in r.stdout and flag in r.stdout and "@@JOB" not in r.stdout, r.stdout
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("args", [("-fullres", "2", "-upguide", "1"), ("-seq", "1", "-seqfull", "2", "-upguide", "1", "-upsigma", "5"), ("-fullres", "2", "-upguide", "0")])
def test_cli_accepts_the_flags_where_they_apply(tmp_path, args):
    inp = tmp_path / "in"; inp.mkdir()
    (inp / "pairs.txt").write_text("a.png b.png 2.0\n")
    r = subprocess.run([BIN, "--plan-only", "-i", str(inp), "-o", str(tmp_path / "out"), *args], capture_output=True, text=True)
    assert r.returncode == 0 and "Error:" not in r.stdout and "@@JOB src=a.png" in r.stdout, r.stdout


@pytest.mark.parametrize("form", [0, 1])
def test_equal_sizes_are_the_upsampling_finish(oracle, form):
    h, w = 37, 29
    s = synth.image(77, h, w)
    ab = smooth_ab(78, h, w)
    exp, elab = oracle_finish_upsample(oracle, ab, h, w, s, form)
    got, lab = gr.finish_guided(oracle, ab, oracle.bgr2lab(s), h, w, s, form=form)
    assert np.array_equal(lab, elab) and np.array_equal(got, exp)


def test_flat_coefficients_stay_flat(oracle):
    """the weights are normalised: constant coefficient maps come back as that constant up to the rounding of 16 products, 16 sums twice and one division
    (at most some 50 roundings of 2^-53 relative each: below 1e-14 at 1.1 and below 1e-15 at 0.03)"""
    (h, w), (H, W) = (9, 7), (40, 23)
    s = synth.image(81, H, W)
    ab = np.empty((2, h * w, 3)); ab[0] = (1.1, 0.9, 1.0); ab[1] = (0.03, -0.02, 0.0)
    a, b = gr.guided_coeffs(ab, oracle.bgr2lab(oracle.resize_u8c3(s, h, w)), h, w, oracle.bgr2lab(s))
    assert np.abs(a - ab[0][0]).max() < 1e-14 and np.abs(b - ab[1][0]).max() < 1e-15


def test_clamp_case_clamps_on_both_sides(oracle):
    ab, lab_w, h, w, s = gr.clamp_inputs(oracle)
    _, lab = gr.finish_guided(oracle, ab, lab_w, h, w, s)
    print("clamp case: %.1f %% zeros, %.1f %% 255" % (100 * (lab == 0).mean(), 100 * (lab == 255).mean()))
    assert (lab == 0).mean() >= 0.01 and (lab == 255).mean() >= 0.01


def test_a_tile_of_32_x_8_pixels_needs_at_most_36_x_12_taps():
    """what k_finish_guided's LDS tile relies on: the source index does not decrease, and from the first pixel's s - 1 to the last pixel's s + 2 (clamped to the grid) a
    run of 32 destination pixels spans at most 36 source pixels, one of 8 at most 12 — also at ratios barely above 1 and at the largest sides"""
    worst = {32: 0, 8: 0}
    for n in list(range(1, 70)) + [1000, 4095, 8191, 12345, 16383]:
        for N in {n, n + 1, n + 2, 2 * n - 1, 2 * n, 3 * n + 1, min(16 * n, 16384), 16384}:
            if not n <= N <= 16384:
                continue
            s, f = gr.lin_coef(n, N)
            assert (np.diff(s) >= 0).all() and s.min() >= 0 and s.max() <= n - 1 and (f >= 0).all() and (f < 1).all()
            for T in (32, 8):
                d0 = np.arange(0, N, T)
                d1 = np.minimum(d0 + T, N) - 1
                worst[T] = max(worst[T], int((np.minimum(s[d1] + 2, n - 1) - np.maximum(s[d0] - 1, 0) + 1).max()))
    print("largest tap extent of a run of 32 / 8 pixels:", worst)
    assert worst[32] <= 36 and worst[8] <= 12


def test_guided_halves_the_error_at_a_slanted_edge(oracle):
    """two flat regions, +-3 noise, a slanted edge off the 12 x 10 working grid, ratio 4, coefficients constant per region and mixed by coverage on edge pixels: the mean
    absolute Lab error against the per-region ideal is less than half of the bilinear composition's at sigma = 10 (measured: 0.135 against 0.452 grey levels, ratio 0.30;
    maximum 6 against 17)"""
    ab, lab_w, h, w, s, ideal = gr.edge_scene(oracle)
    assert (h, w) == (12, 10) and s.shape == (48, 40, 3)
    la, lb = oracle.bgr2lab(np.array([gr.EDGE_BGR], np.uint8))[0].astype(int)
    assert np.abs(la - lb).sum() > 100                                      # the two colours are far apart in Lab
    cover = np.abs(ab.reshape(2, h, w, 3)[0, :, :, 0] - gr.EDGE_AB[0][0][0]) / abs(gr.EDGE_AB[1][0][0] - gr.EDGE_AB[0][0][0])
    assert ((cover > 0.05) & (cover < 0.95)).sum() >= h                     # every row has a mixed pixel: the edge is not aligned to the grid
    _, guided = gr.finish_guided(oracle, ab, lab_w, h, w, s, 10.0)
    _, bilinear = oracle_finish_upsample(oracle, ab, h, w, s)
    eg, eb = np.abs(guided.astype(int) - ideal.astype(int)), np.abs(bilinear.astype(int) - ideal.astype(int))
    print("edge: guided mean %.3f max %d, bilinear mean %.3f max %d, ratio %.3f" % (eg.mean(), eg.max(), eb.mean(), eb.max(), eg.mean() / eb.mean()))
    assert eg.mean() < 0.5 * eb.mean()
