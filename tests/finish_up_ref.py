"""The upsampling finish (SPEC §6.8) composed from the oracle's exported stages: bgr2lab, resize_f64c3 (U1's arithmetic), apply_coeffs (A1's), lab2bgr — no new
reference arithmetic. Shared by tests/test_finish_upsample.py / test_seq_fullres.py (CPU) and tests/test_gpu_finish_upsample.py / test_gpu_seq_fullres.py."""
import numpy as np

import fullres_ref


def oracle_finish_upsample(orc, ab_wls, h, w, s_bgr_full, form=None):
    """ab_wls ([2][h*w][3], the working-size finish's S2 output) upsampled to s_bgr_full's size and applied to its pixels -> (bgr, lab before Lab -> BGR)"""
    fullres_ref._declare(orc.l)
    s = np.ascontiguousarray(s_bgr_full, np.uint8)
    H, W = s.shape[:2]
    N = H * W
    lab = orc.bgr2lab(s)
    full = np.empty(N * 3)
    orc.l.orc_u8_to_f64_scaled(lab.reshape(-1), N * 3, full)
    ab = np.ascontiguousarray(ab_wls, np.float64).reshape(2, h * w, 3)
    if W > w or H > h:
        A = orc.resize_f64c3(ab[0].reshape(h, w, 3), H, W).reshape(N, 3)
        B = orc.resize_f64c3(ab[1].reshape(h, w, 3), H, W).reshape(N, 3)
    else:
        A, B = ab[0].copy(), ab[1].copy()                                # equal sizes: a copy
    olab = orc.apply_coeffs(np.stack([A, B]), full.reshape(N, 3)).reshape(H, W, 3)
    return orc.lab2bgr(olab, form), olab


# (working grid h x w) -> (target H x W): a copy, 2x, a non-integer ratio that differs per axis, ratio 16 (many output tiles per working pixel), a side above 4096,
# the smallest grid
SEAM_CASES = [((61, 47), (61, 47)), ((61, 47), (122, 94)), ((31, 24), (250, 171)), ((17, 17), (272, 272)), ((210, 16), (4200, 320)), ((1, 1), (3, 2))]


def seam_inputs(case):
    import synth
    (h, w), (H, W) = SEAM_CASES[case]
    return fullres_ref.smooth_ab(300 + case, h, w), synth.image(400 + case, H, W)


def clamp_inputs():
    """coefficients scaled so that A1's clamp works on both sides: a large gain around mid-grey pushes dark pixels below 0 and bright ones above 1"""
    import synth
    (h, w), (H, W) = (23, 19), (70, 95)
    ab = fullres_ref.smooth_ab(350, h, w).reshape(2, h * w, 3).copy()
    ab[0] *= 6.0
    ab[1] = ab[1] * 4.0 - 2.5
    return ab, h, w, synth.image(450, H, W)


# ---- the clip of the full-resolution sequence tests (SPEC §6.9): originals of 140 x 160 that work at 56 x 64, a reference that is shrunk as well
FRAME, REF, MAX_SIDE, WORK = (140, 160), (2000, 150, 180), 64, (56, 64)
AUTO = (24, 500, 100, 8)


def pan():
    import seq_ref
    return seq_ref.pan_frames(5, FRAME[0], FRAME[1], step=10)


def auto_clip():
    """four frames of the pan, then two of another scene: with AUTO the plan of the shrunk frames holds a propagated frame, a key frame and a cut"""
    import seq_ref
    return seq_ref.pan_frames(4, FRAME[0], FRAME[1], step=10) + seq_ref.pan_frames(2, FRAME[0], FRAME[1], step=10, seed=3000)
