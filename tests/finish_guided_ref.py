"""The guided finish (SPEC §6.10) in numpy float64: the 4 x 4 joint-bilateral taps accumulated in the rule's order with vectorised IEEE operations. From the oracle
only bgr2lab, apply_coeffs (A1) and lab2bgr, as tests/finish_up_ref.py takes them; lin_coef (cv::resize's INTER_LINEAR index and fraction) is restated here with its
float32 steps. Shared by tests/test_finish_guided.py (CPU) and tests/test_gpu_finish_guided.py."""
import numpy as np

import fullres_ref
from finish_up_ref import oracle_finish_upsample

SIGMA = 10.0                     # nct_guided_params_default


def lin_coef(ssize, dsize):
    """per destination index 0 .. dsize - 1: the source index (int64) and the fraction a1 (float32) of nct_pixel.h's lin_coef, clamping included"""
    d = np.arange(dsize, dtype=np.float64)
    scale = np.float64(ssize) / np.float64(dsize)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    f[s < 0] = 0; s[s < 0] = 0
    f[s >= ssize - 1] = 0; s[s >= ssize - 1] = ssize - 1
    return s, f


def tent(f, j):
    """the spatial weight of tap offset j: 1.0 - fabs(f - (double)j) * 0.5 in double"""
    return 1.0 - np.abs(f.astype(np.float64) - np.float64(j)) * 0.5


def guided_coeffs(ab_wls, lab_w, h, w, lab_full, sigma=SIGMA):
    """rules 2-7: ab_wls [2][h*w][3], lab_w [h][w][3] u8 (the guide), lab_full [H][W][3] u8 (the original pixels' Lab) -> (a, b) [H*W][3] each"""
    ab = np.ascontiguousarray(ab_wls, np.float64).reshape(2, h, w, 3)
    lw = np.ascontiguousarray(lab_w, np.uint8).reshape(h, w, 3).astype(np.int64)
    L = np.ascontiguousarray(lab_full, np.uint8).astype(np.int64)
    H, W = L.shape[:2]
    sy, fy = lin_coef(h, H)
    sx, fx = lin_coef(w, W)
    s2 = np.float64(sigma) * np.float64(sigma)
    den = np.zeros((H, W))
    na, nb = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    with np.errstate(invalid="ignore"):                                  # a NaN coefficient behind a skipped tap is computed and thrown away by np.where
        for j in (-1, 0, 1, 2):
            ty, v = sy + j, tent(fy, j)
            oky = (ty >= 0) & (ty < h) & (v != 0.0)
            tyc = np.clip(ty, 0, h - 1)
            for k in (-1, 0, 1, 2):
                tx, u = sx + k, tent(fx, k)
                okx = (tx >= 0) & (tx < w) & (u != 0.0)
                txc = np.clip(tx, 0, w - 1)
                ok = oky[:, None] & okx[None, :]
                tap = lw[tyc[:, None], txc[None, :]]
                d2 = ((L - tap) ** 2).sum(axis=2)
                g = (v[:, None] * u[None, :]) / (1.0 + d2.astype(np.float64) / s2)
                den = np.where(ok, den + g, den)
                na = np.where(ok[..., None], na + g[..., None] * ab[0][tyc[:, None], txc[None, :]], na)
                nb = np.where(ok[..., None], nb + g[..., None] * ab[1][tyc[:, None], txc[None, :]], nb)
        return (na / den[..., None]).reshape(H * W, 3), (nb / den[..., None]).reshape(H * W, 3)


def finish_guided(orc, ab_wls, lab_w, h, w, s_bgr_full, sigma=SIGMA, form=None):
    """SPEC §6.10 -> (bgr, lab before Lab -> BGR). Equal sizes: the upsampling finish's copy path"""
    s = np.ascontiguousarray(s_bgr_full, np.uint8)
    H, W = s.shape[:2]
    if H == h and W == w:
        return oracle_finish_upsample(orc, ab_wls, h, w, s, form)
    fullres_ref._declare(orc.l)
    N = H * W
    lab = orc.bgr2lab(s)
    full = np.empty(N * 3)
    orc.l.orc_u8_to_f64_scaled(lab.reshape(-1), N * 3, full)
    A, B = guided_coeffs(ab_wls, lab_w, h, w, lab, sigma)
    olab = orc.apply_coeffs(np.stack([A, B]), full.reshape(N, 3)).reshape(H, W, 3)
    return orc.lab2bgr(olab, form), olab


# (working grid h x w) -> (target H x W): a copy, a ratio just above 1 (the largest LDS tile extent), 2x, a non-integer ratio that differs per axis, ratio 16, a side
# above 4096, taps -1 and +2 outside on both sides, the smallest grid
SEAM_CASES = [((61, 47), (61, 47)), ((61, 47), (62, 48)), ((61, 47), (122, 94)), ((31, 24), (250, 171)), ((17, 17), (272, 272)), ((210, 16), (4200, 320)),
              ((2, 3), (5, 7)), ((1, 1), (3, 2))]
NONINT = 3                       # the case that also runs with sigma = 1 and sigma = 1000


def seam_inputs(orc, case):
    """smooth coefficients, a synthetic source at the target size and the guide: bgr2lab of the source shrunk to the working grid"""
    import synth
    (h, w), (H, W) = SEAM_CASES[case]
    s_full = synth.image(600 + case, H, W)
    return fullres_ref.smooth_ab(500 + case, h, w), orc.bgr2lab(orc.resize_u8c3(s_full, h, w)), s_full


def clamp_inputs(orc):
    """finish_up_ref.clamp_inputs() with its guide"""
    import finish_up_ref
    ab, h, w, s_full = finish_up_ref.clamp_inputs()
    return ab, orc.bgr2lab(orc.resize_u8c3(s_full, h, w)), h, w, s_full


# ---- the edge construction: two flat regions split by a slanted edge that is not aligned to the working grid; coefficients constant per region
EDGE_GRID, EDGE_RATIO = (12, 10), 4
EDGE_BGR = ((40, 60, 200), (200, 170, 50))                               # far apart in Lab
EDGE_AB = ((np.array([0.9, 1.1, 0.8]), np.array([0.05, -0.04, 0.10])), (np.array([1.2, 0.7, 1.05]), np.array([-0.10, 0.12, -0.03])))


def edge_scene(orc, seed=7):
    """-> (ab_wls mixed by coverage on edge pixels, lab_w, h, w, s_full, ideal): ideal = the Lab bytes A1 gives with every original pixel's own region's coefficients"""
    (h, w), r = EDGE_GRID, EDGE_RATIO
    H, W = h * r, w * r
    yy, xx = np.mgrid[0:H, 0:W]
    side = ((xx + 0.5) - (0.37 * (yy + 0.5) + 0.31 * W + 1.3) > 0)       # slanted, off the grid
    rng = np.random.default_rng(seed)
    flat = np.where(side[..., None], np.array(EDGE_BGR[1]), np.array(EDGE_BGR[0]))
    s_full = np.clip(flat + rng.integers(-3, 4, (H, W, 3)), 0, 255).astype(np.uint8)
    cover = side.reshape(h, r, w, r).mean(axis=(1, 3))                    # share of region 1 in every working pixel
    ab = np.empty((2, h, w, 3))
    for p in range(2):
        ab[p] = (1.0 - cover)[..., None] * EDGE_AB[0][p] + cover[..., None] * EDGE_AB[1][p]
    lab_w = orc.bgr2lab(orc.resize_u8c3(s_full, h, w))
    fullres_ref._declare(orc.l)
    lab = orc.bgr2lab(s_full)
    full = np.empty(H * W * 3)
    orc.l.orc_u8_to_f64_scaled(lab.reshape(-1), H * W * 3, full)
    A = np.where(side[..., None], EDGE_AB[1][0], EDGE_AB[0][0]).reshape(H * W, 3)
    B = np.where(side[..., None], EDGE_AB[1][1], EDGE_AB[0][1]).reshape(H * W, 3)
    ideal = orc.apply_coeffs(np.stack([A, B]).astype(np.float64), full.reshape(H * W, 3)).reshape(H, W, 3)
    return ab.reshape(2, h * w, 3), lab_w, h, w, s_full, ideal
