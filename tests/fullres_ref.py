"""The full-resolution finish (SPEC §6.1) composed from the oracle's exported stages, and the working-size rule restated in numpy.
Shared by tests/test_fullres.py (CPU) and tests/test_gpu_fullres.py."""
import ctypes as C
import numpy as np

_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")

MAX_SIDE, MAX_PIXELS = 16384, 1 << 26


def working_size(h, w, max_side):
    """rule 1 (host/cli_job.cpp's shrink) in float32 exactly as C evaluates `(int)(max_side / (float)long * short)`, plus the limits of rule 5; None = refused"""
    if not 17 <= max_side <= 4000 or h < 1 or w < 1 or h > MAX_SIDE or w > MAX_SIDE or h * w > MAX_PIXELS:
        return None
    ch, cw = h, w
    if w > max_side or h > max_side:
        cw = max_side
        ch = int(np.float32(np.float32(cw) / np.float32(w)) * np.float32(h))
        if w < h:
            ch = max_side
            cw = int(np.float32(np.float32(ch) / np.float32(h)) * np.float32(w))
    if ch < 17 or cw < 17:
        return None
    return ch, cw


def s2_levels(H, W):
    """number of levels of S2's multigrid hierarchy on an H x W grid (k_wls_mg.hip / orc_wls_mg.c: halve until n <= 64 or both sides <= 8)"""
    n, h, w = 1, H, W
    while not (h * w <= 64 or (h <= 8 and w <= 8)):
        h, w, n = (h + 1) // 2, (w + 1) // 2, n + 1
    return n


def _declare(l):
    l.orc_u8_to_f64_scaled.argtypes = [_u8p, C.c_size_t, _f64p]
    l.orc_u8_to_f64_scaled.restype = None
    l.orc_wls_solve_mg.argtypes = [_f64p, _f64p, _f64p, C.c_int, C.c_int, C.c_double, C.c_double, _f64p, C.c_double, np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")]
    l.orc_wls_solve_mg.restype = C.c_int


def oracle_finish(orc, ab, h, w, work_h, work_w, s_bgr_full, form=None, wls_lambda_init=0.024, wls_alpha=1.2):
    """U1 / roughness / S2 (canonical multigrid PCG to 3e-8) / A1 / Lab -> BGR of S1's coefficients ab ([2][h*w][3]) onto s_bgr_full, as SPEC §6.1 rule 3 states it.
    -> (bgr, {"ab_up", "roughness", "ab_wls", "wls_iters", "lab": the result before Lab -> BGR})"""
    _declare(orc.l)
    s = np.ascontiguousarray(s_bgr_full, np.uint8)
    H, W = s.shape[:2]
    N = H * W
    lab = orc.bgr2lab(s)
    full = np.empty(N * 3)
    orc.l.orc_u8_to_f64_scaled(lab.reshape(-1), N * 3, full)
    ab = np.ascontiguousarray(ab, np.float64).reshape(2, h * w, 3)
    if W > w or H > h:
        A = orc.resize_f64c3(ab[0].reshape(h, w, 3), H, W).reshape(-1)
        B = orc.resize_f64c3(ab[1].reshape(h, w, 3), H, W).reshape(-1)
    else:
        A, B = ab[0].reshape(-1).copy(), ab[1].reshape(-1).copy()
    ab_up = np.stack([A.reshape(N, 3), B.reshape(N, 3)]).copy()
    rough = orc.roughness(ab_up, full.reshape(N, 3))
    r = float(H * W) / float(h * w)
    lamda = wls_lambda_init * r
    if h == work_h and w == work_w:
        lamda *= 4
    wit = np.zeros(6, np.int32)
    rc = orc.l.orc_wls_solve_mg(A, B, full, H, W, lamda, wls_alpha, rough, 3e-8, wit)
    assert rc >= 0, rc
    ab_wls = np.stack([A.reshape(N, 3), B.reshape(N, 3)])
    olab = orc.apply_coeffs(ab_wls, full.reshape(N, 3))
    bgr = orc.lab2bgr(olab.reshape(H, W, 3), form)
    return bgr, {"ab_up": ab_up, "roughness": rough, "ab_wls": ab_wls, "wls_iters": wit, "lab": olab.reshape(H, W, 3)}


def smooth_ab(seed, h, w):
    """smooth random S1 coefficients [2][h*w][3]: a around 1, b around 0, low-frequency cosines (the scale of what S1 returns on natural pairs)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((2, h, w, 3))
    for p in range(2):
        for c in range(3):
            acc = np.zeros((h, w))
            for _ in range(3):
                th, ph, wl = rng.random() * 2 * np.pi, rng.random() * 2 * np.pi, 8 + rng.random() * 40
                acc += np.cos(2 * np.pi * (xx * np.cos(th) + yy * np.sin(th)) / wl + ph)
            out[p, :, :, c] = (1.0 + 0.15 * acc / 3) if p == 0 else 0.08 * acc / 3
    return out.reshape(2, h * w, 3)
