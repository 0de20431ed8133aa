"""numpy reference of the 16-bit table apply (SPEC §6.20): the table of §6.6 at a 16-bit position, a value v standing for the grey level v / 257. Integer weights, one
IEEE binary64 operation per step in the SPEC's order (numpy never contracts), so the GPU result is compared with this bit for bit."""
import numpy as np

W3 = 65535 ** 3          # 281462092005375: the sum of a pixel's eight integer weights, below 2^48


def _axis(v, N):
    t = v.astype(np.int64) * (N - 1)
    i = np.minimum(t // 65535, N - 2)
    return i, t - 65535 * i


def apply(lut, N, bgr16):
    """out [npix, 3] uint16: the double sum over the eight corners (db outer, dr inner) of w * LUT, / 65535^3, * 257, clamped to [0, 65535] (a NaN becomes 0) and
    rounded to nearest even; lut [N^3, 3] float32 in 8-bit grey levels, bgr16 [npix, 3] uint16"""
    lut = np.ascontiguousarray(lut, np.float32).reshape(N ** 3, 3).astype(np.float64)
    px = np.ascontiguousarray(bgr16, np.uint16).reshape(-1, 3)
    (ib, fb), (ig, fg), (ir, fr) = _axis(px[:, 0], N), _axis(px[:, 1], N), _axis(px[:, 2], N)
    acc = np.zeros((len(px), 3))
    for db in (0, 1):
        for dg in (0, 1):
            for dr in (0, 1):
                w = (fb if db else 65535 - fb) * (fg if dg else 65535 - fg) * (fr if dr else 65535 - fr)
                acc = acc + w.astype(np.float64)[:, None] * lut[((ib + db) * N + ig + dg) * N + ir + dr]
    with np.errstate(invalid="ignore"):
        y = acc / float(W3) * 257.0
        y = np.where(y > 0.0, y, 0.0)
        y = np.where(y < 65535.0, y, 65535.0)
    return np.rint(y).astype(np.uint16)
