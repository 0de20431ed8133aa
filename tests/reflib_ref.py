"""Reference libraries (SPEC §6.21) in numpy: the int8 descriptor (D2), the match (D3), the key and the order (D4), a library built and ranked from taps the caller
holds, and the one-texture fixture the rule is tried on."""
import numpy as np

TAP_C = (64, 128, 256, 512, 512)
I32 = 2 ** 31


def grid(h, w, tap):
    return ((h - 1) >> (tap - 1)) + 1, ((w - 1) >> (tap - 1)) + 1


def quantize8(orc, feat_chw, center=None):
    """D2: CHW fp32, center [C] or None -> [H*W][C] int8, rint(N1(F - center) * 127) with the difference and the product in fp32; a non-finite u gives 0"""
    f = np.ascontiguousarray(feat_chw, np.float32)
    C = f.shape[0]
    if center is not None:
        f = np.ascontiguousarray(f - np.asarray(center, np.float32).reshape(C, 1, 1))
        assert f.dtype == np.float32
    with np.errstate(all="ignore"):
        u = orc.feat_normalize(f)
        t = u * np.float32(127)
        assert t.dtype == np.float32
        q = np.where(np.isfinite(u), np.rint(t), np.float32(0)).astype(np.int8)
    return np.ascontiguousarray(q.reshape(C, -1).T)


def products(a, b):
    """P = A B^T with int64 products; every entry and every partial sum of one stays inside int32 (D2)"""
    A, B = np.asarray(a, np.int8).astype(np.int64), np.asarray(b, np.int8).astype(np.int64)
    return A @ B.T


def partial_sum_bound(a, b):
    """the largest magnitude any partial sum of any product row can reach, whatever the order of summation: sum_c |a_c b_c|"""
    return int((np.abs(np.asarray(a, np.int8).astype(np.int64)) @ np.abs(np.asarray(b, np.int8).astype(np.int64)).T).max())


def match(a, b):
    """D3 -> (fwd, bwd) as Python ints"""
    P = products(a, b)
    return int(P.max(axis=1).sum()), int(P.max(axis=0).sum())


def key(fwd, bwd, na, nb, wf=1, wb=1):
    """D4, Python's // being floor division"""
    assert 0 <= wf <= 16 and 0 <= wb <= 16 and wf + wb > 0
    return wf * ((fwd * 1024) // na) + wb * ((bwd * 1024) // nb)


def order(keys):
    """descending key, the lower index first on a tie"""
    return np.array(sorted(range(len(keys)), key=lambda i: (-keys[i], i)), np.int32)


def rank(a, entries, wf=1, wb=1):
    """a [na][C] against a list of entries [n_k][C] -> (order, keys, fwd, bwd)"""
    fb = [match(a, e) for e in entries]
    keys = [key(f, b, len(a), len(e), wf, wb) for (f, b), e in zip(fb, entries)]
    return order(keys), np.array(keys, np.int64), np.array([f for f, _ in fb], np.int64), np.array([b for _, b in fb], np.int64)


def library_center(taps):
    """the console driver's centre: the channel means over every cell of every entry's tap, accumulated in double image after image in raster order, as fp32"""
    C = taps[0].shape[0]
    acc, n = np.zeros(C, np.float64), 0
    for F in taps:
        rows = np.asarray(F, np.float32).reshape(C, -1).T.astype(np.float64)
        acc = np.cumsum(np.vstack([acc[None, :], rows]), axis=0)[-1]      # one cell after the other (a running sum): the order is part of the rule
        n += rows.shape[0]
    return (acc / n).astype(np.float32)


# ---------------------------------------------------------------- the fixture: one texture per image, equal grey values and mean
FIX_H, FIX_W = 96, 112
TEXTURES = ("diagonal", "checker", "hbars", "vbars", "dots")
TINTS = ((10, 0, -10), (-10, 10, 0), (0, -10, 10), (8, 8, -8), (-8, 0, 8))      # BGR offsets of the library's five entries


def texture(name, phase=0):
    """170 / 90 pattern of the named texture, shifted by `phase` pixels"""
    yy, xx = np.mgrid[0:FIX_H, 0:FIX_W]
    yy, xx = yy + phase, xx + 2 * phase
    on = {"diagonal": ((xx + yy) // 3) % 2 == 0,
          "checker": ((xx // 4) + (yy // 4)) % 2 == 0,
          "hbars": (yy // 3) % 2 == 0,
          "vbars": (xx // 3) % 2 == 0,
          "dots": ((xx % 6) < 3) & ((yy % 6) < 3)}[name]
    return np.where(on, 170, 90)


def texture_image(name, seed, phase=0, tint=(0, 0, 0)):
    g = texture(name, phase)
    img = np.repeat(g[:, :, None], 3, axis=2) + np.asarray(tint).reshape(1, 1, 3) + np.random.default_rng(seed).integers(-6, 7, (FIX_H, FIX_W, 3))
    return np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8))


def fixture_library():
    return [texture_image(n, 100 + i, 0, TINTS[i]) for i, n in enumerate(TEXTURES)]


def fixture_sources():
    """a texture of the library each, new noise, shifted phase, untinted"""
    return [texture_image(n, 200 + i, 1 + i % 3) for i, n in enumerate(TEXTURES)]
