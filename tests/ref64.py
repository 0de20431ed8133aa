"""float64 restatements of the reference's colour stage, votes and PatchMatch distances — an independent check of oracle/ and of the kernels.

Every function is written from the reference sources (code/windows/neural_color_transfer/source/: main.cu, Classifier.cpp, GeneralizedPatchMatch.cu,
ColorTransfer/ColorTransfer.cpp, ColorTransfer/SparseSolver_GPU.cu; line numbers in each docstring) and from OpenCV's documented cv::resize mapping — never from oracle/ or csrc/, and this module
imports neither. It computes in float64 throughout, except where the reference itself computes in float32; there np.float32 emulates it.

Conventions: an NNF entry packs a match as (y << 12) | x (GeneralizedPatchMatch.cu:24-34). Feature maps are CHW, images and Lab maps HWC. Colour coefficients are
(n, 3) arrays per part (a, b), the first index of a stage array [2][n][3] being the part.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

VGG_MEAN_BGR = (103.939, 116.779, 123.68)          # Classifier.cpp:40


def _xy(nnf):
    v = np.asarray(nnf, np.uint32).astype(np.int64)
    return v & 0xFFF, (v >> 12) & 0xFFF


def _pack(x, y):
    return ((np.asarray(y, np.int64) << 12) | np.asarray(x, np.int64)).astype(np.uint32)


# ---------------------------------------------------------------- V1, geometry
def vgg19_taps(bgr, ws, bs, deepest=5):
    """Classifier::Predict's VGG19 up to relu{deepest}_1, in float64 with torch.nn.functional on the CPU. Preprocess (Classifier.cpp:211-265): the u8 BGR image
    converted to float and the per-channel mean subtracted by cv::subtract on a CV_32F map (the Scalar is taken to float, the difference rounded to float), no
    scaling. Then conv1_1 .. conv5_1: every convolution 3x3, pad 1, followed by ReLU; a 2x2 stride-2 max pool after conv1_2, conv2_2, conv3_4 and conv4_4 in
    Caffe's ceil mode (pooling_layer.cpp:90-93). ws[i]: [Cout][Cin][3][3], bs[i]: [Cout], i = 0 .. 12. Returns the taps relu1_1 .. relu{deepest}_1, CHW."""
    import torch
    import torch.nn.functional as F
    img = np.asarray(bgr, np.uint8)
    x = img.astype(np.float32) - np.asarray(VGG_MEAN_BGR, np.float32)
    x = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1), np.float64))[None]
    pool_after = {1, 3, 7, 11}
    tap_at = {0: 0, 2: 1, 4: 2, 8: 3, 12: 4}
    taps = []
    for i in range(13):
        x = F.relu(F.conv2d(x, torch.from_numpy(np.asarray(ws[i], np.float64)), torch.from_numpy(np.asarray(bs[i], np.float64)), padding=1))
        if i in tap_at:
            taps.append(x[0].numpy().copy())
            if len(taps) == deepest:
                break
        if i in pool_after:
            x = F.max_pool2d(x, 2, 2, ceil_mode=True)
    return taps


def conv3x3(x, w, b, relu=True):
    """One Caffe convolution layer, 3x3, pad 1, stride 1 (conv_layer.cpp: out = sum_ci sum_taps w * in + bias), optionally followed by ReLU, in float64 with
    torch.nn.functional on the CPU. x: [Cin][H][W], w: [Cout][Cin][3][3], b: [Cout]. Returns (y, M): the map and the magnitude map M = conv(|x|, |w|) + |b|, the sum of
    the absolute values of everything that is added up for an output element — what a rounding-error bound of that sum is proportional to (ReLU moves no bound:
    |max(a, 0) - max(b, 0)| <= |a - b|)."""
    import torch
    import torch.nn.functional as F
    xt, wt, bt = (torch.from_numpy(np.array(a, np.float64)) for a in (x, w, b))          # copies: the caller's arrays may be read-only
    xt = xt[None]
    y = F.conv2d(xt, wt, bt, padding=1)
    if relu:
        y = F.relu(y)
    m = F.conv2d(xt.abs(), wt.abs(), bt.abs(), padding=1)
    return y[0].numpy().copy(), m[0].numpy().copy()


def maxpool2x2_ceil(x):
    """Caffe's MAX pooling, kernel 2, stride 2, pad 0 (pooling_layer.cpp:90-93 ceil mode, :153-170 windows clipped to the map), float64. x: [C][H][W]."""
    import torch
    import torch.nn.functional as F
    return F.max_pool2d(torch.from_numpy(np.array(x, np.float64))[None], 2, 2, ceil_mode=True)[0].numpy().copy()


def pool_out(n):
    """pooling_layer.cpp:90-93 for kernel 2, stride 2, pad 0: ceil((n - 2) / 2) + 1"""
    return int(np.ceil((n - 2) / 2.0)) + 1


def level_geometry(H, W, RH, RW, nlayer=5):
    """transfer_color_single_bds's per-level constants (main.cu:47-454), level 0 = conv5_1 (coarsest) .. 4 = conv1_1. Sizes: the feature maps' (data_C_size /
    data_S_size, main.cu:94,102), the input halved by ceil pooling once per tap below; ah, aw for S (content, A), bh, bw for R (style, B). C: the tap's channels.
    rs_range: PatchMatch's random-search radius (main.cu:77-83, maxLen over both images). knn_samples = 2^l (findKnns, main.cu:351-359); color_samples =
    2^(numlayer - 1 - l) (main.cu:360-380)."""
    maxLen = max(W, H, RW, RH)
    rng = [maxLen // 16, maxLen // 32, maxLen // 64, 32, 32]
    chans = [512, 512, 256, 128, 64]
    out = []
    for l in range(nlayer):
        dims = []
        for n in (H, W, RH, RW):
            for _ in range(nlayer - 1 - l):
                n = pool_out(n)
            dims.append(n)
        out.append(dict(ah=dims[0], aw=dims[1], bh=dims[2], bw=dims[3], C=chans[l], tap=nlayer - l, rs_range=rng[l],
                        knn_samples=2 ** l, color_samples=2 ** (nlayer - 1 - l)))
    return out


# ---------------------------------------------------------------- N0, N1
def normalize(feat):
    """norm, GeneralizedPatchMatch.cu:237-283: every pixel's channel vector divided by its L2 norm (gemv of the squares, powx 0.5, div). No epsilon: a zero
    vector gives 0 / 0 = NaN, as in the reference. feat: [C][h][w]; float64."""
    f = np.asarray(feat, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return f / np.sqrt((f * f).sum(0))[None]


def response(feat):
    """The `smooth` output of norm, GeneralizedPatchMatch.cu:257-272: dis, the pixels' L2 norms (:255), shifted by -min (add_scalar, :270) and scaled by
    1 / (max - min) (scal, :271), in that order. A map whose norms are all equal (one pixel among them) gives 0 * (1 / 0) = NaN at every pixel, as that text
    does; a dead pixel (min = 0) gives 0 there. feat: [C][h][w]; float64 [h][w]."""
    f = np.asarray(feat, np.float64)
    dis = np.sqrt((f * f).sum(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (dis - dis.min()) * (np.float64(1.0) / (dis.max() - dis.min()))


def nnf_init(ah, aw, bh, bw):
    """init_Ann_kernel, GeneralizedPatchMatch.cu:527-545: bx = min(int(float(ax) / float(aw - 1) * (bw - 1)), bw - 1), by likewise; float arithmetic (the int
    bw - 1 is converted to float for the product), int() truncates. Needs aw, ah >= 2."""
    ax = np.arange(aw, dtype=np.float32)
    ay = np.arange(ah, dtype=np.float32)
    bx = np.minimum((ax / np.float32(aw - 1) * np.float32(bw - 1)).astype(np.int64), bw - 1)
    by = np.minimum((ay / np.float32(ah - 1) * np.float32(bh - 1)).astype(np.int64), bh - 1)
    return _pack(np.broadcast_to(bx[None, :], (ah, aw)), np.broadcast_to(by[:, None], (ah, aw)))


# ---------------------------------------------------------------- N2
def nnf_upsample(half, ah, aw, bh, bw):
    """upSample_kernel, GeneralizedPatchMatch.cu:546-580, over the whole map. The ratios are float; `(ax + 0.5) / ratio` is a double division (0.5 is a double
    literal); `ax + (bx_half - ax_half) * ratio` is float arithmetic to which the double 0.5 is added; int() truncates; clamp(x, max, min) (:9-21)."""
    half = np.asarray(half, np.uint32)
    hh, hw = half.shape
    rw = np.float32(aw) / np.float32(hw)
    rh = np.float32(ah) / np.float32(hh)
    ax = np.arange(aw)[None, :].repeat(ah, 0)
    ay = np.arange(ah)[:, None].repeat(aw, 1)
    axh = np.clip(np.trunc((ax + 0.5) / np.float64(rw)).astype(np.int64), 0, hw - 1)
    ayh = np.clip(np.trunc((ay + 0.5) / np.float64(rh)).astype(np.int64), 0, hh - 1)
    bxh, byh = _xy(half[ayh, axh])
    fx = ax.astype(np.float32) + (bxh - axh).astype(np.float32) * rw          # float * float, float + float: each rounded to float
    fy = ay.astype(np.float32) + (byh - ayh).astype(np.float32) * rh
    bx = np.clip(np.trunc(fx.astype(np.float64) + 0.5).astype(np.int64), 0, bw - 1)
    by = np.clip(np.trunc(fy.astype(np.float64) + 0.5).astype(np.int64), 0, bh - 1)
    return _pack(bx, by)


# ---------------------------------------------------------------- P1
def patch_distance(a, b, nnf, patch=3):
    """dist_compute_single, GeneralizedPatchMatch.cu:355-405, at every pixel of A for the match nnf gives it: minus the sum over the patch taps that lie inside
    BOTH maps of the channel dot product, divided by the number of such taps (1 when there is none; weight 1, pixel_sum 0). a: [C][ah][aw], b: [C][bh][bw]."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    C, ah, aw = a.shape
    _, bh, bw = b.shape
    bx, by = _xy(nnf)
    ax = np.arange(aw)[None, :]
    ay = np.arange(ah)[:, None]
    acc = np.zeros((ah, aw))
    cnt = np.zeros((ah, aw))
    r = patch // 2
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ok = (ay + dy >= 0) & (ay + dy < ah) & (ax + dx >= 0) & (ax + dx < aw) & (by + dy >= 0) & (by + dy < bh) & (bx + dx >= 0) & (bx + dx < bw)
            yA, xA = np.clip(ay + dy, 0, ah - 1) + 0 * ax, np.clip(ax + dx, 0, aw - 1) + 0 * ay
            yB, xB = np.clip(by + dy, 0, bh - 1), np.clip(bx + dx, 0, bw - 1)
            dot = np.zeros((ah, aw))
            for c0 in range(0, C, 64):
                dot += np.einsum("chw,chw->hw", a[c0:c0 + 64, yA, xA].astype(np.float64), b[c0:c0 + 64, yB, xB].astype(np.float64))
            acc -= np.where(ok, dot, 0.0)
            cnt += ok
    return np.where(cnt > 0, acc / np.maximum(cnt, 1), 1.0)


def feature_distance(a, b):
    """feature_distance, GeneralizedPatchMatch.cu:833-855: minus the per-pixel channel dot product of two maps of the same size."""
    return -np.einsum("chw,chw->hw", np.asarray(a, np.float64), np.asarray(b, np.float64))


# ---------------------------------------------------------------- B2
def vote_features(ann, bnn, pin, w_coh, w_comp, patch=3):
    """avg_vote_bds_a (:1074-1126), avg_vote_bds_b (:1128-1178) and avg_vote_bds (:1180-1202) of GeneralizedPatchMatch.cu in float64. pin: B's features
    [C][bh][bw]. Coherence: A pixel (ax, ay) gathers, for each tap (dx, dy) inside A, B at ann[ay+dy][ax+dx] - (dx, dy) when that lies inside B, weight
    w_coh / |A|. Completeness: every B pixel scatters, for each tap inside B whose partner bnn[b] + (dx, dy) lies inside A, B's tap value to that A pixel with
    weight w_comp / |B|. Returns (pout [C][ah][aw], pw [ah][aw]); pout is divided by pw where pw > 0."""
    pin = np.asarray(pin, np.float64)
    C, bh, bw = pin.shape
    ann = np.asarray(ann, np.uint32)
    bnn = np.asarray(bnn, np.uint32)
    ah, aw = ann.shape
    wa = w_coh / float(aw * ah)
    wb = w_comp / float(bw * bh)
    out = np.zeros((C, ah * aw))
    pw = np.zeros(ah * aw)
    r = patch // 2
    axg = np.arange(aw)[None, :] + 0 * np.arange(ah)[:, None]
    ayg = np.arange(ah)[:, None] + 0 * np.arange(aw)[None, :]
    pin_flat = pin.reshape(C, -1)
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            inA = (axg + dx >= 0) & (axg + dx < aw) & (ayg + dy >= 0) & (ayg + dy < ah)
            xp, yp = _xy(ann[np.clip(ayg + dy, 0, ah - 1), np.clip(axg + dx, 0, aw - 1)])
            xp, yp = xp - dx, yp - dy
            ok = (inA & (xp >= 0) & (xp < bw) & (yp >= 0) & (yp < bh)).reshape(-1)
            src = (np.clip(yp, 0, bh - 1) * bw + np.clip(xp, 0, bw - 1)).reshape(-1)
            pw += ok * wa
            out += pin_flat[:, src] * (ok * wa)
    bxg = np.arange(bw)[None, :] + 0 * np.arange(bh)[:, None]
    byg = np.arange(bh)[:, None] + 0 * np.arange(bw)[None, :]
    xq, yq = _xy(bnn)
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            xb, yb, xa, ya = bxg + dx, byg + dy, xq + dx, yq + dy
            ok = ((xb >= 0) & (xb < bw) & (yb >= 0) & (yb < bh) & (xa >= 0) & (xa < aw) & (ya >= 0) & (ya < ah)).reshape(-1)
            aid = (ya * aw + xa).reshape(-1)[ok]
            bid = (yb * bw + xb).reshape(-1)[ok]
            scatter = sp.csr_matrix((np.full(aid.size, wb), (aid, bid)), shape=(ah * aw, bh * bw))
            pw += np.asarray(scatter.sum(1)).ravel()
            out += (scatter @ pin_flat.T).T
    pos = pw > 0
    out[:, pos] /= pw[pos]
    return out.reshape(C, ah, aw), pw.reshape(ah, aw)


# ---------------------------------------------------------------- B1
def vote_image(a, b, ann, bnn, w_coh, w_comp, patch=3, want_float=False):
    """reconstruct_bds, GeneralizedPatchMatch.cu:122-235, on u8 BGR images a [ah][aw][3] (only its size is used) and b [bh][bw][3]. Integer colour sums and tap
    counts per A pixel from both directions, then (sa * wa + sb * wb) / (na * wa + nb * wb) in double with wa = w_coh / |A|, wb = w_comp / |B|, stored into a
    uchar: truncation toward zero. want_float: also return that double value."""
    ah, aw = np.asarray(a).shape[:2]
    b = np.asarray(b, np.uint8)
    bh, bw = b.shape[:2]
    ann = np.asarray(ann, np.uint32)
    bnn = np.asarray(bnn, np.uint32)
    bflat = b.reshape(-1, 3).astype(np.int64)
    r = patch // 2
    left = -(patch // 2)                                          # leftSize = -patch_w / 2, rightSize = patch_w + leftSize - 1
    right = patch + left - 1
    ares = np.zeros((ah * aw, 3), np.int64)
    acnt = np.zeros(ah * aw, np.int64)
    axg = np.arange(aw)[None, :] + 0 * np.arange(ah)[:, None]
    ayg = np.arange(ah)[:, None] + 0 * np.arange(aw)[None, :]
    for dx in range(left, right + 1):
        for dy in range(left, right + 1):
            inA = (axg + dx < aw) & (axg + dx >= 0) & (ayg + dy < ah) & (ayg + dy >= 0)
            xp, yp = _xy(ann[np.clip(ayg + dy, 0, ah - 1), np.clip(axg + dx, 0, aw - 1)])
            ok = (inA & (xp - dx < bw) & (xp - dx >= 0) & (yp - dy < bh) & (yp - dy >= 0)).reshape(-1)
            src = (np.clip(yp - dy, 0, bh - 1) * bw + np.clip(xp - dx, 0, bw - 1)).reshape(-1)
            ares += bflat[src] * ok[:, None]
            acnt += ok
    bres = np.zeros((ah * aw, 3), np.int64)
    bcnt = np.zeros(ah * aw, np.int64)
    bxg = np.arange(bw)[None, :] + 0 * np.arange(bh)[:, None]
    byg = np.arange(bh)[:, None] + 0 * np.arange(bw)[None, :]
    xq, yq = _xy(bnn)
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            xb, yb, xa, ya = bxg + dx, byg + dy, xq + dx, yq + dy
            ok = ((xb < bw) & (xb >= 0) & (yb < bh) & (yb >= 0) & (xa < aw) & (xa >= 0) & (ya < ah) & (ya >= 0)).reshape(-1)
            aid = (ya * aw + xa).reshape(-1)[ok]
            bid = (yb * bw + xb).reshape(-1)[ok]
            np.add.at(bres, aid, bflat[bid])
            np.add.at(bcnt, aid, 1)
    wa = w_coh / float(aw * ah)
    wb = w_comp / float(bw * bh)
    v = (ares * wa + bres * wb) / (acnt * wa + bcnt * wb)[:, None]
    out = np.trunc(v).astype(np.uint8).reshape(ah, aw, 3)
    return (out, v.reshape(ah, aw, 3)) if want_float else out


# ---------------------------------------------------------------- T1
def local_stats(cnt_lab, stl_lab, eps, patch=3):
    """transfer_color_downsample's closed form, ColorTransfer.cpp:1195-1250, with the prefix tables of build_accumTable_downsample (:425-455) and getValue
    (:46-58) taken literally: 1-D int64 running sums over the row-major raster (table[0] = 0), and per window row y the difference table[y*w + ex] -
    table[y*w + sx]. Window [x - 1, x + 2) x [y - 1, y + 2) clipped to the map. cnt_lab, stl_lab: level-size Lab u8 [h][w][3]. Returns (a, b) [h*w][3]:
    a = sigma_stl / (sigma_cnt + eps), b = (mean_stl - mean_cnt * a) / 255."""
    cnt = np.asarray(cnt_lab, np.uint8)
    stl = np.asarray(stl_lab, np.uint8)
    h, w = cnt.shape[:2]

    def tables(img):
        v = img.reshape(-1, 3).astype(np.int64)
        t = np.zeros((h * w + 1, 3), np.int64)
        t2 = np.zeros((h * w + 1, 3), np.int64)
        t[1:] = np.cumsum(v, 0)
        t2[1:] = np.cumsum(v * v, 0)
        return t, t2

    left = -(patch // 2)
    right = patch + left
    x = np.arange(w)[None, :] + 0 * np.arange(h)[:, None]
    y = np.arange(h)[:, None] + 0 * np.arange(w)[None, :]
    sx, sy = np.maximum(x + left, 0), np.maximum(y + left, 0)
    ex, ey = np.minimum(x + right, w), np.minimum(y + right, h)
    csum = ((ex - sx) * (ey - sy)).reshape(-1, 1).astype(np.float64)

    def window(t):
        val = np.zeros((h, w, 3), np.int64)
        for k in range(patch):
            row = sy + k
            on = (row < ey)[..., None]
            rr = np.minimum(row, h - 1)
            val += np.where(on, t[rr * w + ex] - t[rr * w + sx], 0)
        return val.reshape(-1, 3)

    ct, ct2 = tables(cnt)
    st, st2 = tables(stl)
    cm = window(ct) / csum
    cv = np.sqrt(np.maximum(window(ct2) / csum - cm * cm, 0.0))
    sm = window(st) / csum
    sv = np.sqrt(np.maximum(window(st2) / csum - sm * sm, 0.0))
    a = sv / (cv + eps)
    b = (sm - cm * a) * (1.0 / 255.0)
    return a, b


# ---------------------------------------------------------------- T2
def err_weight(err):
    """ColorTransfer.cpp:1302-1350: the matching error (float) is rescaled by its extremes — found with < and >, so NaNs never become one — and the confidence is
    max(1 - e, 1e-6) with the Windows max macro ((a) > (b) ? (a) : (b)): a NaN first operand gives 1e-6. A constant map gives 0 / 0, so every weight is 1e-6."""
    e = np.asarray(err, np.float32).reshape(-1).astype(np.float64)
    mn, mx = 1e8, -1e8
    fin = e[~np.isnan(e)]
    if fin.size:
        mn, mx = min(mn, fin.min()), max(mx, fin.max())
    with np.errstate(invalid="ignore", divide="ignore"):
        t = 1.0 - (e - mn) / (mx - mn)
    return np.where(t > 1e-6, t, 1e-6)


# ---------------------------------------------------------------- S1
def gradient_weights(lab, h, w, lamda, alpha):
    """compute_gradientMat, ColorTransfer.cpp:519-546 (the free function; the member :492-517 is the same formula on the full-resolution map): on channel 0,
    gx = sqrt(lamda / (|L(x+1) - L(x)|^alpha + 1e-4)) where x + 1 is inside the map, else 0; gy likewise downwards. lab: [h*w][3] or [h][w][3] in [0, 1]."""
    L = np.asarray(lab, np.float64).reshape(h, w, 3)[..., 0]
    gx = np.zeros((h, w))
    gy = np.zeros((h, w))
    gx[:, :-1] = np.sqrt(lamda / (np.abs(L[:, 1:] - L[:, :-1]) ** alpha + 0.0001))
    gy[:-1, :] = np.sqrt(lamda / (np.abs(L[1:, :] - L[:-1, :]) ** alpha + 0.0001))
    return gx.reshape(-1), gy.reshape(-1)


def s1_system(src, ref, weight, knn_id, knn_w, h, w, lamda, alpha, dweight, nonlocal_weight=2.0, k_num=8.0):
    """solve_nonlocal_downsample_gpu_gradient, ColorTransfer.cpp:548-911: the rectangular least-squares system over the unknowns x = [a (n), b (n)] of one Lab
    channel, per channel c a pair (A_c as scipy CSR, rhs_c). src, ref: level Lab in [0, 1], [n][3]; weight: the T2 confidence [n]; knn_id, knn_w: [n][k]
    (zero-weight entries give zero rows). lamda, alpha, dweight arrive as float in the reference's signature and are rounded to float here; sqrt(dWeight) is the
    float overload of C++ sqrt.
      data term (:611-658):  sqrt(weight) * sqrt(dWeight) * (src_c a + b - ref_c)
      local term (:660-848): for every pixel and each of its four neighbours present, g * (x_nb - x_px) for a and for b, g from gradient_weights of src — so
                             every edge enters twice
      nonlocal (:849-911):   sqrt(w_ij) * sqrt(nonlocal_weight / k_num) * (x_min(i,j) - x_max(i,j)) for a and for b"""
    src = np.asarray(src, np.float64).reshape(-1, 3)
    ref = np.asarray(ref, np.float64).reshape(-1, 3)
    n = h * w
    lamda, alpha = float(np.float32(lamda)), float(np.float32(alpha))
    sq_dw = float(np.sqrt(np.float32(dweight)))
    gx, gy = gradient_weights(src, h, w, lamda, alpha)
    dw = np.sqrt(np.asarray(weight, np.float64).reshape(-1)) * sq_dw
    idx = np.arange(n)
    x, y = idx % w, idx // w
    nrow = n                                       # data rows first: their values depend on the channel
    # local rows: (minus col, plus col, weight) per edge occurrence, for part a and part b
    lm, lp, lg = [], [], []
    for cond, m_off, p_off, g in ((x + 1 < w, 0, 1, gx), (x - 1 >= 0, -1, 0, np.r_[0.0, gx[:-1]]),
                                  (y + 1 < h, 0, w, gy), (y - 1 >= 0, -w, 0, np.r_[np.zeros(w), gy[:-w]] if n > w else np.zeros(n))):
        i = idx[cond]
        for part in (0, n):
            lm.append(i + m_off + part); lp.append(i + p_off + part); lg.append(g[i])
    lm, lp, lg = np.concatenate(lm), np.concatenate(lp), np.concatenate(lg)
    ids = np.asarray(knn_id, np.int64).reshape(n, -1)
    iw = (np.sqrt(np.asarray(knn_w, np.float64).reshape(n, -1)) * np.sqrt(nonlocal_weight / k_num)).reshape(-1)
    i0 = np.repeat(idx, ids.shape[1])
    i1 = ids.reshape(-1)
    nm, npl, ng = [], [], []
    for part in (0, n):
        nm.append(np.minimum(i0, i1) + part); npl.append(np.maximum(i0, i1) + part); ng.append(iw)
    nm, npl, ng = np.concatenate(nm), np.concatenate(npl), np.concatenate(ng)
    nl_rows, nn_rows = lm.size, nm.size
    r_loc = nrow + np.arange(nl_rows)
    r_nl = nrow + nl_rows + np.arange(nn_rows)
    m = nrow + nl_rows + nn_rows
    out = []
    for c in range(3):
        rows = np.concatenate([idx, idx, r_loc, r_loc, r_nl, r_nl])
        cols = np.concatenate([idx, idx + n, lm, lp, nm, npl])
        vals = np.concatenate([dw * src[:, c], dw, -lg, lg, ng, -ng])
        A = sp.csr_matrix((vals, (rows, cols)), shape=(m, 2 * n))
        rhs = np.zeros(m)
        rhs[:n] = dw * ref[:, c]
        out.append((A, rhs))
    return out


def s1_cg(A, rhs, x0, maxit, tol=1e-6):
    """solve_ls_cg_gpu, SparseSolver_GPU.cu:20-159: CG on the normal equations A^T A x = A^T rhs from x0 (Golub & Van Loan 10.2.6), stopped when r.r <= tol^2
    or after maxit iterations; everything in float64 with A^T A formed explicitly. Returns (x, iterations)."""
    AtA = (A.T @ A).tocsr()
    r = A.T @ rhs - AtA @ x0
    x = np.array(x0, np.float64, copy=True)
    r1 = r @ r
    r0 = 0.0
    p = None
    k = 1
    while r1 > tol * tol and k <= maxit:
        p = r.copy() if k == 1 else (r1 / r0) * p + r
        Ap = AtA @ p
        va = r1 / (p @ Ap)
        x += va * p
        r -= va * Ap
        r0 = r1
        r1 = r @ r
        k += 1
    return x, k - 1


def s1_objective(A, rhs, x):
    """f(x) = |A x - rhs|^2, the least-squares energy S1 decreases."""
    d = A @ x - rhs
    return float(d @ d)


# ---------------------------------------------------------------- U1
def _resize_coeffs(ssize, dsize, float_coeffs):
    """cv::resize INTER_LINEAR along one axis (OpenCV's documented mapping): fx = (dx + 0.5) * (ssize / dsize) - 0.5, sx = floor(fx), fx -= sx; sx < 0 gives
    (0, weight 0 on the right tap), sx >= ssize - 1 gives (ssize - 1, weight 0). float_coeffs: fx is computed and kept in float as OpenCV's tables do for 64F."""
    scale = ssize / dsize
    d = np.arange(dsize, dtype=np.float64)
    fx = (d + 0.5) * scale - 0.5
    if float_coeffs:
        fx = fx.astype(np.float32)
        sx = np.floor(fx).astype(np.int64)
        fx = fx - sx.astype(np.float32)
    else:
        sx = np.floor(fx).astype(np.int64)
        fx = fx - sx
    lo = sx < 0
    fx = np.where(lo, 0, fx); sx = np.where(lo, 0, sx)
    hi = sx >= ssize - 1
    fx = np.where(hi, 0, fx); sx = np.where(hi, ssize - 1, sx)
    one = np.float32(1) if float_coeffs else 1.0
    c0, c1 = (one - fx), fx
    return sx, np.minimum(sx + 1, ssize - 1), np.asarray(c0, np.float64), np.asarray(c1, np.float64)


def resize_linear_f64(img, dh, dw, float_coeffs=True):
    """cv::resize(..., INTER_LINEAR) of a 64FC3 map [sh][sw][3] to [dh][dw][3]: horizontal pass S[sx] a0 + S[sx+1] a1, then vertical b0 S0 + b1 S1, in double
    with OpenCV's float coefficient table (float_coeffs=True) or a pure float64 mapping (float_coeffs=False)."""
    img = np.asarray(img, np.float64)
    sh, sw = img.shape[:2]
    x0, x1, a0, a1 = _resize_coeffs(sw, dw, float_coeffs)
    y0, y1, b0, b1 = _resize_coeffs(sh, dh, float_coeffs)
    hz = img[:, x0] * a0[None, :, None] + img[:, x1] * a1[None, :, None]
    return hz[y0] * b0[:, None, None] + hz[y1] * b1[:, None, None]


def resize_linear_u8_exact(img, dh, dw):
    """The float64 value cv::resize(..., INTER_LINEAR) approximates on a u8 image (main.cu:104-108 builds both pyramids with it), before OpenCV rounds to u8:
    the centre mapping (x + 0.5) * s - 0.5 clamped at the borders, in float64 throughout. OpenCV's u8 path computes in fixed point and does not document its
    rounding, so a comparison takes a bound below 1 LSB. img: [sh][sw][3] u8; returns [dh][dw][3] float64."""
    return resize_linear_f64(np.asarray(img, np.uint8).astype(np.float64), dh, dw, float_coeffs=False)


def roughness(ab_up, lab_full):
    """upsample_color_coefficients_bilinear, ColorTransfer.cpp:457-489: per pixel the loop over channels overwrites the flag, so only the LAST channel decides:
    1e-6 when L_2 a_2 + b_2 lies outside [0, 1], else 1. ab_up: [2][N][3]; lab_full: [N][3] in [0, 1]."""
    ab = np.asarray(ab_up, np.float64)
    lab = np.asarray(lab_full, np.float64).reshape(-1, 3)
    nc = lab[:, 2] * ab[0][:, 2] + ab[1][:, 2]
    return np.where((nc < 0) | (nc > 1), 1e-6, 1.0)


# ---------------------------------------------------------------- S2
def wls_system(lab_full, H, W, lamda, alpha, rough):
    """solve_WLS_roughness_cpu, ColorTransfer.cpp:951-1125, with the member compute_gradientMat (:492-517) on channel 0 of the full-resolution Lab map: the
    symmetric system diag(roughness) + the 4-neighbour Laplacian with edge weights gx^2, gy^2. Returns (diag, wx, wy) [H*W] (wx[i]: coupling of i and i + 1,
    wy[i]: of i and i + W; the matrix holds -wx, -wy off the diagonal)."""
    gx, gy = gradient_weights(lab_full, H, W, lamda, alpha)
    wx, wy = gx ** 2, gy ** 2
    d = np.asarray(rough, np.float64).reshape(-1).copy()
    wx2, wy2 = wx.reshape(H, W), wy.reshape(H, W)
    diag = d.reshape(H, W)
    diag = diag + wx2
    diag[:, 1:] += wx2[:, :-1]
    diag = diag + wy2
    diag[1:, :] += wy2[:-1, :]
    return diag.reshape(-1), wx, wy


def wls_matrix(diag, wx, wy, H, W):
    n = H * W
    i = np.arange(n)
    hx = i[(i % W) + 1 < W]
    vy = i[i + W < n]
    rows = np.concatenate([i, hx, hx + 1, vy, vy + W])
    cols = np.concatenate([i, hx + 1, hx, vy + W, vy])
    vals = np.concatenate([diag, -wx[hx], -wx[hx], -wy[vy], -wy[vy]])
    return sp.csc_matrix((vals, (rows, cols)), shape=(n, n))


def wls_solve_exact(ab_up, lab_full, H, W, lamda, alpha, rough):
    """The S2 solve (:1087-1099 and solve_direct_cpu): for each part and channel, M x = roughness * coefficient; a channel whose coefficients are all zero has a
    zero right-hand side and is not solved (its result stays the zero-initialised buffer). Returns [2][N][3]."""
    diag, wx, wy = wls_system(lab_full, H, W, lamda, alpha, rough)
    lu = spla.splu(wls_matrix(diag, wx, wy, H, W))
    ab = np.asarray(ab_up, np.float64)
    out = np.zeros_like(ab)
    r = np.asarray(rough, np.float64).reshape(-1)
    for p in range(2):
        for c in range(3):
            if np.any(ab[p][:, c] != 0):
                out[p][:, c] = lu.solve(r * ab[p][:, c])
    return out


# ---------------------------------------------------------------- A1
def apply_coeffs(ab, lab_full):
    """ColorTransfer.cpp:1440-1478: L a + b clamped to [0, 1] per channel, then convertTo(CV_8U, 255): saturate_cast of v * 255, i.e. cvRound (half to even).
    Returns Lab u8 [N][3]; the Lab -> BGR step that follows is pinned elsewhere."""
    ab = np.asarray(ab, np.float64)
    lab = np.asarray(lab_full, np.float64).reshape(-1, 3)
    v = np.minimum(np.maximum(lab * ab[0] + ab[1], 0.0), 1.0)
    return np.rint(v * 255.0).astype(np.uint8)


def bgr2lab(bgr_u8):
    """CV_BGR2Lab on 8-bit input (main.cu:352,371; ColorTransfer.h:58) by OpenCV's documented mapping, in float64 without its tables: sRGB gamma
    (v <= 0.04045: v / 12.92, else ((v + 0.055) / 1.055)^2.4), the D65 matrix, X / Xn and Z / Zn, f(t) = t^(1/3) above 0.008856 and 7.787 t + 16/116 below,
    L = 116 Y^(1/3) - 16 (903.3 Y below 0.008856), a = 500 (f(X) - f(Y)), b = 200 (f(Y) - f(Z)); then the 8-bit scaling L * 255/100, a + 128, b + 128.
    OpenCV's 8-bit path quantises linear light to 1/2040 (sRGBGammaTab_b) and the cube root to a table (LabCbrtTab_b), so it differs from this, most in dark
    colours. Returns (Lab u8 [..., 3] rounded half to even and saturated, the unrounded float64 values)."""
    v = np.asarray(bgr_u8, np.uint8).astype(np.float64) / 255.0
    lin = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    B, G, R = lin[..., 0], lin[..., 1], lin[..., 2]
    X = (0.412453 * R + 0.357580 * G + 0.180423 * B) / 0.950456
    Y = 0.212671 * R + 0.715160 * G + 0.072169 * B
    Z = (0.019334 * R + 0.119193 * G + 0.950227 * B) / 1.088754

    def f(t):
        return np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)

    L = np.where(Y > 0.008856, 116.0 * np.cbrt(Y) - 16.0, 903.3 * Y)
    val = np.stack([L * 255.0 / 100.0, 500.0 * (f(X) - f(Y)) + 128.0, 200.0 * (f(Y) - f(Z)) + 128.0], -1)
    return np.clip(np.rint(val), 0, 255).astype(np.uint8), val


def lab2bgr(lab_u8, form):
    """CV_Lab2BGR on 8-bit input (ColorTransfer.cpp:1469): L_u8 * 100/255, a - 128, b - 128, the float Lab2RGB_f in float64 without tables (exact sRGB gamma),
    saturate_cast<uchar>(v * 255). The two forms of Lab2RGB_f in OpenCV's history:
      form 0 (piecewise): CIE's linear branch below L* = 8 (Y = L / 903.3) and below f = 6/29 ((f - 16/116) / 7.787); linear RGB clipped to [0, 1];
      form 1 (plain cubes): fY = (L + 16) / 116, fX = fY + a / 500, fZ = fY - b / 200, each cubed; linear RGB not clipped before the gamma table.
    Returns (BGR u8-valued float64 [n][3], far_out [n][3]): far_out marks, in the cube form only, channels far below the gamut (linear value < -0.02), where
    OpenCV's spline table is extrapolated hundreds of steps and its cubic term takes over — a saturated byte (0 or 255) this function does not model."""
    lab = np.asarray(lab_u8).reshape(-1, 3)
    L = lab[:, 0].astype(np.float64) * 100 / 255; a = lab[:, 1].astype(np.float64) - 128; b = lab[:, 2].astype(np.float64) - 128
    if form == 1:
        fy = (L + 16) / 116
        y, X, Z = fy ** 3, (fy + a / 500) ** 3 * 0.950456, (fy - b / 200) ** 3 * 1.088754
    else:
        fy = np.where(L <= 0.008856 * 903.3, 7.787 * (L / 903.3) + 16 / 116, (L + 16) / 116)
        y = np.where(L <= 0.008856 * 903.3, L / 903.3, fy ** 3)
        finv = lambda f: np.where(f <= 7.787 * 0.008856 + 16 / 116, (f - 16 / 116) / 7.787, f ** 3)
        X, Z = finv(a / 500 + fy) * 0.950456, finv(fy - b / 200) * 1.088754
    M = np.array([[3.240479, -1.53715, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])
    rgb = np.stack([X, y, Z], 1) @ M.T
    far_out = rgb[:, ::-1] < -0.02
    if form == 0:
        rgb = np.clip(rgb, 0, 1)
    srgb = np.where(rgb <= 0.0031308, 12.92 * rgb, 1.055 * np.maximum(rgb, 0) ** (1 / 2.4) - 0.055)
    return np.clip(np.rint(srgb[:, ::-1] * 255), 0, 255), (far_out if form == 1 else np.zeros_like(far_out))


# ---------------------------------------------------------------- C1
def _perm_splitmix(n, seed):
    """SPEC.md §4's stand-in for MSVC rand() in UniqueRandom: the Fisher-Yates permutation of 0 .. n-1 driven by SplitMix64 from `seed` — for i = n-1 down to 1,
    j = next() mod (i + 1), swap(perm[i], perm[j])."""
    M = (1 << 64) - 1
    perm = list(range(n))
    x = seed & M
    for i in range(n - 1, 0, -1):
        x = (x + 0x9E3779B97F4A7C15) & M
        z = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        j = (z ^ (z >> 31)) % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def _l2_float(pts, centres, chunk=256):
    """cvflann::L2<float>::operator() (Flann/dist.h:153-181) of float points [n][C] against centres [K][C] (float or double): each difference is taken in the
    wider type and converted to float, the four squares of a group summed left to right in float and added to a float accumulator group by group; a tail of
    C mod 4 terms one at a time. Returns float32 [n][K], emulated exactly with np.float32 (np.add.accumulate adds sequentially)."""
    p = np.asarray(pts, np.float32)
    c = np.asarray(centres)
    wide = np.float64 if c.dtype == np.float64 else np.float32
    n, C = p.shape
    g = C - C % 4
    out = np.empty((n, c.shape[0]), np.float32)
    cw = c.astype(wide)
    for s0 in range(0, n, chunk):
        d = (p[s0:s0 + chunk, None, :].astype(wide) - cw[None]).astype(np.float32)
        q = d * d
        if g:
            q4 = q[..., :g].reshape(q.shape[0], q.shape[1], g // 4, 4)
            grp = ((q4[..., 0] + q4[..., 1]) + q4[..., 2]) + q4[..., 3]
            acc = np.add.accumulate(grp, axis=-1, dtype=np.float32)[..., -1]
        else:
            acc = np.zeros(q.shape[:2], np.float32)
        for i in range(g, C):
            acc = acc + q[..., i]
        out[s0:s0 + chunk] = acc
    return out


def kmeans_labels(feat_chw, K=10, iters=11, seed=1, exact=False, normalized=False, want_info=False):
    """clusterFeastures (ColorTransfer.cpp:355-395): cvflann::hierarchicalClustering<L2<float>> with KMeansIndexParams(K, 11, FLANN_CENTERS_RANDOM) on the
    normalised conv5_1 features (normalize, rounded to the float buffer the reference clusters); the labels are the root's split, computeClustering
    (Flann/kmeans_index.h:700-880):
      - K == 1 is one cluster: every label 0, one label, margin inf. The reference's FLANN refuses a branching below 2 (Flann/kmeans_index.h:370-372), so
        this is the library's own rule (nct_cluster_features, include/nct.h), not the reference's;
      - n < K, or fewer than K distinct centres found, leaves the root a leaf: one label (:705-710, :716-722);
      - chooseCentersRandom (:108-135): candidates in the order of _perm_splitmix (SPEC.md §4), skipping one whose float distance to an earlier centre is
        below 1e-16;
      - assignment: the first centre, then each later one if strictly nearer (sq_dist > new_sq_dist: ties go to the lower id), distances _l2_float against
        the double centres; the radius of a cluster is its largest such distance;
      - up to `iters` Lloyd steps while any label changes: centres are double sums in ascending point order divided by the count; a cluster left empty takes
        the first point (ascending) of the next cluster with more than one member whose distance equals that cluster's radius, and the step is not converged.
    exact: distances in float64 instead (to confirm the float emulation where the margin is large). normalized: feat_chw is already the normalised float map
    (taken as is). want_info: also return {"steps": Lloyd steps run, "converged": bool, "donors": empty-cluster moves}. Returns (labels [h][w] int32, number of labels, margin):
    margin is the smallest relative gap (second - best) / second between the nearest and second-nearest centre over all points and assignment passes, and,
    where a donor moved, between the radius and the next distance in the donor cluster — how far a perturbation of the inputs can go before a label flips."""
    f = np.asarray(feat_chw, np.float32) if normalized else normalize(feat_chw).astype(np.float32)
    C, h, w = f.shape
    info = {"steps": 0, "converged": False, "donors": 0}
    done = (lambda *r: r + (info,)) if want_info else (lambda *r: r)
    n = h * w
    pts = np.ascontiguousarray(f.reshape(C, n).T)
    labels = np.zeros(n, np.int32)
    if n < K or K == 1:
        return done(labels.reshape(h, w), 1, np.inf)
    dist = (lambda p, c: ((p.astype(np.float64)[:, None, :] - np.asarray(c, np.float64)[None]) ** 2).sum(-1)) if exact else _l2_float
    perm = _perm_splitmix(n, seed)
    cidx, pos = [], 0
    while len(cidx) < K:
        if pos >= n:
            return done(labels.reshape(h, w), 1, np.inf)
        cand = perm[pos]; pos += 1
        if cidx and (_l2_float(pts[cand:cand + 1], pts[cidx]) < 1e-16).any():
            continue
        cidx.append(cand)
    centres = pts[cidx].astype(np.float64)
    margin = np.inf

    def assign(centres):
        d = dist(pts, centres)
        lab = np.argmin(d, 1).astype(np.int32)               # first minimum = the lower id on ties, as the strict > does
        best = d[np.arange(n), lab]
        two = np.partition(d, 1, axis=1)[:, :2].astype(np.float64)
        gap = (two[:, 1] - two[:, 0]) / np.where(two[:, 1] > 0, two[:, 1], 1.0)
        return lab, best, float(gap.min())

    bel, best, m = assign(centres)
    margin = min(margin, m)
    count = np.bincount(bel, minlength=K)
    for _ in range(iters):
        info["steps"] += 1
        centres = np.zeros((K, C))
        for i in range(K):                                   # double sums in ascending point order (np.cumsum adds sequentially)
            if count[i]:
                centres[i] = np.cumsum(pts[bel == i].astype(np.float64), 0)[-1]
        with np.errstate(invalid="ignore", divide="ignore"):
            centres /= count[:, None]
        new, best, m = assign(centres)
        margin = min(margin, m)
        radius = np.zeros(K, best.dtype)
        np.maximum.at(radius, new, best)
        converged = np.array_equal(new, bel)
        bel = new
        count = np.bincount(bel, minlength=K)
        for i in range(K):
            if count[i] == 0:
                j, tries = (i + 1) % K, 0
                while count[j] <= 1 and tries < K:           # the reference spins forever when no cluster can give
                    j, tries = (j + 1) % K, tries + 1
                if count[j] <= 1:
                    continue
                dj = dist(pts, centres[j:j + 1])[:, 0]
                mem = np.flatnonzero(bel == j)
                far = np.flatnonzero(dj[mem] == radius[j])     # none when an earlier move this step took cluster j's farthest point
                if far.size:
                    rest = np.sort(dj[mem])[::-1]
                    if rest.size > 1 and rest[0] > 0:
                        margin = min(margin, float((rest[0] - rest[1]) / rest[0]))
                    kk = mem[far[0]]
                    bel[kk] = i; count[j] -= 1; count[i] += 1
                    info["donors"] += 1
                converged = False
        if converged:
            info["converged"] = True
            break
    return done(bel.reshape(h, w), K, margin)


# ---------------------------------------------------------------- K1
def cluster_members(labels, nlabels):
    """getClusters (ColorTransfer.cpp:273-330) on the label grid: cell (x, y) joins its own label's cluster and the cluster of every 4-neighbour whose label
    differs (the neighbour's cell is marked in the cell's cluster). Returns member [nlabels][lh][lw] bool."""
    lab = np.asarray(labels, np.int64)
    lh, lw = lab.shape
    mem = np.zeros((nlabels, lh, lw), bool)
    yy, xx = np.mgrid[0:lh, 0:lw]
    mem[lab, yy, xx] = True
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        ys, xs = yy + dy, xx + dx
        ok = (ys >= 0) & (ys < lh) & (xs >= 0) & (xs < lw)
        ok[ok] &= lab[ys[ok], xs[ok]] != lab[ok]
        mem[lab[ok], ys[ok], xs[ok]] = True
    return mem


def _cluster_top(key, ids, col, k):
    """The first k + 1 (distance, id) pairs of every distinct colour of one cluster over all its members, self included (the query's own colour at distance
    0). key: packed 24-bit colours of the members, ids: their pixel ids, col: their Lab bytes. Returns (colour index per member, top ids [m][k+1] padded -1,
    top distances [m][k+1] padded inf)."""
    from scipy.spatial import cKDTree
    order = np.lexsort((ids, key))
    key, ids, col = key[order], ids[order], col[order]
    uk, first, inv, cnt = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    uc = col[first].astype(np.int64)
    m = uk.size
    kk = min(k + 1, m)
    # each colour's first k + 1 pixel ids (ascending): no colour contributes more
    take = np.minimum(cnt, k + 1)
    rank = np.arange(key.size) - first[inv]
    sel = rank < k + 1
    cid = np.full((m, k + 1), -1, np.int64)
    cid[inv[sel], rank[sel]] = ids[sel]
    # D: the largest integer squared distance among the k + 1 nearest distinct colours; every colour with integer squared distance <= D is a candidate
    tree = cKDTree(uc.astype(np.float64))
    _, nn = tree.query(uc.astype(np.float64), k=kk)
    nn = nn.reshape(m, kk)
    D = ((uc[nn] - uc[:, None, :]) ** 2).sum(-1).max(1)
    balls = tree.query_ball_point(uc.astype(np.float64), np.sqrt(D) + 1e-6, return_sorted=False)
    ln = np.fromiter((len(b) for b in balls), np.int64, m)
    q = np.repeat(np.arange(m), ln)
    c = np.concatenate([np.asarray(b, np.int64) for b in balls])
    keep = ((uc[c] - uc[q]) ** 2).sum(-1) <= D[q]
    q, c = q[keep], c[keep]
    # PointColor::kdtree_distance (ColorTransfer.cpp:20-27) on convertTo(CV_64F, 1/255) values (main.cu:355-356)
    lab = uc.astype(np.float64) * (1.0 / 255.0)
    dv = lab[c] - lab[q]
    d = np.maximum(np.sqrt(dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1] + dv[:, 2] * dv[:, 2]), 0.0)
    # expand every candidate colour to its first take[c] ids, then the k + 1 smallest (d, id) per query colour
    t = take[c]
    qe = np.repeat(q, t)
    de = np.repeat(d, t)
    off = np.arange(t.sum()) - np.repeat(np.cumsum(t) - t, t)
    ie = cid[np.repeat(c, t), off]
    o = np.lexsort((ie, de, qe))
    qe, de, ie = qe[o], de[o], ie[o]
    start = np.searchsorted(qe, np.arange(m))
    r = np.arange(qe.size) - start[qe]
    s = r < k + 1
    top_id = np.full((m, k + 1), -1, np.int64)
    top_d = np.full((m, k + 1), np.inf)
    top_id[qe[s], r[s]] = ie[s]
    top_d[qe[s], r[s]] = de[s]
    inv_orig = np.empty_like(inv)
    inv_orig[order] = inv
    return inv_orig, top_id, top_d


def knn_graph(lab_u8, labels, nlabels, samples, k=8):
    """findKnns (ColorTransfer.cpp:397-423) with the (distance, id) order of cmpDist for the KD-tree's ties (SPEC.md §4): lab_u8 is the level's Lab u8 map
    [h][w][3], labels the k-means grid [lh][lw].
      getClusters (:273-330): cluster_members; insertClusterPixel (:255-271): every member cell (x, y) contributes the samples x samples block at
        (x * samples, y * samples), clipped at the level's edge;
      findSubKNNs (:136-190): per cluster and member, the k + 1 smallest (distance, id) over the cluster, self included; self dropped if among them; the
        first k kept;
      sortMergeComputeWeight (:60-110): a pixel's lists of all its clusters sorted by cmpDist (:44), repeated ids dropped, the first k kept, w = exp(1 - d/3)
        (not normalised: convertDist2Weight is never called on this path); fewer than k distinct neighbours are padded with self at weight 0 (quirk 10, where
        the reference asserts).
    Distinct colours are searched with a KD-tree over integer Lab, every colour up to the (k + 1)-th nearest colour's integer squared distance gathered (equal
    integer distances need not stay equal after the double rounding; distinct ones stay ordered). Returns (ids [h*w][k] int32, weights [h*w][k] float64)."""
    lab = np.asarray(lab_u8, np.uint8)
    h, w = lab.shape[:2]
    n = h * w
    col = lab.reshape(n, 3)
    key = (col[:, 0].astype(np.int64) << 16) | (col[:, 1].astype(np.int64) << 8) | col[:, 2]
    mem = cluster_members(labels, nlabels)
    lh, lw = mem.shape[1:]
    py, px = np.divmod(np.arange(n), w)
    cy, cx = py // samples, px // samples
    inside = (cy < lh) & (cx < lw)
    cand_d = np.full((n, 5 * k), np.inf)
    cand_i = np.full((n, 5 * k), -1, np.int64)
    nc = np.zeros(n, np.int64)
    for l in range(nlabels):
        m_ok = np.zeros(n, bool)
        m_ok[inside] = mem[l, cy[inside], cx[inside]]
        ids = np.flatnonzero(m_ok)
        if ids.size == 0:
            continue
        ci, top_id, top_d = _cluster_top(key[ids], ids, col[ids], k)
        ti, td = top_id[ci], top_d[ci]
        is_self = ti == ids[:, None]
        drop = np.where(is_self.any(1), np.argmax(is_self, 1), k)
        keep = np.arange(k + 1)[None, :] != drop[:, None]
        ti = ti[keep].reshape(-1, k)
        td = td[keep].reshape(-1, k)
        slot = nc[ids][:, None] * k + np.arange(k)[None, :]
        cand_i[ids[:, None], slot] = ti
        cand_d[ids[:, None], slot] = td
        nc[ids] += 1
    o = np.lexsort((cand_i, cand_d), axis=1)
    cd = np.take_along_axis(cand_d, o, 1)
    cdi = np.take_along_axis(cand_i, o, 1)
    valid = cdi >= 0
    first = np.ones_like(valid)
    first[:, 1:] = cdi[:, 1:] != cdi[:, :-1]
    use = valid & first
    rank = np.cumsum(use, 1) - 1
    use &= rank < k
    out_i = np.repeat(np.arange(n, dtype=np.int64)[:, None], k, 1)
    out_w = np.zeros((n, k))
    rr, cc = np.nonzero(use)
    out_i[rr, rank[rr, cc]] = cdi[rr, cc]
    out_w[rr, rank[rr, cc]] = np.exp(1.0 - cd[rr, cc] / 3.0)
    return out_i.astype(np.int32), out_w
