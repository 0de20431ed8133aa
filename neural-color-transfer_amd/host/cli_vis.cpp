// ---- ENABLE_VIS debug outputs (Config.h:8) behind the runtime flag -vis 1: per pyramid level the flow maps of both NNFs (reconstruct_flow,
// GeneralizedPatchMatch.cu:337-353), the level images tCnt / tStl (main.cu:343-347), the matching-error heat map (getHeat,
// ColorTransfer.cpp:1127-1178 on the min-max normalised error, :1318-1338) — under the reference's file names <pre>_aFlow_<l>.png … — plus
// the BDS guidance image and the intermediate result of the level (guide_<l>, result_<l>: not dumped by the reference, but what its
// refine_* images are for); the linear colour coefficients after each stage of the level as aVis / bVis images and the source recoloured by
// them (aVis_init, bVis_init, refine_init: local statistics sampled with x / samples, ColorTransfer.cpp:1268-1300; aVis_nonlocal, bVis_nonlocal,
// refine_nonlocal: after the nonlocal solve and the bilinear upsampling, :1384-1413; aVis, bVis: after the WLS solve, :1450-1463); the
// clusters as <pre>_cluster_small.png and per level as knn_<l>.png (visualizeClusterRandom / findKnns, :222-246, :336-351 — with a hashed
// palette: the reference's 260-entry RandomColorList is a data table of its Config.h); patchVis_<l>: per level pixel a 3-wide, 6-high cell
// with the (border-clipped) 3x3 patch of the guidance image above that of the level image, the windows of the local statistics (:1190-1221).
// <pre> = the output file's stem.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "cli_job.h"

namespace {
const char* const kCannotWrite = "cannot write the -vis images";
// the sizes of an image's five pyramid levels, [4] the image's own, each coarser one the half rounded up
struct LevelSizes {
    int h[5], w[5];
    LevelSizes(int H, int W) { for (int l = 4; l >= 0; --l) { h[l] = H; w[l] = W; H = (H - 1) / 2 + 1; W = (W - 1) / 2 + 1; } }
    size_t n(int l) const { return (size_t)h[l] * w[l]; }
};
// <pre>_<what>_<l>.png, of three channels or of one
bool save(const std::string& pre, const char* what, int l, const uint8_t* px, int h, int w, int ch = 3) {
    char name[1200]; snprintf(name, sizeof name, "%s_%s_%d.png", pre.c_str(), what, l);
    std::string e; return pngio::write(name, px, h, w, e, ch);
}
void heat(double v, uint8_t* bgr) {
    v = !(v >= 0) ? 0 : (v > 1 ? 1 : v);          // NaN -> 0 as well
    double dr, dg, db;
    if (v < 0.1242) { db = 0.504 + ((1. - 0.504) / 0.1242) * v; dg = dr = 0.; }
    else if (v < 0.3747) { db = 1.; dr = 0.; dg = (v - 0.1242) * (1. / (0.3747 - 0.1242)); }
    else if (v < 0.6253) { db = (0.6253 - v) * (1. / (0.6253 - 0.3747)); dg = 1.; dr = (v - 0.3747) * (1. / (0.6253 - 0.3747)); }
    else if (v < 0.8758) { db = 0.; dr = 1.; dg = (0.8758 - v) * (1. / (0.8758 - 0.6253)); }
    else { db = 0.; dg = 0.; dr = 1. - (v - 0.8758) * ((1. - 0.504) / (1. - 0.8758)); }
    auto q = [](double d) { const int i = (int)(255 * d); return (uint8_t)(i > 255 ? 255 : i); };
    bgr[0] = q(db); bgr[1] = q(dg); bgr[2] = q(dr);
}

// The front that both kinds of line share: upload, the masks' set-up, the run with the level buffers of its kind (pl for one reference, ml for several), download, and
// the masks' own dumps: a masked line's level masks (SPEC §6.11 rule 1) as 8-bit grey images <pre>_mask_<l>.png, and the pulled masks P_l of masked references
// (SPEC §6.12 rules 2-3), merged over the references by the level's label map (label; unused with one reference), as <pre>_refmask_<l>.png
bool run_and_dump_masks(const VisLine& L, const LevelSizes& A, nct_pair_levels* pl, nct_multi_levels* ml, const std::vector<std::vector<uint8_t>>& label) {
    nct_ctx* ctx = L.ctx; const ImageBGR& cnt = L.cnt; const int K = L.K, levels = L.prm.levels;
    auto failed = [&] { L.err = nct_last_error(ctx); return false; };
    if ((K > 1 ? nct_multi_upload(ctx, cnt.px.data(), cnt.h, cnt.w, K, L.px, L.rh, L.rw) : nct_pair_upload(ctx, cnt.px.data(), cnt.h, cnt.w, L.px[0], L.rh[0], L.rw[0])) != NCT_OK ||
        (L.mask && nct_pair_set_region(ctx, L.mask, L.region) != NCT_OK)) return failed();
    std::vector<std::vector<uint8_t>> pulled[NCT_MAX_REFS];
    nct_ref_region_levels rl; memset(&rl, 0, sizeof rl);
    for (int k = 0; k < K && L.refmasks; ++k) {
        if (!L.refmasks[k]) continue;
        if (nct_pair_set_ref_region(ctx, k, L.refmasks[k], L.region) != NCT_OK) return failed();
        pulled[k].resize(5);
        for (int l = 0; l < levels; ++l) { pulled[k][l].resize(A.n(l)); rl.pulled[k][l] = pulled[k][l].data(); }
    }
    const int rc = K > 1 ? (L.refmasks ? nct_multi_run_ref_region_levels(ctx, &L.prm, L.tm, ml, &rl) : nct_multi_run_levels(ctx, &L.prm, L.tm, ml))
                         : (L.refmasks ? nct_pair_run_ref_region_levels(ctx, &L.prm, L.tm, pl, &rl) : nct_pair_run_levels(ctx, &L.prm, L.tm, pl));
    if (rc != NCT_OK || nct_pair_download(ctx, L.out) != NCT_OK) return failed();
    if (L.mask) {
        std::vector<std::vector<uint8_t>> m(5);
        m[4].assign(L.mask, L.mask + A.n(4));
        for (int l = 3; l >= 0; --l) {
            m[l].resize(A.n(l));
            if (nct_resize_u8c1(ctx, m[l + 1].data(), A.h[l + 1], A.w[l + 1], m[l].data(), A.h[l], A.w[l]) != NCT_OK) return failed();
        }
        for (int l = 0; l < levels; ++l) if (!save(L.pre, "mask", l, m[l].data(), A.h[l], A.w[l], 1)) { L.err = kCannotWrite; return false; }
    }
    for (int l = 0; l < levels && L.refmasks; ++l) {
        std::vector<uint8_t> P(A.n(l));
        for (size_t i = 0; i < P.size(); ++i) { const auto& pk = pulled[K > 1 ? label[l][i] : 0]; P[i] = pk.empty() ? 255 : pk[l][i]; }
        if (!save(L.pre, "refmask", l, P.data(), A.h[l], A.w[l], 1)) { L.err = kCannotWrite; return false; }
    }
    return true;
}

// one reference: the whole set of dumps
bool pair_with_vis(const VisLine& L) {
    nct_ctx* ctx = L.ctx; const ImageBGR& cnt = L.cnt; const nct_params& prm = L.prm; std::string& err = L.err;
    const LevelSizes A(cnt.h, cnt.w), B(L.rh[0], L.rw[0]);
    const int* ah = A.h; const int* aw = A.w; const int* bh = B.h; const int* bw = B.w;
    std::vector<std::vector<uint32_t>> ann(5), bnn(5);
    std::vector<std::vector<uint8_t>> guide(5), result(5), simg(5), rimg(5);
    std::vector<std::vector<float>> errm(5);
    std::vector<std::vector<double>> ab_local(5), ab_up(5), ab_wls(5);
    std::vector<int> labels(A.n(0));
    nct_color_stages cs[5]; memset(cs, 0, sizeof cs);
    const size_t N = (size_t)cnt.h * cnt.w;
    nct_pair_levels lv; memset(&lv, 0, sizeof lv);
    lv.labels = labels.data();
    for (int l = 0; l < prm.levels; ++l) {
        ab_local[l].resize(6 * A.n(l)); ab_up[l].resize(6 * N); ab_wls[l].resize(6 * N);
        cs[l].ab_local = ab_local[l].data(); cs[l].ab_up = ab_up[l].data(); cs[l].ab_wls = ab_wls[l].data();
        lv.color[l] = &cs[l];
        ann[l].resize(A.n(l)); bnn[l].resize(B.n(l)); guide[l].resize(A.n(l) * 3);
        errm[l].resize(A.n(l)); result[l].resize(N * 3);
        lv.ann[l] = ann[l].data(); lv.bnn[l] = bnn[l].data(); lv.guide[l] = guide[l].data(); lv.err[l] = errm[l].data(); lv.result[l] = result[l].data();
    }
    if (!run_and_dump_masks(L, A, &lv, nullptr, {})) return false;
    // level images: the progressive bilinear pyramid of main.cu:104-108
    simg[4] = cnt.px; rimg[4].assign(L.px[0], L.px[0] + B.n(4) * 3);
    for (int l = 3; l >= 0; --l) {
        simg[l].resize(A.n(l) * 3); rimg[l].resize(B.n(l) * 3);
        if (nct_resize_u8c3(ctx, simg[l + 1].data(), ah[l + 1], aw[l + 1], simg[l].data(), ah[l], aw[l]) != NCT_OK ||
            nct_resize_u8c3(ctx, rimg[l + 1].data(), bh[l + 1], bw[l + 1], rimg[l].data(), bh[l], bw[l]) != NCT_OK) { err = nct_last_error(ctx); return false; }
    }
    auto save = [&](const char* what, int l, const uint8_t* px, int h, int w) { return ::save(L.pre, what, l, px, h, w); };
    // coefficient images: a -> int(a * 50), b -> int(b * 255 + 127), clamped to a byte (the clamp in double first: the cast of an
    // out-of-range double is undefined); recoloured source: clamp(lab / 255 * a + b, 0, 1) -> 8 bit (convertTo, round half to even) -> BGR
    std::vector<uint8_t> lab(N * 3);
    if (nct_bgr2lab_u8(ctx, cnt.px.data(), N, lab.data()) != NCT_OK) { err = nct_last_error(ctx); return false; }
    auto coef_images = [&](const char* tag, int l, const double* ab, int h, int w, int samples) {
        const double* a = ab; const double* b = ab + (size_t)3 * h * w;
        std::vector<uint8_t> av(N * 3), bv(N * 3), rl(N * 3), rb(N * 3);
        for (int y = 0; y < cnt.h; ++y)
            for (int x = 0; x < cnt.w; ++x) {
                const size_t i = (size_t)y * cnt.w + x, j = (size_t)(y / samples) * w + x / samples;
                for (int c = 0; c < 3; ++c) {
                    const double ac = a[3 * j + c], bc = b[3 * j + c];
                    auto byte = [](double v) { return (uint8_t)(int)(v != v ? 0. : (v < 0. ? 0. : (v > 255. ? 255. : v))); };
                    av[3 * i + c] = byte(ac * 50); bv[3 * i + c] = byte(bc * 255 + 127);
                    double v = lab[3 * i + c] / 255.0 * ac + bc;
                    v = v > 0.0 ? v : 0.0; v = v < 1.0 ? v : 1.0;
                    rl[3 * i + c] = (uint8_t)nearbyint(v * 255.0);
                }
            }
        const std::string t(tag);
        if (!save(("aVis" + t).c_str(), l, av.data(), cnt.h, cnt.w) || !save(("bVis" + t).c_str(), l, bv.data(), cnt.h, cnt.w)) return false;
        if (t.empty()) return true;                                      // the recoloured source after the WLS solve is result_<l>
        return nct_lab2bgr_u8(ctx, rl.data(), N, rb.data()) == NCT_OK && save(("refine" + t).c_str(), l, rb.data(), cnt.h, cnt.w);
    };
    auto palette = [](int label, uint8_t* bgr) {
        uint32_t hsh = (uint32_t)(label + 1) * 2654435761u; hsh ^= hsh >> 15; hsh *= 2246822519u; hsh ^= hsh >> 13;
        bgr[0] = (uint8_t)(64 + (hsh & 0xBF)); bgr[1] = (uint8_t)(64 + ((hsh >> 8) & 0xBF)); bgr[2] = (uint8_t)(64 + ((hsh >> 16) & 0xBF));
    };
    auto cluster_image = [&](int h, int w, int samples) {
        std::vector<uint8_t> im((size_t)h * w * 3);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const int ly = std::min(y / samples, ah[0] - 1), lx = std::min(x / samples, aw[0] - 1);
                palette(labels[(size_t)ly * aw[0] + lx], &im[((size_t)y * w + x) * 3]);
            }
        return im;
    };
    { const auto im = cluster_image(ah[0], aw[0], 1);
      std::string e; if (!pngio::write((L.pre + "_cluster_small.png").c_str(), im.data(), ah[0], aw[0], e)) { err = kCannotWrite; return false; } }
    auto patch_image = [&](const uint8_t* stl_px, const uint8_t* cnt_px, int h, int w) {
        const int ps = 3;
        std::vector<uint8_t> im((size_t)h * ps * 2 * w * ps * 3, 0);
        const size_t pitch = (size_t)w * ps * 3;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const int sx0 = std::max(x - 1, 0), sy0 = std::max(y - 1, 0), ex = std::min(x + 2, w), ey = std::min(y + 2, h);
                for (int sy = sy0; sy < ey; ++sy)
                    for (int sx = sx0; sx < ex; ++sx) {
                        memcpy(&im[(size_t)(y * ps * 2 + sy - sy0) * pitch + (size_t)(x * ps + sx - sx0) * 3], &stl_px[((size_t)sy * w + sx) * 3], 3);
                        memcpy(&im[(size_t)(y * ps * 2 + ps + sy - sy0) * pitch + (size_t)(x * ps + sx - sx0) * 3], &cnt_px[((size_t)sy * w + sx) * 3], 3);
                    }
            }
        return im;
    };
    for (int l = 0; l < prm.levels; ++l) {
        if (!save("patchVis", l, patch_image(guide[l].data(), simg[l].data(), ah[l], aw[l]).data(), ah[l] * 6, aw[l] * 3)) { err = kCannotWrite; return false; }
        if (!coef_images("_init", l, ab_local[l].data(), ah[l], aw[l], 1 << (4 - l)) || !coef_images("_nonlocal", l, ab_up[l].data(), cnt.h, cnt.w, 1) ||
            !coef_images("", l, ab_wls[l].data(), cnt.h, cnt.w, 1) || !save("knn", l, cluster_image(ah[l], aw[l], 1 << l).data(), ah[l], aw[l])) {
            err = kCannotWrite; return false; }
        auto flow = [&](const std::vector<uint32_t>& nn, int h, int w, int oh, int ow) {
            std::vector<uint8_t> f((size_t)h * w * 3);
            for (size_t i = 0; i < (size_t)h * w; ++i) {
                const int xb = (int)(nn[i] & 0xFFFu), yb = (int)((nn[i] >> 12) & 0xFFFu);
                f[3 * i] = (uint8_t)(255 * ((float)xb / ow)); f[3 * i + 1] = 0; f[3 * i + 2] = (uint8_t)(255 * ((float)yb / oh));
            }
            return f;
        };
        const auto fa = flow(ann[l], ah[l], aw[l], bh[l], bw[l]), fb = flow(bnn[l], bh[l], bw[l], ah[l], aw[l]);
        float mn = errm[l][0], mx = errm[l][0];
        for (float e : errm[l]) { mn = e < mn ? e : mn; mx = e > mx ? e : mx; }
        std::vector<uint8_t> hm(A.n(l) * 3);
        // a constant error map normalises to 0 (cv::normalize's min-max of a flat image), not 0/0
        for (size_t i = 0; i < errm[l].size(); ++i) heat(mx > mn ? ((double)errm[l][i] - mn) / ((double)mx - mn) : 0.0, &hm[3 * i]);
        if (!save("aFlow", l, fa.data(), ah[l], aw[l]) || !save("bFlow", l, fb.data(), bh[l], bw[l]) || !save("tCnt", l, simg[l].data(), ah[l], aw[l]) ||
            !save("tStl", l, rimg[l].data(), bh[l], bw[l]) || !save("errMap", l, hm.data(), ah[l], aw[l]) || !save("guide", l, guide[l].data(), ah[l], aw[l]) ||
            !save("result", l, result[l].data(), cnt.h, cnt.w)) { err = kCannotWrite; return false; }
    }
    return true;
}

// several references: per level the label map as an 8-bit grey image (label * (255 / max(K - 1, 1))), the merged guidance image and the intermediate result, named
// like a pair's dumps (<pre>_label_<l>.png, <pre>_guide_<l>.png, <pre>_result_<l>.png)
bool multi_with_vis(const VisLine& L) {
    const LevelSizes A(L.cnt.h, L.cnt.w);
    std::vector<std::vector<uint8_t>> label(5), guide(5), result(5);
    nct_multi_levels lv; memset(&lv, 0, sizeof lv);
    for (int l = 0; l < L.prm.levels; ++l) {
        label[l].resize(A.n(l)); guide[l].resize(A.n(l) * 3); result[l].resize(A.n(4) * 3);
        lv.label[l] = label[l].data(); lv.guide[l] = guide[l].data(); lv.result[l] = result[l].data();
    }
    if (!run_and_dump_masks(L, A, nullptr, &lv, label)) return false;
    const int step = 255 / std::max(L.K - 1, 1);
    for (int l = 0; l < L.prm.levels; ++l) {
        for (uint8_t& v : label[l]) v = (uint8_t)(v * step);
        if (!save(L.pre, "label", l, label[l].data(), A.h[l], A.w[l], 1) || !save(L.pre, "guide", l, guide[l].data(), A.h[l], A.w[l]) ||
            !save(L.pre, "result", l, result[l].data(), L.cnt.h, L.cnt.w)) { L.err = kCannotWrite; return false; }
    }
    return true;
}
}  // namespace

bool run_with_vis(const VisLine& L) { return L.K > 1 ? multi_with_vis(L) : pair_with_vis(L); }
