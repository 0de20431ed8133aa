"""The CPU oracle vs tests/ref64.py away from nct_params_default: the seven values of nct_params that reach kernel arguments and kernel dispatch (eps,
nonlocal_weight, local_weight, wls_lambda_init, wls_alpha, cluster_num; k_num stays 8). Every check is one of tests/test_ref64_oracle.py with the parameters
handed to both sides, at that file's bars, unchanged. tests/test_gpu_params.py holds the kernels to the oracle bit for bit on the same sets, so what these pin, the
kernels inherit.

PARAM_SETS: "help" holds the values the console driver's help strings quote (main.cu:40-43), "strong" and "soft" lie well to either side of the defaults. Three of
the local_weight / wls_alpha values (0.001, 0.7, 0.03; 0.8) are not representable in float: S1 takes both as float (ColorTransfer.cpp:548-550), S2 takes wls_alpha
as a double, so a side that rounds at another place misses the short-run bars."""
import numpy as np
import pytest
import ref64
import synth
from test_ref64_oracle import (KM_MARGIN, SIZES, _km_blobs, _km_few, _ulp_close, check_kmeans, check_knn, check_level_stages, check_s1_at_the_cap,
                               check_s1_short_iterations)

PARAM_SETS = {"help": dict(eps=0.60, nonlocal_weight=0.4, local_weight=0.001, wls_lambda_init=0.0234375, wls_alpha=1.2),
              "strong": dict(eps=0.05, nonlocal_weight=5.0, local_weight=0.7, wls_lambda_init=0.1, wls_alpha=2.0),
              "soft": dict(eps=2.5, nonlocal_weight=0.3, local_weight=0.03, wls_lambda_init=0.005, wls_alpha=0.8)}
SET_NAMES = sorted(PARAM_SETS)

# (H, W, h, w, label grid, samples, layer[, "flat"]) as in tests/test_gpu_color.py: two upsampled levels, the finest layer at equal size (the x4 of S2's lambda,
# S1's cap of 50), hub-heavy flat images
LEVEL_CASES = [(48, 48, 12, 12, (3, 3), 4, 2), (40, 56, 20, 28, (5, 7), 4, 3), (64, 64, 64, 64, (4, 4), 16, 4, "flat"), (96, 96, 48, 48, (3, 3), 16, 3, "flat")]


def _orc_case(case):
    return tuple(case[:7]) + (len(case) > 7,)


@pytest.mark.parametrize("hw", SIZES)
def test_local_stats(oracle, hw):
    h, w = hw
    for mk in (synth.image, synth.image_flat):
        s, g = oracle.bgr2lab(mk(1, h, w)), oracle.bgr2lab(mk(2, h, w))
        for name in SET_NAMES:
            eps = PARAM_SETS[name]["eps"]
            ga, gb = oracle.local_stats(s, g, eps)
            ea, eb = ref64.local_stats(s, g, eps)
            assert _ulp_close(ga, ea, 2) and _ulp_close(gb, eb, 2), (mk.__name__, name)


@pytest.mark.parametrize("name", SET_NAMES)
@pytest.mark.parametrize("case", LEVEL_CASES)
def test_s1_short_iterations(oracle, case, name):
    print("s1-short", name, case[:4], "worst / bar %.3g" % check_s1_short_iterations(oracle, _orc_case(case), PARAM_SETS[name]))


@pytest.mark.parametrize("name", SET_NAMES)
@pytest.mark.parametrize("case", LEVEL_CASES)
def test_s1_at_the_cap_descends_like_the_literal_cg(oracle, case, name):
    print("s1-cap", name, case[:4], "ratio %.4f .. %.4f" % check_s1_at_the_cap(oracle, _orc_case(case), PARAM_SETS[name]))


@pytest.mark.parametrize("name", SET_NAMES)
@pytest.mark.parametrize("case", LEVEL_CASES)
def test_level_stages_vs_ref64(oracle, case, name):
    st, frac = check_level_stages(oracle, _orc_case(case), PARAM_SETS[name])
    assert 0 < max(st["wls_iters"]) < 5000
    print("level", name, case[:4], "S2 worst / allowed %.3g" % frac, "wls_iters", max(st["wls_iters"]))


# ---------------------------------------------------------------- C1 at other cluster counts
# K = 11 and 16 lie beyond the two K <= 10 dispatch edges of k_cluster.hip (the staged candidate rows of k_km_init, k_km_dist512); blobs40: 16 blobs, a donor move
# at K = 11 and 16; few70: 12 distinct vectors, so K = 16 finds fewer centres than K and leaves one label. Seed 1 throughout: every margin is at least 1e-5
KM_INPUTS = {"synth16": lambda: synth.features(3, 512, 16, 16) * np.float32(5.0), "c64_9x11": lambda: synth.features(1, 64, 9, 11),
             "blobs40": lambda: _km_blobs(1, 512, 40, 40, 16, 0.05), "few70": lambda: _km_few(4, 512, 70, 70, 12, 0.9)}
KM_KS = (1, 2, 9, 11, 16)


def km_expect(name, K):
    """what a case must reach besides its labels: the one-label exit, or a donor move"""
    if K == 1 or (name == "few70" and K == 16):
        return "one"
    return "donor" if name == "blobs40" and K in (11, 16) else None


@pytest.mark.parametrize("K", KM_KS)
@pytest.mark.parametrize("name", sorted(KM_INPUTS))
def test_kmeans_labels_vs_ref64(oracle, name, K):
    m = check_kmeans(oracle.cluster_features, oracle.feat_normalize, KM_INPUTS[name](), 1, km_expect(name, K), K=K)
    assert m >= KM_MARGIN
    print("kmeans", name, K, "margin %.3g" % m)


# ---------------------------------------------------------------- K1 with 1, 11 and 16 labels
# the sort key of k_cluster.hip reserves 4 bits for the cluster: labels 10 .. 15 are sorted, started and searched only here
KNN_SIZES = [(32, 32, 16, 16, 2), (64, 60, 16, 15, 4), (120, 110, 15, 14, 8)]
KNN_LABELS = (1, 11, 16)


def knn_case(size, nl, seed=9):
    """-> (image, label grid): labels (3x + 7y) mod nl — with nl >= 11 a cell's four neighbours carry four other labels, so an inner cell is in 5 clusters"""
    h, w, lh, lw, samples = size
    yy, xx = np.mgrid[0:lh, 0:lw]
    return synth.image_flat(seed, h, w), ((3 * xx + 7 * yy) % nl).astype(np.int32)


@pytest.mark.parametrize("nl", KNN_LABELS)
@pytest.mark.parametrize("size", KNN_SIZES)
def test_knn_graph_vs_ref64(oracle, size, nl):
    img, labels = knn_case(size, nl)
    assert int(labels.max()) == nl - 1
    lab = oracle.bgr2lab(img)
    gi, gw = oracle.knn_graph(lab, labels, nl, size[4])
    pad, dev = check_knn(gi, gw, *ref64.knn_graph(lab, labels, nl, size[4]), f"{size} {nl} labels")
    print("knn", size, nl, "padded", pad, "max rel dev %.3g" % dev)
