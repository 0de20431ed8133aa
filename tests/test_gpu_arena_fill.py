"""Results do not depend on what the arena's reused blocks held.

Every device buffer of a context comes from nct_ctx::alloc, which clears nothing and hands out blocks larger than asked for; a kernel that reads a word it has not
written is invisible on a fresh context (new memory reads as zero: 0 * w, + 0, a zero count) and on the session context (finite, plausibly scaled leftovers). With
NCT_ARENA_FILL=<byte> every block is filled before it is handed out. Each test here runs one call on a context without the hook (the clean run, computed once per
case and shared by the fill bytes) and the identical call on a context created with the hook, and asserts every output and every downloadable intermediate equal
bit pattern for bit pattern (NaNs the clean run produces: by position), iteration counts included. The clean results are pinned to the oracle and to tests/ref64.py by
the other GPU tests, so no reference is computed here.

Fill bytes: 0xFF — every float, double and half is a NaN (mask-by-multiplication, a stray addend); 0xFE — a float is -1.7e38, a double -5e303, finite: it wins
every minimum search that a NaN would lose (PatchMatch bests, k-means distances, kNN candidates, the error extremes); 0x7F — the same for maximum searches; 0x00 once,
as the control that the hook by itself changes nothing. A filled WLS solve gets NCT_WLS_MAXIT = the clean run's largest iteration count + 8, which only bounds the
time of a failure: the counts are compared anyway, and "did not converge" under fill is a failure with that message."""
import numpy as np
import pytest

import nct
import synth

pytestmark = pytest.mark.gpu

FILLS = [0xFF, 0xFE, 0x7F]
FILL_IDS = ["0xFF", "0xFE", "0x7F"]
HOOKS = ("NCT_ARENA_FILL", "NCT_WLS_MAXIT", "NCT_S2_LINES", "NCT_KNN_RUNS", "NCT_CONV_POOL_FUSE", "NCT_CONV_PAIR", "NCT_S1_MAXIT", "NCT_WLS_FORECAST", "NCT_WLS_RTOL",
         "NCT_S1_HUB_HINT")
TIMING_KEYS = ("wls_iters", "pm_level_launches")          # of a "timing" dict: what is a result, not a clock


# ---------------------------------------------------------------- comparison
def _same_array(a, b):
    """equal bit patterns; float NaNs by position (a payload is not a result: x86 and gfx950 already differ in it)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        na, nb = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))
    return bool(np.array_equal(a, b))


def _differences(clean, got, path, out):
    if isinstance(clean, dict):
        assert isinstance(got, dict) and clean.keys() == got.keys(), path
        for k in clean:
            if k == "timing":
                for t in TIMING_KEYS:
                    if list(clean[k][t]) != list(got[k][t]):
                        out.append("%s.timing.%s: %s -> %s" % (path, t, list(clean[k][t]), list(got[k][t])))
            else:
                _differences(clean[k], got[k], "%s.%s" % (path, k), out)
    elif isinstance(clean, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(clean) == len(got), path
        for i, (x, y) in enumerate(zip(clean, got)):
            _differences(x, y, "%s[%d]" % (path, i), out)
    elif isinstance(clean, np.ndarray):
        if not _same_array(clean, got):
            g = np.ascontiguousarray(got)
            bad = int((np.ascontiguousarray(clean).reshape(-1).view(np.uint8) != g.reshape(-1).view(np.uint8)).sum()) if g.shape == clean.shape and g.dtype == clean.dtype else -1
            out.append("%s: %s %s differs (%d bytes; %d NaN clean, %d NaN filled)" % (path, clean.dtype, clean.shape, bad,
                       int(np.isnan(clean).sum()) if clean.dtype.kind == "f" else 0, int(np.isnan(g).sum()) if g.dtype.kind == "f" else 0))
    elif isinstance(clean, Exception):
        if not (type(clean) is type(got) and str(clean) == str(got)):
            out.append("%s: %r -> %r" % (path, clean, got))
    elif clean is None or isinstance(clean, (int, float, str, np.integer, np.floating)):
        if not (clean is None and got is None) and not (clean == got):
            out.append("%s: %r -> %r" % (path, clean, got))
    else:
        raise TypeError("%s: no comparison for %s" % (path, type(clean)))


def _wls_iters(res, found):
    """every S2 iteration count inside a result: the "wls_iters" arrays of colour stages and of timing dicts"""
    if isinstance(res, dict):
        for k, v in res.items():
            if k == "wls_iters":
                found.extend(int(x) for x in np.asarray(v).reshape(-1))
            else:
                _wls_iters(v, found)
    elif isinstance(res, (list, tuple)):
        for v in res:
            _wls_iters(v, found)
    return found


_CLEAN = {}
_INPUTS = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_results():
    yield
    _CLEAN.clear(); _INPUTS.clear()


def _set_env(monkeypatch, env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)


def clean_run(monkeypatch, key, op, env=()):
    """op(context) on a context without the hook, once per key"""
    if key not in _CLEAN:
        _set_env(monkeypatch, env)
        with nct.Context(0) as c:
            _CLEAN[key] = op(c)
    return _CLEAN[key]


def filled_context(monkeypatch, fill, clean, env=()):
    _set_env(monkeypatch, env)
    monkeypatch.setenv("NCT_ARENA_FILL", str(fill))
    its = _wls_iters(clean, [])
    if its:
        monkeypatch.setenv("NCT_WLS_MAXIT", str(max(its) + 8))
    return nct.Context(0)


def check(monkeypatch, key, op, fill, env=()):
    """the pattern of every test: the clean run, the identical call under the fill, everything equal"""
    clean = clean_run(monkeypatch, key, op, env)
    with filled_context(monkeypatch, fill, clean, env) as c:
        got = op(c)
        assert c.counter(nct.CTR_ARENA_BYTES) > 0, "the filled call took nothing from the arena"
    diff = []
    _differences(clean, got, key, diff)
    assert not diff, "fill 0x%02X changes %d results:\n  %s" % (fill, len(diff), "\n  ".join(diff[:20]))
    return clean


def _try(f):
    """a call the library may refuse: the refusal is the result (and must be the same refusal under fill)"""
    try:
        return f()
    except nct.NctError as e:
        return e


fills = pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)


# ---------------------------------------------------------------- the hook itself
@pytest.mark.parametrize("fill", [0x00, 0x5A, 0xFF], ids=["0x00", "0x5A", "0xFF"])
def test_a_block_handed_out_holds_the_fill_byte(monkeypatch, fill):
    """the only thing that tells "nothing depends on the arena" from "the hook is dead": a block from dev_alloc, downloaded untouched, is the fill byte in every
    requested position (the slack behind the request is not looked at) — a fresh block, and a block that comes back from the cache after it held other data"""
    _set_env(monkeypatch, [("NCT_ARENA_FILL", str(fill))])
    with nct.Context(0) as c:
        for n in (1, 255, 256, 4097, (1 << 20) + 3, 3 << 20):
            p = c.dev_alloc(n)
            assert np.all(c.dev_download(p, (n,), np.uint8) == fill), ("fresh", n)
            c.dev_free(p)
        other = np.uint8(fill ^ 0xA5)
        p = c.dev_upload(np.full(70000, other, np.uint8))
        assert np.all(c.dev_download(p, (70000,), np.uint8) == other)
        c.dev_free(p)
        for n in (70000, 40000):                                   # served by the cached block: the same size, and a smaller request (the block is larger than asked for)
            q = c.dev_alloc(n)
            assert q == p, "the arena was meant to reuse the cached block"
            assert np.all(c.dev_download(q, (n,), np.uint8) == fill), ("reused", n)
            c.dev_free(q)
        assert c.counter(nct.CTR_ARENA_BYTES) > 0
    _set_env(monkeypatch, [])
    with nct.Context(0) as c:                                      # off: a reused block keeps what it held
        p = c.dev_upload(np.full(70000, 0x3C, np.uint8))
        c.dev_free(p)
        q = c.dev_alloc(70000)
        assert q == p and np.all(c.dev_download(q, (70000,), np.uint8) == 0x3C)
        c.dev_free(q)


@pytest.mark.parametrize("value", ["-1", "256", "abc", "12x", ""])
def test_values_outside_the_range_leave_the_hook_off(monkeypatch, value):
    _set_env(monkeypatch, [("NCT_ARENA_FILL", value)])
    with nct.Context(0) as c:
        p = c.dev_upload(np.full(5000, 0x3C, np.uint8))
        c.dev_free(p)
        q = c.dev_alloc(5000)
        assert q == p and np.all(c.dev_download(q, (5000,), np.uint8) == 0x3C)
        c.dev_free(q)


# ---------------------------------------------------------------- colour stage
# from COLOR_CASES of test_gpu_vs_ref64.py: upsampled; equal size (the x4 branch); hub blocks; elongated; and 372 x 368 for the forms of >= 100 000 pixels
COLOR = {"40x56_up": (40, 56, 20, 28, (5, 7), 4, 3), "32x32_equal": (32, 32, 32, 32, (2, 2), 16, 4), "96x96_flat_hubs": (96, 96, 48, 48, (3, 3), 16, 3, "flat"),
         "34x800_elongated": (34, 800, 17, 400, (2, 20), 4, 3), "372x368_large_tiles": (372, 368, 372, 368, (23, 23), 16, 4)}
COLOR_RUNS = [(k, ()) for k in COLOR] + [(k, (("NCT_S2_LINES", "0"),)) for k in ("34x800_elongated", "372x368_large_tiles")]


def _color_inputs(monkeypatch, name):
    """test_gpu_vs_ref64._case's inputs, with the library's own (clean) resize, Lab conversion and kNN graph — each pinned elsewhere"""
    if name not in _INPUTS:
        case = COLOR[name]
        H, W, h, w, grid, samples, layer = case[:7]
        seed, mk = 20 + layer, (synth.image_flat if len(case) > 7 else synth.image)
        full = mk(seed, H, W)
        _set_env(monkeypatch, [])
        with nct.Context(0) as c:
            s = c.resize_u8c3(full, h, w) if (h, w) != (H, W) else full
            g = c.resize_u8c3(mk(seed + 1, H, W), h, w)
            lh, lw = grid
            labels = (np.arange(lh * lw).reshape(lh, lw) % 3).astype(np.int32)
            ids, ws = c.knn_graph(c.bgr2lab(s), labels, 3, samples)
        err = -np.random.default_rng(seed).random((h, w)).astype(np.float32)
        _INPUTS[name] = (err, s, g, full, ids, ws, layer)
    return _INPUTS[name]


@fills
@pytest.mark.parametrize("name,env", COLOR_RUNS, ids=[k + ("_nolines" if e else "") for k, e in COLOR_RUNS])
def test_color_stage(monkeypatch, name, env, fill):
    """local_color_transfer(want_stages=True): ab_local, ab_nonlocal, ab_up, roughness, ab_wls, cg_iters, wls_iters and the image"""
    err, s, g, full, ids, ws, layer = _color_inputs(monkeypatch, name)
    clean = check(monkeypatch, "color/%s/%s" % (name, env), lambda c: c.local_color_transfer(err, s, g, full, ids, ws, layer, want_stages=True), fill, env)
    assert set(clean[1]) == {"ab_local", "ab_nonlocal", "ab_up", "roughness", "ab_wls", "cg_iters", "wls_iters"} and max(clean[1]["wls_iters"]) > 0
    if "flat" in name:
        assert np.bincount(ids.reshape(-1), minlength=ids.shape[0]).max() > 3 * 64, "the flat case is meant to have in-edge lists of several blocks"


def test_color_stage_control_fill_zero(monkeypatch):
    """0x00 on one seam: the hook by itself (the device-wide waits, the memset) changes nothing"""
    err, s, g, full, ids, ws, layer = _color_inputs(monkeypatch, "40x56_up")
    check(monkeypatch, "color/40x56_up/()", lambda c: c.local_color_transfer(err, s, g, full, ids, ws, layer, want_stages=True), 0x00)


@fills
@pytest.mark.parametrize("flags", [0, nct.FLAG_LATENCY], ids=["flags0", "latency"])
@pytest.mark.parametrize("case", [1, 3])
def test_color_finish(monkeypatch, case, flags, fill):
    """SEAM_CASES[1] and [3] of test_gpu_fullres.py (case 3: a 210 x 16 level, coarse grids of width 1), as one 6-wide solve and as the split 3 + 3 solve"""
    from fullres_ref import smooth_ab
    from test_gpu_fullres import SEAM_CASES
    (h, w), (wh, ww), (H, W) = SEAM_CASES[case]
    ab = smooth_ab(100 + case, h, w)
    s_full = synth.image(200 + case, H, W)
    prm = nct.Params.default(); prm.flags = flags
    check(monkeypatch, "finish/%d/%d" % (case, flags), lambda c: c.color_finish(ab, h, w, wh, ww, s_full, prm, want_stages=True), fill)


# ---------------------------------------------------------------- correspondence
def _normalized(monkeypatch, key, f):
    if key not in _INPUTS:
        _set_env(monkeypatch, [])
        with nct.Context(0) as c:
            _INPUTS[key] = c.feat_normalize(f)
    return _INPUTS[key]


@fills
@pytest.mark.parametrize("row", [0, 1, 3, 5, 6], ids=["C64", "C512", "C128", "C8", "C64_6x5_3x4"])
def test_patchmatch(monkeypatch, row, fill):
    from test_gpu_correspondence import PM_CASES
    C_, ah, aw, bh, bw, iters, rs = PM_CASES[row]
    a = _normalized(monkeypatch, ("pm_a", row), synth.features(10 + C_, C_, ah, aw))
    b = _normalized(monkeypatch, ("pm_b", row), synth.features(20 + C_, C_, bh, bw))

    def op(c):
        return c.patchmatch(a, b, c.nnf_init(ah, aw, bh, bw), iters=iters, rs_max=rs, seed=1234)
    nnf, d = check(monkeypatch, "patchmatch/%d" % row, op, fill)
    assert np.isfinite(d).all()


def _bidir(fa, fb, rs, seed):
    def op(c):
        c.pm_bench_setup(fa, fb)
        # mode 2 (fp16 candidate tiles) exists for C = 64 .. 512; where the library refuses it, the refusal is the result
        return [_try(lambda: c.pm_bench_run_bidir(iters=5, rs_max=rs, seed=seed, pm_mode=mode, count=True, fetch=True, both=True)[1:]) for mode in (0, 1, 2)]
    return op


@fills
@pytest.mark.parametrize("case", [(64, 37, 41, 33, 45, 8), (256, 21, 24, 23, 20, 8), (24, 20, 22, 21, 19, 8)], ids=["C64", "C256", "C24"])
def test_patchmatch_bidir(monkeypatch, case, fill):
    """the pipeline's form (both fields per launch), plain, with the row rejection and with fp16 tiles: fields, distances and the evaluation counters"""
    C_, ah, aw, bh, bw, rs = case
    clean = check(monkeypatch, "bidir/%d" % C_, _bidir(synth.features(21, C_, ah, aw), synth.features(22, C_, bh, bw), rs, 77), fill)
    assert not isinstance(clean[0], Exception) and not isinstance(clean[1], Exception)
    assert isinstance(clean[2], Exception) == (C_ == 24)


@fills
def test_patchmatch_dead_feature_pixels(monkeypatch, fill):
    """test_gpu_correspondence.test_patchmatch_dead_feature_pixels' maps at C = 64: the normalised maps hold NaN vectors of their own, next to which a stray word would hide"""
    C_, ah, aw, bh, bw, rs = 64, 37, 41, 33, 45, 8
    fa, fb = synth.features(31, C_, ah, aw), synth.features(32, C_, bh, bw)
    fa[:, 5:9, 7:12] = 0; fa[:, ah - 1, aw - 1] = 0; fb[:, 3:8, 2:6] = 0; fb[:, 0, 0] = 0; fb[:, bh // 2, bw // 2] = 0
    clean = check(monkeypatch, "bidir/dead", _bidir(fa, fb, rs, 91), fill)
    annd = clean[1][2]
    assert np.isnan(annd).any() and np.isfinite(annd).any()


@fills
@pytest.mark.parametrize("case", [0, 4], ids=["C64", "C24"])
def test_bds_vote_features(monkeypatch, case, fill):
    from test_gpu_correspondence import VOTE_CASES
    C_, ah, aw, bh, bw = VOTE_CASES[case]
    pin = synth.features(50 + C_, C_, bh, bw) * np.float32(37.0)
    ann, bnn = synth.random_nnf(1, ah, aw, bh, bw), synth.random_nnf(2, bh, bw, ah, aw)
    collapsed = bnn.copy()
    collapsed[:, : bw // 2] = (np.uint32(ah // 2) << 12) | np.uint32(aw // 2)          # long source lists: the block sums of k_vote_hub
    check(monkeypatch, "vote/%d" % case, lambda c: [c.bds_vote_features(ann, q, pin, 1.0, wc, want_pw=True) for q in (bnn, collapsed) for wc in (2.0, 0.0, 8.0)], fill)


@fills
def test_bds_vote_image(monkeypatch, fill):
    ah, aw, bh, bw = 7, 5, 9, 11
    a, b = synth.image(1, ah, aw), synth.image(2, bh, bw)
    ann, bnn = synth.random_nnf(3, ah, aw, bh, bw), synth.random_nnf(4, bh, bw, ah, aw)
    check(monkeypatch, "vote_image", lambda c: [c.bds_vote_image(a, b, ann, bnn, 1.0, wc) for wc in (2.0, 0.0, 8.0)], fill)


@fills
def test_normalize_distance_upsample(monkeypatch, fill):
    ahh, awh, ah, aw, bh, bw = 29, 43, 57, 85, 75, 120
    fa, fb = synth.features(40, 64, ahh, awh), synth.features(41, 64, ahh, awh)
    dead = fa.copy(); dead[:, 2, 3] = 0
    half = synth.random_nnf(5, ahh, awh, (bh + 1) // 2, (bw + 1) // 2)

    def op(c):
        a, resp = c.feat_normalize(fa, want_resp=True)
        b = c.feat_normalize(fb)
        return [a, resp, b, c.feat_normalize(dead, want_resp=True), c.feature_distance(a, b), c.nnf_upsample(half, ah, aw, bh, bw), c.nnf_init(ah, aw, bh, bw)]
    check(monkeypatch, "feat", op, fill)


# ---------------------------------------------------------------- clustering
def _few_distinct(shape, distinct):
    C_, h, w = shape
    rng = np.random.default_rng(17)
    protos = (rng.random((distinct, C_), dtype=np.float32) + np.float32(0.05)) * np.float32(3.0)
    return np.ascontiguousarray(protos[rng.integers(0, distinct, size=h * w)].T.reshape(C_, h, w))


@fills
@pytest.mark.parametrize("name", ["512x44x44", "512x44x44_4_distinct"])
def test_cluster_features(monkeypatch, name, fill):
    """one test_kmeans_labels_exact shape (the pipeline's: C = 512 from LDS, the member-list centres) and one map with fewer distinct vectors than K would like (hundreds
    of duplicate rejections, the full shuffle)"""
    f = synth.features(3, 512, 44, 44) * np.float32(5.0) if name == "512x44x44" else _few_distinct((512, 44, 44), 4)
    check(monkeypatch, "kmeans/" + name, lambda c: [c.cluster_features(f, 10, 11, seed) for seed in (1, 99)], fill)


@fills
@pytest.mark.parametrize("runs", ["0", "1"])
def test_knn_graph(monkeypatch, runs, fill):
    """the 64 x 60 flat case of test_knn_graph_both_search_forms, every entry for itself and one search per run"""
    h, w, lh, lw, samples = 64, 60, 16, 15, 4
    img = synth.image_flat(9, h, w)
    img[h // 2:h // 2 + 3, : w // 2] = (255, 0, 255)
    img[0, 0] = (0, 255, 0)
    labels = (np.arange(lh * lw).reshape(lh, lw) % 4).astype(np.int32)
    if "knn_lab" not in _INPUTS:
        _set_env(monkeypatch, [])
        with nct.Context(0) as c:
            _INPUTS["knn_lab"] = c.bgr2lab(img)
    lab = _INPUTS["knn_lab"]
    check(monkeypatch, "knn/" + runs, lambda c: c.knn_graph(lab, labels, 4, samples), fill, (("NCT_KNN_RUNS", runs),))


# ---------------------------------------------------------------- VGG
@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@fills
@pytest.mark.parametrize("fuse", ["0", "1"])
def test_vgg19_features(monkeypatch, weights, fuse, fill):
    """an odd size of test_vgg19_features_bit_exact, the pool as a pass of its own and inside the conv epilogue"""
    img = synth.image(7, 70, 45)

    def op(c):
        c.vgg19_load_raw(*weights)
        return [c.vgg19_features(img, 5), c.vgg19_features(img, 2)]
    check(monkeypatch, "vgg/" + fuse, op, fill, (("NCT_CONV_POOL_FUSE", fuse),))


@fills
def test_conv3x3_padded_input_channel(monkeypatch, fill):
    """nct_conv3x3_relu at Cin = 3 on a 17 x 23 map: the kernel consumes channels in pairs, the fourth plane's packed weights are 0 — and 0 * NaN is not"""
    cin, cout, H, W = 3, 64, 17, 23
    rng = np.random.default_rng(cin * 1000 + W)
    x = rng.standard_normal((cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2 / (9 * cin))).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    out = check(monkeypatch, "conv3", lambda c: [c.conv3x3_relu(x, w, b, relu) for relu in (True, False)], fill)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()


@fills
def test_conv3x3_paired_launch(monkeypatch, fill):
    """PAIR_CASES[0] of test_gpu_conv_forms.py (one launch for two images), planar and channel-last maps of both"""
    from test_gpu_conv_forms import PAIR_CASES, PAIR_OUTPUTS, pair_dev, pair_is_one_launch
    case = PAIR_CASES[0]
    assert pair_is_one_launch(case[0][1], case[1], case[2])
    check(monkeypatch, "conv_pair", lambda c: pair_dev(c, case, True, PAIR_OUTPUTS["both"]), fill)


# ---------------------------------------------------------------- whole calls (synthetic weights; SRC, REF of test_gpu_seq_mc.py)
SRC, REF = (1000, 64, 56), (1001, 48, 64)


def _pair_levels(weights, src, ref, flags):
    def op(c):
        c.vgg19_load_raw(*weights)
        prm = nct.Params.default(); prm.levels = 5; prm.flags = flags
        c.pair_upload(src, ref)
        lv = c.pair_run_levels(src.shape, ref.shape, prm, want_color=True)
        return lv, c.pair_download()
    return op


@fills
@pytest.mark.parametrize("flags", [0, nct.FLAG_LATENCY, nct.FLAG_FEAT16], ids=["flags0", "latency", "feat16"])
def test_pair_levels(monkeypatch, weights, flags, fill):
    """every level's NNFs, distances, guide, error, colour stages (with both solvers' iteration counts), result, and the labels"""
    src, ref = synth.image(*SRC), synth.image(*REF)
    lv, out = check(monkeypatch, "pair/%d" % flags, _pair_levels(weights, src, ref, flags), fill)
    assert np.array_equal(out, lv["result"][4]) and len(lv["color"]) == 5 and min(lv["timing"]["wls_iters"]) > 0


@fills
def test_multi_levels(monkeypatch, weights, fill):
    """K = 2: per reference the fields, G_k and E_k, per level the labels and the merged maps"""
    src, refs = synth.image(*SRC), [synth.image(*REF), synth.image(1002, 72, 50)]

    def op(c):
        c.vgg19_load_raw(*weights)
        c.multi_upload(src, refs)
        lv = c.multi_run_levels()
        return lv, c.pair_download()
    lv, out = check(monkeypatch, "multi", op, fill)
    assert np.array_equal(out, lv["result"][4]) and len(lv["ann"]) == 2


@fills
def test_sequence_with_motion_and_a_propagated_frame(monkeypatch, weights, fill):
    """three frames with motion compensation on: a first frame, a blended frame, a propagated frame (the kept state X', L, the packed maps and the fields live in the
    arena from frame to frame)"""
    import seq_ref
    ref = synth.image(*REF)
    frames = seq_ref.pan_frames(3, SRC[1], SRC[2], step=2)

    def op(c):
        c.vgg19_load_raw(*weights)
        c.seq_begin(ref, frames[0].shape)
        try:
            c.seq_set_motion()
            res = [c.seq_frame_levels(frames[0]), c.seq_frame_levels(frames[1]), c.seq_frame_propagate_levels(frames[2])]
        finally:
            c.seq_end()
        return res
    clean = check(monkeypatch, "seq", op, fill)
    assert clean[1][1]["motion"][4].any(), "the pan is meant to give the blended frame a field"
    assert not np.array_equal(clean[2][0], clean[1][0])


@fills
def test_pair_fullres(monkeypatch, weights, fill):
    """the 300 x 220 case of test_gpu_fullres.py at max_side 128: the originals shrunk in the arena, the last level finished on the original source"""
    src0, ref0 = synth.image(31, 300, 220), synth.image(32, 260, 200)

    def op(c):
        c.vgg19_load_raw(*weights)
        out, tm = c.process_pair_fullres(src0, ref0, 128, want_timing=True)
        return {"out": out, "timing": tm}
    clean = check(monkeypatch, "fullres", op, fill)
    assert clean["out"].shape == src0.shape and clean["timing"]["wls_iters"][4] > 0


def test_arena_history_on_one_context(monkeypatch, weights):
    """one filled context (0xFF), shrinking sizes — the order in which oversized reused blocks are most common: the 5-level pair at 96 x 80, then at 64 x 56, then a
    colour seam. Each result equals the result of a clean context that ran only that call."""
    big = (synth.image(1000, 96, 80), synth.image(1001, 72, 104))
    small = (synth.image(*SRC), synth.image(*REF))
    err, s, g, full, ids, ws, layer = _color_inputs(monkeypatch, "40x56_up")
    ops = [("pair/96x80", _pair_levels(weights, big[0], big[1], 0)), ("pair/0", _pair_levels(weights, small[0], small[1], 0)),
           ("color/40x56_up/()", lambda c: c.local_color_transfer(err, s, g, full, ids, ws, layer, want_stages=True))]
    cleans = [clean_run(monkeypatch, key, op) for key, op in ops]
    with filled_context(monkeypatch, 0xFF, cleans) as c:
        before = 0
        for (key, op), clean in zip(ops, cleans):
            got = op(c)
            diff = []
            _differences(clean, got, key, diff)
            assert not diff, "after %d bytes of arena history, fill 0xFF changes:\n  %s" % (before, "\n  ".join(diff[:20]))
            before = c.counter(nct.CTR_ARENA_BYTES)
            assert before > 0
