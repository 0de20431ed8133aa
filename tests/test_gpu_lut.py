"""3D colour look-up tables on the GPU (SPEC §6.6) against the numpy reference tests/lut_ref.py: the splat's integer sums, the displacement field and the fp32 table of
the fit, and the apply, all compared on bit patterns; nct_pair_fit_lut, the device-pointer forms, every refusal, the arena fill hook and the CLI's -lut flags."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "neural-color-transfer_amd", "python"))
import lut_ref
import nct
import synth

pytestmark = pytest.mark.gpu
CLI = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def pixels(kind, npix):
    """source and result pixels [npix, 3]: random, one constant colour, colours on node planes (f = 0 or 255 in every channel), and random ones mixed with the value 255"""
    rng = np.random.default_rng(1000 + npix)
    o = rng.integers(0, 256, (npix, 3)).astype(np.uint8)
    if kind == "random":
        s = rng.integers(0, 256, (npix, 3)).astype(np.uint8)
    elif kind == "constant":
        s = np.tile(np.array([[37, 201, 118]], np.uint8), (npix, 1))
    elif kind == "planes":                                   # N - 1 is a power of two, so only 0 lies on a node plane (f = 0) and only 255 in the clamped cell (f = 255):
        s = rng.choice(np.array([0, 255], np.uint8), (npix, 3))         # pixels made of these two have one non-zero corner weight, 255^3
    else:                                                    # "last": every channel 255 somewhere, elsewhere random
        s = rng.integers(0, 256, (npix, 3)).astype(np.uint8)
        s[rng.random((npix, 3)) < 0.5] = 255
    for a in (s, o):
        a.setflags(write=False)
    return s, o


@functools.lru_cache(maxsize=None)
def ref_splat(kind, npix, N):
    return lut_ref.splat(*pixels(kind, npix), N)


SPLAT_CASES = [(k, n, N) for k in ("random", "planes", "last") for n in (1, 7, 63, 64, 65, 37 * 70) for N in (3, 9, 17, 33)
               if (n in (1, 65, 37 * 70) or N == 17) or k == "random"] + [("constant", 64 * 64, N) for N in (3, 9, 17, 33)] + [("random", 37 * 70, 65), ("constant", 64 * 64, 65)]


@pytest.mark.parametrize("kind, npix, N", SPLAT_CASES)
def test_splat_equals_numpy(ctx, kind, npix, N):
    s, o = pixels(kind, npix)
    W, R = ref_splat(kind, npix, N)
    _, st = ctx.lut_fit(s, o, N, 1.0, want_stages=True)
    assert same(st["weight"], W) and same(st["resid"], R)
    assert int(st["weight"].astype(object).sum()) == lut_ref.W3 * npix


@functools.lru_cache(maxsize=None)
def synthetic_pair():
    return synth.image(1000, 56, 64), synth.image(1001, 48, 64)


@pytest.fixture(scope="module")
def pair_ctx():
    """a context that has run the 56 x 64 synthetic pair: (context, source, result)"""
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    src, ref = synthetic_pair()
    with nct.Context(0) as c:
        c.vgg19_load_raw(ws, bs)
        res = c.process_pair(src, ref)
        res.setflags(write=False)
        yield c, src, res


def sparse_pair():
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, (5, 3)).astype(np.uint8), rng.integers(0, 256, (5, 3)).astype(np.uint8)


_fit_cache = {}


def ref_fit(name, s, o, N, lam):
    key = (name, N, lam)
    if key not in _fit_cache:
        _fit_cache[key] = lut_ref.fit(s, o, N, lam)
    return _fit_cache[key]


@pytest.mark.parametrize("N", [5, 17, 33])
@pytest.mark.parametrize("name", ["synthetic", "sparse", "same"])
def test_fit_equals_numpy(pair_ctx, name, N):
    """the displacement field after the SPEC's fixed number of cycles and the fp32 table, bit for bit: one workgroup runs the whole solve at N <= 9, launches per
    operation carry the 17^3 and 33^3 levels"""
    c, src, res = pair_ctx
    s, o = {"synthetic": (src, res), "sparse": sparse_pair(), "same": (src, src)}[name]
    lam = 1.0 if name != "sparse" else 0.1
    lut, W, R, D = ref_fit(name, s, o, N, lam)
    got, st = c.lut_fit(s, o, N, lam, want_stages=True)
    assert same(st["weight"], W) and same(st["resid"], R)
    assert same(st["disp"], D), "max |D - reference| = %g" % np.abs(st["disp"] - D).max()
    assert same(got.reshape(-1, 3), lut)
    if name == "same":
        assert same(got.reshape(-1, 3), lut_ref.identity(N))


@pytest.mark.parametrize("N", [17, 33])
def test_fit_at_the_default_lambda_equals_numpy(pair_ctx, N):
    """the synthetic pair at nct_lut_params_default's lambda (0.1): with so small a smoothness weight the mass term dominates the data-rich coarse rows, so the
    smoother's divisor takes its l1 branch there"""
    c, src, res = pair_ctx
    lam = nct.LutParams.default().lambda_
    assert lam == 0.1
    lut, W, R, D = ref_fit("synthetic", src, res, N, lam)
    got, st = c.lut_fit(src, res, N, lam, want_stages=True)
    assert same(st["disp"], D), "max |D - reference| = %g" % np.abs(st["disp"] - D).max()
    assert same(got.reshape(-1, 3), lut)


def test_fit_at_65_equals_numpy(ctx):
    """three levels above the one-workgroup part of the hierarchy"""
    s, o = sparse_pair()
    lut, W, R, D = ref_fit("sparse", s, o, 65, 1.0)
    got, st = ctx.lut_fit(s, o, 65, 1.0, want_stages=True)
    assert same(st["disp"], D) and same(got.reshape(-1, 3), lut)


@functools.lru_cache(maxsize=None)
def random_table(N):
    t = (np.random.default_rng(N).random((N, N, N, 3)) * 400.0 - 70.0).astype(np.float32)        # reaches outside [0, 255]: the cast saturates
    t.setflags(write=False)
    return t


@pytest.mark.parametrize("N", [3, 17, 33, 65])
@pytest.mark.parametrize("npix", [1, 63, 64, 65, 4097])
def test_apply_equals_numpy(ctx, N, npix):
    px = pixels("last", npix)[0]
    exp = lut_ref.apply(random_table(N), N, px)
    assert exp.min() == 0 and exp.max() == 255 or npix < 63
    assert same(ctx.lut_apply(random_table(N), px), exp)
    assert same(ctx.lut_apply_dev(random_table(N), px), exp)
    assert same(ctx.lut_apply(lut_ref.identity(N).reshape(N, N, N, 3), px), px)


def test_apply_in_place_and_unaligned_dev_pointers(ctx):
    """the _dev form over its own input, and on pointers that are not 4-byte aligned (the byte path of the packed loads and stores)"""
    N, npix = 17, 1001
    px = pixels("random", npix)[0]
    exp = lut_ref.apply(random_table(N), N, px)
    assert same(ctx.lut_apply_dev(random_table(N), px, in_place=True), exp)
    t, buf, out = ctx.dev_upload(random_table(N)), ctx.dev_upload(np.concatenate([np.zeros(1, np.uint8), px.reshape(-1)])), ctx.dev_alloc(3 * npix + 3)
    try:
        ctx.dev_call("lut_apply", t, N, buf + 1, npix, out + 3)
        assert same(ctx.dev_download(out, (3 * npix + 3,), np.uint8)[3:].reshape(-1, 3), exp)
    finally:
        ctx.synchronize()
        for p in (t, buf, out):
            ctx.dev_free(p)


def test_pair_fit_lut_and_dev_forms(pair_ctx):
    c, src, res = pair_ctx
    for N, lam in ((17, 1.0), (33, 3.0)):
        host, st = c.lut_fit(src, res, N, lam, want_stages=True)
        assert same(c.pair_fit_lut(N, lam), host)
        dev, dst = c.lut_fit_dev(src, res, N, lam, want_stages=True)
        assert same(dev, host) and all(same(dst[k], st[k]) for k in st)
        assert same(c.lut_fit_dev(src, res, N, lam), host)
    assert same(c.pair_fit_lut(), c.lut_fit(src, res))                  # the defaults: size 33, nct_lut_params_default's lambda
    assert c.pair_fit_lut().shape == (33, 33, 33, 3)


def test_pair_fit_lut_after_a_full_resolution_run(pair_ctx):
    """after nct_process_pair_fullres the table comes from the original source and the full-resolution result"""
    c, _, _ = pair_ctx
    src0 = c.resize_u8c3(synth.image(61, 60, 40), 150, 100)
    ref = synthetic_pair()[1]
    res0 = c.process_pair_fullres(src0, ref, 64)
    assert res0.shape == src0.shape
    assert same(c.pair_fit_lut(9, 1.0), c.lut_fit(src0, res0, 9, 1.0))
    res = c.process_pair(*synthetic_pair())                              # a plain pair afterwards: its own images again
    assert same(c.pair_fit_lut(9, 1.0), c.lut_fit(synthetic_pair()[0], res, 9, 1.0))


def test_pair_fit_lut_follows_a_rerun_after_a_full_resolution_run(pair_ctx):
    """nct_pair_run on the working-size pair a full-resolution run left resident: the table is that run's, no longer the full-resolution one's"""
    c, _, _ = pair_ctx
    src0 = c.resize_u8c3(synth.image(61, 60, 40), 150, 100)
    c.process_pair_fullres(src0, synthetic_pair()[1], 64)
    wh, ww = nct.working_size(150, 100, 64)
    c.pair_run()
    c._pair_shape = (wh, ww, 3)
    res = c.pair_download()
    assert same(c.pair_fit_lut(9, 1.0), c.lut_fit(c.resize_u8c3(src0, wh, ww), res, 9, 1.0))


def test_pair_fit_lut_after_several_references(pair_ctx):
    c, src, _ = pair_ctx
    res = c.process_multi(src, [synthetic_pair()[1], synth.image(1003, 40, 52)])
    assert same(c.pair_fit_lut(9, 1.0), c.lut_fit(src, res, 9, 1.0))


def refused(call, code, *words):
    with pytest.raises(nct.NctError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(ctx):
    import ctypes as C
    s, o = pixels("random", 64)
    with nct.Context(0) as fresh:                                        # a context of its own: the shared one may have run a pair
        refused(lambda: fresh.pair_fit_lut(17, 1.0), -5, "pair_fit_lut", "no finished run")
        fresh.lut_fit(s, o, 5, 1.0)
        refused(lambda: fresh.pair_fit_lut(17, 1.0), -5, "pair_fit_lut", "no finished run")      # a fit is not a run
    for N in (0, 2, 4, 16, 32, 64, 129, -3):
        refused(lambda: ctx.lut_fit(s, o, N, 1.0), -2, "lut_fit", "size")
        refused(lambda: ctx.lut_apply(np.zeros((max(N, 1),) * 3 + (3,), np.float32), s), -2, "lut_apply", "size")
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: ctx.lut_fit(s, o, 17, lam), -2, "lut_fit", "lambda")
        refused(lambda: ctx.lut_fit_dev(s, o, 17, lam), -2, "lut_fit_dev", "lambda")
    prm = nct.LutParams.default()
    lut = np.zeros((33, 33, 33, 3), np.float32)
    L = ctx._l
    for args in ((None, o.ctypes.data, 64, C.addressof(prm), lut.ctypes.data, None), (s.ctypes.data, None, 64, C.addressof(prm), lut.ctypes.data, None),
                 (s.ctypes.data, o.ctypes.data, 64, None, lut.ctypes.data, None), (s.ctypes.data, o.ctypes.data, 64, C.addressof(prm), None, None)):
        for fn in (L.nct_lut_fit, L.nct_lut_fit_dev):
            refused(lambda: ctx._chk(fn(ctx._h, *args)), -2, "null pointer")
    for fn in (L.nct_lut_fit, L.nct_lut_fit_dev):
        for npix in (0, (1 << 26) + 1):
            refused(lambda: ctx._chk(fn(ctx._h, s.ctypes.data, o.ctypes.data, npix, C.addressof(prm), lut.ctypes.data, None)), -2, "pixels")
    for fn in (L.nct_lut_apply, L.nct_lut_apply_dev):
        for args in ((None, 33, s.ctypes.data, 64, o.ctypes.data), (lut.ctypes.data, 33, None, 64, o.ctypes.data), (lut.ctypes.data, 33, s.ctypes.data, 64, None)):
            refused(lambda: ctx._chk(fn(ctx._h, *args)), -2, "null pointer")
        for npix in (0, (1 << 26) + 1):
            refused(lambda: ctx._chk(fn(ctx._h, lut.ctypes.data, 33, s.ctypes.data, npix, lut.ctypes.data)), -2, "pixels")
    bad = lut_ref.identity(9).reshape(9, 9, 9, 3).copy()
    for v in (np.nan, np.inf, -np.inf):
        bad[4, 5, 6, 1] = v
        refused(lambda: ctx.lut_apply(bad, s), -2, "lut_apply", "non-finite")


def test_results_ignore_what_arena_blocks_held(monkeypatch):
    """the method of tests/test_gpu_arena_fill.py: the same fit and apply on a context whose arena fills every block with 0xFF before it hands it out"""
    s, o = pixels("random", 37 * 70)
    monkeypatch.delenv("NCT_ARENA_FILL", raising=False)
    with nct.Context(0) as c:
        clean = [c.lut_fit(s, o, N, 1.0, want_stages=True) for N in (17, 33)]
        clean_apply = [c.lut_apply(random_table(N), s) for N in (17, 33)]
    monkeypatch.setenv("NCT_ARENA_FILL", "255")
    with nct.Context(0) as c:
        probe = c.dev_alloc(4096)
        assert (c.dev_download(probe, (4096,), np.uint8) == 255).all(), "the fill hook is not active"
        c.dev_free(probe)
        for (lut, st), ap, N in zip(clean, clean_apply, (17, 33)):
            got, gst = c.lut_fit(s, o, N, 1.0, want_stages=True)
            assert same(got, lut) and all(same(gst[k], st[k]) for k in st)
            assert same(c.lut_apply(random_table(N), s), ap)
            assert same(c.lut_fit_dev(s, o, N, 1.0), lut)


def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=300)


def test_cli_writes_the_table_and_the_applied_original(tmp_path, pair_ctx):
    from caffemodel_io import synthetic_vgg19, write_caffemodel
    c, _, _ = pair_ctx
    ws, bs = synthetic_vgg19(19)
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    inp = tmp_path / "in"; inp.mkdir()
    a, b = synth.image(1, 72, 64), synth.image(2, 60, 80)
    Image.fromarray(a[..., ::-1].copy()).save(inp / "a.png"); Image.fromarray(b[..., ::-1].copy()).save(inp / "b.png")
    (inp / "pairs.txt").write_text("a.png b.png 2.0\n")
    base = ["-m", str(tmp_path / "model"), "-i", str(inp), "-g", "0"]
    r = run_cli(*base, "-o", str(tmp_path / "plain"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "plain")) == ["a_b_2.00.png", "status.jsonl"]           # without -lut: the file set of before
    r = run_cli(*base, "-o", str(tmp_path / "lut"), "-lut", "17", "-lutlambda", "3", "-lutfull", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "lut")) == ["a_b_2.00.cube", "a_b_2.00.png", "a_b_2.00_lut.png", "status.jsonl"]
    res = np.ascontiguousarray(np.asarray(Image.open(tmp_path / "lut" / "a_b_2.00.png").convert("RGB"))[..., ::-1])
    assert same(res, np.ascontiguousarray(np.asarray(Image.open(tmp_path / "plain" / "a_b_2.00.png").convert("RGB"))[..., ::-1]))
    lut = c.lut_fit(a, res, 17, 3.0)
    N, vals = lut_ref.read_cube(str(tmp_path / "lut" / "a_b_2.00.cube"))
    assert N == 17 and same(vals, lut_ref.cube_values(lut.reshape(-1, 3)))
    full = np.ascontiguousarray(np.asarray(Image.open(tmp_path / "lut" / "a_b_2.00_lut.png").convert("RGB"))[..., ::-1])
    assert same(full, lut_ref.apply(lut, 17, a).reshape(a.shape))
    # -resume counts the table and the applied image as part of the job's output
    os.remove(tmp_path / "lut" / "a_b_2.00.cube")
    r = run_cli(*base, "-o", str(tmp_path / "lut"), "-lut", "17", "-lutlambda", "3", "-lutfull", "1", "-resume", "1")
    assert r.returncode == 0 and "Skipping" not in r.stdout and os.path.exists(tmp_path / "lut" / "a_b_2.00.cube")
    r = run_cli(*base, "-o", str(tmp_path / "lut"), "-lut", "17", "-lutlambda", "3", "-lutfull", "1", "-resume", "1")
    assert r.returncode == 0 and "Skipping (-resume)" in r.stdout
