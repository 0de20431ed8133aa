"""Source region masks (SPEC §6.11) on the GPU: the three kernels alone (host and device-pointer forms) and the whole masked pair level by level against
tests/region_ref.py, the identities of rule 4, several references, full resolution, tables, refusals and the CLI's -mask. Every comparison is equality of bytes or
bit patterns."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import nct
import region_ref
import synth
from fullres_ref import oracle_finish, working_size

pytestmark = pytest.mark.gpu
BIN = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")
SH, SW, RH, RW = 56, 64, 48, 60


def _params(levels=5, flags=0):
    p = nct.Params.default()
    p.levels, p.flags = levels, flags
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def gpu(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


@pytest.fixture(scope="module")
def images():
    return synth.image(1000, SH, SW), synth.image(1001, RH, RW)


@pytest.fixture(scope="module")
def refs(oracle, weights, images):
    """the CPU references, computed once: the masked pair with the half-plane and the ramp"""
    src, ref = images
    return {kind: region_ref.pair(oracle, src, region_ref.mask(kind, SH, SW), ref, *weights) for kind in ("half", "ramp")}


# ---- 1. the resize seam
@pytest.mark.parametrize("shape, dst", region_ref.RESIZE_SHAPES + [((272, 272), (17, 17))])
def test_resize_u8c1(gpu, oracle, shape, dst):
    for kind in region_ref.MASK_KINDS:
        m = region_ref.mask(kind, *shape)
        exp = region_ref.resize_u8c1(oracle, m, *dst)
        assert np.array_equal(gpu.resize_u8c1(m, *dst), exp), (kind, "host")
        assert np.array_equal(gpu.resize_u8c1_dev(m, *dst), exp), (kind, "dev")
    assert np.array_equal(gpu.resize_u8c1(m, *shape), m)          # equal sizes: a copy


# ---- 2. the mix
@pytest.mark.parametrize("shape", region_ref.MIX_SHAPES)
def test_region_mix(gpu, shape):
    for kind in region_ref.MASK_KINDS:
        for nans in (False, True):
            x, m = region_ref.mix_case(*shape, kind)
            if nans:
                x, m = region_ref.with_nans(x, m)
            exp = _bits(region_ref.mix(x, m))
            assert np.array_equal(_bits(gpu.region_mix(x, m)), exp), (kind, nans, "host")
            assert np.array_equal(_bits(gpu.region_mix_dev(x, m)), exp), (kind, nans, "dev")
            assert np.array_equal(_bits(gpu.region_mix_dev(x, m, in_place=True)), exp), (kind, nans, "in place")


# ---- 3. the compose
def test_region_compose(gpu, oracle):
    s, lab_s, lab_o, m = region_ref.compose_case(oracle, 61, 47)
    shares = region_ref.compose_shares(lab_s, lab_o, m)
    assert min(shares) >= 0.01, shares
    for flags, form in ((0, 0), (nct.FLAG_LAB2BGR_CUBE, 1)):
        for protect in (0, 1):
            exp = region_ref.compose(oracle, s, lab_o, m, protect, form)
            assert np.array_equal(gpu.region_compose(s, lab_o, m, protect, _params(flags=flags)), exp), (form, protect, "host")
            assert np.array_equal(gpu.region_compose_dev(s, lab_o, m, protect, _params(flags=flags)), exp), (form, protect, "dev")
    one = gpu.region_compose(s[:1, :1], lab_o[:1, :1], m[:1, :1])
    assert np.array_equal(one, region_ref.compose(oracle, s[:1, :1], lab_o[:1, :1], m[:1, :1], 0, 0))


# ---- 4. the whole pair, level by level
@pytest.mark.parametrize("kind", ["half", "ramp"])
def test_masked_pair_level_by_level(gpu, oracle, images, refs, kind):
    src, ref = images
    m = region_ref.mask(kind, SH, SW)
    exp_out, exp = refs[kind]
    gpu.pair_upload(src, ref)
    gpu.pair_set_region(m)
    keep = gpu.pair_run_region_levels(src.shape, ref.shape, _params(5))
    got = gpu.pair_download()
    mp = region_ref.mask_pyramid(oracle, m)
    for l in range(5):
        assert np.array_equal(keep["mask"][l], mp[l]), l
        own = keep["color"][l]["ab_nonlocal"]
        assert np.array_equal(_bits(keep["ab_mix"][l]), _bits(region_ref.mix(own, keep["mask"][l]))), l
        assert np.array_equal(_bits(own), _bits(exp["ab_nonlocal"][l])), l
        assert np.array_equal(keep["ann"][l], exp["ann"][0][l]) and np.array_equal(keep["bnn"][l], exp["bnn"][0][l]), l
        assert np.array_equal(keep["guide"][l], exp["guide"][l]), l
        assert np.array_equal(keep["err"][l].view(np.uint32), exp["err"][l].view(np.uint32)), l
        assert np.array_equal(keep["result"][l], exp["result"][l]), (l, int((keep["result"][l] != exp["result"][l]).sum()))
    assert np.array_equal(got, exp_out)
    assert np.array_equal(gpu.process_pair_region(src, m, ref), exp_out)


# ---- 5. identities on the device
def test_identities(gpu, images):
    src, ref = images
    plain, tm0 = gpu.process_pair(src, ref, want_timing=True)
    for protect in (0, 1):
        assert np.array_equal(gpu.process_pair_region(src, region_ref.mask("full", SH, SW), ref, protect), plain)
        for levels in (1, 5):
            assert np.array_equal(gpu.process_pair_region(src, region_ref.mask("empty", SH, SW), ref, protect, _params(levels)), src), (protect, levels)
    out, tm1 = gpu.process_pair_region(src, None, ref, want_timing=True)
    assert np.array_equal(out, plain) and tm1["pm_level_launches"] == tm0["pm_level_launches"]
    # the mask goes with the upload: a masked pair, then a plain one on the same context
    assert not np.array_equal(gpu.process_pair_region(src, region_ref.mask("half", SH, SW), ref), plain)
    assert np.array_equal(gpu.process_pair(src, ref), plain)
    # … and nct_pair_set_region(NULL) removes it without a new upload
    gpu.pair_upload(src, ref)
    gpu.pair_set_region(region_ref.mask("half", SH, SW))
    gpu.pair_set_region(None)
    gpu.pair_run()
    assert np.array_equal(gpu.pair_download(), plain)


def test_no_mask_leaves_the_arena_as_it_was(weights, images):
    src, ref = images
    held = []
    for region in (False, True):
        with nct.Context(0) as c:
            c.vgg19_load_raw(*weights)
            out = c.process_pair_region(src, None, ref) if region else c.process_pair(src, ref)
            held.append((c.counter(nct.CTR_ARENA_BYTES), out))
    assert held[0][0] == held[1][0] and np.array_equal(held[0][1], held[1][1])


# ---- 6. several references
def test_several_references(gpu, oracle, weights, images, refs):
    src, ref = images
    ref2 = synth.image(1002, 40, 52)
    m = region_ref.mask("ramp", SH, SW)
    exp, keep = region_ref.run(oracle, src, m, [ref, ref2], *weights)
    gpu.multi_upload(src, [ref, ref2])
    gpu.pair_set_region(m)
    got = gpu.multi_run_levels(_params(5))
    for l in range(5):
        assert np.array_equal(got["label"][l], keep["label"][l]), l
        assert np.array_equal(got["result"][l], keep["result"][l]), l
    assert np.array_equal(gpu.pair_download(), exp)
    assert len(np.unique(keep["label"][4])) == 2, "one reference took every pixel: the case does not exercise the merge"
    gpu.multi_upload(src, [ref])
    gpu.pair_set_region(m)
    gpu.multi_run()
    assert np.array_equal(gpu.pair_download(), refs["ramp"][0])


# ---- 7. full resolution
def test_fullres_region(gpu, oracle, weights):
    src0, ref0 = synth.image(1010, 112, 128), synth.image(1011, 48, 60)
    m0 = region_ref.mask("ramp", 112, 128)
    wh, ww = working_size(112, 128, 64)
    assert (wh, ww) == (56, 64)
    for protect in (0, 1):
        got = gpu.process_pair_fullres_region(src0, m0, ref0, 64, protect)
        # the GPU's own working-size levels, then the finish at the original size from the oracle's stages and the compose with M0
        S, M = gpu.resize_u8c3(src0, wh, ww), gpu.resize_u8c1(m0, wh, ww)
        assert np.array_equal(M, region_ref.resize_u8c1(oracle, m0, wh, ww))
        gpu.pair_upload(S, ref0)
        gpu.pair_set_region(M, protect)
        keep = gpu.pair_run_region_levels(S.shape, ref0.shape, _params(5))
        h, w = keep["dims"][4][:2]
        _, fin = oracle_finish(oracle, keep["ab_mix"][4], h, w, wh, ww, src0)
        exp = region_ref.compose(oracle, src0, fin["lab"], m0, protect, 0)
        assert got.shape == src0.shape and np.array_equal(got, exp), (protect, int((got != exp).sum()))
    # the table of a full-resolution masked run uses M0
    got = gpu.process_pair_fullres_region(src0, m0, ref0, 64, 1)
    lut = gpu.pair_fit_lut(9)
    assert np.array_equal(lut.view(np.uint32), gpu.lut_fit_masked(src0, got, m0, 9).view(np.uint32))
    # a source that is not shrunk gives the masked pair
    small, ms = synth.image(1000, SH, SW), region_ref.mask("half", SH, SW)
    assert np.array_equal(gpu.process_pair_fullres_region(small, ms, ref0, 64), gpu.process_pair_region(small, ms, ref0))
    assert np.array_equal(gpu.process_pair_fullres_region(src0, None, ref0, 64), gpu.process_pair_fullres(src0, ref0, 64))


def test_upsampling_finish_with_a_mask_is_refused(weights):
    src0, ref0 = synth.image(1010, 112, 128), synth.image(1011, 48, 60)
    with nct.Context(0) as c:
        c.vgg19_load_raw(*weights)
        before = c.counter(nct.CTR_ARENA_BYTES)
        with pytest.raises(nct.NctError) as e:
            c.process_pair_fullres_region(src0, region_ref.mask("half", 112, 128), ref0, 64, finish=nct.FINISH_UPSAMPLE)
        assert e.value.code == -2 and "mask" in str(e.value) and "NCT_FINISH_UPSAMPLE" in str(e.value)
        assert c.counter(nct.CTR_ARENA_BYTES) == before
        c.set_finish_guided(10.0)
        with pytest.raises(nct.NctError) as e:
            c.process_pair_fullres_region(src0, region_ref.mask("half", 112, 128), ref0, 64, finish=nct.FINISH_UPSAMPLE)
        assert e.value.code == -2 and c.counter(nct.CTR_ARENA_BYTES) == before
        # without a mask the upsampling finish runs as it did
        assert c.process_pair_fullres_region(src0, None, ref0, 64, finish=nct.FINISH_UPSAMPLE).shape == src0.shape


# ---- 8. tables
@pytest.mark.parametrize("N", [9, 17])
def test_lut_fit_masked(gpu, N):
    rng = np.random.default_rng(N)
    src = rng.integers(0, 256, (4096, 3), dtype=np.uint8)
    res = np.clip(src.astype(int) + rng.integers(-20, 21, src.shape), 0, 255).astype(np.uint8)
    for kind in ("half", "ramp", "random", "full"):
        m = region_ref.mask(kind, 64, 64).reshape(-1)
        k = region_ref.kept(m)
        exp, est = gpu.lut_fit(src[k], res[k], N, want_stages=True)
        for fit in (gpu.lut_fit_masked, gpu.lut_fit_masked_dev):
            got, st = fit(src, res, m, N, want_stages=True)
            assert np.array_equal(st["weight"], est["weight"]) and np.array_equal(st["resid"], est["resid"]), (kind, fit.__name__)
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (kind, fit.__name__)
    assert np.array_equal(gpu.lut_fit_masked(src, res, None, N).view(np.uint32), gpu.lut_fit(src, res, N).view(np.uint32))
    for fit in (gpu.lut_fit_masked, gpu.lut_fit_masked_dev):
        with pytest.raises(nct.NctError) as e:
            fit(src, res, np.full(4096, 127, np.uint8), N)
        assert e.value.code == -2 and "mask" in str(e.value)


def test_pair_fit_lut_after_a_masked_pair(gpu, images):
    src, ref = images
    m = region_ref.mask("half", SH, SW)
    out = gpu.process_pair_region(src, m, ref)
    assert np.array_equal(gpu.pair_fit_lut(9).view(np.uint32), gpu.lut_fit_masked(src, out, m, 9).view(np.uint32))
    gpu.process_pair_region(src, region_ref.mask("empty", SH, SW), ref, None, _params(1))
    with pytest.raises(nct.NctError) as e:
        gpu.pair_fit_lut(9)
    assert e.value.code == -2 and "mask" in str(e.value)


# ---- 9. refusals and state
def test_refusals_and_state(gpu, images):
    src, ref = images
    m = region_ref.mask("half", SH, SW)
    gpu.seq_begin(ref, src.shape)
    try:
        with pytest.raises(nct.NctError) as e:
            gpu._chk(gpu._l.nct_pair_set_region(gpu._h, m.ctypes.data, None))
        assert e.value.code == -5 and "sequence" in str(e.value)
        with pytest.raises(nct.NctError) as e:
            gpu.process_pair_region(src, m, ref)
        assert e.value.code == -5
    finally:
        gpu.seq_end()
    with pytest.raises(nct.NctError) as e:                          # nothing uploaded since the sequence closed
        gpu._chk(gpu._l.nct_pair_set_region(gpu._h, m.ctypes.data, None))
    assert e.value.code == -5
    for call in (lambda: gpu.process_pair_region(src, m[:-1], ref), lambda: gpu.process_pair_region(src, m.T.copy(), ref),
                 lambda: gpu.process_pair_fullres_region(src, m[:, :-1], ref, 64)):
        with pytest.raises(nct.NctError) as e:
            call()
        assert e.value.code == -2 and "mask" in str(e.value)
    gpu.pair_upload(src, ref)
    with pytest.raises(nct.NctError) as e:
        gpu.pair_set_region(m[:-1])
    assert e.value.code == -2 and "mask" in str(e.value)
    prm, rg = _params(1), nct.RegionParams.default()
    out = np.empty_like(src)
    import ctypes as C
    rc = gpu._l.nct_process_pair_region(gpu._h, None, SH, SW, m.ctypes.data, ref.ctypes.data, RH, RW, C.addressof(rg), C.addressof(prm), out.ctypes.data, None)
    assert rc == -2 and b"null" in gpu._l.nct_last_error(gpu._h)
    for protect in (-1, 2):
        for call in (lambda: gpu.process_pair_region(src, m, ref, protect), lambda: gpu.pair_set_region(m, protect),
                     lambda: gpu.process_pair_fullres_region(src, m, ref, 64, protect), lambda: gpu.region_compose(src, src, m, protect)):
            with pytest.raises(nct.NctError) as e:
                call()
            assert e.value.code == -2 and "protect" in str(e.value), protect
    with pytest.raises(nct.NctError) as e:                          # region levels without a mask
        gpu.pair_run_region_levels(src.shape, ref.shape, _params(1))
    assert e.value.code == -5
    with pytest.raises(nct.NctError) as e:
        gpu.region_mix(np.zeros((2, 0, 3)), np.zeros((0, 5), np.uint8))
    assert e.value.code == -2


# ---- 10. the CLI
def test_cli_mask(tmp_path, gpu, weights):
    from caffemodel_io import write_caffemodel
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), *weights)
    inp, masks = tmp_path / "in", tmp_path / "masks"
    inp.mkdir(); masks.mkdir()
    imgs = {n: synth.image(2000 + i, 40 + 8 * i, 56) for i, n in enumerate(("a", "b", "c", "r"))}
    for n, im in imgs.items():
        Image.fromarray(im[..., ::-1].copy()).save(inp / (n + ".png"))
    ma = region_ref.mask("ramp", *imgs["a"].shape[:2])
    Image.fromarray(ma, "L").save(masks / "a.png")
    Image.fromarray(region_ref.mask("half", 30, 30), "L").save(masks / "c.png")        # not c's size
    (inp / "pairs.txt").write_text("a.png r.png 2.0\nb.png r.png 2.0\nc.png r.png 2.0\n")
    base = [BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-levels", "1"]

    def run(tag, *extra):
        r = subprocess.run(base + ["-o", str(tmp_path / tag), *extra], capture_output=True, text=True)
        pngs = sorted(n for n in os.listdir(tmp_path / tag) if n.endswith(".png"))
        return r, {n: np.asarray(Image.open(tmp_path / tag / n).convert("RGB"))[..., ::-1] for n in pngs}
    prm = _params(1)
    prm.bds_weight = 2.0
    for protect in (0, 1):
        r, files = run("masked%d" % protect, "-mask", str(masks), "-maskprotect", str(protect))
        assert sorted(files) == ["a_r_2.00.png", "b_r_2.00.png"], r.stdout + r.stderr
        assert "-mask" in r.stdout and "30 x 30" in r.stdout            # the wrong-size mask refuses its line, and the run goes on
        assert np.array_equal(files["a_r_2.00.png"], gpu.process_pair_region(imgs["a"], ma, imgs["r"], protect, prm))
        assert np.array_equal(files["b_r_2.00.png"], gpu.process_pair(imgs["b"], imgs["r"], prm))
    r1, plain1 = run("plain1", "-maskprotect", "0")
    r2, plain2 = run("plain2")
    assert r1.returncode == 0 and r2.returncode == 0, r1.stdout + r2.stdout
    assert sorted(plain1) == sorted(plain2) == ["a_r_2.00.png", "b_r_2.00.png", "c_r_2.00.png"]
    for n in plain2:
        assert np.array_equal(plain1[n], plain2[n]), n
    assert np.array_equal(plain2["a_r_2.00.png"], gpu.process_pair(imgs["a"], imgs["r"], prm))
    assert not np.array_equal(plain2["a_r_2.00.png"], files["a_r_2.00.png"])
