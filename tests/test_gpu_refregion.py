"""Reference region masks (SPEC §6.12) on the GPU: the pull alone (host and device-pointer forms) against the numpy pull, the masked pair level by level against
tests/refregion_ref.py, the identities of rule 6, both masks together, two references, full resolution, the table, refusals, the CLI's -refmask and its -mask on a line of two references. Every comparison is
equality of bytes or bit patterns."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import nct
import refregion_ref
import region_ref
import synth

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
    """the CPU references, computed once: the pair with the half-plane and the ramp on the reference"""
    src, ref = images
    return {kind: refregion_ref.pair(oracle, src, None, ref, region_ref.mask(kind, RH, RW), *weights) for kind in ("half", "ramp")}


# ---- 1. the pull alone
@pytest.mark.parametrize("grid", refregion_ref.PULL_GRIDS)
def test_region_pull(gpu, grid):
    ah, aw, bh, bw = grid
    fields = [(refregion_ref.random_field(11, ah, aw, bh, bw), refregion_ref.random_field(12, bh, bw, ah, aw))]
    if grid == (56, 64, 48, 60):
        # every reference pixel on ONE source pixel — a list of 2 880 sources, far beyond 64 — in a corner and inside; and the list split over two adjacent targets
        ann = fields[0][0]
        fields += [(ann, refregion_ref.collapsed_field(bh, bw, [(0, 0)])), (ann, refregion_ref.collapsed_field(bh, bw, [(20, 31)])),
                   (ann, refregion_ref.collapsed_field(bh, bw, [(20, 31), (20, 32)]))]
    for f, (ann, bnn) in enumerate(fields):
        for kind in region_ref.MASK_KINDS:
            q = region_ref.mask(kind, bh, bw)
            for bds in (2.0, 0.3):                                   # 0.3 is not a float: the weights are doubles
                exp = refregion_ref.pull(q, ann, bnn, 1.0, bds)
                assert np.array_equal(gpu.region_pull(q, ann, bnn, 1.0, bds), exp), (f, kind, bds, "host")
                assert np.array_equal(gpu.region_pull_dev(q, ann, bnn, 1.0, bds), exp), (f, kind, bds, "dev")
            if kind == "full":
                assert (exp == 255).all()
            if kind == "empty":
                assert (exp == 0).all()
    if len(fields) > 1:
        q = region_ref.mask("random", bh, bw)
        one = refregion_ref.pull(q, *fields[2])
        assert len(np.unique(one)) > 2 and not np.array_equal(one, refregion_ref.pull(q, *fields[0])), "the collapsed list does not show in the result"


# ---- 2. the masked pair, level by level
@pytest.mark.parametrize("kind", ["half", "ramp"])
def test_masked_pair_level_by_level(gpu, images, refs, kind):
    src, ref = images
    q = region_ref.mask(kind, RH, RW)
    exp_out, exp = refs[kind]
    gpu.pair_upload(src, ref)
    gpu.pair_set_ref_region(0, q)
    got = gpu.multi_run_ref_region_levels(_params(5))
    for l in range(5):
        assert np.array_equal(got["ref_mask"][0][l], exp["ref_mask"][0][l]), l
        assert np.array_equal(got["ann"][0][l], exp["ann"][0][l]) and np.array_equal(got["bnn"][0][l], exp["bnn"][0][l]), l
        assert np.array_equal(got["pulled"][0][l], exp["pulled"][0][l]), (l, int((got["pulled"][0][l] != exp["pulled"][0][l]).sum()))
        assert np.array_equal(got["mask"][l], exp["mask"][l]) and np.array_equal(got["mask_full"][l], exp["mask_full"][l]), l
        assert np.array_equal(got["guide"][l], exp["guide"][l]), l
        assert np.array_equal(got["err"][l].view(np.uint32), exp["err"][l].view(np.uint32)), l
        assert np.array_equal(_bits(got["ab_mix"][l]), _bits(exp["ab_mix"][l])), l
        assert np.array_equal(got["result"][l], exp["result"][l]), (l, int((got["result"][l] != exp["result"][l]).sum()))
    assert np.array_equal(gpu.pair_download(), exp_out)
    assert np.array_equal(gpu.process_pair_ref_region(src, None, ref, q), exp_out)
    # the pipeline's pull (behind the votes, on their inversion) is the seam's
    assert np.array_equal(gpu.region_pull(got["ref_mask"][0][4], got["ann"][0][4], got["bnn"][0][4]), got["pulled"][0][4])


# ---- 3. identities on the device
def test_identities(gpu, images):
    src, ref = images
    plain, tm0 = gpu.process_pair(src, ref, want_timing=True)
    full, empty = region_ref.mask("full", RH, RW), region_ref.mask("empty", RH, RW)
    for protect in (0, 1):
        out, tm1 = gpu.process_pair_ref_region(src, None, ref, full, protect, want_timing=True)
        assert np.array_equal(out, plain) and tm1["pm_level_launches"] == tm0["pm_level_launches"]
        for levels in (1, 5):
            assert np.array_equal(gpu.process_pair_ref_region(src, None, ref, empty, protect, _params(levels)), src), (protect, levels)
    ms = region_ref.mask("ramp", SH, SW)
    assert np.array_equal(gpu.process_pair_ref_region(src, ms, ref, full), gpu.process_pair_region(src, ms, ref))
    out, tm1 = gpu.process_pair_ref_region(src, None, ref, None, want_timing=True)
    assert np.array_equal(out, plain) and tm1["pm_level_launches"] == tm0["pm_level_launches"]
    # the masks go with the upload: a masked pair, then a plain one on the same context
    assert not np.array_equal(gpu.process_pair_ref_region(src, None, ref, region_ref.mask("half", RH, RW)), plain)
    assert np.array_equal(gpu.process_pair(src, ref), plain)
    # … and nct_pair_set_ref_region(k, NULL) removes one without a new upload
    gpu.pair_upload(src, ref)
    gpu.pair_set_ref_region(0, region_ref.mask("half", RH, RW))
    gpu.pair_set_ref_region(0, None)
    gpu.pair_run()
    assert np.array_equal(gpu.pair_download(), plain)
    # several references, every mask 255: nct_process_multi's bytes
    ref2 = synth.image(1002, 40, 52)
    assert np.array_equal(gpu.process_multi_ref_region(src, None, [ref, ref2], [full, None]), gpu.process_multi(src, [ref, ref2]))


def test_no_mask_leaves_the_arena_as_it_was(weights, images):
    src, ref = images
    held = []
    for region in (False, True):
        with nct.Context(0) as c:
            c.vgg19_load_raw(*weights)
            out = c.process_pair_ref_region(src, None, ref, None) if region else c.process_pair(src, ref)
            held.append((c.counter(nct.CTR_ARENA_BYTES), out))
    assert held[0][0] == held[1][0] and np.array_equal(held[0][1], held[1][1])


# ---- 4. a source mask and a reference mask together
def test_source_and_reference_mask(gpu, oracle, weights, images):
    src, ref = images
    ms, q = region_ref.mask("ramp", SH, SW), region_ref.mask("half", RH, RW)
    for protect in (0, 1):
        exp_out, exp = refregion_ref.pair(oracle, src, ms, ref, q, *weights, protect=protect) if protect == 0 else (None, None)
        gpu.pair_upload(src, ref)
        gpu.pair_set_region(ms, 1 - protect)
        gpu.pair_set_ref_region(0, q, protect)                     # the last setter decides protect
        got = gpu.multi_run_ref_region_levels(_params(5))
        if protect == 0:
            for l in range(5):
                assert np.array_equal(got["mask"][l], exp["mask"][l]) and np.array_equal(got["mask"][l], np.minimum(got["pulled"][0][l], region_ref.mask_pyramid(oracle, ms)[l])), l
                assert np.array_equal(got["mask_full"][l], exp["mask_full"][l]), l
                assert np.array_equal(got["result"][l], exp["result"][l]), l
            assert np.array_equal(gpu.pair_download(), exp_out)
            assert np.array_equal(gpu.process_pair_ref_region(src, ms, ref, q, 0), exp_out)
        else:
            F = got["mask_full"][4]
            out = gpu.pair_download()
            assert (F == 0).any() and np.array_equal(out[F == 0], src[F == 0])


def test_both_report_forms_describe_one_masked_run(gpu, images):
    """with both masks set, nct_pair_run_region_levels reports the M_l and X' that nct_multi_run_ref_region_levels reports (whose values the test above pins to the oracle)"""
    src, ref = images
    gpu.pair_upload(src, ref)
    gpu.pair_set_region(region_ref.mask("ramp", SH, SW))
    gpu.pair_set_ref_region(0, region_ref.mask("half", RH, RW))
    a = gpu.pair_run_region_levels(src.shape, ref.shape, _params(5))
    out_a = gpu.pair_download()
    b = gpu.multi_run_ref_region_levels(_params(5))
    for l in range(5):
        assert np.array_equal(a["mask"][l], b["mask"][l]), l
        assert np.array_equal(_bits(a["ab_mix"][l]), _bits(b["ab_mix"][l])), l
    assert np.array_equal(out_a, gpu.pair_download())


def test_a_report_form_is_refused_without_its_own_mask(gpu, images):
    src, ref = images
    gpu.pair_upload(src, ref)
    gpu.pair_set_region(region_ref.mask("ramp", SH, SW))
    before = gpu.counter(nct.CTR_ARENA_BYTES)
    with pytest.raises(nct.NctError) as e:                          # a source mask only
        gpu.multi_run_ref_region_levels(_params(1))
    assert e.value.code == -5 and "reference mask" in str(e.value)
    assert gpu.counter(nct.CTR_ARENA_BYTES) == before
    gpu.pair_upload(src, ref)                                       # drops the source mask
    gpu.pair_set_ref_region(0, region_ref.mask("half", RH, RW))
    before = gpu.counter(nct.CTR_ARENA_BYTES)
    with pytest.raises(nct.NctError) as e:                          # a reference mask only
        gpu.pair_run_region_levels(src.shape, ref.shape, _params(1))
    assert e.value.code == -5 and "region mask" in str(e.value)
    assert gpu.counter(nct.CTR_ARENA_BYTES) == before


# ---- 5. two references, the first masked
def test_two_references(gpu, oracle, weights, images):
    src, ref = images
    ref2 = synth.image(1002, 40, 52)
    q = region_ref.mask("half", RH, RW)
    exp_out, exp = refregion_ref.run(oracle, src, None, [ref, ref2], [q, None], *weights)
    gpu.multi_upload(src, [ref, ref2])
    gpu.pair_set_ref_region(0, q)
    got = gpu.multi_run_ref_region_levels(_params(5))
    for l in range(5):
        assert np.array_equal(got["label"][l], exp["label"][l]), l
        assert np.array_equal(got["pulled"][0][l], exp["pulled"][0][l]), l
        assert np.array_equal(got["mask"][l], exp["p"][l]) and np.array_equal(got["mask_full"][l], exp["mask_full"][l]), l
        assert np.array_equal(got["result"][l], exp["result"][l]), l
    assert np.array_equal(gpu.pair_download(), exp_out)
    lab = exp["label"][4]
    assert len(np.unique(lab)) == 2, "one reference took every pixel: the case does not exercise the merge"
    assert (exp["p"][4][lab == 1] == 255).all() and (exp["p"][4][lab == 0] < 255).any()
    assert np.array_equal(gpu.process_multi_ref_region(src, None, [ref, ref2], [q, None]), exp_out)


# ---- 6. full resolution
def test_fullres_ref_region(gpu, oracle, weights, images, refs):
    src0, ref0 = synth.image(1010, 112, 128), synth.image(1011, 96, 120)
    m0, q0 = region_ref.mask("ramp", 112, 128), region_ref.mask("half", 96, 120)
    exp, keep = refregion_ref.fullres_pair(oracle, src0, m0, ref0, q0, *weights, 64)
    assert keep["mask_full"][4].shape == (112, 128) and keep["p"][4].shape == (56, 64)
    got = gpu.process_pair_fullres_ref_region(src0, m0, ref0, q0, 64)
    assert got.shape == src0.shape and np.array_equal(got, exp), int((got != exp).sum())
    # the table of such a run uses the final F at the original size
    assert np.array_equal(gpu.pair_fit_lut(9).view(np.uint32), gpu.lut_fit_masked(src0, got, keep["mask_full"][4], 9).view(np.uint32))
    # a source that is not shrunk gives the masked pair
    src, ref = images
    assert np.array_equal(gpu.process_pair_fullres_ref_region(src, None, ref, region_ref.mask("half", RH, RW), 64), refs["half"][0])
    assert np.array_equal(gpu.process_pair_fullres_ref_region(src0, None, ref0, None, 64), gpu.process_pair_fullres(src0, ref0, 64))


# ---- 7. the table
def test_pair_fit_lut_after_a_masked_pair(gpu, images, refs):
    src, ref = images
    out = gpu.process_pair_ref_region(src, None, ref, region_ref.mask("half", RH, RW))
    F = refs["half"][1]["mask_full"][4]
    assert 0 < refregion_ref.fit_pixels(refs["half"][1]).sum() < F.size
    assert np.array_equal(gpu.pair_fit_lut(9).view(np.uint32), gpu.lut_fit_masked(src, out, F, 9).view(np.uint32))
    # the next, plain run's table is the plain one
    out = gpu.process_pair(src, ref)
    assert np.array_equal(gpu.pair_fit_lut(9).view(np.uint32), gpu.lut_fit(src, out, 9).view(np.uint32))


# ---- 8. refusals and state
def test_refusals_and_state(gpu, images):
    import ctypes as C
    src, ref = images
    q = region_ref.mask("half", RH, RW)
    gpu.seq_begin(ref, src.shape)
    try:
        with pytest.raises(nct.NctError) as e:
            gpu._chk(gpu._l.nct_pair_set_ref_region(gpu._h, 0, q.ctypes.data, None))
        assert e.value.code == -5 and "sequence" in str(e.value)
        with pytest.raises(nct.NctError) as e:
            gpu.process_pair_ref_region(src, None, ref, q)
        assert e.value.code == -5
    finally:
        gpu.seq_end()
    with pytest.raises(nct.NctError) as e:                          # nothing uploaded since the sequence closed
        gpu._chk(gpu._l.nct_pair_set_ref_region(gpu._h, 0, q.ctypes.data, None))
    assert e.value.code == -5
    gpu.pair_upload(src, ref)
    for k in (-1, 1):
        with pytest.raises(nct.NctError) as e:
            gpu.pair_set_ref_region(k, q)
        assert e.value.code == -2 and "k = %d" % k in str(e.value)
    for protect in (-1, 2):
        for call in (lambda: gpu.pair_set_ref_region(0, q, protect), lambda: gpu.process_pair_ref_region(src, None, ref, q, protect),
                     lambda: gpu.process_pair_fullres_ref_region(src, None, ref, q, 64, protect), lambda: gpu.process_multi_ref_region(src, None, [ref], [q], protect)):
            with pytest.raises(nct.NctError) as e:
                call()
            assert e.value.code == -2 and "protect" in str(e.value), protect
    gpu.pair_upload(src, ref)
    with pytest.raises(nct.NctError) as e:                          # levels without a reference mask
        gpu.multi_run_ref_region_levels(_params(1))
    assert e.value.code == -5 and "mask" in str(e.value)
    for call in (lambda: gpu.pair_set_ref_region(0, q[:-1]), lambda: gpu.process_pair_ref_region(src, None, ref, q.T.copy()),
                 lambda: gpu.process_pair_fullres_ref_region(src, None, ref, q[:, :-1], 64), lambda: gpu.process_multi_ref_region(src, None, [ref], [q, q])):
        with pytest.raises(nct.NctError) as e:
            call()
        assert e.value.code == -2 and "mask" in str(e.value)
    # the seam: null pointers and sides out of range, each named
    ann, bnn = refregion_ref.random_field(1, 4, 4, 3, 4), refregion_ref.random_field(2, 3, 4, 4, 4)
    qq, out = region_ref.mask("random", 3, 4), np.empty((4, 4), np.uint8)
    args = [qq.ctypes.data, 3, 4, ann.ctypes.data, bnn.ctypes.data, 4, 4, 1.0, 2.0, out.ctypes.data]
    for fn in (gpu._l.nct_region_pull, gpu._l.nct_region_pull_dev):
        for i, word in ((0, b"q_mask"), (3, b"ann"), (4, b"bnn"), (9, b"out")):
            bad = list(args); bad[i] = None
            assert fn(gpu._h, *bad) == -2 and word in gpu._l.nct_last_error(gpu._h), word
        for i, word, v in ((1, b"bh", 0), (2, b"bw", 4097), (5, b"ah", -1), (6, b"aw", 4097)):
            bad = list(args); bad[i] = v
            assert fn(gpu._h, *bad) == -2 and word in gpu._l.nct_last_error(gpu._h), word
    assert C.sizeof(nct.RefRegionLevels) == 8 * (2 * nct.MAX_REFS * 5 + 15)


# ---- 9. the CLI
def test_cli_refmask(tmp_path, gpu, weights):
    from caffemodel_io import write_caffemodel
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), *weights)
    inp, masks = tmp_path / "in", tmp_path / "refmasks"
    inp.mkdir(); masks.mkdir()
    imgs = {n: synth.image(2000 + i, 40 + 8 * i, 56) for i, n in enumerate(("a", "r", "s", "t"))}
    for n, im in imgs.items():
        Image.fromarray(im[..., ::-1].copy()).save(inp / (n + ".png"))
    qr = region_ref.mask("half", *imgs["r"].shape[:2])
    Image.fromarray(qr, "L").save(masks / "r.png")
    Image.fromarray(region_ref.mask("half", 30, 30), "L").save(masks / "t.png")        # not t's size
    (inp / "pairs.txt").write_text("a.png r.png 2.0\na.png s.png 2.0\na.png t.png 2.0\n")
    base = [BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-levels", "1"]

    def run(tag, *extra):
        r = subprocess.run(base + ["-o", str(tmp_path / tag), *extra], capture_output=True, text=True)
        pngs = sorted(n for n in os.listdir(tmp_path / tag) if n.endswith(".png"))
        return r, {n: np.asarray(Image.open(tmp_path / tag / n).convert("RGB"))[..., ::-1] for n in pngs}
    prm = _params(1)
    prm.bds_weight = 2.0
    r, files = run("masked", "-refmask", str(masks))
    assert sorted(files) == ["a_r_2.00.png", "a_s_2.00.png"], r.stdout + r.stderr
    assert "-refmask" in r.stdout and "30 x 30" in r.stdout            # the wrong-size mask refuses its line, and the run goes on
    assert np.array_equal(files["a_r_2.00.png"], gpu.process_pair_ref_region(imgs["a"], None, imgs["r"], qr, None, prm))
    assert np.array_equal(files["a_s_2.00.png"], gpu.process_pair(imgs["a"], imgs["s"], prm))
    assert not np.array_equal(files["a_r_2.00.png"], gpu.process_pair(imgs["a"], imgs["r"], prm))
    # -lut: the masked line's table is fitted over the last level's target mask (rule 7), the other line's over every pixel
    import lut_ref
    r, lfiles = run("lut", "-refmask", str(masks), "-lut", "9")
    assert np.array_equal(lfiles["a_r_2.00.png"], files["a_r_2.00.png"]), r.stdout + r.stderr
    same = lambda a, b: np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    gpu.process_pair_ref_region(imgs["a"], None, imgs["r"], qr, None, prm)
    N, vals = lut_ref.read_cube(str(tmp_path / "lut" / "a_r_2.00.cube"))
    assert N == 9 and same(vals, lut_ref.cube_values(gpu.pair_fit_lut(9).reshape(-1, 3)))
    N, vals = lut_ref.read_cube(str(tmp_path / "lut" / "a_s_2.00.cube"))
    assert N == 9 and same(vals, lut_ref.cube_values(gpu.lut_fit(imgs["a"], files["a_s_2.00.png"], 9).reshape(-1, 3)))
    # -vis 1 writes the run's own P_l per level, for a pair and for a comma line; -mask and -maskprotect combine
    ms = region_ref.mask("ramp", *imgs["a"].shape[:2])
    smasks = tmp_path / "masks"
    smasks.mkdir()
    Image.fromarray(ms, "L").save(smasks / "a.png")
    (inp / "pairs.txt").write_text("a.png r.png 2.0\na.png r.png,s.png 2.0\n")
    r, vfiles = run("vis", "-refmask", str(masks), "-mask", str(smasks), "-maskprotect", "1", "-vis", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    gpu.pair_upload(imgs["a"], imgs["r"])
    gpu.pair_set_region(ms, 1)
    gpu.pair_set_ref_region(0, qr)
    got = gpu.multi_run_ref_region_levels(prm)
    assert np.array_equal(vfiles["a_r_2.00.png"], gpu.pair_download())
    assert np.array_equal(vfiles["a_r_2.00_refmask_0.png"][..., 0], got["pulled"][0][0])
    gpu.multi_upload(imgs["a"], [imgs["r"], imgs["s"]])
    gpu.pair_set_region(ms, 1)
    gpu.pair_set_ref_region(0, qr)
    got = gpu.multi_run_ref_region_levels(prm)
    name = [n for n in vfiles if n.endswith("_refmask_0.png") and n != "a_r_2.00_refmask_0.png"]
    assert len(name) == 1, sorted(vfiles)
    assert np.array_equal(vfiles[name[0]][..., 0], np.where(got["label"][0] == 0, got["pulled"][0][0], 255))
    assert np.array_equal(vfiles[name[0].replace("_refmask_0", "")], gpu.pair_download())


def test_cli_refmask_fullres_shrinks_the_mask_with_its_image(tmp_path, gpu, weights):
    """-fullres 1 hands both masks over at the original sizes; without it the CLI shrinks a reference above the working size together with its mask"""
    from caffemodel_io import write_caffemodel
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), *weights)
    inp, masks = tmp_path / "in", tmp_path / "refmasks"
    inp.mkdir(); masks.mkdir()
    a, big = synth.image(2100, 40, 56), synth.image(2101, 36, 1040)              # the reference is wider than the CLI's working size of 1000
    for n, im in (("a", a), ("r", big)):
        Image.fromarray(im[..., ::-1].copy()).save(inp / (n + ".png"))
    q = region_ref.mask("half", 36, 1040)
    Image.fromarray(q, "L").save(masks / "r.png")
    (inp / "pairs.txt").write_text("a.png r.png 2.0\n")
    prm = _params(1)
    prm.bds_weight = 2.0
    for tag, extra in (("plain", []), ("full", ["-fullres", "1"])):
        r = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-levels", "1", "-o", str(tmp_path / tag), "-refmask", str(masks), *extra], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        out = np.asarray(Image.open(tmp_path / tag / "a_r_2.00.png").convert("RGB"))[..., ::-1]
        assert np.array_equal(out, gpu.process_pair_fullres_ref_region(a, None, big, q, 1000, None, prm)), tag


def test_cli_mask_with_two_references(tmp_path, gpu, weights):
    """-mask on a comma line: the bytes of nct_multi_upload + nct_pair_set_region + nct_multi_run + nct_pair_download"""
    from caffemodel_io import write_caffemodel
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), *weights)
    inp, masks = tmp_path / "in", tmp_path / "masks"
    inp.mkdir(); masks.mkdir()
    imgs = {n: synth.image(2000 + i, 40, 56) for i, n in enumerate(("a", "r", "s"))}
    for n, im in imgs.items():
        Image.fromarray(im[..., ::-1].copy()).save(inp / (n + ".png"))
    ms = region_ref.mask("ramp", 40, 56)
    Image.fromarray(ms, "L").save(masks / "a.png")
    (inp / "pairs.txt").write_text("a.png r.png,s.png 2.0\n")
    prm = _params(1)
    prm.bds_weight = 2.0
    outs = {}
    for tag, extra in (("masked", ["-mask", str(masks), "-maskprotect", "1"]), ("plain", [])):
        r = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-levels", "1", "-o", str(tmp_path / tag), *extra], capture_output=True, text=True)
        pngs = [n for n in os.listdir(tmp_path / tag) if n.endswith(".png")]
        assert r.returncode == 0 and len(pngs) == 1, r.stdout + r.stderr
        outs[tag] = np.asarray(Image.open(tmp_path / tag / pngs[0]).convert("RGB"))[..., ::-1]
    gpu.multi_upload(imgs["a"], [imgs["r"], imgs["s"]])
    gpu.pair_set_region(ms, 1)
    gpu.multi_run(prm)
    assert np.array_equal(outs["masked"], gpu.pair_download())
    assert np.array_equal(outs["plain"], gpu.process_multi(imgs["a"], [imgs["r"], imgs["s"]], prm))
    assert not np.array_equal(outs["masked"], outs["plain"])
