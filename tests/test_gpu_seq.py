"""Frame sequences (SPEC §6.3) on the GPU: the blend kernel against the numpy rule, whole sequences against the composition of the oracle's stages
(tests/seq_ref.py) frame by frame and level by level, the identities of rule 5, the refusals, what a context holds before and after a sequence, and the
console driver's -seq 1. All comparisons are equality of bytes / bit patterns."""
import os
import subprocess
import numpy as np
import pytest
from PIL import Image

import nct
import seq_ref
import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "neural-color-transfer_amd", "bin", "neural_color_transfer")


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- seam: nct_seq_blend / nct_seq_blend_dev against the numpy rule

def _check_blend(ctx, x, xp, lab, labp, tau, sigma):
    exp, etm = seq_ref.blend(x, xp, lab, labp, tau, sigma)
    got, tm = ctx.seq_blend(x, xp, lab, labp, tau, sigma)
    assert np.array_equal(bits(tm), bits(etm))
    assert np.array_equal(bits(got), bits(exp))
    dev, dtm = ctx.seq_blend_dev(x, xp, lab, labp, tau, sigma)
    assert np.array_equal(bits(dtm), bits(etm)) and np.array_equal(bits(dev), bits(exp))
    only, none = ctx.seq_blend(x, xp, lab, labp, tau, sigma, want_tau_map=False)         # without the tau_p map
    assert none is None and np.array_equal(bits(only), bits(exp))
    return etm


@pytest.mark.parametrize("grid,kind", seq_ref.BLEND_CASES + [((44, 44), "random"), ((175, 233), "nan_both")])
@pytest.mark.parametrize("tau,sigma", [(0.7, 10.0), (0.5, 4.0), (0.85, 0.75)])
def test_seq_blend_matches_the_numpy_rule(ctx, grid, kind, tau, sigma):
    x, xp, lab, labp = seq_ref.blend_case(grid[0], grid[1], 17 * grid[0] + grid[1], kind)
    etm = _check_blend(ctx, x, xp, lab, labp, tau, sigma)
    if kind == "equal":
        assert (etm == tau).all()


def test_seq_blend_on_a_700_level(ctx):
    x, xp, lab, labp = seq_ref.blend_case(700, 700, 7)
    etm = _check_blend(ctx, x, xp, lab, labp, 0.7, 10.0)
    assert 0 < etm.min() < 0.1 and etm.max() > 0.5             # the comparison covers both ends of the weight


# ---- whole sequences against the composition

SRC, REF = (1000, 64, 56), (1001, 48, 64)
PAN = (96, 80)                                                 # frames of the noisy pan
PAN_REF = (1001, 72, 100)


@pytest.mark.parametrize("levels", [5, 1])
def test_sequence_matches_the_composition_level_by_level(wctx, oracle, weights, levels):
    ws, bs = weights
    ref = synth.image(*PAN_REF)
    frames = seq_ref.pan_frames(3, *PAN)
    exp, keeps = seq_ref.sequence(oracle, frames, ref, ws, bs, levels=levels)
    # conditions on the expected side, before anything of the GPU's is looked at: later frames are blended, with weights that vary over the image
    assert all((k["tau_map"][levels - 1] > 0).all() and k["tau_map"][levels - 1].std() > 0 for k in keeps[1:])
    assert not keeps[0]["tau_map"][0].any()
    prm = nct.Params.default(); prm.levels = levels
    wctx.seq_begin(ref, frames[0].shape, prm)
    try:
        for t, f in enumerate(frames):
            out, lv = wctx.seq_frame_levels(f)
            for l in range(levels):
                assert np.array_equal(bits(lv["color"][l]["ab_nonlocal"]), bits(keeps[t]["ab_nonlocal"][l])), ("ab_nonlocal", t, l)
                assert np.array_equal(bits(lv["tau_map"][l]), bits(keeps[t]["tau_map"][l])), ("tau_map", t, l)
                assert np.array_equal(bits(lv["ab_blend"][l]), bits(keeps[t]["ab_blend"][l])), ("ab_blend", t, l)
                assert np.array_equal(lv["result"][l], keeps[t]["result"][l]), ("result", t, l)
            assert np.array_equal(out, exp[t]), t
            assert lv["timing"]["color_ms"] > 0
    finally:
        wctx.seq_end()
    # the plain entry point gives the same frames
    wctx.seq_begin(ref, frames[0].shape, prm)
    try:
        for t, f in enumerate(frames):
            assert np.array_equal(wctx.seq_frame(f), exp[t]), t
    finally:
        wctx.seq_end()


# ---- identities (rule 5)

@pytest.mark.parametrize("levels", [5, 1])
def test_first_frames_and_tau_zero_are_process_pair(wctx, levels):
    ref = synth.image(*PAN_REF)
    frames = seq_ref.pan_frames(3, *PAN)
    prm = nct.Params.default(); prm.levels = levels
    pairs = [wctx.process_pair(f, ref, prm, want_timing=True) for f in frames]
    try:
        wctx.seq_begin(ref, frames[0].shape, prm)
        outs = [wctx.seq_frame(f) for f in frames]
        assert np.array_equal(outs[0], pairs[0][0])                                          # (a) frame 0
        assert not np.array_equal(outs[1], pairs[1][0]) and not np.array_equal(outs[2], pairs[2][0])
        wctx.seq_reset()
        assert np.array_equal(wctx.seq_frame(frames[2]), pairs[2][0])                        # (a) the first frame after a reset
        wctx.seq_begin(ref, frames[0].shape, prm, tau=0.0)                                   # (b); begin on an open sequence replaces it
        for f, (exp, tp) in zip(frames, pairs):
            got, tm = wctx.seq_frame(f, want_timing=True)
            assert np.array_equal(got, exp)
            assert tm["pm_level_launches"] == tp["pm_level_launches"]
    finally:
        wctx.seq_end()


def test_identical_frames_and_two_contexts(wctx, weights):
    src, ref = synth.image(*SRC), synth.image(*REF)
    frames = seq_ref.static_frames(3, SRC[1], SRC[2])
    try:
        wctx.seq_begin(ref, src.shape, tau=0.9, sigma=3.0)
        same = [wctx.seq_frame(src) for _ in range(3)]
        assert np.array_equal(same[1], same[0]) and np.array_equal(same[2], same[0])        # (c)
        wctx.seq_begin(ref, src.shape)
        a = [wctx.seq_frame(f) for f in frames]
    finally:
        wctx.seq_end()
    with nct.Context(0) as c:                                                                # (d) the same sequence on another context
        c.vgg19_load_raw(*weights)
        c.seq_begin(ref, src.shape)
        b = [c.seq_frame(f) for f in frames]
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert not np.array_equal(b[1], c.seq_frame(frames[1]))                              # a frame's result depends on what came before it


# ---- what a context holds

# NCT_CTR_ARENA_BYTES of a fresh context after vgg19_load_raw and one process_pair of the SRC / REF pair, measured on the commit before sequences existed
ARENA_BYTES_AFTER_ONE_PAIR = 36111616


def test_pair_and_arena_are_untouched_by_a_sequence(weights):
    src, ref = synth.image(*SRC), synth.image(*REF)
    frames = seq_ref.static_frames(2, SRC[1], SRC[2])
    with nct.Context(0) as c:
        c.vgg19_load_raw(*weights)
        before = c.process_pair(src, ref)
        fresh = c.counter(nct.CTR_ARENA_BYTES)
        print("arena bytes of a fresh context after one pair:", fresh)
        assert fresh == ARENA_BYTES_AFTER_ONE_PAIR
        assert c.counter(nct.CTR_ARENA_BYTES) == fresh and np.array_equal(c.process_pair(src, ref), before)
        c.seq_begin(ref, src.shape)
        for f in frames:
            c.seq_frame(f)
        print("arena bytes with an open sequence:", c.counter(nct.CTR_ARENA_BYTES))
        c.seq_end()
        c.seq_end()                                                                          # ending twice is harmless
        assert np.array_equal(c.process_pair(src, ref), before)
        after = c.counter(nct.CTR_ARENA_BYTES)
        for _ in range(2):                                                                   # sequences and pairs in turn: the arena stops growing
            c.seq_begin(ref, src.shape)
            for f in frames:
                c.seq_frame(f)
            c.seq_end()
            assert np.array_equal(c.process_pair(src, ref), before)
        assert c.counter(nct.CTR_ARENA_BYTES) == after


# ---- refusals

def test_refusals(wctx):
    src, ref = synth.image(*SRC), synth.image(*REF)
    for call in (lambda: wctx.seq_frame(src), lambda: wctx.seq_reset()):
        with pytest.raises(nct.NctError) as e:
            call()
        assert e.value.code == -5 and "no sequence is open" in str(e.value)
    for kw, word in ((dict(tau=1.0), "tau"), (dict(tau=-0.01), "tau"), (dict(tau=float("nan")), "tau"), (dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"),
                     (dict(sigma=float("inf")), "sigma"), (dict(sigma=float("nan")), "sigma")):
        with pytest.raises(nct.NctError) as e:
            wctx.seq_begin(ref, src.shape, **kw)
        assert e.value.code == -2 and word in str(e.value), str(e.value)
    for r, shape in ((synth.image(5, 16, 40), src.shape), (ref, (16, 40, 3)), (ref, (4001, 64, 3))):
        with pytest.raises(nct.NctError) as e:
            wctx.seq_begin(r, shape)
        assert e.value.code == -2 and "sides" in str(e.value), str(e.value)
    e1 = np.zeros((2, 16, 3)); l1 = np.zeros((4, 4, 3), np.uint8)
    for tau, sigma, word in ((1.0, 10.0, "tau"), (0.5, 0.0, "sigma")):
        with pytest.raises(nct.NctError) as e:
            wctx.seq_blend(e1, e1, l1, l1, tau, sigma)
        assert e.value.code == -2 and word in str(e.value)
    exp = wctx.process_pair(src, ref)                                                        # nothing above left a sequence open
    wctx.seq_begin(ref, src.shape)
    try:
        for call in (lambda: wctx.pair_upload(src, ref), lambda: wctx.process_pair(src, ref), lambda: wctx.multi_upload(src, [ref, ref]), lambda: wctx.process_multi(src, [ref]),
                     lambda: wctx.process_pair_fullres(src, ref), lambda: wctx.pair_run()):
            with pytest.raises(nct.NctError) as e:
                call()
            assert e.value.code == -5 and "a sequence is open" in str(e.value), str(e.value)
        with pytest.raises(nct.NctError) as e:
            wctx.seq_frame(synth.image(3, 70, 56))                                           # another size than begun
        assert e.value.code == -2
        assert np.array_equal(wctx.seq_frame(src), exp)                                      # the sequence is still usable, and this is its first frame
    finally:
        wctx.seq_end()
    assert np.array_equal(wctx.process_pair(src, ref), exp)


# ---- console driver

def test_cli_seq(tmp_path, wctx, weights):
    from caffemodel_io import write_caffemodel
    ws, bs = weights
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    inp = tmp_path / "in"; inp.mkdir()
    save = lambda name, img: Image.fromarray(img[..., ::-1].copy()).save(inp / name)
    read = lambda p: np.asarray(Image.open(p).convert("RGB"))[..., ::-1]
    r, q = synth.image(*REF), synth.image(1002, 72, 50)
    f = seq_ref.static_frames(3, SRC[1], SRC[2])
    g = seq_ref.pan_frames(2, SRC[1], SRC[2], seed=1004)
    big = synth.image(1005, 80, 70)
    save("r.png", r); save("q.png", q); save("big.png", big)
    for t in range(3):
        save("f%d.png" % t, f[t])
    for t in range(2):
        save("g%d.png" % t, g[t])
    (inp / "bad.png").write_bytes(b"not an image")
    # sequence 0: three frames to r; a comma line; sequence 1 to q: a frame, a line that cannot be decoded (skipped: the state goes on), a frame, then a frame of
    # another size (a new sequence begins at it)
    (inp / "pairs.txt").write_text("f0.png r.png 2.0\nf1.png r.png 2.0\nf2.png r.png 2.0\nf0.png r.png,q.png 2.0\ng0.png q.png 1.0\nbad.png q.png 1.0\ng1.png q.png 1.0\nbig.png q.png 1.0\n")
    p2 = nct.Params.default(); p2.bds_weight = 2.0
    p1 = nct.Params.default(); p1.bds_weight = 1.0
    exp = {}
    exp["f0_r+q_2.00.png"] = wctx.process_multi(f[0], [r, q], p2)
    exp["big_q_1.00.png"] = wctx.process_pair(big, q, p1)
    try:
        wctx.seq_begin(r, f[0].shape, p2)
        for t in range(3):
            exp["f%d_r_2.00.png" % t] = wctx.seq_frame(f[t])
        wctx.seq_begin(q, g[0].shape, p1)
        for t in range(2):
            exp["g%d_q_1.00.png" % t] = wctx.seq_frame(g[t])
    finally:
        wctx.seq_end()
    assert not np.array_equal(exp["f1_r_2.00.png"], wctx.process_pair(f[1], r, p2))          # the blend is at work in what the files are compared with

    def run(out, *extra):
        res = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(out), "-g", "0", "-seq", "1", *extra], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout

    def check(out):
        assert sorted(n for n in os.listdir(out) if n.endswith(".png")) == sorted(exp)
        for name, img in exp.items():
            assert np.array_equal(read(out / name), img), name

    o1 = tmp_path / "out1"
    log = run(o1, "-gpus", "1")
    check(o1)
    assert log.count("begins at this frame") == 3 and "Fail reading content image" in log
    o2 = tmp_path / "out2"
    run(o2, "-inflight", "2")
    check(o2)
    # -resume 1: a sequence with an output missing is redone from its first frame; one whose outputs are all there is skipped
    os.remove(o1 / "f1_r_2.00.png")
    log = run(o1, "-resume", "1")
    check(o1)
    assert log.count("Skipping (-resume)") == 1                                              # the comma line; sequence 1 has a line that never gets an output
    log = run(o1, "-resume", "1")
    assert log.count("Skipping (-resume)") == 4
    # -tau 0: every frame on its own
    o3 = tmp_path / "out3"
    run(o3, "-tau", "0")
    assert np.array_equal(read(o3 / "f1_r_2.00.png"), wctx.process_pair(f[1], r, p2))
