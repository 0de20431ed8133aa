"""Full-resolution sequences (SPEC §6.9) on the GPU: keyed plans frame by frame against the composition from a plain sequence on the shrunk frames and the finish
seams, the state maps bit for bit, the identities of rule 4, nct_seq_frame_auto against the plain sequence's decisions and the manual calls, nct_pair_fit_lut,
the refusals, and the console driver's -seqfull. All comparisons are equality of bytes / bit patterns."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from PIL import Image

import nct
import finish_up_ref as fr
import seq_auto_ref as ar
import seq_mc_ref
import synth

pytestmark = pytest.mark.gpu
BIN = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")

MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
PLAN = "FPPKP"
WH, WW = fr.WORK
MAPS = ("ab_blend", "tau_map", "motion")


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


@pytest.fixture(scope="module")
def frames():
    return fr.pan()


@pytest.fixture(scope="module")
def ref0():
    return synth.image(*fr.REF)


def _params(levels=5):
    p = nct.Params.default()
    p.levels = levels
    return p


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def run_plan(c, frames, plan):
    """the *_levels calls a plan names -> [(result, maps)]"""
    outs = []
    for f, k in zip(frames, plan):
        outs.append(c.seq_frame_propagate_levels(f) if k == "P" else c.seq_frame_levels(f, want_color=False))
    return outs


_plain = {}


def plain_run(c, frames, ref0, levels, motion):
    """the plain nct_seq_begin sequence on the shrunk frames and the shrunk reference, once per configuration: [(shrunk frame, result, maps)]"""
    key = (levels, motion)
    if key not in _plain:
        S = [c.resize_u8c3(f, WH, WW) for f in frames]
        R = c.resize_u8c3(ref0, *nct.working_size(*ref0.shape[:2], fr.MAX_SIDE))
        c.seq_begin(R, (WH, WW, 3), _params(levels))
        try:
            if motion:
                c.seq_set_motion(*MOT)
            _plain[key] = [(s, o, m) for s, (o, m) in zip(S, run_plan(c, S, PLAN))]
        finally:
            c.seq_end()
    return _plain[key]


def expected_frame(c, x_top, levels, S, S0, finish, prm):
    d, hh, ww = [], WH, WW
    for _ in range(5):
        d.insert(0, (hh, ww)); hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
    h, w = d[levels - 1]
    if finish == nct.FINISH_EXACT:
        return c.color_finish(x_top, h, w, WH, WW, S0, prm)
    _, st = c.color_finish(x_top, h, w, WH, WW, S, prm, want_stages=True)
    return c.color_finish_upsample(st["ab_wls"], WH, WW, S0, prm)


@pytest.mark.parametrize("finish", [nct.FINISH_EXACT, nct.FINISH_UPSAMPLE])
@pytest.mark.parametrize("levels", [5, 2])
@pytest.mark.parametrize("motion", [True, False])
def test_keyed_plan_equals_the_composition(wctx, frames, ref0, motion, levels, finish):
    prm = _params(levels)
    plain = plain_run(wctx, frames, ref0, levels, motion)
    if motion:                                                             # condition on the expected side: a propagated frame carries a field
        assert any(k == "P" and any(np.any(m) for m in maps["motion"]) for k, (_, _, maps) in zip(PLAN, plain))
    wctx.seq_begin_fullres(ref0, frames[0].shape, fr.MAX_SIDE, finish, prm)
    try:
        if motion:
            wctx.seq_set_motion(*MOT)
        got = run_plan(wctx, frames, PLAN)
    finally:
        wctx.seq_end()
    for t, ((out, maps), (S, _, pmaps)) in enumerate(zip(got, plain)):
        assert out.shape == frames[t].shape
        for k in MAPS:                                                     # rule 1: the state is the plain sequence's, word for word
            assert len(maps[k]) == levels
            for l in range(levels):
                assert np.array_equal(bits(maps[k][l]), bits(pmaps[k][l])), (t, k, l)
        exp = expected_frame(wctx, pmaps["ab_blend"][levels - 1], levels, S, frames[t], finish, prm)
        assert np.array_equal(out, exp), (t, PLAN[t], int((out != exp).sum()))


def test_first_frame_and_reset_equal_the_pair(wctx, frames, ref0):
    prm = _params(5)
    pair = [wctx.process_pair_fullres(f, ref0, fr.MAX_SIDE, prm) for f in frames[:2]]
    wctx.seq_begin_fullres(ref0, frames[0].shape, fr.MAX_SIDE, nct.FINISH_EXACT, prm)
    try:
        wctx.seq_set_motion(*MOT)
        assert np.array_equal(wctx.seq_frame(frames[0]), pair[0])
        blended = wctx.seq_frame(frames[1])
        assert not np.array_equal(blended, pair[1])                        # a blended frame is another picture
        wctx.seq_reset()
        assert np.array_equal(wctx.seq_frame(frames[1]), pair[1])
    finally:
        wctx.seq_end()
    # with the upsampling finish the first frame is the pair with that finish
    wctx.seq_begin_fullres(ref0, frames[0].shape, fr.MAX_SIDE, nct.FINISH_UPSAMPLE, prm)
    try:
        got = wctx.seq_frame(frames[0])
    finally:
        wctx.seq_end()
    assert np.array_equal(got, wctx.process_pair_fullres(frames[0], ref0, fr.MAX_SIDE, prm, finish=nct.FINISH_UPSAMPLE))


def test_frames_that_need_no_shrinking_equal_the_plain_sequence(wctx, frames, ref0):
    prm = _params(5)
    simple = lambda c: [c.seq_frame_propagate(f) if k == "P" else c.seq_frame(f) for f, k in zip(frames, PLAN)]
    wctx.seq_begin(ref0, frames[0].shape, prm)
    try:
        wctx.seq_set_motion(*MOT)
        exp = simple(wctx)
    finally:
        wctx.seq_end()
    for finish in (nct.FINISH_EXACT, nct.FINISH_UPSAMPLE):
        wctx.seq_begin_fullres(ref0, frames[0].shape, 1000, finish, prm)
        try:
            wctx.seq_set_motion(*MOT)
            got = simple(wctx)
        finally:
            wctx.seq_end()
        assert all(np.array_equal(a, b) for a, b in zip(got, exp)), finish


@pytest.mark.parametrize("finish", [nct.FINISH_EXACT, nct.FINISH_UPSAMPLE])
def test_auto_decisions_are_the_plain_sequences(wctx, ref0, finish):
    clip = fr.auto_clip()
    prm = _params(5)
    auto = nct.seq_auto(*fr.AUTO)
    S = [wctx.resize_u8c3(f, WH, WW) for f in clip]
    R = wctx.resize_u8c3(ref0, *nct.working_size(*ref0.shape[:2], fr.MAX_SIDE))
    wctx.seq_begin(R, (WH, WW, 3), prm)
    try:
        wctx.seq_set_motion(*MOT)
        plain = [wctx.seq_frame_auto(s, auto)[1] for s in S]
    finally:
        wctx.seq_end()
    assert ar.kinds(plain) == "FPKPCP"
    wctx.seq_begin_fullres(ref0, clip[0].shape, fr.MAX_SIDE, finish, prm)
    try:
        wctx.seq_set_motion(*MOT)
        probe = None
        outs, ds = [], []
        for t, f in enumerate(clip):
            if t == 1:
                probe = wctx.seq_probe(f, auto)                            # a probe takes the original frame, too, and leaves no trace
            o, d = wctx.seq_frame_auto(f, auto)
            outs.append(o); ds.append(d)
        wctx.seq_reset()
        manual = []
        for f, d in zip(clip, ds):
            if d["kind"] == ar.SCENE_CUT:
                wctx.seq_reset()
            manual.append(wctx.seq_frame_propagate(f) if d["kind"] == ar.PROPAGATED else wctx.seq_frame(f))
    finally:
        wctx.seq_end()
    strip = lambda d: {k: v for k, v in d.items() if k != "probe_ms"}
    assert [strip(d) for d in ds] == [strip(d) for d in plain]
    assert strip(probe) == strip(plain[1])
    assert all(o.shape == clip[0].shape for o in outs)
    assert all(np.array_equal(a, b) for a, b in zip(outs, manual))
    t = ar.kinds(ds).index("C")
    if finish == nct.FINISH_EXACT:                                         # rule 4: a CUT frame is the pair
        assert np.array_equal(outs[t], wctx.process_pair_fullres(clip[t], ref0, fr.MAX_SIDE, prm))


def test_pair_fit_lut_after_a_frame(wctx, frames, ref0):
    prm = _params(2)
    wctx.seq_begin_fullres(ref0, frames[0].shape, fr.MAX_SIDE, nct.FINISH_UPSAMPLE, prm)
    try:
        out = wctx.seq_frame(frames[0])
        assert np.array_equal(wctx.pair_fit_lut(9), wctx.lut_fit(frames[0], out, 9))
        out = wctx.seq_frame_propagate(frames[1])
        assert np.array_equal(wctx.pair_fit_lut(9), wctx.lut_fit(frames[1], out, 9))
    finally:
        wctx.seq_end()


def refused(call, code, word):
    with pytest.raises(nct.NctError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_refusals_and_state(wctx, frames, ref0):
    prm = _params(2)
    shape = frames[0].shape
    S = [wctx.resize_u8c3(f, WH, WW) for f in frames[:2]]
    R = wctx.resize_u8c3(ref0, 53, 64)

    def plain():
        wctx.seq_begin(R, (WH, WW, 3), prm)
        try:
            return [wctx.seq_frame(s) for s in S]
        finally:
            wctx.seq_end()
    before = plain()
    refused(lambda: wctx.seq_begin_fullres(ref0, shape, fr.MAX_SIDE, 2, prm), -2, "finish")
    refused(lambda: wctx.seq_begin_fullres(ref0, shape, fr.MAX_SIDE, -1, prm), -2, "finish")
    refused(lambda: wctx.seq_begin_fullres(ref0, shape, 16, 0, prm), -2, "max_side")
    refused(lambda: wctx.seq_begin_fullres(ref0, (16385, 100, 3), fr.MAX_SIDE, 0, prm), -2, "frames")
    refused(lambda: wctx.seq_begin_fullres(np.zeros((100, 16385, 3), np.uint8), shape, fr.MAX_SIDE, 0, prm), -2, "reference")
    refused(lambda: wctx.seq_frame(frames[0]), -5, "no sequence is open")                      # the refused begins opened nothing
    wctx.seq_begin_fullres(ref0, shape, fr.MAX_SIDE, nct.FINISH_EXACT, prm)
    try:
        a0 = wctx.seq_frame(frames[0])
        refused(lambda: wctx.seq_frame_levels(frames[1], want_levels=True), -2, "levels")
        refused(lambda: wctx.pair_upload(S[0], R), -5, "sequence is open")
        refused(lambda: wctx.process_pair_fullres(frames[0], ref0, fr.MAX_SIDE, prm), -5, "sequence is open")
        refused(lambda: wctx.seq_frame(S[0]), -2, "the sequence was begun for")
        a1 = wctx.seq_frame(frames[1])                                     # the refused calls changed nothing
        wctx.seq_reset()
        assert np.array_equal(wctx.seq_frame(frames[0]), a0) and np.array_equal(wctx.seq_frame(frames[1]), a1)
    finally:
        wctx.seq_end()
    after = plain()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_cli_seqfull(tmp_path, wctx, weights):
    from caffemodel_io import write_caffemodel
    ws, bs = weights
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    inp = tmp_path / "in"; inp.mkdir()
    import seq_ref
    big = seq_ref.pan_frames(3, 1100, 700, step=8, seed=4)
    for t, f in enumerate(big):
        Image.fromarray(f[..., ::-1].copy()).save(inp / ("f%d.jpg" % t), quality=90, subsampling=2)
    small = synth.image(5, 120, 160)
    Image.fromarray(small[..., ::-1].copy()).save(inp / "small.png")
    (inp / "pairs.txt").write_text("".join("f%d.jpg small.png 2.0\n" % t for t in range(3)))
    dec = [np.ascontiguousarray(np.asarray(Image.open(inp / ("f%d.jpg" % t)).convert("RGB"))[..., ::-1]) for t in range(3)]
    prm = _params(1); prm.bds_weight = 2.0; prm.flags = nct.FLAG_LATENCY                       # what the driver runs one pair at a time with
    for mode, finish, word in ((1, nct.FINISH_EXACT, "exact finish"), (2, nct.FINISH_UPSAMPLE, "upsampling finish")):
        out = tmp_path / ("o%d" % mode)
        r = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(out), "-levels", "1", "-seq", "1", "-key", "2", "-seqfull", str(mode)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.count("full resolution, " + word) == 1, r.stdout
        got = [np.asarray(Image.open(out / ("f%d_small_2.00.png" % t)).convert("RGB"))[..., ::-1] for t in range(3)]
        wctx.seq_begin_fullres(small, dec[0].shape, 1000, finish, prm)
        try:
            exp = [wctx.seq_frame(dec[0]), wctx.seq_frame_propagate(dec[1]), wctx.seq_frame(dec[2])]
        finally:
            wctx.seq_end()
        for t in range(3):
            assert got[t].shape == (1100, 700, 3) and np.array_equal(got[t], exp[t]), (mode, t)
