"""Propagated frames (SPEC §6.5) on the GPU: k_seq_warp against the numpy rule (tests/seq_prop_ref.py), keyed sequences against the composition frame by frame,
the identities of rule 7, the refusals, the timing fields, what a context holds, and the console driver's -key. All comparisons are equality of bytes / bit patterns."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from PIL import Image

import nct
import seq_mc_ref
import seq_prop_ref
import seq_ref
import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "neural-color-transfer_amd", "bin", "neural_color_transfer")

H, W = 56, 64
REF = (2000, 60, 72)
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
PLAN = [True, False, False, True, False]                     # key-frame grid 3 over five frames


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
    return seq_ref.pan_frames(5, H, W, step=4)


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def level_dims(levels):
    d, h, w = [], H, W
    for _ in range(5):
        d.insert(0, (h, w)); h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return d[:levels]


# ---- seams: nct_seq_warp / nct_seq_warp_dev against the numpy rule

@pytest.mark.parametrize("grid", [(1, 1), (1, 7), (6, 1), (5, 4), (9, 11), (37, 70)])          # 37 x 70: more than one block, rows that straddle blocks
def test_warp_matches_the_numpy_rule(ctx, grid):
    h, w = grid
    for kind in ("random", "outside", "nan"):
        x, field = seq_prop_ref.warp_case(h, w, 13 * h + w, kind)
        exp = words(seq_prop_ref.warp(x, field))
        assert np.array_equal(words(ctx.seq_warp(x, field)), exp), kind
        assert np.array_equal(words(ctx.seq_warp_dev(x, field)), exp), kind
    assert np.array_equal(words(ctx.seq_warp(x, np.zeros((h, w, 2), np.int16))), words(x))      # m = 0 moves nothing, NaN payloads included


def test_warp_refusals(ctx):
    x, field = seq_prop_ref.warp_case(6, 7, 1)
    with pytest.raises(nct.NctError) as e:
        ctx.seq_warp_dev(x, field, alias=True)                                                  # the warp gathers: not in place
    assert e.value.code == -2 and "alias" in str(e.value)
    a = np.ascontiguousarray(x, np.float64).reshape(-1)
    for args, word in (((a, 0, 7, field.ctypes.data, a.copy()), "grid"), ((a, 6, 4097, field.ctypes.data, a.copy()), "grid"), ((a, 6, 7, None, a.copy()), "null")):
        with pytest.raises(nct.NctError) as e:
            ctx._chk(ctx._l.nct_seq_warp(ctx._h, *args))
        assert e.value.code == -2 and word in str(e.value)


# ---- keyed sequences against the composition

_expected = {}


def expected(oracle, weights, frames, motion, levels):
    """seq_prop_ref.sequence_keyed of the five frames, once per (motion, levels)"""
    if (motion, levels) not in _expected:
        ws, bs = weights
        _expected[(motion, levels)] = seq_prop_ref.sequence_keyed(oracle, frames, synth.image(*REF), ws, bs, full=PLAN, mot=MOT if motion else None, levels=levels)
    return _expected[(motion, levels)]


def begin(c, levels=5, motion=True, **kw):
    prm = nct.Params.default(); prm.levels = levels
    c.seq_begin(synth.image(*REF), (H, W, 3), prm, **kw)
    if motion:
        c.seq_set_motion(*MOT)


def run_keyed(c, frames, plan=PLAN):
    return [c.seq_frame(f) if whole else c.seq_frame_propagate(f) for f, whole in zip(frames, plan)]


@pytest.mark.parametrize("motion", [True, False])
@pytest.mark.parametrize("levels", [5, 2])
def test_keyed_sequence_matches_the_composition(wctx, oracle, weights, frames, motion, levels):
    exp, keeps, _ = expected(oracle, weights, frames, motion, levels)
    dims = level_dims(levels)
    # conditions on the expected side: with motion the propagated frames carry a field that is not zero and their X' differs from the previous frame's
    if motion and levels == 5:
        assert all(keeps[t]["motion"][4].any() for t in (1, 2, 4))
        assert not np.array_equal(words(keeps[1]["ab_blend"][4]), words(keeps[0]["ab_blend"][4]))
    begin(wctx, levels, motion)
    try:
        for t, (f, whole) in enumerate(zip(frames, PLAN)):
            if whole:
                out, lv = wctx.seq_frame_levels(f, want_color=False)
            else:
                out, lv = wctx.seq_frame_propagate_levels(f)
                assert lv["dims"][:levels] == dims and all((tm == 1.0).all() for tm in lv["tau_map"])
                h, w = dims[-1]
                assert np.array_equal(out, wctx.color_finish(lv["ab_blend"][-1], h, w, H, W, f)), ("finish", t)        # rule 5: the finish of the last level run alone
            for l in range(levels):
                assert np.array_equal(lv["motion"][l], keeps[t]["motion"][l]), ("motion", t, l)
                assert np.array_equal(words(lv["ab_blend"][l]), words(keeps[t]["ab_blend"][l])), ("ab_blend", t, l)
            assert np.array_equal(out, exp[t]), t
    finally:
        wctx.seq_end()
    # the plain entry points give the same frames
    begin(wctx, levels, motion)
    try:
        assert all(np.array_equal(a, b) for a, b in zip(run_keyed(wctx, frames), exp))
    finally:
        wctx.seq_end()


# ---- identities (rule 7)

@pytest.mark.parametrize("levels,mot", [(5, MOT), (2, (8, 3, 0)), (5, None)])
def test_identical_frame_returns_the_previous_output(wctx, frames, levels, mot):
    begin(wctx, levels, motion=False, tau=0.9, sigma=3.0)
    try:
        if mot:
            wctx.seq_set_motion(*mot)
        wctx.seq_frame(frames[0])
        prev, lv_prev = wctx.seq_frame_levels(frames[1], want_color=False)                      # a blended full frame
        for _ in range(2):                                                                      # after a full frame, then after a propagated one
            out, lv = wctx.seq_frame_propagate_levels(frames[1])
            assert np.array_equal(out, prev)
            assert not any(m.any() for m in lv["motion"])
            assert all(np.array_equal(words(a), words(b)) for a, b in zip(lv["ab_blend"], lv_prev["ab_blend"]))
        moved, lv = wctx.seq_frame_propagate_levels(frames[2])                                  # and a frame that moved is another picture
        assert not np.array_equal(moved, prev)
        assert np.array_equal(wctx.seq_frame_propagate(frames[2]), moved)
    finally:
        wctx.seq_end()


def test_two_contexts_give_the_same_bytes(wctx, weights, frames):
    begin(wctx)
    try:
        a = run_keyed(wctx, frames)
    finally:
        wctx.seq_end()
    with nct.Context(0) as c:
        c.vgg19_load_raw(*weights)
        begin(c)
        b = run_keyed(c, frames)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        c.seq_reset()                                                                           # and twice on one context
        assert all(np.array_equal(x, y) for x, y in zip(a, run_keyed(c, frames)))


def test_a_sequence_that_never_propagates_is_unchanged(wctx, weights, frames):
    """identity 7(b): the plain frames are a second context's, and so is what the arena holds after three of them; the first propagated frame reserves at most
    one map of the last level run (48 B per pixel, rounded up to the arena's 256 B)"""
    begin(wctx)
    try:
        a = [wctx.seq_frame(f) for f in frames[:3]]
    finally:
        wctx.seq_end()
    held = []
    for _ in range(2):
        with nct.Context(0) as c:
            c.vgg19_load_raw(*weights)
            begin(c)
            assert all(np.array_equal(c.seq_frame(f), x) for f, x in zip(frames[:3], a))
            held.append(c.counter(nct.CTR_ARENA_BYTES))
            c.seq_frame_propagate(frames[3])
            grown = c.counter(nct.CTR_ARENA_BYTES) - held[-1]
            c.seq_frame_propagate(frames[4])
            assert c.counter(nct.CTR_ARENA_BYTES) - held[-1] == grown                          # reserved once
    print("arena bytes after three full frames: %d and %d; the first propagated frame adds %d" % (held[0], held[1], grown))
    assert held[0] == held[1]
    assert 0 <= grown <= (48 * H * W + 255) // 256 * 256
    with nct.Context(0) as c:                                                                   # motion off: no warp, nothing reserved
        c.vgg19_load_raw(*weights)
        begin(c, motion=False)
        c.seq_frame(frames[0])
        before = c.counter(nct.CTR_ARENA_BYTES)
        c.seq_frame_propagate(frames[1])
        assert c.counter(nct.CTR_ARENA_BYTES) == before


# ---- refusals

def test_refusals(wctx, frames):
    def refused(call, code, word):
        with pytest.raises(nct.NctError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)

    refused(lambda: wctx.seq_frame_propagate(frames[0]), -5, "no sequence is open")
    refused(lambda: wctx.seq_frame_propagate_levels(frames[0]), -5, "no sequence is open")
    begin(wctx)
    try:
        refused(lambda: wctx.seq_frame_propagate(frames[0]), -5, "no state")                    # before any frame
        a0 = wctx.seq_frame(frames[0])
        a1 = wctx.seq_frame_propagate(frames[1])
        raw = C.CDLL(nct.LIB_PATH).nct_seq_frame_propagate                                      # the binding's own prototype takes arrays only
        raw.restype, raw.argtypes = C.c_int, [C.c_void_p] * 4
        refused(lambda: wctx._chk(raw(wctx._h, None, a1.ctypes.data, None)), -2, "null")
        refused(lambda: wctx._chk(raw(wctx._h, a1.ctypes.data, None, None)), -2, "null")
        wctx.seq_reset()
        refused(lambda: wctx.seq_frame_propagate(frames[1]), -5, "no state")                    # after a reset
        assert np.array_equal(wctx.seq_frame(frames[0]), a0)                                    # the sequence still works
        assert np.array_equal(wctx.seq_frame_propagate(frames[1]), a1)
        refused(lambda: wctx.seq_frame_propagate(frames[0][:40]), -2, "the sequence was begun for")
    finally:
        wctx.seq_end()


# ---- timing

@pytest.mark.parametrize("levels", [5, 2])
def test_timing_of_a_propagated_frame(wctx, frames, levels):
    begin(wctx, levels)
    try:
        _, full = wctx.seq_frame(frames[0], want_timing=True)
        _, tm = wctx.seq_frame_propagate(frames[1], want_timing=True)
    finally:
        wctx.seq_end()
    top = levels - 1
    assert full["vgg_ms"] > 0 and full["patchmatch_ms"] > 0 and all(n > 0 for n in full["pm_level_launches"][:levels])
    for k in ("vgg_ms", "patchmatch_ms", "vote_ms", "knn_ms", "cluster_ms", "nonlocal_ms"):
        assert tm[k] == 0, k
    assert not any(tm["pm_level_launches"]) and not any(tm["pm_level_ms"]) and not any(tm["nonlocal_level_ms"])
    assert tm["wls_iters"][top] > 0 and not any(n for l, n in enumerate(tm["wls_iters"]) if l != top)
    assert tm["wls_level_ms"][top] > 0 and not any(v for l, v in enumerate(tm["wls_level_ms"]) if l != top)
    assert tm["wls_ms"] > 0 and tm["color_ms"] >= tm["wls_ms"] and tm["total_ms"] > 0


# ---- console driver

def test_cli_key(tmp_path, wctx, weights, frames):
    from caffemodel_io import write_caffemodel
    ws, bs = weights
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    inp = tmp_path / "in"; inp.mkdir()
    save = lambda name, img: Image.fromarray(img[..., ::-1].copy()).save(inp / name)
    read = lambda p: np.asarray(Image.open(p).convert("RGB"))[..., ::-1]
    save("r.png", synth.image(*REF))
    for t in range(5):
        save("f%d.png" % t, frames[t])
    (inp / "pairs.txt").write_text("".join("f%d.png r.png 2.0\n" % t for t in range(5)))

    def run(out, *extra):
        res = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(out), "-g", "0", "-seq", "1", "-motion", "1", "-levels", "2", *extra], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout, [read(out / ("f%d_r_2.00.png" % t)) for t in range(5)]

    p2 = nct.Params.default(); p2.bds_weight = 2.0; p2.levels = 2; p2.flags = nct.FLAG_LATENCY
    keyed, plain = [], []
    for plan, outs in ((PLAN, keyed), ([True] * 5, plain)):
        try:
            wctx.seq_begin(synth.image(*REF), (H, W, 3), p2)
            wctx.seq_set_motion(*MOT)
            outs += run_keyed(wctx, frames, plan)
        finally:
            wctx.seq_end()
    assert not np.array_equal(keyed[1], plain[1])                                               # the grid is at work in what the files are compared with
    log, got = run(tmp_path / "o1", "-key", "3")
    assert all(np.array_equal(a, b) for a, b in zip(got, keyed))
    assert [("frame %d is propagated" % t) in log for t in range(5)] == [not whole for whole in PLAN]
    log1, got1 = run(tmp_path / "o2", "-key", "1")
    log0, got0 = run(tmp_path / "o3")
    assert all(np.array_equal(a, b) for a, b in zip(got1, got0)) and all(np.array_equal(a, b) for a, b in zip(got0, plain))
    assert "propagated" not in log1 and "propagated" not in log0
