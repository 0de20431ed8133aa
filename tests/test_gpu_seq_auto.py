"""Adaptive key frames (SPEC §6.7) on the GPU: k_seq_change against the numpy measure (tests/seq_auto_ref.py), the probe against the reference's, that a probe changes
nothing, three clips through nct_seq_frame_auto against the plan and against the manual calls the plan names, the identities, the refusals and the console driver's
-autokey. All comparisons are equality of integers / bytes. The tests pass their parameters explicitly: none depends on nct_seq_auto_default's values."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from PIL import Image

import nct
import seq_auto_ref as ar
import seq_mc_ref
import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "neural-color-transfer_amd", "bin", "neural_color_transfer")

H, W = 56, 64
REF = (2000, 60, 72)
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
KEYS = ("sad", "changed", "pixels")


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


@pytest.fixture(scope="module")
def clips():
    return ar.clips(H, W)


@pytest.fixture(scope="module")
def plans(oracle, clips):
    return {name: ar.plan(oracle, frames, 5, mot, auto) for name, (frames, mot, auto) in clips.items()}


def begin(c, levels=5, mot=MOT, prm=None, **kw):
    if prm is None:
        prm = nct.Params.default(); prm.levels = levels
    c.seq_begin(synth.image(*REF), (H, W, 3), prm, **kw)
    if mot:
        c.seq_set_motion(*mot)


def refused(call, code, word):
    with pytest.raises(nct.NctError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


# ---- the measure's seams against the numpy rule

# (37, 70) and (70, 130): many workgroups, rows that straddle them, a last workgroup that is partly empty
@pytest.mark.parametrize("grid", [(1, 1), (1, 7), (6, 1), (5, 4), (9, 11), (37, 70), (70, 130)])
def test_change_matches_the_numpy_measure(ctx, grid):
    h, w = grid
    for kind in ("random", "equal", "noise"):
        for field in ("field", "none", "outside"):
            L, Lp, m = ar.change_case(h, w, 17 * h + w, kind, field)
            for T in (0, 24, 765):
                exp = ar.change(L, Lp, m, T)
                assert ctx.seq_change(L, Lp, m, T) == exp, (kind, field, T)
                assert ctx.seq_change_dev(L, Lp, m, T) == exp, (kind, field, T)
    L, Lp = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)                    # the largest sums the grid can give
    assert ctx.seq_change(L, Lp, None, 764) == {"sad": 765 * h * w, "changed": h * w, "pixels": h * w}


def test_change_refusals(ctx):
    L, Lp, m = ar.change_case(6, 7, 1)
    rec = nct.SeqChange()
    out = C.addressof(rec)
    for args, word in (((None, Lp.ctypes.data, 6, 7, None, 24, out), "image"), ((L.ctypes.data, None, 6, 7, None, 24, out), "image"),
                       ((L.ctypes.data, Lp.ctypes.data, 6, 7, None, 24, None), "out"),
                       ((L.ctypes.data, Lp.ctypes.data, 0, 7, None, 24, out), "grid"), ((L.ctypes.data, Lp.ctypes.data, 6, 4097, None, 24, out), "grid"),
                       ((L.ctypes.data, Lp.ctypes.data, 6, 7, None, -1, out), "threshold"), ((L.ctypes.data, Lp.ctypes.data, 6, 7, None, 766, out), "threshold")):
        refused(lambda: ctx._chk(ctx._l.nct_seq_change(ctx._h, *args)), -2, word)
    dl, dr = ctx.dev_upload(L), ctx.dev_alloc(16)
    try:
        for args, word in (((None, dl, 6, 7, None, 24, dr), "image"), ((dl, dl, 6, 7, None, 24, None), "out"), ((dl, dl, 4097, 7, None, 24, dr), "grid"),
                           ((dl, dl, 6, 7, None, 766, dr), "threshold")):
            refused(lambda: ctx._chk(ctx._l.nct_seq_change_dev(ctx._h, *args)), -2, word)
    finally:
        ctx.synchronize()
        ctx.dev_free(dl); ctx.dev_free(dr)


# ---- the probe

@pytest.mark.parametrize("motion", [True, False])
@pytest.mark.parametrize("levels", [5, 2, 1])
def test_probe_equals_the_reference(wctx, oracle, clips, levels, motion):
    frames = clips["pan"][0]
    mot = MOT if motion else None
    labs = [ar.labs(oracle, f, levels) for f in frames[:3]]
    auto = nct.seq_auto(24, 500, 60, 8)
    begin(wctx, levels, mot)
    try:
        wctx.seq_frame(frames[0])
        for t, gap in ((1, 0), (2, 1)):                        # after one frame, then after two (the second one propagated: it counts in gap, not in acc)
            exp = ar.probe(labs[t], labs[t - 1], mot, 24)
            got = wctx.seq_probe(frames[t], auto)
            assert {k: got[k] for k in KEYS} == exp, (t, got, exp)
            assert got["level"] == ar.probe_level(levels) and got["pixels"] == labs[t][-1].shape[0] * labs[t][-1].shape[1]
            assert got["kind"] == ar.decide(exp, 0, gap, 500, 60, 8) and got["gap"] == gap and got["acc_changed"] == 0
            assert got["probe_ms"] > 0
            assert {k: v for k, v in wctx.seq_probe(frames[t], auto).items() if k != "probe_ms"} == {k: v for k, v in got.items() if k != "probe_ms"}      # a probe leaves the next one what it found
            if t == 1:
                wctx.seq_frame_propagate(frames[1])
        same = wctx.seq_probe(frames[1], nct.seq_auto(0, 1001, 1001, 8))                         # identity (e): the frame the state holds, even at T = 0
        assert same["sad"] == 0 and same["changed"] == 0 and same["kind"] == ar.PROPAGATED
    finally:
        wctx.seq_end()


@pytest.mark.parametrize("motion", [True, False])
def test_probe_changes_nothing(wctx, weights, clips, motion):
    frames = clips["pan"][0]
    mot = MOT if motion else None
    auto = nct.seq_auto(24, 500, 60, 8)
    with nct.Context(0) as c:                                  # never probed
        c.vgg19_load_raw(*weights)
        begin(c, 5, mot)
        plain = [c.seq_frame(frames[0]), c.seq_frame_propagate(frames[1]), c.seq_frame_propagate(frames[2]), c.seq_frame(frames[3])]
        held = c.counter(nct.CTR_ARENA_BYTES)
    with nct.Context(0) as c:                                  # and once more: what a sequence that never probes holds is a fixed number
        c.vgg19_load_raw(*weights)
        begin(c, 5, mot)
        for f, whole in zip(frames[:4], (True, False, False, True)):
            c.seq_frame(f) if whole else c.seq_frame_propagate(f)
        assert c.counter(nct.CTR_ARENA_BYTES) == held
    begin(wctx, 5, mot)
    try:
        got = [wctx.seq_frame(frames[0])]
        d1 = wctx.seq_probe(frames[1], auto)
        wctx.seq_probe(frames[4], auto)                        # a probe of another frame in between leaves no trace either
        assert wctx.seq_probe(frames[1], auto)["sad"] == d1["sad"]
        got.append(wctx.seq_frame_propagate(frames[1]))
        wctx.seq_probe(frames[2], auto)
        got.append(wctx.seq_frame_propagate(frames[2]))
        d3 = wctx.seq_probe(frames[3], auto)
        assert d3["gap"] == 2 and d3["acc_changed"] == 0       # manual propagated frames count in gap only
        got.append(wctx.seq_frame(frames[3]))                  # a blended full frame reads X' and L: both as the plain run left them
        assert wctx.seq_probe(frames[4], auto)["gap"] == 0
    finally:
        wctx.seq_end()
    assert all(np.array_equal(a, b) for a, b in zip(got, plain))


# ---- three clips through nct_seq_frame_auto

def run_manual(c, frames, kinds):
    outs = []
    for f, k in zip(frames, kinds):
        if k == ar.SCENE_CUT:
            c.seq_reset()
        outs.append(c.seq_frame_propagate(f) if k == ar.PROPAGATED else c.seq_frame(f))
    return outs


def run_auto(c, frames, auto):
    outs, ds = [], []
    for f in frames:
        o, d = c.seq_frame_auto(f, nct.seq_auto(*auto))
        outs.append(o); ds.append(d)
    return outs, ds


_manual = {}


def manual(weights, frames, mot, kinds, tag):
    """the manual calls a plan names, on a context of their own; once per plan"""
    key = (tag, tuple(kinds))
    if key not in _manual:
        with nct.Context(0) as c:
            c.vgg19_load_raw(*weights)
            begin(c, 5, mot)
            _manual[key] = run_manual(c, frames, kinds)
    return _manual[key]


@pytest.mark.parametrize("clip", ["pan", "motion_off", "cut"])
def test_clip_matches_the_plan_and_the_manual_calls(wctx, weights, clips, plans, clip):
    frames, mot, auto = clips[clip]
    plan = plans[clip]
    begin(wctx, 5, mot)
    try:
        outs, ds = run_auto(wctx, frames, auto)
        again = None
        if clip == "cut":                                      # identity (f): after a reset the same calls give the same decisions and bytes
            wctx.seq_reset()
            again = run_auto(wctx, frames, auto)
    finally:
        wctx.seq_end()
    for t, (d, e) in enumerate(zip(ds, plan)):
        assert {k: d[k] for k in e} == e, (t, d, e)
        assert (d["probe_ms"] > 0) == (t > 0)
    exp = manual(weights, frames, mot, [e["kind"] for e in plan], clip)
    assert all(np.array_equal(a, b) for a, b in zip(outs, exp))                                 # identity (a)
    if clip == "cut":
        t = ar.kinds(plan).index("C")
        assert np.array_equal(outs[t], wctx.process_pair(frames[t], synth.image(*REF)))         # identity (b)
        assert not np.array_equal(outs[t], manual(weights, frames, mot, [ar.FIRST, ar.PROPAGATED, ar.KEYFRAME, ar.PROPAGATED], "cut as key")[t])   # a blended frame is another picture
        assert all(np.array_equal(a, b) for a, b in zip(again[0], outs)) and [d["kind"] for d in again[1]] == [d["kind"] for d in ds]


def test_identities_c_and_d(wctx, weights, clips):
    frames, mot, _ = clips["pan"]
    for auto, kinds in (((24, 1001, 0, 8), "FKKKK"), ((24, 1001, 1001, 3), "FPPKP")):           # (c) all full; (d) the grid of -key 3
        begin(wctx, 5, mot)
        try:
            outs, ds = run_auto(wctx, frames, auto)
        finally:
            wctx.seq_end()
        assert ar.kinds(ds) == kinds
        exp = manual(weights, frames, mot, ["FPKC".index(k) for k in kinds], "pan")
        assert all(np.array_equal(a, b) for a, b in zip(outs, exp))


# ---- refusals

def test_refusals(wctx, clips):
    frames = clips["pan"][0]
    auto = nct.seq_auto(24, 500, 60, 8)
    refused(lambda: wctx.seq_probe(frames[0], auto), -5, "no sequence is open")
    refused(lambda: wctx.seq_frame_auto(frames[0], auto), -5, "no sequence is open")
    begin(wctx)
    try:
        refused(lambda: wctx.seq_probe(frames[0], auto), -5, "no state")                        # before any frame
        a0, d0 = wctx.seq_frame_auto(frames[0], auto)
        assert d0["kind"] == ar.FIRST and d0["level"] == -1 and d0["pixels"] == 0 and d0["probe_ms"] == 0
        bad = [nct.seq_auto(-1, 500, 60, 8), nct.seq_auto(766, 500, 60, 8), nct.seq_auto(24, -1, 60, 8), nct.seq_auto(24, 1002, 60, 8),
               nct.seq_auto(24, 500, -1, 8), nct.seq_auto(24, 500, 1002, 8), nct.seq_auto(24, 500, 60, 0), nct.seq_auto(24, 500, 60, 1001)]
        words = ["threshold", "threshold", "cut_permille", "cut_permille", "key_permille", "key_permille", "max_gap", "max_gap"]
        for p, word in zip(bad, words):
            refused(lambda: wctx.seq_probe(frames[1], p), -2, word)
            refused(lambda: wctx.seq_frame_auto(frames[1], p), -2, word)
        out = np.empty_like(frames[1])
        d = nct.SeqDecision()
        raw = lambda *a: wctx._chk(wctx._l.nct_seq_frame_auto(wctx._h, *a))
        refused(lambda: raw(None, out.ctypes.data, None, C.addressof(auto), C.addressof(d)), -2, "null")
        refused(lambda: raw(frames[1].ctypes.data, None, None, C.addressof(auto), C.addressof(d)), -2, "null")
        refused(lambda: wctx._chk(wctx._l.nct_seq_probe(wctx._h, None, C.addressof(auto), C.addressof(d))), -2, "null")
        refused(lambda: wctx._chk(wctx._l.nct_seq_probe(wctx._h, frames[1].ctypes.data, C.addressof(auto), None)), -2, "null")
        refused(lambda: wctx.seq_frame_auto(frames[0][:40], auto), -2, "the sequence was begun for")
        a1, d1 = wctx.seq_frame_auto(frames[1], auto)          # the refused calls changed nothing: frame 1 is what it is without them
        wctx.seq_reset()
        refused(lambda: wctx.seq_probe(frames[1], auto), -5, "no state")                        # after a reset
        b0, _ = wctx.seq_frame_auto(frames[0], auto)
        b1, e1 = wctx.seq_frame_auto(frames[1], auto)
        assert np.array_equal(a0, b0) and np.array_equal(a1, b1) and {k: d1[k] for k in KEYS + ("kind",)} == {k: e1[k] for k in KEYS + ("kind",)}
        # NULL parameters are the defaults
        dflt = nct.SeqAuto.default()
        assert wctx.seq_probe(frames[2], None)["changed"] == wctx.seq_probe(frames[2], nct.seq_auto(dflt.threshold, 500, 60, 8))["changed"]
    finally:
        wctx.seq_end()


# ---- console driver

def test_cli_autokey(tmp_path, wctx, weights, clips, plans):
    from caffemodel_io import write_caffemodel
    frames, mot, auto = clips["cut"]
    plan = plans["cut"]
    ws, bs = weights
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    inp = tmp_path / "in"; inp.mkdir()
    save = lambda name, img: Image.fromarray(img[..., ::-1].copy()).save(inp / name)
    read = lambda p: np.asarray(Image.open(p).convert("RGB"))[..., ::-1]
    save("r.png", synth.image(*REF))
    for t, f in enumerate(frames):
        save("f%d.png" % t, f)
    (inp / "pairs.txt").write_text("".join("f%d.png r.png 2.0\n" % t for t in range(len(frames))))
    base = [BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-g", "0"]

    res = subprocess.run(base + ["-o", str(tmp_path / "o1"), "-seq", "1", "-motion", "1", "-autokey", "1", "-keythr", "24", "-keycut", "500", "-keychange", "60", "-keygap", "8"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    got = [read(tmp_path / "o1" / ("f%d_r_2.00.png" % t)) for t in range(len(frames))]
    prm = nct.Params.default(); prm.bds_weight = 2.0; prm.flags = nct.FLAG_LATENCY             # what the driver runs one pair at a time with
    assert auto == (24, 500, 60, 8)                                                              # the command line's values are the plan's
    begin(wctx, 5, mot, prm)
    try:
        outs, ds = run_auto(wctx, frames, auto)
    finally:
        wctx.seq_end()
    assert ar.kinds(ds) == ar.kinds(plan) == "FPCP"
    assert all(np.array_equal(a, b) for a, b in zip(got, outs))
    log = res.stdout
    for t, d in enumerate(plan):
        said = [("frame %d is %s (changed %d of %d at level %d)" % (t, what, d["changed"], d["pixels"], d["level"])) in log for what in ("propagated", "a key frame", "a scene cut")]
        assert said == [d["kind"] == ar.PROPAGATED, d["kind"] == ar.KEYFRAME, d["kind"] == ar.SCENE_CUT], (t, log)
    assert log.count("is propagated (changed") == 2 and log.count("is a scene cut") == 1 and "is a key frame" not in log

    for extra, text in ((["-autokey", "1"], "-autokey 1 needs -seq 1"), (["-seq", "1", "-autokey", "1", "-key", "3"], "-autokey 1 cannot be combined with -key 3"),
                        (["-seq", "1", "-autokey", "1", "-keygap", "0"], "-keygap 0 is not in [1, 1000]")):
        res = subprocess.run(base + ["-o", str(tmp_path / "o2")] + extra, capture_output=True, text=True)
        assert res.returncode != 0 and ("Error: " + text) in res.stdout, res.stdout
    assert not (tmp_path / "o2").exists()                                                       # refused before any work
