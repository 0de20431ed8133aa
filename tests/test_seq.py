"""Frame sequences (SPEC §6.3) without a GPU: the numpy blend rule against a scalar loop in the canonical order, the composition of the oracle's stages
(tests/seq_ref.py) against oracle.process_pair for the frames that have no blend, the identical-frames identity, what the blend is for (less flicker), and the
console driver's grouping of pairs.txt lines into sequences through its --plan-only hook."""
import math
import os
import subprocess
import numpy as np
import pytest

import fullres_ref
import seq_ref
import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "neural-color-transfer_amd", "bin", "neural_color_transfer")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def blend_scalar(x, xp, lab, labp, tau, sigma):
    """rule 3 pixel by pixel, python floats (IEEE doubles) and ints, dy outer / dx inner"""
    h, w = lab.shape[:2]
    n = h * w
    x, xp = np.asarray(x, np.float64).reshape(2, n, 3), np.asarray(xp, np.float64).reshape(2, n, 3)
    out, tm = np.empty((2, n, 3)), np.empty((h, w))
    for y in range(h):
        for xx in range(w):
            D, taps = 0, 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qy, qx = y + dy, xx + dx
                    if 0 <= qy < h and 0 <= qx < w:
                        taps += 1
                        for c in range(3):
                            d = int(lab[qy, qx, c]) - int(labp[qy, qx, c])
                            D += d * d
            qbar = float(D) / float(3 * taps)
            g = 1.0 / (1.0 + qbar / (sigma * sigma))
            tp = tau * g
            tm[y, xx] = tp
            p = y * w + xx
            for part in range(2):
                for c in range(3):
                    a, b = float(x[part, p, c]), float(xp[part, p, c])
                    out[part, p, c] = a if math.isnan(b) else a + tp * (b - a)
    return out, tm


BLEND_CASES, blend_case = seq_ref.BLEND_CASES, seq_ref.blend_case


@pytest.mark.parametrize("grid,kind", BLEND_CASES)
@pytest.mark.parametrize("tau,sigma", [(0.7, 10.0), (0.5, 4.0), (0.85, 0.75)])
def test_numpy_blend_equals_the_scalar_loop(grid, kind, tau, sigma):
    x, xp, lab, labp = blend_case(grid[0], grid[1], 17 * grid[0] + grid[1], kind)
    got, tm = seq_ref.blend(x, xp, lab, labp, tau, sigma)
    exp, etm = blend_scalar(x, xp, lab, labp, tau, sigma)
    assert np.array_equal(bits(tm), bits(etm))
    assert np.array_equal(bits(got), bits(exp))                # NaNs of x included: they come through as they went in or as the arithmetic makes them
    if kind == "equal":
        assert (tm == tau).all()                               # no change between the frames: g = 1 exactly
    if kind in ("nan_prev", "nan_both"):
        m = np.isnan(xp)
        assert m.any() and np.array_equal(bits(got[m]), bits(x[m]))
    if kind == "nan_x":
        assert np.isnan(got[np.isnan(x)]).all() and not np.isnan(got[~np.isnan(x)]).any()


def test_blend_border_pixels_use_only_in_grid_taps():
    h, w = 4, 5
    lab = np.zeros((h, w, 3), np.uint8); labp = lab.copy()
    labp[0, 0] = (3, 0, 0)                                     # D = 9 wherever the window holds (0, 0): the corner has 4 taps, (0, 1) and (1, 0) 6, (1, 1) 9
    x = np.zeros((2, h * w, 3)); xp = np.ones((2, h * w, 3))
    _, tm = seq_ref.blend(x, xp, lab, labp, 0.5, 1.0)
    exp = np.full((h, w), 0.5)
    for (y, xx), taps in (((0, 0), 4), ((0, 1), 6), ((1, 0), 6), ((1, 1), 9)):
        exp[y, xx] = 0.5 * (1.0 / (1.0 + (9.0 / (3 * taps)) / 1.0))
    assert np.array_equal(bits(tm), bits(exp))


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


SRC, REF = (1000, 64, 56), (1001, 48, 64)


@pytest.mark.parametrize("levels", [5, 1])
def test_composition_equals_oracle_without_a_blend(oracle, weights, levels):
    """frame 0 of any sequence and every frame with tau = 0 are oracle.process_pair; and with no blend the finish the blended frames go through
    (fullres_ref.oracle_finish at the working size) reproduces local_color_transfer's own result on every level"""
    ws, bs = weights
    ref = synth.image(*REF)
    frames = seq_ref.pan_frames(2, SRC[1], SRC[2])
    exp = [oracle.process_pair(f, ref, ws, bs, params=dict(levels=levels)) for f in frames]
    outs, keeps = seq_ref.sequence(oracle, frames, ref, ws, bs, tau=0.0, levels=levels)
    assert np.array_equal(outs[0], exp[0]) and np.array_equal(outs[1], exp[1])
    assert not any(t.any() for k in keeps for t in k["tau_map"])
    outs7, keeps7 = seq_ref.sequence(oracle, frames, ref, ws, bs, levels=levels)
    assert np.array_equal(outs7[0], exp[0])
    assert not np.array_equal(outs7[1], exp[1])                # the second frame is blended: it is no pair result
    assert all(0 < t.min() and t.max() <= seq_ref.TAU for t in keeps7[1]["tau_map"])
    H, W = frames[0].shape[:2]
    for l in range(levels):
        h, w = keeps7[0]["tau_map"][l].shape
        fin, _ = fullres_ref.oracle_finish(oracle, keeps7[0]["ab_nonlocal"][l], h, w, H, W, frames[0])
        assert np.array_equal(fin, keeps7[0]["result"][l]), l


def test_identical_frames_give_identical_outputs(oracle, weights):
    ws, bs = weights
    src, ref = synth.image(*SRC), synth.image(*REF)
    for tau, sigma in ((0.7, 10.0), (0.9, 3.0)):
        outs, keeps = seq_ref.sequence(oracle, [src] * 3, ref, ws, bs, tau=tau, sigma=sigma)
        assert np.array_equal(outs[1], outs[0]) and np.array_equal(outs[2], outs[0])
        assert all((t == tau).all() for t in keeps[2]["tau_map"])


def test_blend_lowers_flicker_on_the_static_noisy_scene(oracle, weights):
    """What the feature is for. Four frames of seq_ref.static_frames (one 64 x 56 scene, sensor noise of sigma = 2 grey levels per frame, default_rng(5)):
    the source itself flickers at 2.2552 grey levels; the composition's flicker is 2.8861 with tau = 0 (independent frames) and 2.0417 with the defaults
    tau = 0.7, sigma = 10 (transform flicker 2.5474 against 1.6466). Both sides are deterministic CPU results: strictly less, no margin."""
    ws, bs = weights
    ref = synth.image(*REF)
    frames = seq_ref.static_frames(4, SRC[1], SRC[2])
    independent, _ = seq_ref.sequence(oracle, frames, ref, ws, bs, tau=0.0)
    blended, _ = seq_ref.sequence(oracle, frames, ref, ws, bs, tau=0.7, sigma=10.0)
    f0, f1 = seq_ref.flicker(independent), seq_ref.flicker(blended)
    print("flicker: source %.4f, tau = 0 %.4f, tau = 0.7 / sigma = 10 %.4f; transform flicker %.4f -> %.4f"
          % (seq_ref.flicker(frames), f0, f1, seq_ref.transform_flicker(independent, frames), seq_ref.transform_flicker(blended, frames)))
    assert f1 < f0


# ---- console driver

def _run(tmp_path, lines, *extra):
    inp = tmp_path / "in"; inp.mkdir(exist_ok=True)
    (inp / "pairs.txt").write_text("".join(l + "\n" for l in lines))
    return subprocess.run([BIN, "--plan-only", "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(tmp_path / "out"), *extra], capture_output=True, text=True)


def _plan(tmp_path, lines, *extra):
    r = _run(tmp_path, lines, *extra)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not (tmp_path / "out").exists()
    return [l[len("@@JOB "):] for l in r.stdout.splitlines() if l.startswith("@@JOB ")]


MIXED = ["f0.png r.png 2.0", "f1.png r.png 2.0", "f2.png r.png 2", "g0.png r.png 1.0", "g1.png q.png 1.0", "g2.png q.png,r.png 1.0", "g3.png q.png 1.0", "g4.png q.png 1.0",
         "h.png a.png,,b.png 1.0", "h.png sub/q.png 1.0", "h2.png q.png 1.0"]


def test_cli_groups_lines_into_sequences(tmp_path):
    out = str(tmp_path / "out")
    jobs = _plan(tmp_path, MIXED, "-seq", "1")
    assert len(jobs) == len(MIXED)
    seq = [j.rsplit(" seq=", 1)[1] if " seq=" in j else None for j in jobs]
    # same reference token and weight: one run; another weight, another reference, a comma line, a refused line and another spelling of a name each end it
    assert seq == ["0:0", "0:1", "0:2", "1:0", "2:0", None, "3:0", "3:1", None, "4:0", "5:0"]
    assert jobs[0] == "src=f0.png refs=r.png bds=2 out=%s/f0_r_2.00.png seq=0:0" % out                    # the output names are those of single pairs
    assert jobs[5] == "src=g2.png refs=q.png|r.png bds=1 out=%s/g2_q+r_1.00.png" % out
    assert jobs[8].startswith("error=") and "empty reference name" in jobs[8]


def test_cli_plan_is_unchanged_without_seq(tmp_path):
    jobs = _plan(tmp_path, MIXED)
    assert len(jobs) == len(MIXED) and not any("seq=" in j for j in jobs)
    assert jobs[0] == "src=f0.png refs=r.png bds=2 out=%s/f0_r_2.00.png" % str(tmp_path / "out")
    assert _plan(tmp_path, MIXED, "-tau", "0.5", "-sigma", "4") == jobs                                    # the two knobs alone change nothing


@pytest.mark.parametrize("extra,word", [(("-fullres", "1"), "-fullres 1"), (("-vis", "1"), "-vis 1"), (("-tau", "1.0"), "-tau"), (("-tau", "-0.1"), "-tau"),
                                        (("-sigma", "0"), "-sigma"), (("-sigma", "-3"), "-sigma")])
def test_cli_refuses_at_startup(tmp_path, extra, word):
    r = _run(tmp_path, MIXED[:2], "-seq", "1", *extra)
    assert r.returncode != 0
    assert "Error:" in r.stdout and word in r.stdout and "@@JOB" not in r.stdout
    assert not (tmp_path / "out").exists()
