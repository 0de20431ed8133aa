"""Correspondence carry (SPEC §6.23) without a GPU: the numpy rules (tests/seq_carry_ref.py) against scalar python loops, the identities of the moves and of the
composition, what the feature is for (less flicker without the blend, a two-iteration sequence close to the ten-iteration one with it), the surface of the library and
the binding, and the console driver's -carry options through its --plan-only hook."""
import ctypes
import os
import subprocess
import numpy as np
import pytest

import nct
import seq_carry_ref as ref
import seq_mc_ref
import seq_prop_ref
import seq_ref
import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "neural-color-transfer_amd", "bin", "neural_color_transfer")
KINDS = ("random", "outside", "shift", "zero")


def test_library_and_binding_have_the_entry_points():
    l = ctypes.CDLL(nct.LIB_PATH)
    for name in ("nct_seq_set_carry", "nct_seq_get_carry", "nct_nnf_carry", "nct_nnf_forward_map", "nct_nnf_remap", "nct_nnf_merge"):
        assert hasattr(l, name) and name in nct.SIGNATURES, name
    for name in ("nct_nnf_carry_dev", "nct_nnf_forward_map_dev", "nct_nnf_remap_dev", "nct_nnf_merge_dev"):
        assert hasattr(l, name) and name in nct.SIGNATURES, name
    for name in ("seq_set_carry", "seq_get_carry", "nnf_carry", "nnf_forward_map", "nnf_remap", "nnf_merge"):
        assert callable(getattr(nct.Context, name)), name
    assert "6.23" in open(os.path.join(REPO, "include", "nct.h")).read()


# ---- the rules against scalar loops

@pytest.mark.parametrize("grid,rgrid", ref.GRIDS)
def test_numpy_rules_equal_the_scalar_loops(grid, rgrid):
    (h, w), (bh, bw) = grid, rgrid
    seen_holes = seen_many = seen_outside = False
    for kind in KINDS:
        field = ref.field_case(h, w, 7 * h + w, kind)
        a = ref.nnf_case(h, w, bh, bw, 3 * h + w)
        b = ref.nnf_case(bh, bw, h, w, 5 * h + w)
        assert np.array_equal(ref.move_a(a, field), ref.loop_move_a(a, field)), kind
        F, holes = ref.loop_forward_map(field)
        got = ref.forward_map(field)
        assert got.dtype == np.uint32 and np.array_equal(got, F), kind
        assert np.array_equal(ref.remap_b(b, got), ref.loop_remap_b(b, F)), kind
        # every word of F addresses the grid
        assert ((got >> 12) < h).all() and ((got & 0xFFF) < w).all()
        f = field.astype(np.int64)
        yy, xx = np.mgrid[0:h, 0:w]
        ty, tx = np.clip(yy + f[..., 0], 0, h - 1), np.clip(xx + f[..., 1], 0, w - 1)
        seen_holes |= holes > 0
        seen_many |= len(np.unique(ty * w + tx)) < h * w
        seen_outside |= bool(((yy + f[..., 0] < 0) | (yy + f[..., 0] >= h) | (xx + f[..., 1] < 0) | (xx + f[..., 1] >= w)).any())
    assert seen_holes and seen_many and seen_outside                 # the cases reach holes, several p on one s, and vectors that leave the grid


@pytest.mark.parametrize("grid,rgrid", ref.GRIDS)
def test_a_zero_field_moves_nothing(grid, rgrid):
    (h, w), (bh, bw) = grid, rgrid
    zero = ref.field_case(h, w, 0, "zero")
    a, b = ref.nnf_case(h, w, bh, bw, 1), ref.nnf_case(bh, bw, h, w, 2)
    yy, xx = np.mgrid[0:h, 0:w]
    assert np.array_equal(ref.move_a(a, zero), a)
    assert np.array_equal(ref.forward_map(zero), ref.word(yy, xx))
    assert np.array_equal(ref.remap_b(b, ref.forward_map(zero)), b)


def test_a_remapped_field_follows_a_shift():
    """a uniform shift: B'(q) names the pixel that now shows what B(q) showed, wherever that pixel is inside the grid"""
    h, w, bh, bw = 12, 15, 7, 9
    field = np.broadcast_to(np.array([2, -3], np.int16), (h, w, 2)).copy()         # frame t at p shows what frame t-1 showed at p + (2, -3)
    b = ref.nnf_case(bh, bw, h, w, 4)
    by, bx = (b >> 12).astype(int), (b & 0xFFF).astype(int)
    got = ref.remap_b(b, ref.forward_map(field))
    inside = (by - 2 >= 0) & (bx + 3 < w) & (by < h - 1) & (bx > 0)              # the bottom row and the left column also collect the clamped vectors: the minimum decides there
    assert inside.any() and np.array_equal(got[inside], ref.word(by - 2, bx + 3)[inside])


def test_merge_rule():
    z = np.arange(12, dtype=np.uint32).reshape(3, 4)
    c = z + 100
    dz = np.array([[0, 1, 2, np.nan], [1, 1, 1, 1], [np.inf, -1, 0, 5]], np.float32)
    dc = np.array([[1, 1, 1, 0], [np.nan, 1, 0.5, 2], [3, -1, -0.0, np.nan]], np.float32)
    start, gz, gc = ref.merge(lambda f: dz if f is z else dc, z, c)
    take = np.array([[0, 0, 1, 0], [0, 0, 1, 0], [1, 0, 0, 0]], bool)                   # strictly smaller only; any NaN keeps Z; -0.0 is not below 0.0
    assert np.array_equal(start, np.where(take, c, z)) and gz is not None and gc is not None
    same, _, _ = ref.merge(lambda f: dz, z, z)
    assert np.array_equal(same, z)


# ---- the composition

@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


SRC, REF = (1000, 64, 56), (1001, 48, 64)
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_first_frame_is_the_plain_sequences(oracle, weights):
    """identity 8(b) and test 4: carry on with carry_iters = pm_iters, first frame only, equals seq_ref.sequence; so does the frame after a reset"""
    ws, bs = weights
    rimg = synth.image(*REF)
    frames = seq_ref.pan_frames(2, SRC[1], SRC[2], step=2)
    exp, _ = seq_ref.sequence(oracle, frames[:1], rimg, ws, bs)
    outs, keeps, carries = ref.sequence(oracle, frames[:1], rimg, ws, bs, carry=True, carry_iters=10)
    assert np.array_equal(outs[0], exp[0]) and keeps[0]["dz_a"][0] is None and len(carries[0]) == 5
    R = seq_ref.prepare_reference(oracle, rimg, ws, bs)
    again, _, _, _ = ref.frame(oracle, frames[0], R, ws, bs, None, None, seq_ref.TAU, seq_ref.SIGMA, carry_iters=2)      # after a reset: no state, no kept fields
    assert np.array_equal(again, exp[0])


def test_composition_identities(oracle, weights):
    """8(c): per query the level's final distance is at most min(d_Z, d_C), and on identical frames level 0's distances never rise; 8(d): with carry_iters = 0 the
    reported field is the start field and its distances are the minimum's operands. Two levels keep the test short"""
    ws, bs = weights
    rimg = synth.image(*REF)
    frames = seq_ref.pan_frames(3, SRC[1], SRC[2], step=2)
    for it in (2, 0):
        outs, keeps, _ = ref.sequence(oracle, frames, rimg, ws, bs, carry_iters=it, mot=MOT, levels=2)
        for t in (1, 2):
            for l in range(2):
                dz, dc, d = keeps[t]["dz_a"][l], keeps[t]["dc_a"][l], keeps[t]["annd"][l]
                ok = ~(np.isnan(dz) | np.isnan(dc))
                assert (d[ok] <= np.minimum(dz, dc)[ok]).all(), (it, t, l)
                if it == 0:
                    assert np.array_equal(keeps[t]["ann"][l], keeps[t]["start_a"][l]) and np.array_equal(keeps[t]["bnn"][l], keeps[t]["start_b"][l])
                    assert np.array_equal(fbits(d[ok]), fbits(np.minimum(dz, dc)[ok]))
        assert any((keeps[t]["dc_a"][l] < keeps[t]["dz_a"][l]).any() for t in (1, 2) for l in range(2))       # the kept match wins somewhere
    same = [frames[0]] * 3
    _, keeps, _ = ref.sequence(oracle, same, rimg, ws, bs, carry_iters=2, levels=1)
    assert (keeps[1]["annd"][0] <= keeps[0]["annd"][0]).all() and (keeps[2]["annd"][0] <= keeps[1]["annd"][0]).all()


def test_carry_off_is_the_motion_sequence(oracle, weights):
    ws, bs = weights
    rimg = synth.image(*REF)
    frames = seq_ref.pan_frames(2, SRC[1], SRC[2], step=2)
    exp, _ = seq_mc_ref.sequence(oracle, frames, rimg, ws, bs, mot=MOT, levels=2)
    outs, _, _ = ref.sequence(oracle, frames, rimg, ws, bs, carry=False, mot=MOT, levels=2)
    assert all(np.array_equal(a, b) for a, b in zip(outs, exp))


def test_what_the_carry_is_for(oracle, weights):
    """seq_ref.static_frames(4, 64, 56), reference synth.image(1001, 48, 64), motion off; both sides deterministic CPU results.
    tau = 0: the transform flicker with the carry at ten iterations is strictly below the sequence without it (the issue's scratch run: 2.3106 against 2.5474).
    tau = 0.7: every frame of the two-iteration carry stays above 45 dB from the sequence without the carry (the scratch run's minimum: 48.9 dB; the threshold leaves
    3.9 dB for a composition that differs from it in a detail the rules allow). The figures of this composition are printed and recorded in DESIGN.md §3.28"""
    ws, bs = weights
    rimg = synth.image(*REF)
    frames = seq_ref.static_frames(4, SRC[1], SRC[2])
    plain0, _, _ = ref.sequence(oracle, frames, rimg, ws, bs, carry=False, tau=0.0)
    carry0, _, _ = ref.sequence(oracle, frames, rimg, ws, bs, carry_iters=10, tau=0.0)
    f_plain, f_carry = seq_ref.transform_flicker(plain0, frames), seq_ref.transform_flicker(carry0, frames)
    print("static scene, tau 0: transform flicker without the carry %.4f, carry 10 %.4f" % (f_plain, f_carry))
    plain7, _, _ = ref.sequence(oracle, frames, rimg, ws, bs, carry=False)
    carry7, _, _ = ref.sequence(oracle, frames, rimg, ws, bs, carry_iters=2)
    db = [seq_prop_ref.psnr(a, b) for a, b in zip(carry7[1:], plain7[1:])]
    print("static scene, tau 0.7: PSNR of carry 2 against no carry, frames 1-3: %s dB; transform flicker %.4f / %.4f"
          % (", ".join("%.1f" % d for d in db), seq_ref.transform_flicker(plain7, frames), seq_ref.transform_flicker(carry7, frames)))
    assert np.array_equal(carry7[0], plain7[0])
    assert f_carry < f_plain
    assert min(db) > 45.0


# ---- console driver

LINES = ["f0.png r.png 2.0", "f1.png r.png 2.0", "f2.png r.png 2"]


def _run(tmp_path, *extra):
    inp = tmp_path / "in"; inp.mkdir(exist_ok=True)
    (inp / "pairs.txt").write_text("".join(l + "\n" for l in LINES))
    return subprocess.run([BIN, "--plan-only", "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(tmp_path / "out"), *extra], capture_output=True, text=True)


def test_cli_plan_with_the_carry_is_the_sequence_plan(tmp_path):
    jobs = lambda r: [l for l in r.stdout.splitlines() if l.startswith("@@JOB ")]
    base = _run(tmp_path, "-seq", "1")
    assert base.returncode == 0 and len(jobs(base)) == 3
    for extra in (("-carry", "1"), ("-carry", "1", "-carryiters", "2"), ("-carry", "1", "-carryiters", "0"), ("-carry", "1", "-carryiters", "64"), ("-carry", "0")):
        r = _run(tmp_path, "-seq", "1", *extra)
        assert r.returncode == 0 and jobs(r) == jobs(base), r.stdout + r.stderr


@pytest.mark.parametrize("extra,word", [(("-carry", "1"), "-carry 1"), (("-seq", "1", "-carryiters", "2"), "-carryiters"), (("-seq", "1", "-carry", "0", "-carryiters", "2"), "-carryiters"),
                                        (("-seq", "1", "-carry", "1", "-carryiters", "65"), "-carryiters"), (("-seq", "1", "-carry", "1", "-carryiters", "-1"), "-carryiters"), (("-seq", "1", "-carry", "1", "-carryiters", "-2"), "-carryiters"),
                                        (("-seq", "1", "-carryiters", "-2"), "-carryiters"),
                                        (("-seq", "1", "-carry", "2"), "-carry")])
def test_cli_refuses_at_startup(tmp_path, extra, word):
    r = _run(tmp_path, *extra)
    assert r.returncode != 0
    assert "Error:" in r.stdout and word in r.stdout and "@@JOB" not in r.stdout
    assert not (tmp_path / "out").exists()
