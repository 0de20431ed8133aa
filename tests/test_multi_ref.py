"""Several references (SPEC §6.2) without a GPU: the numpy selection rule on hand-made maps, the composition of the oracle's stages against oracle.process_pair
for K = 1 and a repeated reference, and the console driver's handling of comma lines through its --plan-only hook."""
import os
import subprocess
import numpy as np
import pytest

import multi_ref
import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "neural-color-transfer_amd", "bin", "neural_color_transfer")


def f32(a):
    return np.asarray(a, np.float32)


def test_select_tie_goes_to_the_lower_index():
    e = f32(np.full((4, 5), -0.5))
    assert not multi_ref.select([e, e.copy(), e.copy()]).any()
    a, b = e.copy(), e.copy()
    b[2, 2] = -0.75                                     # reference 1 is better wherever the window holds (2, 2), tied elsewhere
    lab = multi_ref.select([a, b])
    exp = np.zeros((4, 5), np.uint8); exp[1:4, 1:4] = 1
    assert np.array_equal(lab, exp)
    assert np.array_equal(multi_ref.select([b, a]), 0 * exp)          # the better one first: it wins its window and every tie


def test_select_nan_counts_as_zero_and_a_selected_nan_stays_nan():
    a = f32(np.full((5, 5), -0.25)); b = f32(np.full((5, 5), -0.5))
    b[2, 2] = np.nan
    lab = multi_ref.select([a, b])
    # window sums at (2, 2): a = 9 * -0.25 = -2.25, b = 8 * -0.5 + 0 = -4.0 -> b, although its own centre is NaN
    assert lab[2, 2] == 1 and lab.all()
    g = [np.full((5, 5, 3), 10, np.uint8), np.full((5, 5, 3), 20, np.uint8)]
    G, E = multi_ref.merge(lab, g, [a, b])
    assert np.isnan(E[2, 2]) and E.view(np.uint32)[2, 2] == b.view(np.uint32)[2, 2] and (G == 20).all()
    allnan = f32(np.full((3, 3), np.nan))
    assert not multi_ref.select([allnan, f32(np.zeros((3, 3)))]).any()       # NaN = 0.0 ties with 0.0: lower index
    assert multi_ref.select([allnan, f32(np.full((3, 3), -0.1))]).all()


def test_select_border_pixels_use_only_in_grid_taps():
    a = f32(np.zeros((4, 4))); b = f32(np.zeros((4, 4)))
    a[:] = -0.1                                          # corner window: 4 taps -> -0.4, edge: 6 -> -0.6, inside: 9 -> -0.9
    b[0, 0] = -0.45                                      # only windows holding (0, 0) see it: (0,0), (0,1), (1,0), (1,1)
    lab = multi_ref.select([a, b])
    exp = np.zeros((4, 4), np.uint8); exp[0, 0] = 1      # -0.45 < -0.4 at the corner; -0.45 > -0.6 on the edges; > -0.9 inside
    assert np.array_equal(lab, exp)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (6, 1), (5, 4)])
def test_select_single_reference_and_thin_grids(shape):
    rng = np.random.default_rng(3)
    e = [f32(-rng.random(shape)) for _ in range(3)]
    assert not multi_ref.select(e[:1]).any()
    lab = multi_ref.select(e)
    # brute force, scalar, in the canonical order
    h, w = shape
    for y in range(h):
        for x in range(w):
            sc = []
            for k in range(3):
                acc = 0.0
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if 0 <= y + dy < h and 0 <= x + dx < w:
                            acc += float(e[k][y + dy, x + dx])
                sc.append(acc)
            assert lab[y, x] == sc.index(min(sc))


@pytest.mark.parametrize("levels", [5, 1])
def test_composition_equals_oracle_for_one_and_for_a_repeated_reference(oracle, levels):
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    src, ref = synth.image(1000, 64, 56), synth.image(1001, 48, 64)
    exp = oracle.process_pair(src, ref, ws, bs, params=dict(levels=levels))
    got, lv = multi_ref.multi(oracle, src, [ref], ws, bs, levels=levels)
    assert np.array_equal(got, exp)
    assert len(lv["label"]) == levels and not any(l.any() for l in lv["label"])
    got2, lv2 = multi_ref.multi(oracle, src, [ref, ref], ws, bs, levels=levels)
    assert np.array_equal(got2, exp)
    assert not any(l.any() for l in lv2["label"])


def _plan(tmp_path, lines, *extra):
    inp = tmp_path / "in"; inp.mkdir(exist_ok=True)
    (inp / "pairs.txt").write_text("".join(l + "\n" for l in lines))
    r = subprocess.run([BIN, "--plan-only", "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(tmp_path / "out"), *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    jobs = [l[len("@@JOB "):] for l in r.stdout.splitlines() if l.startswith("@@JOB ")]
    assert not (tmp_path / "out").exists()               # planning creates nothing
    return jobs


def test_cli_plans_comma_lines(tmp_path):
    out = str(tmp_path / "out")
    nine = ",".join("r%d.png" % i for i in range(9))
    eight = ",".join("r%d.png" % i for i in range(8))
    jobs = _plan(tmp_path, ["in/in0.png in/tar0.png,in/tar1.png 2.0", "a.png " + nine + " 1.0", "a.png a.png,,b.png 1.0", "a.png sub/b.jpg 0.5", "a.png " + eight + " 4"])
    assert len(jobs) == 5
    assert jobs[0] == "src=in/in0.png refs=in/tar0.png|in/tar1.png bds=2 out=%s/in0_tar0+tar1_2.00.png" % out
    assert jobs[1].startswith("error=") and "9 references" in jobs[1]
    assert jobs[2].startswith("error=") and "empty reference name" in jobs[2]
    assert jobs[3] == "src=a.png refs=sub/b.jpg bds=0.5 out=%s/a_b_0.50.png" % out          # a single reference: today's %s/%s_%s_%2.2f.png
    assert jobs[4] == "src=a.png refs=%s bds=4 out=%s/a_%s_4.00.png" % (eight.replace(",", "|"), out, "+".join("r%d" % i for i in range(8)))


def test_cli_refuses_fullres_on_a_comma_line_only(tmp_path):
    jobs = _plan(tmp_path, ["a.png b.png,c.png 2.0", "a.png b.png 2.0"], "-fullres", "1")
    assert jobs[0].startswith("error=") and "-fullres" in jobs[0]
    assert jobs[1] == "src=a.png refs=b.png bds=2 out=%s/a_b_2.00.png" % str(tmp_path / "out")
