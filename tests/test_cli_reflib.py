"""The console driver's reference library (SPEC §6.21; -reflib, -refk, -reftap, -refcenter): a pairs.txt line whose style field is "auto" runs with the library's best
entries, its files carry the names and the bytes of the same line with those references written out, the choice is the numpy rule's on the GPU's own taps, and the
three refusals."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import nct
import reflib_ref as R

pytestmark = pytest.mark.gpu

BIN = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")
TAP = 3


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """model/, in/ with two sources, an "auto" line each and the library under in/lib, file names in another order than the textures"""
    from caffemodel_io import synthetic_vgg19, write_caffemodel
    root = tmp_path_factory.mktemp("cli_reflib")
    ws, bs = synthetic_vgg19(19)
    (root / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(root / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    lib = root / "in" / "lib"; lib.mkdir(parents=True)
    names = ["e_diagonal.png", "d_checker.png", "c_hbars.png", "b_vbars.png", "a_dots.png"]
    imgs = dict(zip(names, R.fixture_library()))
    for n, im in imgs.items():
        Image.fromarray(im[..., ::-1].copy()).save(lib / n)
    (lib / "notes.txt").write_text("not an image\n")
    srcs = R.fixture_sources()
    Image.fromarray(srcs[1][..., ::-1].copy()).save(root / "in" / "s1.png")
    Image.fromarray(srcs[3][..., ::-1].copy()).save(root / "in" / "s3.png")
    (root / "in" / "pairs.txt").write_text("s1.png auto 2.0\ns3.png auto 1.0\n")
    return root, (ws, bs), imgs, {"s1": srcs[1], "s3": srcs[3]}


def expected_choice(ctx, oracle, imgs, src, K, centred=True):
    """the numpy rule on the GPU's own taps, the library in byte order of its file names"""
    names = sorted(imgs)
    taps = [ctx.vgg19_features(imgs[n], deepest_tap=TAP)[TAP - 1] for n in names]
    mu = R.library_center(taps) if centred else None
    ents = [R.quantize8(oracle, F, mu) for F in taps]
    o, k, _, _ = R.rank(R.quantize8(oracle, ctx.vgg19_features(src, deepest_tap=TAP)[TAP - 1], mu), ents)
    return [names[i] for i in o[:K]], [int(k[i]) for i in o[:K]]


@pytest.mark.parametrize("K", [1, 2])
def test_auto_line_equals_the_line_written_out(tree, ctx, oracle, K):
    root, (ws, bs), imgs, srcs = tree
    ctx.vgg19_load_raw(ws, bs)
    out = root / ("out%d" % K)
    r = run("-m", str(root / "model"), "-i", str(root / "in"), "-o", str(out), "-reflib", str(root / "in" / "lib"), "-refk", str(K), "-reftap", str(TAP))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Reference library: 5 image(s)" in r.stdout and "at tap 3, centred" in r.stdout
    lines, files = [], []
    for s, w in (("s1", 2.0), ("s3", 1.0)):
        chosen, keys = expected_choice(ctx, oracle, imgs, srcs[s], K)
        assert "Reference library: chose " + ", ".join("%s (key %d)" % (n, k) for n, k in zip(chosen, keys)) + " of 5." in r.stdout, r.stdout
        lines.append("%s.png %s %.1f\n" % (s, ",".join("lib/" + n for n in chosen), w))
        files.append("%s_%s_%2.2f.png" % (s, "+".join(n[:-4] for n in chosen), w))
    # each source ranks its own texture first
    assert files[0].startswith("s1_d_checker") and files[1].startswith("s3_b_vbars")
    assert sorted(os.listdir(out)) == sorted(files + ["status.jsonl"])
    # the same lines with the chosen references written out
    (root / "in" / "pairs.txt").rename(root / "in" / "pairs_auto.txt")
    try:
        (root / "in" / "pairs.txt").write_text("".join(lines))
        out2 = root / ("named%d" % K)
        r2 = run("-m", str(root / "model"), "-i", str(root / "in"), "-o", str(out2))
        assert r2.returncode == 0, r2.stdout + r2.stderr
    finally:
        (root / "in" / "pairs.txt").unlink()
        (root / "in" / "pairs_auto.txt").rename(root / "in" / "pairs.txt")
    assert sorted(os.listdir(out2)) == sorted(os.listdir(out))
    for f in files:
        assert (out / f).read_bytes() == (out2 / f).read_bytes(), f


def test_refusals(tree):
    root = tree[0]
    common = ("-m", str(root / "model"), "-i", str(root / "in"))
    # "auto" without -reflib: the line is refused when its turn comes, the run goes on
    r = run(*common, "-o", str(root / "r0"))
    assert r.returncode == 0 and r.stdout.count('Error: the reference "auto" needs -reflib <dir>') == 2 and sorted(os.listdir(root / "r0")) == ["status.jsonl"], r.stdout
    # -reflib with -seq 1
    r = run(*common, "-o", str(root / "r1"), "-reflib", str(root / "in" / "lib"), "-seq", "1")
    assert r.returncode != 0 and "Error: -reflib cannot be combined with -seq 1" in r.stdout and not (root / "r1").exists()
    # an empty directory (one without an image), and one that is not there
    (root / "empty").mkdir(exist_ok=True); (root / "empty" / "readme.txt").write_text("x\n")
    r = run(*common, "-o", str(root / "r2"), "-reflib", str(root / "empty"))
    assert r.returncode != 0 and "holds no image" in r.stdout and "Set device" not in r.stdout
    r = run(*common, "-o", str(root / "r3"), "-reflib", str(root / "absent"))
    assert r.returncode != 0 and "cannot open the directory" in r.stdout
    for flag, v, word in (("-refk", "0", "-refk 0 is not in [1, 8]"), ("-refk", "9", "-refk 9"), ("-reftap", "6", "-reftap 6 is not in [1, 5]"), ("-refcenter", "2", "-refcenter 2")):
        r = run(*common, "-o", str(root / "r4"), "-reflib", str(root / "in" / "lib"), flag, v)
        assert r.returncode != 0 and word in r.stdout, r.stdout
