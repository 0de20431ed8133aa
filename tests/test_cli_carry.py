"""The console driver's -carry 1 -carryiters n (SPEC §6.23) on the GPU: the files of a three-line pairs.txt equal the binding's frames of the same sequence."""
import os
import subprocess
import numpy as np
import pytest
from PIL import Image

import nct
import seq_mc_ref
import seq_ref
import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "neural-color-transfer_amd", "bin", "neural_color_transfer")
H, W = 56, 64
REF = (2000, 60, 72)
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)


def test_cli_carry(tmp_path, ctx):
    from caffemodel_io import synthetic_vgg19, write_caffemodel
    ws, bs = synthetic_vgg19(19)
    ctx.vgg19_load_raw(ws, bs)
    frames = seq_ref.pan_frames(3, H, W, step=2)
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    inp = tmp_path / "in"; inp.mkdir()
    save = lambda name, img: Image.fromarray(img[..., ::-1].copy()).save(inp / name)
    read = lambda p: np.asarray(Image.open(p).convert("RGB"))[..., ::-1]
    save("r.png", synth.image(*REF))
    for t in range(3):
        save("f%d.png" % t, frames[t])
    (inp / "pairs.txt").write_text("".join("f%d.png r.png 2.0\n" % t for t in range(3)))

    def run(out, *extra):
        res = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(out), "-g", "0", "-seq", "1", "-motion", "1", "-levels", "2", *extra], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout, [read(out / ("f%d_r_2.00.png" % t)) for t in range(3)]

    p2 = nct.Params.default(); p2.bds_weight = 2.0; p2.levels = 2; p2.flags = nct.FLAG_LATENCY
    exp = {}
    for carry in (None, 2):
        try:
            ctx.seq_begin(synth.image(*REF), (H, W, 3), p2)
            ctx.seq_set_motion(*MOT)
            if carry is not None:
                ctx.seq_set_carry(True, carry)
            exp[carry] = [ctx.seq_frame(f) for f in frames]
        finally:
            ctx.seq_end()
    assert not np.array_equal(exp[2][1], exp[None][1])                              # the carry is at work in what the files are compared with
    log, got = run(tmp_path / "o1", "-carry", "1", "-carryiters", "2")
    assert "correspondence carry" in log
    assert all(np.array_equal(a, b) for a, b in zip(got, exp[2]))
    log0, got0 = run(tmp_path / "o2")
    assert "correspondence carry" not in log0
    assert all(np.array_equal(a, b) for a, b in zip(got0, exp[None]))
