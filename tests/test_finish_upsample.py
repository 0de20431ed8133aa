"""The upsampling finish (SPEC §6.8) without a GPU: the library exports its entry points, the CLI's -fullres takes 0 / 1 / 2 and refuses the rest before any work, and
the oracle-side composition the GPU tests compare against (tests/finish_up_ref.py) reproduces the exact finish's bytes where both are defined to agree."""
import os
import subprocess
import numpy as np
import pytest

import nct
import synth
from finish_up_ref import oracle_finish_upsample, clamp_inputs
from fullres_ref import oracle_finish, smooth_ab

BIN = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")


def test_library_exports_the_new_symbols():
    l = nct.lib()
    for name in ("nct_color_finish_upsample", "nct_color_finish_upsample_dev", "nct_process_pair_fullres_finish"):
        assert name in nct.SIGNATURES and getattr(l, name) is not None
    assert (nct.FINISH_EXACT, nct.FINISH_UPSAMPLE) == (0, 1)
    assert l.nct_version() == nct.NCT_VERSION == 118


def test_fullres_help_line_names_the_second_finish():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("-fullres: ")]
    assert len(lines) == 1 and lines[0].startswith("-fullres: (default=0) [extension] ") and "2 = " in lines[0], lines


@pytest.mark.parametrize("args,flag", [(("-fullres", "3"), "-fullres"), (("-fullres", "-1"), "-fullres"), (("-fullres", "2", "-vis", "1"), "-fullres 2"),
                                       (("-fullres", "2", "-lut", "33", "-lutfull", "1"), "-fullres 2")])
def test_cli_refuses_at_startup(tmp_path, args, flag):
    r = subprocess.run([BIN, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"), *args], capture_output=True, text=True)
    assert r.returncode != 0 and "Error:" in r.stdout and flag in r.stdout and "@@JOB" not in r.stdout, r.stdout
    assert not (tmp_path / "out").exists()


def test_cli_fullres_2_refuses_several_references(tmp_path):
    inp = tmp_path / "in"; inp.mkdir()
    (inp / "pairs.txt").write_text("a.png b.png,c.png 2.0\n")
    r = subprocess.run([BIN, "--plan-only", "-i", str(inp), "-o", str(tmp_path / "out"), "-fullres", "2"], capture_output=True, text=True)
    assert "-fullres 2 cannot be combined with several references" in r.stdout, r.stdout


@pytest.mark.parametrize("form", [0, 1])
def test_composition_equals_the_exact_finish_at_the_working_size(oracle, form):
    """target == working size: the exact finish's U1 is a copy, so its A1 on its own ab_wls is what the composition computes"""
    h, w = 37, 29
    s = synth.image(77, h, w)
    exp, st = oracle_finish(oracle, smooth_ab(78, h, w), h, w, h, w, s, form)
    got, lab = oracle_finish_upsample(oracle, st["ab_wls"], h, w, s, form)
    assert np.array_equal(lab, st["lab"]) and np.array_equal(got, exp)


def test_clamp_case_clamps_on_both_sides(oracle):
    """the condition of the GPU clamp case, on the oracle's output: at least 1 % of the expected Lab bytes are 0 and at least 1 % are 255"""
    ab, h, w, s = clamp_inputs()
    _, lab = oracle_finish_upsample(oracle, ab, h, w, s)
    print("clamp case: %.1f %% zeros, %.1f %% 255" % (100 * (lab == 0).mean(), 100 * (lab == 255).mean()))
    assert (lab == 0).mean() >= 0.01 and (lab == 255).mean() >= 0.01
