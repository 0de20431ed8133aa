"""Full-resolution sequences (SPEC §6.9) without a GPU: the export, the CLI's -seqfull flag and its refusals, and the conditions the GPU tests rely on, asserted on the
reference side: the working sizes of the clip and a plan of the shrunk frames that holds a propagated frame, a key frame and a cut."""
import os
import subprocess
import pytest

import nct
import finish_up_ref as fr
import seq_auto_ref as ar
import seq_mc_ref
import synth
from fullres_ref import working_size

BIN = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")


def test_library_exports_seq_begin_fullres():
    assert "nct_seq_begin_fullres" in nct.SIGNATURES and nct.lib().nct_seq_begin_fullres is not None


def test_seqfull_help_line_is_an_extension():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("-seqfull: ")]
    assert len(lines) == 1 and lines[0].startswith("-seqfull: (default=0) [extension] "), lines


@pytest.mark.parametrize("args,flag", [(("-seqfull", "1"), "-seqfull"), (("-seq", "1", "-seqfull", "3"), "-seqfull"), (("-fullres", "3"), "-fullres"),
                                       (("-seq", "1", "-seqfull", "1", "-lut", "33", "-lutfull", "1"), "-seqfull"), (("-fullres", "2", "-vis", "1"), "-fullres"),
                                       (("-seq", "1", "-fullres", "1"), "-seqfull")])
def test_cli_refuses_at_startup(tmp_path, args, flag):
    r = subprocess.run([BIN, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"), *args], capture_output=True, text=True)
    assert r.returncode != 0 and "Error:" in r.stdout and flag in r.stdout and "@@JOB" not in r.stdout, r.stdout
    assert not (tmp_path / "out").exists()


def test_seq_with_fullres_keeps_its_words(tmp_path):
    r = subprocess.run([BIN, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"), "-seq", "1", "-fullres", "1"], capture_output=True, text=True)
    assert r.returncode != 0 and "Error: -seq 1 cannot be combined with -fullres 1 (a sequence runs at the working size only)." in r.stdout, r.stdout


def test_the_clip_of_the_gpu_tests(oracle):
    assert working_size(*fr.FRAME, fr.MAX_SIDE) == fr.WORK and working_size(*fr.REF[1:], fr.MAX_SIDE) == (53, 64)
    assert working_size(*fr.FRAME, 1000) == fr.FRAME                                            # the identity run shrinks nothing
    mot = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
    shrunk = [oracle.resize_u8c3(f, *fr.WORK) for f in fr.auto_clip()]
    p = ar.plan(oracle, shrunk, 5, mot, fr.AUTO)
    print("auto clip:", ar.kinds(p), [(d["changed"], d["pixels"]) for d in p])
    assert ar.kinds(p) == "FPKPCP"
