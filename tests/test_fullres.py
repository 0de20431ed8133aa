"""Full-resolution output (SPEC §6.1), the parts that need no GPU: the working-size rule of nct_working_size against a float32 restatement of the CLI's
shrink, its refusals, and the CLI's -fullres flag."""
import os
import subprocess
import pytest

import nct
from fullres_ref import working_size

BIN = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")


def _sizes():
    out = [(1100, 700), (700, 1100), (1000, 1000), (1001, 1000), (1000, 1001), (999, 17), (4000, 3000), (6000, 4000), (4000, 6000), (3024, 4032),
           (16384, 1000), (1000, 16384), (16384, 279), (16384, 278), (8192, 8192), (8193, 8192), (16385, 100), (100, 16385), (16384, 4096), (16384, 4097),
           (17, 17), (16, 500), (500, 16), (1, 1), (0, 5), (5, 0), (2, 3000)]
    for h in (17, 18, 333, 640, 999, 1000, 1001, 1023, 1500, 2047, 3000, 4095, 4097, 7777, 12345, 16384):
        for w in (17, 31, 480, 777, 1000, 1001, 1999, 2500, 4000, 6001, 9999, 16384):
            out.append((h, w))
    return out


@pytest.mark.parametrize("max_side", [17, 128, 1000, 1234, 4000])
def test_working_size_matches_the_cli_rule(max_side):
    n_ok = n_refused = 0
    for h, w in _sizes():
        exp = working_size(h, w, max_side)
        if exp is None:
            with pytest.raises(nct.NctError) as e:
                nct.working_size(h, w, max_side)
            assert e.value.code == -2 and str(e.value).split(": ", 1)[1], (h, w, max_side)
            n_refused += 1
        else:
            assert nct.working_size(h, w, max_side) == exp, (h, w, max_side)
            n_ok += 1
    assert n_ok > 0 and n_refused > 0


def test_working_size_examples():
    assert nct.working_size(1100, 700) == (1000, 636)             # the CLI's own shrink of the same JPEG (tests/test_cli.py)
    assert nct.working_size(700, 1100) == (636, 1000)
    assert nct.working_size(999, 1000) == (999, 1000)             # nothing shrinks at max_side
    assert nct.working_size(4000, 6000) == (666, 1000)
    assert nct.working_size(16384, 1000) == (1000, 61)
    assert nct.working_size(300, 220, 128) == (128, 93)


@pytest.mark.parametrize("h,w,max_side", [(16385, 100, 1000), (100, 16385, 1000), (8193, 8192, 1000), (16384, 200, 1000), (200, 16384, 1000),
                                          (500, 500, 16), (500, 500, 4001), (0, 10, 1000), (10, 10, 1000), (5000, 40, 1000)])
def test_working_size_refusals(h, w, max_side):
    assert working_size(h, w, max_side) is None
    with pytest.raises(nct.NctError) as e:
        nct.working_size(h, w, max_side)
    assert e.value.code == -2


def test_cli_fullres_help_line_is_an_extension():
    r = subprocess.run([BIN, "-h"], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("-fullres: ")]
    assert len(lines) == 1, r.stdout
    assert lines[0].startswith("-fullres: (default=0) [extension] "), lines[0]


def test_cli_refuses_fullres_with_vis(tmp_path):
    r = subprocess.run([BIN, "-i", str(tmp_path / "in"), "-o", str(tmp_path / "out"), "-fullres", "1", "-vis", "1"], capture_output=True, text=True)
    assert r.returncode != 0
    assert "-fullres 1 cannot be combined with -vis 1" in r.stdout
    assert not (tmp_path / "out").exists()                        # refused at startup, before anything is created or read
