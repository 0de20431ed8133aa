"""The console driver's text, pinned: tests/golden/cli_messages.json holds, for a list of argument vectors that need no GPU and no image file, the exit status
and stdout of the driver as it was before its source was split into units (generator: tests/golden/gen_cli_messages.py). The help, every option-check refusal
with its boundary values, the errors in front of the first device call, the job plan of a mixed pairs.txt and the parser's view of the [extension] flags must
come out byte for byte."""
import importlib.util
import json
import os
import subprocess

import nct

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")


def _generator():
    spec = importlib.util.spec_from_file_location("gen_cli_messages", os.path.join(HERE, "golden", "gen_cli_messages.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_cli_host_pieces_under_sanitizers(tmp_path):
    """tests/cli_host_check.cpp: the parser and the refusal rules on the fixture's vectors, split_refs, plan_groups, output_name and Tickets::draw's modulo form,
    built with AddressSanitizer + UBSan as a program of its own and linked without the library (unused sections are dropped: the pieces under test call nothing of it)."""
    fx = json.load(open(os.path.join(HERE, "golden", "cli_messages.json")))
    vectors = tmp_path / "vectors.txt"
    vectors.write_text("".join("\t".join(c["argv"]) + "\n" for c in fx["cases"]))
    host = os.path.join(nct.PKG_ROOT, "host")
    exe = str(tmp_path / "cli_host_check")
    r = subprocess.run(["g++", "-O0", "-g1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffunction-sections", "-Wl,--gc-sections",
                        "-I", host, "-I", os.path.join(nct.PKG_ROOT, "..", "include"), os.path.join(HERE, "cli_host_check.cpp"),
                        *[os.path.join(host, f) for f in ("cli_options.cpp", "cli_job.cpp", "cli_sequence.cpp")], "-o", exe, "-lz"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(vectors)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split("\n")[-2].startswith("vectors %d parsed " % len(fx["cases"]))


def test_cli_prints_what_the_fixture_recorded(tmp_path):
    gen = _generator()
    fx = json.load(open(os.path.join(HERE, "golden", "cli_messages.json")))
    # the fixture is the generator's: same pairs.txt, same vectors in the same order — one refused vector per option check of main(), 36 of them
    assert fx["pairs_txt"] == gen.PAIRS and [(c["section"], c["argv"]) for c in fx["cases"]] == [(s, a) for s, a in gen.vectors()]
    assert sum(c["section"] == "rule" for c in fx["cases"]) == 36
    assert len({c["stdout"] for c in fx["cases"] if c["section"] == "rule"}) == 36
    tmp = os.path.realpath(str(tmp_path))
    gen.stage(tmp)
    for c in fx["cases"]:
        rc, out = gen.run(BIN, tmp, c["argv"])
        assert (rc, out) == (c["rc"], c["stdout"]), c["argv"]
