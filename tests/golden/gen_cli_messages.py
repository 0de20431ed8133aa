"""Generates tests/golden/cli_messages.json: what the console driver prints, and how it exits, for a list of argument vectors that need no GPU and no image
file — the help, every option-check refusal of main() (with the boundary values of the rules that guard a range), the errors in front of the first device
call, the job plan of a mixed pairs.txt under the modes that change it, and the parser's view of the [extension] flags.

    python tests/golden/gen_cli_messages.py [--bin <neural_color_transfer>]

The fixture pins the driver's text ACROSS a change of the driver, so it is written from the binary of the commit BEFORE that change (--bin), never from the code
under test; regenerating it from the changed driver must give the same file. tests/test_cli_messages.py replays it.

Every vector runs with the working directory at a temporary directory that holds in/pairs.txt (PAIRS below) and the empty directory empty/, with relative -i / -o,
so that no line depends on where it ran; the binary's own path (the help's "Running:" line) becomes @@BIN@@ and the temporary directory, should it appear, @@TMP@@."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_BIN = os.path.join(os.path.dirname(os.path.dirname(HERE)), "neural-color-transfer_amd", "bin", "neural_color_transfer")

# a plain line, three references, nine (refused, the run goes on), an empty reference name, four frames of one reference, and the same reference at another weight
PAIRS = ("a.png s.png 2\n"
         "b.png r1.png,r2.png,r3.jpg 1.5\n"
         "c.png r1.png,r2.png,r3.png,r4.png,r5.png,r6.png,r7.png,r8.png,r9.png 2\n"
         "d.png r1.png,,r2.png 2\n"
         "f1.png t.jpg 0.5\nf2.png t.jpg 0.5\nf3.png t.jpg 0.5\nf4.png t.jpg 0.5\n"
         "g.png t.jpg 1\n")
IO = ["-i", "in", "-o", "out"]
PLAN = ["--plan-only"] + IO
SEQ, MOT, AUTO = ["-seq", "1"], ["-seq", "1", "-motion", "1"], ["-seq", "1", "-autokey", "1"]

# main()'s option checks in their order: (the vector that the rule refuses, vectors just inside it, further vectors it refuses: the range's other end and the
# like). `inside` vectors go on to print the plan of PAIRS
RULES = [
    (["-rank", "2", "-world", "2"], [["-rank", "1", "-world", "2"], ["-rank", "0", "-world", "1"]], [["-world", "0"], ["-rank", "-1"]]),
    (["-fullres", "3"], [["-fullres", "0"]], [["-fullres", "-1"]]),
    (SEQ + ["-seqfull", "3"], [SEQ + ["-seqfull", "2"], SEQ + ["-seqfull", "1"]], [SEQ + ["-seqfull", "-1"]]),
    (["-seqfull", "1"], [], [["-seqfull", "2"]]),
    (["-fullres", "2", "-upguide", "2"], [["-fullres", "2", "-upguide", "1"], SEQ + ["-seqfull", "2", "-upguide", "1"]], [["-fullres", "2", "-upguide", "-1"]]),
    (["-upguide", "1"], [], [["-fullres", "1", "-upguide", "1"], SEQ + ["-seqfull", "1", "-upguide", "1"]]),
    (["-upsigma", "0"], [["-upsigma", "1e-150"], ["-upsigma", "1e154"]], [["-upsigma", "1e-170"], ["-upsigma", "1e155"], ["-upsigma", "-1"]]),
    (["-fullres", "1", "-vis", "1"], [["-vis", "1"]], [["-fullres", "2", "-vis", "1"]]),
    (SEQ + ["-fullres", "1"], [], [SEQ + ["-fullres", "2"]]),
    (SEQ + ["-vis", "1"], [], []),
    (SEQ + ["-tau", "1"], [SEQ + ["-tau", "0.999"], SEQ + ["-tau", "0"], ["-tau", "1"]], [SEQ + ["-tau", "-0.001"]]),
    (SEQ + ["-sigma", "0"], [SEQ + ["-sigma", "1e-300"], SEQ + ["-sigma", "1e308"], ["-sigma", "0"]], [SEQ + ["-sigma", "-1"]]),
    (["-motion", "1"], [MOT], []),
    (MOT + ["-mr0", "9"], [MOT + ["-mr0", "8"], MOT + ["-mr0", "0"], SEQ + ["-mr0", "9"]], [MOT + ["-mr0", "-1"]]),
    (MOT + ["-mr", "4"], [MOT + ["-mr", "3"], MOT + ["-mr", "0"], SEQ + ["-mr", "4"]], [MOT + ["-mr", "-1"]]),
    (MOT + ["-mpen", "256"], [MOT + ["-mpen", "255"], MOT + ["-mpen", "0"], SEQ + ["-mpen", "256"]], [MOT + ["-mpen", "-1"]]),
    (["-key", "1001"], [SEQ + ["-key", "1000"], ["-key", "1"]], [["-key", "0"], SEQ + ["-key", "1001"]]),
    (["-key", "2"], [], []),
    (["-autokey", "1"], [], []),
    (AUTO + ["-key", "2"], [AUTO + ["-key", "1"]], []),
    (AUTO + ["-keythr", "766"], [AUTO + ["-keythr", "765"], AUTO + ["-keythr", "0"], SEQ + ["-keythr", "766"]], [AUTO + ["-keythr", "-1"]]),
    (AUTO + ["-keycut", "1002"], [AUTO + ["-keycut", "1001"], AUTO + ["-keycut", "0"], SEQ + ["-keycut", "1002"]], [AUTO + ["-keycut", "-1"]]),
    (AUTO + ["-keychange", "1002"], [AUTO + ["-keychange", "1001"], AUTO + ["-keychange", "0"], SEQ + ["-keychange", "1002"]], [AUTO + ["-keychange", "-1"]]),
    (AUTO + ["-keygap", "1001"], [AUTO + ["-keygap", "1000"], AUTO + ["-keygap", "1"], SEQ + ["-keygap", "1001"]], [AUTO + ["-keygap", "0"]]),
    (["-mask", "m", "-maskprotect", "2"], [["-mask", "m", "-maskprotect", "1"], ["-mask", "m", "-maskprotect", "0"]], [["-mask", "m", "-maskprotect", "-1"]]),
    (["-maskprotect", "1"], [["-refmask", "r", "-maskprotect", "1"]], []),
    (["-refmask", "r", "-fullres", "2"], [["-refmask", "r", "-fullres", "1"]], []),
    (["-refmask", "r"] + SEQ, [["-refmask", "r"]], []),
    (["-mask", "m", "-fullres", "2"], [["-mask", "m", "-fullres", "1"]], []),
    (["-mask", "m"] + SEQ, [["-mask", "m", "-refmask", "r"]], []),
    (["-lut", "4"], [["-lut", n] for n in ("0", "3", "5", "9", "17", "33", "65")], [["-lut", "2"], ["-lut", "66"], ["-lut", "-9"]]),
    (["-lutlambda", "0.5"], [["-lut", "9", "-lutlambda", "0.5"], ["-lut", "9", "/lutlambda", "0"]], []),
    (["-lut", "9", "-lutlambda", "0"], [["-lut", "9", "-lutlambda", "1e-300"], ["-lut", "9", "-lutlambda", "1e308"]], [["-lut", "9", "-lutlambda", "-1"], ["-lut", "9", "-lutlambda"]]),
    (["-lutfull", "1"], [["-lut", "9", "-lutfull", "1"]], []),
    (["-lut", "9", "-lutfull", "1", "-fullres", "1"], [], [["-lut", "9", "-lutfull", "1", "-fullres", "2"]]),
    (["-lut", "9", "-lutfull", "1"] + SEQ + ["-seqfull", "1"], [["-lut", "9", "-lutfull", "1"] + SEQ], [["-lut", "9", "-lutfull", "1"] + SEQ + ["-seqfull", "2"]]),
]
# vectors that break two rules: the earlier rule answers
ORDER = [["-fullres", "3", "-seqfull", "3"], ["-seqfull", "1", "-upguide", "1"], SEQ + ["-vis", "1", "-fullres", "1"], ["-motion", "1", "-key", "2"],
         ["-autokey", "1", "-key", "2"], ["-lutfull", "1", "-lutlambda", "1"], ["-mask", "m", "-refmask", "r", "-fullres", "2"], ["-maskprotect", "1", "-lut", "4"],
         ["-rank", "1", "-lut", "4"], ["-key", "0", "-autokey", "1"]]
PLANS = [[], SEQ, SEQ + ["-key", "3"], AUTO, ["-fullres", "1"], ["-fullres", "2"], SEQ + ["-key", "2", "-rank", "1", "-world", "2"], ["-o", "elsewhere/deep"]]
# every [extension] flag away from its default, then the help: it prints each flag with the value parsed so far
EXT = ["-gpus", "3", "-inflight", "4", "-io", "5", "-pin", "0", "-seed", "7", "-levels", "2", "-resume", "1", "-vis", "1", "-fullres", "2", "-procs", "2", "-world", "3",
       "-rank", "2", "-rccl", "1", "-steal", "1", "-feat16", "1", "-seq", "1", "-seqfull", "2", "-upguide", "1", "-upsigma", "12.5", "-tau", "0.25", "-sigma", "7.5",
       "-motion", "1", "-mr0", "5", "-mr", "2", "-mpen", "9", "-key", "4", "-autokey", "1", "-keythr", "30", "-keycut", "400", "-keychange", "50", "-keygap", "12",
       "-lut", "17", "-lutlambda", "0.25", "-mask", "/masks/of the run", "-refmask", "rm", "-maskprotect", "1", "-lutfull", "1"]
PARSE = [EXT + ["-h"], ["--parse-only"] + EXT, ["--parse-only"] + EXT + ["-?"], ["--parse-only", "-mask", "-refmask", "x", "-lut", "-h"],
         ["--parse-only", "-tau", "-.5", "-mr0", "-3", "-upsigma", "abc", "-key", "12abc", "stray", "-m", "/models", "/help"], ["--parse-only", "-gpus", "2", "-nosuch", "1"]]


def vectors():
    """(section, argv) of every run, in the fixture's order."""
    v = [("help", ["-h"]), ("help", ["-zzz", "1"])]
    for refused, inside, more in RULES:
        v.append(("rule", PLAN + refused))
        v += [("inside", PLAN + a) for a in inside] + [("outside", PLAN + a) for a in more]
    v += [("order", PLAN + a) for a in ORDER]
    v += [("error", ["--plan-only", "-i", "empty", "-o", "out"]), ("error", ["-i", "empty", "-o", "out"]),
("error", IO + ["-procs", "2", "-world", "2"]), ("error", IO + ["-procs", "2", "-world", "2", "-steal", "1"])]
    v += [("plan", PLAN + a) for a in PLANS]
    v += [("parse", a) for a in PARSE]
    return v


def stage(tmp):
    os.makedirs(os.path.join(tmp, "in")); os.makedirs(os.path.join(tmp, "empty"))
    with open(os.path.join(tmp, "in", "pairs.txt"), "w") as f:
        f.write(PAIRS)


def run(binary, tmp, argv):
    r = subprocess.run([binary] + argv, cwd=tmp, capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout.replace(binary, "@@BIN@@").replace(tmp, "@@TMP@@")


def main():
    binary = os.path.abspath(sys.argv[sys.argv.index("--bin") + 1] if "--bin" in sys.argv else DEFAULT_BIN)
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = os.path.realpath(tmp)
        stage(tmp)
        for section, argv in vectors():
            rc, out = run(binary, tmp, argv)
            cases.append({"section": section, "argv": argv, "rc": rc, "stdout": out})
    errors = lambda sections: {l for c in cases if c["section"] in sections for l in c["stdout"].split("\n") if l.startswith("Error:")}
    # every rule answers its own vector with a text of its own; the vectors just inside pass every rule; the others are refused as well
    assert len(RULES) == 36 and len(errors({"rule"})) == len(RULES), (len(RULES), len(errors({"rule"})))
    for c in cases:
        refused = c["stdout"].startswith("Error:") and c["stdout"].count("\n") == 1 and c["rc"] == 255
        assert refused == (c["section"] in ("rule", "outside", "order", "error")) or c["section"] in ("help", "parse"), c
        assert c["section"] not in ("inside", "plan") or (c["rc"] == 0 and c["stdout"].count("@@JOB") == PAIRS.count("\n")), c
    assert "@@TMP@@" not in "".join(c["stdout"] for c in cases)
    with open(os.path.join(HERE, "cli_messages.json"), "w") as f:
        json.dump({"generator": "tests/golden/gen_cli_messages.py", "pairs_txt": PAIRS, "cases": cases}, f, indent=1)
        f.write("\n")
    print("%d vectors, %d distinct Error lines (%d from the %d rules)" % (len(cases), len(errors({"rule", "outside", "order", "error"})), len(errors({"rule"})), len(RULES)))


if __name__ == "__main__":
    main()
