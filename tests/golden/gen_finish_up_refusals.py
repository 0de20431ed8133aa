"""Generates tests/golden/finish_up_refusals.json: the message of every refused call in the table of tests/test_gpu_finish_refusals.py. Needs a GPU.

    NCT_LIB=<libnct.so of the commit before the change> python tests/golden/gen_finish_up_refusals.py [--out <file>]

The fixture pins the messages ACROSS a change of the entry points, so it is recorded from the library of the commit BEFORE that change (NCT_LIB), never from the
code under test. It was recorded from the library before the four forms got one check, whose host entry points worded the limits on their own; REWORDED below
turns those fragments into the one wording that is left (the launchers', formatted from the constants), and nothing else was edited."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "neural-color-transfer_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "tests"))

REWORDED = [("outside [1x1, 16384 per side, 2^26 px]", "outside [1x1, 16384 per side, 67108864 px]"),
            ("above 16384 per side or 2^26 pixels", "above 16384 per side or 67108864 pixels")]


def main():
    import nct
    import test_gpu_finish_refusals as t
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "finish_up_refusals.json")
    with nct.Context(0) as c:
        got = t.run_rows(c)
    golden, edits = {}, 0
    for key, (rc, msg, taken) in got.items():
        assert rc == -2 and msg and taken == 0, (key, rc, msg, taken)
        for old, new in REWORDED:
            edits += old in msg
            msg = msg.replace(old, new)
        golden[key] = msg
    with open(out, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d rows from %s, %d reworded" % (len(golden), nct.LIB_PATH, edits))


if __name__ == "__main__":
    main()
