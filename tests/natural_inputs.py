"""Natural-image test inputs.

The tests use committed STAND-INS of the reference's ten demo photographs (demo/example/in/{in,tar}{0,1,2,3,4}.png): tests/golden/standin/*.png, written by
tests/golden/gen_natural_standin.py with what natural photographs have and cosines + noise do not (large groups of one colour, isolated colours, one-pixel edges),
the demo's colour types and a third of its sizes, plus the oracle's fixtures on them (tests/golden/standin/pair_<case>.npz, tests/golden/gen_natural.py). require()
returns that directory and fails when it is incomplete: the tests never depend on files outside the repository.

The photographs themselves (third-party images of unknown licence) are never committed. Where a source directory exists ($NCT_DEMO_DIR, else the reference's
demo/example/in) stage() copies them byte for byte into tests/golden/natural/ (git-ignored); __graft_entry__.build() runs it, and bench.py's `natural` key measures them
when they are there."""
import os
import shutil

NAMES = ("in0", "in1", "in2", "in3", "in4", "tar0", "tar1", "tar2", "tar3", "tar4")
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "natural")
STANDIN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "standin")


def source_dir():
    for d in (os.environ.get("NCT_DEMO_DIR"), "/root/reference/demo/example/in"):
        if d and all(os.path.exists(os.path.join(d, n + ".png")) for n in NAMES):
            return d
    return None


def present():
    return all(os.path.exists(os.path.join(DIR, n + ".png")) for n in NAMES)


def stage():
    """copies the ten photographs from the source directory if they are not there yet; returns True when they are present afterwards"""
    src = source_dir()
    if src and not present():
        os.makedirs(DIR, exist_ok=True)
        for n in NAMES:
            shutil.copyfile(os.path.join(src, n + ".png"), os.path.join(DIR, n + ".png"))
    return present()


def require():
    """the committed stand-in directory (images + oracle fixtures); raises when any stand-in image is missing"""
    missing = [n for n in NAMES if not os.path.exists(os.path.join(STANDIN_DIR, n + ".png"))]
    if missing:
        raise FileNotFoundError(f"stand-in images missing from {STANDIN_DIR}: {missing} (python tests/golden/gen_natural_standin.py)")
    return STANDIN_DIR


if __name__ == "__main__":
    print("staged" if stage() else "no source directory: nothing staged", DIR)
