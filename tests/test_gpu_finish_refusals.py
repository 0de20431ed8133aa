"""What the eight upsampling-finish entry points refuse (SPEC §6.8, §6.10, §6.13 rule 4): one table of bad calls on tiny blocks, each through every symbol it applies to
with that symbol's own argument list. Every row: NCT_ERR_INVALID, the message byte for byte as recorded in tests/golden/finish_up_refusals.json
(tests/golden/gen_finish_up_refusals.py), and the arena's byte counter where it was — a refused call reserves nothing. The rows with two faults pin the order of
the checks: the earlier check answers. The context is the test's own: every block of a fresh arena is in use (the device blocks below), so a reservation in front of
a refusal would have to grow it."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finish_up_refusals.json")
h, w, H, W = 4, 5, 9, 11                      # a 4 x 5 grid to a 9 x 11 target

# the argument lists after the context, in the symbols' own order; the _dev forms take the same lists on device blocks
ARGS = {
    "nct_color_finish_upsample": ["ab", "h", "w", "s", "H", "W", "prm", "out"],
    "nct_color_finish_guided": ["ab", "lab", "h", "w", "s", "H", "W", "guided", "prm", "out"],
    "nct_color_finish_upsample_region": ["ab", "h", "w", "s", "H", "W", "mask", "region", "prm", "out"],
    "nct_color_finish_guided_region": ["ab", "lab", "h", "w", "s", "H", "W", "mask", "region", "guided", "prm", "out"],
}
ARGS.update({k + "_dev": v for k, v in list(ARGS.items())})
# mask and region are pointers too, but NULL is a value of theirs (the unmasked call; protect = 0): tests/test_gpu_seq_region.py holds those to the unmasked results
MUST_POINT = ("ab", "lab", "s", "guided", "prm", "out")
CONDITIONS = [("null " + p, {p: None}) for p in MUST_POINT] + [
    ("h = 0", {"h": 0}), ("w = W = 16385", {"w": 16385, "W": 16385}), ("H = h - 1", {"H": h - 1}), ("W = w - 1", {"W": w - 1}), ("H = 16385", {"H": 16385}),
    ("protect = 2", {"protect": 2}), ("sigma = 0", {"sigma": 0.0}),
    # two faults: a null pointer answers before protect, protect before the grid, the target before sigma
    ("null ab, protect = 2", {"ab": None, "protect": 2}), ("protect = 2, h = 0", {"protect": 2, "h": 0}), ("sigma = 0, H = 16385", {"sigma": 0.0, "H": 16385})]
# a condition applies to the symbols that take its argument
NEEDS = {"protect = 2": "region", "sigma = 0": "guided", "null ab, protect = 2": "region", "protect = 2, h = 0": "region", "sigma = 0, H = 16385": "guided"}


def rows():
    for name, args in ARGS.items():
        for cond, change in CONDITIONS:
            if NEEDS.get(cond, next(iter(change))) in args:
                yield name, cond, change


def run_rows(c):
    """every row on context c -> {"symbol | condition": [code, message, arena bytes taken by the call]}"""
    l = C.CDLL(nct.LIB_PATH)                  # handles of its own: every pointer argument a plain address, so that it can be NULL
    l.nct_last_error.restype = C.c_char_p
    host = {"ab": np.zeros(6 * h * w), "lab": np.zeros(3 * h * w, np.uint8), "s": np.zeros(3 * H * W, np.uint8), "mask": np.full(H * W, 128, np.uint8),
            "out": np.zeros(3 * H * W, np.uint8)}
    dev = {k: c.dev_upload(a) for k, a in host.items()}
    got = {}
    try:
        for name, cond, change in rows():
            prm, gp, rg = nct.Params.default(), nct.GuidedParams.default(), nct.RegionParams.default()
            gp.sigma, rg.protect = change.get("sigma", gp.sigma), change.get("protect", rg.protect)
            v = {"h": h, "w": w, "H": H, "W": W, "prm": C.addressof(prm), "guided": C.addressof(gp), "region": C.addressof(rg)}
            v.update(dev if name.endswith("_dev") else {k: a.ctypes.data for k, a in host.items()})
            v.update({k: x for k, x in change.items() if k in v})
            fn = getattr(l, name)
            fn.restype, fn.argtypes = C.c_int, [C.c_void_p] + [C.c_int if a in ("h", "w", "H", "W") else C.c_void_p for a in ARGS[name]]
            held = c.counter(nct.CTR_ARENA_BYTES)
            rc = fn(c._h, *[v[a] for a in ARGS[name]])
            got["%s | %s" % (name, cond)] = [rc, l.nct_last_error(c._h).decode() if rc else "", c.counter(nct.CTR_ARENA_BYTES) - held]
    finally:
        c.synchronize()
        for p in dev.values():
            c.dev_free(p)
    return got


@pytest.mark.gpu
def test_finish_up_refusals():
    with open(GOLDEN) as f:
        golden = json.load(f)
    with nct.Context(0) as c:
        got = run_rows(c)
    assert sorted(got) == sorted(golden) and len(got) == 8 * 9 + 4 * 4 + 4 * 3            # 9 conditions fit every symbol, 4 more the guided ones, 3 more the masked ones
    for key, (rc, msg, taken) in got.items():
        assert (rc, msg, taken) == (-2, golden[key], 0), key
