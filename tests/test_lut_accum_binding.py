"""The shot accumulator and the 16-bit apply at the C ABI and in the binding, without a GPU (SPEC §6.20): the header declares the entry points, the library exports
them, and the binding's methods hand them what the header says, in both forms, against the stub arena of tests/test_binding_seams.py."""
import os
import re

import numpy as np

import nct
import test_binding_seams as tb

NEW = ("nct_lut_apply_u16", "nct_lut_apply_u16_dev", "nct_lut_accum_begin", "nct_lut_accum_add", "nct_lut_accum_add_dev", "nct_lut_accum_add_run", "nct_lut_accum_info",
       "nct_lut_accum_solve", "nct_lut_accum_solve_dev", "nct_lut_accum_end")


def test_header_library_and_binding_hold_the_entry_points():
    hdr = open(os.path.join(os.path.dirname(nct.PKG_ROOT), "include", "nct.h")).read()
    assert "6.20" in hdr and nct.lib().nct_version() == nct.NCT_VERSION == 118       # entry points were only added
    for name in NEW:
        assert re.search(r"\bint %s\(nct_ctx\* ctx" % name, hdr), name
        assert name in nct.SIGNATURES and hasattr(nct.lib(), name), name
    for twin in ("nct_lut_apply_u16", "nct_lut_accum_add", "nct_lut_accum_solve"):
        assert nct.SIGNATURES[twin] == nct.SIGNATURES[twin + "_dev"]


class _Stub(tb._Stub):
    """the arena of test_binding_seams; every other entry point is logged by name with the kinds of its arguments"""

    def __getattr__(self, name):
        if not name.startswith("nct_"):
            raise AttributeError(name)

        def fn(*args):
            assert args[0] is None and len(args) == len(nct.SIGNATURES[name][1]), name
            self.log.append("%s(%s)" % (name, ", ".join("b%d" % self.blocks[a] if a in self.blocks else "null" if a is None else type(a).__name__ for a in args[1:])))
            return 0
        return fn


def _context():
    ctx = nct.Context.__new__(nct.Context)
    ctx._h, ctx._l = None, _Stub({})
    return ctx


def test_host_forms_touch_no_arena():
    c = _context()
    px, t = np.zeros((5, 3), np.uint16), np.zeros((3, 3, 3, 3), np.float32)
    out = c.lut_apply_u16(t, px)
    assert out.dtype == np.uint16 and out.shape == px.shape
    c.lut_accum_begin(5)
    c.lut_accum_add(np.zeros((4, 3), np.uint8), np.zeros((4, 3), np.uint8))
    c.lut_accum_add(np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2), np.uint8))
    c.lut_accum_add_run()
    lut, st = c.lut_accum_solve(want_stages=True)
    assert lut.shape == (5, 5, 5, 3) and lut.dtype == np.float32
    assert {k: (v.shape, v.dtype) for k, v in st.items()} == {"weight": ((125,), np.uint64), "resid": ((125, 3), np.int64), "disp": ((125, 3), np.float64)}
    assert c.lut_accum_solve(2.0).shape == (5, 5, 5, 3)
    c.lut_accum_end()
    assert c._l.log == ["nct_lut_apply_u16(int, int, int, int, int)", "nct_lut_accum_begin(int)", "nct_lut_accum_add(int, int, null, int)",
                        "nct_lut_accum_add(int, int, int, int)", "nct_lut_accum_add_run()", "nct_lut_accum_solve(float, int, int)", "nct_lut_accum_solve(float, int, null)",
                        "nct_lut_accum_end()"]


def test_device_forms_stage_through_the_arena():
    c = _context()
    px, t = np.zeros((5, 3), np.uint16), np.zeros((3, 3, 3, 3), np.float32)
    assert c.lut_apply_u16(t, px, dev=True).dtype == np.uint16
    assert c.lut_apply_u16(t, px, dev=True, in_place=True).shape == (5, 3)
    c.lut_accum_begin(5)
    c.lut_accum_add(np.zeros((4, 3), np.uint8), np.zeros((4, 3), np.uint8), np.zeros(4, np.uint8), dev=True)
    c.lut_accum_solve(0.5, want_stages=True, dev=True)
    calls = [l for l in c._l.log if l.startswith("nct_")]
    assert calls == ["nct_lut_apply_u16_dev(b1, int, b2, int, b3)", "nct_lut_apply_u16_dev(b4, int, b5, int, b5)", "nct_lut_accum_begin(int)",
                     "nct_lut_accum_add_dev(b7, b8, b9, int)", "nct_lut_accum_solve_dev(float, b10, int)"]
    log = c._l.log
    at = log.index("nct_lut_accum_add_dev(b7, b8, b9, int)")
    assert log[at + 1:at + 5] == ["sync", "free 7", "free 8", "free 9"]                 # the uploads live until the enqueued splat has run
    assert log[-9:] == ["download 10 1500", "download 11 1000", "download 12 3000", "download 13 3000", "sync", "free 10", "free 11", "free 12", "free 13"]
