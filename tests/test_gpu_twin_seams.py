"""The seams that exist as nct_X and nct_X_dev, one table: the host form and the device form of the binding return equal bits on the same data.

Every twin whose inputs tests/host_seams.py's data() provides, which is all but region_select and region_model_apply (they need weights and are compared in their own
tests), at the sizes of tests/test_gpu_host_seams.py: grids of 5 x 7 and 6 x 5 (odd, no multiple of any tile, every 3 x 3 window touching a border), K = 2, C = 8,
lattices of 3 and 5, a 9 x 11 target. The arithmetic is pinned by the seams' own tests; this file is about the two forms being one seam."""
import numpy as np
import pytest

import host_seams
import nct
from test_gpu_arena_fill import _same_array

pytestmark = pytest.mark.gpu

SIZES = {"5x7": host_seams.sizes(5, 7, 9, 11, 8, 3), "6x5": host_seams.sizes(6, 5, 9, 11, 8, 5)}


def _forms(name, *args, **kw):
    """a twin with a second method X_dev -> (host call, device call)"""
    return (lambda c: getattr(c, name)(*args, **kw)), (lambda c: getattr(c, name + "_dev")(*args, **kw))


def _switch(name, *args, **kw):
    """a twin with a dev=True switch -> (host call, device call)"""
    return (lambda c: getattr(c, name)(*args, **kw)), (lambda c: getattr(c, name)(*args, dev=True, **kw))


def twins(c, d):
    s = d.s
    qmask = np.ascontiguousarray(d.img_b[..., 0])
    lut = c.lut_fit(d.full, d.res, size=s.N)
    return {
        "color_finish_upsample": _forms("color_finish_upsample", d.ab, s.h, s.w, d.full),
        "color_finish_guided": _forms("color_finish_guided", d.ab, d.lab, s.h, s.w, d.full, sigma=10.0),
        "color_finish_upsample_region": _forms("color_finish_upsample_region", d.ab, s.h, s.w, d.full, d.mask_full, 1),
        "color_finish_guided_region": _forms("color_finish_guided_region", d.ab, d.lab, s.h, s.w, d.full, d.mask_full, 1, sigma=10.0),
        "select_reference": _forms("select_reference", d.errs, d.guides),
        "region_pull": _forms("region_pull", qmask, d.ann, d.bnn),
        "seq_warp": _forms("seq_warp", d.x_prev, d.field),
        "seq_blend": _forms("seq_blend", d.x, d.x_prev, d.lab, d.lab_prev, 0.7, 10.0),
        "seq_blend_mc": _forms("seq_blend_mc", d.x, d.x_prev, d.lab, d.lab_prev, 0.7, 10.0, d.field),
        "seq_motion_field": _forms("seq_motion_field", d.lab, d.lab_prev, d.parent, 2, 8),
        "seq_change": _forms("seq_change", d.lab, d.lab_prev, d.field),
        "lut_fit": _forms("lut_fit", d.full, d.res, size=s.N, want_stages=True),
        "lut_fit_masked": _forms("lut_fit_masked", d.full, d.res, d.mask_full, size=s.N, want_stages=True),
        "lut_apply": _forms("lut_apply", lut, d.full),
        "resize_u8c1": _forms("resize_u8c1", d.score, s.H, s.W),
        "region_mix": _forms("region_mix", d.x, d.src_mask),
        "region_compose": _forms("region_compose", d.full, d.res, d.mask_full, 1),
        "select_reference_hold": _switch("select_reference_hold", d.errs, d.guides, d.prev_label, d.lab, d.lab_prev, d.field, hold=0.01),
        "seq_pull_hold": _switch("seq_pull_hold", d.pulled, d.label, d.prev, d.lab, d.lab_prev, d.field, d.src_mask),
        "seq_matte_warp": _switch("seq_matte_warp", d.mask_full, d.field),
        "region_snap": _switch("region_snap", d.mask_full, d.full),
        "feat_quantize": _switch("feat_quantize", d.fa),
        "region_score": _switch("region_score", d.q, d.seeds_in, d.seeds_out),
        "region_refind": _switch("region_refind", d.score, (s.H, s.W), d.mask_full, 32),
    }


NAMES = ("color_finish_upsample", "color_finish_guided", "color_finish_upsample_region", "color_finish_guided_region", "select_reference", "region_pull", "seq_warp",
         "seq_blend", "seq_blend_mc", "seq_motion_field", "seq_change", "lut_fit", "lut_fit_masked", "lut_apply", "resize_u8c1", "region_mix", "region_compose",
         "select_reference_hold", "seq_pull_hold", "seq_matte_warp", "region_snap", "feat_quantize", "region_score", "region_refind")


@pytest.fixture(scope="module")
def ctx():
    with nct.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def table(ctx):
    return {k: twins(ctx, host_seams.data(s)) for k, s in SIZES.items()}


def same(a, b, path):
    """equal structure, equal bits -> the paths that differ"""
    if isinstance(a, np.ndarray):
        return [] if isinstance(b, np.ndarray) and _same_array(a, b) else [path]
    if isinstance(a, (tuple, list)):
        return [path] if type(a) is not type(b) or len(a) != len(b) else [p for i, (x, y) in enumerate(zip(a, b)) for p in same(x, y, "%s[%d]" % (path, i))]
    if isinstance(a, dict):
        return [path] if not isinstance(b, dict) or list(a) != list(b) else [p for k in a for p in same(a[k], b[k], "%s.%s" % (path, k))]
    return [] if type(a) is type(b) and a == b else [path]


def test_the_table_names_every_twin_with_inputs(table):
    assert all(sorted(t) == sorted(NAMES) for t in table.values()) and len(NAMES) == 24


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("name", NAMES)
def test_both_forms_return_equal_bits(ctx, table, size, name):
    host, dev = table[size][name]
    a, b = host(ctx), dev(ctx)
    assert a is not None and not same(a, b, name), "the forms differ in %s" % same(a, b, name)
