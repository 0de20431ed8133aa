"""The nullable arguments of the host-pointer seams (tests/host_seams.py lists them): a call with one optional argument absent against the call with everything present.

An absent output, or an absent input that only feeds absent outputs, changes nothing else: every output both calls return is equal bit for bit. An absent input that
enters the arithmetic equals the call that passes its neutral value (a zero field, an all-255 mask, an empty list); the coarser level's field has none and is compared
with tests/seq_mc_ref.py, the prior of the re-find with the resize it falls back to. Grids of 5 x 7 and 6 x 5 (odd, no multiple of any tile, 3 x 3 windows that touch
every border), K = 2, C = 8, lattices of 3 and 5, a 9 x 11 target for the finishes. The arithmetic itself is pinned by the seams' own tests; this file is about which
block a pointer names and how large it is."""
import numpy as np
import pytest

import host_seams
import nct
import seq_mc_ref
from test_gpu_arena_fill import _same_array

pytestmark = pytest.mark.gpu

SIZES = {"5x7": host_seams.sizes(5, 7, 9, 11, 8, 3), "6x5": host_seams.sizes(6, 5, 9, 11, 8, 5)}
# absent arguments that enter the arithmetic of what is still returned
ARITHMETIC = {("select_reference_hold", "field"), ("seq_pull_hold", "pulled1"), ("seq_pull_hold", "field"), ("seq_pull_hold", "src_mask"), ("seq_motion_field", "parent"),
              ("seq_change", "field"), ("region_score", "seeds_out"), ("region_refind", "prior"), ("color_finish_upsample_region", "mask"), ("color_finish_guided_region", "mask")}
CALLS = {name: call for name, _, call in host_seams.NULLABLE}


@pytest.fixture(scope="module")
def ctx():
    with nct.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def full(ctx):
    """(size, seam) -> (the data, the call with every optional argument present), each computed once"""
    cache, datas = {}, {k: host_seams.data(s) for k, s in SIZES.items()}

    def get(size, name):
        if (size, name) not in cache:
            cache[size, name] = CALLS[name](ctx, datas[size], ())
        return datas[size], cache[size, name]
    return get


def same(got, exp, what):
    assert got.keys() == exp.keys(), what
    for k in exp:
        assert _same_array(got[k], exp[k]), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("name,opt", [(n, o) for n, opts, _ in host_seams.NULLABLE for o in opts if (n, o) not in ARITHMETIC and n != "seq_pull_hold_k1"])
def test_an_absent_output_changes_no_other(ctx, full, size, name, opt):
    d, exp = full(size, name)
    got = CALLS[name](ctx, d, (opt,))
    gone = set(exp) - set(got)
    assert gone, "%s without %s returned everything" % (name, opt)
    same(got, {k: v for k, v in exp.items() if k not in gone}, "%s without %s" % (name, opt))


@pytest.mark.parametrize("size", list(SIZES))
def test_an_unread_label_map_is_not_needed(ctx, full, size):
    """one reference: the label map is not read, with it and without it the same maps come back"""
    d, exp = full(size, "seq_pull_hold_k1")
    same(host_seams._seq_pull_hold(ctx, d, ("label",), K=1), exp, "seq_pull_hold, K = 1, without the label map")


@pytest.mark.parametrize("size", list(SIZES))
def test_an_absent_input_is_its_neutral_value(ctx, full, size):
    d = full(size, "seq_change")[0]
    hs = host_seams
    same(hs._select_reference_hold(ctx, d, ("field",)), hs._select_reference_hold(ctx, d, (), field="zero"), "select_reference_hold: no field / a zero field")
    for opt in ("pulled1", "field", "src_mask"):
        same(hs._seq_pull_hold(ctx, d, (opt,)), hs._seq_pull_hold(ctx, d, (), **{opt: True}), "seq_pull_hold: no %s / its neutral value" % opt)
    same(hs._seq_change(ctx, d, ("field",)), hs._seq_change(ctx, d, (), zero=True), "seq_change: no field / a zero field")
    same(hs._region_score(ctx, d, ("seeds_out",)), hs._region_score(ctx, d, (), empty_list=True), "region_score: no outside list / an empty one")
    plain = hs._lut_fit(ctx, d, ())
    same(hs._lut_fit(ctx, d, (), mask="all"), plain, "lut_fit_masked with an all-255 mask / lut_fit")
    assert not _same_array(hs._lut_fit(ctx, d, (), mask="given")["weight"], plain["weight"]), "the given mask is meant to drop pixels"
    for guided in (False, True):
        unmasked = hs._finish(ctx, d, (), guided, region=False)
        same(hs._finish(ctx, d, ("mask",), guided, region=True), unmasked, "the masked finish (guided: %s) without a mask / the unmasked one" % guided)
        same(hs._finish(ctx, d, (), guided, region=True, mask="all"), unmasked, "the masked finish (guided: %s) with an all-255 mask / the unmasked one" % guided)
        assert not _same_array(full(size, "color_finish_guided_region" if guided else "color_finish_upsample_region")[1]["out"], unmasked["out"]), "the given mask is meant to act"


@pytest.mark.parametrize("size", list(SIZES))
def test_motion_field_without_a_parent(ctx, full, size):
    """the coarser level's field has no neutral value: both forms against tests/seq_mc_ref.py"""
    d, exp = full(size, "seq_motion_field")
    assert np.array_equal(exp["m"], seq_mc_ref.motion(d.lab, d.lab_prev, d.parent, 2, 8))
    got = CALLS["seq_motion_field"](ctx, d, ("parent",))["m"]
    assert np.array_equal(got, seq_mc_ref.motion(d.lab, d.lab_prev, None, 2, 8))
    assert not np.array_equal(got, exp["m"]), "the parent is meant to move the search"


@pytest.mark.parametrize("size", list(SIZES))
def test_refind_without_a_prior(ctx, full, size):
    """SPEC §6.17 rule R3: no prior = the resized score; margin 0 = the prior is never read"""
    d, exp = full(size, "region_refind")
    s = d.s
    resized = ctx.resize_u8c1(d.score, s.H, s.W)
    assert np.array_equal(CALLS["region_refind"](ctx, d, ("prior",))["out"], resized)
    assert np.array_equal(ctx.region_refind(d.score, (s.H, s.W), d.mask_full, 0), resized)
    assert not np.array_equal(exp["out"], resized), "the prior is meant to act at margin 32"


def test_two_seams_back_to_back_on_filled_blocks(monkeypatch, full):
    """two different seams in a row on one context whose blocks are filled with 0x5A before they are handed out: a block read before its upload, or an output block that
    is larger than what was written, shows against the unfilled results. Every optional argument absent first (the blocks nobody asks for are gone), then present"""
    monkeypatch.setenv("NCT_ARENA_FILL", "0x5A")
    with nct.Context(0) as c:
        for name in ("select_reference_hold", "seq_pull_hold", "feat_normalize", "seq_blend_mc", "lut_fit_masked"):
            d, exp = full("5x7", name)
            opts = next(o for n, o, _ in host_seams.NULLABLE if n == name)
            got = CALLS[name](c, d, tuple(o for o in opts if (name, o) not in ARITHMETIC))
            same(got, {k: exp[k] for k in got}, "%s on filled blocks, outputs absent" % name)
            same(CALLS[name](c, d, ()), exp, "%s on filled blocks" % name)
        assert c.counter(nct.CTR_ARENA_BYTES) > 0
