"""Correspondence carry (SPEC §6.23) on the GPU: the four seams in their host and device forms against the numpy rules (tests/seq_carry_ref.py), carrying sequences
frame by frame and level by level against the composition, the kept fields, the launch counts, the identities and what a sequence that never turns the carry on
holds. All comparisons are equality of bytes / bit patterns."""
import numpy as np
import pytest

import finish_up_ref as fr
import nct
import seq_carry_ref as ref
import seq_mc_ref
import seq_ref
import synth

pytestmark = pytest.mark.gpu

H, W = 56, 64
REF = (2000, 60, 72)
REF2 = (2001, 52, 66)
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
INVALID, STATE = -2, -5


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


@pytest.fixture(scope="module")
def frames():
    return seq_ref.pan_frames(4, H, W, step=2)


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_f(a, b):
    """bit-identical where neither is NaN, NaN where the other is (x86 and gfx950 give a 0/0 different payloads)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(fbits(a[~na]), fbits(b[~nb]))


def dbits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def refused(call, code, word):
    with pytest.raises(nct.NctError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


# ---- seams

@pytest.mark.parametrize("grid,rgrid", ref.GRIDS)
def test_moves_match_the_numpy_rules(ctx, grid, rgrid):
    (h, w), (bh, bw) = grid, rgrid
    for kind in ("random", "outside", "shift", "zero"):
        field = ref.field_case(h, w, 7 * h + w, kind)
        a, b = ref.nnf_case(h, w, bh, bw, 3 * h + w), ref.nnf_case(bh, bw, h, w, 5 * h + w)
        F = ref.forward_map(field)
        for dev in (False, True):
            assert np.array_equal(ctx.nnf_carry(a, field, dev=dev), ref.move_a(a, field)), (kind, dev)
            assert np.array_equal(ctx.nnf_forward_map(field, dev=dev), F), (kind, dev)
            assert np.array_equal(ctx.nnf_remap(b, F, dev=dev), ref.remap_b(b, F)), (kind, dev)
    wild = np.full((bh, bw), 0xFFFFFFFF, np.uint32)                  # coordinates past the grid are clamped to it
    assert np.array_equal(ctx.nnf_remap(wild, F), ref.remap_b(wild, F))


@pytest.mark.parametrize("grid,rgrid", ref.GRIDS)
@pytest.mark.parametrize("C", [4, 64])
def test_merge_matches_the_numpy_rule(ctx, oracle, grid, rgrid, C):
    for (ah, aw), (bh, bw) in ((grid, rgrid), (rgrid, grid)):      # both directions
        fa, fb = synth.features(10 + C, C, ah, aw), synth.features(20 + C, C, bh, bw)
        a, b = oracle.feat_normalize(fa), oracle.feat_normalize(fb)
        a[:, ah // 2, aw // 3] = np.nan                            # dead pixels: their 3 x 3 neighbourhoods have NaN distances
        b[:, bh // 2, bw // 2] = np.nan
        z, c = ref.nnf_case(ah, aw, bh, bw, ah + aw), ref.nnf_case(ah, aw, bh, bw, ah * aw)
        dist = lambda f: oracle.patchmatch(a, b, f, 0, 0, 0)[1]
        start, dz, dc = ref.merge(dist, z, c)
        assert np.isnan(dz).any()
        if ah * aw > 16:                                           # on the smallest grids every patch holds the dead pixel
            assert (dc < dz).any() and (dz < dc).any()
        for dev in (False, True):
            got, gz, gc = ctx.nnf_merge(a, b, z, c, dev=dev)
            assert same_f(gz, dz) and same_f(gc, dc), dev
            assert np.array_equal(got, start), dev
            assert np.array_equal(got[np.isnan(dz) | np.isnan(dc)], z[np.isnan(dz) | np.isnan(dc)])
            assert np.array_equal(ctx.nnf_merge(a, b, z, c, dev=dev, want_dist=False), start)
            assert np.array_equal(ctx.nnf_merge(a, b, z, z, dev=dev)[0], z)          # Z equal to C everywhere: the output is Z
        # the distances are nct_patchmatch(iters = 0)'s
        assert same_f(ctx.patchmatch(a, b, z, iters=0, rs_max=0, seed=0)[1], dz)


def test_seam_refusals(ctx, oracle):
    h, w, bh, bw = 5, 7, 6, 4
    field, a, b = ref.field_case(h, w, 1, "random"), ref.nnf_case(h, w, bh, bw, 2), ref.nnf_case(bh, bw, h, w, 3)
    F = ref.forward_map(field)
    refused(lambda: ctx.nnf_carry(a, field, dev=True, alias=True), INVALID, "alias")
    refused(lambda: ctx.nnf_forward_map(field, dev=True, alias=True), INVALID, "alias")
    refused(lambda: ctx.nnf_remap(b, F, dev=True, alias=True), INVALID, "alias")
    fa, fb = oracle.feat_normalize(synth.features(1, 8, h, w)), oracle.feat_normalize(synth.features(2, 8, bh, bw))
    refused(lambda: ctx.nnf_merge(fa, fb, a, a, dev=True, alias=True), INVALID, "alias")
    refused(lambda: ctx.nnf_merge(fa, fb, a, a, patch=5), INVALID, "patch")
    refused(lambda: ctx.nnf_merge(fa[:6], fb[:6], a, a), INVALID, "multiple of 4")
    out = np.empty((h, w), np.uint32)
    l, hd = ctx._l, ctx._h
    for call, word in ((lambda: l.nct_nnf_carry(hd, None, h, w, field, out), "null"), (lambda: l.nct_nnf_carry(hd, a, h, w, None, out), "null"),
                       (lambda: l.nct_nnf_carry(hd, a, h, w, field, None), "null"), (lambda: l.nct_nnf_carry(hd, a, 0, w, field, out), "grid"),
                       (lambda: l.nct_nnf_carry(hd, a, h, 4096, field, out), "12-bit"), (lambda: l.nct_nnf_forward_map(hd, None, h, w, out), "null"),
                       (lambda: l.nct_nnf_forward_map(hd, field, 4096, w, out), "12-bit"), (lambda: l.nct_nnf_remap(hd, b, bh, bw, None, h, w, out), "null"),
                       (lambda: l.nct_nnf_remap(hd, b, bh, 4096, F, h, w, out), "12-bit"), (lambda: l.nct_nnf_remap(hd, b, bh, bw, F, 0, w, out), "12-bit"),
                       (lambda: l.nct_nnf_merge(hd, fa, fb, 8, h, w, bh, bw, 3, a, None, out, None, None), "null"),
                       (lambda: l.nct_nnf_merge(hd, fa, fb, 8, h, 4096, bh, bw, 3, a, a, out, None, None), "12-bit"),
                       (lambda: l.nct_nnf_carry_dev(hd, None, h, w, None, None), "null"), (lambda: l.nct_nnf_merge_dev(hd, None, None, 8, h, w, bh, bw, 3, None, None, None, None, None), "null")):
        refused(lambda: ctx._chk(call()), INVALID, word)


def test_state_refusals(wctx, frames):
    refused(lambda: wctx.seq_set_carry(True), STATE, "no sequence is open")
    refused(lambda: wctx._chk(wctx._l.nct_seq_get_carry(wctx._h, 0, 0, None, None)), STATE, "no sequence is open")
    begin(wctx, 2)
    try:
        refused(lambda: wctx.seq_set_carry(2), INVALID, "on must be")
        refused(lambda: wctx.seq_set_carry(True, 65), INVALID, "iters")
        refused(lambda: wctx.seq_set_carry(True, -2), INVALID, "iters")
        refused(lambda: wctx.seq_get_carry(0, 0), STATE, "no kept fields")             # carry off
        wctx.seq_set_carry(True, 2)
        refused(lambda: wctx.seq_get_carry(0, 0), STATE, "no kept fields")             # on, but no full frame yet
        refused(lambda: wctx.seq_set_carry(True, 65), INVALID, "iters")                # a refused call changes nothing
        wctx.seq_frame(frames[0])
        wctx.seq_get_carry(0, 1)
        refused(lambda: wctx.seq_get_carry(1, 0), INVALID, "references")
        refused(lambda: wctx.seq_get_carry(0, 2), INVALID, "level runs")
        wctx.seq_reset()
        refused(lambda: wctx.seq_get_carry(0, 0), STATE, "no kept fields")             # a reset drops them
        wctx.seq_frame(frames[0])
        wctx.seq_set_carry(False)
        refused(lambda: wctx.seq_get_carry(0, 0), STATE, "no kept fields")             # and so does turning the carry off
    finally:
        wctx.seq_end()


# ---- sequences against the composition

def begin(c, levels=5, motion=True, carry=None, **kw):
    prm = nct.Params.default(); prm.levels = levels
    c.seq_begin(synth.image(*REF), (H, W, 3), prm, **kw)
    if motion:
        c.seq_set_motion(*MOT)
    if carry is not None:
        c.seq_set_carry(True, carry)
    return prm


def check_frame(c, lv, out, keep, kept, levels, t, it, merged, pm_iters=10):
    for l in range(levels):
        for name, same in (("ann", np.array_equal), ("bnn", np.array_equal), ("annd", same_f), ("bnnd", same_f), ("result", np.array_equal)):
            assert same(lv[name][l], keep[name][l]), (name, t, l)
        assert np.array_equal(dbits(lv["ab_blend"][l]), dbits(keep["ab_blend"][l])), ("ab_blend", t, l)
        ga, gb = c.seq_get_carry(0, l)
        assert np.array_equal(ga, kept[l][0]) and np.array_equal(gb, kept[l][1]), ("kept", t, l)
    assert np.array_equal(out, keep["result"][levels - 1]), t
    # rule 7: 1 + 4 it launches per reference on a frame that merged, 1 + 4 pm_iters on one that did not
    assert lv["timing"]["pm_level_launches"][:levels] == [1 + 4 * (it if merged else pm_iters)] * levels, (t, lv["timing"]["pm_level_launches"])


_first = {}


def first_frame(oracle, weights, frames, levels):
    """the composition's first frame, once per number of levels: it depends on nothing else (seq_carry_ref.first_frame)"""
    if levels not in _first:
        _first[levels] = ref.first_frame(oracle, frames[0], synth.image(*REF), *weights, levels=levels)
    return _first[levels]


# three frames each, so that the third frame's kept fields come from a frame that merged itself; all five levels (level 4 is the C = 64 path) for every carry_iters
@pytest.mark.parametrize("carry_iters,levels,motion,tau,n", [(-1, 5, True, None, 3), (2, 5, True, None, 3), (0, 5, True, None, 3), (2, 3, False, None, 3), (2, 3, True, 0.0, 3)])
def test_carrying_sequence_matches_the_composition(wctx, oracle, weights, frames, carry_iters, levels, motion, tau, n):
    ws, bs = weights
    it = 10 if carry_iters < 0 else carry_iters
    kw = {} if tau is None else {"tau": tau}
    exp, keeps, carries = ref.sequence(oracle, frames[:n], synth.image(*REF), ws, bs, carry_iters=it, mot=MOT if motion else None, levels=levels,
                                       first=first_frame(oracle, weights, frames, levels), **kw)
    # conditions on the expected side: the kept match wins the merge somewhere at every level of the later frames, and with motion the fields move it
    assert all((keeps[t]["dc_a"][l] < keeps[t]["dz_a"][l]).any() for t in range(1, n) for l in range(levels))
    if motion:
        assert any(keeps[t]["motion"][levels - 1].any() for t in range(1, n))
    begin(wctx, levels, motion, carry_iters, **kw)
    try:
        for t in range(n):
            out, lv = wctx.seq_frame_levels(frames[t], want_color=False)
            check_frame(wctx, lv, out, keeps[t], carries[t], levels, t, it, merged=t > 0)
            if carry_iters == 0 and t > 0:                       # identity 8(d): the seam is visible through the frame
                for l in range(levels):
                    assert np.array_equal(lv["ann"][l], keeps[t]["start_a"][l]) and np.array_equal(lv["bnn"][l], keeps[t]["start_b"][l])
                    dz, dc = keeps[t]["dz_a"][l], keeps[t]["dc_a"][l]
                    ok = ~(np.isnan(dz) | np.isnan(dc))
                    assert np.array_equal(fbits(lv["annd"][l][ok]), fbits(np.minimum(dz, dc)[ok]))
    finally:
        wctx.seq_end()


def test_full_propagated_full(wctx, oracle, weights, frames):
    ws, bs = weights
    levels, plan = 3, [True, False, True]
    exp, keeps, carries = ref.sequence(oracle, frames[:3], synth.image(*REF), ws, bs, carry_iters=2, plan=plan, mot=MOT, levels=levels,
                                       first=first_frame(oracle, weights, frames, levels))
    assert any(not np.array_equal(a0, a1) for (a0, _), (a1, _) in zip(carries[0], carries[1]))        # the propagated frame moved the kept fields
    begin(wctx, levels, True, 2)
    try:
        out, lv = wctx.seq_frame_levels(frames[0], want_color=False)
        check_frame(wctx, lv, out, keeps[0], carries[0], levels, 0, 2, merged=False)
        out = wctx.seq_frame_propagate(frames[1])
        assert np.array_equal(out, exp[1])
        for l in range(levels):
            ga, gb = wctx.seq_get_carry(0, l)
            assert np.array_equal(ga, carries[1][l][0]) and np.array_equal(gb, carries[1][l][1]), l
        out, lv = wctx.seq_frame_levels(frames[2], want_color=False)
        check_frame(wctx, lv, out, keeps[2], carries[2], levels, 2, 2, merged=True)
    finally:
        wctx.seq_end()


def test_two_references(wctx, oracle, weights, frames):
    ws, bs = weights
    levels, refs = 2, [synth.image(*REF), synth.image(*REF2)]
    exp, keeps, carries = ref.sequence_multi(oracle, frames[:3], refs, ws, bs, carry_iters=2, mot=MOT, levels=levels)
    prm = nct.Params.default(); prm.levels = levels
    wctx.seq_begin_multi(refs, (H, W, 3), prm)
    try:
        wctx.seq_set_motion(*MOT)
        wctx.seq_set_carry(True, 2)
        for t in range(3):
            out, lv = wctx.seq_frame_multi_levels(frames[t])
            assert np.array_equal(out, exp[t]), t
            for l in range(levels):
                assert np.array_equal(lv["label"][l], keeps[t]["label"][l]), (t, l)
                for k in range(2):
                    assert np.array_equal(lv["ann"][k][l], keeps[t]["ann"][k][l]) and np.array_equal(lv["bnn"][k][l], keeps[t]["bnn"][k][l]), (t, k, l)
                    assert same_f(lv["annd"][k][l], keeps[t]["annd"][k][l]) and same_f(lv["bnnd"][k][l], keeps[t]["bnnd"][k][l]), (t, k, l)
                    ga, gb = wctx.seq_get_carry(k, l)
                    assert np.array_equal(ga, carries[t][l][k][0]) and np.array_equal(gb, carries[t][l][k][1]), (t, k, l)
            assert lv["timing"]["pm_level_launches"][:levels] == [2 * (1 + 4 * (2 if t else 10))] * levels
    finally:
        wctx.seq_end()


def test_full_resolution_sequence_with_the_upsampling_finish(wctx, oracle, weights):
    """SPEC §6.9 rule 1 with the carry: the state and the kept fields are seq_carry_ref's on the shrunk frames and the shrunk reference, the result is the upsampling
    finish of that composition's X' on the original frame. (A full-resolution sequence reports no nct_pair_levels: SPEC §6.9 rule 5; the kept fields are its final NNFs.)"""
    ws, bs = weights
    levels = 2
    frames0, ref0 = fr.pan()[:3], synth.image(*fr.REF)
    WH, WW = fr.WORK
    prm = nct.Params.default(); prm.levels = levels
    S = [wctx.resize_u8c3(f, WH, WW) for f in frames0]
    R = wctx.resize_u8c3(ref0, *nct.working_size(*ref0.shape[:2], fr.MAX_SIDE))
    exp, keeps, carries = ref.sequence(oracle, S, R, ws, bs, carry_iters=2, mot=MOT, levels=levels)
    # condition on the expected side: the kept match wins the merge on both later frames (at the last level run; on level 0's 4 x 4 grid of this clip it only ties)
    assert all((keeps[t]["dc_a"][levels - 1] < keeps[t]["dz_a"][levels - 1]).any() for t in (1, 2))
    d, hh, ww = [], WH, WW
    for _ in range(5):
        d.insert(0, (hh, ww)); hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
    h, w = d[levels - 1]
    wctx.seq_begin_fullres(ref0, frames0[0].shape, fr.MAX_SIDE, nct.FINISH_UPSAMPLE, prm)
    try:
        wctx.seq_set_motion(*MOT); wctx.seq_set_carry(True, 2)
        for t, f in enumerate(frames0):
            out, lv = wctx.seq_frame_levels(f, want_color=False)
            for l in range(levels):
                assert np.array_equal(dbits(lv["ab_blend"][l]), dbits(keeps[t]["ab_blend"][l])), (t, l)
                assert np.array_equal(lv["motion"][l], keeps[t]["motion"][l] if t else np.zeros_like(lv["motion"][l])), (t, l)
                ga, gb = wctx.seq_get_carry(0, l)
                assert np.array_equal(ga, carries[t][l][0]) and np.array_equal(gb, carries[t][l][1]), (t, l)
                assert np.array_equal(ga, keeps[t]["ann"][l]) and np.array_equal(gb, keeps[t]["bnn"][l]), (t, l)
            _, st = wctx.color_finish(keeps[t]["ab_blend"][levels - 1], h, w, WH, WW, S[t], prm, want_stages=True)
            assert np.array_equal(out, wctx.color_finish_upsample(st["ab_wls"], WH, WW, f, prm)), t
            assert lv["timing"]["pm_level_launches"][:levels] == [1 + 4 * (2 if t else 10)] * levels
    finally:
        wctx.seq_end()


def test_auto_frames_through_a_cut(wctx, oracle, weights, frames):
    """nct_seq_frame_auto with max_gap = 1 (every frame that is no cut is a key frame) over two frames of one scene and two of another: FIRST, KEY, CUT, KEY. Every
    frame and the kept fields after it are seq_carry_ref's, the cut frame being the first frame of a new sequence: nothing is merged into it and it runs pm_iters"""
    ws, bs = weights
    levels = 2
    clip = frames[:2] + seq_ref.pan_frames(2, H, W, step=2, seed=3000)
    auto = nct.SeqAuto(24, 500, 100, 1)
    exp, carries = [], []
    for part in (clip[:2], clip[2:]):                            # the plan taken from the decisions: the cut starts the composition over
        o, _, k = ref.sequence(oracle, part, synth.image(*REF), ws, bs, carry_iters=2, mot=MOT, levels=levels)
        exp += o; carries += k
    plain = ref.sequence(oracle, clip[2:3], synth.image(*REF), ws, bs, carry=False, mot=MOT, levels=levels)[0][0]
    assert np.array_equal(exp[2], plain)                         # identity 8(b) on the expected side
    begin(wctx, levels, True, 2)
    try:
        kinds = []
        for t, f in enumerate(clip):
            out, dec, tm = wctx.seq_frame_auto(f, auto, want_timing=True)
            kinds.append(dec["kind"])
            assert np.array_equal(out, exp[t]), t
            for l in range(levels):
                ga, gb = wctx.seq_get_carry(0, l)
                assert np.array_equal(ga, carries[t][l][0]) and np.array_equal(gb, carries[t][l][1]), (t, l)
            assert tm["pm_level_launches"][:levels] == [9 if t in (1, 3) else 41] * levels, (t, tm["pm_level_launches"])
        assert kinds == [nct.SEQ_FIRST, nct.SEQ_KEY, nct.SEQ_CUT, nct.SEQ_KEY], kinds
    finally:
        wctx.seq_end()


# ---- a sequence that never turns the carry on

def test_carry_never_turned_on(wctx, weights, frames):
    """identity 8(a): bytes, launches and arena of a sequence on a context that never called nct_seq_set_carry; on and off again before the first frame: the bytes.
    The arena counter is the sum of the device allocations a context has ever made; its blocks are cached and reused best-fit. Two contexts that never call
    nct_seq_set_carry must agree on it: while the carry is off the hook requests nothing, so the two make the requests a build without the feature makes (that
    build's own figure is not recorded in the tree, so it is not compared here). A context that turned the carry on and off again has made the carry's allocations and
    holds them as free cached blocks, which later requests may or may not take instead of allocating: its counter legitimately differs, in either direction of the
    blocks' total, and is only printed"""
    levels = 3
    res = []
    for mode in ("never", "never", "on_off"):
        with nct.Context(0) as c:
            c.vgg19_load_raw(*weights)
            begin(c, levels)
            if mode == "on_off":
                c.seq_set_carry(True, 2); c.seq_set_carry(False)
            outs = [c.seq_frame(frames[0], want_timing=True), c.seq_frame(frames[1], want_timing=True), (c.seq_frame_propagate(frames[2]), None),
                    c.seq_frame(frames[3], want_timing=True)]
            res.append(([o for o, _ in outs], [tm["pm_level_launches"] for _, tm in outs if tm], c.counter(nct.CTR_ARENA_BYTES)))
            c.seq_end()
    print("arena bytes: never %d / %d, on and off again %d" % (res[0][2], res[1][2], res[2][2]))
    assert res[0][1] == [[41] * levels + [0] * (5 - levels)] * 3
    assert res[0][2] == res[1][2] and res[0][1] == res[1][1] == res[2][1]
    for mode in (1, 2):
        assert all(np.array_equal(a, b) for a, b in zip(res[0][0], res[mode][0]))
    # and the same sequence on the shared context, which has carried before, gives the same bytes
    begin(wctx, levels)
    try:
        assert all(np.array_equal(wctx.seq_frame(f), o) for f, o in zip(frames[:2], res[0][0][:2]))
    finally:
        wctx.seq_end()


def test_two_contexts_give_the_same_bytes(wctx, weights, frames):
    """identity 8(e)"""
    def run(c):
        begin(c, 2, True, 2)
        try:
            return [c.seq_frame(frames[0]), c.seq_frame(frames[1]), c.seq_frame_propagate(frames[2]), c.seq_frame(frames[3])], [c.seq_get_carry(0, l) for l in range(2)]
        finally:
            c.seq_end()
    a, ka = run(wctx)
    with nct.Context(0) as c:
        c.vgg19_load_raw(*weights)
        b, kb = run(c)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(ka, kb))


def test_distances_never_rise_above_the_candidates(wctx, frames):
    """identity 8(c) on the GPU's own reports: with carry_iters = 0 the frame reports min(d_Z, d_C) per query; with more iterations the final distance is at most that.
    On identical consecutive frames level 0's distances never rise"""
    levels = 2
    got = {}
    for it in (0, 2):
        begin(wctx, levels, True, it)
        try:
            wctx.seq_frame(frames[0])
            got[it] = wctx.seq_frame_levels(frames[1], want_color=False)[1]
        finally:
            wctx.seq_end()
    # level 0 of both runs starts from the same features and the same kept fields
    d0, d2 = got[0]["annd"][0], got[2]["annd"][0]
    ok = ~np.isnan(d0)
    assert (d2[ok] <= d0[ok]).all() and (got[2]["bnnd"][0] <= got[0]["bnnd"][0])[~np.isnan(got[0]["bnnd"][0])].all()
    begin(wctx, 1, False, 2)
    try:
        prev = None
        for _ in range(3):
            d = wctx.seq_frame_levels(frames[0], want_color=False)[1]["annd"][0]
            assert prev is None or (d <= prev).all()
            prev = d
    finally:
        wctx.seq_end()
