"""Frame sequences over several references (SPEC §6.18) on the GPU: k_select_hold through its two seams against the numpy rule (tests/seq_multi_ref.py), whole sequences
against the composition level by level, the identities, propagated and auto frames, full-resolution sequences, region masks, the refusals, and what a context holds.
All comparisons are equality of bytes / bit patterns."""
import numpy as np
import pytest

import multi_ref
import nct
import seq_multi_ref as smr
import seq_ref
import synth

pytestmark = pytest.mark.gpu

FRAME = (96, 80)                                  # the whole-sequence fixture: K = 2, three pan frames, motion on
SMALL = (64, 56)                                  # the identities


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


@pytest.fixture(scope="module")
def refs():
    return smr.quality_references()


def fresh(weights):
    c = nct.Context(0)
    c.vgg19_load_raw(*weights)
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- seams: nct_select_reference_hold and its _dev form against the numpy rule

def _check_hold(ctx, c, hold, sigma, dev):
    elab, efree, emargin = smr.select_hold(c["errs"], c["prev_label"], c["lab"], c["lab_prev"], c["field"], hold, sigma)
    eG, eE = multi_ref.merge(elab, c["guides"], c["errs"])
    args = (c["errs"], c["guides"], c["prev_label"], c["lab"], c["lab_prev"], c["field"])
    got = ctx.select_reference_hold(*args, hold=hold, sigma=sigma, dev=dev)
    assert got["label"].dtype == np.uint8 and np.array_equal(got["label"], elab)
    assert np.array_equal(got["free_label"], efree) and np.array_equal(bits(got["margin"]), bits(emargin))
    assert np.array_equal(got["guide"], eG) and np.array_equal(words(got["err"]), words(eE))
    return elab, efree


@pytest.mark.parametrize("grid", [(1, 1), (1, 7), (3, 3), (44, 44), (175, 233)])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_select_hold_matches_the_numpy_rule(ctx, grid, K):
    h, w = grid
    switched = kept = 0
    for kind in smr.KINDS:
        for with_field in (True, False):
            c = smr.hold_case(h, w, K, 1000 * K + 31 * h + w, kind, with_field)
            for dev in (False, True):
                lab, free = _check_hold(ctx, c, 0.02, 10.0, dev)
            j = smr.carry(c["prev_label"], c["field"])
            switched += int(((lab != j) & (j < K)).sum()); kept += int(((lab == j) & (lab != free)).sum())
            # hold = 2 with equal Lab maps: g = 1, the margin is 2 n and nothing switches where the kept label is one of the K
            c2 = dict(c, lab_prev=c["lab"], field=None)
            lab, free = _check_hold(ctx, c2, 2.0, 0.75, True)
            ok = c["prev_label"] < K
            assert np.array_equal(lab[ok], c["prev_label"][ok]) and np.array_equal(lab[~ok], free[~ok])
    if K > 1 and h * w > 9:
        assert switched > 0 and kept > 0                # both branches of rule 5 were taken on this grid


def test_select_hold_nullable_outputs(ctx):
    c = smr.hold_case(7, 5, 3, 9, "random")
    args = (c["errs"], c["guides"], c["prev_label"], c["lab"], c["lab_prev"], c["field"])
    for dev in (False, True):
        full = ctx.select_reference_hold(*args, hold=0.02, dev=dev)
        for name in ("label", "guide", "err", "free_label", "margin"):
            one = ctx.select_reference_hold(*args, hold=0.02, dev=dev, want=(name,))
            assert list(one) == [name] and np.array_equal(one[name].view(np.uint8), full[name].view(np.uint8)), (dev, name)
        rest = ctx.select_reference_hold(c["errs"], None, c["prev_label"], c["lab"], c["lab_prev"], None, hold=0.02, dev=dev, want=("label", "err"))
        assert np.array_equal(rest["label"], smr.select_hold(c["errs"], c["prev_label"], c["lab"], c["lab_prev"], None, 0.02, 10.0)[0])
        assert ctx.select_reference_hold(*args, hold=0.02, dev=dev, want=()) == {}


# ---- whole sequences against the composition

@pytest.fixture(scope="module")
def pan():
    return seq_ref.pan_frames(3, FRAME[0], FRAME[1], step=2)


@pytest.mark.parametrize("levels", [5, 1])
def test_sequence_matches_the_composition_level_by_level(wctx, oracle, weights, refs, pan, levels):
    ws, bs = weights
    if levels == 1:
        # the only grid is the coarsest, 6 x 5, where the noisy copy wins every pixel: there the second reference is the first one upside down, and both hold a share
        refs = [refs[0], np.ascontiguousarray(refs[0][::-1])]
    exp, keeps = smr.sequence(oracle, pan, refs, ws, bs, levels=levels)
    # conditions on the expected side: on every later frame the held selection differs from the free one somewhere, and both references hold a share of the finest map
    for k in keeps[1:]:
        assert any((k["free_label"][l] != k["label"][l]).any() for l in range(levels))
        assert any(m.any() for m in k["margin"])
    assert all(min(multi_ref.shares(k["label"][-1], 2)) > 0 for k in keeps)
    prm = nct.Params.default(); prm.levels = levels
    wctx.seq_begin_multi(refs, pan[0].shape, prm)
    try:
        wctx.seq_set_motion()
        for t, f in enumerate(pan):
            out, lv = wctx.seq_frame_multi_levels(f)
            for l in range(levels):
                for k in range(2):
                    assert np.array_equal(words(lv["ref_err"][k][l]), words(keeps[t]["ref_err"][k][l])), ("ref_err", t, l, k)
                assert np.array_equal(lv["free_label"][l], keeps[t]["free_label"][l]), ("free_label", t, l)
                assert np.array_equal(bits(lv["margin"][l]), bits(keeps[t]["margin"][l])), ("margin", t, l)
                assert np.array_equal(lv["label"][l], keeps[t]["label"][l]), ("label", t, l)
                assert np.array_equal(lv["guide"][l], keeps[t]["guide"][l]), ("guide", t, l)
                assert np.array_equal(words(lv["err"][l]), words(keeps[t]["err"][l])), ("err", t, l)
                assert np.array_equal(bits(lv["color"][l]["ab_nonlocal"]), bits(keeps[t]["ab_nonlocal"][l])), ("ab_nonlocal", t, l)
                assert np.array_equal(bits(lv["ab_blend"][l]), bits(keeps[t]["ab_blend"][l])), ("ab_blend", t, l)
                assert np.array_equal(bits(lv["tau_map"][l]), bits(keeps[t]["tau_map"][l])), ("tau_map", t, l)
                assert np.array_equal(lv["motion"][l], keeps[t]["motion"][l]), ("motion", t, l)
                assert np.array_equal(lv["result"][l], keeps[t]["result"][l]), ("result", t, l)
            assert np.array_equal(out, exp[t]), t
        # the plain entry point gives the same frames
        wctx.seq_reset()
        assert all(np.array_equal(wctx.seq_frame(f), e) for f, e in zip(pan, exp))
    finally:
        wctx.seq_end()


# ---- identities

def small_pan(n=3, step=4):
    return seq_ref.pan_frames(n, SMALL[0], SMALL[1], step=step)


def run_multi(c, refs, frames, motion=True, **kw):
    """a sequence over `refs` through the reporting entry point -> list of (result, levels)"""
    c.seq_begin_multi(refs, frames[0].shape, **kw)
    try:
        if motion:
            c.seq_set_motion()
        return [c.seq_frame_multi_levels(f, want_color=False) for f in frames]
    finally:
        c.seq_end()


def test_one_reference_is_nct_seq_begin(weights, refs):
    frames = small_pan()
    res, arena = [], []
    for begin in ("seq_begin", "seq_begin_multi"):
        with fresh(weights) as c:
            if begin == "seq_begin":
                c.seq_begin(refs[0], frames[0].shape)
            else:
                c.seq_begin_multi(refs[:1], frames[0].shape, hold=0.05)
            c.seq_set_motion()
            res.append([c.seq_frame(frames[0]), c.seq_frame(frames[1]), c.seq_frame_propagate(frames[2])])
            arena.append(c.counter(nct.CTR_ARENA_BYTES))
            c.seq_end()
    assert all(np.array_equal(a, b) for a, b in zip(*res))
    print("arena bytes of a one-reference sequence: nct_seq_begin %d, nct_seq_begin_multi %d" % tuple(arena))
    assert arena[0] == arena[1]


def test_frames_without_a_hold_are_process_multi(wctx, weights, refs):
    frames = small_pan()
    with fresh(weights) as p:
        multi = [p.process_multi(f, refs) for f in frames]
    try:
        # a first frame and the frame after nct_seq_reset
        wctx.seq_begin_multi(refs, frames[0].shape)
        wctx.seq_set_motion()
        assert np.array_equal(wctx.seq_frame(frames[0]), multi[0])
        held = wctx.seq_frame(frames[1])
        assert not np.array_equal(held, multi[1])
        wctx.seq_reset()
        out, lv = wctx.seq_frame_multi_levels(frames[2], want_color=False)
        assert np.array_equal(out, multi[2]) and not any(m.any() for m in lv["margin"])
        assert all(np.array_equal(a, b) for a, b in zip(lv["free_label"], lv["label"]))
        # tau == 0: every frame
        wctx.seq_begin_multi(refs, frames[0].shape, tau=0.0, hold=0.1)
        wctx.seq_set_motion()
        assert all(np.array_equal(wctx.seq_frame(f), m) for f, m in zip(frames, multi))
    finally:
        wctx.seq_end()


def test_hold_zero_labels_are_the_free_selection(wctx, refs):
    frames = small_pan()
    for out, lv in run_multi(wctx, refs, frames, hold=0.0):
        for l in range(5):
            sel = multi_ref.select([lv["ref_err"][k][l] for k in range(2)])
            assert np.array_equal(lv["label"][l], sel) and np.array_equal(lv["free_label"][l], sel) and not lv["margin"][l].any()


def test_a_repeated_reference_is_the_single_reference_sequence(wctx, refs):
    frames = small_pan()
    try:
        wctx.seq_begin(refs[0], frames[0].shape)
        wctx.seq_set_motion()
        single = [wctx.seq_frame(f) for f in frames]
    finally:
        wctx.seq_end()
    twice = run_multi(wctx, [refs[0], refs[0]], frames, hold=0.05)
    assert all(np.array_equal(out, s) for (out, _), s in zip(twice, single))
    assert not any(lab.any() for _, lv in twice for lab in lv["label"])
    assert any(m.any() for m in twice[1][1]["margin"])                                    # the held selection ran


def test_identical_frames_and_two_contexts(wctx, weights, refs):
    src = synth.image(1000, *SMALL)
    for hold in (0.0, 0.02, 2.0):
        same = run_multi(wctx, refs, [src] * 3, hold=hold, tau=0.9, sigma=3.0)
        assert all(np.array_equal(out, same[0][0]) for out, _ in same[1:]), hold
        assert all(np.array_equal(a, b) for _, lv in same[1:] for a, b in zip(lv["label"], same[0][1]["label"]))
    frames = small_pan()
    a = run_multi(wctx, refs, frames)
    with fresh(weights) as c:
        b = run_multi(c, refs, frames)
        again = run_multi(c, refs, frames)
    for x in (b, again):
        assert all(np.array_equal(p[0], q[0]) for p, q in zip(a, x))
        assert all(np.array_equal(l1, l2) for p, q in zip(a, x) for l1, l2 in zip(p[1]["label"], q[1]["label"]))


# ---- propagated and auto frames

def test_a_full_frame_holds_against_carried_labels(wctx, oracle, weights, refs):
    ws, bs = weights
    frames = small_pan()
    exp, keeps = smr.sequence(oracle, frames, refs, ws, bs, full=[True, False, True])
    assert keeps[1]["motion"][4].any() and not np.array_equal(keeps[1]["label"][4], keeps[0]["label"][4])      # the carry moved labels
    assert (keeps[2]["free_label"][4] != keeps[2]["label"][4]).any()                                               # and the next full frame held some of them
    try:
        wctx.seq_begin_multi(refs, frames[0].shape)
        wctx.seq_set_motion()
        assert np.array_equal(wctx.seq_frame(frames[0]), exp[0])
        assert np.array_equal(wctx.seq_frame_propagate(frames[1]), exp[1])
        out, lv = wctx.seq_frame_multi_levels(frames[2], want_color=False)
        for l in range(5):
            assert np.array_equal(lv["label"][l], keeps[2]["label"][l]) and np.array_equal(lv["free_label"][l], keeps[2]["free_label"][l]), l
            assert np.array_equal(bits(lv["margin"][l]), bits(keeps[2]["margin"][l])), l
        assert np.array_equal(out, exp[2])
        # a propagated frame identical to the previous one returns its bytes
        assert np.array_equal(wctx.seq_frame_propagate(frames[2]), out)
    finally:
        wctx.seq_end()


def test_auto_frames_decide_as_the_single_reference_sequence(wctx, refs):
    pan = small_pan(4, step=2)
    cut = synth.image(1234, *SMALL)
    frames = pan[:3] + [cut, cut]
    auto = nct.SeqAuto.default()
    runs = []
    for begin in (lambda: wctx.seq_begin(refs[0], frames[0].shape), lambda: wctx.seq_begin_multi(refs, frames[0].shape)):
        try:
            begin()
            wctx.seq_set_motion()
            recs, outs = [], []
            for f in frames:
                probe = wctx.seq_probe(f, auto) if recs else None
                out, d = wctx.seq_frame_auto(f, auto)
                for r in (probe, d):
                    if r is not None:
                        r.pop("probe_ms", None)
                recs.append((probe, d)); outs.append(out)
            runs.append((recs, outs))
        finally:
            wctx.seq_end()
    assert runs[0][0] == runs[1][0]
    kinds = [d["kind"] for _, d in runs[1][0]]
    assert nct.SEQ_CUT in kinds and nct.SEQ_PROPAGATED in kinds, kinds
    t = kinds.index(nct.SEQ_CUT)
    with nct.Context(0) as p:
        from caffemodel_io import synthetic_vgg19
        p.vgg19_load_raw(*synthetic_vgg19(19))
        assert np.array_equal(runs[1][1][t], p.process_multi(frames[t], refs))              # a CUT frame is nct_process_multi's bytes


# ---- full resolution

@pytest.mark.parametrize("finish", [nct.FINISH_EXACT, nct.FINISH_UPSAMPLE])
def test_fullres_sequence(wctx, oracle, refs, finish):
    frames0 = seq_ref.pan_frames(3, 96, 80, step=2)
    refs0 = [synth.image(1001, 96, 72), smr.competing(synth.image(1001, 96, 72))]
    (wh, ww) = nct.working_size(96, 80, 48)
    shrunk = [oracle.resize_u8c3(f, wh, ww) for f in frames0]
    rshrunk = [oracle.resize_u8c3(r, *nct.working_size(r.shape[0], r.shape[1], 48)) for r in refs0]
    work = run_multi(wctx, rshrunk, shrunk)
    try:
        wctx.seq_begin_multi_fullres(refs0, frames0[0].shape, max_side=48, finish=finish)
        wctx.seq_set_motion()
        for t, f in enumerate(frames0):
            out, lv = wctx.seq_frame_multi_levels(f)
            assert out.shape == f.shape and "result" not in lv and "color" not in lv
            for name in ("label", "free_label", "motion"):
                assert all(np.array_equal(a, b) for a, b in zip(lv[name], work[t][1][name])), (name, t)
            for name in ("margin", "ab_blend", "tau_map"):
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(lv[name], work[t][1][name])), (name, t)
        assert any((lv["free_label"][l] != lv["label"][l]).any() for l in range(5))
        # frames that need no shrinking: nct_seq_begin_multi's bytes
        wctx.seq_begin_multi_fullres(rshrunk, shrunk[0].shape, max_side=48, finish=finish)
        wctx.seq_set_motion()
        assert all(np.array_equal(wctx.seq_frame(f), w[0]) for f, w in zip(shrunk, work))
    finally:
        wctx.seq_end()


# ---- masks

def test_region_masks(wctx, refs):
    frames = small_pan()
    plain = [out for out, _ in run_multi(wctx, refs, frames)]
    for value in (255, 0):
        try:
            wctx.seq_begin_multi(refs, frames[0].shape)
            wctx.seq_set_motion()
            wctx.seq_set_region(np.full(SMALL, value, np.uint8))
            got = [wctx.seq_frame(f) for f in frames]
        finally:
            wctx.seq_end()
        assert all(np.array_equal(a, b) for a, b in zip(got, plain if value else frames)), value


# ---- refusals and state

def test_refusals(wctx, refs):
    shape = (SMALL[0], SMALL[1], 3)

    def refused(f, code, word):
        with pytest.raises(nct.NctError) as e:
            f()
        assert e.value.code == code and word in str(e.value), str(e.value)
    refused(lambda: wctx.seq_begin_multi([], shape), -2, "K must be")
    refused(lambda: wctx.seq_begin_multi([refs[0]] * 9, shape), -2, "K must be")
    refused(lambda: wctx.seq_begin_multi([refs[0], None], shape), -2, "reference 1 is null")
    for hold in (-0.01, 2.5, float("nan"), float("inf")):
        refused(lambda: wctx.seq_begin_multi(refs, shape, hold=hold), -2, "hold")
        refused(lambda: wctx.seq_begin_multi_fullres(refs, shape, hold=hold), -2, "hold")
    refused(lambda: wctx.seq_begin_multi_fullres(refs, shape, finish=2), -2, "finish")
    refused(lambda: wctx.seq_begin_multi_fullres([refs[0]] * 9, shape), -2, "K must be")
    c = smr.hold_case(3, 3, 2, 1)
    args = (c["errs"], c["guides"], c["prev_label"], c["lab"], c["lab_prev"], c["field"])
    for dev in (False, True):
        for hold in (-0.01, 2.5, float("nan"), float("inf")):
            refused(lambda: wctx.select_reference_hold(*args, hold=hold, dev=dev), -2, "hold")
        refused(lambda: wctx.select_reference_hold(*args, hold=0.1, sigma=0.0, dev=dev), -2, "sigma")
        refused(lambda: wctx.select_reference_hold([c["errs"][0]] * 9, None, *args[2:], hold=0.1, dev=dev, want=("label",)), -2, "K must be")
    src = synth.image(1000, *SMALL)
    try:
        wctx.seq_begin_multi(refs, shape)
        refused(lambda: wctx.seq_frame_levels(src, want_color=False, want_levels=True), -2, "several references")
        refused(lambda: wctx.pair_set_ref_region(0, np.full(refs[0].shape[:2], 255, np.uint8)), -5, "sequence")
        refused(lambda: wctx.multi_upload(src, refs), -5, "sequence")
        with nct.Context(0) as p:                                                            # the sequence is still usable
            from caffemodel_io import synthetic_vgg19
            p.vgg19_load_raw(*synthetic_vgg19(19))
            assert np.array_equal(wctx.seq_frame(src), p.process_multi(src, refs))
    finally:
        wctx.seq_end()


# ---- what a context holds

def test_arena_after_seq_end(weights, refs):
    frames = small_pan()
    with fresh(weights) as c:
        first = run_multi(c, refs, frames)
        before = c.counter(nct.CTR_ARENA_BYTES)
        for _ in range(2):                                                                   # the blocks a sequence gave back serve the next one: the arena stops growing
            again = run_multi(c, refs, frames)
            assert c.counter(nct.CTR_ARENA_BYTES) == before
            assert all(np.array_equal(a[0], b[0]) for a, b in zip(first, again))


@pytest.mark.parametrize("fill", [0xFF, 0x07])
def test_results_do_not_depend_on_what_reused_blocks_held(monkeypatch, weights, refs, fill):
    """the first frame reads no kept label, and no later frame a byte the sequence has not written: the same calls on a context whose arena fills every block it hands
    out with `fill` (NCT_ARENA_FILL; 0x07 is a valid label of another reference list, 0xFF a stale one) give the same bytes"""
    frames = small_pan()

    def op(c):
        c.vgg19_load_raw(*weights)
        c.seq_begin_multi(refs, frames[0].shape)
        try:
            c.seq_set_motion()
            return [c.seq_frame_multi_levels(frames[0]), (c.seq_frame_propagate(frames[1]), {}), c.seq_frame_multi_levels(frames[2])]
        finally:
            c.seq_end()
    monkeypatch.delenv("NCT_ARENA_FILL", raising=False)
    monkeypatch.delenv("NCT_WLS_MAXIT", raising=False)
    with nct.Context(0) as c:
        clean = op(c)
    its = [int(x) for _, lv in clean for d in lv.get("color", []) for x in d["wls_iters"]] + [int(x) for _, lv in clean if lv for x in lv["timing"]["wls_iters"]]
    monkeypatch.setenv("NCT_ARENA_FILL", str(fill))
    monkeypatch.setenv("NCT_WLS_MAXIT", str(max(its) + 8))                                   # a solve fed with the fill would otherwise run to the default budget
    with nct.Context(0) as c:
        got = op(c)
        assert c.counter(nct.CTR_ARENA_BYTES) > 0
    for (a, la), (b, lb) in zip(clean, got):
        assert np.array_equal(a, b)
        for name in ("label", "free_label", "margin", "guide", "err", "ab_blend", "tau_map", "motion"):
            if name in la:
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(la[name], lb[name])), name
    assert (clean[2][1]["free_label"][4] != clean[2][1]["label"][4]).any()
