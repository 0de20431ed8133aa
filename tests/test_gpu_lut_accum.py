"""The shot accumulator on the GPU (SPEC §6.20): a table over many adds equals the fit of the pixels laid end to end — tests/lut_ref.py's splat and fit, and the
library's own nct_lut_fit[_masked] — bit for bit, in any order of the adds and in any mix of the host and the device form; masked adds, nct_lut_accum_add_run after
every kind of run, the state rules, the accumulator's lifetime, the arena fill hook, and a shot table put onto 16-bit originals."""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "neural-color-transfer_amd", "python"))
import lut16_ref
import lut_ref
import nct
import synth

pytestmark = pytest.mark.gpu

SIZES = (1, 65, 37 * 70)                                     # three chunks of unequal length: a single pixel, one past a wave, several workgroups' worth
BAD_SIZES = (0, 2, 4, 16, 32, 64, 129, -3)
CONSISTENCY_BOUND = 0.5 + 0.5 / 257 + 1e-9                   # tests/test_lut16.py


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def same_fit(got, exp):
    """(table, stages) of the binding against (table, W, R, D) of lut_ref.fit or another (table, stages)"""
    lut, st = got
    if isinstance(exp[1], dict):
        exp = (exp[0], exp[1]["weight"], exp[1]["resid"], exp[1]["disp"])
    return same(lut.reshape(-1, 3), exp[0].reshape(-1, 3)) and same(st["weight"], exp[1]) and same(st["resid"], exp[2]) and same(st["disp"], exp[3])


def refused(call, code, *words):
    with pytest.raises(nct.NctError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


@functools.lru_cache(maxsize=None)
def chunks():
    """[(source, result, mask)] of SIZES pixels; the masks keep about half of the pixels"""
    rng = np.random.default_rng(77)
    out = []
    for n in SIZES:
        s, o = rng.integers(0, 256, (n, 3)).astype(np.uint8), rng.integers(0, 256, (n, 3)).astype(np.uint8)
        m = rng.integers(0, 256, n).astype(np.uint8)
        m[0] = 200                                           # the single pixel is kept
        out.append((s, o, m))
    return out


def joined(parts, k):
    return np.concatenate([p[k] for p in parts])


@functools.lru_cache(maxsize=None)
def ref_fit(N, lam, masked=False):
    s, o, m = (joined(chunks(), k) for k in range(3))
    keep = m >= 128 if masked else np.ones(len(m), bool)
    return lut_ref.fit(s[keep], o[keep], N, lam)


@contextlib.contextmanager
def accum(c, N):
    """an accumulator that is closed on every way out, so that one failing test leaves none open on a shared context"""
    c.lut_accum_begin(N)
    try:
        yield
    finally:
        c.lut_accum_end()


@functools.lru_cache(maxsize=None)
def synthetic_pair():
    return synth.image(1000, 56, 64), synth.image(1001, 48, 64)


@pytest.fixture(scope="module")
def actx():
    """a context of this module's own, with the synthetic VGG19: the shared one must not be left with an open accumulator"""
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    with nct.Context(0) as c:
        c.vgg19_load_raw(ws, bs)
        yield c


@pytest.mark.parametrize("lam", [1.0, None])
@pytest.mark.parametrize("N", [5, 17, 33])
def test_equals_the_fit_of_the_concatenation(actx, N, lam):
    c, parts = actx, chunks()
    lam_ = nct.LutParams.default().lambda_ if lam is None else lam
    exp = ref_fit(N, lam_)
    s, o = joined(parts, 0), joined(parts, 1)
    own = c.lut_fit(s, o, N, lam_, want_stages=True)
    assert same_fit(own, exp)
    with accum(c, N):
        for k, (cs, co, _) in enumerate(parts):
            c.lut_accum_add(cs, co, dev=(k == 1))            # host, device, host
        assert c.lut_accum_info() == {"size": N, "adds": 3, "pixels_offered": sum(SIZES), "pixels_kept": sum(SIZES)}
        assert same_fit(c.lut_accum_solve(lam, want_stages=True), exp)
        assert same_fit(c.lut_accum_solve(lam, want_stages=True, dev=True), own)
        assert same(c.lut_accum_solve(lam), own[0]) and same(c.lut_accum_solve(lam, dev=True), own[0])
    with accum(c, N):
        for k, (cs, co, _) in enumerate(reversed(parts)):   # the reverse order, the forms the other way round
            c.lut_accum_add(cs, co, dev=(k != 1))
        assert same_fit(c.lut_accum_solve(lam, want_stages=True), exp)


@pytest.mark.parametrize("N", [9, 17])
def test_masked_adds(actx, N):
    c, parts = actx, chunks()
    exp = ref_fit(N, 1.0, masked=True)
    s, o, m = (joined(parts, k) for k in range(3))
    kept = int((m >= 128).sum())
    assert 0 < kept < len(m)
    assert same_fit(c.lut_fit_masked(s, o, m, N, 1.0, want_stages=True), exp)
    nothing = np.full(SIZES[1], 127, np.uint8)                # the largest value that is not kept
    with accum(c, N):
        for k, (cs, co, cm) in enumerate(parts):
            c.lut_accum_add(cs, co, cm, dev=(k == 2))
        before = c.lut_accum_info()
        assert before == {"size": N, "adds": 3, "pixels_offered": sum(SIZES), "pixels_kept": kept}
        got = c.lut_accum_solve(1.0, want_stages=True)
        assert same_fit(got, exp)
        for dev in (False, True):                              # a chunk of which nothing is kept: offered and counted, but neither a sum nor pixels_kept moves
            c.lut_accum_add(parts[1][0], parts[1][1], nothing, dev=dev)
        after = c.lut_accum_info()
        assert after == dict(before, adds=5, pixels_offered=sum(SIZES) + 2 * SIZES[1])
        assert same_fit(c.lut_accum_solve(1.0, want_stages=True), got)
        c.lut_accum_add(parts[0][0], parts[0][1])            # an unmasked add among masked ones: every pixel of it
        assert c.lut_accum_info()["pixels_kept"] == kept + SIZES[0]
    with accum(c, N):                                          # nothing kept at all
        refused(lambda: c.lut_accum_solve(1.0), -2, "lut_accum_solve", "keeps no pixel")
        c.lut_accum_add(parts[1][0], parts[1][1], nothing)
        assert c.lut_accum_info()["pixels_kept"] == 0
        refused(lambda: c.lut_accum_solve(1.0), -2, "lut_accum_solve", "keeps no pixel")
        refused(lambda: c.lut_accum_solve(1.0, dev=True), -2, "lut_accum_solve_dev", "keeps no pixel")
        c.lut_accum_add(parts[0][0], parts[0][1], parts[0][2])
        assert same(c.lut_accum_solve(1.0).reshape(-1, 3), lut_ref.fit(parts[0][0], parts[0][1], N, 1.0)[0])


def test_solve_does_not_consume(actx):
    c, parts, N = actx, chunks(), 9
    with accum(c, N):
        c.lut_accum_add(parts[2][0], parts[2][1])
        assert same_fit(c.lut_accum_solve(1.0, want_stages=True), lut_ref.fit(parts[2][0], parts[2][1], N, 1.0))
        c.lut_accum_add(parts[1][0], parts[1][1])
        both = (np.concatenate([parts[2][0], parts[1][0]]), np.concatenate([parts[2][1], parts[1][1]]))
        for lam in (1.0, 0.25, 1.0):                            # two lambdas in a row, and the first again
            assert same_fit(c.lut_accum_solve(lam, want_stages=True), lut_ref.fit(both[0], both[1], N, lam))


@pytest.fixture(scope="module")
def shot(actx):
    """three frames of a 56 x 64 sequence with nct_lut_accum_add_run after each: (frames, outputs, (table, stages) at N = 17 and the default lambda)"""
    src, ref = synthetic_pair()
    frames = [src, np.clip(src.astype(int) + 3, 0, 255).astype(np.uint8), synth.image(1002, 56, 64)]
    outs = []
    with accum(actx, 17):
        actx.seq_begin(ref, src.shape)
        try:
            for k, f in enumerate(frames):
                outs.append(actx.seq_frame(f))
                actx.lut_accum_add_run()
                assert actx.lut_accum_info() == {"size": 17, "adds": k + 1, "pixels_offered": (k + 1) * 56 * 64, "pixels_kept": (k + 1) * 56 * 64}
        finally:
            actx.seq_end()
        fit = actx.lut_accum_solve(want_stages=True)
    return frames, outs, fit


def test_add_run_after_every_frame_of_a_sequence(shot):
    frames, outs, fit = shot
    assert not same(outs[0], outs[1])
    assert same_fit(fit, lut_ref.fit(np.concatenate(frames).reshape(-1, 3), np.concatenate(outs).reshape(-1, 3), 17, nct.LutParams.default().lambda_))


def test_add_run_after_pair_runs(actx):
    c, N = actx, 9
    src, ref = synthetic_pair()
    res = c.process_pair(src, ref)
    with accum(c, N):
        c.lut_accum_add_run()
        by_run = c.lut_accum_solve(1.0, want_stages=True)
    with accum(c, N):
        c.lut_accum_add(src, res)
        assert same_fit(c.lut_accum_solve(1.0, want_stages=True), by_run)
    assert same_fit(by_run, lut_ref.fit(src, res, N, 1.0)) and same(by_run[0], c.pair_fit_lut(N, 1.0))
    # a masked pair run: its mask
    mask = np.zeros(src.shape[:2], np.uint8)
    mask[10:40, 8:50] = 255
    mask[20:30, 50:56] = 127
    mask[30:36, 50:56] = 128
    res = c.process_pair_region(src, mask, ref)
    keep = mask.reshape(-1) >= 128
    with accum(c, N):
        c.lut_accum_add_run()
        assert c.lut_accum_info()["pixels_kept"] == int(keep.sum()) and c.lut_accum_info()["pixels_offered"] == keep.size
        got = c.lut_accum_solve(1.0, want_stages=True)
    assert same_fit(got, lut_ref.fit(src.reshape(-1, 3)[keep], res.reshape(-1, 3)[keep], N, 1.0)) and same(got[0], c.pair_fit_lut(N, 1.0))
    # a full-resolution run: the original-size pair
    src0 = c.resize_u8c3(synth.image(61, 60, 40), 150, 100)
    res0 = c.process_pair_fullres(src0, ref, 64)
    with accum(c, N):
        c.lut_accum_add_run()
        assert c.lut_accum_info()["pixels_offered"] == 150 * 100
        got = c.lut_accum_solve(1.0, want_stages=True)
    assert same_fit(got, lut_ref.fit(src0, res0, N, 1.0)) and same(got[0], c.pair_fit_lut(N, 1.0))


def test_add_run_without_a_finished_run():
    s, o, _ = chunks()[1]
    with nct.Context(0) as fresh, accum(fresh, 9):
        fresh.lut_accum_add(s, o)
        before = fresh.lut_accum_info()
        refused(fresh.lut_accum_add_run, -5, "lut_accum_add_run", "no finished run")
        fresh.lut_fit(s, o, 5, 1.0)                              # a fit is not a run
        refused(fresh.lut_accum_add_run, -5, "lut_accum_add_run", "no finished run")
        assert fresh.lut_accum_info() == before
        assert same(fresh.lut_accum_solve(1.0).reshape(-1, 3), lut_ref.fit(s, o, 9, 1.0)[0])


def test_lifetime_and_state(actx):
    import ctypes as C
    c, parts, N = actx, chunks(), 9
    src, ref = synthetic_pair()
    L, h = c._l, c._h
    s, o, m = parts[1]
    lut = np.zeros((N, N, N, 3), np.float32)
    without = {"lut_accum_add": lambda: c.lut_accum_add(s, o), "lut_accum_add_dev": lambda: c.lut_accum_add(s, o, dev=True), "lut_accum_add_run": c.lut_accum_add_run,
               "lut_accum_info": c.lut_accum_info, "lut_accum_solve": lambda: c.lut_accum_solve(1.0), "lut_accum_solve_dev": lambda: c.lut_accum_solve(1.0, dev=True),
               "lut_accum_end": c.lut_accum_end}
    for name, call in without.items():
        refused(call, -5, name, "no accumulator")
    for bad in BAD_SIZES:
        refused(lambda: c.lut_accum_begin(bad), -2, "lut_accum_begin", "size")
    refused(c.lut_accum_info, -5, "lut_accum_info")             # a refused begin opens nothing
    with accum(c, N):
        refused(lambda: c.lut_accum_begin(N), -5, "lut_accum_begin", "is open")
        refused(lambda: c.lut_accum_begin(0), -5, "lut_accum_begin", "is open")
        c.lut_accum_add(*parts[0][:2])
        c.pair_upload(src, ref)                                  # an upload, a run and a whole sequence between the adds
        c.pair_run()
        c.lut_accum_add(*parts[1][:2], dev=True)
        c.seq_begin(ref, src.shape)
        c.seq_frame(src)
        c.seq_reset()
        c.seq_frame(src)
        c.seq_end()
        c.lut_accum_add(*parts[2][:2])
        assert same_fit(c.lut_accum_solve(1.0, want_stages=True), ref_fit(N, 1.0))
        for lam in (0.0, -1.0, float("nan"), float("inf")):
            refused(lambda: c.lut_accum_solve(lam), -2, "lut_accum_solve", "lambda")
            refused(lambda: c.lut_accum_solve(lam, dev=True), -2, "lut_accum_solve_dev", "lambda")
        refused(lambda: c._chk(L.nct_lut_accum_solve(h, 1.0, None, None)), -2, "lut_accum_solve", "null pointer")
        refused(lambda: c._chk(L.nct_lut_accum_solve_dev(h, 1.0, None, None)), -2, "lut_accum_solve_dev", "null pointer")
        before = c.lut_accum_info()
        for fn, name in ((L.nct_lut_accum_add, "lut_accum_add"), (L.nct_lut_accum_add_dev, "lut_accum_add_dev")):
            refused(lambda: c._chk(fn(h, None, o.ctypes.data, None, len(s))), -2, name, "null pointer")
            refused(lambda: c._chk(fn(h, s.ctypes.data, None, None, len(s))), -2, name, "null pointer")
            for npix in (0, (1 << 26) + 1):
                refused(lambda: c._chk(fn(h, s.ctypes.data, o.ctypes.data, None, npix)), -2, name, "pixels")
        assert c.lut_accum_info() == before                     # a refused add changes nothing
        size = C.c_int()
        c._chk(L.nct_lut_accum_info(h, C.byref(size), None, None, None))        # every pointer of info is nullable
        c._chk(L.nct_lut_accum_info(h, None, None, None, None))
        assert size.value == N
    with accum(c, 5):                                            # after end, a new begin starts from zero, at another size
        assert c.lut_accum_info() == {"size": 5, "adds": 0, "pixels_offered": 0, "pixels_kept": 0}
        c.lut_accum_add(s, o, m)
        keep = m >= 128
        assert same_fit(c.lut_accum_solve(1.0, want_stages=True), lut_ref.fit(s[keep], o[keep], 5, 1.0))
    refused(c.lut_accum_end, -5, "lut_accum_end", "no accumulator")


def test_nothing_else_moves(actx):
    """with an accumulator open, a pair run and its table give the bytes they give without one"""
    c = actx
    src, ref = synthetic_pair()
    res, lut = c.process_pair(src, ref), c.pair_fit_lut(17, 1.0)
    with accum(c, 33):
        c.lut_accum_add(*chunks()[2][:2])
        assert same(c.process_pair(src, ref), res) and same(c.pair_fit_lut(17, 1.0), lut)
        assert same(c.lut_fit(src, res, 17, 1.0), lut)
    assert same(c.process_pair(src, ref), res) and same(c.pair_fit_lut(17, 1.0), lut)


def test_results_ignore_what_arena_blocks_held(monkeypatch):
    """the method of tests/test_gpu_arena_fill.py: the same adds and solves on a context whose arena fills every block with 0xFF before it hands it out"""
    parts = chunks()
    monkeypatch.setenv("NCT_ARENA_FILL", "255")
    with nct.Context(0) as c:
        probe = c.dev_alloc(4096)
        assert (c.dev_download(probe, (4096,), np.uint8) == 255).all(), "the fill hook is not active"
        c.dev_free(probe)
        for N in (9, 17):
            with accum(c, N):
                for k, (cs, co, cm) in enumerate(parts):
                    c.lut_accum_add(cs, co, cm, dev=(k == 1))
                assert same_fit(c.lut_accum_solve(1.0, want_stages=True), ref_fit(N, 1.0, masked=True))
                assert same_fit(c.lut_accum_solve(1.0, want_stages=True, dev=True), ref_fit(N, 1.0, masked=True))
            with accum(c, N):
                for cs, co, _ in parts:
                    c.lut_accum_add(cs, co)
                assert same_fit(c.lut_accum_solve(1.0, want_stages=True), ref_fit(N, 1.0))


def test_a_shot_table_on_16_bit_originals(actx, shot):
    """end to end: the table of the three frames on their 16-bit originals"""
    frames, _, (table, _) = shot
    rng = np.random.default_rng(16)
    for f in frames:
        deep = np.minimum(f.astype(np.uint32) * 257 + rng.integers(0, 256, f.shape), 65535).astype(np.uint16)      # 255 * 257 is 65535 already: saturated, not wrapped
        exp = lut16_ref.apply(table, 17, deep.reshape(-1, 3)).reshape(f.shape)
        assert same(actx.lut_apply_u16(table, deep), exp) and same(actx.lut_apply_u16(table, deep, dev=True), exp)
        flat = f.astype(np.uint16) * 257                            # low = 0: the 8-bit frame itself
        o16 = actx.lut_apply_u16(table, flat)
        assert same(o16, lut16_ref.apply(table, 17, flat.reshape(-1, 3)).reshape(f.shape))
        assert np.abs(o16.astype(np.float64) / 257.0 - actx.lut_apply(table, f).astype(np.float64)).max() <= CONSISTENCY_BOUND
