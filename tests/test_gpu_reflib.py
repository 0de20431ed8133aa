"""Reference libraries (SPEC §6.21) on the GPU, bit for bit against the numpy rule (tests/reflib_ref.py): nct_feat_quantize8[_dev] (G1), the int8 MFMA lane map of
k_desc_match (G2), the shapes where its tiling can go wrong (G3), nct_reflib_rank end to end on the GPU's own taps (G4) and the refusals (G5).

The match kernel's edges (k_reflib.hip): a workgroup owns 128 source rows as 2 x 2 waves of 64 x 64 (na 1, 31 … 33: one 32-row block and its border; 127, 129, 300: the
wave and tile borders); an entry is walked 128 rows at a time (the same sizes as nb, and 65536 = 512 chunks under three source tiles' atomicMax); channels are staged 128
bytes at a time in steps of 32 (C = 16: half a step; 48: a step and a half; 64; 512: four stages)."""
import numpy as np
import pytest

import nct
import reflib_ref as R
import region_select_ref as sel
import synth

pytestmark = pytest.mark.gpu

INVALID, STATE = -2, -5
SIZES = (1, 31, 32, 33, 127, 129, 300)


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


def raw_refused(c, fn, args, code, word):
    before = c.counter(nct.CTR_ARENA_BYTES)
    rc = getattr(c._l, fn)(c._h, *args)
    msg = c._l.nct_last_error(c._h).decode()
    assert rc == code and word in msg, (fn, rc, msg)
    assert c.counter(nct.CTR_ARENA_BYTES) == before, fn


def both_forms(ctx, a, ents):
    exp = [R.match(a, e) for e in ents]
    ef, eb = np.array([f for f, _ in exp], np.int64), np.array([b for _, b in exp], np.int64)
    for dev in (False, True):
        f, b = ctx.descriptor_match(a, ents, dev=dev)
        assert f.dtype == np.int64 and np.array_equal(f, ef) and np.array_equal(b, eb), (a.shape, [e.shape for e in ents], dev, f, ef, b, eb)


# ---------------------------------------------------------------- G1
@pytest.mark.parametrize("Cc", [16, 64, 512])
@pytest.mark.parametrize("grid", [(1, 1), (3, 5), (9, 11)])
def test_g1_quantize8(ctx, oracle, Cc, grid):
    gh, gw = grid
    f = synth.features(70 + Cc + gh, Cc, gh, gw, smooth=False)
    mu = np.random.default_rng(Cc + gw).random(Cc, dtype=np.float32) * np.float32(0.7)
    variants = [f]
    if gh * gw == 1:
        z = np.zeros_like(f); one = np.zeros_like(f); one[Cc // 3, 0, 0] = 2.5
        variants += [z, one, mu.reshape(Cc, 1, 1).copy()]
    else:
        f[:, 0, 1] = 0                                           # a zero pixel: a row of zeros without a centre
        f[:, 1, 2] = mu                                          # a pixel equal to the centre: a row of zeros with it
        f[:, gh - 1, gw - 2] = 0; f[Cc - 1, gh - 1, gw - 2] = 0.125   # one-hot: exactly 127 without a centre
    for v in variants:
        for centre in (None, mu):
            exp = R.quantize8(oracle, v, centre)
            for dev in (False, True):
                got = ctx.feat_quantize8(v, centre, dev=dev)
                assert got.dtype == np.int8 and got.shape == (gh * gw, Cc) and np.array_equal(got, exp), (Cc, grid, centre is not None, dev)
    if gh * gw == 1:
        assert not R.quantize8(oracle, variants[1]).any() and R.quantize8(oracle, variants[2])[0, Cc // 3] == 127 and not R.quantize8(oracle, variants[3], mu).any()
    else:
        plain, cen = R.quantize8(oracle, f), R.quantize8(oracle, f, mu)
        assert not plain[1].any() and not cen[gw + 2].any() and cen[1].any()
        assert plain[(gh - 1) * gw + gw - 2, Cc - 1] == 127 and np.count_nonzero(plain[(gh - 1) * gw + gw - 2]) == 1


# ---------------------------------------------------------------- G2
@pytest.mark.parametrize("Cc", [32, 64, 512])
def test_g2_lane_map(ctx, Cc):
    """127 times a 32 x 32 identity block against an ASYMMETRIC matrix, both ways round: P is 127 times the other operand's first 32 channels (transposed), so a
    transposed or permuted fragment of either operand, or a wrong C/D map, changes the row or the column maxima"""
    eye = np.zeros((32, Cc), np.int8); eye[np.arange(32), np.arange(32)] = 127
    q, c = np.mgrid[0:32, 0:Cc]
    asym = (((7 * q + 3 * c) % 251) - 125).astype(np.int8)
    assert not np.array_equal(asym[:, :32], asym[:, :32].T)
    P = R.products(eye, asym)
    assert np.array_equal(P, 127 * asym[:, :32].astype(np.int64).T)
    assert P.max(axis=1).sum() != P.max(axis=0).sum() and R.match(eye, asym) != R.match(asym, eye)
    both_forms(ctx, eye, [asym])
    both_forms(ctx, asym, [eye])
    # the same with the block in rows 32 … 63 of a 64-row operand and channels 16 … 47: the second row block of a wave, the second lane half's bytes
    eye2 = np.zeros((64, Cc), np.int8); eye2[32 + np.arange(32), (16 + np.arange(32)) % Cc] = 127
    q2, c2 = np.mgrid[0:64, 0:Cc]
    asym2 = (((7 * q2 + 3 * c2) % 251) - 125).astype(np.int8)
    both_forms(ctx, eye2, [asym2])
    both_forms(ctx, asym2, [eye2])


# ---------------------------------------------------------------- G3
def rand8(rng, n, Cc):
    x = rng.integers(-128, 128, (n, Cc), dtype=np.int8)
    x[rng.integers(0, n), rng.integers(0, Cc)] = -128
    return x


@pytest.mark.parametrize("Cc", [16, 48, 64, 512])
def test_g3_sizes(ctx, Cc):
    rng = np.random.default_rng(Cc)
    for na in SIZES:
        a = rand8(rng, na, Cc)
        for nb in SIZES:
            both_forms(ctx, a, [rand8(rng, nb, Cc)]) if (na + nb) % 2 else both_forms(ctx, a, [rand8(rng, nb, Cc), rand8(rng, 1, Cc), rand8(rng, 33, Cc)])


@pytest.mark.parametrize("Cc", [16, 512])
def test_g3_entries_of_different_sizes(ctx, Cc):
    rng = np.random.default_rng(Cc + 5)
    a = rand8(rng, 300, Cc)
    ents = [rand8(rng, n, Cc) for n in (300, 1, 129, 31, 127)]     # a 1-row entry between two large ones
    both_forms(ctx, a, ents)
    both_forms(ctx, rand8(rng, 33, Cc), ents[:3])
    z = [e.copy() for e in ents]
    z[0][5:40] = 0; z[2][:] = 0                                  # rows of zeros, an entry of zeros
    az = a.copy(); az[100:140] = 0
    both_forms(ctx, az, z)


@pytest.mark.parametrize("Cc", [16, 48, 512])
def test_g3_all_negative(ctx, Cc):
    """a all positive, the entries all negative, sizes that are no multiple of 32: every product is negative, a padded zero must not win a maximum"""
    rng = np.random.default_rng(Cc + 9)
    for na, nbs in ((31, (33,)), (129, (127, 1, 300)), (300, (31, 129))):
        a = rng.integers(1, 128, (na, Cc), dtype=np.int8)
        ents = [rng.integers(-128, 0, (nb, Cc), dtype=np.int8) for nb in nbs]
        assert all(R.products(a, e).max() < 0 for e in ents)
        both_forms(ctx, a, ents)


def test_g3_largest_entry(ctx):
    """300 source rows (three tiles) against one entry of 65536 rows at C = 16: 512 chunks, and every column maximum is the atomicMax of three workgroups"""
    rng = np.random.default_rng(65536)
    a, b = rand8(rng, 300, 16), rand8(rng, 65536, 16)
    exp = R.match(a, b)
    for dev in (False, True):
        f, bw = ctx.descriptor_match(a, [b], dev=dev)
        assert (int(f[0]), int(bw[0])) == exp, dev


# ---------------------------------------------------------------- G4
def gpu_tap(c, img, tap):
    return c.vgg19_features(img, deepest_tap=tap)[tap - 1]


def expect_rank(c, oracle, lib_imgs, src, tap, mu, wf=1, wb=1):
    ents = [R.quantize8(oracle, gpu_tap(c, i, tap), mu) for i in lib_imgs]
    return (ents,) + R.rank(R.quantize8(oracle, gpu_tap(c, src, tap), mu), ents, wf, wb)


def assert_rank(got, exp):
    for g, e, name in zip(got, exp, ("order", "key", "fwd", "bwd")):
        assert np.array_equal(g, e), (name, g, e)


def test_g4_rank_textures(wctx, oracle):
    tap, imgs, srcs = 3, R.fixture_library(), R.fixture_sources()
    mu = R.library_center([gpu_tap(wctx, i, tap) for i in imgs])
    L = nct.RefLib(tap, mu)
    for i in imgs[:4]:
        L.add(wctx, i)
    ents, o, k, f, b = expect_rank(wctx, oracle, imgs[:4], srcs[0], tap, mu)
    rows, offs, cen = L.rows()
    assert L.info() == (tap, 256, 4, sum(len(e) for e in ents), True) and np.array_equal(rows, np.concatenate(ents)) and np.array_equal(cen, mu)
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(e) for e in ents])]).tolist()
    assert_rank(wctx.reflib_rank(L, srcs[0]), (o, k, f, b))
    held = wctx.counter(nct.CTR_ARENA_BYTES)
    assert_rank(wctx.reflib_rank(L, srcs[0]), (o, k, f, b))       # the library is resident: nothing new is reserved
    assert wctx.counter(nct.CTR_ARENA_BYTES) == held
    # a second rank after another add sees the new entry
    L.add(wctx, imgs[4])
    firsts = []
    for i, s in enumerate(srcs):
        exp = expect_rank(wctx, oracle, imgs, s, tap, mu)[1:]
        got = wctx.reflib_rank(L, s)
        assert_rank(got, exp)
        firsts.append(int(got[0][0]))
    assert firsts == [0, 1, 2, 3, 4]                             # and the rule does what it is for on the GPU's taps as well
    for wf, wb in ((0, 1), (1, 0), (16, 3)):
        assert_rank(wctx.reflib_rank(L, srcs[1], wf, wb), expect_rank(wctx, oracle, imgs, srcs[1], tap, mu, wf, wb)[1:])
    # a saved library ranks identically
    rows, offs, cen = L.rows()
    S = nct.RefLib.from_rows(tap, rows, offs, cen)
    assert S.info() == L.info()
    assert_rank(wctx.reflib_rank(S, srcs[2]), wctx.reflib_rank(L, srcs[2]))
    wctx.reflib_release()
    assert_rank(wctx.reflib_rank(L, srcs[2]), expect_rank(wctx, oracle, imgs, srcs[2], tap, mu)[1:])
    S.close(); L.close()
    wctx.reflib_release()


@pytest.mark.parametrize("tap", [1, 2, 4, 5])
def test_g4_rank_sizes(wctx, oracle, tap):
    """the library and the sources at region selection's two sizes (56 x 64 and 57 x 67) and one more: entries of different grids, with and without a centre"""
    imgs = [sel.call_source(*sel.SIZES[0]), synth.image(31, 40, 93), sel.call_source(*sel.SIZES[1]), synth.image(32, *sel.SIZES[0])]
    for centred in (False, True):
        mu = R.library_center([gpu_tap(wctx, i, tap) for i in imgs]) if centred else None
        L = nct.RefLib(tap, mu)
        for i in imgs:
            L.add(wctx, i)
        for h, w in sel.SIZES:
            src = synth.image(50 + h, h, w)
            assert_rank(wctx.reflib_rank(L, src), expect_rank(wctx, oracle, imgs, src, tap, mu)[1:])
        L.close()
    wctx.reflib_release()


def test_g4_rank_leaves_an_open_sequence_alone(wctx):
    src, ref = synth.image(1000, 64, 56), synth.image(1001, 48, 64)
    nxt = np.clip(src.astype(int) + 2, 0, 255).astype(np.uint8)
    wctx.seq_begin(ref, src.shape)
    first, second = wctx.seq_frame(src), wctx.seq_frame(nxt)
    wctx.seq_end()
    L = nct.RefLib(5)
    L.add(wctx, ref); L.add(wctx, src)
    wctx.seq_begin(ref, src.shape)
    assert np.array_equal(wctx.seq_frame(src), first)
    order = wctx.reflib_rank(L, nxt)[0]
    assert sorted(order.tolist()) == [0, 1]
    assert np.array_equal(wctx.seq_frame(nxt), second)
    wctx.seq_end()
    # and an uploaded pair: its result is the same with a rank between upload and run
    exp = wctx.process_pair(src, ref)
    wctx.pair_upload(src, ref)
    wctx.reflib_rank(L, nxt)
    wctx.pair_run()
    assert np.array_equal(wctx.pair_download(), exp)
    L.close()
    wctx.reflib_release()


# ---------------------------------------------------------------- G5
def test_g5_refusals(wctx):
    c = wctx
    f = np.zeros((5, 16), np.float32); q8 = np.zeros((5, 16), np.int8); mu = np.zeros(16, np.float32)
    p = lambda x: x.ctypes.data
    raw_refused(c, "nct_feat_quantize8", (None, p(mu), p(q8), 16, 1, 5), INVALID, "src_chw")
    raw_refused(c, "nct_feat_quantize8", (p(f), None, None, 16, 1, 5), INVALID, "dst")
    raw_refused(c, "nct_feat_quantize8_dev", (None, None, 256, 16, 1, 5), INVALID, "d_src_hwc")
    for fn in ("nct_feat_quantize8", "nct_feat_quantize8_dev"):
        raw_refused(c, fn, (p(f), None, p(q8), 24, 1, 5), INVALID, "C must be a multiple of 16")
        raw_refused(c, fn, (p(f), None, p(q8), 4112, 1, 5), INVALID, "C must be")
        raw_refused(c, fn, (p(f), None, p(q8), 16, 0, 5), INVALID, "grid")
    a, rows = np.zeros((4, 16), np.int8), np.zeros((6, 16), np.int8)
    off = np.array([0, 2, 6], np.int32); fw, bw = np.zeros(2, np.int64), np.zeros(2, np.int64)
    ok = lambda **kw: tuple({**dict(a=p(a), na=4, C=16, rows=p(rows), off=p(off), N=2, f=p(fw), b=p(bw)), **kw}.values())
    for fn in ("nct_descriptor_match", "nct_descriptor_match_dev"):
        raw_refused(c, fn, ok(a=None), INVALID, "null a")
        raw_refused(c, fn, ok(rows=None), INVALID, "null rows")
        raw_refused(c, fn, ok(off=None), INVALID, "null offsets")
        raw_refused(c, fn, ok(f=None), INVALID, "null fwd")
        raw_refused(c, fn, ok(b=None), INVALID, "null bwd")
        raw_refused(c, fn, ok(C=24), INVALID, "C must be a multiple of 16")
        raw_refused(c, fn, ok(N=0), INVALID, "N must be in [1, 4096]")
        raw_refused(c, fn, ok(N=4097), INVALID, "N must be in [1, 4096]")
        raw_refused(c, fn, ok(na=0), INVALID, "na must be")
        raw_refused(c, fn, ok(na=65537), INVALID, "na must be")
        raw_refused(c, fn, ok(off=p(np.array([0, 2, 2], np.int32))), INVALID, "entry 1")
        raw_refused(c, fn, ok(off=p(np.array([0, 2, 70000], np.int32))), INVALID, "entry 1")
    raw_refused(c, "nct_descriptor_match_dev", ok(a=p(a) + 8), INVALID, "a must be 16-byte aligned")
    raw_refused(c, "nct_descriptor_match_dev", ok(rows=p(rows) + 4), INVALID, "rows must be 16-byte aligned")
    ms = np.zeros(1, np.float32)
    raw_refused(c, "nct_descriptor_match_bench", ok() + (0, ms.ctypes.data_as(nct.C.POINTER(nct.C.c_float))), INVALID, "reps")
    # the library calls
    img = np.zeros((64, 56, 3), np.uint8); order = np.zeros(8, np.int32)
    L = nct.RefLib(5)
    rank = lambda **kw: tuple({**dict(lib=L._m, src=p(img), h=64, w=56, prm=None, order=p(order), key=None, f=None, b=None), **kw}.values())
    raw_refused(c, "nct_reflib_rank", rank(), INVALID, "lib holds no entry")
    L.add(c, img)
    for wf, wb, word in ((0, 0, "wf and wb"), (17, 1, "wf must be"), (1, -1, "wb must be")):
        prm = nct.RefLibParams(wf, wb)
        raw_refused(c, "nct_reflib_rank", rank(prm=nct.C.addressof(prm)), INVALID, word)
    raw_refused(c, "nct_reflib_rank", rank(lib=None), INVALID, "null lib")
    raw_refused(c, "nct_reflib_rank", rank(src=None), INVALID, "null src_bgr")
    raw_refused(c, "nct_reflib_rank", rank(order=None), INVALID, "null order")
    raw_refused(c, "nct_reflib_rank", rank(h=16), INVALID, "h must be")
    raw_refused(c, "nct_reflib_rank", rank(w=4001), INVALID, "w must be")
    raw_refused(c, "nct_reflib_add", (None, p(img), 64, 56), INVALID, "null lib")
    raw_refused(c, "nct_reflib_add", (L._m, None, 64, 56), INVALID, "null bgr")
    # a tap whose grid exceeds 65536 cells: tap 1 of 300 x 300
    L1 = nct.RefLib(1)
    big = np.zeros((300, 300, 3), np.uint8)
    raw_refused(c, "nct_reflib_add", (L1._m, p(big), 300, 300), INVALID, "h, w: the grid of tap 1 holds 90000 cells")
    raw_refused(c, "nct_reflib_rank", rank(lib=L1._m, src=p(big), h=300, w=300), INVALID, "h, w: the grid of tap 1 holds 90000 cells")
    assert L1.info()[2] == 0 and L.info()[2] == 1
    # no weights: a context of its own
    with nct.Context(0) as bare:
        raw_refused(bare, "nct_reflib_add", (L._m, p(img), 64, 56), STATE, "weights")
        raw_refused(bare, "nct_reflib_rank", rank(), STATE, "weights")
    L.close(); L1.close()
