"""The 16-bit table apply on the GPU (SPEC §6.20) against the numpy reference tests/lut16_ref.py, bit for bit: every tail of the four-pixel groups, the LDS and the L2
form of the table, host and device pointers, in place and unaligned, the two properties of the SPEC, every refusal and the arena fill hook. The expectations come
from lut16_ref alone, never from the library's 8-bit or host path."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "neural-color-transfer_amd", "python"))
import lut16_ref
import lut_ref
import nct

pytestmark = pytest.mark.gpu

KINDS = ("random", "ends", "last", "x257")
# both calls round the same real value x (the double sums differ from it by about 1e-12): nct_lut_apply to an integer, the 16-bit apply 257 x to an integer
CONSISTENCY_BOUND = 0.5 + 0.5 / 257 + 1e-9


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def pixels(kind, npix):
    """[npix, 3] uint16: random; only 0 and 65535 (one non-zero corner weight, 65535^3); random mixed with 65535 (the clamped cell, f = 65535); multiples of 257 (the
    8-bit colours). The seed is the pixel count: with it every expectation of npix >= 63 below holds both 0 and 65535"""
    rng = np.random.default_rng(npix)
    if kind == "random":
        s = rng.integers(0, 65536, (npix, 3))
    elif kind == "ends":
        s = rng.choice(np.array([0, 65535]), (npix, 3))
    elif kind == "last":
        s = rng.integers(0, 65536, (npix, 3))
        s[rng.random((npix, 3)) < 0.5] = 65535
    else:
        s = rng.integers(0, 256, (npix, 3)) * 257
    s = s.astype(np.uint16)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def random_table(N):
    t = (np.random.default_rng(N).random((N, N, N, 3)) * 400.0 - 70.0).astype(np.float32)        # reaches outside [0, 255]: the cast saturates at both ends
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def expected(N, kind, npix):
    e = lut16_ref.apply(random_table(N), N, pixels(kind, npix))
    e.setflags(write=False)
    return e


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("npix", [1, 3, 4, 5, 63, 64, 65, 4097])
@pytest.mark.parametrize("N", [3, 17, 33, 65])
def test_apply_equals_numpy(ctx, N, npix, kind):
    px, exp = pixels(kind, npix), expected(N, kind, npix)
    assert npix < 63 or (exp.min() == 0 and exp.max() == 65535)
    assert same(ctx.lut_apply_u16(random_table(N), px), exp)
    assert same(ctx.lut_apply_u16(random_table(N), px, dev=True), exp)


@pytest.mark.parametrize("N", [3, 17, 33, 65])
def test_the_identity_table_returns_every_input(ctx, N):
    rng = np.random.default_rng(N)
    px = rng.integers(0, 65536, (3, 65536, 3)).astype(np.uint16)
    for a in range(3):
        px[a, :, a] = np.arange(65536, dtype=np.uint16)          # all 65536 values on each axis, the other two random
    px = px.reshape(-1, 3)
    ident = lut_ref.identity(N).reshape(N, N, N, 3)
    assert same(lut16_ref.apply(ident, N, px), px)
    assert same(ctx.lut_apply_u16(ident, px), px)
    assert same(ctx.lut_apply_u16(ident, px, dev=True), px)


@pytest.mark.parametrize("N", [3, 17, 33, 65])
def test_consistency_with_the_8_bit_apply(ctx, N):
    rng = np.random.default_rng(70 + N)
    u = rng.integers(0, 256, (20000, 3)).astype(np.uint8)
    t = (lut_ref.identity(N).astype(np.float64) + rng.normal(0.0, 6.0, (N ** 3, 3))).astype(np.float32).reshape(N, N, N, 3)
    o8 = ctx.lut_apply(t, u).astype(np.float64)
    o16 = ctx.lut_apply_u16(t, u.astype(np.uint16) * 257)
    assert same(o16, lut16_ref.apply(t, N, u.astype(np.uint16) * 257))
    worst = np.abs(o16.astype(np.float64) / 257.0 - o8).max()
    print("N = %d: max |o16 / 257 - o8| = %.5f" % (N, worst))
    assert worst <= CONSISTENCY_BOUND


@pytest.mark.parametrize("N", [17, 33])
def test_apply_in_place_and_unaligned_dev_pointers(ctx, N):
    """the _dev form over its own input, and on pointers offset by 2 bytes (neither 4- nor 8-byte aligned: the element path of the packed loads and stores)"""
    npix = 1001
    px = pixels("random", npix)
    exp = lut16_ref.apply(random_table(N), N, px)
    assert same(ctx.lut_apply_u16(random_table(N), px, dev=True, in_place=True), exp)
    guard = np.uint16(0xA5A5)
    t = ctx.dev_upload(random_table(N))
    buf = ctx.dev_upload(np.concatenate([np.zeros(1, np.uint16), px.reshape(-1)]))
    out = ctx.dev_upload(np.full(3 * npix + 2, guard, np.uint16))
    try:
        ctx.dev_call("lut_apply_u16", t, N, buf + 2, npix, out + 2)
        got = ctx.dev_download(out, (3 * npix + 2,), np.uint16)
        assert same(got[1:-1].reshape(-1, 3), exp) and got[0] == guard and got[-1] == guard      # nothing written in front of or behind the image
        ctx.dev_call("lut_apply_u16", t, N, buf + 2, npix, buf + 2)                                # unaligned and in place
        assert same(ctx.dev_download(buf, (3 * npix + 1,), np.uint16)[1:].reshape(-1, 3), exp)
    finally:
        ctx.synchronize()
        for p in (t, buf, out):
            ctx.dev_free(p)


def refused(call, code, *words):
    with pytest.raises(nct.NctError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_non_finite_tables(ctx):
    """a NaN entry through the _dev form gives 0 (the cast), the host form refuses the table"""
    N = 9
    bad = lut_ref.identity(N).reshape(N, N, N, 3).copy()
    bad[4, 5, 6, 1] = np.nan
    px = np.concatenate([pixels("random", 4097), np.array([[32768, 40960, 49152], [33000, 41000, 49000]], np.uint16)])      # the node itself and a cell it bounds
    exp = lut16_ref.apply(bad, N, px)
    assert exp[-2, 1] == 0 and exp[-1, 1] == 0 and exp[-2, 0] == 32768 and exp[-2, 2] == 49152
    assert same(ctx.lut_apply_u16(bad, px, dev=True), exp)
    for v in (np.nan, np.inf, -np.inf):
        bad[4, 5, 6, 1] = v
        refused(lambda: ctx.lut_apply_u16(bad, px), -2, "lut_apply_u16", "non-finite")


def test_refusals(ctx):
    px = pixels("random", 64)
    out = np.zeros_like(px)
    lut = np.zeros((33, 33, 33, 3), np.float32)
    L = ctx._l
    for fn, name in ((L.nct_lut_apply_u16, "lut_apply_u16"), (L.nct_lut_apply_u16_dev, "lut_apply_u16_dev")):
        for args in ((None, 33, px.ctypes.data, 64, out.ctypes.data), (lut.ctypes.data, 33, None, 64, out.ctypes.data), (lut.ctypes.data, 33, px.ctypes.data, 64, None)):
            refused(lambda: ctx._chk(fn(ctx._h, *args)), -2, name, "null pointer")
        for N in (0, 2, 4, 16, 32, 64, 129, -3):
            refused(lambda: ctx._chk(fn(ctx._h, lut.ctypes.data, N, px.ctypes.data, 64, out.ctypes.data)), -2, name, "size")
        for npix in (0, (1 << 26) + 1):
            refused(lambda: ctx._chk(fn(ctx._h, lut.ctypes.data, 33, px.ctypes.data, npix, out.ctypes.data)), -2, name, "pixels")
    for N in (0, 2, 4, 16, 32, 64, 129, -3):                             # through the binding as well, both forms
        t = np.zeros((max(N, 1),) * 3 + (3,), np.float32)
        refused(lambda: ctx.lut_apply_u16(t, px), -2, "lut_apply_u16", "size")
        refused(lambda: ctx.lut_apply_u16(t, px, dev=True), -2, "lut_apply_u16_dev", "size")


def test_results_ignore_what_arena_blocks_held(monkeypatch):
    """the method of tests/test_gpu_arena_fill.py: the same applies on a context whose arena fills every block with 0xFF before it hands it out"""
    px = pixels("last", 4097)
    monkeypatch.setenv("NCT_ARENA_FILL", "255")
    with nct.Context(0) as c:
        probe = c.dev_alloc(4096)
        assert (c.dev_download(probe, (4096,), np.uint8) == 255).all(), "the fill hook is not active"
        c.dev_free(probe)
        for N in (17, 33):
            assert same(c.lut_apply_u16(random_table(N), px), expected(N, "last", 4097))
            assert same(c.lut_apply_u16(random_table(N), px, dev=True), expected(N, "last", 4097))
            assert same(c.lut_apply_u16(random_table(N), px[:1001], dev=True, in_place=True), lut16_ref.apply(random_table(N), N, px[:1001]))
