"""Source region masks (SPEC §6.11) without a GPU: the identities of rule 4 and the protect guarantee on the CPU reference (tests/region_ref.py over the oracle's
stages), the single-channel resize against its definition, the numpy mix and compose against their rules, the table rule against lut_ref on the kept subsequence,
the CLI's flag refusals and the ABI symbols. Every comparison is equality of bytes or bit patterns."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "neural-color-transfer_amd", "python"))
import lut_ref
import region_ref
import synth

CLI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "neural-color-transfer_amd", "bin", "neural_color_transfer")
SH, SW, RH, RW = 56, 64, 48, 60


@pytest.fixture(scope="module")
def pair(oracle):
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    src, ref = synth.image(1000, SH, SW), synth.image(1001, RH, RW)
    return {"orc": oracle, "ws": ws, "bs": bs, "src": src, "ref": ref, "plain": oracle.process_pair(src, ref, ws, bs)}


def _run(p, kind, **kw):
    return region_ref.pair(p["orc"], p["src"], region_ref.mask(kind, SH, SW), p["ref"], p["ws"], p["bs"], **kw)


def test_full_mask_is_the_plain_pair(pair):
    """rule 4: M = 255 everywhere gives oracle.process_pair's bytes, for either protect"""
    for protect in (0, 1):
        out, keep = _run(pair, "full", protect=protect)
        assert np.array_equal(out, pair["plain"])
        assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(keep["ab_mix"], keep["ab_nonlocal"]))


@pytest.mark.parametrize("levels", [1, 5])
def test_empty_mask_returns_the_source(pair, levels):
    """rule 4: M = 0 everywhere gives the source byte for byte, at every level, for either protect — with protect = 0 through S2 and A1 alone: the solve of the
    identity coefficients stays within A1's rounding, and the compose then finds every Lab byte unchanged"""
    for protect in (0, 1):
        out, keep = _run(pair, "empty", levels=levels, protect=protect)
        assert len(keep["result"]) == levels
        for r in keep["result"]:
            assert np.array_equal(r, pair["src"])


def test_protect_keeps_every_unmasked_pixel_and_bleed_is_reported(pair):
    """the half-plane mask: with protect = 1 no M == 0 pixel changes at any level; with protect = 0 the pixels of the M == 0 half that differ from the source are the
    measured bleed (printed per level, recorded in DESIGN.md §3.16, not asserted)"""
    m = region_ref.mask("half", SH, SW)
    out1, keep1 = _run(pair, "half", protect=1)
    for r in keep1["result"]:
        assert np.array_equal(r[m == 0], pair["src"][m == 0])
    assert not np.array_equal(out1[m == 255], pair["src"][m == 255]), "the masked half was not recoloured"
    out0, keep0 = _run(pair, "half", protect=0)
    for l, r in enumerate(keep0["result"]):
        d = (r != pair["src"]).any(axis=-1) & (m == 0)
        print("level %d: %d of %d M == 0 pixels differ from the source (max %d grey levels)" % (l, int(d.sum()), int((m == 0).sum()),
              int(np.abs(r.astype(int) - pair["src"].astype(int))[m == 0].max())))


@pytest.mark.parametrize("shape, dst", region_ref.RESIZE_SHAPES)
def test_single_channel_resize_definition(oracle, shape, dst):
    """rule 1: channel 0 of the three-channel resize of (M, M, M) — all three channels agree, and the integer restatement written without the oracle gives the same bytes"""
    for kind in region_ref.MASK_KINDS:
        m = region_ref.mask(kind, *shape)
        c3 = oracle.resize_u8c3(np.repeat(m[:, :, None], 3, axis=2), *dst)
        got = region_ref.resize_u8c1(oracle, m, *dst)
        assert got.shape == dst and np.array_equal(c3[..., 1], got) and np.array_equal(c3[..., 2], got)
        assert np.array_equal(got, region_ref.resize_u8c1_np(m, *dst))
    if shape == (64, 64):            # the INTER_AREA switch: (sum of the 2 x 2 block + 2) >> 2, not the bilinear chain
        m = region_ref.mask("random", *shape).astype(int)
        assert np.array_equal(region_ref.resize_u8c1(oracle, m.astype(np.uint8), 32, 32), (m[0::2, 0::2] + m[0::2, 1::2] + m[1::2, 0::2] + m[1::2, 1::2] + 2) >> 2)


def test_mask_pyramid_follows_the_image_pyramid(oracle):
    lv = region_ref.mask_pyramid(oracle, region_ref.mask("ramp", SH, SW))
    assert [a.shape for a in lv] == [(4, 4), (7, 8), (14, 16), (28, 32), (56, 64)]
    assert len(np.unique(lv[4])) == 256, "the ramp holds every byte value"


@pytest.mark.parametrize("shape", region_ref.MIX_SHAPES)
def test_mix_rule(shape):
    """rule 2 in numpy: the endpoints are exact (M = 255 copies the words, a NaN included; M = 0 writes the identity and heals a NaN), between them the two formulas"""
    for kind in region_ref.MASK_KINDS:
        x, m = region_ref.with_nans(*region_ref.mix_case(*shape, kind))
        out = region_ref.mix(x, m)
        M = m.reshape(-1)
        assert np.array_equal(out[:, M == 255].view(np.uint64), x[:, M == 255].view(np.uint64))
        assert (out[0, M == 0] == 1.0).all() and (out[1, M == 0] == 0.0).all() and not np.signbit(out[1, M == 0]).any()
        mid = (M != 0) & (M != 255)
        f = (M[mid].astype(np.float64) / 255.0)[:, None]
        with np.errstate(invalid="ignore"):
            assert np.array_equal((1.0 + f * (x[0, mid] - 1.0)).view(np.uint64), out[0, mid].view(np.uint64))
            assert np.array_equal((f * x[1, mid]).view(np.uint64), out[1, mid].view(np.uint64))
        assert np.isnan(out[:, mid]).sum() == np.isnan(x[:, mid]).sum()


def test_compose_rule(oracle):
    """rule 3 in numpy: kept pixels are the source's bytes, the others Lab -> BGR of the result in the chosen form; an unchanged Lab pixel under M == 255 is NOT kept"""
    s, lab_s, lab_o, m = region_ref.compose_case(oracle, 37, 41)
    assert min(region_ref.compose_shares(lab_s, lab_o, m)) >= 0.01
    same = (lab_o == lab_s).all(axis=-1)
    for form in (0, 1):
        conv = oracle.lab2bgr(lab_o, form)
        for protect in (0, 1):
            out = region_ref.compose(oracle, s, lab_o, m, protect, form)
            keep = (same & (m != 255)) | ((m == 0) if protect else np.zeros_like(same))
            assert np.array_equal(out[keep], s[keep]) and np.array_equal(out[~keep], conv[~keep])
    assert (conv[same & (m == 255)] != s[same & (m == 255)]).any(), "the case has no pixel the Lab round trip changes: it cannot tell keep from convert"


@pytest.mark.parametrize("N", [9, 17])
def test_masked_table_is_the_fit_of_the_kept_pixels(pair, N):
    """rule 7: the masked splat skips M < 128 and is lut_ref.splat of the kept subsequence — written here pixel by pixel, against region_ref's slicing — in any order"""
    src, res = pair["src"].reshape(-1, 3), pair["plain"].reshape(-1, 3)
    for kind in ("half", "ramp", "random"):
        m = region_ref.mask(kind, SH, SW).reshape(-1)
        W, R = region_ref.splat(src, res, m, N)
        idx = [i for i in range(len(m)) if m[i] >= 128]
        W2, R2 = lut_ref.splat(src[idx[::-1]], res[idx[::-1]], N)
        assert np.array_equal(W, W2) and np.array_equal(R, R2)
        assert int(W.astype(object).sum()) == lut_ref.W3 * len(idx)
    assert not region_ref.kept(region_ref.mask("empty", SH, SW)).any()


def run_cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args, word", [
    (["-mask", "masks", "-fullres", "2"], "-fullres 2"),
    (["-mask", "masks", "-seq", "1"], "-seq 1"),
    (["-mask", "masks", "-maskprotect", "2"], "-maskprotect"),
    (["-maskprotect", "1"], "-maskprotect"),
])
def test_cli_refuses_bad_mask_flags(tmp_path, args, word):
    """the flags are checked before any model, input, output directory or device is touched: a failing exit code and an Error line that names the flag"""
    r = run_cli("-m", str(tmp_path), "-i", str(tmp_path), "-o", str(tmp_path / "out"), "-g", "0", *args)
    assert r.returncode != 0, (r.returncode, r.stdout)
    line = [t for t in r.stdout.split("\n") if t.startswith("Error:")]
    assert len(line) == 1 and word in line[0] and "-mask" in line[0], r.stdout
    assert not os.path.exists(tmp_path / "out")


def test_abi_symbols_exist():
    import nct
    l = ctypes.CDLL(nct.LIB_PATH)
    for name in ("nct_region_params_default", "nct_resize_u8c1", "nct_resize_u8c1_dev", "nct_region_mix", "nct_region_mix_dev", "nct_region_compose", "nct_region_compose_dev",
                 "nct_pair_set_region", "nct_pair_run_region_levels", "nct_process_pair_region", "nct_process_pair_fullres_region", "nct_process_pair_fullres_finish_region",
                 "nct_lut_fit_masked", "nct_lut_fit_masked_dev"):
        assert hasattr(l, name) and name in nct.SIGNATURES, name
    p = nct.RegionParams.default()
    assert p.protect == 0 and ctypes.sizeof(nct.RegionParams) == 4 and ctypes.sizeof(nct.RegionLevels) == 80
    hdr = open(os.path.join(nct.REPO_ROOT, "include", "nct.h")).read()
    assert "mask" in hdr and nct.lib().nct_version() == 118
