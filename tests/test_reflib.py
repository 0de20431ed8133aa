"""Reference libraries (SPEC §6.21) without a GPU: the binding's surface, the numpy rule (tests/reflib_ref.py) on hand-computed cases, the int32 bound of rule D2, the
host object and rule D4 of csrc/nct_reflib_host.h under the host sanitizers, and whether the rule does what it is for — on five one-texture stills with the oracle's
VGG19 and synthetic weights every source must rank its own texture first."""
import os
import subprocess

import numpy as np
import pytest

import nct
import reflib_ref as R

NAMES = ("nct_feat_quantize8", "nct_feat_quantize8_dev", "nct_descriptor_match", "nct_descriptor_match_dev", "nct_descriptor_match_bench", "nct_reflib_params_default",
         "nct_reflib_create", "nct_reflib_add", "nct_reflib_info", "nct_reflib_rows", "nct_reflib_from_rows", "nct_reflib_free", "nct_reflib_rank", "nct_reflib_release")


def test_binding_surface():
    l = nct.lib()
    for n in NAMES:
        assert n in nct.SIGNATURES, n
        assert hasattr(l, n), n
    for n in ("feat_quantize8", "descriptor_match", "reflib_rank", "reflib_release"):
        assert callable(getattr(nct.Context, n)), n
    for n in ("add", "info", "rows", "from_rows", "close"):
        assert callable(getattr(nct.RefLib, n)), n
    assert nct.lib().nct_version() == 118


def test_reflib_object_needs_no_context():
    rng = np.random.default_rng(3)
    rows = rng.integers(-128, 128, (7, 256), dtype=np.int8)
    mu = rng.random(256, dtype=np.float32)
    L = nct.RefLib.from_rows(3, rows, [0, 2, 3, 7], mu)
    assert L.info() == (3, 256, 3, 7, True)
    r, o, m = L.rows()
    assert np.array_equal(r, rows) and o.tolist() == [0, 2, 3, 7] and np.array_equal(m, mu)
    L.close()
    E = nct.RefLib(5)
    assert E.info() == (5, 512, 0, 0, False) and E.rows()[1].tolist() == [0] and E.rows()[2] is None
    for bad, word in ((lambda: nct.RefLib(6), "tap"), (lambda: nct.RefLib(3, C_=128), "C must be 256"),
                      (lambda: nct.RefLib.from_rows(3, rows, [0, 2, 2, 7]), "entry 1"), (lambda: nct.RefLib.from_rows(3, rows[:, :128], [0, 7]), "C must be 256"),
                      (lambda: nct.RefLib.from_rows(3, rows, [1, 7]), "offsets[0]"), (lambda: nct.RefLib.from_rows(3, rows, [0]), "N must be")):
        with pytest.raises(nct.NctError) as e:
            bad()
        assert e.value.code == -2 and word in str(e.value), str(e.value)


def test_int32_bound_on_partial_sums():
    """|d| <= 128 (the match takes any int8) and C <= 4096: the sum of the magnitudes of one dot product's terms, which bounds every partial sum in any order, is
    4096 * 128 * 128 = 2^26 < 2^31; descriptors (|d| <= 127) stay below 4096 * 127^2"""
    worst = np.full((1, 4096), -128, np.int8)
    assert R.partial_sum_bound(worst, worst) == 4096 * 128 * 128 == 2 ** 26 < R.I32
    assert int(R.products(worst, worst)[0, 0]) == 2 ** 26
    d = np.full((2, 4096), 127, np.int8); d[1] = -127
    assert R.partial_sum_bound(d, d) == 4096 * 127 * 127 < R.I32
    # a row of N1 has unit norm: its int8 image has |d|^2 <= (sqrt(C) / 2 + 127)^2 by the triangle inequality, so a real dot product is far smaller still
    rng = np.random.default_rng(1)
    a, b = rng.integers(-128, 128, (33, 512), dtype=np.int8), rng.integers(-128, 128, (65, 512), dtype=np.int8)
    A, B = a.astype(np.int64), b.astype(np.int64)
    running = np.cumsum(A[:, None, :] * B[None, :, :], axis=2)
    assert np.abs(running).max() <= R.partial_sum_bound(a, b) < R.I32


def test_hand_computed_3_by_2():
    a = np.array([[1, 0], [0, 2], [1, 1]], np.int8)             # na = 3
    b = np.array([[3, 0], [0, 1]], np.int8)                     # nb = 2
    # P = [[3, 0], [0, 2], [3, 1]]: row maxima 3, 2, 3; column maxima 3, 2
    assert R.products(a, b).tolist() == [[3, 0], [0, 2], [3, 1]]
    assert R.match(a, b) == (8, 5)
    assert R.key(8, 5, 3, 2) == 8 * 1024 // 3 + 5 * 1024 // 2 == 2730 + 2560
    assert R.key(8, 5, 3, 2, wf=0, wb=1) == 2560 and R.key(8, 5, 3, 2, wf=1, wb=0) == 2730 and R.key(8, 5, 3, 2, wf=16, wb=3) == 16 * 2730 + 3 * 2560
    # floor, not truncation, on a negative sum
    assert R.key(-8, -5, 3, 2) == -2731 + -2560
    # equal keys: the lower index first; a larger key in front of both
    o, k, f, bw = R.rank(a, [b, b.copy(), 2 * b])
    assert k.tolist() == [5290, 5290, 2 * 8 * 1024 // 3 + 10 * 1024 // 2] and o.tolist() == [2, 0, 1]
    assert R.rank(a, [b, 2 * b, b], wf=0)[0].tolist() == [1, 0, 2] and R.rank(a, [2 * b, b, 2 * b], wb=0)[0].tolist() == [0, 2, 1]


def test_all_negative_products():
    """a all positive, b all negative: every product is negative and the maxima are the LEAST negative ones — a padded zero would win"""
    a = np.array([[1, 2], [3, 1], [2, 2]], np.int8)
    b = np.array([[-1, -1], [-2, -3]], np.int8)
    assert R.products(a, b).tolist() == [[-3, -8], [-4, -9], [-4, -10]]
    assert R.match(a, b) == (-3 - 4 - 4, -3 - 8)
    assert R.key(-11, -11, 3, 2) == (-11 * 1024) // 3 + (-11 * 1024) // 2 == -3755 - 5632


def test_host_object_under_sanitizers(tmp_path):
    """csrc/nct_reflib_host.h — the object's offsets and checks, the key and the order — in a stand-alone program under AddressSanitizer + UBSan"""
    exe = str(tmp_path / "reflib_host_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(nct.PKG_ROOT, "csrc"),
                        os.path.join(os.path.dirname(__file__), "reflib_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(9)
    ranks = []
    for N in (1, 2, 7, 64):
        na = int(rng.integers(1, 65537))
        rows = [(int(rng.integers(-2 ** 42, 2 ** 42)), int(rng.integers(-2 ** 42, 2 ** 42)), int(rng.integers(1, 65537))) for _ in range(N)]
        if N == 7:
            rows[5] = rows[2]; rows[6] = rows[2]                 # ties
        ranks.append((na, int(rng.integers(0, 17)), int(rng.integers(1, 17)), rows))
    ranks.append((3, 1, 1, [(8, 5, 2), (-8, -5, 2), (8, 5, 2)]))
    lines = ["tap 3 256", "tap 0 64", "tap 5 256",
             "table 16 3 0 5 6 300", "table 32 2 0 65536 65537", "table 24 1 0 5", "table 16 0 0", "table 16 2 0 5 5", "table 16 2 0 5 70000", "table 16 1 1 5",
             "table 4096 9 0 65536 131072 196608 262144 327680 393216 458752 524288 589824", "table 16 4097 " + " ".join(str(i) for i in range(4098))]
    lines += ["rank %d %d %d %d " % (na, wf, wb, len(rows)) + " ".join("%d %d %d" % t for t in rows) for na, wf, wb, rows in ranks]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    assert out[0] == "ok" and "tap must be in [1, 5]" in out[1] and "C must be 512 at tap 5" in out[2]
    s3 = sum((k + 1 - 3 * (c % 7)) * n for k, n in enumerate((5, 1, 294)) for c in range(16))
    assert out[3] == "lib 3 300 3 0 5 6 300 %d refusals-ok" % s3
    s4 = sum((k + 1 - 3 * (c % 7)) * n for k, n in enumerate((65536, 1)) for c in range(32))
    assert out[4] == "lib 2 65537 2 0 65536 65537 %d refusals-ok" % s4
    assert "C must be a multiple of 16" in out[5] and "N must be in [1, 4096]" in out[6] and "entry 1 must hold 1 to 65536 rows (got 0)" in out[7]
    assert "entry 1 must hold 1 to 65536 rows (got 69995)" in out[8] and "offsets[0] must be 0" in out[9] and "exceed 2^31 bytes" in out[10] and "N must be in [1, 4096]" in out[11]
    for ln, (na, wf, wb, rows) in zip(out[12:], ranks):
        keys = [R.key(f, b, na, nb, wf, wb) for f, b, nb in rows]
        assert ln == "key " + " ".join(str(k) for k in keys) + " order " + " ".join(str(int(i)) for i in R.order(keys)), ln
    assert out[-1].endswith("order 0 2 1")


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


def test_rule_ranks_each_texture_first(oracle, weights):
    """Five stills of ONE texture each (diagonal stripes, checkerboard, horizontal bars, vertical bars, dots; grey values 170 / 90, noise +-6, a tint each) and five
    sources — the same textures with new noise and a shifted phase, untinted. Tap 3, centred on the library's mean tap vector: every source ranks its own texture first.
    Margins first - second as a fraction of the full scale 2 * 1024 * 127^2, printed per source (DESIGN.md §3.26 records them, and the uncentred ones)."""
    tap = 3
    lt = [oracle.vgg19_features(i, *weights, deepest_tap=tap)[tap - 1] for i in R.fixture_library()]
    st = [oracle.vgg19_features(i, *weights, deepest_tap=tap)[tap - 1] for i in R.fixture_sources()]
    full = 2 * 1024 * 127 * 127
    firsts = {}
    for name, mu in (("centred", R.library_center(lt)), ("uncentred", None)):
        ents = [R.quantize8(oracle, F, mu) for F in lt]
        firsts[name] = []
        for i, F in enumerate(st):
            a = R.quantize8(oracle, F, mu)
            assert max(R.partial_sum_bound(a, e) for e in ents) < R.I32
            o, k, _, _ = R.rank(a, ents)
            print("%s source %d (%s): order %s, margin %.4f of the full scale" % (name, i, R.TEXTURES[i], o.tolist(), (k[o[0]] - k[o[1]]) / full))
            firsts[name].append(int(o[0]))
    assert firsts["centred"] == [0, 1, 2, 3, 4]
