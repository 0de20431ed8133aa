"""Several references (SPEC §6.2) on the GPU: the selection kernel against the numpy rule, whole runs against the composition of the oracle's stages
(tests/multi_ref.py) level by level, the K = 1 / repeated-reference identities, limits, arena stability and the console driver. All comparisons are equality of
bytes / bit patterns."""
import os
import subprocess
import numpy as np
import pytest
from PIL import Image

import multi_ref
import nct
import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "neural-color-transfer_amd", "bin", "neural_color_transfer")


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- seam: nct_select_reference against the numpy rule

def _maps(kind, K, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        errs = [(-rng.random((h, w))).astype(np.float32) for _ in range(K)]
    elif kind == "ties":
        errs = [(-rng.integers(0, 4, (h, w)) / 4.0).astype(np.float32) for _ in range(K)]
    elif kind == "nan":
        errs = [(-rng.random((h, w))).astype(np.float32) for _ in range(K)]
        for k in range(K):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            errs[k][y0:y0 + max(1, h // 3), x0:x0 + max(1, w // 3)] = np.nan
        errs[0].reshape(-1)[::7] = np.nan
    else:
        e = (-rng.random((h, w))).astype(np.float32)
        errs = [e.copy() for _ in range(K)]
    guides = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(K)]
    return errs, guides


@pytest.mark.parametrize("kind", ["random", "ties", "nan", "identical"])
@pytest.mark.parametrize("grid", [(1, 1), (1, 37), (53, 1), (44, 44), (175, 233)])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_select_reference_matches_the_numpy_rule(ctx, K, grid, kind):
    errs, guides = _maps(kind, K, grid[0], grid[1], 100 * K + grid[0] + grid[1])
    lab = multi_ref.select(errs)
    G, E = multi_ref.merge(lab, guides, errs)
    if kind == "identical" or K == 1:
        assert not lab.any()
    elif kind == "random" and grid[0] * grid[1] > 1000:
        assert min(multi_ref.shares(lab, K)) > 0.2 / K                     # every reference is selected somewhere: the comparison below is not vacuous
    got = ctx.select_reference(errs, guides)
    assert np.array_equal(got[0], lab)
    assert np.array_equal(got[1], G)
    assert np.array_equal(bits(got[2]), bits(E))                          # the selected fp32 words, NaN payloads included
    dev = ctx.select_reference_dev(errs, guides)
    assert np.array_equal(dev[0], lab) and np.array_equal(dev[1], G) and np.array_equal(bits(dev[2]), bits(E))
    only = ctx.select_reference(errs)                                      # without guidance images: labels and errors alone
    assert only[1] is None and np.array_equal(only[0], lab) and np.array_equal(bits(only[2]), bits(E))


# ---- whole runs against the composition

SRC = (1000, 64, 56)
REFS = [(1001, 48, 64), (1002, 72, 50), (1003, 60, 60)]


def _check_run(c, orc, weights, src, refs, levels, flags=0, min_share=0.05):
    """GPU multi run vs the composition, every level; returns (gpu result, expected level dict)"""
    ws, bs = weights
    K = len(refs)
    exp, elv = multi_ref.multi(orc, src, refs, ws, bs, levels=levels, lab2bgr_form=1 if flags & nct.FLAG_LAB2BGR_CUBE else 0)
    # a condition on the INPUTS, asserted on the expected labels before anything of the GPU's is looked at: every reference holds at least 5 % of the last level
    sh = multi_ref.shares(elv["label"][levels - 1], K)
    print("expected shares per level:", [[round(x, 3) for x in multi_ref.shares(l, K)] for l in elv["label"]])
    assert min(sh) >= min_share, sh
    prm = nct.Params.default(); prm.levels = levels; prm.flags = flags
    c.multi_upload(src, refs)
    got = c.multi_run_levels(prm)
    out = c.pair_download()
    for l in range(levels):
        for k in range(K):
            for name in ("ann", "bnn"):
                assert np.array_equal(got[name][k][l], elv[name][k][l]), (name, k, l)
            for name in ("annd", "bnnd", "ref_err"):
                assert np.array_equal(bits(got[name][k][l]), bits(elv[name][k][l])), (name, k, l)
            assert np.array_equal(got["ref_guide"][k][l], elv["ref_guide"][k][l]), ("ref_guide", k, l)
        assert np.array_equal(got["label"][l], elv["label"][l]), ("label", l)
        assert np.array_equal(got["guide"][l], elv["guide"][l]), ("guide", l)
        assert np.array_equal(bits(got["err"][l]), bits(elv["err"][l])), ("err", l)
        assert np.array_equal(got["result"][l], elv["result"][l]), ("result", l)
    assert np.array_equal(out, exp)
    return out, elv


@pytest.mark.parametrize("K,levels,flags", [(2, 5, 0), (2, 1, 0), (3, 5, 0), (3, 1, 0), (2, 5, nct.FLAG_LAB2BGR_CUBE | nct.FLAG_LATENCY)])
def test_multi_run_matches_the_composition_level_by_level(wctx, oracle, weights, K, levels, flags):
    src = synth.image(*SRC)
    refs = [synth.image(*r) for r in REFS[:K]]
    out, _ = _check_run(wctx, oracle, weights, src, refs, levels, flags)
    prm = nct.Params.default(); prm.levels = levels; prm.flags = flags
    assert np.array_equal(wctx.process_multi(src, refs, prm), out)           # the one-call form gives the same bytes
    for r in refs:                                                           # and the result is no single-reference result
        assert not np.array_equal(wctx.process_pair(src, r, prm), out)


def test_multi_run_on_the_natural_standins(wctx, oracle, weights):
    import natural_inputs
    d = natural_inputs.require()
    load = lambda n: np.ascontiguousarray(np.asarray(Image.open(os.path.join(d, n + ".png")).convert("RGB"))[..., ::-1])
    src, refs = load("in0"), [load("tar0"), load("tar1")]
    assert src.shape[:2] == (150, 226) and refs[0].shape[:2] == (200, 320) and refs[1].shape[:2] == (131, 233)
    out, _ = _check_run(wctx, oracle, weights, src, refs, 5)
    for r in refs:
        single = wctx.process_pair(src, r)
        mse = float(((single.astype(np.float64) - out) ** 2).mean())
        print("PSNR against the single-reference result: %.1f dB" % (10 * np.log10(255.0 ** 2 / mse) if mse else np.inf))
        assert mse > 0


# ---- identities

@pytest.mark.parametrize("levels", [5, 1])
def test_one_reference_is_process_pair(wctx, levels):
    src, ref = synth.image(*SRC), synth.image(*REFS[0])
    prm = nct.Params.default(); prm.levels = levels
    exp, tp = wctx.process_pair(src, ref, prm, want_timing=True)
    got, tm = wctx.process_multi(src, [ref], prm, want_timing=True)
    assert np.array_equal(got, exp)
    assert tm["pm_level_launches"] == tp["pm_level_launches"]
    wctx.multi_upload(src, [ref, ref])
    lv = wctx.multi_run_levels(prm)
    assert np.array_equal(wctx.pair_download(), exp)
    assert not any(lv["label"][l].any() for l in range(levels))
    assert lv["timing"]["pm_level_launches"][:levels] == [2 * n for n in tp["pm_level_launches"][:levels]]
    wctx.multi_upload(src, [ref])                                             # K = 1 through the level form: label 0, merged maps = reference 0's
    lv1 = wctx.multi_run_levels(prm)
    assert np.array_equal(wctx.pair_download(), exp)
    for l in range(levels):
        assert not lv1["label"][l].any() and np.array_equal(lv1["guide"][l], lv1["ref_guide"][0][l]) and np.array_equal(bits(lv1["err"][l]), bits(lv1["ref_err"][0][l]))


def test_one_reference_is_process_pair_at_350(wctx):
    src, ref = synth.image(7, 350, 350), synth.image(8, 300, 400)
    assert np.array_equal(wctx.process_multi(src, [ref]), wctx.process_pair(src, ref))


def test_alternating_calls_on_one_context_match_fresh_contexts(weights):
    s1, s2 = synth.image(*SRC), synth.image(11, 80, 70)
    r = [synth.image(*q) for q in REFS]
    calls = [("pair", s1, [r[0]]), ("multi", s1, r[:2]), ("pair", s2, [r[2]]), ("multi", s2, r), ("multi", s1, r[:1])]

    def run(c, kind, s, refs):
        return c.process_pair(s, refs[0]) if kind == "pair" else c.process_multi(s, refs)
    fresh = []
    for call in calls:
        with nct.Context(0) as c:
            c.vgg19_load_raw(*weights)
            fresh.append(run(c, *call))
    with nct.Context(0) as c:
        c.vgg19_load_raw(*weights)
        arena = []
        for rnd in range(4):
            for call, exp in zip(calls, fresh):
                assert np.array_equal(run(c, *call), exp), (rnd, call[0], len(call[2]))
            arena.append(c.counter(nct.CTR_ARENA_BYTES))
        print("arena bytes per round:", arena)
        assert arena[1] == arena[2] == arena[3]


# ---- limits

def test_limits(wctx):
    src, ref = synth.image(*SRC), synth.image(*REFS[0])
    for refs, word in (([], "references"), ([ref] * 9, "references"), ([ref, None], "null"), ([ref, synth.image(5, 16, 40)], "sides")):
        with pytest.raises(nct.NctError) as e:
            wctx.process_multi(src, refs)
        assert e.value.code == -2 and word in str(e.value), str(e.value)
    e1 = np.zeros((4, 4), np.float32)
    for K in (0, 9):
        with pytest.raises(nct.NctError) as e:
            wctx.select_reference([e1] * K)
        assert e.value.code == -2 and "K must be in" in str(e.value)
    assert np.array_equal(wctx.process_multi(src, [ref]), wctx.process_pair(src, ref))          # the context is still usable


# ---- console driver

def test_cli_comma_line(tmp_path, wctx, weights):
    from caffemodel_io import write_caffemodel
    ws, bs = weights
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    inp = tmp_path / "in"; (inp / "sub").mkdir(parents=True)
    a, b, c = synth.image(*SRC), synth.image(*REFS[0]), synth.image(*REFS[1])
    Image.fromarray(a[..., ::-1].copy()).save(inp / "a.png"); Image.fromarray(b[..., ::-1].copy()).save(inp / "sub" / "b.png")
    Image.fromarray(c[..., ::-1].copy()).save(inp / "c.png")
    (inp / "pairs.txt").write_text("a.png sub/b.png,c.png 2.0\na.png c.png 0.5\n")
    read = lambda p: np.asarray(Image.open(p).convert("RGB"))[..., ::-1]
    pm = nct.Params.default(); pm.bds_weight = 2.0
    pp = nct.Params.default(); pp.bds_weight = 0.5
    exp_multi, exp_pair = wctx.process_multi(a, [b, c], pm), wctx.process_pair(a, c, pp)

    out = tmp_path / "out"
    r = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(out), "-g", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == ["a_b+c_2.00.png", "a_c_0.50.png", "status.jsonl"]
    assert np.array_equal(read(out / "a_b+c_2.00.png"), exp_multi) and np.array_equal(read(out / "a_c_0.50.png"), exp_pair)
    assert r.stdout.count("Read style file:") == 3

    vis = tmp_path / "vis"
    r = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(vis), "-g", "0", "-vis", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(read(vis / "a_b+c_2.00.png"), exp_multi) and np.array_equal(read(vis / "a_c_0.50.png"), exp_pair)
    wctx.multi_upload(a, [b, c])
    lv = wctx.multi_run_levels(pm)
    for l in range(5):
        im = Image.open(vis / ("a_b+c_2.00_label_%d.png" % l))
        assert im.mode == "L"
        assert np.array_equal(np.asarray(im), lv["label"][l] * 255)                    # K = 2: label * (255 // 1)

    full = tmp_path / "full"
    r = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(full), "-g", "0", "-fullres", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "-fullres 1 cannot be combined with several references" in r.stdout
    assert sorted(os.listdir(full)) == ["a_c_0.50.png", "status.jsonl"]
    assert np.array_equal(read(full / "a_c_0.50.png"), exp_pair)                        # nothing is shrunk at this size: -fullres gives process_pair's bytes
