"""S2 (k_wls_mg.hip) on the grid shapes that change its hierarchy (tests/s2_shapes.py): every case through nct_color_finish — no kNN graph, no VGG weights, S2 on the
full H x W grid — against the mirror (oracle/orc_wls_mg.c) on bit patterns and against the exact float64 solve within the project's S2 bound and the tighter
s2_shapes.MIRROR_DEV_BOUND (tests/test_s2_shapes.py shows on the CPU that the mirror itself solves the system at every one of these shapes).

Read before the first run, once with H == 1 and once with W == 1 in mind, for an access outside an array at an accepted shape; none was found:
 * nb_mask / coup8 / px_coef: every read at i - 1, i - W, i - W + 1, i - W - 1 sits behind its existence bit; with W == 1 the index i - W + 1 is i itself and the bit
   (xr && yu) is off; a 5-point level never touches the diagonal arrays (null on level 0).
 * mg_weights_at: a one-row grid has only coarse points and row line points (r = 0), whose denominators take w[2] = w[3] = 0; mg_pstencil_at and mg_galerkin_at test
   y, x against H, W before every fine-point read and the coarse neighbour (jok) before every column of P; mg_pweights_at tests Y < C.H, X < C.W, and its index
   (r - 2Y + 1) * 3 + (c - 2X + 1) stays in 0 .. 8. fpst holds ceil(H/2) * ceil(W/2) columns, the coarse level's n.
 * k_mg_down / k_mg_up: `valid` keeps only threads whose pixel is inside the grid (one row of the thread grid when H == 1); lds_op reads a neighbour only behind its
   existence bit, and only from ring(k >= 1), so the LDS index stays inside the tile; the restriction's nine reads and the prolongation's parents are predicated the
   same way (an even-sized side ends in a line point with one parent: e1 = xr / yd). Coarse indices (gy >> 1) * Wc + (gx >> 1) are below the coarse n.
 * k_mg_lines_setup / k_mg_block: pieces of length 1 take line_solve's general path (y(0) = r(0), e(0) = y(0) lp(0), no read at k >= len); the cross terms test
   ly + 1 < bh, ly > 0, lx + 1 < bw, lx > 0; the post step's halo tile is filled and read behind the same image-border tests.
 * mg_tile_of_block: a bijection of [0, ntiles) for every ntiles, fewer than eight included (q = 0: the identity).
 * k_mg_mid: the plan (nct_wls_plan.h) admits depth d only up to mid_cap(d) points, which is what sA / sB / sC and the stash offsets are sized for, at a 2x shrink as at 4x (the caps
   bind earlier and more levels stay on tile launches); depth 3 is capped at 64 points, i.e. it is always the coarsest grid, so the run has at most four levels.
   mid_op, mid_restrict and mid_prolong index behind existence tests. The coarsest wave's lane index (i + dy W + dx) & 63 is used only behind the existence bit.
 * k_mg_setup_tail: strides of 1024 over n of either level; LvlPack holds MG_MAXL = 12 levels and the plan refuses a grid that needs more; pst is sized for level 1, the largest.
 * nctk_wls_solve_mg refuses a grid of 64 points or fewer from its plan, before it reserves an array or starts an S2 kernel: what has run by then is the Lab conversion, the copy or
   resize, k_roughness, k_gradient_weights and k_wls_system, all one thread per pixel behind i < n (and, for nct_local_color_transfer, T1 / T2 / S1, whose
   operator walks pixels linearly and tests x, y against w, h). lin_coef clamps its source index into [0, size - 1], so U1 from a one-row or one-column grid stays inside.
"""
import numpy as np
import pytest

import nct
import s2_shapes as S
from test_gpu_vs_ref64 import _check_after_s1, _check_pair, _lab2bgr_of, vgg  # noqa: F401 (vgg: fixture)

pytestmark = pytest.mark.gpu
ERR_INVALID = -2                       # nct.h NCT_ERR_INVALID: what ctx->fail(NCT_ERR_INVALID, ...) returns and the binding raises


def _params(flags=0):
    p = nct.Params.default()
    p.flags = flags
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _run(c, H, W, kind="cos", level=None, flags=0):
    ab, (h, w), s = S.case_inputs(H, W, kind, level)
    return c.color_finish(ab, h, w, H, W, s, _params(flags), want_stages=True)


def _equals_mirror(got, st, exp_bgr, exp, tag):
    for k in ("ab_up", "roughness", "ab_wls"):
        assert np.array_equal(_bits(st[k]), _bits(exp[k])), (tag, k, int((_bits(st[k]) != _bits(exp[k])).sum()))
    assert list(st["wls_iters"]) == list(exp["wls_iters"]), tag
    assert np.array_equal(got, exp_bgr), tag


def _vs_exact(c, got, st, H, W, kind, level=None, step_bound=False):
    """_check_after_s1 from the GPU's own ab_up and roughness, and the measured bound on top of the project's"""
    ab, (h, w), s = S.case_inputs(H, W, kind, level)
    flab = c.bgr2lab(s).reshape(-1, 3) / 255.0
    stats = {}
    _check_after_s1(_lab2bgr_of(c), dict(st, ab_nonlocal=ab), got, H, W, h, w, flab, step_bound=step_bound, stats=stats)
    print(f"s2-shape gpu {H}x{W} {kind} level={level}: iters {[int(v) for v in st['wls_iters']]} dev {stats['s2_frac']:.3g} of the S2 bound")
    assert stats["s2_frac"] <= S.MIRROR_DEV_BOUND, stats


@pytest.mark.parametrize("shape", S.HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_equal_size_matches_mirror_and_exact(ctx, oracle, shape):
    H, W = shape
    exp_bgr, exp = S.mirror(oracle, H, W)
    got, st = _run(ctx, H, W)
    _equals_mirror(got, st, exp_bgr, exp, shape)
    _vs_exact(ctx, got, st, H, W, "cos")


@pytest.mark.parametrize("shape", S.THIN, ids=lambda s: f"{s[0]}x{s[1]}")
def test_thin_flat_source_matches_mirror_and_exact(ctx, oracle, shape):
    """runs of one colour along the thin grid: the coupling contrasts the block step is for"""
    H, W = shape
    exp_bgr, exp = S.mirror(oracle, H, W, "flat")
    got, st = _run(ctx, H, W, "flat")
    _equals_mirror(got, st, exp_bgr, exp, shape)
    _vs_exact(ctx, got, st, H, W, "flat")


@pytest.mark.parametrize("shape", S.THIN + [(337, 321)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_solve_same_bits(ctx, oracle, shape):
    """NCT_FLAG_LATENCY: the 3 + 3 solve, its second half on the helper thread, gives the 6-wide solve's bits and six iteration counts"""
    H, W = shape
    exp_bgr, exp = S.mirror(oracle, H, W)
    got1, st1 = _run(ctx, H, W, flags=nct.FLAG_LATENCY)
    got0, st0 = _run(ctx, H, W)
    _equals_mirror(got1, st1, exp_bgr, exp, shape)
    _equals_mirror(got1, st1, got0, st0, shape)


@pytest.mark.parametrize("kind", ["cos", "flat"])
def test_block_step_off_matches_its_mirror(oracle, kind, monkeypatch):
    """NCT_S2_LINES=0 in a fresh context against orc_set_mg_lines(0), on the thin shapes"""
    monkeypatch.setenv("NCT_S2_LINES", "0")
    with nct.Context(0) as c:
        for H, W in S.THIN:
            exp_bgr, exp = S.mirror(oracle, H, W, kind, False)
            got, st = _run(c, H, W, kind)
            _equals_mirror(got, st, exp_bgr, exp, (H, W, kind))
            on = S.mirror(oracle, H, W, kind)[1]
            assert not np.array_equal(_bits(on["ab_wls"]), _bits(exp["ab_wls"])), (H, W, "the hook is meant to change the cycle")


@pytest.mark.parametrize("case", S.UPSAMPLE, ids=lambda c: f"{c[0][0]}x{c[0][1]}-to-{c[1][0]}x{c[1][1]}")
def test_upsampling_from_thin_level_grids(ctx, oracle, case):
    """U1 reads a level grid of one or two rows / one column: the mirror's bits; ref64.resize_linear_f64 and the exact solve through _check_after_s1"""
    level, (H, W) = case
    exp_bgr, exp = S.mirror(oracle, H, W, "cos", True, level)
    got, st = _run(ctx, H, W, level=level)
    _equals_mirror(got, st, exp_bgr, exp, case)
    _vs_exact(ctx, got, st, H, W, "cos", level, step_bound=True)


def test_pair_17x520_levels_vs_ref64(ctx, vgg):  # noqa: F811
    """a whole 17x520 pair (reference 40x23, bds 0.0, as test_ref64_oracle.PAIR_CASES[2]): every level's S2 runs on the 17x520 grid, whose hierarchy ends 2x33, 1x17,
    fed by the product's own S1 output from level grids 2x33 .. 17x520"""
    import synth
    assert S.describe(17, 520)["levels"][-2:] == [(2, 33), (1, 17)]
    _check_pair(ctx, vgg, synth.image(1000, 17, 520), synth.image(1001, 40, 23), 0.0, "17x520")


def _lct_args(h, w):
    """a valid nct_local_color_transfer call at equal size: any graph with ids inside the grid will do (the call is refused behind S1)"""
    import synth
    n = h * w
    ids = ((np.arange(n)[:, None] + np.arange(1, 9)[None, :]) % n).astype(np.int32)
    err = -np.random.default_rng(h * 100 + w).random((h, w)).astype(np.float32)
    s = synth.image(3, h, w)
    return err, s, synth.image(4, h, w), s, ids, np.full((n, 8), 0.5), 4


def test_refused_grids_leave_the_context_usable():
    """64 points or fewer, through both entry points: NCT_ERR_INVALID with "unsupported grid" — a return of nctk_wls_solve_mg in front of every S2 kernel — and the
    next valid call (17x17) gives a fresh context's bits: the refused call's arena blocks went back"""
    with nct.Context(0) as fresh:
        want, want_st = _run(fresh, 17, 17)
    with nct.Context(0) as c:
        for H, W in S.REFUSED:
            ab, _, s = S.case_inputs(H, W)
            with pytest.raises(nct.NctError) as e:
                c.color_finish(ab, H, W, H, W, s, _params(), want_stages=True)
            assert e.value.code == ERR_INVALID and "unsupported grid" in str(e.value), (H, W, str(e.value))
            with pytest.raises(nct.NctError) as e:
                c.local_color_transfer(*_lct_args(H, W), want_stages=True)
            assert e.value.code == ERR_INVALID and "unsupported grid" in str(e.value), (H, W, str(e.value))
            got, st = _run(c, 17, 17)
            _equals_mirror(got, st, want, want_st, (H, W))
