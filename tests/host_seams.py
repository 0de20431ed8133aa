"""The host-pointer seams as a table: inputs from tests/synth.py and a fixed seed at sizes the caller chooses, every optional argument present or — named in `drop` —
absent. Shared by tests/test_gpu_host_seams.py (small grids, one argument absent at a time) and scripts/arena_probe.py's `seams` mode (large ones, all present / all
absent). A seam is (name, the names of its optional arguments, call(c, d, drop) -> dict of what the call returned); d: the arrays of data(). Where the binding has no
switch for an argument the C entry point is called directly."""
import ctypes as C
import types

import numpy as np

import nct
import synth
from fullres_ref import smooth_ab


def sizes(h, w, H, W, C_, N, bh=None, bw=None):
    """h x w: the level grid; H x W: the image / finish target; C_: feature channels; N: LUT lattice; bh x bw: the other map of a field (default: 1 larger / smaller)"""
    return types.SimpleNamespace(h=h, w=w, H=H, W=W, C=C_, N=N, bh=bh or h + 1, bw=bw or max(w - 1, 2), K=2)


def data(s, seed=7):
    rng = np.random.default_rng(seed)
    n, d = s.h * s.w, types.SimpleNamespace(s=s)
    u8 = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)
    d.fa, d.fb = synth.features(seed, s.C, s.h, s.w), synth.features(seed + 1, s.C, s.bh, s.bw)
    d.ann, d.bnn = synth.random_nnf(seed, s.h, s.w, s.bh, s.bw), synth.random_nnf(seed + 1, s.bh, s.bw, s.h, s.w)
    d.img, d.img_b = synth.image(seed, s.h, s.w), synth.image(seed + 1, s.bh, s.bw)
    d.full = synth.image(seed + 2, s.H, s.W)
    d.lab, d.lab_prev = u8(s.h, s.w, 3), u8(s.h, s.w, 3)
    d.lab_prev[: s.h // 2] = d.lab[: s.h // 2]                                       # half the grid unchanged: tau_p and the hold weights take both ends of their range
    d.errs = [-rng.random((s.h, s.w)).astype(np.float32) for _ in range(s.K)]
    d.guides = [u8(s.h, s.w, 3) for _ in range(s.K)]
    d.prev_label = rng.integers(0, s.K, (s.h, s.w)).astype(np.uint8)
    d.label = rng.integers(0, s.K, (s.h, s.w)).astype(np.uint8)
    d.field = rng.integers(-2, 3, (s.h, s.w, 2)).astype(np.int16)
    d.parent = rng.integers(-3, 4, ((s.h - 1) // 2 + 1, (s.w - 1) // 2 + 1, 2)).astype(np.int16)
    d.pulled = [u8(s.h, s.w) for _ in range(s.K)]
    d.prev, d.src_mask = u8(s.h, s.w), u8(s.h, s.w)
    d.x, d.x_prev = rng.standard_normal((2, n, 3)), rng.standard_normal((2, n, 3))
    d.ab = smooth_ab(seed, s.h, s.w)
    d.mask_full = u8(s.H, s.W)
    d.mask_full[: s.H // 3] = 0                                                      # a protected part: where the compose of a masked finish keeps the source
    d.res = synth.image(seed + 3, s.H, s.W)
    d.q = rng.integers(-3000, 3001, (n, s.C)).astype(np.int16)
    d.seeds_in, d.seeds_out = d.q[:: max(n // 5, 1)][:5].copy(), d.q[1:: max(n // 3, 1)][:3].copy()
    d.score = u8(s.h, s.w)
    return d


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _list(arrs):
    return (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])


def _feat_normalize(c, d, drop):
    r = c.feat_normalize(d.fa, want_resp="resp" not in drop)
    return {"dst": r} if "resp" in drop else {"dst": r[0], "resp": r[1]}


def _bds_vote_features(c, d, drop):
    r = c.bds_vote_features(d.ann, d.bnn, d.fb, 1.0, 2.0, want_pw="pw" not in drop)
    return {"pout": r} if "pw" in drop else {"pout": r[0], "pw": r[1]}


def _select_outputs(d, drop, more=()):
    s = d.s
    spec = {"label": ((s.h, s.w), np.uint8), "guide_out": ((s.h, s.w, 3), np.uint8), "err_out": ((s.h, s.w), np.float32), "free_label": ((s.h, s.w), np.uint8),
            "margin": ((s.h, s.w), np.float64)}
    names = ("label", "guide_out", "err_out") + tuple(more)
    gone = set(drop) | ({"guide_out"} if "guides" in drop else set())              # without the guidance images there is no merged guide
    return names, {k: np.empty(*spec[k]) for k in names if k not in gone}


def _select_reference(c, d, drop):
    s = d.s
    names, outs = _select_outputs(d, drop)
    c._chk(c._l.nct_select_reference(c._h, _list(d.errs), None if "guides" in drop else _list(d.guides), s.K, s.h, s.w, *[_p(outs.get(k)) for k in names]))
    return outs


def _select_reference_hold(c, d, drop, field="given"):
    s = d.s
    names, outs = _select_outputs(d, drop, ("free_label", "margin"))
    f = None if "field" in drop else d.field if field == "given" else np.zeros_like(d.field)
    c._chk(c._l.nct_select_reference_hold(c._h, _list(d.errs), None if "guides" in drop else _list(d.guides), s.K, s.h, s.w, _p(d.prev_label), _p(d.lab), _p(d.lab_prev), _p(f),
                                          0.01, 10.0, *[_p(outs.get(k)) for k in names]))
    return outs


def _seq_pull_hold(c, d, drop, K=2, **neutral):
    """neutral: field / src_mask / pulled1 = True passes the neutral value (zeros, all 255) in the place of the given array"""
    pulled = [d.pulled[0], None if "pulled1" in drop else np.full_like(d.pulled[1], 255) if neutral.get("pulled1") else d.pulled[1]][:K]
    f = None if "field" in drop else np.zeros_like(d.field) if neutral.get("field") else d.field
    ms = None if "src_mask" in drop else np.full_like(d.src_mask, 255) if neutral.get("src_mask") else d.src_mask
    want = ["p"] + [k for k, o in (("m", "m_out"), ("p_free", "p_free")) if o not in drop]
    return c.seq_pull_hold(pulled, None if "label" in drop else d.label, d.prev, d.lab, d.lab_prev, f, ms, 0.7, 10.0, want=want)


def _seq_blend(c, d, drop, mc=False):
    x, tm = (c.seq_blend_mc(d.x, d.x_prev, d.lab, d.lab_prev, 0.7, 10.0, d.field, want_tau_map="tau_map" not in drop) if mc else
             c.seq_blend(d.x, d.x_prev, d.lab, d.lab_prev, 0.7, 10.0, want_tau_map="tau_map" not in drop))
    return {"x_out": x} if tm is None else {"x_out": x, "tau_map": tm}


def _seq_change(c, d, drop, zero=False):
    r = c.seq_change(d.lab, d.lab_prev, None if "field" in drop else np.zeros_like(d.field) if zero else d.field)
    return {"rec": np.array([r["sad"], r["changed"], r["pixels"]], np.uint64)}


def _lut_fit(c, d, drop, mask="none"):
    s = d.s
    src, res = d.full.reshape(-1, 3), d.res.reshape(-1, 3)
    m = {"none": None, "given": d.mask_full.reshape(-1), "all": np.full(s.H * s.W, 255, np.uint8)}[mask]
    prm = nct._lut_params(s.N, None)
    lut = np.empty((s.N, s.N, s.N, 3), np.float32)
    st = {k: np.empty(shape, t) for k, shape, t in (("weight", s.N ** 3, np.uint64), ("resid", (s.N ** 3, 3), np.int64), ("disp", (s.N ** 3, 3), np.float64)) if k not in drop}
    cs = nct.LutStages(*[_p(st.get(k)) for k in ("weight", "resid", "disp")])
    if mask == "none":
        c._chk(c._l.nct_lut_fit(c._h, _p(src), _p(res), len(src), C.addressof(prm), _p(lut), C.addressof(cs) if st else None))
    else:
        c._chk(c._l.nct_lut_fit_masked(c._h, _p(src), _p(res), _p(m), len(src), C.addressof(prm), _p(lut), C.addressof(cs) if st else None))
    return dict(st, lut=lut)


def _region_score(c, d, drop, empty_list=False):
    """seeds_out absent: n_out = 0 and a null list; empty_list: n_out = 0 and a list the call must not read"""
    so = None if "seeds_out" in drop else d.seeds_out
    n_out = 0 if so is None or empty_list else len(so)
    out = np.empty(len(d.q), np.uint8)
    c._chk(c._l.nct_region_score(c._h, _p(d.q), len(d.q), d.s.C, _p(d.seeds_in), len(d.seeds_in), _p(so), n_out, 1024, 700, _p(out)))
    return {"score": out}


def _finish(c, d, drop, guided, region, mask="given"):
    """the masked forms run with protect = 1: where the mask is 0 the source stays, so a mask acts (SPEC §6.11 rule 3); an all-255 mask keeps nothing"""
    s = d.s
    m = None if "mask" in drop else d.mask_full if mask == "given" else np.full_like(d.mask_full, 255)
    if guided:
        out = c.color_finish_guided_region(d.ab, d.lab, s.h, s.w, d.full, m, 1, sigma=10.0) if region else c.color_finish_guided(d.ab, d.lab, s.h, s.w, d.full, sigma=10.0)
    else:
        out = c.color_finish_upsample_region(d.ab, s.h, s.w, d.full, m, 1) if region else c.color_finish_upsample(d.ab, s.h, s.w, d.full)
    return {"out": out}


# the seams with an argument that may be NULL: name, those arguments, the call with everything given except `drop`
NULLABLE = [
    ("feat_normalize", ("resp",), _feat_normalize),
    ("bds_vote_features", ("pw",), _bds_vote_features),
    ("select_reference", ("guides", "label", "guide_out", "err_out"), _select_reference),
    ("select_reference_hold", ("field", "guides", "label", "guide_out", "err_out", "free_label", "margin"), _select_reference_hold),
    ("seq_pull_hold", ("pulled1", "field", "src_mask", "m_out", "p_free"), _seq_pull_hold),
    ("seq_pull_hold_k1", ("label",), lambda c, d, drop: _seq_pull_hold(c, d, drop, K=1)),
    ("seq_blend", ("tau_map",), _seq_blend),
    ("seq_blend_mc", ("tau_map",), lambda c, d, drop: _seq_blend(c, d, drop, mc=True)),
    ("seq_motion_field", ("parent",), lambda c, d, drop: {"m": c.seq_motion_field(d.lab, d.lab_prev, None if "parent" in drop else d.parent, 2, 8)}),
    ("seq_change", ("field",), _seq_change),
    ("lut_fit", ("weight", "resid", "disp"), _lut_fit),
    ("lut_fit_masked", ("weight", "resid", "disp"), lambda c, d, drop: _lut_fit(c, d, drop, mask="given")),
    ("region_score", ("seeds_out",), _region_score),
    ("region_refind", ("prior",), lambda c, d, drop: {"out": c.region_refind(d.score, (d.s.H, d.s.W), None if "prior" in drop else d.mask_full, 32)}),
    ("color_finish_upsample_region", ("mask",), lambda c, d, drop: _finish(c, d, drop, False, True)),
    ("color_finish_guided_region", ("mask",), lambda c, d, drop: _finish(c, d, drop, True, True)),
]
