"""What the binding's eleven "levels" report methods hand the library, pinned on the CPU (no device, no GPU mark).

A context made without nct_create gets a stub in place of the library handle: every entry point records its arguments and returns 0, while nct.lib() stays the real
library (nct_working_size and the *_default calls answer truthfully). For each case the module derives a description and compares it for equality with
tests/golden/binding_reports.json, which `python tests/test_binding_reports.py --record` wrote from the binding as it stood before its report methods were folded:

  "frame"  the returned frame's dtype and shape, where the method returns one
  "dict"   the returned dict: its keys and, per key, dtypes and shapes ("zero": the arrays hold zeros; the colour stage's maps are np.empty and carry no such word);
           "dims" / "adims" / "bdims" by value
  "call"   the library function and its arguments: scalars by value, every report struct read back inside the call (<Struct>.from_address) with each pointer named
           after the returned array whose .ctypes.data it equals, "null", or "private" with dtype, shape and byte size of the live array behind it (found in the frames
           of the call, so an array that was let go before the call shows as DANGLING); a pointer to a nct_color_stages is "color[l]" when its seven pointers are
           the seven arrays of that returned entry. Neighbours that count up or repeat are written once: "mask[0..2] null*2"
  "attrs"  _pair_shape and _multi_shapes on the context afterwards (pair_download, pair_set_region and tests/test_gpu_lut.py read them)
"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np

if __name__ == "__main__":
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(_repo, "neural-color-transfer_amd", "python"))

import nct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_reports.json")

SRC, REFS = (40, 56), [(33, 47), (48, 40)]                       # pairs, lists and working-size sequences
FULL_SRC, FULL_REFS, MAX_SIDE = (90, 120), [(70, 100), (96, 80)], 60      # full-resolution sequences
UNINITIALISED = ("ab_local", "ab_nonlocal", "ab_up", "roughness", "ab_wls")     # np.empty: the library writes every element of a level that runs

# the arguments after the context, by role: "int" a scalar; "image" / "src" / "out" an image; "ints" / "ptrs" a C array; "color" a void*[5] of nct_color_stages; a struct's name
_FRAME = ("src", "out", "PairTiming")
ROLES = {
    "nct_pair_run_levels": ("Params", "PairTiming", "PairLevels"),
    "nct_pair_run_region_levels": ("Params", "PairTiming", "PairLevels", "RegionLevels"),
    "nct_multi_run_levels": ("Params", "PairTiming", "MultiLevels"),
    "nct_multi_run_ref_region_levels": ("Params", "PairTiming", "MultiLevels", "RefRegionLevels"),
    "nct_seq_frame_levels": _FRAME + ("PairLevels", "SeqLevels"),
    "nct_seq_frame_region_levels": _FRAME + ("PairLevels", "SeqLevels", "RegionLevels"),
    "nct_seq_frame_multi_levels": _FRAME + ("MultiLevels", "SeqLevels", "SeqHoldLevels"),
    "nct_seq_frame_multi_stage_levels": _FRAME + ("MultiLevels", "color", "SeqLevels", "SeqHoldLevels"),
    "nct_seq_frame_ref_region_levels": _FRAME + ("MultiLevels", "color", "SeqLevels", "SeqHoldLevels", "RefRegionLevels", "SeqPullLevels"),
    "nct_seq_frame_propagate_levels": _FRAME + ("SeqLevels",),
    "nct_seq_frame_propagate_region_levels": _FRAME + ("SeqLevels", "RegionLevels"),
    "nct_seq_frame_propagate_ref_region_levels": _FRAME + ("SeqLevels", "RefRegionLevels", "SeqPullLevels"),
    "nct_seq_begin": ("image",) + ("int",) * 4 + ("Params", "SeqParams"),
    "nct_seq_begin_fullres": ("image",) + ("int",) * 6 + ("Params", "SeqParams"),
    "nct_seq_begin_multi": ("int", "ptrs", "ints", "ints", "int", "int", "Params", "SeqParams", "SeqHold"),
    "nct_seq_begin_multi_fullres": ("int", "ptrs", "ints", "ints") + ("int",) * 4 + ("Params", "SeqParams", "SeqHold"),
}
PARAM_FIELDS = {"Params": ("levels",), "SeqParams": ("tau", "sigma"), "SeqHold": ("hold",), "PairTiming": ()}


def _addr(a):
    """the address an argument stands for, as the declared argument types would pass it"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if isinstance(a, C.c_void_p):
        return a.value
    if isinstance(a, (C.Structure, C.Array)):
        return C.addressof(a)
    return int(a) or None


def _live(stop_code):
    """every numpy array and ctypes structure the frames of the running call still reference (through locals and their lists, tuples and dicts) -> by address"""
    arrays, structs, seen = {}, set(), set()

    def walk(v, depth):
        if id(v) in seen or depth > 6:
            return
        seen.add(id(v))
        if isinstance(v, np.ndarray):
            arrays.setdefault(v.ctypes.data, v)
        elif isinstance(v, C.Structure):
            structs.add(C.addressof(v))
        elif isinstance(v, (list, tuple)):
            for x in v:
                walk(x, depth + 1)
        elif isinstance(v, dict):
            for x in v.values():
                walk(x, depth + 1)
    f = sys._getframe(2)
    while f is not None and f.f_code is not stop_code:
        walk(dict(f.f_locals), 0)
        f = f.f_back
    return {p: "%s %s %dB" % (a.dtype, "x".join(map(str, a.shape)), a.nbytes) for p, a in arrays.items()}, structs


def _pointers(v):
    """a struct field or C array of pointers -> nested lists of addresses (None: null)"""
    if isinstance(v, C.Array):
        return [_pointers(x) for x in v]
    return v or None


def _stages(p, structs):
    """a nct_color_stages read back -> (whether a live ColorStages stands at p, its seven pointers)"""
    st = nct.ColorStages.from_address(p)
    return (p in structs, [getattr(st, k) or None for k, _ in nct.ColorStages._fields_])


def _capture(name, args, stop_code):
    """inside the call: the arguments by role, everything behind an address copied out while it is alive"""
    assert args[0] is None and len(args) == len(ROLES[name]) + 1 == len(nct.SIGNATURES[name][1]), name
    arrays, structs = _live(stop_code)
    got = []
    for role, a in zip(ROLES[name], args[1:]):
        p = _addr(a)
        if role == "int":
            got.append(int(a))
        elif role in ("image", "src", "out"):
            got.append((role, p, "%s %s" % (a.dtype, "x".join(map(str, a.shape)))))
        elif role == "ints":
            got.append(list(a))
        elif role == "ptrs":
            got.append("%d pointers, %d null" % (len(a), sum(1 for x in a if not x)))
        elif p is None:
            got.append(None)
        elif role in PARAM_FIELDS:
            st = getattr(nct, role).from_address(p)
            got.append({role: {k: getattr(st, k) for k in PARAM_FIELDS[role]}})
        elif role == "color":
            ptrs = _pointers((C.c_void_p * 5).from_address(p))
            got.append(("color", [q and _stages(q, structs) for q in ptrs]))
        else:
            st = getattr(nct, role).from_address(p)
            fields = {k: _pointers(getattr(st, k)) for k, _ in st._fields_}
            if role == "PairLevels":
                fields["color"] = [q and _stages(q, structs) for q in fields["color"]]
            got.append((role, fields))
    return name, got, arrays


class _Stub:
    """stands where the library handle does: every entry point records its call and returns 0"""

    def __init__(self, stop_code):
        self.calls, self._stop = [], stop_code

    def __getattr__(self, name):
        if not name.startswith("nct_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append(_capture(name, args, self._stop) if name in ROLES else (name, None, None))
            return 0
        return fn


def _text(a, key):
    return "%s %s" % (a.dtype, "x".join(map(str, a.shape))) + ("" if key in UNINITIALISED else " zero" if not a.any() else " NONZERO")


def _describe_value(v, key):
    if isinstance(v, np.ndarray):
        return _text(v, key)
    if key in ("dims", "adims", "bdims"):
        return json.loads(json.dumps(v))
    if key == "timing":
        return "dict of %d" % len(v)
    assert isinstance(v, list), (key, type(v))
    if v and isinstance(v[0], dict):                              # "color": per level, per entry -> per entry, the levels side by side
        assert all(sorted(d) == sorted(v[0]) for d in v)
        return {k: _describe_value([d[k] for d in v], k) for k in sorted(v[0])}
    if v and isinstance(v[0], list):
        return [_describe_value(row, key) for row in v]
    kinds = {_text(a, key).split(" ", 1)[0] + _text(a, key).partition(" zero")[1] for a in v}
    assert len(kinds) <= 1 and "NONZERO" not in str(kinds), (key, kinds)         # one dtype per list; the shapes side by side
    return "".join(kinds) + ":" + "".join(" " + "x".join(map(str, a.shape)) for a in v)


def _names(keep):
    names = {}

    def walk(v, name):
        if isinstance(v, np.ndarray):
            names[v.ctypes.data] = name
        elif isinstance(v, list):
            for i, x in enumerate(v):
                walk(x, "%s[%d]" % (name, i))
        elif isinstance(v, dict):
            for k, x in v.items():
                walk(x, "%s.%s" % (name, k))
    for k, v in keep.items():
        walk(v, k)
    return names


def _runs(words):
    """"a[0] a[1] a[2] null null" -> "a[0..2] null*2": neighbours that count up, or repeat, written once"""
    out = []
    for w in words:
        m = re.fullmatch(r"(.*)\[(\d+)\]", w)
        if out and m and out[-1][0] == m.group(1) and out[-1][2] + 1 == int(m.group(2)):
            out[-1][2] += 1
        elif out and not m and out[-1][0] == w and out[-1][1] is None:
            out[-1][2] += 1
        else:
            out.append([m.group(1), int(m.group(2)), int(m.group(2))] if m else [w, None, 1])
    return " ".join((w if n == 1 else "%s*%d" % (w, n)) if a is None else "%s[%d]" % (w, a) if a == n else "%s[%d..%d]" % (w, a, n) for w, a, n in out)


def _resolve(p, names, arrays):
    if isinstance(p, list):
        rows = [_resolve(q, names, arrays) for q in p]
        if p and isinstance(p[0], list):                          # [reference][level]: the rows of the references that are not there are all null
            while rows and rows[-1] == "null*5":
                rows.pop()
            return rows
        return _runs(rows)
    if isinstance(p, tuple):                                      # a nct_color_stages
        alive, ptrs = p
        got = [_resolve(q, names, arrays) for q in ptrs]
        level = got[0].split(".")[0]
        same = got == ["%s.%s" % (level, k) for k, _ in nct.ColorStages._fields_]
        return ("" if alive else "DANGLING ") + (level if same else "{%s}" % ",".join(got))
    if p is None:
        return "null"
    return names.get(p) or ("private:" + arrays[p].replace(" ", ":") if p in arrays else "DANGLING")


def _describe_call(call, frame, out, keep):
    name, got, arrays = call
    names = _names(keep or {})
    args = []
    for g in got:
        if isinstance(g, tuple) and g[0] in ("image", "src", "out"):
            role, p, text = g
            args.append("the frame" if frame is not None and p == frame.ctypes.data else "the result" if out is not None and p == out.ctypes.data else text)
        elif isinstance(g, tuple) and g[0] == "color":
            args.append({"color": _runs([_resolve(q, names, arrays) for q in g[1]])})
        elif isinstance(g, tuple):
            args.append({g[0]: {k: (_runs([_resolve(q, names, arrays) for q in v]) if k == "color" else _resolve(v, names, arrays)) for k, v in g[1].items()}})
        else:
            args.append(g)
    return {"fn": name, "args": args}


def _attrs(ctx):
    return {k: json.loads(json.dumps(getattr(ctx, k, "unset"), default=int)) for k in ("_pair_shape", "_multi_shapes")}


def _params(levels):
    prm = nct.Params.default()
    prm.levels = levels
    return prm


def _image(hw):
    return np.zeros(tuple(hw) + (3,), np.uint8)


# ---- the cases: id -> (how the context is prepared, the method, its arguments)
BEGINS = []       # (id, method, K, levels, arguments)
for L in (3, 5):
    t = {"tau": 0.5} if L == 3 else {"sigma": 4.0}
    BEGINS.append(("seq_begin[levels=%d]" % L, "seq_begin", 1, L, dict(t)))
    for fin in (nct.FINISH_EXACT, nct.FINISH_UPSAMPLE):
        BEGINS.append(("seq_begin_fullres[levels=%d,finish=%d]" % (L, fin), "seq_begin_fullres", 1, L, dict(t, max_side=MAX_SIDE, finish=fin)))
    for K in (1, 2):
        t = {"tau": 0.5} if K == 1 else {"sigma": 4.0, "hold": 0.25}
        BEGINS.append(("seq_begin_multi[K=%d,levels=%d]" % (K, L), "seq_begin_multi", K, L, dict(t)))
        for fin in (nct.FINISH_EXACT, nct.FINISH_UPSAMPLE):
            BEGINS.append(("seq_begin_multi_fullres[K=%d,levels=%d,finish=%d]" % (K, L, fin), "seq_begin_multi_fullres", K, L, dict(t, max_side=MAX_SIDE, finish=fin)))

FRAME_CALLS = [("seq_frame_levels", {}), ("seq_frame_levels", {"want_color": False}), ("seq_frame_levels", {"want_levels": True}), ("seq_frame_levels", {"want_levels": False}),
               ("seq_frame_region_levels", {}), ("seq_frame_multi_levels", {}), ("seq_frame_multi_levels", {"want_color": False}), ("seq_frame_ref_region_levels", {}),
               ("seq_frame_propagate_levels", {}), ("seq_frame_propagate_region_levels", {}), ("seq_frame_propagate_ref_region_levels", {})]
CHECKED_FRAME_CALLS = sorted({m for m, _ in FRAME_CALLS} | {"seq_frame", "seq_frame_propagate", "seq_probe", "seq_frame_auto"})


def _call_id(method, kw):
    return "%s(%s)" % (method, ",".join("%s=%s" % kv for kv in sorted(kw.items())))


def _begin(ctx, begin):
    _, method, K, levels, kw = begin
    full = "fullres" in method
    src, refs = (FULL_SRC, FULL_REFS) if full else (SRC, REFS)
    if full:                                                  # the sizes are ones the library accepts
        for hw in [src] + refs[:K]:
            nct.working_size(hw[0], hw[1], MAX_SIDE)
    imgs = [_image(r) for r in refs[:K]]
    getattr(ctx, method)(imgs if "multi" in method else imgs[0], _image(src).shape, params=_params(levels), **kw)
    return src


def _cases():
    cases = {}
    for L in (5, 3):
        for kw in ({}, {"want_color": True}, {"want_color": False}):
            cases["pair_run_levels[levels=%d](%s)" % (L, _call_id("", kw)[1:-1])] = (None, "pair_run_levels", (SRC + (3,), REFS[0] + (3,), L), kw)
        for kw in ({}, {"want_color": False}):
            cases["pair_run_region_levels[levels=%d](%s)" % (L, _call_id("", kw)[1:-1])] = (None, "pair_run_region_levels", (SRC + (3,), REFS[0] + (3,), L), kw)
        for K in (1, 2):
            for m in ("multi_run_levels", "multi_run_ref_region_levels"):
                cases["multi_upload[K=%d]/%s[levels=%d]" % (K, m, L)] = (("multi_upload", K), m, (L,), {})
    for b in BEGINS:
        cases[b[0]] = (b, None, (), {})
        for method, kw in FRAME_CALLS:
            cases[b[0] + "/" + _call_id(method, kw)] = (b, method, (), kw)
    cases["no sequence/seq_frame_propagate_levels()"] = (None, "seq_frame_propagate_levels", (), {})
    return cases


CASES = _cases()


def _run_case(case):
    """-> the description of one case (this function's frame is where the search for live arrays stops)"""
    prep, method, args, kw = case
    ctx = nct.Context.__new__(nct.Context)
    ctx._h, ctx._l = None, _Stub(_run_case.__code__)
    frame = None
    if prep is not None and prep[0] == "multi_upload":
        ctx.multi_upload(_image(SRC), [_image(r) for r in REFS[:prep[1]]])
    elif prep is not None:
        frame = _image(_begin(ctx, prep))
    if method is None:                                            # the begin call itself
        return {"call": _describe_call(ctx._l.calls[-1], None, None, None)}
    if method.startswith("seq_frame"):
        if frame is None:
            frame = _image(SRC)
        out, keep = getattr(ctx, method)(frame, **kw)
    else:
        out, keep = None, getattr(ctx, method)(*args[:-1], params=_params(args[-1]), **kw)
    d = {"dict": {k: _describe_value(v, k) for k, v in sorted(keep.items())}, "call": _describe_call(ctx._l.calls[-1], frame, out, keep), "attrs": _attrs(ctx)}
    if out is not None:
        d["frame"] = _text(out, "ab_up")
    assert [c[0] for c in ctx._l.calls[:-1]] == ([] if prep is None else ["nct_" + prep[0]] if prep[0] == "multi_upload" else ["nct_" + prep[1]])
    return json.loads(json.dumps(d))


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_holds_these_cases_and_no_others():
    assert sorted(_golden()) == sorted(CASES)


def _pytest_cases():
    import pytest
    return pytest.mark.parametrize("cid", sorted(CASES))


@_pytest_cases()
def test_report_is_what_the_table_recorded(cid):
    got, want = _run_case(CASES[cid]), _golden()[cid]
    assert "DANGLING" not in json.dumps(want) and "NONZERO" not in json.dumps(want)
    assert got == want


def _wrong_size_cases():
    import pytest
    return pytest.mark.parametrize("method", CHECKED_FRAME_CALLS)


@_wrong_size_cases()
def test_a_frame_of_the_wrong_size_is_refused(method):
    """every seq_frame* method (and the probe) refuses a frame that is not the size the sequence was begun for, before it touches the library or the context"""
    import pytest
    ctx = nct.Context.__new__(nct.Context)
    ctx._h, ctx._l = None, _Stub(_run_case.__code__)
    ctx.pair_upload(_image((8, 9)), _image((7, 6)))
    ctx.seq_begin(_image(REFS[0]), SRC + (3,), params=_params(3))
    before, calls = _attrs(ctx), len(ctx._l.calls)
    for hw in ((SRC[0] + 1, SRC[1]), (SRC[0], SRC[1] - 1), (SRC[1], SRC[0])):
        with pytest.raises(nct.NctError) as e:
            getattr(ctx, method)(_image(hw))
        assert e.value.code == -2
    assert len(ctx._l.calls) == calls and _attrs(ctx) == before


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_binding_reports.py --record")
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(cid), json.dumps(_run_case(CASES[cid]), separators=(",", ":"))) for cid in sorted(CASES)) + "\n}\n")
    print("%s: %d cases, %d bytes" % (GOLDEN, len(CASES), os.path.getsize(GOLDEN)))
