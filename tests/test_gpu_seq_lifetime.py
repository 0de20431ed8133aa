"""Every arena block an open sequence holds has one owner, and every one goes back (nct_pipeline.h: seq_state, pair_state).

One round opens and ends four sequences in turn on one context, through every path that gives blocks back: settings removed one by one, nct_seq_end on a
full-resolution sequence with both masks, a region model replaced and removed, nct_seq_begin on a context whose sequence is still open.
- A block that is lost stays reserved, so the next round has to take a fresh one from the device: NCT_CTR_ARENA_BYTES grows from round to round. Round 1 fills the
  arena's cache; round 3 must hold what round 2 held and return its bytes.
- A block that is given back twice is handed to a second owner while the first still uses it; with NCT_ARENA_FILL the second owner's block is filled as it is handed
  out, which overwrites what the first one kept. The filled rounds must return the clean rounds' bytes.
The results themselves are pinned to the float64 and oracle compositions by the other sequence tests; no reference is computed here."""
import numpy as np
import pytest

import nct
import region_select_ref as sel
import seq_ref
import synth
from test_gpu_arena_fill import HOOKS

pytestmark = pytest.mark.gpu

H, W = 56, 64
REF = (2000, 48, 60)
ROUNDS = 3
_CLEAN = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_results():
    yield
    _CLEAN.clear()


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


def _rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


def one_round(c):
    """the four sequences -> everything they returned, in order"""
    prm = nct.Params.default(); prm.levels = 2
    ref, ref2 = synth.image(*REF), synth.image(2001, 50, 58)
    frames = seq_ref.pan_frames(3, H, W, step=2)
    big = seq_ref.pan_frames(3, 2 * H, 2 * W, step=4)
    out = []

    def run(fr, kinds):
        for f, k in zip(fr, kinds):
            out.append(c.seq_frame_propagate(f) if k == "P" else c.seq_frame(f))

    # 1: two references, motion, a tracked and snapped source matte, a mask on reference 0 — each setting removed again before the end
    c.seq_begin_multi([ref, ref2], frames[0].shape, prm)
    c.seq_set_motion()
    c.seq_set_region(_rect(H, W, 14, 42, 8, 40), protect=1)
    c.seq_set_region_tracking(True)
    c.seq_set_region_snap(True)
    c.seq_set_ref_region(0, _rect(REF[1], REF[2], 8, 40, 6, 50))
    run(frames, "FBP")
    out.append(c.seq_get_region()[0])
    c.seq_set_ref_region(0, None)
    c.seq_set_region(None)
    c.seq_set_motion(off=True)
    c.seq_end()
    # 2: a full-resolution sequence with the upsampling finish and both masks; the table is fitted under the kept target mask
    c.seq_begin_fullres(ref, big[0].shape, max_side=W, finish=nct.FINISH_UPSAMPLE, params=prm)
    c.seq_set_region(_rect(2 * H, 2 * W, 28, 84, 16, 80), protect=1)
    c.seq_set_ref_region(0, _rect(REF[1], REF[2], 8, 40, 6, 50))
    run(big, "FBP")
    out.append(c.pair_fit_lut(size=9))
    c.seq_end()
    # 3: a region model, replaced and then removed
    T = sel.call_strokes(H, W)
    model = c.region_model_fit(frames[0], T, nct.region_select_params(tap=2, max_seeds=7))
    other = c.region_model_fit(frames[0], T, nct.region_select_params(tap=3, max_seeds=3))
    c.seq_begin(ref, frames[0].shape, prm)
    c.seq_set_motion()
    c.seq_set_region_tracking(True)
    c.seq_set_region_model(model, nct.region_refind_params(snap_iters=1))
    run(frames, "FB")
    out.append(c.seq_get_region()[0])
    c.seq_set_region_model(other)
    c.seq_set_region_model(None)
    c.seq_end()
    model.close(); other.close()
    # 4: nct_seq_begin on a context whose sequence is still open
    c.seq_begin(ref, frames[0].shape, prm)
    c.seq_set_motion()
    c.seq_set_region(_rect(H, W, 14, 42, 8, 40))
    run(frames, "FP")
    c.seq_begin_multi([ref2, ref], frames[0].shape, prm)
    run(frames, "FB")
    c.seq_end()
    return out


def rounds(monkeypatch, weights, fill=None):
    """ROUNDS rounds on one fresh context -> [(outputs, NCT_CTR_ARENA_BYTES behind the round)]"""
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    if fill is not None:
        monkeypatch.setenv("NCT_ARENA_FILL", str(fill))
    with nct.Context(0) as c:
        c.vgg19_load_raw(*weights)
        got = []
        for _ in range(ROUNDS):
            out = one_round(c)
            got.append((out, c.counter(nct.CTR_ARENA_BYTES)))
    return got


def clean_rounds(monkeypatch, weights):
    if "clean" not in _CLEAN:
        _CLEAN["clean"] = rounds(monkeypatch, weights)
    return _CLEAN["clean"]


def _unequal(a, b):
    assert len(a) == len(b)
    return [i for i, (x, y) in enumerate(zip(a, b)) if x.shape != y.shape or x.tobytes() != y.tobytes()]


def test_no_block_is_lost(monkeypatch, weights):
    got = clean_rounds(monkeypatch, weights)
    bytes_held = [b for _, b in got]
    print("NCT_CTR_ARENA_BYTES behind each round:", bytes_held)
    assert bytes_held[0] > 0
    assert bytes_held[2] == bytes_held[1], "the arena grew between rounds 2 and 3: a block stayed reserved %s" % bytes_held
    assert not _unequal(got[1][0], got[2][0]), "round 3 differs from round 2 in outputs %s" % _unequal(got[1][0], got[2][0])
    assert len(got[0][0]) == 15 and not any(np.array_equal(got[0][0][0], o) for o in got[0][0][1:3])       # the frames of a sequence differ


def test_no_block_has_two_owners(monkeypatch, weights):
    clean = clean_rounds(monkeypatch, weights)
    filled = rounds(monkeypatch, weights, fill=0xA5)
    for r in range(ROUNDS):
        bad = _unequal(clean[r][0], filled[r][0])
        assert not bad, "NCT_ARENA_FILL=0xA5 changes outputs %s of round %d" % (bad, r + 1)
    assert [b for _, b in filled] == [b for _, b in clean]
