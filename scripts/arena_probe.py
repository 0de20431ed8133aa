"""Device memory a context's arena holds (NCT_CTR_ARENA_BYTES).
usage: python scripts/arena_probe.py [sizes ...]      the high-water mark per image size after one pair and after two
       python scripts/arena_probe.py seq [file]       sequence mode: one line per call of a fixed list of sequence scenarios — the arena's bytes and a CRC32 of what the
                                                      call returned. The arena serves a request from any free block of up to twice its size plus 1 MiB, so small frames
                                                      hide a changed order of requests; these frames are large enough that several requests exceed 1 MiB. Two trees that
                                                      request the same blocks in the same order print the same lines (and, with `file`, write them there): diff them."""
import sys
import zlib
sys.path.insert(0, "tests"); sys.path.insert(0, "neural-color-transfer_amd/python")
import numpy as np
import nct, synth
from caffemodel_io import synthetic_vgg19
ws, bs = synthetic_vgg19(19)


def pairs(sizes):
    for S in sizes or [256, 700, 1000]:
        with nct.Context(0) as c:
            c.vgg19_load_raw(ws, bs)
            c.pair_upload(synth.image(1000, S, S), synth.image(1001, S, S))
            c.pair_run(nct.Params.default())
            b1 = c.counter(nct.CTR_ARENA_BYTES)
            c.pair_run(nct.Params.default())
            print(f"{S}x{S}: arena {b1 / 1e9:.3f} GB after one pair, {c.counter(nct.CTR_ARENA_BYTES) / 1e9:.3f} GB after two = {b1 / (S * S):.0f} B per pixel", flush=True)


def rect(h, w, y0, y1, x0, x1, inside=255, outside=0):
    m = np.full((h, w), outside, np.uint8)
    m[y0 * h // 100:y1 * h // 100, x0 * w // 100:x1 * w // 100] = inside
    return m


def sequences(out):
    import seq_ref
    H, W, RH, RW, KINDS = 480, 640, 420, 560, "FBPB"                  # F: a first frame, B: a blended full frame, P: a propagated frame
    frames = seq_ref.pan_frames(4, H, W, step=2)
    refs = [synth.image(1001, RH, RW), synth.image(1002, 400, 600)]
    big = seq_ref.pan_frames(4, 960, 1280, step=4)
    big_ref = synth.image(1003, 900, 1200)
    strokes = np.zeros((H, W), np.uint8)
    strokes[200:260, 200:420] = nct.STROKE_IN; strokes[10:40, 20:600] = nct.STROKE_OUT; strokes[400:470, 420:620] = nct.STROKE_OUT
    lines = []

    def note(c, name, what, res=None):
        crc = "-" if res is None else "%08x" % zlib.crc32(np.ascontiguousarray(res).tobytes())
        lines.append("%-16s %-28s arena %12d  crc %s" % (name, what, c.counter(nct.CTR_ARENA_BYTES), crc))
        print(lines[-1], flush=True)

    def run_frames(c, name, fr):
        for t, k in enumerate(KINDS):
            note(c, name, "frame %d %s" % (t, k), c.seq_frame_propagate(fr[t]) if k == "P" else c.seq_frame(fr[t]))

    def plain(c, name):
        c.seq_begin(refs[0], frames[0].shape); note(c, name, "seq_begin")

    def motion(c, name):
        plain(c, name)
        c.seq_set_motion(); note(c, name, "seq_set_motion")

    def two_refs(c, name):
        c.seq_begin_multi(refs, frames[0].shape, hold=0.01); note(c, name, "seq_begin_multi")
        c.seq_set_motion(); note(c, name, "seq_set_motion")

    def matte(c, name):
        motion(c, name)
        c.seq_set_region(rect(H, W, 30, 70, 25, 75), protect=1); note(c, name, "seq_set_region")
        c.seq_set_region_tracking(True); c.seq_set_region_snap(True); note(c, name, "tracking and snap")

    def ref_mask(c, name):
        motion(c, name)
        c.seq_set_ref_region(0, rect(RH, RW, 20, 80, 10, 60)); note(c, name, "seq_set_ref_region")

    def both(c, name):
        matte(c, name)
        c.seq_set_ref_region(0, rect(RH, RW, 20, 80, 10, 60)); note(c, name, "seq_set_ref_region")

    def model(c, name):
        motion(c, name)
        m = c.region_model_fit(frames[0], strokes, nct.region_select_params(tap=2, max_seeds=7)); note(c, name, "region_model_fit")
        c.seq_set_region_tracking(True)
        c.seq_set_region_model(m, nct.region_refind_params(snap_iters=2)); note(c, name, "seq_set_region_model")     # the rows are on the device: the model may go
        m.close()

    def fullres(c, name):
        c.seq_begin_fullres(big_ref, big[0].shape, max_side=640, finish=nct.FINISH_UPSAMPLE); note(c, name, "seq_begin_fullres")
        c.seq_set_motion(); note(c, name, "seq_set_motion")
        c.seq_set_region(rect(960, 1280, 30, 70, 25, 75), protect=1); note(c, name, "seq_set_region")
        c.seq_set_region_tracking(True); c.seq_set_region_snap(True)
        c.seq_set_ref_region(0, rect(900, 1200, 20, 80, 10, 60)); note(c, name, "seq_set_ref_region")

    for name, setup, fr in (("plain", plain, frames), ("motion", motion, frames), ("two_refs_hold", two_refs, frames), ("matte_track_snap", matte, frames),
                            ("ref_mask", ref_mask, frames), ("both_masks", both, frames), ("region_model", model, frames), ("fullres_up_both", fullres, big)):
        with nct.Context(0) as c:
            c.vgg19_load_raw(ws, bs)
            for rep in (1, 2):                                        # twice on one context: the second pass runs on the blocks the first gave back
                setup(c, "%s/%d" % (name, rep))
                run_frames(c, "%s/%d" % (name, rep), fr)
                if fr is big:
                    note(c, "%s/%d" % (name, rep), "pair_fit_lut", c.pair_fit_lut(size=9))
                c.seq_end(); note(c, "%s/%d" % (name, rep), "seq_end")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if sys.argv[1:2] == ["seq"]:
    sequences(sys.argv[2] if len(sys.argv) > 2 else None)
else:
    pairs([int(a) for a in sys.argv[1:]])
