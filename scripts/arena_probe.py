"""Device memory a context's arena holds (NCT_CTR_ARENA_BYTES).
usage: python scripts/arena_probe.py [sizes ...]      the high-water mark per image size after one pair and after two
       python scripts/arena_probe.py seams [file]     seams mode: the same per call of every host-pointer seam (tests/host_seams.py), with every optional argument (pass
                                                      A) and with none (pass B); profiles/host_seams_arena_parent.txt holds the lines of the tree before the seams
                                                      went through one staging helper: pass A equal line for line, pass B equal in every CRC and smaller where a
                                                      placeholder block is gone (profiles/README.md has the figures, and the one place where it is 10 KB larger)
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


def seams(out):
    """every host-pointer seam once in a fixed order on one context, then the whole list again on the blocks the first round gave back; pass A with every optional
    argument present, pass B with every one absent. 480 x 640 images, 120 x 160 level grids (the fp64 coefficient maps: 900 KB), C = 64, K = 2, a lattice of 33: several
    requests of a call exceed 1 MiB, for the reason the `seq` mode states"""
    import host_seams as hs
    s = hs.sizes(120, 160, 480, 640, 64, 33, bh=110, bw=170)
    d = hs.data(s)
    strokes = np.zeros((s.H, s.W), np.uint8)
    strokes[200:260, 200:420] = nct.STROKE_IN; strokes[10:40, 20:600] = nct.STROKE_OUT; strokes[400:470, 420:620] = nct.STROKE_OUT
    half = synth.random_nnf(3, (s.h - 1) // 2 + 1, (s.w - 1) // 2 + 1, (s.bh - 1) // 2 + 1, (s.bw - 1) // 2 + 1)
    labels = (np.arange(30 * 40).reshape(30, 40) % 3).astype(np.int32)
    rng = np.random.default_rng(5)
    cw, cb = (rng.standard_normal((64, 64, 3, 3)) * 0.06).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    sel = nct.region_select_params(tap=2, max_seeds=7)
    lines = []

    def flat(res):
        if isinstance(res, dict):
            return [a for k in sorted(res) for a in flat(res[k])]
        if isinstance(res, (list, tuple)):
            return [a for r in res for a in flat(r)]
        return [] if res is None else [np.ascontiguousarray(res)]

    def note(c, tag, name, res):
        crc = 0
        for a in flat(res):
            crc = zlib.crc32(a.tobytes(), crc)
        lines.append("%-4s %-30s arena %12d  crc %08x" % (tag, name, c.counter(nct.CTR_ARENA_BYTES), crc))
        print(lines[-1], flush=True)

    # the seams without an optional argument (stage reports count as one: `stages`), in the order of the source files
    def plain(c, stages):
        yield "nnf_init", c.nnf_init(s.h, s.w, s.bh, s.bw)
        yield "nnf_upsample", c.nnf_upsample(half, s.h, s.w, s.bh, s.bw)
        yield "patchmatch", c.patchmatch(c.feat_normalize(d.fa), c.feat_normalize(d.fb), c.nnf_init(s.h, s.w, s.bh, s.bw), iters=2, rs_max=4, seed=11)
        yield "bds_vote_image", c.bds_vote_image(d.img, d.img_b, d.ann, d.bnn)
        yield "feature_distance", c.feature_distance(d.fa, synth.features(9, s.C, s.h, s.w))
        yield "seq_warp", c.seq_warp(d.x_prev, d.field)
        yield "seq_matte_warp", c.seq_matte_warp(d.mask_full, d.field)
        yield "region_snap", c.region_snap(d.mask_full, c.bgr2lab(d.full))
        yield "bgr2lab", c.bgr2lab(d.full)
        yield "lab2bgr_form", c.lab2bgr(d.full, form=nct.LAB2BGR_CUBE)
        yield "resize_u8c3", c.resize_u8c3(d.full, s.h, s.w)
        yield "resize_u8c1", c.resize_u8c1(d.score, s.H, s.W)
        yield "resize_f64c3", c.resize_f64c3(d.ab[0].reshape(s.h, s.w, 3), s.H, s.W)
        yield "region_mix", c.region_mix(d.x, d.score)
        yield "region_compose", c.region_compose(d.full, d.res, d.mask_full)
        yield "region_pull", c.region_pull(np.ascontiguousarray(d.img_b[:, :, 0]), d.ann, d.bnn)
        yield "cluster_features", c.cluster_features(d.fa, 10, 3, 1)
        ids, kw = c.knn_graph(d.lab, labels, 3, 4)
        yield "knn_graph", (ids, kw)
        yield "local_color_transfer", c.local_color_transfer(d.errs[0], d.img, d.guides[0], d.full, ids, kw, 3, want_stages=stages)
        yield "color_finish", c.color_finish(d.ab, s.h, s.w, s.H, s.W, d.full, want_stages=stages)
        yield "color_finish_upsample", c.color_finish_upsample(d.ab, s.h, s.w, d.full)
        yield "color_finish_guided", c.color_finish_guided(d.ab, d.lab, s.h, s.w, d.full, sigma=10.0)
        yield "lut_apply", c.lut_apply(np.random.default_rng(6).random((s.N, s.N, s.N, 3), dtype=np.float32) * 255, d.full)
        yield "region_select", c.region_select(d.full, strokes, sel, want_stages=stages)
        yield "feat_quantize", c.feat_quantize(d.fa)
        model = c.region_model_fit(d.full, strokes, sel)
        yield "region_model_fit", model.rows()
        yield "region_model_apply", c.region_model_apply(model, d.full, None if not stages else d.mask_full, want_stages=stages)
        yield "vgg19_features", c.vgg19_features(d.full, 5 if stages else 2)
        yield "conv3x3_relu", c.conv3x3_relu(d.fa, cw, cb)
        yield "maxpool2x2", c.maxpool2x2(d.fa)
        model.close()

    for pas, everything in (("A", True), ("B", False)):
        with nct.Context(0) as c:
            c.vgg19_load_raw(ws, bs)
            for tag in (pas + "/1", pas + "/2"):                      # twice on one context: the second round runs on the blocks the first gave back
                for name, opts, call in hs.NULLABLE:
                    note(c, tag, name, call(c, d, () if everything else opts))
                for name, res in plain(c, everything):
                    note(c, tag, name, res)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if sys.argv[1:2] == ["seq"]:
    sequences(sys.argv[2] if len(sys.argv) > 2 else None)
elif sys.argv[1:2] == ["seams"]:
    seams(sys.argv[2] if len(sys.argv) > 2 else None)
else:
    pairs([int(a) for a in sys.argv[1:]])
