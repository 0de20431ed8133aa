"""What every entry point refuses in nct_params (include/nct.h at nct_params): eps, nonlocal_weight, local_weight, wls_lambda_init and wls_alpha must each be finite and
> 0, bds_weight finite and >= 0. One table of bad values, each field in turn, through nct_process_pair, nct_seq_begin, nct_local_color_transfer and nct_color_finish:
NCT_ERR_INVALID with a message that names the entry point and the field, no sequence left open, nothing reserved by the two seams (their check stands in front of their
buffers) — and the same call with the defaults succeeds right after each refusal."""
import numpy as np
import pytest

import nct
import synth

POSITIVE = ("eps", "nonlocal_weight", "local_weight", "wls_lambda_init", "wls_alpha")
BAD = [(f, v) for f in POSITIVE + ("bds_weight",) for v in (float("nan"), float("inf"), -1.0)] + [(f, 0.0) for f in POSITIVE]


def _prm(field=None, value=None, levels=1):
    p = nct.Params.default()
    p.levels = levels
    if field:
        setattr(p, field, value)
    return p


@pytest.mark.gpu
def test_params_outside_the_solvers_domain_are_refused():
    from caffemodel_io import synthetic_vgg19
    from fullres_ref import smooth_ab
    src, ref = synth.image(1, 20, 24), synth.image(2, 24, 20)
    h, w = 12, 14                                  # S2's hierarchy needs a second level: more than 64 points
    err = -np.random.default_rng(3).random((h, w)).astype(np.float32)
    lvl, guide = synth.image(4, h, w), synth.image(5, h, w)
    ab = smooth_ab(8, h, w)
    with nct.Context(0) as c:
        c.vgg19_load_raw(*synthetic_vgg19(19))
        ids, kw = c.knn_graph(c.bgr2lab(lvl), np.zeros((3, 4), np.int32), 1, 4)

        def seq_begin(p):
            c.seq_begin(ref, src.shape, p)
            c.seq_end()

        calls = {"process": lambda p: c.process_pair(src, ref, p), "seq_begin": seq_begin,
                 "local_color_transfer": lambda p: c.local_color_transfer(err, lvl, guide, lvl, ids, kw, 4, params=p),
                 "color_finish": lambda p: c.color_finish(ab, h, w, h, w, lvl, p)}
        for call in calls.values():                                  # the arena holds every block a valid call takes
            call(_prm())
        assert len(BAD) == 6 * 3 + 5
        for field, value in BAD:
            for who, call in calls.items():
                held = c.counter(nct.CTR_ARENA_BYTES)
                with pytest.raises(nct.NctError) as e:
                    call(_prm(field, value))
                bound = ">= 0" if field == "bds_weight" else "> 0"
                assert e.value.code == -2 and f"{who}: {field} must be finite and {bound}" in str(e.value), (who, field, value, str(e.value))
                if who != "process":                                 # nct_process_pair uploads its images before the run is checked
                    assert c.counter(nct.CTR_ARENA_BYTES) == held, (who, field, value)
                call(_prm())
        # the rule is one: a field the entry point itself never reads is refused there too, and bds_weight 0 is a value
        c.process_pair(src, ref, _prm("bds_weight", 0.0))
