"""S2's batch schedule on the GPU: NCT_WLS_TRACE=1 prints, per (half-)solve, the iterations enqueued, the iterations needed and the snapshots read. The schedule is a function of
the published solver states in publication order, not of timing, so these triples repeat; they are pinned to what the solver gave before its host code was split up
(two runs of this file against that build agreed: profiles/wls_host_refactor_ab.md). Results and wls_iters do not depend on the schedule — without this test a forecast that is
switched off costs speed and fails nothing."""
import re

import pytest

from test_gpu_color import _level_case

# _level_case shapes of test_gpu_color.py (S2 runs on the full H x W grid), the smallest that reach each form of the cycle
SMALL = (40, 56, 20, 28, (5, 7), 4, 3)                  # 2 240 pixels: 16x8 tiles, deep fused middle
MEDIUM = (100, 141, 100, 141, (5, 7), 8, 1)             # 14 100 pixels
LARGE = (372, 368, 372, 368, (23, 23), 16, 4)           # 136 896 pixels: the first size with 32x16 / 32x14 tiles
# (shape, variant) -> sorted (enqueued, needed, snapshots) of every `nct wls:` line of the call.
# "latency": nct_local_color_transfer with NCT_FLAG_LATENCY — that entry does not read the flag, so the solve is the 6-wide one and prints one line.
# "split": the same S2 solve through nct_color_finish, which does: two lines, one per 3-wide half (helper thread and caller).
PARENT = {
    (SMALL, "default"): [(11, 10, 7)], (MEDIUM, "default"): [(12, 11, 7)], (LARGE, "default"): [(14, 13, 8)],
    (SMALL, "noforecast"): [(14, 10, 7)], (MEDIUM, "noforecast"): [(14, 11, 7)],
    (SMALL, "nolines"): [(16, 15, 10)], (MEDIUM, "nolines"): [(17, 16, 10)],
    (SMALL, "latency"): [(11, 10, 7)], (MEDIUM, "latency"): [(12, 11, 7)],
    (SMALL, "split"): [(11, 10, 7), (11, 10, 7)], (MEDIUM, "split"): [(11, 10, 7), (12, 11, 7)], (LARGE, "split"): [(13, 11, 7), (14, 13, 8)],
}
CASES = ([(s, "default") for s in (SMALL, MEDIUM, LARGE)] + [(s, v) for v in ("noforecast", "nolines", "latency") for s in (SMALL, MEDIUM)]
         + [(s, "split") for s in (SMALL, MEDIUM, LARGE)])
LINE = re.compile(r"nct wls: \d+ x \d+, (\d+) iterations enqueued, (\d+) needed \(\+1 that finds every system converged\), (\d+) snapshots read")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,variant", CASES, ids=[f"{s[0]}x{s[1]}-{v}" for s, v in CASES])
def test_wls_schedule_triples(oracle, monkeypatch, capfd, shape, variant):
    import nct
    H, W, h, w, grid, samples, layer = shape
    err, s_lvl, g_lvl, s_full, ids, ws = _level_case(30 + layer, H, W, h, w, grid, samples, oracle)
    monkeypatch.setenv("NCT_WLS_TRACE", "1")
    if variant == "noforecast": monkeypatch.setenv("NCT_WLS_FORECAST", "0")
    if variant == "nolines": monkeypatch.setenv("NCT_S2_LINES", "0")
    prm = nct.Params.default()
    if variant in ("latency", "split"): prm.flags = nct.FLAG_LATENCY
    with nct.Context(0) as c:
        capfd.readouterr()
        _, stages = c.local_color_transfer(err, s_lvl, g_lvl, s_full, ids, ws, layer, params=prm, want_stages=True)
        if variant == "split":
            capfd.readouterr()
            _, stages = c.color_finish(stages["ab_nonlocal"], h, w, H, W, s_full, params=prm, want_stages=True)
        triples = sorted(tuple(int(x) for x in m.groups()) for m in LINE.finditer(capfd.readouterr().err))
    iters = stages["wls_iters"].tolist()
    print("wls schedule", (shape, variant), triples, "wls_iters", iters)
    halves = [iters[:3], iters[3:]] if variant == "split" else [iters]
    assert sorted(t[1] for t in triples) == sorted(max(half) for half in halves)           # needed == max(wls_iters), per line
    assert all(enqueued > needed for enqueued, needed, _ in triples)
    assert triples == PARENT[(shape, variant)]
