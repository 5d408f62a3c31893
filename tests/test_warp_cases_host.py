"""CPU: the rigs and forged window tables of tests/warp_cases.py are well-formed and reach what
they were forged for, judged on the oracle's inverse maps (tests/test_gpu_warp_windows.py runs
them through pano_warp_windows)."""
import numpy as np
import pytest

import warp_cases as wc


@pytest.fixture(scope="module", params=wc.RIGS)
def rig(request, oracle):
    from pano360_amd import engine
    r = wc.rig(request.param)
    plan, oplan = wc.make_plan(engine.Plan, r), wc.make_plan(oracle.Plan, r)
    shapes = [im.shape[:2] for im in r["imgs"]]
    maps = [oracle.inverse_map(oplan.projs[i], oplan, oplan.rects[i], shapes[i])
            for i in range(len(shapes))]
    return request.param, r, plan, oplan, shapes, maps


def test_rig_geometry(rig):
    name, r, plan, oplan, shapes, maps = rig
    assert plan.shape == oplan.shape and list(plan.rects) == list(oplan.rects)
    assert np.array_equal(plan.sin_t, oplan.sin_t) and np.array_equal(plan.cos_t, oplan.cos_t)
    assert np.array_equal(plan.tan_p, oplan.tan_p)
    H, W = plan.shape
    assert 64 < W <= 400 and H <= 400                      # a few hundred columns at the most
    for y0, y1, x0, x1 in plan.rects:
        assert 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W
    if name == "mixed":
        assert sorted(shapes) == sorted([(48, 64), (1, 1), (1, 9), (7, 1), (2, 2), (33, 130)])
    if name == "behind":
        assert all(rect == (0, H, 0, W) for rect in plan.rects)
        assert sum(int((np.abs(mx) > 40000).sum()) for mx, _, _ in maps) > 0    # behind the camera
    # every rig masks pixels and leaves pixels unmasked
    assert any(mk.any() for _, _, mk in maps) and any((~mk).any() for _, _, mk in maps)


def test_windows_obey_the_rules_and_reach_both_tap_paths(rig):
    name, r, plan, _, shapes, maps = rig
    rec, floats = wc.windows(plan.rects, plan.centres, 7)
    assert len(rec) == 4 * len(shapes)
    at = wc.GUARD_FLOATS
    corners = set()
    for q in rec:
        i = int(q["index"])
        y0, y1, x0, x1 = plan.rects[i]
        h, w = y1 - y0, x1 - x0
        vy0, vx0, vh, vw = (int(q[k]) for k in ("vy0", "vx0", "vh", "vw"))
        ay0, ax0, ah, aw = (int(q[k]) for k in ("ay0", "ax0", "ah", "aw"))
        assert (int(q["y0"]), int(q["x0"]), int(q["h"]), int(q["w"])) == (y0, x0, h, w)
        assert 0 <= vy0 and 0 <= vx0 and vh > 0 and vw > 0 and vy0 + vh <= h and vx0 + vw <= w
        assert vx0 % 4 == 0 and ((vx0 + vw) % 4 == 0 or vx0 + vw == w)
        assert q["vpitch"] % 4 == 0 and q["vpitch"] >= vw
        assert vy0 <= ay0 and vx0 <= ax0 and ah > 0 and aw > 0
        assert ay0 + ah <= vy0 + vh and ax0 + aw <= vx0 + vw
        assert int(q["planes"]) == at                       # blocks in table order, guards between
        at += 3 * vh * int(q["vpitch"]) + wc.GUARD_FLOATS
        if (vh, vw) != (h, w):
            corners |= {(cy, cx) for cy in (0, 1) for cx in (0, 1)
                        if vy0 + vh * cy == h * cy and vx0 + vw * cx == w * cx}
    assert at == floats
    assert corners == {(0, 0), (0, 1), (1, 0), (1, 1)}      # a window on each corner of a patch
    order = rec["index"].tolist()
    assert order != sorted(order)                           # shuffled table order
    whole, mixed = wc.windows_by_taps(rec, [(mx, my) for mx, my, _ in maps], shapes)
    assert whole >= 1 and mixed >= 1, (name, whole, mixed)
