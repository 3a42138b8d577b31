"""The lit pass that tests whole ray corridors (vrt_lit.hip: accel_lit_kernel; docs/NUMERICS.md "Lit stops") on the GPU.

The marks of vrt_get_sun_marks against the rule as tests/lit_corridor_ref.py states it, over the grid the device built
(vrt_read_accel): whatever the kernel lights, the rule evaluated in float64 without any margin must light too, and whatever the
same build lights at slab depth 1 (VRT_LIT_SLAB=1: the reach of a sweep layer by layer) must stay lit.  The frames drawn with
those marks against the oracle, one and two in flight, and the counting kernel's step counts.  The trips of a frame's tiles: none
dearer than at depth 1, and fewer in all.

Grids: 16^3 and 32^3 cells (one launch: the whole corridor), 24^3 cells with a slab depth of 5 (four full slabs and a short one:
the hand-over between slabs), 80^3 cells (above 64 a side: the default there is slabs of 32, so two full slabs and one of 16).  The 2^3-chunk world lies under
water — no cell of it is an air leaf, and nothing may be lit there."""
import numpy as np
import pytest

import lit_corridor_ref as R
from test_gpu_sun_marks import SETTLE, render_and_check, suns
from util import gpu_for_scene
from voxelraytracing_amd import MODE_PRIMARY_SHADOW, scenes

pytestmark = pytest.mark.gpu

SIZE = (64, 40)
SUNS = ("+y", "-x", "close over the world", "below the horizon")
# (chunks a side, VRT_LIT_SLAB or None for the default, the depth that gives)
GRIDS = [(2, None, 16), (4, None, 32), (3, "5", 5), (10, None, 32)]


def _scene(chunks):
    sc = scenes.procedural(chunks, SIZE)
    if chunks == 2:   # (an eye inside the world: just under its top face, in the water)
        sc = scenes._scene(sc.name, sc.world, SIZE, (32.5, 62.5, 32.5), sc.rot, MODE_PRIMARY_SHADOW)
    return sc


def _gpu(monkeypatch, sc, slab):
    if slab is None:
        monkeypatch.delenv("VRT_LIT_SLAB", raising=False)
    else:
        monkeypatch.setenv("VRT_LIT_SLAB", slab)
    return gpu_for_scene(sc)


@pytest.mark.parametrize("chunks,slab,depth", GRIDS)
def test_marks_and_frames(orc, monkeypatch, chunks, slab, depth):
    sc = _scene(chunks)
    G = chunks * 8
    layer_by_layer = _gpu(monkeypatch, sc, "1")
    gpu = _gpu(monkeypatch, sc, slab)
    try:
        layer_by_layer.set_frames_in_flight(1)
        lo = None
        for name, sun, marks in suns(chunks * 32):
            if name not in SUNS:
                continue
            assert marks
            sc.settings.sun_pos[:] = sun
            o = orc.from_package_scene(sc)
            for g in (gpu, layer_by_layer):
                g.write_settings(sc.settings)
            for in_flight in (1, 2):
                gpu.set_frames_in_flight(in_flight)
                render_and_check(orc, gpu, sc, f"{chunks}^3 slab {slab} sun {name}, {in_flight} in flight", oracle=o, stats=True)
            for _ in range(SETTLE):
                layer_by_layer.render(MODE_PRIMARY_SHADOW, timed=True)
            if lo is None:   # (the tables exist once a frame has been drawn; the suns do not change them)
                grid, _ = gpu.read_accel()
                lo = np.where(grid >= 0xFF800000, (grid & 31).astype(np.int32), -1)
            m, m1 = gpu.sun_marks(cells=True), layer_by_layer.sun_marks(cells=True)
            assert m["min_leaf"] == 4 and m1["min_leaf"] == 4, (name, m["min_leaf"], m1["min_leaf"])
            lit, lit1 = m["lit"].astype(bool), m1["lit"].astype(bool)
            free = R.lit(lo, sun, depth, margins=False).astype(bool)
            ref = R.lit(lo, sun, depth).astype(bool)
            print(f"{chunks}^3 slab {slab} sun {name}: air cells {int((lo >= 0).sum())}, lit {int(lit.sum())}, at depth 1 {int(lit1.sum())}, "
                  f"the rule without margins {int(free.sum())}, with them {int(ref.sum())} ({int((ref != lit).sum())} cells differ)")
            assert not (lit & ~free).any(), f"{name}: {int((lit & ~free).sum())} lit cells the rule does not allow"
            assert not (lit1 & ~lit).any(), f"{name}: {int((lit1 & ~lit).sum())} cells lit at depth 1 and not now"
            assert not (lit1 & ~R.lit(lo, sun, 1, margins=False).astype(bool)).any(), name
            if chunks > 2 and name != "below the horizon":
                assert lit.sum() > lit1.sum(), (name, "the corridor lights nothing more than the sweep layer by layer")
            else:
                assert chunks > 2 or not lit.any()
    finally:
        gpu.close()
        layer_by_layer.close()


def test_no_tile_takes_more_trips_and_the_frame_takes_fewer(orc, monkeypatch):
    """vrt_read_tile_cost at 128 x 72 on the 4^3 world, as tests/test_gpu_sun_marks.py reads it: the marks are made while another
    view is drawn, then the second plain frame of the view at rest notes its tiles' trips."""
    sc = scenes.procedural(4, (128, 72))
    other = scenes._scene("another view", sc.world, sc.size, sc.eye, (35.0, 120.0, 0.0), MODE_PRIMARY_SHADOW)
    w, h = sc.size
    _, r_ids, r_steps, _ = orc.from_package_scene(sc).render(MODE_PRIMARY_SHADOW, w, h, want_steps=True)
    tiles = (h // 8) * (w // 8)
    cost = {}
    for slab in ("1", None):
        gpu = _gpu(monkeypatch, sc, slab)
        try:
            gpu.set_frames_in_flight(1)
            gpu.write_cam_data(other.cam)
            for _ in range(SETTLE):
                gpu.render(MODE_PRIMARY_SHADOW, timed=True)
            gpu.write_cam_data(sc.cam)
            for _ in range(3):
                gpu.render(MODE_PRIMARY_SHADOW, timed=True)
            _, ids, _ = gpu.read_output()
            assert np.array_equal(ids, r_ids)
            assert gpu.sun_marks()["passes"] == 1
            cost[slab] = gpu.read_tile_cost(tiles).astype(np.int64)
            gpu.render(MODE_PRIMARY_SHADOW, stats=True)
            assert np.array_equal(gpu.read_steps(), r_steps)
        finally:
            gpu.close()
    print("trips per frame: at depth 1", int(cost["1"].sum()), "whole corridor", int(cost[None].sum()))
    assert (cost[None] <= cost["1"]).all()
    assert cost[None].sum() < cost["1"].sum()
