"""The cases of tests/test_gpu_refract.py, from the reference's counts alone (tests/refract_ref.py), before any kernel is asked: every
branch of vrt_set_water_refraction's contract is taken by at least one case the GPU tests run, at the sizes and settings they run.

    branch                                                           case
    underside event: total reflection and transmission out           pool under_up (one frame has both, on primary segments)
    ... reflected by the draw                                        pool under_up
    walk ended on a solid voxel                                      pool under_bed
    walk crossed a liquid-to-liquid boundary (id 300 a liquid)       two across
    walk ended on that boundary (id 300 a solid)                     solid across
    walk still in liquid after max_span steps                        two across, max_span = 2
    entering transmission bent                                       pool down, pool grazing
    exit into a chunk that chunk_roots holds 0 for                   column column_up (4609 events at 128 x 72, 4 bounces, 1 spp);
                                                                     "pool above" has none — its water ends 20 voxels under the
                                                                     chunks the generator left out — so the column world was added
    event on a path's last allowed segment                           pool under_up at 1 bounce
    a zero normal in A                                               none of these frames (asked of the bends directly:
                                                                     tests/test_refract_ref.py)
"""
import numpy as np
import pytest

import refract_cases as RC
import refract_ref
import segment_cases as SC
import water_cases as K

SIZE = (128, 72)
IOR = RC.IOR


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return refract_ref.load(tmp_path_factory.mktemp("refract_ref"))


def _render(rref, orc, sc, refract=IOR, spp=1, prim=False, **kw):
    plane = np.zeros((sc.size[1], sc.size[0]), np.uint8) if prim else None
    out = rref.render(orc.from_package_scene(sc), *sc.size, water=K.OPTICS, refract=refract, spp=spp, seed=K.SEED, prim=plane, **kw)
    return out + (plane,)


def test_under_up_has_total_reflection_and_transmission_in_one_frame(rref, orc):
    sc = K.pool("under_up", SIZE)
    _, _, n, prim = _render(rref, orc, sc, prim=True)
    print(n, np.bincount(prim.ravel(), minlength=5))
    assert n.under_total >= 1000 and n.under_out >= 1000 and n.under_fresnel >= 100
    assert n.under > n.under_total + n.under_fresnel + n.under_out, "events on a path's last allowed segment: counted, in no branch"
    # on primary segments: the pixel sets of the visible check
    assert (prim == refract_ref.PRIM_TOTAL).sum() >= 1000 and (prim == refract_ref.PRIM_OUT).sum() >= 1000
    # one bounce: every event is on the path's last allowed segment — counted, nothing drawn
    _, _, n1, prim1 = _render(rref, orc, K.pool("under_up", SIZE, bounces=1), prim=True)
    assert n1.under == (prim1 == refract_ref.PRIM_LAST).sum() >= 5000 and n1.under_total == n1.under_out == n1.under_fresnel == 0


def test_under_bed_walks_end_on_a_solid(rref, orc):
    _, _, n, _ = _render(rref, orc, K.pool("under_bed", SIZE))
    print(n)
    assert n.walk_solid >= SIZE[0] * SIZE[1] and n.under >= 1000   # every primary walk ends on the bed; later ones reach the surface


def test_across_crosses_the_liquid_boundary_ends_on_it_and_runs_into_the_cap(rref, orc):
    _, _, liquid, _ = _render(rref, orc, K.two_liquids("across", SIZE))
    _, _, solid, _ = _render(rref, orc, K.two_liquids("across", SIZE, liquid=False))
    _, _, plain, _ = _render(rref, orc, K.pool("across", SIZE))
    _, _, capped, _ = _render(rref, orc, K.two_liquids("across", SIZE), refract=(IOR, 2))
    print(liquid, solid, capped, sep="\n")
    assert liquid.walk_cross >= 1000 and plain.walk_cross == 0 and solid.walk_cross == 0
    assert solid.walk_solid > plain.walk_solid, "walks that end on the block of id 300"
    assert liquid.walk_cap == 0 and capped.walk_cap >= 10000 and capped.under >= 100 and capped.walk_solid >= 100
    # the cap changes the frame, and 64 is what 0 means
    a = _render(rref, orc, K.two_liquids("across", SIZE), refract=(IOR, 64))
    b = _render(rref, orc, K.two_liquids("across", SIZE), refract=(IOR, 0))
    c = _render(rref, orc, K.two_liquids("across", SIZE), refract=(IOR, 2))
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and not np.array_equal(a[0], c[0])


def test_down_and_grazing_bend_entries(rref, orc):
    for cam, at_least in (("down", 5000), ("grazing", 100)):
        _, _, n, _ = _render(rref, orc, K.pool(cam, SIZE))
        print(cam, n)
        assert n.bent >= at_least and n.bent == n.transmitted


def test_the_column_leaves_into_a_chunk_that_does_not_exist_and_above_does_not(rref, orc):
    _, _, above, _ = _render(rref, orc, K.pool("above", SIZE))
    _, _, column, _ = _render(rref, orc, RC.column("column_up", SIZE))
    print(above, column, sep="\n")
    assert above.under >= 1000 and above.under_no_chunk == 0
    assert column.under_no_chunk == 4609 and column.under_total >= 1000 and column.under_out >= 1000
    sc = RC.column("column_up", SIZE)
    roots = np.asarray(sc.world.chunk_roots())
    assert roots.size == 8 and (roots.reshape(2, 2, 2)[:, 1, :] == 0).all() and (roots.reshape(2, 2, 2)[:, 0, :] != 0).all()   # [z][y][x]


@pytest.mark.parametrize("name", ["water", "underwater", "water down"])
def test_c4s_lake_cameras(rref, orc, name):
    _, _, n, prim = _render(rref, orc, K.c4_lake(name, SIZE), prim=True)
    print(name, n)
    assert n.under >= 1000 and n.walk_solid >= 1000 and n.walk_cap >= 1000 and n.under_no_chunk >= 100
    if name == "underwater":
        assert (prim == refract_ref.PRIM_TOTAL).sum() >= 1000 and (prim == refract_ref.PRIM_OUT).sum() >= 1000
    else:
        assert n.bent >= 5000 and not prim.any()


def test_one_over_follows_bent_entries_past_256_workgroups(rref, orc):
    size = SC.CASES["one_over"].size
    assert (size[0] // 8) * (size[1] // 8) > 1024   # more than 256 primary workgroups of four tiles
    sc = K.c4_lake(K.SEGMENT_CASES["one_over"], size)
    _, _, n = rref.render(orc.from_package_scene(sc), *size, water=K.OPTICS, refract=IOR, spp=1, seed=K.SEED, sun=1.0)
    print(n)
    assert n.surface >= 60000 and n.bent >= 50000 and n.under >= 10000
    assert n.wet_bounces >= n.bent, "every bent entry is followed by a wet bounce segment"
