"""tests/segment_cases.py without a GPU: segment_loads against hand-made planes, and — from the reference alone — that every case
reaches the code tests/test_gpu_path_segments.py is there for: segments with a second, third and fourth producer, path, sun and
lamp records beyond a segment's first 256 and 512, chains whose pool workgroups with part = 1 have work, and radiance below the
bound under which util.assert_frame_parity's 1e-4 is above an ulp.  A case that stops reaching the code fails here, not there."""
import numpy as np
import pytest

import lamp_ref
import segment_cases as SC

PATH, SUN, LAMP = lamp_ref.LOAD_PATH, lamp_ref.LOAD_SUN, lamp_ref.LOAD_LAMP


@pytest.fixture(scope="module")
def refs(tmp_path_factory, orc):
    return SC.References(lamp_ref.load(tmp_path_factory.mktemp("lamp_ref")), orc)


def _loads(frame, case, bit, sample=0, segment=0, rank=None):
    """Per segment: the records of `bit` that trace launch `segment` of `sample` appends (rank: of that shard's context)."""
    c = SC.CASES[case]
    tiles = None if rank is None else SC.shard_tiles(*c.size, rank, c.shards)
    return SC.segment_loads((frame.load[sample, segment] & bit) != 0, *c.size, tiles)


# ---- segment_loads ----

def test_segment_loads_of_hand_made_planes():
    w, h = 328, 200   # 41 x 25 tiles
    ones = np.ones((h, w), np.uint8)
    got = SC.segment_loads(ones, w, h)
    assert got.shape == (256,) and got.sum() == 1025 * 64
    assert got[0] == 256 + 64 and (got[1:] == 256).all()   # workgroup 256 is tile 1024 alone
    # one pixel of tile (row 3, column 7) = tile 130 = workgroup 32; one of tile 1024; one of the frame's last column of tile 40
    p = np.zeros((h, w), np.uint8)
    p[3 * 8 + 5, 7 * 8 + 2] = 1
    p[24 * 8, 40 * 8] = 1
    p[7, 327] = 1
    got = SC.segment_loads(p, w, h)
    assert got[32] == 1 and got[0] == 1 and got[10] == 1 and got.sum() == 3
    # a frame that is not whole tiles: the border is nobody's
    ragged = np.ones((204, 332), np.uint8)
    assert np.array_equal(SC.segment_loads(ragged, 332, 204), SC.segment_loads(ones, w, h))
    # counts, not flags: three samples' records
    assert np.array_equal(SC.segment_loads(ones * 3, w, h), 3 * SC.segment_loads(ones, w, h))
    # a shard's tiles: its t-th tile is tiles[t]; workgroup k of ITS launch feeds segment k % 256
    w, h = 1024, 256   # 128 x 32 tiles
    ones = np.ones((h, w), np.uint8)
    for rank in range(2):
        tiles = SC.shard_tiles(w, h, rank, 2)
        assert tiles.size == 2048 and tiles[0] == rank and (np.diff(tiles) == 2).all()
        assert (SC.segment_loads(ones, w, h, tiles) == 512).all()
    p = np.zeros((h, w), np.uint8)
    p[8, 24] = 1   # tile 128 + 3 = 131: shard 1's 65th tile, its workgroup 16; the whole frame's workgroup 32
    assert SC.segment_loads(p, w, h)[32] == 1
    assert SC.segment_loads(p, w, h, SC.shard_tiles(w, h, 1, 2))[16] == 1
    assert SC.segment_loads(p, w, h, SC.shard_tiles(w, h, 0, 2)).sum() == 0
    assert SC.segment_loads(ones, w, h, np.arange(1024, 1028))[0] == 256


def test_the_cases_are_the_sizes_they_are_meant_to_be():
    assert {k: (SC.workgroups(k), SC.capacity(k)) for k in SC.CASES} == {
        "one_over": (257, 512), "one_over_ragged": (257, 512), "three_parts": (516, 768), "four_parts": (1024, 1024), "two_shards": (512, 512)}
    for case, tiles in (("one_over", 1025), ("one_over_ragged", 1025), ("three_parts", 2064), ("four_parts", 4096)):
        w, h = SC.CASES[case].size
        assert (w // 8) * (h // 8) == tiles
    w, h = SC.CASES["one_over_ragged"].size
    assert w % 8 and h % 8 and (w & ~7, h & ~7) == SC.CASES["one_over"].size


# ---- what each case reaches, from the reference alone ----

def test_the_tables_name_four_materials(refs):
    for case in SC.CASES:
        t = refs.tables(case)
        assert int((t["alone"][0] != 0).sum()) == 1 and int((t["all"][0] != 0).sum()) == 2
        assert int((t["all"][1]["chance"] != 0).sum()) == 1 and int((t["all"][2]["chance"] != 0).sum()) == 2


@pytest.mark.parametrize("case", ["one_over", "one_over_ragged"])
@pytest.mark.parametrize("kind", ["sun", "everything"])
def test_one_over_gives_segment_0_a_second_producer_with_work(refs, case, kind):
    f = refs.frame(case, kind, 4, 3, load=True)
    for sample in range(3):
        path, sun = _loads(f, case, PATH, sample), _loads(f, case, SUN, sample)
        print(f"{case} {kind} sample {sample}: segment 0 holds {path[0]} path and {sun[0]} sun records; the others at most {path[1:].max()}, {sun[1:].max()}")
        assert path[0] > 256 and sun[0] > 256
        assert path[1:].max() <= 256 and sun[1:].max() <= 256   # (one producer each)
    if case == "one_over_ragged":
        w, h = SC.CASES["one_over"].size
        assert not f.load[:, :, h:].any() and not f.load[:, :, :, w:].any() and not f.rgb[h:].any() and not f.rgb[:, w:].any()


@pytest.mark.parametrize("kind", ["sun", "everything"])
def test_three_parts_fills_a_segment_past_512(refs, kind):
    f = refs.frame("three_parts", kind, 4, 3, load=True)
    for sample in range(3):
        path, sun = _loads(f, "three_parts", PATH, sample), _loads(f, "three_parts", SUN, sample)
        print(f"three_parts {kind} sample {sample}: {int((path > 512).sum())} segments over 512 path records, {int((sun > 512).sum())} over 512 sun records")
        assert (path > 512).sum() >= 1 and (sun > 512).sum() >= 1
        assert path[4:].max() <= 512   # (segments 0-3 alone have a third producer)


def test_four_parts_fills_the_path_sun_and_lamp_buffers(refs):
    for kind, bits in (("sun", (PATH, SUN)), ("lamps", (PATH, LAMP)), ("everything", (PATH, SUN, LAMP))):
        f = refs.frame("four_parts", kind, 4, 3, load=True)
        for sample in range(3):
            for bit in bits:
                n = _loads(f, "four_parts", bit, sample)
                print(f"four_parts {kind} sample {sample} bit {bit}: max {n.max()}, {int((n > 256).sum())} segments over 256, {int((n > 512).sum())} over 512")
                if bit == LAMP:
                    assert (n > 256).sum() >= 64
                else:
                    assert (n > 512).sum() >= 128
    # (why the lamp buffer needs this frame: at half its width no segment's lamp records pass 256)


@pytest.mark.parametrize("bounces", [2, 4])
def test_four_parts_translucent_chains_give_the_pools_second_workgroup_work(refs, bounces):
    """A plain (here: translucent) frame of 3 spp on the default route is ONE chain of three samples: the primary launch appends all
    three samples' paths, and the pool kernel's workgroup `part` of a segment takes records part * 4E ..., E = 256 (four batches
    of 64 a wave) or 320 (five, with two frames in flight).  Past 1280 records part = 1 has work under both."""
    f = refs.frame("four_parts", "translucent", bounces, 3, load=True)
    c = SC.CASES["four_parts"]
    chain = SC.segment_loads(((f.load[:, 0] & PATH) != 0).sum(0), *c.size)
    print(f"four_parts translucent b{bounces}: chain load max {chain.max()}, {int((chain > 1280).sum())} segments over 1280, {int((chain > 2560).sum())} over 2560")
    assert chain.max() > 1280
    assert chain.max() <= 3 * SC.capacity("four_parts")
    assert (chain > 2048).any() and (chain > 2560).any()   # part = 2 as well, 4 and 5 batches


def test_two_shards_fill_each_shards_buffers_past_256(refs):
    """Of the two frames tests/test_gpu_path_segments.py renders shard by shard: "everything" fills a segment of each shard's path
    and sun buffers past 256 records; its fullest lamp segment holds 257 and 253 (measured here), which is why the second frame,
    with the ground dark, is there: 338 and 353."""
    best = {}
    for kind in ("everything", "everything, second lit"):
        f = refs.frame("two_shards", kind, 4, 3, load=True)
        for rank in range(2):
            for bit in (PATH, SUN, LAMP):
                best[kind, rank, bit] = max(int(_loads(f, "two_shards", bit, sample, segment, rank).max()) for sample in range(3) for segment in range(4))
                first = max(int(_loads(f, "two_shards", bit, sample, 0, rank).max()) for sample in range(3))
                print(f"two_shards {kind} rank {rank} bit {bit}: at most {best[kind, rank, bit]} records in a segment ({first} behind a primary launch)")
            assert best[kind, rank, PATH] <= SC.capacity("two_shards")
    for rank in range(2):
        assert best["everything", rank, PATH] > 256 and best["everything", rank, SUN] > 256
        assert best["everything, second lit", rank, LAMP] > 256


@pytest.mark.parametrize("case", list(SC.CASES))
def test_the_radiance_stays_below_512(refs, case):
    for kind in ("everything", "lamps", "sun", "translucent") + (("everything, second lit",) if case == "two_shards" else ()):
        for spp in (1, 3):
            f = refs.frame(case, kind, 4, spp, load=(spp == 3))
            assert np.isfinite(f.rgb).all() and float(f.rgb.max()) < 512.0, (kind, spp, float(f.rgb.max()))
