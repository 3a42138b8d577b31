"""vrt_generate_chunks / vrt_build_chunks on the MI355X — every chunk held word for word and count for count to the host's
svo_build_bottom_up(gen_dense(seed, pos)) / svo_build_bottom_up(dense) (csrc/host/worldgen.hpp is the specification), and the
worlds ClientWorld.generate(gpu=...) makes held byte for byte to the CPU path's."""
import ctypes as C

import numpy as np
import pytest

from voxelraytracing_amd import Gpu, MODE_PRIMARY_SHADOW, VrtError, _ffi, scenes
from voxelraytracing_amd.world import ClientWorld, SetVoxelErr, gen_dense, svo_build_bottom_up

from util import gpu_for_scene

pytestmark = pytest.mark.gpu

BATCH = 2048   # chunks per internal batch (include/vrt.h)
LIM = 1 << 26


@pytest.fixture(scope="module")
def gpu():
    g = Gpu(1 << 16, 2, (64, 64), device=0)
    yield g
    g.close()


def _want(dense):
    try:
        return svo_build_bottom_up(dense)
    except SetVoxelErr:
        return None   # refused: more than 32767 nodes


def _check(nodes, offs, wants, what):
    assert offs.size == len(wants) + 1 and offs[0] == 0 and int(offs[-1]) == nodes.size, what
    for i, w in enumerate(wants):
        got = nodes[int(offs[i]):int(offs[i + 1])]
        if w is None:
            assert got.size == 0, f"{what}: chunk {i} should be refused, got {got.size} nodes"
            continue
        assert got.size == w.size, f"{what}: chunk {i}: {got.size} nodes, host {w.size}"
        bad = np.flatnonzero(got != w)
        assert bad.size == 0, f"{what}: chunk {i}: {bad.size} words differ, first at {bad[0]}: {got[bad[0]]:#06x} host {w[bad[0]]:#06x}"


# ---- blocks for the builder ----

def _morton_cells():
    """(x4, y4, z4) of the 4096 level-4 cells."""
    c = np.arange(4096)
    ax = lambda s: ((s & 1) | ((s >> 2) & 2) | ((s >> 4) & 4) | ((s >> 6) & 8))
    return ax(c), ax(c >> 1), ax(c >> 2)


def _mixed_exactly(k_uniform, rng):
    """A block whose tree has 4681 - k_uniform mixed cells: a voxel checkerboard (every cell mixed) with k_uniform level-4
    cells, at most two per level-3 cell, filled with one id (their parents stay mixed)."""
    x = np.arange(32)
    d = (((x[None, None, :] + x[None, :, None] + x[:, None, None]) & 1) + 1).astype(np.uint16)   # d[z, y, x]
    x4, y4, z4 = _morton_cells()
    parents = rng.permutation(512)
    picked = []
    for p in parents:
        picked += list(8 * p + rng.choice(8, 2, replace=False))
    for c in picked[:k_uniform]:
        d[2 * z4[c]:2 * z4[c] + 2, 2 * y4[c]:2 * y4[c] + 2, 2 * x4[c]:2 * x4[c] + 2] = 9
    return d.reshape(-1)


def _blocks(rng):
    """At least 2 000 blocks of every kind the builder meets, refused ones in the middle of batches."""
    out = []
    x = np.arange(32)
    X, Y, Z = x[None, None, :], x[None, :, None], x[:, None, None]
    for _ in range(700):   # random sparse, random ids
        d = np.zeros(32768, np.uint16)
        k = int(rng.integers(1, 600))
        d[rng.integers(0, 32768, k)] = rng.integers(1, 0x10000, k)
        out.append(d)
    for _ in range(40):    # random dense (refused, mostly) and dense over two ids
        out.append(rng.integers(0, 3 if rng.random() < 0.5 else 0x10000, 32768).astype(np.uint16))
    for _ in range(700):   # few ids in boxes
        d = np.full((32, 32, 32), rng.choice([0, 4, 0x8004]), np.uint16)
        ids = rng.choice([0, 4, 5, 0x8004, 0x7FFF, 0xFFFF], 3)
        for _ in range(int(rng.integers(1, 7))):
            lo = rng.integers(0, 32, 3)
            hi = lo + rng.integers(1, 17, 3)
            d[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = rng.choice(ids)
        out.append(d.reshape(-1))
    for _ in range(300):   # one voxel at a sampled position
        d = np.zeros(32768, np.uint16)
        d[int(rng.integers(0, 32768))] = int(rng.integers(1, 0x10000))
        out.append(d)
    for s in range(5):     # checkerboards at every scale (s = 0: every cell mixed, refused)
        for a, b in ((1, 2), (0, 0x8000), (0x7FFF, 0xFFFF)):
            out.append(np.where((((X >> s) + (Y >> s) + (Z >> s)) & 1) == 1, a, b).astype(np.uint16).reshape(-1))
    for k in (586, 585, 600, 584):   # 4095 mixed cells (accepted: 32 761 nodes), 4096 (refused), 4081, 4097
        out.append(_mixed_exactly(k, rng))
    for a, b in ((0x0001, 0x8001), (0x7FFF, 0xFFFF), (0, 0x8000)):   # ids equal under 0x7FFF but not as 16-bit ids
        for _ in range(4):
            d = np.full(32768, a, np.uint16)
            d[rng.integers(0, 32768, int(rng.integers(1, 50)))] = b
            out.append(d)
        out.append(np.where(np.broadcast_to(X, (32, 32, 32)) < 16, a, b).astype(np.uint16).reshape(-1))
    for v in (0, 7, 0x7FFF, 0x8000, 0xFFFF):   # all-air and uniform blocks
        out.append(np.full(32768, v, np.uint16))
    for _ in range(400):   # generated terrain
        out.append(gen_dense(1, (int(rng.integers(-40, 40)), int(rng.integers(0, 7)), int(rng.integers(-40, 40)))))
    order = rng.permutation(len(out))
    blocks = [out[i] for i in order]
    full = rng.integers(0, 0x10000, 32768).astype(np.uint16)   # refused, at a batch's first and last chunk and mid-batch
    for at in (1000, BATCH - 1, BATCH):
        blocks.insert(at, full)
    return np.stack(blocks)


@pytest.fixture(scope="module")
def blocks():
    return _blocks(np.random.default_rng(20261016))


def test_build_chunks_matches_the_host_builder(gpu, blocks):
    assert blocks.shape[0] >= 2000 and blocks.shape[0] > BATCH
    wants = [_want(d) for d in blocks]
    refused = [i for i, w in enumerate(wants) if w is None]
    assert 1000 in refused and BATCH - 1 in refused and BATCH in refused
    sizes = [w.size for w in wants if w is not None]
    assert 32761 in sizes and 1 in sizes
    nodes, offs = gpu.build_chunks(blocks, strict=False)
    _check(nodes, offs, wants, "build_chunks")
    with pytest.raises(VrtError) as e:
        gpu.build_chunks(blocks[995:1005])
    assert e.value.code == _ffi.VRT_ERR_OUT_OF_RANGE


def test_the_refusal_limit_is_4096_mixed_cells(gpu):
    rng = np.random.default_rng(5)
    d = np.stack([_mixed_exactly(586, rng), _mixed_exactly(585, rng)])
    assert svo_build_bottom_up(d[0]).size == 32761 and _want(d[1]) is None
    nodes, offs = gpu.build_chunks(d, strict=False)
    assert list(np.diff(offs)) == [32761, 0]
    _check(nodes, offs, [svo_build_bottom_up(d[0]), None], "4095 / 4096")


def test_full_16_bit_ids_decide_uniformity(gpu):
    d = np.stack([np.full(32768, 0xFFFF, np.uint16), np.full(32768, 0x8001, np.uint16),
                  np.where(np.arange(32768) % 2 == 0, 0x0001, 0x8001).astype(np.uint16),
                  np.where(np.arange(32768) < 16384, 0x7FFF, 0xFFFF).astype(np.uint16)])
    nodes, offs = gpu.build_chunks(d, strict=False)
    wants = [_want(b) for b in d]
    assert wants[0].tolist() == [0x7FFF] and wants[1].tolist() == [0x0001] and wants[2] is None and wants[3].size == 9
    _check(nodes, offs, wants, "16-bit ids")


# ---- the generator ----

def _pool(seed, r=8):
    return [(x, y, z) for z in range(-r, r) for y in range(-1, 7) for x in range(-r, r)]


def test_generate_chunks_matches_the_host_generator(gpu):
    pos = _pool(1)   # 2 048 chunks, negative coordinates included
    dense = [gen_dense(1, p) for p in pos]
    assert any((d == 3).any() for d in dense) and any((d == 45).any() for d in dense)   # under sea level, at the snow line
    crowns = [i for i, d in enumerate(dense) if (d.reshape(32, 32, 32)[[0, -1]] == 62).any() or
              (d.reshape(32, 32, 32)[:, [0, -1]] == 62).any() or (d.reshape(32, 32, 32)[:, :, [0, -1]] == 62).any()]
    assert len(crowns) >= 10   # chunks whose faces cut through a tree's crown
    nodes, offs = gpu.generate_chunks(1, pos)
    _check(nodes, offs, [svo_build_bottom_up(d) for d in dense], "seed 1")


@pytest.mark.parametrize("seed", [7, 0xDEADBEEF])
def test_generate_chunks_other_seeds(gpu, seed):
    rng = np.random.default_rng(seed & 0xFFFF)
    pos = np.stack([rng.integers(-200, 200, 600), rng.integers(-2, 8, 600), rng.integers(-200, 200, 600)], axis=1)
    nodes, offs = gpu.generate_chunks(seed, pos)
    _check(nodes, offs, [svo_build_bottom_up(gen_dense(seed, tuple(p))) for p in pos], f"seed {seed:#x}")


def test_positions_near_the_int32_limit(gpu):
    edge = [LIM - 1, -(LIM - 1), LIM - 2, -(LIM - 7), 0]
    pos = [(x, y, z) for x in edge for z in edge for y in (1, 3, -LIM + 1, -LIM + 3, -LIM + 6, -LIM + 7, LIM - 1)]
    nodes, offs = gpu.generate_chunks(1, pos)
    wants = [svo_build_bottom_up(gen_dense(1, p)) for p in pos]
    assert len({w.tobytes() for w in wants}) > 10
    _check(nodes, offs, wants, "near 2^26")
    for bad in [(LIM, 0, 0), (0, -LIM, 0), (0, 0, LIM), (-LIM, 5, 5), (0x7FFFFFFF, 0, 0)]:
        with pytest.raises(VrtError) as e:
            gpu.generate_chunks(1, [(0, 2, 0), bad])
        assert e.value.code == _ffi.VRT_ERR_INVALID_ARG


def test_batch_sizes_and_capacity(gpu):
    pos = np.array(_pool(1, 9)[:BATCH + 5], np.int32)
    wants = [svo_build_bottom_up(gen_dense(1, tuple(p))) for p in pos]
    for n in (0, 1, 63, 65, BATCH + 5):
        nodes, offs = gpu.generate_chunks(1, pos[:n])
        assert offs.size == n + 1
        _check(nodes, offs, wants[:n], f"n = {n}")
    lib = _ffi.vrt()
    for n in (65, BATCH + 5):
        need = sum(w.size for w in wants[:n])
        buf = np.full(need + 16, 0xABCD, np.uint16)
        offs = np.zeros(n + 1, np.uint64)
        p = np.ascontiguousarray(pos[:n])
        rc = lib.vrt_generate_chunks(gpu._h, 1, p.ctypes.data, n, buf.ctypes.data, need - 1, offs.ctypes.data)
        assert rc == _ffi.VRT_ERR_OOM
        assert int(offs[n]) == need and list(np.diff(offs)) == [w.size for w in wants[:n]]
        assert (buf == 0xABCD).all(), "nodes must be untouched on VRT_ERR_OOM"
        rc = lib.vrt_generate_chunks(gpu._h, 1, p.ctypes.data, n, None, 0, offs.ctypes.data)
        assert rc == _ffi.VRT_ERR_OOM and int(offs[n]) == need
        rc = lib.vrt_generate_chunks(gpu._h, 1, p.ctypes.data, n, buf.ctypes.data, need, offs.ctypes.data)
        assert rc == 0
        _check(buf[:need], offs, wants[:n], f"exact capacity, n = {n}")
        assert (buf[need:] == 0xABCD).all()
    offs = np.full(1, 7, np.uint64)
    assert lib.vrt_build_chunks(gpu._h, None, 0, None, 0, offs.ctypes.data) == 0 and offs[0] == 0


# ---- worlds ----

def _state(w):
    return w.nodes().copy(), w.chunk_roots(), w.chunk_alloc_status(), w.populated_count()


def _same_world(a, b):
    sa, sb = _state(a), _state(b)
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def test_generate_on_the_gpu_makes_the_cpu_world(gpu):
    cpu = ClientWorld((8, 8, 8), 1 << 25, 16)
    cpu.generate(0, 1)
    got = ClientWorld((8, 8, 8), 1 << 25, 16)
    got.generate(0, 1, gpu=gpu)
    _same_world(cpu, got)
    # an anchor step (center_chunks): the missing chunks, in grid order, with the same ranges
    for w in (cpu, got):
        w.center_chunks((9, 8, 7))
    r_cpu = cpu.generate_missing(0, 1)
    r_gpu = got.generate_missing(0, 1, gpu=gpu)
    assert r_cpu.shape[0] > 100 and np.array_equal(r_cpu, r_gpu)
    _same_world(cpu, got)
    with pytest.raises(ValueError):
        got.generate(1, 0, gpu=gpu)
    with pytest.raises(ValueError):
        got.generate_missing(1, 0, gpu=gpu)


def test_a_gpu_generated_world_renders_the_cpu_worlds_frame(gpu):
    sc = scenes.c2((128, 72))
    w = ClientWorld((4, 4, 4), sc.world.max_nodes(), 8)
    w.generate(0, 1, gpu=gpu)
    _same_world(sc.world, w)
    ref = gpu_for_scene(sc)
    ref.render(MODE_PRIMARY_SHADOW)
    rgb0, ids0, _ = ref.read_output()
    g = Gpu(w.max_nodes(), 8, sc.size, device=0)
    g.upload_world(w, sc.materials)
    g.write_cam_data(sc.cam)
    g.write_settings(sc.settings)
    g.render(MODE_PRIMARY_SHADOW)
    rgb1, ids1, _ = g.read_output()
    assert np.array_equal(ids0, ids1) and np.array_equal(rgb0, rgb1)
    # render, then generate on the same context, then read: the frame is the one rendered
    g.render(MODE_PRIMARY_SHADOW)
    nodes, offs = g.generate_chunks(1, _pool(1, 3))
    rgb2, ids2, _ = g.read_output()
    assert np.array_equal(ids0, ids2) and np.array_equal(rgb0, rgb2)
    assert offs.size == 6 * 6 * 8 + 1
    ref.close()
    g.close()


def test_a_multi_device_rehearsal_generates_on_its_first_device(gpu, blocks):
    grp = Gpu(1 << 16, 2, (64, 64), devices=[0, 0])
    pos = _pool(7, 4)
    assert all(np.array_equal(a, b) for a, b in zip(grp.generate_chunks(7, pos), gpu.generate_chunks(7, pos)))
    assert all(np.array_equal(a, b) for a, b in zip(grp.build_chunks(blocks[:300], strict=False),
                                                   gpu.build_chunks(blocks[:300], strict=False)))
    grp.close()
