"""Host world — thin Python handles on the C++ mirror of the reference's ``ClientWorld``.

Names and argument meaning follow client/src/world.rs:259-367 and common/src/world/mod.rs; all logic
lives in libvrt_host.so (voxelraytracing_amd/csrc/host/world.hpp).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _ffi

CHUNK_SIZE = 32               # common/src/world/mod.rs:10
CHUNK_DEPTH = 5               # :14
NODES_PER_CHUNK = 37449       # :18
CHUNK_INIT_FREE_MEM = 2048    # :23


class SetVoxelErr(Exception):
    """common/src/world/mod.rs:129-135"""
    NAMES = {1: "PosOutOfBounds", 2: "OutOfMemory", 3: "NoChunk", 4: "NoChange", 5: "BadChunkData"}

    def __init__(self, code: int):
        super().__init__(self.NAMES.get(code, str(code)))
        self.code = code
        self.kind = self.NAMES.get(code, str(code))


def _i3(v):
    return (C.c_int32 * 3)(int(v[0]), int(v[1]), int(v[2]))


def _u16p(a: np.ndarray):
    assert a.dtype == np.uint16 and a.flags.c_contiguous
    return a.ctypes.data_as(C.c_void_p)


class Node:
    """Node word helpers, common/src/world/mod.rs:150-194."""
    SPLIT_MASK, DATA_MASK = 0x8000, 0x7FFF

    @staticmethod
    def new(voxel: int) -> int:
        return voxel & Node.DATA_MASK

    @staticmethod
    def new_split(child_idx: int) -> int:
        return child_idx | Node.SPLIT_MASK

    @staticmethod
    def is_split(w: int) -> bool:
        return (w & Node.SPLIT_MASK) != 0

    @staticmethod
    def voxel(w: int) -> int:
        return w & Node.DATA_MASK

    child_idx = voxel


@dataclass
class ChunkState:
    range_start: int
    range_end: int
    last_used_addr: int
    free_mem: list


class ClientWorld:
    """client/src/world.rs:259-367."""

    def __init__(self, center, max_nodes: int, size: int):
        self._lib = _ffi.host()
        self._h = self._lib.vrth_world_new(_i3(center), max_nodes, size)
        if not self._h:
            raise MemoryError("vrth_world_new failed")

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.vrth_world_free(self._h)
            self._h = None

    # --- chunk ingest / edits ---
    def create_chunk(self, pos, nodes: np.ndarray) -> int:
        nodes = np.ascontiguousarray(nodes, dtype=np.uint16)
        root = C.c_uint32()
        rc = self._lib.vrth_world_create_chunk(self._h, _i3(pos), _u16p(nodes), nodes.size, C.byref(root))
        if rc:
            raise SetVoxelErr(rc)
        return root.value

    def set_voxel(self, pos, voxel: int):
        """-> (range_start, range_len) of the chunk to re-upload (main.rs:352-362)."""
        s, n = C.c_uint32(), C.c_uint32()
        rc = self._lib.vrth_world_set_voxel(self._h, _i3(pos), voxel, C.byref(s), C.byref(n))
        if rc:
            e = SetVoxelErr(rc)
            if e.kind == "OutOfMemory":      # Svo::set_node returned mid-way: the splits made so far are in the pool
                e.range = (s.value, n.value)
            raise e
        return s.value, n.value

    def get_voxel(self, pos) -> int:
        v = C.c_uint16()
        rc = self._lib.vrth_world_get_voxel(self._h, _i3(pos), C.byref(v))
        if rc:
            raise SetVoxelErr(rc)
        return v.value

    def cast_ray(self, start, dir, max_dist: float):
        """common::math::cast_ray(start, dir, max_dist, |p| get_voxel(p) is solid) — math.rs:153-226, as the client's pick calls
        it (clientdesktop/src/main.rs:320-325): None, or (pos, face) like Option<HitResult>.  Strict binary32 (vrth_world_cast_ray);
        a query the reference would loop forever or overflow on (include/vrt.h) raises ValueError."""
        h = self.cast_ray_record(start, dir, max_dist)
        if h.status == _ffi.RAY_REJECTED:
            raise ValueError(f"cast_ray rejected: start {tuple(start)} / max_dist {max_dist} (|start| < 2^24, max_dist <= 2^20)")
        if h.status != _ffi.RAY_HIT:
            return None
        return tuple(h.pos), tuple(h.face)

    def cast_ray_record(self, start, dir, max_dist: float) -> _ffi.RayHit:
        """The same as the whole vrt_ray_hit record (the DDA's dist and the status included)."""
        out = _ffi.RayHit()
        self._lib.vrth_world_cast_ray(self._h, (C.c_float * 3)(*[float(v) for v in start]), (C.c_float * 3)(*[float(v) for v in dir]),
                                      float(max_dist), C.byref(out))
        return out

    def cast_rays(self, starts, dirs, max_dist, threads: int = 0) -> np.ndarray:
        """Many casts on the CPU (vrth_world_cast_rays): (n,3) starts and dirs, a scalar or (n,) max_dist; returns the
        _ffi.RAY_HIT_DTYPE records."""
        q = ray_queries(starts, dirs, max_dist)
        out = np.zeros(q.size, _ffi.RAY_HIT_DTYPE)
        if q.size:
            self._lib.vrth_world_cast_rays(self._h, q.ctypes.data, q.size, out.ctypes.data, threads)
        return out

    # --- collisions (csrc/host/collide.hpp): materials is a (Material * 256) table, e.g. graphics.std_materials() ---
    def get_collisions(self, from_, to, materials) -> np.ndarray:
        """ClientWorld::get_collisions_w(&Aabb::new(from, to), voxelpack) — world.rs:369-391: the (n,3) integer positions of
        the solid voxels (each stands for the box [p, p + 1]) in the reference's order.  ValueError where vrt_clip_moves
        would reject the box (include/vrt.h)."""
        f3 = lambda v: (C.c_float * 3)(*[float(c) for c in v])  # noqa: E731
        n = C.c_uint32()
        out = np.zeros((_ffi.BOX_MAX_VOXELS, 3), np.int32)
        if self._lib.vrth_world_get_collisions(self._h, f3(from_), f3(to), C.cast(materials, C.c_void_p), out.ctypes.data, out.shape[0],
                                               C.byref(n)):
            raise ValueError(f"get_collisions rejected: {tuple(from_)} .. {tuple(to)} (|v| < 2^23, at most {_ffi.BOX_MAX_VOXELS} voxels)")
        return out[:n.value].copy()

    def clip_move(self, from_, to, mv, materials, autojump: bool = True) -> _ffi.BoxMove:
        """clip_aabb_movement(Aabb::new(from, to), mv, |bb| get_collisions_w(bb), autojump) — player.rs:202-244 in strict binary32
        (vrth_world_clip_move): the whole vrt_box_move record; .mv is the reference's answer when .status is BOX_MOVED."""
        q = box_queries([from_], [to], [mv], autojump)
        out = _ffi.BoxMove()
        self._lib.vrth_world_clip_move(self._h, C.cast(materials, C.c_void_p), C.cast(q.ctypes.data, C.POINTER(_ffi.BoxQuery)), C.byref(out))
        return out

    def clip_moves(self, queries: np.ndarray, materials, threads: int = 0) -> np.ndarray:
        """Many of them on the CPU (vrth_world_clip_moves): _ffi.BOX_QUERY_DTYPE records (box_queries) in, _ffi.BOX_MOVE_DTYPE out."""
        q = np.ascontiguousarray(queries, _ffi.BOX_QUERY_DTYPE)
        out = np.zeros(q.size, _ffi.BOX_MOVE_DTYPE)
        if q.size:
            self._lib.vrth_world_clip_moves(self._h, C.cast(materials, C.c_void_p), q.ctypes.data, q.size, out.ctypes.data, threads)
        return out

    def center_chunks(self, anchor) -> int:
        return self._lib.vrth_world_center_chunks(self._h, _i3(anchor))

    def resize(self, size: int) -> None:
        self._lib.vrth_world_resize(self._h, size)

    def generate(self, kind: int = 0, seed: int = 1, threads: int = 0, gpu=None) -> None:
        """Every cell of the grid.  gpu: a Gpu that builds the chunks (kind 0 only; Gpu.generate_chunks), then create_chunks —
        the same world as the CPU path, byte for byte."""
        if gpu is not None:
            self._generate_on(gpu, kind, seed, self.grid_positions())
            return
        rc = self._lib.vrth_world_generate(self._h, kind, seed, threads)
        if rc:
            raise SetVoxelErr(rc)

    def generate_missing(self, kind: int = 0, seed: int = 1, threads: int = 0, gpu=None) -> np.ndarray:
        """Fill the grid's empty cells (what the server answers request_missing_chunks with, client/src/lib.rs:80-108).
        -> u32[n, 2] of (root, node count): the ranges to upload, as GameState::process_cmd returns them.  gpu: as generate's."""
        if gpu is not None:
            pos = self.grid_positions()
            return self._generate_on(gpu, kind, seed, pos[self.chunk_roots() == 0])
        cap = self.size_in_chunks() ** 3
        out = np.zeros((cap, 2), dtype=np.uint32)
        n = C.c_uint32()
        rc = self._lib.vrth_world_generate_missing(self._h, kind, seed, threads, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
        if rc:
            raise SetVoxelErr(rc)
        return out[:n.value].copy()

    def create_chunks(self, positions, nodes: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        """create_chunk(positions[i], nodes[offsets[i]:offsets[i+1]]) in order, all-air chunks skipped (vrth_world_create_chunks):
        -> u32[n, 2] of (root, node count) of the chunks created, as generate_missing returns them."""
        pos = np.ascontiguousarray(np.asarray(positions, np.int32).reshape(-1, 3))
        nodes = np.ascontiguousarray(nodes, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = pos.shape[0]
        if offsets.size != n + 1 or (n and int(offsets[n]) > nodes.size):
            raise ValueError(f"{n} positions need {n + 1} offsets within the {nodes.size} nodes")
        out = np.zeros((max(n, 1), 2), dtype=np.uint32)
        cnt = C.c_uint32()
        rc = self._lib.vrth_world_create_chunks(self._h, pos.ctypes.data, n, nodes.ctypes.data, offsets.ctypes.data,
                                                out.ctypes.data, n, C.byref(cnt))
        if rc:
            raise SetVoxelErr(rc)
        return out[:cnt.value].copy()

    def grid_positions(self) -> np.ndarray:
        """The chunk position of every cell of the grid, (S^3, 3) int32 in grid order (x fastest), as chunk_roots() lists them."""
        S = self.size_in_chunks()
        mn = np.asarray(self.min_voxel(), np.int64) // CHUNK_SIZE
        i = np.arange(S ** 3, dtype=np.int64)
        return np.stack([mn[0] + i % S, mn[1] + (i // S) % S, mn[2] + i // (S * S)], axis=1).astype(np.int32)

    def _generate_on(self, gpu, kind: int, seed: int, positions) -> np.ndarray:
        if kind != 0:
            raise ValueError(f"generate kind {kind} on the GPU: only kind 0 (the procedural generator) is built there")
        nodes, offs = gpu.generate_chunks(seed, positions, strict=False)
        return self.create_chunks(positions, nodes, offs)   # (a refused chunk: SetVoxelErr OutOfMemory, as the CPU path)

    # --- views ---
    def nodes(self) -> np.ndarray:
        """The whole flat pool as a zero-copy u16 view (client/src/world.rs:292-294)."""
        n = self._lib.vrth_world_max_nodes(self._h)
        buf = (C.c_uint16 * n).from_address(self._lib.vrth_world_nodes(self._h))
        a = np.frombuffer(buf, dtype=np.uint16)
        a.flags.writeable = False
        return a

    def nodes_ptr(self) -> int:
        return self._lib.vrth_world_nodes(self._h)

    def max_nodes(self) -> int:
        return self._lib.vrth_world_max_nodes(self._h)

    def chunk_roots(self) -> np.ndarray:
        """ChunkGrid::chunk_roots (world.rs:154-159): a fresh array, as the reference's fresh Vec."""
        n = self._lib.vrth_world_chunk_roots(self._h, None, 0)
        out = np.empty(n, dtype=np.uint32)
        self._lib.vrth_world_chunk_roots(self._h, out.ctypes.data_as(C.c_void_p), n)
        return out

    def chunk_roots_view(self) -> np.ndarray:
        """The mirror's own table, zero-copy and read-only: valid until resize(); its entries follow the grid (include/vrt_host.h)."""
        n = self._lib.vrth_world_chunk_roots(self._h, None, 0)
        a = np.frombuffer((C.c_uint32 * n).from_address(self._lib.vrth_world_chunk_roots_ptr(self._h)), dtype=np.uint32)
        a.flags.writeable = False
        return a

    def roots_generation(self) -> int:
        """Changes whenever chunk_roots() may have: the tag of Gpu.write_chunk_roots(..., tag=)."""
        return self._lib.vrth_world_chunk_roots_generation(self._h)

    def _info(self):
        mn = (C.c_int32 * 3)()
        sv, sc, pop = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._lib.vrth_world_info(self._h, mn, C.byref(sv), C.byref(sc), C.byref(pop))
        return tuple(mn), sv.value, sc.value, pop.value

    def min_voxel(self):
        return self._info()[0]

    def size_in_voxels(self) -> int:
        return self._info()[1]

    def size_in_chunks(self) -> int:
        return self._info()[2]

    def populated_count(self) -> int:
        return self._info()[3]

    def chunk_alloc_status(self):
        f, m = C.c_uint32(), C.c_uint32()
        self._lib.vrth_world_alloc_status(self._h, C.byref(f), C.byref(m))
        return f.value, m.value

    def chunk_state(self, pos):
        rs, re, lu = C.c_uint32(), C.c_uint32(), C.c_uint32()
        spans = (C.c_uint32 * 4096)()
        n = self._lib.vrth_world_chunk_state(self._h, _i3(pos), C.byref(rs), C.byref(re), C.byref(lu), spans, 2048)
        if n < 0:
            return None
        return ChunkState(rs.value, re.value, lu.value, [(spans[2 * i], spans[2 * i + 1]) for i in range(min(n, 2048))])

    def highest_vox_at(self, x: int, z: int):
        y = C.c_int32()
        return y.value if self._lib.vrth_world_highest_vox_at(self._h, x, z, C.byref(y)) else None

    def get_voxels(self, positions, threads: int = 0) -> np.ndarray:
        """get_voxel for every (n,3) integer position on the CPU (vrth_world_get_voxels), as vrt_get_voxels records it:
        _ffi.VOXEL_AT_DTYPE records (voxel, status = VOXEL_OK / VOXEL_OUT_OF_BOUNDS / VOXEL_NO_CHUNK)."""
        pos = np.ascontiguousarray(np.asarray(positions, np.int32).reshape(-1, 3))
        out = np.zeros(pos.shape[0], _ffi.VOXEL_AT_DTYPE)
        if pos.shape[0]:
            self._lib.vrth_world_get_voxels(self._h, pos.ctypes.data, pos.shape[0], out.ctypes.data, threads)
        return out

    # --- column tops (csrc/both/column_top.h): materials is a (Material * 256) table or None when no query sets COLUMN_SOLID ---
    def column_top(self, x: int, z: int, from_y=None, solid: bool = False, materials=None) -> _ffi.ColumnTop:
        """highest_vox_at with include/vrt.h's flags (vrth_world_column_top): the whole vrt_column_top record.  from_y: start at
        min(from_y, top of the world); solid: a voxel counts when the material table says it is solid."""
        q = _ffi.ColumnQuery(x, z, 0 if from_y is None else from_y,
                             (0 if from_y is None else _ffi.COLUMN_FROM_Y) | (_ffi.COLUMN_SOLID if solid else 0))
        out = _ffi.ColumnTop()
        self._lib.vrth_world_column_top(self._h, C.cast(materials, C.c_void_p), C.byref(q), C.byref(out))
        return out

    def column_tops(self, queries: np.ndarray, materials=None, threads: int = 0) -> np.ndarray:
        """Many of them on the CPU (vrth_world_column_tops): _ffi.COLUMN_QUERY_DTYPE records (column_queries) in,
        _ffi.COLUMN_TOP_DTYPE records out."""
        q = np.ascontiguousarray(queries, _ffi.COLUMN_QUERY_DTYPE)
        out = np.zeros(q.size, _ffi.COLUMN_TOP_DTYPE)
        if q.size:
            self._lib.vrth_world_column_tops(self._h, C.cast(materials, C.c_void_p), q.ctypes.data, q.size, out.ctypes.data, threads)
        return out

    def top_map(self, solid: bool = False, materials=None, threads: int = 0) -> np.ndarray:
        """The whole world from above on the CPU (vrth_world_top_map): _ffi.TOP_ENTRY_DTYPE records [z - min.z][x - min.x]; a
        column where nothing counts holds y = min.y - 1, voxel 0."""
        W = self.size_in_voxels()
        out = np.zeros((W, W), _ffi.TOP_ENTRY_DTYPE)
        if self._lib.vrth_world_top_map(self._h, C.cast(materials, C.c_void_p), _ffi.COLUMN_SOLID if solid else 0, out.ctypes.data, threads):
            raise ValueError("top_map: a null world")
        return out

    # --- region files (servercli/src/main.rs:25-73) ---
    def load_region(self, data: bytes, region_pos) -> int:
        """create_chunk every chunk of a reference region file that lies inside the grid; returns how many."""
        n = C.c_uint32()
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        rc = self._lib.vrth_region_load_into_world(self._h, buf, len(data), _i3(region_pos), C.byref(n))
        if rc < 0:
            raise ValueError("malformed region file")
        if rc:
            raise SetVoxelErr(rc)
        return n.value

    def save_region(self, region_pos) -> bytes:
        size = self._lib.vrth_region_save_from_world(self._h, _i3(region_pos), None, 0)
        buf = (C.c_uint8 * size)()
        self._lib.vrth_region_save_from_world(self._h, _i3(region_pos), buf, size)
        return bytes(buf)

    # --- the wire protocol's chunk payload (common/src/net.rs:46-55) ---
    def ingest_chunk_msg(self, data: bytes):
        """GameState::process_cmd for one `ClientCmd::GiveChunkData` at the front of `data` (client/src/lib.rs:110-118).
        -> (consumed bytes, chunk pos, root, node count): upload pool[root, root + count) afterwards (main.rs:289-295).
        None if the message is incomplete; ValueError if it is malformed or another command; SetVoxelErr from create_chunk
        (PosOutOfBounds = the reference's `received_oob_chunks`)."""
        used, pos, root, n = C.c_uint64(), (C.c_int32 * 3)(), C.c_uint32(), C.c_uint32()
        buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
        rc = self._lib.vrth_chunk_msg_ingest(self._h, buf, len(data), C.byref(used), pos, C.byref(root), C.byref(n))
        if rc == -2:
            return None
        if rc < 0:
            raise ValueError("malformed GiveChunkData" if rc == -1 else "not a GiveChunkData message")
        if rc:
            e = SetVoxelErr(rc)
            e.consumed = used.value
            raise e
        return used.value, tuple(pos), root.value, n.value

    def encode_chunk_msg(self, pos) -> bytes:
        """What the reference server sends for this chunk (server/src/lib.rs:229-233)."""
        size = self._lib.vrth_chunk_msg_encode(self._h, _i3(pos), None, 0)
        if size == 0:
            raise KeyError(f"no chunk at {tuple(pos)}")
        buf = (C.c_uint8 * size)()
        self._lib.vrth_chunk_msg_encode(self._h, _i3(pos), buf, size)
        return bytes(buf)

    def world_data(self) -> _ffi.WorldData:
        """WorldData::from(&world), clientdesktop/src/graphics/mod.rs:121-130."""
        wd = _ffi.WorldData()
        self._lib.vrth_world_data_from(self._h, C.byref(wd))
        return wd


# ---- SVO construction helpers (server/src/world/gen.rs:171-286 and the build's bottom-up builder) ----

def ray_queries(starts, dirs, max_dist) -> np.ndarray:
    """vrt_ray_query records (_ffi.RAY_QUERY_DTYPE) from (n,3) starts and dirs and a scalar or (n,) max_dist, all as float32."""
    starts = np.asarray(starts, np.float32).reshape(-1, 3)
    dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
    if starts.shape != dirs.shape:
        raise ValueError(f"starts {starts.shape} and dirs {dirs.shape} differ")
    q = np.zeros(starts.shape[0], _ffi.RAY_QUERY_DTYPE)
    q["start"] = starts
    q["dir"] = dirs
    q["max_dist"] = np.broadcast_to(np.asarray(max_dist, np.float32), (starts.shape[0],))
    return q


def box_queries(froms, tos, mvs, autojump=True) -> np.ndarray:
    """vrt_box_query records (_ffi.BOX_QUERY_DTYPE) from (n,3) box corners and movements, all as float32; autojump: a bool or (n,)."""
    froms = np.asarray(froms, np.float32).reshape(-1, 3)
    q = np.zeros(froms.shape[0], _ffi.BOX_QUERY_DTYPE)
    q["from"] = froms
    q["to"] = np.asarray(tos, np.float32).reshape(-1, 3)
    q["mv"] = np.asarray(mvs, np.float32).reshape(-1, 3)
    q["flags"] = np.where(np.broadcast_to(np.asarray(autojump, bool), q.shape), _ffi.BOX_AUTOJUMP, 0)
    return q


def column_queries(xs, zs, from_y=None, solid=False) -> np.ndarray:
    """vrt_column_query records (_ffi.COLUMN_QUERY_DTYPE) from (n,) xs and zs; from_y: None (the top of the world), a scalar or
    (n,); solid: a bool or (n,)."""
    xs = np.asarray(xs, np.int32).reshape(-1)
    q = np.zeros(xs.size, _ffi.COLUMN_QUERY_DTYPE)
    q["x"] = xs
    q["z"] = np.asarray(zs, np.int32).reshape(-1)
    if from_y is not None:
        q["from_y"] = np.broadcast_to(np.asarray(from_y, np.int32), q.shape)
        q["flags"] |= _ffi.COLUMN_FROM_Y
    q["flags"] |= np.where(np.broadcast_to(np.asarray(solid, bool), q.shape), _ffi.COLUMN_SOLID, 0).astype(np.uint32)
    return q


def svo_build_by_set_node(dense: np.ndarray, cap: int = NODES_PER_CHUNK + 64) -> np.ndarray:
    dense = np.ascontiguousarray(dense, dtype=np.uint16).reshape(-1)
    assert dense.size == 32768
    nodes = np.zeros(cap, dtype=np.uint16)
    used = _ffi.host().vrth_svo_build_by_set_node(_u16p(dense), _u16p(nodes), cap)
    if not used:
        raise SetVoxelErr(2)
    return nodes[:used].copy()


def svo_build_bottom_up(dense: np.ndarray) -> np.ndarray:
    dense = np.ascontiguousarray(dense, dtype=np.uint16).reshape(-1)
    assert dense.size == 32768
    nodes = np.zeros(32768, dtype=np.uint16)
    n = _ffi.host().vrth_svo_build_bottom_up(_u16p(dense), _u16p(nodes), nodes.size)
    if not n:
        raise SetVoxelErr(2)
    return nodes[:n].copy()


def svo_to_dense(nodes: np.ndarray) -> np.ndarray:
    nodes = np.ascontiguousarray(nodes, dtype=np.uint16)
    dense = np.zeros(32768, dtype=np.uint16)
    _ffi.host().vrth_svo_to_dense(_u16p(nodes), _u16p(dense))
    return dense


def gen_dense(seed: int, chunk_pos) -> np.ndarray:
    dense = np.zeros(32768, dtype=np.uint16)
    _ffi.host().vrth_gen_dense(seed, _i3(chunk_pos), _u16p(dense))
    return dense


def gen_dense_superflat(chunk_pos) -> np.ndarray:
    dense = np.zeros(32768, dtype=np.uint16)
    _ffi.host().vrth_gen_dense_superflat(_i3(chunk_pos), _u16p(dense))
    return dense


# ---- feature shapes (include/vrt.h vrt_shape; server/src/world/gen.rs:312-354) ----

class ShapeError(ValueError):
    """A status of vrth_apply_shapes / vrth_edit_chunks (include/vrt.h vrt_status: -1 invalid argument, -2 out of range, -4 the
    nodes do not fit)."""
    def __init__(self, code: int, what: str):
        super().__init__(f"{what}: vrt status {code}")
        self.code = code


def shape_point(a, voxel: int):
    """BuiltFeature::set_voxel(a, voxel) as a vrt_shape record."""
    return (_ffi.SHAPE_POINT, voxel, tuple(a), (0, 0, 0), 0.0, 0)


def shape_line(a, b, voxel: int):
    """place_line(a, b, voxel)"""
    return (_ffi.SHAPE_LINE, voxel, tuple(a), tuple(b), 0.0, 0)


def shape_sphere(a, r: float, voxel: int):
    """place_sphere(a, r, voxel)"""
    return (_ffi.SHAPE_SPHERE, voxel, tuple(a), (0, 0, 0), r, 0)


def shape_disc(a, r: float, height: int, voxel: int):
    """place_disc(a, r, height, voxel)"""
    return (_ffi.SHAPE_DISC, voxel, tuple(a), (0, 0, 0), r, height)


def shape_records(shapes) -> np.ndarray:
    """vrt_shape records (_ffi.SHAPE_DTYPE) from such an array or a list of shape_point / _line / _sphere / _disc."""
    if isinstance(shapes, np.ndarray) and shapes.dtype == _ffi.SHAPE_DTYPE:
        return np.ascontiguousarray(shapes).reshape(-1)
    return np.array(list(shapes), _ffi.SHAPE_DTYPE).reshape(-1)


def apply_shapes(dense: np.ndarray, chunk_pos, shapes) -> np.ndarray:
    """The shapes, in order, onto a copy of the block dense[x + 32*(y + 32*z)] of the chunk at chunk_pos (vrth_apply_shapes)."""
    out = np.array(dense, dtype=np.uint16).reshape(-1)
    assert out.size == 32768
    sh = shape_records(shapes)
    rc = _ffi.host().vrth_apply_shapes(_u16p(out), _i3(chunk_pos), sh.ctypes.data if sh.size else None, sh.size)
    if rc:
        raise ShapeError(rc, "apply_shapes")
    return out


def edit_chunks(positions, nodes, offsets, shapes, strict: bool = True, threads: int = 0):
    """vrth_edit_chunks, the CPU twin of Gpu.edit_chunks: (n,3) chunk positions, their trees nodes[offsets[i]:offsets[i+1]] and
    the shapes -> (nodes, offsets, changed).  strict=False returns the other chunks when the builder refuses one."""
    pos = np.ascontiguousarray(np.asarray(positions, np.int32).reshape(-1, 3))
    nin = np.ascontiguousarray(nodes, np.uint16)
    oin = np.ascontiguousarray(offsets, np.uint64)
    sh = shape_records(shapes)
    n = pos.shape[0]
    assert oin.size == n + 1
    offs = np.zeros(n + 1, np.uint64)
    changed = np.zeros(n, np.uint8)
    out = np.empty(max(1, 2048 * n), np.uint16)

    def call():
        return _ffi.host().vrth_edit_chunks(pos.ctypes.data, n, nin.ctypes.data, oin.ctypes.data, sh.ctypes.data if sh.size else None,
                                            sh.size, out.ctypes.data, out.size, offs.ctypes.data, changed.ctypes.data, threads)
    rc = call()
    if rc == _ffi.VRT_ERR_OOM and int(offs[n]) > out.size:
        out = np.empty(int(offs[n]), np.uint16)
        rc = call()
    if rc and not (rc == _ffi.VRT_ERR_OUT_OF_RANGE and not strict):
        raise ShapeError(rc, "edit_chunks")
    return out[:int(offs[n])].copy(), offs, changed


def gen_height(seed: int, x: int, z: int) -> int:
    return _ffi.host().vrth_gen_height(seed, x, z)


def region_of_chunk(chunk_pos):
    """ChunkPos::region — common/src/world/mod.rs:90-96: (region pos, position inside the 16^3 region)."""
    rp, ip = (C.c_int32 * 3)(), (C.c_uint32 * 3)()
    _ffi.host().vrth_region_of_chunk(_i3(chunk_pos), rp, ip)
    return tuple(rp), tuple(ip)


def region_file_name(region_pos) -> str:
    """region_path_by_pos — servercli/src/main.rs:25-27."""
    buf = C.create_string_buffer(128)
    _ffi.host().vrth_region_file_name(_i3(region_pos), buf, 128)
    return buf.value.decode()
