"""The client's collisions restated in numpy float32, and the worlds and boxes the clip tests use.

Aabb::expand / translate / clip_{x,y,z}_collide (common/src/math.rs:18-126), ClientWorld::get_collisions_w
(client/src/world.rs:369-391) and clip_aabb_movement (client/src/player.rs:202-244), written from the Rust text, scalar, one
numpy float32 operation per operation of the reference, in its order.  Independent of the C++ mirror and of the kernel: the
world is cast_ray_cases.DenseWorld (the voxels as a dense array), the solid test a list of 256 bools made from the material
table, the record include/vrt.h's vrt_box_move.
"""
from __future__ import annotations

import numpy as np

from voxelraytracing_amd import ClientWorld, _ffi
from voxelraytracing_amd.world import box_queries

from cast_ray_cases import DenseWorld, floor_world  # noqa: F401  (floor_world: re-exported for the tests)

F = np.float32
EPSILON = F(0.00001)              # math.rs:3
LIMIT = F(8388608.0)              # 2^23: include/vrt.h
MAX_VOXELS = 4096                 # VRT_BOX_MAX_VOXELS
ZERO, ONE = F(0.0), F(1.0)
PLAYER = (0.9, 4.0, 0.9)          # the issue's player-sized box


class Aabb:
    """math.rs:5-16: from and to as [x, y, z] lists of float32."""

    def __init__(self, from_, to):
        self.from_ = [F(v) for v in from_]
        self.to = [F(v) for v in to]

    def expand(self, a):
        """math.rs:18-44"""
        from_, to = list(self.from_), list(self.to)
        for k in range(3):
            if a[k] < ZERO:
                from_[k] = from_[k] + a[k]
            if a[k] > ZERO:
                to[k] = to[k] + a[k]
        return Aabb(from_, to)

    def translate(self, a):
        """math.rs:123-125"""
        return Aabb([self.from_[k] + a[k] for k in range(3)], [self.to[k] + a[k] for k in range(3)])

    def _clip(self, c, a, k, i, j):
        """clip_x_collide (k, i, j = 0, 1, 2), clip_y_collide (1, 0, 2), clip_z_collide (2, 0, 1): math.rs:50-115"""
        if c.to[i] <= self.from_[i] or c.from_[i] >= self.to[i]:
            return a
        if c.to[j] <= self.from_[j] or c.from_[j] >= self.to[j]:
            return a
        if a > ZERO and c.to[k] <= self.from_[k]:
            m = self.from_[k] - c.to[k] - EPSILON
            if m < a:
                a = m
        if a < ZERO and c.from_[k] >= self.to[k]:
            m = self.to[k] - c.from_[k] + EPSILON
            if m > a:
                a = m
        return a

    def clip_x_collide(self, c, a):
        return self._clip(c, a, 0, 1, 2)

    def clip_y_collide(self, c, a):
        return self._clip(c, a, 1, 0, 2)

    def clip_z_collide(self, c, a):
        return self._clip(c, a, 2, 0, 1)


def unit_box(p) -> Aabb:
    """world.rs:383-385: Aabb::new(pos.as_vec3(), pos.as_vec3() + 1.0)"""
    lo = [F(int(v)) for v in p]
    return Aabb(lo, [v + ONE for v in lo])


def solid_table(materials) -> list:
    """voxelpack.get(v).is_solid() for v = 0..255 as the material table holds it (graphics/mod.rs:38-46)."""
    return [materials[v].is_empty == 0 and materials[v].is_liquid == 0 for v in range(256)]


def voxel_at(world: DenseWorld, p) -> int:
    """self.get_voxel(pos).unwrap_or(Voxel::EMPTY): 0 outside the world (and where there is no chunk: DenseWorld holds 0)."""
    x, y, z = (int(p[a]) - int(world.min[a]) for a in range(3))
    if 0 <= x < world.W and 0 <= y < world.W and 0 <= z < world.W:
        return int(world.v[z, y, x])
    return 0


def collisions_range(bb: Aabb):
    lo = [int(np.floor(v)) for v in bb.from_]
    hi = [int(np.ceil(v)) for v in bb.to]
    return lo, hi


def get_collisions_w(world: DenseWorld, bb: Aabb, solid) -> list:
    """world.rs:369-391, the three loops as written -> the solid voxels' positions (each stands for unit_box(p))."""
    lo, hi = collisions_range(bb)
    out = []
    for x in range(lo[0], hi[0]):
        for y in range(lo[1], hi[1]):
            for z in range(lo[2], hi[2]):
                if solid[min(voxel_at(world, (x, y, z)), 255)]:
                    out.append((x, y, z))
    return out


def get_collisions_w_block(world: DenseWorld, bb: Aabb, solid) -> list:
    """The same positions in the same order with one array lookup for the whole range (the fuzz asks for 60 000 boxes);
    tests/test_clip_move.py holds it to the loops above."""
    lo, hi = collisions_range(bb)
    n = [hi[a] - lo[a] for a in range(3)]
    if min(n) <= 0:
        return []
    ax = [np.arange(lo[a], hi[a], dtype=np.int64) - int(world.min[a]) for a in range(3)]
    inside = [(c >= 0) & (c < world.W) for c in ax]
    v = np.zeros(n, np.int64)   # [x][y][z]
    ix, iy, iz = (np.nonzero(m)[0] for m in inside)
    if ix.size and iy.size and iz.size:
        v[np.ix_(ix, iy, iz)] = world.v[np.ix_(ax[2][iz], ax[1][iy], ax[0][ix])].transpose(2, 1, 0)
    hit = np.asarray(solid, bool)[np.minimum(v, 255)]
    return [(int(x) + lo[0], int(y) + lo[1], int(z) + lo[2]) for x, y, z in np.argwhere(hit)]   # argwhere: x, then y, then z


def clip_list(bbox: Aabb, mv, boxes):
    """player.rs:210-215: the loop over an explicit list of world boxes, in list order."""
    c = [F(v) for v in mv]
    for wb in boxes:
        c[1] = wb.clip_y_collide(bbox, c[1])
        c[0] = wb.clip_x_collide(bbox, c[0])
        c[2] = wb.clip_z_collide(bbox, c[2])
    return c


def clip_aabb_movement(bbox: Aabb, mv, world_fn, autojump: bool):
    """player.rs:202-244 -> (mv_clipped, flags, boxes) with flags and boxes as include/vrt.h's vrt_box_move has them."""
    mv = [F(v) for v in mv]
    world_bboxs = world_fn(bbox.expand(mv))
    mv_clipped = clip_list(bbox, mv, [unit_box(p) for p in world_bboxs])
    eq = [mv_clipped[k] == mv[k] for k in range(3)]
    flags = sum(0 if eq[k] else 1 << k for k in range(3))
    boxes = [len(world_bboxs), 0]
    if autojump and (not eq[0] or not eq[2]):
        bbox = bbox.translate([F(0.0), F(1.1), F(0.0)])
        world_bboxs = world_fn(bbox.expand(mv))
        jmp_clipped = clip_list(bbox, mv, [unit_box(p) for p in world_bboxs])
        jmp_clipped[1] = F(0.0)
        boxes[1] = len(world_bboxs)
        if any(abs(jmp_clipped[k]) > abs(mv_clipped[k]) for k in range(3)):
            mv_clipped[1] = mv_clipped[1] + ONE
            mv_clipped[0] = jmp_clipped[0]
            mv_clipped[2] = jmp_clipped[2]
            flags |= 8
    return mv_clipped, flags, boxes


def rejected(q, bb: Aabb, mv) -> bool:
    """include/vrt.h: a float that is not finite or is 2^23 or more in magnitude; more than 4096 voxels in the first range."""
    vals = [F(v) for v in list(q["from"]) + list(q["to"]) + list(q["mv"])]
    if not all(abs(v) < LIMIT for v in vals):   # (a NaN compares false)
        return True
    lo, hi = collisions_range(bb.expand(mv))
    n = [hi[a] - lo[a] for a in range(3)]
    return min(n) > 0 and n[0] * n[1] * n[2] > MAX_VOXELS


def clip_moves(q: np.ndarray, world: DenseWorld, solid, gather=get_collisions_w_block) -> np.ndarray:
    """The restatement's vrt_box_move record for every query of q (BOX_QUERY_DTYPE)."""
    out = np.zeros(q.size, _ffi.BOX_MOVE_DTYPE)
    with np.errstate(all="ignore"):
        for i in range(q.size):
            bb = Aabb(q["from"][i], q["to"][i])
            mv = [F(v) for v in q["mv"][i]]
            if rejected(q[i], bb, mv):
                out["status"][i] = _ffi.BOX_REJECTED
                continue
            c, flags, boxes = clip_aabb_movement(bb, mv, lambda b: gather(world, b, solid), bool(q["flags"][i] & _ffi.BOX_AUTOJUMP))
            out["mv"][i] = c
            out["flags"][i] = flags
            out["boxes"][i] = boxes
    return out


def records_differ(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Indices where two BOX_MOVE_DTYPE arrays differ in any of their 32 bytes."""
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1, 32)
    b = np.ascontiguousarray(b).view(np.uint8).reshape(-1, 32)
    assert a.shape == b.shape
    return np.nonzero(np.any(a != b, axis=1))[0]


def floor_materials():
    """The standard table with voxel 1 — the stone of cast_ray_cases.floor_world, "fire" (a gas) in the standard pack — made solid."""
    from voxelraytracing_amd import std_materials
    m = std_materials()
    m[1].is_empty = 0
    m[1].is_liquid = 0
    return m


def known_world() -> ClientWorld:
    """The world of the known answers: 2^3 chunks with min voxel (-32, -32, -32).  The lower four chunks are limestone (4: a
    floor whose top face is y = 0), the upper four air, except chunk (-1, 0, -1), which is missing.  On the floor stand a wall
    two voxels high (x = 5, y = 0..1, z = -1..1), a step one voxel high (x = 2, y = 0, z = 9..11) and a wall of water two
    voxels high (3: x = 5, y = 0..1, z = 19..21)."""
    w = ClientWorld((0, 0, 0), 1 << 16, 2)
    assert tuple(w.min_voxel()) == (-32, -32, -32)
    for cx in (-1, 0):
        for cz in (-1, 0):
            w.create_chunk((cx, -1, cz), np.array([4], np.uint16))
            if (cx, cz) != (-1, -1):
                w.create_chunk((cx, 0, cz), np.array([0], np.uint16))
    for z in (-1, 0, 1):
        for y in (0, 1):
            w.set_voxel((5, y, z), 4)
            w.set_voxel((5, y, z + 20), 3)
        w.set_voxel((2, 0, z + 10), 4)
    return w


def height_map(world: ClientWorld) -> np.ndarray:
    """highest_vox_at (world.rs:359-366) for every column: H[z][x] in world coordinates, the world's min y - 1 where the
    column is empty (liquids count: they are not Voxel::EMPTY)."""
    d = DenseWorld(world)
    full = d.v != 0                                    # [z][y][x]
    top = d.W - 1 - np.argmax(full[:, ::-1, :], axis=1)
    return np.where(full.any(axis=1), top, -1) + int(d.min[1])


def fuzz_queries(world: ClientWorld, n: int, seed: int) -> np.ndarray:
    """n boxes over a world.  Player-sized boxes and boxes of random size up to 3 voxels per axis; feet within a few voxels of
    highest_vox_at — on the ground, in it, above it — a share snapped to integer or half-integer coordinates; mv in
    [-1.5, 1.5] with exact zeros and -0; walkers (a small fall, a horizontal step); boxes outside the world, over missing
    chunks and in water wherever the world has them; inverted boxes; every kind of rejected query."""
    rng = np.random.default_rng(seed)
    lo = np.array(world.min_voxel(), np.float64)
    W = float(world.size_in_voxels())
    H = height_map(world)
    size = np.where(rng.random((n, 1)) < 0.5, np.array(PLAYER), rng.uniform(0.2, 3.0, (n, 3)))
    # the column under the box's centre; a tenth of the boxes up to 6 voxels outside the world
    cxz = lo[[0, 2]] + rng.uniform(0.0, W, (n, 2))
    out = rng.random(n) < 0.1
    cxz[out] = lo[[0, 2]] + np.where(rng.random((int(out.sum()), 2)) < 0.5, rng.uniform(-6.0, 1.0, (int(out.sum()), 2)),
                                      W + rng.uniform(-1.0, 6.0, (int(out.sum()), 2)))
    col = np.clip(np.floor(cxz - lo[[0, 2]]).astype(np.int64), 0, int(W) - 1)
    ground = H[col[:, 1], col[:, 0]].astype(np.float64) + 1.0   # the top face of the highest voxel
    kind = rng.choice(5, n, p=[0.3, 0.2, 0.2, 0.1, 0.2])
    feet = ground + np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0.0, rng.uniform(-0.9, 0.0, n), rng.uniform(-3.0, 0.0, n),
                                                                            rng.uniform(0.0, 4.0, n)], rng.uniform(-6.0, 6.0, n))
    frm = np.stack([cxz[:, 0] - size[:, 0] / 2, feet, cxz[:, 1] - size[:, 2] / 2], axis=1)
    snap = rng.integers(0, 6, n)
    frm[snap == 1] = np.floor(frm[snap == 1])
    frm[snap == 2] = np.floor(frm[snap == 2]) + 0.5
    whole = rng.random(n) < 0.15                      # sizes of whole voxels: with a snapped corner every face is on a plane
    size[whole] = np.ceil(size[whole])
    to = frm + size
    mv = rng.uniform(-1.5, 1.5, (n, 3))
    walk = rng.random(n) < 0.4                        # Player::update's usual question: a small fall and a horizontal step
    mv[walk, 1] = np.where(rng.random(int(walk.sum())) < 0.7, -0.05, rng.uniform(-0.6, 0.6, int(walk.sum())))
    mv[walk, 0] *= 0.3
    mv[walk, 2] *= 0.3
    z = rng.random((n, 3))
    mv[z < 0.08] = 0.0
    mv[(z >= 0.08) & (z < 0.12)] = -0.0
    q = box_queries(frm, to, mv, rng.random(n) < 0.7)
    q["flags"] |= (rng.integers(0, 4, n) == 0).astype(np.uint32) << 7   # unknown bits are ignored
    inv = np.nonzero(rng.random(n) < 0.01)[0]         # inverted on one axis
    a = rng.integers(0, 3, inv.size)
    q["from"][inv, a], q["to"][inv, a] = q["to"][inv, a], q["from"][inv, a].copy()
    bad = np.nonzero(rng.random(n) < 0.02)[0]         # rejected: a float that is not finite or too large ...
    vals = np.array([np.nan, np.inf, -np.inf, 8388608.0, -8388608.0, 3.0e7], np.float32)
    field = np.array(["from", "to", "mv"])[rng.integers(0, 3, bad.size)]
    for i, f, a, v in zip(bad, field, rng.integers(0, 3, bad.size), vals[rng.integers(0, vals.size, bad.size)]):
        q[f][i, a] = v
    big = np.nonzero(rng.random(n) < 0.01)[0]         # ... or a range of more than 4096 voxels
    q["to"][big] = q["from"][big] + rng.uniform(16.0, 40.0, (big.size, 3)).astype(np.float32)
    return q


def player_queries(world: ClientWorld, n: int, seed: int) -> np.ndarray:
    """n player-sized boxes standing on the world's terrain (feet on the top face of highest_vox_at), a quarter at rest, the
    others walking: Player::update's question, frame after frame."""
    rng = np.random.default_rng(seed)
    lo = np.array(world.min_voxel(), np.float64)
    W = float(world.size_in_voxels())
    H = height_map(world)
    cxz = lo[[0, 2]] + rng.uniform(1.0, W - 1.0, (n, 2))
    col = np.floor(cxz - lo[[0, 2]]).astype(np.int64)
    feet = H[col[:, 1], col[:, 0]].astype(np.float64) + 1.0
    frm = np.stack([cxz[:, 0] - PLAYER[0] / 2, feet, cxz[:, 1] - PLAYER[2] / 2], axis=1)
    mv = np.stack([rng.uniform(-0.3, 0.3, n), np.full(n, -0.05), rng.uniform(-0.3, 0.3, n)], axis=1)
    mv[rng.random(n) < 0.25, 0::2] = 0.0
    return box_queries(frm, frm + np.array(PLAYER), mv, True)


def population_facts(q: np.ndarray, r: np.ndarray) -> dict:
    """The shares the issue's conditions on a fuzz population are stated in (of the queries that ran)."""
    moved = r["status"] == _ffi.BOX_MOVED
    ran = r[moved]
    n = max(1, ran.size)
    two = ((q["flags"][moved] & _ffi.BOX_AUTOJUMP) != 0) & ((ran["flags"] & 5) != 0)   # player.rs:221: the second pass ran
    return {"ran": int(ran.size), "rejected": int((r["status"] == _ffi.BOX_REJECTED).sum()),
            "clipped": float(((ran["flags"] & 7) != 0).sum()) / n,
            "x": float(((ran["flags"] & 1) != 0).sum()) / n, "y": float(((ran["flags"] & 2) != 0).sum()) / n,
            "z": float(((ran["flags"] & 4) != 0).sum()) / n,
            "stepped": float(((ran["flags"] & 8) != 0).sum()) / n,
            "pass2_not_taken": float((two & ((ran["flags"] & 8) == 0)).sum()) / n,
            "no_boxes": int((ran["boxes"][:, 0] == 0).sum()), "eight_boxes": int((ran["boxes"][:, 0] >= 8).sum())}


def assert_population(facts: dict, what=""):
    """The issue's conditions: a population that met them cannot have passed on trivia."""
    assert facts["clipped"] >= 0.25, (what, facts)
    assert min(facts["x"], facts["y"], facts["z"]) >= 0.05, (what, facts)
    assert facts["stepped"] >= 0.02, (what, facts)
    assert facts["pass2_not_taken"] >= 0.02, (what, facts)
    assert facts["ran"] and facts["rejected"], (what, facts)
    assert facts["no_boxes"] and facts["eight_boxes"], (what, facts)
