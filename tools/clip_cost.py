"""Throughput of the box queries (include/vrt.h vrt_clip_moves): 1 M player-sized boxes (0.9 x 4 x 0.9, Player::create_aabb's
shape) with their feet on C2's terrain, once standing (mv = (0, -0.05, 0): the fall Player::update asks about at rest) and once
walking (a horizontal step of up to 0.3 besides), autojump on as the client has it.  The GPU launch is timed by events on the
context's stream with device pointers (no host copies): 30 warm-up launches, then 50 timed ones; the CPU mirror
(vrth_world_clip_moves) runs on 1 thread and on 16.  Prints one JSON line; with an argument, also writes it to that path."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from voxelraytracing_amd import Gpu, _ffi, scenes  # noqa: E402
from voxelraytracing_amd.world import box_queries  # noqa: E402

PLAYER = np.array((0.9, 4.0, 0.9))


def player_boxes(world, top, n, walking, seed=1):
    """top: highest_vox_at per column, [z][x], min.y - 1 where there is none (Gpu.top_map()["y"])."""
    W = world.size_in_voxels()
    lo = np.array(world.min_voxel(), np.float64)
    rng = np.random.default_rng(seed)
    cxz = lo[[0, 2]] + rng.uniform(1.0, W - 1.0, (n, 2))
    col = np.floor(cxz - lo[[0, 2]]).astype(np.int64)
    feet = top[col[:, 1], col[:, 0]] + 1.0
    frm = np.stack([cxz[:, 0] - PLAYER[0] / 2, feet, cxz[:, 1] - PLAYER[2] / 2], axis=1)
    mv = np.zeros((n, 3))
    mv[:, 1] = -0.05
    if walking:
        mv[:, 0::2] = rng.uniform(-0.3, 0.3, (n, 2))
    return box_queries(frm, frm + PLAYER, mv, True)


def gpu_rate(gpu, q, warmup=30, reps=50):
    dq = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
    dout = torch.empty(q.size * 32, dtype=torch.uint8, device="cuda")
    for _ in range(warmup):
        gpu.clip_moves_device(dq.data_ptr(), q.size, dout.data_ptr())
    torch.cuda.current_stream().synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gpu.clip_moves_device(dq.data_ptr(), q.size, dout.data_ptr())
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    out = dout.cpu().numpy().view(_ffi.BOX_MOVE_DTYPE)
    return ms, out


def cpu_rate(world, mats, q, threads):
    t0 = time.perf_counter()
    out = world.clip_moves(q, mats, threads=threads)
    return time.perf_counter() - t0, out


def main():
    sc = scenes.c2((64, 64))
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    side = torch.cuda.Stream()   # (not torch's default stream: vrt_set_stream(NULL) would mean the context's own)
    gpu.set_stream(side.cuda_stream)
    res = {"world": "C2 8^3 procedural", "boxes": 1 << 20, "box": PLAYER.tolist(), "warmup_launches": 30, "timed_launches": 50}
    top = gpu.top_map()["y"].astype(np.int64)   # the ground under every column: one vrt_read_top_map
    for name, walking in (("standing", False), ("walking", True)):
        q = player_boxes(sc.world, top, 1 << 20, walking)
        with torch.cuda.stream(side):
            ms, out = gpu_rate(gpu, q)
        host = sc.world.clip_moves(q, sc.materials)
        same = bool((out.view(np.uint8) == host.view(np.uint8)).all())
        med = statistics.median(ms)
        r1_s, _ = cpu_rate(sc.world, sc.materials, q[:65536], 1)
        r16_s = min(cpu_rate(sc.world, sc.materials, q, 16)[0] for _ in range(3))
        res[name] = {"gpu_ms_median": round(med, 4), "gpu_ms_best": round(min(ms), 4), "gpu_ms_worst": round(max(ms), 4),
                     "gpu_gboxes_per_s": round(q.size / med / 1e6, 3), "bit_exact_vs_cpu_mirror": same,
                     "clipped": int(((out["flags"] & 7) != 0).sum()), "stepped_up": int(((out["flags"] & 8) != 0).sum()),
                     "second_passes": int((out["boxes"][:, 1] > 0).sum()), "mean_boxes_first_pass": round(float(out["boxes"][:, 0].mean()), 2),
                     "cpu_1_thread_mboxes_per_s": round(65536 / r1_s / 1e6, 3), "cpu_16_threads_mboxes_per_s": round(q.size / r16_s / 1e6, 3)}
    regs = {k: v for k, v in _ffi.kernel_registers().items() if "clip_moves_kernel" in k}
    res["kernel_registers"] = list(regs.values())[0] if regs else None
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
