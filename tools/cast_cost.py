"""Throughput of the world queries (include/vrt.h vrt_cast_rays): 1 M picking rays (max_dist 10, the client's pick of
clientdesktop/src/main.rs:320-325) and 1 M rays with max_dist 300 over C2's world, cast from C2's eye over a 70-degree square
of view directions; the GPU launch timed by events on the context's stream (device pointers: no host copies), the CPU mirror
(vrth_world_cast_rays) on 1 thread and on 16.  Prints one JSON line; with an argument, also writes it to that path."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from voxelraytracing_amd import Gpu, _ffi, scenes  # noqa: E402
from voxelraytracing_amd.world import column_queries, ray_queries  # noqa: E402


def camera_rays(sc, n_side):
    pitch0, yaw0 = np.radians(np.float32(sc.rot[0])), np.radians(np.float32(sc.rot[1]))
    a = np.radians(np.linspace(-35.0, 35.0, n_side, dtype=np.float32))
    p, y = np.meshgrid(pitch0 + a, yaw0 + a, indexing="ij")
    p, y = p.ravel().astype(np.float32), y.ravel().astype(np.float32)
    r = np.cos(p)
    dirs = np.stack([r * -np.sin(y), -np.sin(p), r * -np.cos(y)], axis=1).astype(np.float32)
    return np.broadcast_to(np.asarray(sc.eye, np.float32), dirs.shape), dirs


def gpu_rate(gpu, q, reps=20):
    dq = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
    dout = torch.empty(q.size * 32, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        gpu.cast_rays_device(dq.data_ptr(), q.size, dout.data_ptr())
    torch.cuda.current_stream().synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gpu.cast_rays_device(dq.data_ptr(), q.size, dout.data_ptr())
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    out = dout.cpu().numpy().view(_ffi.RAY_HIT_DTYPE)
    return statistics.median(ms), min(ms), out


def cpu_rate(world, q, threads):
    t0 = time.perf_counter()
    out = world.cast_rays(q["start"], q["dir"], q["max_dist"], threads=threads)
    return time.perf_counter() - t0, out


def main():
    sc = scenes.c2((64, 64))
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    side = torch.cuda.Stream()   # (not torch's default stream: vrt_set_stream(NULL) would mean the context's own)
    gpu.set_stream(side.cuda_stream)
    starts, dirs = camera_rays(sc, 1024)
    # the pick: a player's eye 2.5 voxels above the terrain at the world's centre (from C2's own eye, 24 voxels up, nothing is
    # within 10)
    c = sc.world.size_in_chunks() * 16
    player = np.asarray((c + 0.5, int(gpu.column_tops(column_queries([c], [c]))["y"][0]) + 2.5, c + 0.5), np.float32)
    res = {"world": "C2 8^3 procedural", "rays": int(starts.shape[0]), "pick_eye": player.tolist(), "eye": list(sc.eye)}
    for name, md, eye in (("pick_max_dist_10", 10.0, player), ("max_dist_300", 300.0, None)):
        q = ray_queries(starts if eye is None else np.broadcast_to(eye, dirs.shape), dirs, md)
        with torch.cuda.stream(side):
            med, best, out = gpu_rate(gpu, q)
        host = sc.world.cast_rays(q["start"], q["dir"], q["max_dist"])
        same = bool((out.view(np.uint8) == host.view(np.uint8)).all())
        r1_s, _ = cpu_rate(sc.world, q[:65536], 1)
        r16_s, _ = cpu_rate(sc.world, q, 16)
        res[name] = {"gpu_ms_median": round(med, 4), "gpu_ms_best": round(best, 4), "gpu_grays_per_s": round(q.size / med / 1e6, 3),
                     "hits": int((out["status"] == 1).sum()), "bit_exact_vs_cpu_mirror": same,
                     "cpu_1_thread_mrays_per_s": round(65536 / r1_s / 1e6, 3), "cpu_16_threads_mrays_per_s": round(q.size / r16_s / 1e6, 3)}
    regs = {k: v for k, v in _ffi.kernel_registers().items() if "cast_rays_kernel" in k}
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
