"""Cost of the column queries (include/vrt.h vrt_read_top_map, vrt_column_tops, vrt_get_voxels) on C2's world (8^3 chunks) and on
a 32^3-chunk procedural world: the whole map from above, 2^20 column queries and 2^20 voxel look-ups, the GPU beside the host
twin (vrth_world_top_map, vrth_world_column_tops, vrth_world_get_voxels) on 16 threads.  A GPU launch is timed by events on the
context's stream around the _device call (device pointers, no host copies): 20 warm-up launches, then 50 timed ones; the host
twin is the best of 3 runs by the host's clock.  Every GPU result is compared with the host twin's, byte for byte.  The map's
host form (vrt_read_top_map: launch, copy out, wait) is timed too, by the host's clock.  One process; prints one JSON line and
with an argument writes the table and that line to the path (profiles/column_cost.txt is such a file with notes around it)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from voxelraytracing_amd import Gpu, _ffi, scenes  # noqa: E402
from voxelraytracing_amd.world import column_queries  # noqa: E402

N = 1 << 20
WARMUP, REPS, THREADS = 20, 50, 16


def gpu_ms(launch):
    for _ in range(WARMUP):
        launch()
    torch.cuda.current_stream().synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"gpu_ms_median": round(statistics.median(ms), 4), "gpu_ms_best": round(min(ms), 4), "gpu_ms_worst": round(max(ms), 4)}


def host_ms(fn):
    best, out = None, None
    for _ in range(3):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return round(best, 3), out


def same(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint8).ravel(), np.ascontiguousarray(b).view(np.uint8).ravel()))


def measure(sc, side):
    world, mats = sc.world, sc.materials
    gpu = Gpu(world.max_nodes(), world.size_in_chunks(), (64, 64), device=0)
    gpu.upload_world(world, mats)
    gpu.set_stream(side.cuda_stream)
    W = world.size_in_voxels()
    lo = np.array(world.min_voxel(), np.int64)
    rng = np.random.default_rng(1)
    res = {"size_in_chunks": world.size_in_chunks(), "columns": W * W}
    with torch.cuda.stream(side):
        # the map, every voxel that is not air and the solid ones
        for name, solid in (("map", False), ("map_solid", True)):
            dmap = torch.empty(W * W * 8, dtype=torch.uint8, device="cuda")
            r = gpu_ms(lambda: gpu.top_map_device(dmap.data_ptr(), _ffi.COLUMN_SOLID if solid else 0))
            got = dmap.cpu().numpy().view(_ffi.TOP_ENTRY_DTYPE)
            r["host_16_threads_ms"], want = host_ms(lambda: world.top_map(solid, mats, threads=THREADS))
            t0 = time.perf_counter()
            for _ in range(10):
                gpu.top_map(solid)
            r["gpu_host_form_ms"] = round((time.perf_counter() - t0) * 100.0, 3)
            r["equal_to_host_twin"] = same(got, want)
            r["host_over_gpu"] = round(r["host_16_threads_ms"] / r["gpu_ms_median"], 1)
            r["columns_with_a_top"] = int((got["voxel"] != 0).sum())
            res[name] = r
        # 2^20 column queries: random columns of the box, half of them from a random y, half of them solid
        pos = rng.integers(0, W, (N, 3)) + lo
        q = column_queries(pos[:, 0], pos[:, 2], from_y=pos[:, 1], solid=rng.random(N) < 0.5)
        q["flags"][::2] &= ~np.uint32(_ffi.COLUMN_FROM_Y)
        dq = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
        dout = torch.empty(N * 16, dtype=torch.uint8, device="cuda")
        r = gpu_ms(lambda: gpu.column_tops_device(dq.data_ptr(), N, dout.data_ptr()))
        got = dout.cpu().numpy().view(_ffi.COLUMN_TOP_DTYPE)
        r["host_16_threads_ms"], want = host_ms(lambda: world.column_tops(q, mats, threads=THREADS))
        r["equal_to_host_twin"] = same(got, want)
        r["host_over_gpu"] = round(r["host_16_threads_ms"] / r["gpu_ms_median"], 1)
        r["found"] = int((got["status"] == _ffi.COLUMN_FOUND).sum())
        res["column_tops"] = r
        # 2^20 voxel look-ups: random positions in the box and a margin of 8 around it
        p = np.ascontiguousarray((rng.integers(-8, W + 8, (N, 3)) + lo).astype(np.int32))
        dp = torch.from_numpy(p.view(np.uint8).reshape(-1).copy()).to("cuda")
        dv = torch.empty(N * 4, dtype=torch.uint8, device="cuda")
        r = gpu_ms(lambda: gpu.get_voxels_device(dp.data_ptr(), N, dv.data_ptr()))
        got = dv.cpu().numpy().view(_ffi.VOXEL_AT_DTYPE)
        r["host_16_threads_ms"], want = host_ms(lambda: world.get_voxels(p, threads=THREADS))
        r["equal_to_host_twin"] = same(got, want)
        r["host_over_gpu"] = round(r["host_16_threads_ms"] / r["gpu_ms_median"], 1)
        r["by_status"] = np.bincount(got["status"], minlength=4).tolist()
        res["get_voxels"] = r
    res["tables"] = bool(gpu.accel_info().available)
    gpu.close()
    return res


def table(res):
    lines = ["                                   GPU per launch (median / best / worst)   host twin, 16 threads   host / GPU   equal"]
    for world in ("c2", "s32"):
        r = res[world]
        lines.append(f"  {world}: {r['size_in_chunks']}^3 chunks, {r['columns']} columns, derived tables {'present' if r['tables'] else 'absent (octree walk)'}")
        for key, what in (("map", "the map"), ("map_solid", "the map, SOLID"), ("column_tops", "2^20 column queries"), ("get_voxels", "2^20 voxel look-ups")):
            k = r[key]
            lines.append(f"    {what:<22}         {k['gpu_ms_median']:8.4f} / {k['gpu_ms_best']:8.4f} / {k['gpu_ms_worst']:8.4f} ms"
                         f"        {k['host_16_threads_ms']:10.3f} ms     {k['host_over_gpu']:8.1f}x   {'yes' if k['equal_to_host_twin'] else 'NO'}")
    return "\n".join(lines)


def main():
    side = torch.cuda.Stream()   # (not torch's default stream: vrt_set_stream(NULL) would mean the context's own)
    res = {"queries": N, "warmup_launches": WARMUP, "timed_launches": REPS, "host_threads": THREADS}
    res["c2"] = measure(scenes.c2((64, 64)), side)
    res["s32"] = measure(scenes.procedural(32, (64, 64)), side)
    regs = _ffi.kernel_registers()
    res["kernel_registers"] = {n: next((v for k, v in regs.items() if n in k), None) for n in ("get_voxels_kernel", "column_tops_kernel", "top_map_kernel")}
    line = json.dumps(res)
    print(table(res))
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(table(res) + "\n\n" + line + "\n")


if __name__ == "__main__":
    main()
