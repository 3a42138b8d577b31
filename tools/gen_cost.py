"""What filling the world costs (include/vrt.h vrt_generate_chunks, include/vrt_host.h vrth_world_create_chunks), on one MI355X
against the CPU path (vrth_world_generate / vrth_world_generate_missing) on 1 and 16 threads:
  - Gpu.generate_chunks end to end (host clock around the call, which waits for its results) for one anchor step's 900 chunks
    and for the 27 000 of the 30^3 operating point; Gpu.build_chunks of 900 host blocks (their 59 MB go up first);
  - ClientWorld.generate(gpu=...) of the 30^3 world and of C5's 32^3, split into the GPU call and the create_chunk loop;
  - one anchor step of the 30^3 grid (center_chunks + generate_missing: 900 chunks) on either path.
Every GPU result is compared with the CPU path's world.  The kernel times come from a rocprofv3 --kernel-trace --stats run of
this script (`--quick`: fewer repetitions).  Prints one JSON line; with a path argument, also writes it there."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from voxelraytracing_amd import Gpu, _ffi  # noqa: E402
from voxelraytracing_amd.world import ClientWorld, gen_dense  # noqa: E402

MAX_NODES = 1 << 27   # the 32^3 scenes' budget (scenes.procedural)


def timed(f, reps):
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), out


def same_world(a, b):
    return bool(np.array_equal(a.nodes(), b.nodes()) and np.array_equal(a.chunk_roots(), b.chunk_roots())
                and a.chunk_alloc_status() == b.chunk_alloc_status())


def main():
    quick = "--quick" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = 2 if quick else 5
    gpu = Gpu(1 << 16, 2, (64, 64), device=0)
    res = {"device": "MI355X", "reps": reps}

    # the chunk source alone
    w30 = ClientWorld((15, 15, 15), MAX_NODES, 30)
    cells = w30.grid_positions()
    face = cells[cells[:, 0] == cells[:, 0].max()] + np.array([1, 0, 0], np.int32)   # the 900 cells one anchor step brings in
    gpu.generate_chunks(1, face[:64])   # warm-up: code objects, staging
    for name, pos in (("generate_chunks_900", face), ("generate_chunks_27000", cells)):
        med, best, (nodes, offs) = timed(lambda: gpu.generate_chunks(1, pos), reps)
        res[name] = {"ms_median": round(med, 3), "ms_best": round(best, 3), "nodes": int(offs[-1]),
                     "us_per_chunk": round(med * 1e3 / len(pos), 3)}
    dense = np.stack([gen_dense(1, tuple(p)) for p in face])
    med, best, (nodes_b, offs_b) = timed(lambda: gpu.build_chunks(dense), reps)
    nodes_g, offs_g = gpu.generate_chunks(1, face)
    res["build_chunks_900"] = {"ms_median": round(med, 3), "ms_best": round(best, 3),
                               "same_as_generate": bool(np.array_equal(nodes_b, nodes_g) and np.array_equal(offs_b, offs_g))}

    # whole worlds: the GPU path split into its two halves, then the CPU path
    for name, S, center in (("world_30", 30, (15, 15, 15)), ("world_32_c5", 32, (16, 16, 16))):
        w = ClientWorld(center, MAX_NODES, S)
        pos = w.grid_positions()
        t0 = time.perf_counter()
        nodes, offs = gpu.generate_chunks(1, pos, strict=False)
        t1 = time.perf_counter()
        w.create_chunks(pos, nodes, offs)
        t2 = time.perf_counter()
        e2e = []
        for _ in range(reps):
            wg = ClientWorld(center, MAX_NODES, S)
            t = time.perf_counter()
            wg.generate(0, 1, gpu=gpu)
            e2e.append((time.perf_counter() - t) * 1e3)
        r = {"gpu_generate_ms_median": round(statistics.median(e2e), 2), "of_which_generate_chunks_ms": round((t1 - t0) * 1e3, 2),
             "of_which_create_chunks_ms": round((t2 - t1) * 1e3, 2), "nodes": int(offs[-1]), "d2h_mb": round(int(offs[-1]) * 2 / 1e6, 1)}
        for th in (16, 1):
            if th == 1 and quick:
                continue
            wc = ClientWorld(center, MAX_NODES, S)
            t = time.perf_counter()
            wc.generate(0, 1, threads=th)
            r[f"cpu_{th}_threads_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            r["same_world"] = same_world(wc, wg)
        res[name] = r

    # anchor steps of the 30^3 grid: each moves the grid one chunk in +x (900 new cells)
    worlds = {}
    for path in ("gpu", "cpu16", "cpu1"):
        w = ClientWorld((15, 15, 15), MAX_NODES, 30)
        w.generate(0, 1, gpu=gpu)
        worlds[path] = w
    steps = {"gpu": [], "cpu16": [], "cpu1": []}
    ranges = {}
    for k in range(1, reps + 1):
        for path, w in worlds.items():
            if path == "cpu1" and quick:
                continue
            w.center_chunks((15 + k, 15, 15))
            t = time.perf_counter()
            if path == "gpu":
                ranges[path] = w.generate_missing(0, 1, gpu=gpu)
            else:
                ranges[path] = w.generate_missing(0, 1, threads=16 if path == "cpu16" else 1)
            steps[path].append((time.perf_counter() - t) * 1e3)
    res["anchor_step_30"] = {f"{p}_ms_median": round(statistics.median(v), 2) for p, v in steps.items() if v}
    res["anchor_step_30"]["chunks_created"] = int(ranges["gpu"].shape[0])
    res["anchor_step_30"]["same_ranges_and_world"] = bool(np.array_equal(ranges["gpu"], ranges["cpu16"]) and
                                                          same_world(worlds["gpu"], worlds["cpu16"]))
    regs = {k: v for k, v in _ffi.kernel_registers().items() if "gen_" in k}
    res["kernel_registers"] = regs or None
    line = json.dumps(res)
    print(line)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(line + "\n")
    gpu.close()


if __name__ == "__main__":
    main()
