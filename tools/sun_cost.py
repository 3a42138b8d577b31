"""What direct sunlight (vrt_set_sun_light, include/vrt.h) costs a path-traced frame: C4 (1920x1080, 8^3 chunks, 4-bounce
diffuse path trace, 1 spp) with 1 and 2 frames in flight, as a sun-lit frame (strength 1) and against two baselines of the same
build: the same frame with the setting off on the lane route (VRT_PATH_POOL=0: one lane = path launch per bounce, which is what
a sun-lit frame is planned onto) and on the default route (the pool kernel over the march cells).  No threshold is fixed in
advance.  What to read the sun-lit time against is the lane route's time scaled by (segments + sun rays) / segments: a sun ray is
one more march per hit that sees the sun, over the march cells without a brick load.  The ray counts are a stats frame's, not
the CPU reference's (a 1080p frame of it is minutes): vrt_stats.primary_rays — the primary rays marched, 64 per tile, hit or
not — and vrt_stats.secondary_rays with the setting on and off; tests/test_gpu_sun.py holds those counts to the reference's
at the sizes it runs.

    python tools/sun_cost.py [out.txt] [--runs N]

Every measurement is a process of its own (this file again, with --worker and the leg's environment), the legs' processes
alternating: N runs each.  Within a process a leg is `frames` back-to-back frames between two synchronisations, and a figure
is the median over the rounds.  Across processes: the median of the runs' figures, and their spread (max - min, in per cent of
the median).  docs/MEASUREMENT.md has the rules.  Writes profiles/sun_cost.txt (or the path given as the first argument) and
prints it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, ROUNDS, WARM = 200, 5, 40
# leg: (strength, environment)
LEGS = {"sun-lit": (1.0, {}), "off, lane route": (0.0, {"VRT_PATH_POOL": "0"}), "off, pool route": (0.0, {})}


def leg(gpu, frames):
    from voxelraytracing_amd import MODE_PATH
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        gpu.render(MODE_PATH, spp=1, seed=1)
    gpu.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def worker(strength):
    """One process: {"us": {in flight: median us per frame}, "primary": .., "secondary": ..} as a JSON line."""
    from voxelraytracing_amd import Gpu, MODE_PATH, scenes
    sc = scenes.c4()
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    gpu.write_cam_data(sc.cam)
    gpu.write_settings(sc.settings)
    gpu.set_sun_light(strength)
    gpu.render(MODE_PATH, spp=1, seed=1, stats=True)
    st = gpu.stats()
    out = {"us": {}, "primary": int(st.primary_rays), "secondary": int(st.secondary_rays)}
    for in_flight in (1, 2):
        gpu.set_frames_in_flight(in_flight)
        leg(gpu, WARM)
        out["us"][str(in_flight)] = statistics.median(leg(gpu, FRAMES) for _ in range(ROUNDS))
    gpu.close()
    print("SUN_COST " + json.dumps(out))


def run(name):
    strength, extra = LEGS[name]
    env = dict(os.environ)
    for k in ("VRT_PATH_POOL", "VRT_PATH_CELLS", "VRT_MARCH_DIRECT_MAX_S", "VRT_PATH_SAMPLES_PER_CHAIN"):
        env.pop(k, None)
    env.update(extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--strength", str(strength)], env=env, capture_output=True,
                       text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"a measuring process failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("SUN_COST "))[len("SUN_COST "):])


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) * 100.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "sun_cost.txt"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--strength", type=float, default=0.0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.strength)
        return
    res = {k: [] for k in LEGS}
    for _ in range(a.runs):
        for k in LEGS:
            res[k].append(run(k))
    on, off = res["sun-lit"][0], res["off, lane route"][0]
    segments = off["primary"] + off["secondary"]   # path segments marched: the primary rays and the bounce segments
    sun_rays = on["secondary"] - off["secondary"]
    scale = (segments + sun_rays) / segments
    lines = ["# tools/sun_cost.py: C4 1920x1080 8^3 4 bounces 1 spp, one device; us per frame: the median of %d processes, each the median of "
             "%d legs of %d frames; (spread: max - min over the processes)" % (a.runs, ROUNDS, FRAMES),
             f"rays of a frame (a stats frame's counts on the GPU, which tests/test_gpu_sun.py holds to the reference's at its sizes): {segments} path "
             f"segments marched, {sun_rays} sun rays: (segments + sun rays) / segments = {scale:.4f}"]
    for in_flight in ("1", "2"):
        med = {}
        parts = []
        for k in LEGS:
            v = [r["us"][in_flight] for r in res[k]]
            med[k] = statistics.median(v)
            parts.append(f"{k} {med[k]:8.1f} us (spread {spread(v):.2f} %)")
        lines.append(f"{in_flight} in flight:  " + "   ".join(parts))
        lines.append(f"{in_flight} in flight:  sun-lit / lane route = {med['sun-lit'] / med['off, lane route']:.4f} (expected from the ray counts: {scale:.4f}); "
                     f"sun-lit / pool route = {med['sun-lit'] / med['off, pool route']:.4f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
