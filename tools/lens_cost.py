"""What camera sampling (vrt_set_camera_sampling, include/vrt.h) costs a path-traced frame: C4 (1920x1080, 8^3 chunks, 4-bounce
diffuse path trace) at 1 and 4 spp, one frame in flight, with the setting off, with jitter alone (pixel_spread 1) and with the
lens (aperture 0.25, focus 32), in microseconds per frame.  Beside them the same frames at max_ray_bounces 1 — a frame that is
its primary launch alone (at 4 spp: one launch of a chain of four samples, and the pass that adds their planes) — which is the
time of the old primary kernel (off) and of the new one (on).  No threshold is fixed in advance.  The yardstick for a frame with
the setting on is the off frame plus one primary-only frame of the off kind per extra primary march: one at 1 spp (the centre
ray), four at 4 spp (the off frame marches one primary ray for its four samples, the on frame the centre ray and four).

    python tools/lens_cost.py [out.txt] [--runs N]

A run is a process of its own (this file again, with --worker): one context, every leg in turn, round after round, so that the
legs of a process see the same device in the same state; a leg is `FRAMES` back-to-back frames between two synchronisations and
a process's figure the median over its rounds.  Across processes: the median of the runs' figures and their spread (max - min,
in per cent of the median).  docs/MEASUREMENT.md has the rules.  Writes profiles/lens_cost.txt (or the path given as the first
argument) and prints it."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, ROUNDS, WARM = 60, 5, 10
SETTINGS = {"off": (0.0, 0.0, 0.0), "jitter": (1.0, 0.0, 0.0), "lens": (0.0, 0.25, 32.0)}
SPPS = (1, 4)
BOUNCES = (4, 1)   # the frame; its primary launch alone


def leg(gpu, spp, frames):
    from voxelraytracing_amd import MODE_PATH
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        gpu.render(MODE_PATH, spp=spp, seed=1)
    gpu.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def worker():
    """One process: {"bounces/spp/setting": median us per frame} as a JSON line."""
    from voxelraytracing_amd import Gpu, scenes
    sc = scenes.c4()
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    gpu.write_cam_data(sc.cam)
    times = {}
    for r in range(ROUNDS + 1):   # (round 0 warms every leg's kernels and buffers up)
        for bounces in BOUNCES:
            s = copy.copy(sc.settings)
            s.max_ray_bounces = bounces
            gpu.write_settings(s)
            for spp in SPPS:
                for name, setting in SETTINGS.items():
                    gpu.set_camera_sampling(*setting)
                    t = leg(gpu, spp, WARM if r == 0 else FRAMES)
                    if r:
                        times.setdefault(f"{bounces}/{spp}/{name}", []).append(t)
    gpu.close()
    print("LENS_COST " + json.dumps({k: statistics.median(v) for k, v in times.items()}))


def run():
    env = dict(os.environ)
    for k in ("VRT_PATH_POOL", "VRT_PATH_CELLS", "VRT_MARCH_DIRECT_MAX_S", "VRT_PATH_SAMPLES_PER_CHAIN"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"a measuring process failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("LENS_COST "))[len("LENS_COST "):])


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) * 100.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "lens_cost.txt"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker()
        return
    runs = [run() for _ in range(a.runs)]
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    spr = {k: spread([r[k] for r in runs]) for k in runs[0]}
    lines = ["# tools/lens_cost.py: C4 1920x1080 8^3, one device, one frame in flight; us per frame: the median of %d processes, each the median of "
             "%d legs of %d frames; (spread: max - min over the processes)" % (a.runs, ROUNDS, FRAMES)]
    for spp in SPPS:
        def cell(bounces, name):
            k = f"{bounces}/{spp}/{name}"
            return f"{name} {med[k]:8.1f} us ({spr[k]:.2f} %)"
        lines.append(f"{spp} spp, 4 bounces:           " + "   ".join(cell(4, n) for n in SETTINGS))
        lines.append(f"{spp} spp, primary launch only: " + "   ".join(cell(1, n) for n in SETTINGS) + "   (off: the old primary kernel; on: the new one)")
        extra = 1 if spp == 1 else spp
        yard = med[f"4/{spp}/off"] + extra * med[f"1/1/off"]
        for n in ("jitter", "lens"):
            on = med[f"4/{spp}/{n}"]
            over = on - yard
            lines.append(f"{spp} spp, {n}: yardstick = off frame + {extra} x the 1-spp primary-only frame = {yard:.1f} us; frame / yardstick = {on / yard:.4f} "
                         f"({over:+.1f} us; the new primary launch alone: {med[f'1/{spp}/{n}']:.1f} us)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
