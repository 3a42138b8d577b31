"""What exposure and tone mapping (vrt_set_tone_map, include/vrt.h) cost: C4 (1920x1080, 8^3 chunks, 4-bounce diffuse path trace,
1 spp), one frame at a time, with the setting off, with FILMIC at a manual exposure and with FILMIC + VRT_TONE_AUTO — the frame's
GPU time between its own events (VRT_RENDER_TIMED: the metering is inside it) — and the 1:1 blit of such a frame alone, mapped
against unmapped (vrt_present_device back to back over one frame, a host clock around calls that end in a synchronise).

    python tools/tone_cost.py [out.txt] [--parent-lib libvrt_parent.so]
    python tools/tone_cost.py --leg off|filmic|auto                     (one process' figures, as a JSON line)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/tone_cost.py --leg trace   (a run of its own)
    python tools/tone_cost.py [out.txt] --kernel-stats kernel_stats.csv     (... folded into the report)

Every figure is taken in a fresh process, three of each, the settings in turn; --parent-lib: another build of the library (the
parent commit's, which has no such entry points) in the same rotation, for the unmapped frame and blit.  The trace leg is the
metered frame with one pass of the denoiser in front, so that the trace holds the denoiser's guide launch beside the metering
kernels and the mapped blits.  Writes
profiles/tone_cost.txt (or the path given first) and prints it."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, WARM, BLITS, RUNS = 300, 60, 2000, 3
NEW_SYMBOLS = "vrt_set_tone_map,vrt_get_tone_info,vrt_read_tone_histogram"


def leg(mode):
    from voxelraytracing_amd import Gpu, MODE_PATH, _ffi, scenes
    sc = scenes.c4()
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    gpu.write_cam_data(sc.cam)
    gpu.write_settings(sc.settings)
    gpu.set_frames_in_flight(1)
    if mode == "filmic":
        gpu.set_tone_map(curve=_ffi.TONE_FILMIC, exposure=0.5)
    elif mode in ("auto", "trace"):
        gpu.set_tone_map(curve=_ffi.TONE_FILMIC, auto=True, adapt=0.25)
    if mode == "trace":
        gpu.set_denoise(1, 0.0)
    for _ in range(WARM):
        gpu.render(MODE_PATH, spp=1, seed=1, timed=True)
    gpu.stats()   # (folds the warm-up's events away)
    t0 = time.perf_counter()
    for _ in range(FRAMES):
        gpu.render(MODE_PATH, spp=1, seed=1, timed=True)
    gpu.synchronize()
    wall = (time.perf_counter() - t0) / FRAMES * 1e6
    s = gpu.stats()
    out = {"mode": mode, "frame_gpu_us": s.sum_ms_total / s.frames * 1e3, "frame_wall_us": wall, "timed_frames": s.frames}
    for name, style in (("blit_plain_us", 0), ("blit_crosshair_us", 2)):
        for n in (200, BLITS):   # (the first round warms the kernel up)
            gpu.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                gpu.present_device(style=style)
            gpu.synchronize()
            out[name] = (time.perf_counter() - t0) / n * 1e6
    if mode in ("auto", "trace"):
        info = gpu.tone_info()
        out["exposure"], out["counted"], out["frames"] = info.exposure, info.counted, info.frames
    gpu.close()
    print(json.dumps(out))


def run(mode, lib=None):
    env = dict(os.environ)
    env.pop("VRT_LIB", None)
    env.pop("VRT_LIB_WITHOUT", None)
    if lib:
        env["VRT_LIB"] = os.path.abspath(lib)
        env["VRT_LIB_WITHOUT"] = NEW_SYMBOLS
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", mode], env=env, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def kernel_lines(path):
    import csv
    lines = ["kernel trace of the metered frame behind one denoiser pass, and of its blits (rocprofv3 --kernel-trace --stats, a run of its own); "
             f"the histogram kernel reads the frame once, {1920 * 1080 * 16 / 1e6:.1f} MB:"]
    for row in csv.DictReader(open(path)):
        name = row["Name"]
        if not any(k in name for k in ("tone_", "present_", "denoise_guide")):
            continue
        avg_us = float(row["AverageNs"]) / 1e3
        short = name.split("(")[0] if not name.startswith("void") else name.split("(")[0][5:]
        if "(anonymous namespace)::" in name:
            short = name.split("(anonymous namespace)::")[1].split("(")[0]
        note = f"   {1920 * 1080 * 16 / 1e6 / avg_us:5.2f} TB/s" if "tone_histogram" in name else ""
        lines.append(f"  {short:40s} {int(row['Calls']):6d} calls  {avg_us:8.2f} us each{note}")
    return lines


def main():
    args = sys.argv[1:]
    if "--leg" in args:
        return leg(args[args.index("--leg") + 1])
    stats = args[args.index("--kernel-stats") + 1] if "--kernel-stats" in args else None
    parent = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
    out = args[0] if args and not args[0].startswith("--") else os.path.join(ROOT, "profiles", "tone_cost.txt")
    legs = ([("parent, off", "off", parent)] if parent else []) + [("off", "off", None), ("FILMIC manual", "filmic", None), ("FILMIC + AUTO", "auto", None)]
    res = {name: [] for name, _, _ in legs}
    for _ in range(RUNS):
        for name, mode, lib in legs:
            res[name].append(run(mode, lib))

    def fig(name, key):
        v = [r[key] for r in res[name]]
        return statistics.median(v), min(v), max(v)

    lines = [f"# tools/tone_cost.py: vrt_set_tone_map on C4 (1920x1080, 8^3 chunks, 4 bounces, 1 spp), one device, one frame at a time; "
             f"{RUNS} fresh processes per setting, in turn: median (min..max)",
             f"# frame: GPU time between the frame's own events (VRT_RENDER_TIMED), mean of {FRAMES} frames; blit: vrt_present_device 1:1, "
             f"{BLITS} back to back, host clock / calls"]
    base = fig("off", "frame_gpu_us")[0]
    for name, _, _ in legs:
        m, lo, hi = fig(name, "frame_gpu_us")
        w = fig(name, "frame_wall_us")[0]
        lines.append(f"frame  {name:14s} {m:8.1f} us ({lo:.1f}..{hi:.1f})   {m - base:+7.1f} us against off   wall {w:8.1f} us/frame")
    for key, what in (("blit_plain_us", "no crosshair"), ("blit_crosshair_us", "default crosshair")):
        base = fig("off", key)[0]
        for name, _, _ in legs:
            m, lo, hi = fig(name, key)
            mapped = "unmapped" if name.endswith("off") else "mapped"
            lines.append(f"blit   {what:17s} {name:14s} {mapped:8s} {m:7.2f} us ({lo:.2f}..{hi:.2f})   {m - base:+6.2f} us against off")
    a = res["FILMIC + AUTO"][-1]
    lines.append(f"metered: {a['counted']} of {1920 * 1080} pixels counted, exposure {a['exposure']:.6g} after {a['frames']} frames")
    if parent:
        p, t = fig("parent, off", "frame_gpu_us"), fig("off", "frame_gpu_us")
        where = "above" if t[0] > p[2] else ("below" if t[0] < p[1] else "inside")
        lines.append(f"off against the parent build: {(t[0] / p[0] - 1.0) * 100.0:+.2f} % on the frame, this build's median {where} the parent's spread")
    if stats:
        lines += kernel_lines(stats)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
