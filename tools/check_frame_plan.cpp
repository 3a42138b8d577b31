// tools/check_frame_plan.cpp — vrt::plan_frame (voxelraytracing_amd/csrc/vrt_frame_plan.h: what kind of frame a vrt_render call is,
// decided once) against the predicates it replaced, as a program of its own under AddressSanitizer + UBSan.  old_frame() restates
// those predicates word for word, each beside the line of vrt_frames.hip / vrt_order.hip (as of the commit before the header,
// fcdc4a9) it was copied from; main() compares the two over the full product of the facts — 3 modes x 4 variants x 3 stats values
// x the flags x every boolean fact x 1 or 2 frames in flight x no tile or one — skipping what vrt_render refuses, by vrt_render's own
// tests in vrt_render's order.  Every (mode, variant) pair vrt_render accepts must have been compared.  It also holds the
// equality the two places that asked for the derived tables relied on: asked of the variant before the fallback to the octree
// walk, and accel_ok, is the same as asked of the variant after it, and accel_ok.
//
// The path-traced frame the same way: old_path_frame() restates launch_path_frame's decisions and its double loop word for word,
// each line beside its line of vrt_frames.hip as of the commit before plan_path (f9d6f41), with the launches replaced by a record
// of what they were given.  The branches of the window experiment (deleted with that commit's successor: a library without the
// experiment's hooks never took them) are left out.  new_path_frame() records vrt::plan_path + vrt::for_each_path_step the way
// the new launch_path_frame enqueues them.  The two must give the same launches in the same order with the same arguments and the
// same buffers, over the full product of the facts that can reach the function.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//       -static-libasan -static-libubsan -o /tmp/check_frame_plan tools/check_frame_plan.cpp && /tmp/check_frame_plan
// (the sanitizers' runtimes linked into the program: it then runs the same whatever else the process is made to load first)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>

#include "../voxelraytracing_amd/csrc/vrt_frame_plan.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n  %s\n", __FILE__, __LINE__, #x, g_case); std::exit(1); } } while (0)
static char g_case[256];

using vrt::FrameFacts;
using vrt::FramePlan;

static bool variant_supported(uint32_t variant) { return variant <= 3u; }   // vrt_kernels.hip:686

// vrt_render's refusals that depend on the facts, in its order
static bool refused(const FrameFacts &F) {
    if (F.mode > VRT_MODE_PATH) return true;                                                          // vrt_frames.hip:685
    if (F.mode == VRT_MODE_PATH && F.variant != 0) return true;                                       // :686
    if (F.stats > 2u) return true;                                                                    // :687
    if (F.stats == 2u && (F.mode != VRT_MODE_PRIMARY_SHADOW || (F.variant != 0u))) return true;       // :688
    if (!variant_supported(F.variant)) return true;                                                   // :690
    if ((F.flags & VRT_RENDER_ACCUMULATE) && F.mode != VRT_MODE_PATH) return true;                    // :694 (accum_frame_start, :328-329)
    if (F.compact && (F.mode == VRT_MODE_PATH || (F.variant != 0u && F.variant != 2u) || F.show_step_count)) return true;   // :705
    if (F.air_liquid && F.compact) return true;                                                       // :727-729
    return false;
}

// What the code decided, where it decided it
struct Old {
    uint32_t variant, march;
    bool asked_before, wants_after, kstats, chain, pipelined, path_set, fused, second_launch, one_launch_shadow, fuse_present, walks, lpt_kind,
        counters_cleared, path_frame, literal;
};
static Old old_frame(const FrameFacts &F) {
    Old o;
    uint32_t variant = F.variant;                                                                     // :723
    const bool air_liquid = F.air_liquid;                                                             // :726
    if (air_liquid) variant = 1u;                                                                     // :727, :730
    o.asked_before = variant == 0u || variant == 3u || (F.mode == VRT_MODE_PATH && !air_liquid);      // :732
    if (o.asked_before) {
        if (!F.accel_ok && (variant == 0u || variant == 3u)) variant = 2u;                            // :736
    }
    o.kstats = F.stats == 1u || F.show_step_count;                                                    // :740
    o.wants_after = variant == 0u || variant == 3u || (F.mode == VRT_MODE_PATH && !air_liquid);       // :758
    o.variant = variant;
    // pick_frame_set
    o.chain = F.mode == VRT_MODE_PRIMARY || (F.mode == VRT_MODE_PRIMARY_SHADOW && (variant == 0u || (variant == 2u && F.compact))) ||
              F.mode == VRT_MODE_PATH;                                                                // :258-259
    const bool own_streams = (F.flags & VRT_RENDER_OWN_STREAMS) != 0u;                                // :263
    o.pipelined = F.in_flight > 1u && o.chain && !o.kstats && (own_streams || (!F.caller_stream && !F.output_bound));   // :264
    o.path_set = F.mode == VRT_MODE_PATH;                                                             // :274
    // launch_march_frame (called with shadow = mode == VRT_MODE_PRIMARY_SHADOW, :875)
    const bool shadow = F.mode == VRT_MODE_PRIMARY_SHADOW;
    o.march = variant == 3u ? 0u : variant;                                                           // :488
    o.fused = shadow && (variant == 0u || (variant == 2u && F.compact));                              // :492 (and n_counts, :493)
    o.second_launch = shadow && !o.fused;                                                             // :498
    // vrt_render
    o.walks = variant == 1u || variant == 2u;                                                         // :807
    o.one_launch_shadow = F.mode == VRT_MODE_PRIMARY_SHADOW && (variant == 0u || (variant == 2u && F.compact));   // :819
    o.fuse_present = (F.mode == VRT_MODE_PRIMARY || o.one_launch_shadow) && F.tiles_local && F.present_fusable;   // :820
    o.counters_cleared = o.kstats || F.mode == VRT_MODE_PATH;                                         // :862
    o.path_frame = F.mode == VRT_MODE_PATH;                                                           // :865
    o.literal = air_liquid;                                                                           // :871, :873
    // tile_order_before_frame: what of `lpt` the kind of frame decides
    o.lpt_kind = (F.mode == VRT_MODE_PRIMARY_SHADOW || F.mode == VRT_MODE_PRIMARY) && variant == 0u && !o.kstats && F.stats == 0u;   // vrt_order.hip:52-53
    return o;
}

// ---- the path-traced frame ----
using vrt::PathFacts;
using vrt::PathPlan;
using vrt::PathStep;

enum Kind : int { kPrimary, kLaneBounce, kCellsBounce, kChainFinish, kResolve, kFinalDivide };
enum Where : int { kNowhere, kFrame, kContextSum, kPlanes };   // a buffer a finishing pass is given
// kind, sample, chain, seg_counts / seg_in / seg_clear (which of the three cursor sets), path_out / path_in (which of the two
// buffers), last_bounce, segments, pool batches, first, last, count, the sum, the mean (resolve: the texels it reads and leaves the mean in)
using Launch = std::tuple<int, uint32_t, uint32_t, int, int, int, int, int, uint32_t, uint32_t, uint32_t, bool, bool, uint32_t, int, int>;
struct PathRecord {
    std::vector<Launch> launches;
    bool acc_planes = false, accum_sum = false, out_is_planes = false, acc_set = false, zeroed = false;
    size_t cap = 0, path_buf = 0;
    uint32_t seg_cap = 0, acc_frames = 0, sample_base = 0, spp = 0, seed = 0, refill = 0;
    bool kstats = false, literal = false, emit = false, polish = false, translucent = false;   // what the trace's launchers are given
    bool operator==(const PathRecord &o) const {
        return launches == o.launches && acc_planes == o.acc_planes && accum_sum == o.accum_sum && out_is_planes == o.out_is_planes &&
               acc_set == o.acc_set && zeroed == o.zeroed && cap == o.cap && path_buf == o.path_buf && seg_cap == o.seg_cap &&
               acc_frames == o.acc_frames && sample_base == o.sample_base && spp == o.spp && seed == o.seed && refill == o.refill &&
               kstats == o.kstats && literal == o.literal && emit == o.emit && polish == o.polish && translucent == o.translucent;
    }
};
constexpr uint32_t kHitSegments = 256;   // vrt_device.h

static PathRecord old_path_frame(const PathFacts &F) {
    PathRecord r;
    const bool accum = F.accum;                                                                       // :323
    const uint32_t accum_from = F.accum ? F.accum_from : 0u;                                          // :323 (accum_frame_start: 0 unless accumulating, :309-310)
    const bool kstats = F.kstats, literal = F.literal;                                                // :324
    const uint32_t spp = F.spp, bounces = F.bounces;                                                  // :325
    const uint32_t samples = (spp > 1u && !kstats && !literal && F.has_grid && bounces > 0) ? (spp < F.path_samples ? spp : F.path_samples) : 1u;   // :330
    const bool planes = samples > 1u;                                                                 // :331
    const bool emit = F.emissive || F.polished || F.translucent;                                                       // :337 (vrt_write_polish and vrt_write_translucency, later: such a frame is an emissive frame to everything but the launchers)
    const bool own_sum = emit && !planes && !accum && spp > 1u && bounces > 0;                        // :338
    const uint32_t seg_cap = F.hit_seg_cap * samples;                                                 // :339
    const size_t cap = (size_t)kHitSegments * seg_cap;                                                // :340
    r.path_buf = (2 * 3) * cap;                                                                       // :343
    if (planes || own_sum) { r.acc_planes = true; r.acc_frames = samples; }                           // :344
    if (accum) r.accum_sum = true;                                                                    // :345-348
    const uint32_t accum_count = accum_from + spp;                                                    // :357
    r.seg_cap = seg_cap;                                                                              // :359, :369
    r.acc_set = planes;                                                                               // :360
    if (planes) r.out_is_planes = true;                                                               // :363
    r.cap = cap;                                                                                      // :367-368
    r.spp = spp;                                                                                      // :370
    r.seed = F.seed;                                                                                  // :371
    r.sample_base = accum ? accum_from : 0u;                                                          // :372
    const bool pool = !kstats && !literal && F.has_grid && bounces > 1 && F.path_pool;                // :375
    const bool cells = pool && F.has_cells && F.path_cells;                                           // :376
    r.kstats = kstats; r.literal = literal; r.emit = emit; r.polish = F.polished; r.translucent = F.translucent; r.refill = F.path_refill;   // :411, :418, :422
    if (bounces == 0) r.zeroed = true;                                                                // :395
    uint32_t g = 0;                                                                                   // :397
    for (uint32_t smp = 0; smp < spp && bounces > 0; smp += samples) {                                // :398
        const uint32_t chain = spp - smp < samples ? spp - smp : samples;                             // :400
        for (uint32_t b = 0; b < bounces; b++, g++) {                                                 // :401
            const int seg_counts = g % 3u, seg_in = (g + 2u) % 3u, seg_clear = (g + 1u) % 3u;         // :402-404
            const int path_out = g & 1u, path_in = (g + 1u) & 1u;                                     // :405-406
            uint32_t last_bounce = b + 1 == bounces;                                                  // :407
            if (b == 0) {                                                                             // :409
                r.launches.emplace_back(kPrimary, smp, chain, seg_counts, seg_in, seg_clear, path_out, path_in, last_bounce, 1u, 0u, false, false, 0u, kNowhere, kNowhere);   // :411
            } else if (cells) {                                                                       // :412
                const uint32_t segments = bounces - b;                                                // :415
                last_bounce = 1u;                                                                     // :416
                r.launches.emplace_back(kCellsBounce, smp, chain, seg_counts, seg_in, seg_clear, path_out, path_in, last_bounce, segments,
                                        F.path_pool_batches ? F.path_pool_batches : (F.in_flight > 1u ? 5u : 4u), false, false, 0u, kNowhere, kNowhere);   // :418
                b += segments - 1u;                                                                   // :420
            } else {
                r.launches.emplace_back(kLaneBounce, smp, chain, seg_counts, seg_in, seg_clear, path_out, path_in, last_bounce, 1u, 0u, false, false, 0u, kNowhere, kNowhere);   // :422
            }
        }
        if (planes) {                                                                                 // :428
            if (accum) r.launches.emplace_back(kChainFinish, smp, chain, -1, -1, -1, -1, -1, 0u, 0u, 0u, accum_from + smp == 0u, smp + chain >= spp, accum_count, kContextSum, kFrame);   // :429-430
            else r.launches.emplace_back(kChainFinish, smp, chain, -1, -1, -1, -1, -1, 0u, 0u, 0u, smp == 0u, smp + chain >= spp, spp, kFrame, kFrame);   // :431
        } else if (accum) {                                                                           // :433
            r.launches.emplace_back(kResolve, smp, chain, -1, -1, -1, -1, -1, 0u, 0u, 0u, accum_from + smp == 0u, smp + 1u >= spp, accum_count, kContextSum, kFrame);   // :434
        } else if (own_sum) {                                                                         // :436
            r.launches.emplace_back(kResolve, smp, chain, -1, -1, -1, -1, -1, 0u, 0u, 0u, smp == 0u, smp + 1u >= spp, spp, kPlanes, kFrame);   // :437
        }
    }
    if (bounces > 0 && spp > 1u && !planes && !accum && !own_sum)                                     // :443
        r.launches.emplace_back(kFinalDivide, 0u, 0u, -1, -1, -1, -1, -1, 0u, 0u, 0u, false, true, spp, kNowhere, kFrame);   // :444
    return r;
}

// plan_path + for_each_path_step, recorded as launch_path_frame (vrt_frames.hip) enqueues them
static PathRecord new_path_frame(const PathFacts &F) {
    PathRecord r;
    const PathPlan p = vrt::plan_path(F);
    r.path_buf = 6 * p.cap;
    if (p.needs_acc_planes) { r.acc_planes = true; r.acc_frames = p.samples; }
    r.accum_sum = p.needs_accum_sum;
    r.seg_cap = p.seg_cap; r.acc_set = p.planes; r.out_is_planes = p.planes; r.cap = p.cap;
    r.spp = p.spp; r.seed = p.seed; r.sample_base = p.sample_base;
    r.kstats = p.kstats; r.literal = p.literal; r.emit = p.emit; r.polish = p.polish; r.translucent = p.translucent; r.refill = p.refill;
    r.zeroed = p.zero_output;
    const int sum_chain = p.finish_into_accum ? kContextSum : kFrame, sum_resolve = p.finish_into_accum ? kContextSum : kPlanes;
    vrt::for_each_path_step(p, [&](const PathStep &s) {
        const uint32_t g = s.launch;
        switch (s.kind) {
            case vrt::kStepPrimary: case vrt::kStepLaneBounce: case vrt::kStepCellsBounce:
                r.launches.emplace_back(s.kind == vrt::kStepPrimary ? kPrimary : s.kind == vrt::kStepLaneBounce ? kLaneBounce : kCellsBounce, s.sample,
                                        s.chain, g % 3u, (g + 2u) % 3u, (g + 1u) % 3u, g & 1u, (g + 1u) & 1u, s.last_bounce ? 1u : 0u, s.segments,
                                        s.kind == vrt::kStepCellsBounce ? p.pool_batches : 0u, false, false, 0u, kNowhere, kNowhere);
                break;
            case vrt::kStepSunlitPrimary: case vrt::kStepSunlitBounce: case vrt::kStepSunRays:
                CHECK(!"a frame without vrt_set_sun_light has no sun-lit step");
                break;
            case vrt::kStepLampPrimary: case vrt::kStepLampBounce: case vrt::kStepLampRays:
                CHECK(!"a frame without vrt_set_lamp_light has no lamp-lit step");
                break;
            case vrt::kStepWaterPrimary: case vrt::kStepWaterBounce:
                CHECK(!"a frame without vrt_set_water_optics has no water step");
                break;
            case vrt::kStepChainFinish:
                r.launches.emplace_back(kChainFinish, s.sample, s.chain, -1, -1, -1, -1, -1, 0u, 0u, 0u, s.first, s.last, s.count, sum_chain, kFrame);
                break;
            case vrt::kStepResolve:
                r.launches.emplace_back(kResolve, s.sample, s.chain, -1, -1, -1, -1, -1, 0u, 0u, 0u, s.first, s.last, s.count, sum_resolve, kFrame);
                break;
            case vrt::kStepFinalDivide:
                r.launches.emplace_back(kFinalDivide, 0u, 0u, -1, -1, -1, -1, -1, 0u, 0u, 0u, false, true, s.count, kNowhere, kFrame);
                break;
        }
    });
    return r;
}

static void check_path_frames() {
    long compared = 0, launches = 0, skipped = 0;
    const uint32_t spps[] = {1, 2, 3, 4, 5, 16, 17}, per_chain[] = {1, 2, 4, 16}, batches[] = {0, 4, 5};
    const int accums[] = {-1, 0, 7};   // not accumulating; accumulating from 0 and from 7 samples
    for (uint32_t spp : spps)
    for (uint32_t bounces = 0; bounces <= 5; bounces++)
    for (uint32_t bits = 0; bits < 512; bits++)
    for (int accum : accums)
    for (uint32_t samples : per_chain)
    for (uint32_t kb : batches)
    for (uint32_t in_flight = 1; in_flight <= 2; in_flight++) {
        PathFacts F;
        F.spp = spp; F.seed = 11u; F.bounces = bounces;
        F.kstats = bits & 1u; F.literal = bits & 2u; F.has_grid = bits & 4u; F.has_cells = bits & 8u; F.emissive = bits & 16u;
        F.path_pool = bits & 32u; F.path_cells = bits & 64u; F.polished = bits & 128u; F.translucent = bits & 256u;
        F.march_direct = F.has_cells;   // (no decision reads it)
        F.accum = accum >= 0; F.accum_from = accum >= 0 ? (uint32_t)accum : 0u;
        F.path_samples = samples; F.path_pool_batches = kb; F.path_refill = 16u; F.in_flight = in_flight; F.hit_seg_cap = 512u;
        // what cannot reach the function: a literal frame is never handed the tables (vrt_frame_plan.h: asks_for_tables), and the
        // march cells come with the tables (vrt_render fills P.mblk inside the branch that fills P.grid)
        if ((F.literal && F.has_grid) || (F.has_cells && !F.has_grid)) { skipped++; continue; }
        std::snprintf(g_case, sizeof g_case, "path: spp %u bounces %u kstats %d literal %d grid %d cells %d emissive %d polished %d translucent %d pool %d path_cells %d accum %d "
                      "per chain %u batches %u in_flight %u", spp, bounces, F.kstats, F.literal, F.has_grid, F.has_cells, F.emissive, F.polished, F.translucent, F.path_pool,
                      F.path_cells, accum, samples, kb, in_flight);
        const PathRecord o = old_path_frame(F), n = new_path_frame(F);
        CHECK(o.launches.size() == n.launches.size());
        for (size_t i = 0; i < o.launches.size(); i++) CHECK(o.launches[i] == n.launches[i]);
        CHECK(o == n);
        compared++;
        launches += (long)o.launches.size();
    }
    std::printf("check_path_plan: ok (%ld frames compared, %ld launches, %ld unreachable)\n", compared, launches, skipped);
}

// vrt_set_sun_light: a sun-lit frame has no predecessor to be held to; what vrt_frames.hip and the kernels rely on is asked of
// the plan directly, over the same combinations of the facts.  (F.sun false is every frame above: the plan is what it was.)
static void check_sun_frames() {
    long frames = 0, launches = 0;
    const uint32_t spps[] = {1, 2, 3, 12, 17}, per_chain[] = {1, 4, 16};
    const int accums[] = {-1, 0, 7};
    for (uint32_t spp : spps)
    for (uint32_t bounces = 0; bounces <= 5; bounces++)
    for (uint32_t bits = 0; bits < 512; bits++)
    for (int accum : accums)
    for (uint32_t samples : per_chain) {
        PathFacts F;
        F.spp = spp; F.seed = 11u; F.bounces = bounces; F.sun = true;
        F.kstats = bits & 1u; F.literal = bits & 2u; F.has_grid = bits & 4u; F.has_cells = bits & 8u; F.emissive = bits & 16u;
        F.path_pool = bits & 32u; F.path_cells = bits & 64u; F.polished = bits & 128u; F.translucent = bits & 256u;
        F.march_direct = F.has_cells;
        F.accum = accum >= 0; F.accum_from = accum >= 0 ? (uint32_t)accum : 0u;
        F.path_samples = samples; F.hit_seg_cap = 512u;
        if ((F.literal && F.has_grid) || (F.has_cells && !F.has_grid)) continue;
        std::snprintf(g_case, sizeof g_case, "sun: spp %u bounces %u bits %u accum %d per chain %u", spp, bounces, bits, accum, samples);
        const PathPlan p = vrt::plan_path(F);
        PathFacts E = F;   // the same frame of an emissive context without the setting, on the lane route, one sample per chain
        E.sun = false; E.emissive = true; E.path_pool = false; E.path_samples = 1u;
        const PathPlan e = vrt::plan_path(E);
        CHECK(p.sun == (bounces > 0u) && p.emit == (p.sun || F.emissive || F.polished || F.translucent) && !p.cells && (p.samples == 1u || !p.sun) && (!p.planes || !p.sun));
        CHECK(p.sun_cells == (p.sun && !F.kstats && !F.literal && F.has_cells && F.path_cells));
        CHECK(p.polish == F.polished && p.translucent == F.translucent);
        if (!p.sun) continue;
        CHECK(p.finish == e.finish && p.own_sum == e.own_sum && p.seg_cap == e.seg_cap && p.cap == e.cap && p.divide_at_end == e.divide_at_end &&
              p.needs_acc_planes == e.needs_acc_planes && p.needs_accum_sum == e.needs_accum_sum && p.sample_base == e.sample_base &&
              p.accum_count == e.accum_count && p.finish_into_accum == e.finish_into_accum);
        // the launches: the emissive frame's, each trace launch in its sun-lit kind and followed by the launch over its sun rays
        std::vector<PathStep> ps, es;
        vrt::for_each_path_step(p, [&](const PathStep &s) { ps.push_back(s); });
        vrt::for_each_path_step(e, [&](const PathStep &s) { es.push_back(s); });
        size_t i = 0;
        for (const PathStep &s : es) {
            CHECK(i < ps.size());
            const PathStep &t = ps[i++];
            CHECK(t.sample == s.sample && t.chain == s.chain && t.launch == s.launch &&
                  t.segments == s.segments && t.last_bounce == s.last_bounce && t.first == s.first && t.last == s.last && t.count == s.count);
            if (s.kind == vrt::kStepPrimary || s.kind == vrt::kStepLaneBounce) {
                CHECK(t.kind == (s.kind == vrt::kStepPrimary ? vrt::kStepSunlitPrimary : vrt::kStepSunlitBounce) && vrt::traces_paths(t.kind));
                CHECK(i < ps.size() && ps[i].kind == vrt::kStepSunRays && ps[i].launch == t.launch && !vrt::traces_paths(ps[i].kind));
                i++;
            } else {
                CHECK(s.kind != vrt::kStepCellsBounce && t.kind == s.kind && !vrt::traces_paths(t.kind));
            }
        }
        CHECK(i == ps.size());
        frames++;
        launches += (long)ps.size();
    }
    std::printf("check_sun_plan: ok (%ld sun-lit frames, %ld launches)\n", frames, launches);
}

// vrt_set_camera_sampling: the setting changes which kernels a frame's bounce-0 launches are (plan.lens) and nothing else — the
// plan of a frame with it is the plan of the same frame without it, field for field and step for step, over the same
// combinations of the facts, sun-lit or not.  A frame of no bounces has no primary launch: the flag stays off there.
static void check_lens_frames() {
    long frames = 0, launches = 0;
    const uint32_t spps[] = {1, 2, 3, 12, 17}, per_chain[] = {1, 4, 16};
    const int accums[] = {-1, 0, 7};
    for (uint32_t spp : spps)
    for (uint32_t bounces = 0; bounces <= 5; bounces++)
    for (uint32_t bits = 0; bits < 1024; bits++)
    for (int accum : accums)
    for (uint32_t samples : per_chain) {
        PathFacts F;
        F.spp = spp; F.seed = 11u; F.bounces = bounces; F.camera_sampling = true;
        F.kstats = bits & 1u; F.literal = bits & 2u; F.has_grid = bits & 4u; F.has_cells = bits & 8u; F.emissive = bits & 16u;
        F.path_pool = bits & 32u; F.path_cells = bits & 64u; F.polished = bits & 128u; F.translucent = bits & 256u; F.sun = bits & 512u;
        F.march_direct = F.has_cells;
        F.accum = accum >= 0; F.accum_from = accum >= 0 ? (uint32_t)accum : 0u;
        F.path_samples = samples; F.hit_seg_cap = 512u;
        if ((F.literal && F.has_grid) || (F.has_cells && !F.has_grid)) continue;
        std::snprintf(g_case, sizeof g_case, "lens: spp %u bounces %u bits %u accum %d per chain %u", spp, bounces, bits, accum, samples);
        const PathPlan p = vrt::plan_path(F);
        PathFacts E = F;
        E.camera_sampling = false;
        const PathPlan e = vrt::plan_path(E);
        CHECK(p.lens == (bounces > 0u) && !e.lens);
        CHECK(p.spp == e.spp && p.seed == e.seed && p.bounces == e.bounces && p.kstats == e.kstats && p.literal == e.literal && p.emit == e.emit &&
              p.polish == e.polish && p.translucent == e.translucent && p.sun == e.sun && p.sun_cells == e.sun_cells && p.samples == e.samples &&
              p.planes == e.planes && p.own_sum == e.own_sum && p.cells == e.cells && p.seg_cap == e.seg_cap && p.cap == e.cap &&
              p.pool_batches == e.pool_batches && p.refill == e.refill && p.zero_output == e.zero_output && p.finish == e.finish &&
              p.finish_into_accum == e.finish_into_accum && p.divide_at_end == e.divide_at_end && p.needs_acc_planes == e.needs_acc_planes &&
              p.needs_accum_sum == e.needs_accum_sum && p.sample_base == e.sample_base && p.accum_count == e.accum_count);
        std::vector<PathStep> ps, es;
        vrt::for_each_path_step(p, [&](const PathStep &s) { ps.push_back(s); });
        vrt::for_each_path_step(e, [&](const PathStep &s) { es.push_back(s); });
        CHECK(ps.size() == es.size());
        uint32_t primaries = 0;
        for (size_t i = 0; i < ps.size() && i < es.size(); i++) {
            const PathStep &t = ps[i], &s = es[i];
            CHECK(t.kind == s.kind && t.sample == s.sample && t.chain == s.chain && t.launch == s.launch && t.segments == s.segments &&
                  t.last_bounce == s.last_bounce && t.first == s.first && t.last == s.last && t.count == s.count);
            primaries += t.kind == vrt::kStepPrimary || t.kind == vrt::kStepSunlitPrimary;
        }
        // one bounce-0 launch per chain — the launch of the chain that holds sample 0 is the one that marches the centre ray
        CHECK(primaries == (bounces ? (spp + p.samples - 1u) / p.samples : 0u));
        frames++;
        launches += (long)ps.size();
    }
    std::printf("check_lens_plan: ok (%ld frames with camera sampling, %ld launches)\n", frames, launches);
}

// vrt_set_lamp_light: a lamp-lit frame is planned like a sun-lit one — the same chains, launch numbers and finishing passes — with
// the lamp-lit kinds in the place of the sun-lit ones and a kStepLampRays behind each trace launch, behind its kStepSunRays when the
// frame is sun-lit too.  The kinds from before keep their values.
static void check_lamp_frames() {
    static_assert(vrt::kStepPrimary == 0 && vrt::kStepLaneBounce == 1 && vrt::kStepCellsBounce == 2 && vrt::kStepSunlitPrimary == 3 &&
                  vrt::kStepSunlitBounce == 4 && vrt::kStepSunRays == 5 && vrt::kStepChainFinish == 6 && vrt::kStepResolve == 7 &&
                  vrt::kStepFinalDivide == 8, "the step kinds from before vrt_set_lamp_light keep their values");
    long frames = 0, launches = 0;
    const uint32_t spps[] = {1, 2, 3, 12, 17}, per_chain[] = {1, 4, 16};
    const int accums[] = {-1, 0, 7};
    for (uint32_t spp : spps)
    for (uint32_t bounces = 0; bounces <= 5; bounces++)
    for (uint32_t bits = 0; bits < 2048; bits++)
    for (int accum : accums)
    for (uint32_t samples : per_chain) {
        PathFacts F;
        F.spp = spp; F.seed = 11u; F.bounces = bounces; F.lamp = true;
        F.kstats = bits & 1u; F.literal = bits & 2u; F.has_grid = bits & 4u; F.has_cells = bits & 8u; F.emissive = bits & 16u;
        F.path_pool = bits & 32u; F.path_cells = bits & 64u; F.polished = bits & 128u; F.translucent = bits & 256u;
        F.sun = bits & 512u; F.camera_sampling = bits & 1024u;
        F.march_direct = F.has_cells;
        F.accum = accum >= 0; F.accum_from = accum >= 0 ? (uint32_t)accum : 0u;
        F.path_samples = samples; F.hit_seg_cap = 512u;
        if ((F.literal && F.has_grid) || (F.has_cells && !F.has_grid)) continue;
        std::snprintf(g_case, sizeof g_case, "lamp: spp %u bounces %u bits %u accum %d per chain %u", spp, bounces, bits, accum, samples);
        const PathPlan p = vrt::plan_path(F);
        PathFacts E = F;   // the same frame with the lamps off and the sun on: the structure a lamp-lit frame takes
        E.lamp = false; E.sun = true;
        const PathPlan e = vrt::plan_path(E);
        CHECK(p.lamp == (bounces > 0u) && p.sun == (F.sun && bounces > 0u) && p.lens == (F.camera_sampling && bounces > 0u));
        CHECK(p.polish == F.polished && p.translucent == F.translucent);
        if (!p.lamp) continue;
        CHECK(p.emit && !p.cells && p.samples == 1u && !p.planes);
        CHECK(p.finish == e.finish && p.own_sum == e.own_sum && p.seg_cap == e.seg_cap && p.cap == e.cap && p.divide_at_end == e.divide_at_end &&
              p.needs_acc_planes == e.needs_acc_planes && p.needs_accum_sum == e.needs_accum_sum && p.sample_base == e.sample_base &&
              p.accum_count == e.accum_count && p.finish_into_accum == e.finish_into_accum);
        std::vector<PathStep> ps, es;
        vrt::for_each_path_step(p, [&](const PathStep &s) { ps.push_back(s); });
        vrt::for_each_path_step(e, [&](const PathStep &s) { es.push_back(s); });
        size_t i = 0;
        for (const PathStep &s : es) {
            if (s.kind == vrt::kStepSunRays) {   // (the sun's launch: only in a frame that is sun-lit too, checked below)
                continue;
            }
            CHECK(i < ps.size());
            const PathStep &t = ps[i++];
            CHECK(t.sample == s.sample && t.chain == s.chain && t.launch == s.launch &&
                  t.segments == s.segments && t.last_bounce == s.last_bounce && t.first == s.first && t.last == s.last && t.count == s.count);
            if (s.kind == vrt::kStepSunlitPrimary || s.kind == vrt::kStepSunlitBounce) {
                CHECK(t.kind == (s.kind == vrt::kStepSunlitPrimary ? vrt::kStepLampPrimary : vrt::kStepLampBounce) && vrt::traces_paths(t.kind));
                if (p.sun) {
                    CHECK(i < ps.size() && ps[i].kind == vrt::kStepSunRays && ps[i].launch == t.launch);
                    i++;
                }
                CHECK(i < ps.size() && ps[i].kind == vrt::kStepLampRays && ps[i].launch == t.launch && !vrt::traces_paths(ps[i].kind));
                i++;
            } else {
                CHECK(t.kind == s.kind && !vrt::traces_paths(t.kind));
            }
        }
        CHECK(i == ps.size());
        frames++;
        launches += (long)ps.size();
    }
    std::printf("check_lamp_plan: ok (%ld lamp-lit frames, %ld launches)\n", frames, launches);
}

// vrt_set_water_optics: a water frame is planned like a sun-lit one — the same chains, launch numbers and finishing passes, no pool
// kernel, one sample per chain — with the water kinds in the place of the trace launches' and a kStepSunRays behind each only when
// the frame is sun-lit too.  The kinds from before keep their values.  (F.water false is every frame above: the plan is what it was.)
static void check_water_frames() {
    static_assert(vrt::kStepLampPrimary == 9 && vrt::kStepLampBounce == 10 && vrt::kStepLampRays == 11,
                  "the step kinds from before vrt_set_water_optics keep their values");
    long frames = 0, launches = 0;
    const uint32_t spps[] = {1, 2, 3, 12, 17}, per_chain[] = {1, 4, 16};
    const int accums[] = {-1, 0, 7};
    for (uint32_t spp : spps)
    for (uint32_t bounces = 0; bounces <= 5; bounces++)
    for (uint32_t bits = 0; bits < 1024; bits++)
    for (int accum : accums)
    for (uint32_t samples : per_chain) {
        PathFacts F;
        F.spp = spp; F.seed = 11u; F.bounces = bounces; F.water = true;
        F.kstats = bits & 1u; F.literal = bits & 2u; F.has_grid = bits & 4u; F.has_cells = bits & 8u; F.emissive = bits & 16u;
        F.path_pool = bits & 32u; F.path_cells = bits & 64u; F.polished = bits & 128u; F.translucent = bits & 256u; F.sun = bits & 512u;
        F.march_direct = F.has_cells;
        F.accum = accum >= 0; F.accum_from = accum >= 0 ? (uint32_t)accum : 0u;
        F.path_samples = samples; F.hit_seg_cap = 512u;
        if ((F.literal && F.has_grid) || (F.has_cells && !F.has_grid)) continue;
        std::snprintf(g_case, sizeof g_case, "water: spp %u bounces %u bits %u accum %d per chain %u", spp, bounces, bits, accum, samples);
        const PathPlan p = vrt::plan_path(F);
        PathFacts E = F;   // the same frame with the water off and the sun on: the structure a water frame takes
        E.water = false; E.sun = true;
        const PathPlan e = vrt::plan_path(E);
        PathFacts O = F;   // ... and with the water off: what the setting must not change when it is off
        O.water = false;
        const PathPlan o = vrt::plan_path(O);
        CHECK(!o.water && p.water == (bounces > 0u) && p.sun == (F.sun && bounces > 0u) && p.sun_cells == o.sun_cells && !p.lamp && !p.lens);
        CHECK(p.polish == F.polished && p.translucent == F.translucent);
        if (!p.water) continue;
        CHECK(p.emit && !p.cells && p.samples == 1u && !p.planes);
        CHECK(p.finish == e.finish && p.own_sum == e.own_sum && p.seg_cap == e.seg_cap && p.cap == e.cap && p.divide_at_end == e.divide_at_end &&
              p.needs_acc_planes == e.needs_acc_planes && p.needs_accum_sum == e.needs_accum_sum && p.sample_base == e.sample_base &&
              p.accum_count == e.accum_count && p.finish_into_accum == e.finish_into_accum);
        std::vector<PathStep> ps, es;
        vrt::for_each_path_step(p, [&](const PathStep &s) { ps.push_back(s); });
        vrt::for_each_path_step(e, [&](const PathStep &s) { es.push_back(s); });
        size_t i = 0;
        for (const PathStep &s : es) {
            if (s.kind == vrt::kStepSunRays) {   // (the sun's launch: only in a frame that is sun-lit too, checked below)
                continue;
            }
            CHECK(i < ps.size());
            const PathStep &t = ps[i++];
            CHECK(t.sample == s.sample && t.chain == s.chain && t.launch == s.launch &&
                  t.segments == s.segments && t.last_bounce == s.last_bounce && t.first == s.first && t.last == s.last && t.count == s.count);
            if (s.kind == vrt::kStepSunlitPrimary || s.kind == vrt::kStepSunlitBounce) {
                CHECK(t.kind == (s.kind == vrt::kStepSunlitPrimary ? vrt::kStepWaterPrimary : vrt::kStepWaterBounce) && vrt::traces_paths(t.kind));
                if (p.sun) {
                    CHECK(i < ps.size() && ps[i].kind == vrt::kStepSunRays && ps[i].launch == t.launch);
                    i++;
                }
            } else {
                CHECK(t.kind == s.kind && !vrt::traces_paths(t.kind));
            }
        }
        CHECK(i == ps.size());
        frames++;
        launches += (long)ps.size();
    }
    std::printf("check_water_plan: ok (%ld water frames, %ld launches)\n", frames, launches);
}

// vrt_set_haze: a haze frame is planned like a sun-lit one as well — the same chains, launch numbers and finishing passes, no pool
// kernel, one sample per chain — with the haze kinds in the place of the trace launches' and a kStepSunRays behind each only when
// the frame is sun-lit too; sun_cells is the sun-lit frame's.  The kinds from before keep their values.  haze = false leaves every
// plan what it was: every check above plans with F.haze false and still holds, against the loop plan_path replaced and against each
// setting's own structure; here a frame without a traced segment is the plan without the setting, field by field, and no plan with
// haze false has a haze step.
static bool same_plan(const PathPlan &a, const PathPlan &b) {
    return a.spp == b.spp && a.seed == b.seed && a.bounces == b.bounces && a.kstats == b.kstats && a.literal == b.literal && a.emit == b.emit &&
           a.polish == b.polish && a.translucent == b.translucent && a.sun == b.sun && a.sun_cells == b.sun_cells && a.lens == b.lens && a.lamp == b.lamp &&
           a.water == b.water && a.haze == b.haze && a.samples == b.samples && a.planes == b.planes && a.own_sum == b.own_sum && a.cells == b.cells &&
           a.seg_cap == b.seg_cap && a.cap == b.cap && a.pool_batches == b.pool_batches && a.refill == b.refill && a.zero_output == b.zero_output &&
           a.finish == b.finish && a.finish_into_accum == b.finish_into_accum && a.divide_at_end == b.divide_at_end &&
           a.needs_acc_planes == b.needs_acc_planes && a.needs_accum_sum == b.needs_accum_sum && a.sample_base == b.sample_base &&
           a.accum_count == b.accum_count;
}

static void check_haze_frames() {
    static_assert(vrt::kStepWaterPrimary == 12 && vrt::kStepWaterBounce == 13 && vrt::kStepHazePrimary == 14 && vrt::kStepHazeBounce == 15,
                  "the step kinds from before vrt_set_haze keep their values; the haze kinds are appended");
    long frames = 0, launches = 0;
    const uint32_t spps[] = {1, 2, 3, 12, 17}, per_chain[] = {1, 4, 16};
    const int accums[] = {-1, 0, 7};
    for (uint32_t spp : spps)
    for (uint32_t bounces = 0; bounces <= 5; bounces++)
    for (uint32_t bits = 0; bits < 1024; bits++)
    for (int accum : accums)
    for (uint32_t samples : per_chain) {
        PathFacts F;
        F.spp = spp; F.seed = 11u; F.bounces = bounces; F.haze = true;
        F.kstats = bits & 1u; F.literal = bits & 2u; F.has_grid = bits & 4u; F.has_cells = bits & 8u; F.emissive = bits & 16u;
        F.path_pool = bits & 32u; F.path_cells = bits & 64u; F.polished = bits & 128u; F.translucent = bits & 256u; F.sun = bits & 512u;
        F.march_direct = F.has_cells;
        F.accum = accum >= 0; F.accum_from = accum >= 0 ? (uint32_t)accum : 0u;
        F.path_samples = samples; F.hit_seg_cap = 512u;
        if ((F.literal && F.has_grid) || (F.has_cells && !F.has_grid)) continue;
        std::snprintf(g_case, sizeof g_case, "haze: spp %u bounces %u bits %u accum %d per chain %u", spp, bounces, bits, accum, samples);
        const PathPlan p = vrt::plan_path(F);
        PathFacts E = F;   // the same frame with the haze off and the sun on: the structure a haze frame takes
        E.haze = false; E.sun = true;
        const PathPlan e = vrt::plan_path(E);
        PathFacts O = F;   // ... and with the haze off: what the setting must not change when it is off
        O.haze = false;
        const PathPlan o = vrt::plan_path(O);
        CHECK(!o.haze && !e.haze && p.haze == (bounces > 0u) && p.sun == (F.sun && bounces > 0u) && p.sun == o.sun && p.sun_cells == o.sun_cells &&
              !p.lamp && !p.lens && !p.water);
        CHECK(p.polish == F.polished && p.translucent == F.translucent);
        if (!p.haze) {   // no segment is traced: the plan is the plan without the setting
            CHECK(same_plan(p, o));
            continue;
        }
        // off leaves the kinds of every other frame alone: a frame with haze off has no haze step
        {
            bool any = false;
            vrt::for_each_path_step(o, [&](const PathStep &s) { any = any || s.kind == vrt::kStepHazePrimary || s.kind == vrt::kStepHazeBounce; });
            CHECK(!any);
        }
        CHECK(p.emit && !p.cells && p.samples == 1u && !p.planes);
        CHECK(p.sun_cells == (p.sun && e.sun_cells));
        CHECK(p.finish == e.finish && p.own_sum == e.own_sum && p.seg_cap == e.seg_cap && p.cap == e.cap && p.divide_at_end == e.divide_at_end &&
              p.needs_acc_planes == e.needs_acc_planes && p.needs_accum_sum == e.needs_accum_sum && p.sample_base == e.sample_base &&
              p.accum_count == e.accum_count && p.finish_into_accum == e.finish_into_accum && p.zero_output == e.zero_output);
        std::vector<PathStep> ps, es;
        vrt::for_each_path_step(p, [&](const PathStep &s) { ps.push_back(s); });
        vrt::for_each_path_step(e, [&](const PathStep &s) { es.push_back(s); });
        size_t i = 0;
        for (const PathStep &s : es) {
            if (s.kind == vrt::kStepSunRays) {   // (the sun's launch: only in a frame that is sun-lit too, checked below)
                continue;
            }
            CHECK(i < ps.size());
            const PathStep &t = ps[i++];
            CHECK(t.sample == s.sample && t.chain == s.chain && t.launch == s.launch &&
                  t.segments == s.segments && t.last_bounce == s.last_bounce && t.first == s.first && t.last == s.last && t.count == s.count);
            if (s.kind == vrt::kStepSunlitPrimary || s.kind == vrt::kStepSunlitBounce) {
                CHECK(t.kind == (s.kind == vrt::kStepSunlitPrimary ? vrt::kStepHazePrimary : vrt::kStepHazeBounce) && vrt::traces_paths(t.kind));
                if (p.sun) {
                    CHECK(i < ps.size() && ps[i].kind == vrt::kStepSunRays && ps[i].launch == t.launch);
                    i++;
                }
            } else {
                CHECK(t.kind == s.kind && !vrt::traces_paths(t.kind));
            }
        }
        CHECK(i == ps.size());
        frames++;
        launches += (long)ps.size();
    }
    // haze = false, with every other setting: the plan does not read the field's neighbours differently (water, lamp and camera
    // sampling never meet haze = true: vrt_render refuses the pairs)
    for (uint32_t bits = 0; bits < 4096; bits++)
    for (uint32_t bounces = 0; bounces <= 3; bounces++) {
        PathFacts F;
        F.spp = 3u; F.bounces = bounces;
        F.kstats = bits & 1u; F.literal = bits & 2u; F.has_grid = bits & 4u; F.has_cells = bits & 8u; F.emissive = bits & 16u;
        F.path_pool = bits & 32u; F.path_cells = bits & 64u; F.polished = bits & 128u; F.translucent = bits & 256u; F.sun = bits & 512u;
        F.water = bits & 1024u; F.lamp = bits & 2048u;
        if ((F.literal && F.has_grid) || (F.has_cells && !F.has_grid) || (F.water && F.lamp)) continue;
        std::snprintf(g_case, sizeof g_case, "haze off: bounces %u bits %u", bounces, bits);
        const PathPlan p = vrt::plan_path(F);
        CHECK(!p.haze);
        vrt::for_each_path_step(p, [&](const PathStep &s) { CHECK(s.kind != vrt::kStepHazePrimary && s.kind != vrt::kStepHazeBounce); });
    }
    std::printf("check_haze_plan: ok (%ld haze frames, %ld launches)\n", frames, launches);
}

int main() {
    long compared[3][4] = {}, skipped = 0;
    const uint32_t flag_sets[4] = {0u, VRT_RENDER_OWN_STREAMS, VRT_RENDER_ACCUMULATE, VRT_RENDER_OWN_STREAMS | VRT_RENDER_ACCUMULATE};
    for (uint32_t mode = 0; mode < 3; mode++)
    for (uint32_t variant = 0; variant < 4; variant++)
    for (uint32_t stats = 0; stats < 3; stats++)
    for (uint32_t flags : flag_sets)
    for (uint32_t bits = 0; bits < 128; bits++)
    for (uint32_t in_flight = 1; in_flight <= 2; in_flight++)
    for (uint32_t tiles_local = 0; tiles_local <= 1; tiles_local++) {
        FrameFacts F;
        F.mode = mode; F.variant = variant; F.stats = stats; F.flags = flags;
        F.compact = bits & 1u; F.show_step_count = bits & 2u; F.air_liquid = bits & 4u; F.accel_ok = bits & 8u;
        F.caller_stream = bits & 16u; F.output_bound = bits & 32u; F.present_fusable = bits & 64u;
        F.in_flight = in_flight; F.tiles_local = tiles_local;
        std::snprintf(g_case, sizeof g_case, "mode %u variant %u stats %u flags %u compact %d step_count %d air_liquid %d accel_ok %d caller_stream %d "
                      "bound %d fusable %d in_flight %u tiles_local %u", mode, variant, stats, flags, F.compact, F.show_step_count, F.air_liquid,
                      F.accel_ok, F.caller_stream, F.output_bound, F.present_fusable, in_flight, tiles_local);
        // the one refusal that reads the plan's name for its test refuses what it refused
        if (F.compact)
            CHECK((F.mode == VRT_MODE_PATH || !vrt::one_launch_march(F.variant, F.compact) || F.show_step_count) ==
                  (F.mode == VRT_MODE_PATH || (F.variant != 0u && F.variant != 2u) || F.show_step_count));   // :705
        if (refused(F)) { skipped++; continue; }
        const Old o = old_frame(F);
        const FramePlan p = vrt::plan_frame(F);
        CHECK(vrt::asks_for_tables(F) == o.asked_before);
        // what the two places that asked relied on, and what every use of either made of it (:769, :770, :790)
        CHECK((o.asked_before && F.accel_ok) == (o.wants_after && F.accel_ok));
        CHECK(p.tables == (o.wants_after && F.accel_ok));
        CHECK(!(p.tables && F.air_liquid));   // (:790 also asked for !air_liquid: the tables are never asked for with it)
        CHECK(p.mode == F.mode && p.shadow == (F.mode == VRT_MODE_PRIMARY_SHADOW));
        CHECK(p.path == o.path_set && p.path == o.path_frame);
        CHECK(p.variant == o.variant);
        CHECK(p.kstats == o.kstats);
        CHECK(p.literal == o.literal);
        CHECK(p.may_pipeline == o.chain);
        CHECK(p.pipelined == o.pipelined);
        CHECK(p.fuse_present == o.fuse_present);
        CHECK(p.walks_octree == o.walks);
        CHECK((p.kstats || p.path) == o.counters_cleared);
        CHECK(p.orderable == o.lpt_kind);
        if (!p.path) {   // launch_march_frame
            CHECK(p.march == o.march);
            CHECK((p.shadow && p.one_launch) == o.fused);
            CHECK(!p.one_launch == o.second_launch);
            CHECK(p.counts_per_tile == o.fused);
            CHECK(p.one_launch == (F.mode == VRT_MODE_PRIMARY || o.one_launch_shadow));
        }
        compared[mode][variant]++;
    }
    long total = 0;
    for (uint32_t mode = 0; mode < 3; mode++)
        for (uint32_t variant = 0; variant < 4; variant++) {
            const bool accepted = mode != VRT_MODE_PATH || variant == 0u;
            std::snprintf(g_case, sizeof g_case, "mode %u variant %u: %ld compared", mode, variant, compared[mode][variant]);
            CHECK(accepted ? compared[mode][variant] > 0 : compared[mode][variant] == 0);
            total += compared[mode][variant];
            if (accepted) std::printf("  mode %u variant %u: %ld\n", mode, variant, compared[mode][variant]);
        }
    std::printf("check_frame_plan: ok (%ld frames compared, %ld refused)\n", total, skipped);
    check_path_frames();
    check_sun_frames();
    check_lamp_frames();
    check_lens_frames();
    check_water_frames();
    check_haze_frames();
    return 0;
}
