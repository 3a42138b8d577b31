// tools/check_frame_plan.cpp — vrt::plan_frame (voxelraytracing_amd/csrc/vrt_frame_plan.h: what kind of frame a vrt_render call is,
// decided once) against the predicates it replaced, as a program of its own under AddressSanitizer + UBSan.  old_frame() restates
// those predicates word for word, each beside the line of vrt_frames.hip / vrt_order.hip (as of the commit before the header,
// fcdc4a9) it was copied from; main() compares the two over the full product of the facts — 3 modes x 4 variants x 3 stats values
// x the flags x every boolean fact x 1 or 2 frames in flight x no tile or one — skipping what vrt_render refuses, by vrt_render's own
// tests in vrt_render's order.  Every (mode, variant) pair vrt_render accepts must have been compared.  It also holds the
// equality the two places that asked for the derived tables relied on: asked of the variant before the fallback to the octree
// walk, and accel_ok, is the same as asked of the variant after it, and accel_ok.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//       -static-libasan -static-libubsan -o /tmp/check_frame_plan tools/check_frame_plan.cpp && /tmp/check_frame_plan
// (the sanitizers' runtimes linked into the program: it then runs the same whatever else the process is made to load first)
#include <cstdint>
#include <cstdio>
#include <cstdlib>

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
    return 0;
}
