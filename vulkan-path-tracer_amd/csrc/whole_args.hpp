// whole_args.hpp — the arguments of the whole-path kernel (kernels_whole.hip k_whole) as ONE struct, and the types through which its loop reads them.
// The kernel takes a DeviceScene, a RenderParams and a PathState: several dozen pointers and scalars, most of them read at one place of the shade
// step.  Held in registers they stay live across both trace loops, and what does not fit the 106 scalar registers lives in VGPR lanes (232
// v_readlane / v_writelane in the PLAIN instantiation).  Instead the loop reads each word again where it is used, from the kernel's own argument
// segment: a scalar load that hits the scalar cache, a result in scalar registers, no LDS.  WholeArgs is that segment — a kernel whose only
// parameter is this struct has it at offset 0 — and the loop reads it through a pointer to the constant address space, from which the compiler
// also knows that the pointers it loads point to global memory.
// WholeScene / WholeParams are DeviceScene / RenderParams with what k_whole knows at compile time as constant members that hide the fields
// (STRICT, PLAIN and its black environment, one-sample frames), so the shared shader code (shade_core.hpp, shading.hpp, traverse.hpp), which
// reads `sc.all_plain`, `P.samples_per_frame`, ... through a template parameter as camera_ray<Cam> does, folds them.  They add no word: a
// DeviceScene in memory is read as a WholeScene.
// Compiled for the device and — by tests/tools/whole_uniforms_driver.cpp — for the host (tests/test_whole_uniforms_cpu.py).
#pragma once
#include <stddef.h>

#include "device_types.hpp"
#include "whole_deal.hpp"

namespace vpt {

struct WholeArgs {
    DeviceScene sc;
    RenderParams P;
    PathState ps;
    Counters* ctr;
    uint32_t n_slots, dispatch_base;
    uint32_t static_rounds, chunk_tiles;   // chunk_tiles: whole_refill.hpp Shape (bits 0-8) | kernels.hpp kWholeNarrowOff
};

// What a launch hands over: the arguments, and behind them the rectangle of the image outside which no camera ray can reach the scene, as
// camera_cull.hpp packs it (cull::Packed; both words cull::kAxisAll: every sample runs, launch index = slot).  With a rectangle the launch's
// indices run over the samples inside it alone (whole_deal.hpp: `deal`, a.n_slots counts those; the others get their zero frame sums in runs), and
// `culled` is what the launch adds to the closest-hit rays for the samples it never sees.  The kernel's one parameter is this struct, so a WholeArgs still lies at offset 0 of the
// argument segment.
struct WholeLaunch {
    WholeArgs a;
    uint32_t cull_x, cull_y;
    deal::Deal deal;
    unsigned long long culled;
};
static_assert(offsetof(WholeLaunch, a) == 0, "the loop reads the argument segment as a WholeArgs");

template <bool STRICT, bool PLAIN>
struct WholeScene : DeviceScene {
    static constexpr uint32_t strict_hits = STRICT ? 1u : 0u, all_plain = 0u;
};
template <bool STRICT>
struct WholeScene<STRICT, true> : DeviceScene {   // the PLAIN instantiation runs on scenes with an all-zero env map only (launch_whole)
    static constexpr uint32_t strict_hits = STRICT ? 1u : 0u, all_plain = 1u, env_black = 1u;
};
struct WholeParams : RenderParams {
    static constexpr uint32_t samples_per_frame = 1u;   // the planner gives k_whole one-sample frames only (path_plan.hpp whole_possible)
};
static_assert(sizeof(WholeScene<false, false>) == sizeof(DeviceScene) && sizeof(WholeScene<true, true>) == sizeof(DeviceScene) && sizeof(WholeParams) == sizeof(RenderParams),
              "the views add no word");

}  // namespace vpt
