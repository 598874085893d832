// Host driver of vulkan-path-tracer_amd/csrc/camera.hpp for tests/test_whole_camera_cpu.py: the camera ray of the whole-path kernel
// (kernels_whole.hip k_whole), which reads the camera's position from its per-block CameraBlock and, with the lens off, draws the lens sample
// without evaluating it, held against the general statements the other kernels run.  The arithmetic is the header's.  A stand-alone program
// (so that it can be built with sanitizers as it is):
//   whole_camera_driver <32 hex words: view_inv, proj_inv> <width> <height> <focus hex> <dof hex> <count> <seed>
// It prints one line of "key value" pairs and exits 1 if a ray differed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "camera.hpp"

using namespace vpt;

namespace {
struct Rand {   // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
};
struct Params {   // RenderParams' fields of this name
    float view_inv[16], proj_inv[16];
    uint32_t width, height;
    float focus_distance, dof_strength;
};

uint32_t hex32(const char* s) { return (uint32_t)std::strtoul(s, nullptr, 16); }
int run_camera(char** a) {
    Params P{};
    for (int i = 0; i < 16; i++) { P.view_inv[i] = u2f(hex32(a[i])); P.proj_inv[i] = u2f(hex32(a[16 + i])); }
    P.width = (uint32_t)std::atoi(a[32]); P.height = (uint32_t)std::atoi(a[33]);
    P.focus_distance = u2f(hex32(a[34])); P.dof_strength = u2f(hex32(a[35]));
    const uint32_t count = (uint32_t)std::atoi(a[36]);
    Rand rnd{std::strtoull(a[37], nullptr, 10)};
    CameraBlock cam;
    fill_camera_block(cam, P.view_inv, P.proj_inv, P.width, P.height, P.focus_distance, P.dof_strength);
    uint64_t wrong = 0;
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t x = (uint32_t)(rnd.next() % P.width), y = (uint32_t)(rnd.next() % P.height), seed = (uint32_t)rnd.next();
        Rng ra{seed}, rb{seed};
        V3 oa, da, ob, db;
        camera_ray(P, ra, x, y, oa, da);
        camera_ray(cam, rb, x, y, ob, db);
        const float va[6] = {oa.x, oa.y, oa.z, da.x, da.y, da.z}, vb[6] = {ob.x, ob.y, ob.z, db.x, db.y, db.z};
        if (std::memcmp(va, vb, sizeof va) != 0 || ra.s != rb.s) wrong++;
    }
    std::printf("lens_off %u origin %08x %08x %08x rays %u wrong %" PRIu64 "\n", cam.flags & kCamLensOff, f2u(cam.origin[0]), f2u(cam.origin[1]), f2u(cam.origin[2]), count, wrong);
    return wrong == 0 ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 39) return run_camera(argv + 1);
    std::fprintf(stderr, "usage: see the head of whole_camera_driver.cpp\n");
    return 2;
}
