// camera.hpp — the camera ray of a sample (RayGen.slang:35-50) in its two forms: camera_ray<Cam>, the reference's statements, which every
// kernel but one calls with its RenderParams; and camera_ray(CameraBlock), the whole-path kernel's (kernels_whole.hip k_whole), which reads a
// per-block copy of the camera in LDS and leaves out what is the same for every sample of a launch.  Both give the same bits: origin,
// direction and the RNG state behind them.  Compiled for the device and — by tests/tools/whole_camera_driver.cpp — for the host, where
// tests/test_whole_camera_cpu.py holds one against the other.  All arithmetic goes through include/vpt_fp32.h and is compiled with
// -ffp-contract=off, so expression order here is part of the parity contract.
#pragma once
#include <stdint.h>

#include "../../include/vpt_fp32.h"

namespace vpt {
using namespace vptfp;

// Defines.slang:1-7 (as fp32)
#define VPT_PI 3.1415926535897F
#define VPT_2PI 6.2831853071795F
#define VPT_1_OVER_PI 0.3183098861837F

#if defined(__HIPCC__)
#define VPT_HD_MEMBER __host__ __device__ inline
#else
#define VPT_HD_MEMBER inline
#endif
struct Rng {  // Sampler.slang:21-43
    uint32_t s;
    VPT_HD_MEMBER float uf() { s = pcg_hash(s); return u32_to_unit(s); }
};
VPT_HD V4 v4(float x, float y, float z, float w) { V4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

VPT_HD V2 random_circle(Rng& r) {  // Sampler.slang:102-112
    float u1 = r.uf(), u2 = r.uf();
    float s, c; sincos_(2.0f * VPT_PI * u1, &s, &c);
    float rad = sqrt_(u2);
    V2 o; o.x = rad * c; o.y = rad * s; return o;
}

// Camera ray + AA jitter + DOF, RayGen.slang:35-50 (4 draws, the DOF pair always drawn).  Cam: anything with RenderParams' camera fields.
template <class Cam>
VPT_HD void camera_ray(const Cam& P, Rng& r, uint32_t x, uint32_t y, V3& origin, V3& direction) {
    float j0 = r.uf(), j1 = r.uf();
    float cx = ((float)x + 0.5f) + (j0 * (0.5f - -0.5f) + -0.5f);
    float cy = ((float)y + 0.5f) + (j1 * (0.5f - -0.5f) + -0.5f);
    float dx = (cx / (float)P.width) * 2.0f - 1.0f, dy = (cy / (float)P.height) * 2.0f - 1.0f;
    V4 o4 = mat_v4(P.view_inv, v4(0.0f, 0.0f, 0.0f, 1.0f));
    origin = v3(o4.x, o4.y, o4.z);
    V4 tg = mat_v4(P.proj_inv, v4(dx, dy, 1.0f, 1.0f));
    V3 tn = normalize(v3(tg.x, tg.y, tg.z));
    V4 dd = mat_v4(P.view_inv, v4(tn.x, tn.y, tn.z, 0.0f));
    direction = v3(dd.x, dd.y, dd.z);
    V3 focus = origin + direction * max_(P.focus_distance, 0.001f);
    V2 rc = random_circle(r);
    float rox = rc.x * 0.5f * P.dof_strength, roy = rc.y * 0.5f * P.dof_strength;
    V3 right = v3(P.view_inv[0], P.view_inv[1], P.view_inv[2]);
    V3 upv = v3(P.view_inv[4], P.view_inv[5], P.view_inv[6]);
    origin = origin + (rox * right + roy * upv);
    direction = normalize(focus - origin);
}

// camera_ray with its four draws handed in — the jitter pair and random_circle's point — instead of drawn: the same expressions in the same
// order, so with the integrator's draws it is the integrator's ray bit for bit, and with (0.5, 0.5) and (0, 0) it is the ray through the pixel centre
// with no lens offset.  k_first_hit (kernels_aux.hip) calls it, and temporal.hpp to find the world point of a pixel again: the integrators keep camera_ray.
template <class Cam>
VPT_HD void camera_ray_with(const Cam& P, float j0, float j1, V2 rc, uint32_t x, uint32_t y, V3& origin, V3& direction) {
    float cx = ((float)x + 0.5f) + (j0 * (0.5f - -0.5f) + -0.5f);
    float cy = ((float)y + 0.5f) + (j1 * (0.5f - -0.5f) + -0.5f);
    float dx = (cx / (float)P.width) * 2.0f - 1.0f, dy = (cy / (float)P.height) * 2.0f - 1.0f;
    V4 o4 = mat_v4(P.view_inv, v4(0.0f, 0.0f, 0.0f, 1.0f));
    origin = v3(o4.x, o4.y, o4.z);
    V4 tg = mat_v4(P.proj_inv, v4(dx, dy, 1.0f, 1.0f));
    V3 tn = normalize(v3(tg.x, tg.y, tg.z));
    V4 dd = mat_v4(P.view_inv, v4(tn.x, tn.y, tn.z, 0.0f));
    direction = v3(dd.x, dd.y, dd.z);
    V3 focus = origin + direction * max_(P.focus_distance, 0.001f);
    float rox = rc.x * 0.5f * P.dof_strength, roy = rc.y * 0.5f * P.dof_strength;
    V3 right = v3(P.view_inv[0], P.view_inv[1], P.view_inv[2]);
    V3 upv = v3(P.view_inv[4], P.view_inv[5], P.view_inv[6]);
    origin = origin + (rox * right + roy * upv);
    direction = normalize(focus - origin);
}

// ---- the whole-path kernel's camera
// What camera_ray reads of RenderParams — of the two matrices only rows 0-2: their rows 3 feed the .w that camera_ray drops — and, in that
// room, what is the same for every sample of a launch: the camera's position and whether the lens sample can move it.  No larger than the
// field-for-field copy it replaces (144 bytes): the kernel's static LDS decides how many blocks a CU holds (profiles/r14_whole_uniforms_ab.md).
constexpr uint32_t kCamLensOff = 1u;     // CameraBlock::flags: the lens sample leaves every origin as it is (lens_off)
struct CameraBlock {
    float view[12], proj[12];            // rows 0-2 of view_inv / proj_inv, column by column: m[col*3+row]
    float origin[3];                     // mul(view_inv, float4(0, 0, 0, 1)).xyz
    uint32_t flags;
    uint32_t width, height;
    float focus_distance, dof_strength;
};
static_assert(sizeof(CameraBlock) <= 144, "the camera block's LDS is part of k_whole's static bytes, which must not grow");

// mat_v4's .xyz on rows 0-2
VPT_HD V3 mat_rows3(const float* m, float x, float y, float z, float w) {
    return v3(((m[0] * x + m[3] * y) + m[6] * z) + m[9] * w,
              ((m[1] * x + m[4] * y) + m[7] * z) + m[10] * w,
              ((m[2] * x + m[5] * y) + m[8] * z) + m[11] * w);
}
VPT_HD bool finite_(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }
// True where camera_ray's lens statements change nothing but the RNG state.  With dof_strength +0 or -0 and a finite view_inv, rox * right +
// roy * upv is a zero of either sign in every component, and x + (+-0) is x bit for bit for every x but -0 (-0 + +0 is +0) — NaN payloads aside,
// which a finite origin does not have.
VPT_HD bool lens_off(const float* view_inv, V3 origin, float dof_strength) {
    bool ok = (f2u(dof_strength) & 0x7fffffffu) == 0u;
    for (int i = 0; i < 16; i++) ok = ok && finite_(view_inv[i]);
    return ok && finite_(origin.x) && finite_(origin.y) && finite_(origin.z) && f2u(origin.x) != 0x80000000u && f2u(origin.y) != 0x80000000u && f2u(origin.z) != 0x80000000u;
}
// Once per block.
VPT_HD void fill_camera_block(CameraBlock& C, const float* view_inv, const float* proj_inv, uint32_t width, uint32_t height, float focus_distance, float dof_strength) {
    for (int col = 0; col < 4; col++)
        for (int row = 0; row < 3; row++) { C.view[col * 3 + row] = view_inv[col * 4 + row]; C.proj[col * 3 + row] = proj_inv[col * 4 + row]; }
    const V4 o4 = mat_v4(view_inv, v4(0.0f, 0.0f, 0.0f, 1.0f));   // camera_ray's expression: the same bits
    C.origin[0] = o4.x; C.origin[1] = o4.y; C.origin[2] = o4.z;
    C.flags = lens_off(view_inv, v3(o4.x, o4.y, o4.z), dof_strength) ? kCamLensOff : 0u;
    C.width = width; C.height = height; C.focus_distance = focus_distance; C.dof_strength = dof_strength;
}
// A word of the block as the wave-uniform value it is: on the device an LDS load lands in a vector register, and a branch on it is only a
// scalar branch once the compiler has been told that all lanes hold the same.
VPT_HD uint32_t cam_uniform(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}
// camera_ray<Cam> on the block.  The origin is read, not multiplied out; and where the lens is off (a wave-uniform branch) the lens sample is
// its two draws alone.  focus and the closing normalize stay: their roundings count.
VPT_HD void camera_ray(const CameraBlock& C, Rng& r, uint32_t x, uint32_t y, V3& origin, V3& direction) {
    float j0 = r.uf(), j1 = r.uf();
    float cx = ((float)x + 0.5f) + (j0 * (0.5f - -0.5f) + -0.5f);
    float cy = ((float)y + 0.5f) + (j1 * (0.5f - -0.5f) + -0.5f);
    float dx = (cx / (float)C.width) * 2.0f - 1.0f, dy = (cy / (float)C.height) * 2.0f - 1.0f;
    origin = v3(C.origin[0], C.origin[1], C.origin[2]);
    V3 tn = normalize(mat_rows3(C.proj, dx, dy, 1.0f, 1.0f));
    direction = mat_rows3(C.view, tn.x, tn.y, tn.z, 0.0f);
    V3 focus = origin + direction * max_(C.focus_distance, 0.001f);
    if (cam_uniform(C.flags) & kCamLensOff) {
        r.s = pcg_hash(pcg_hash(r.s));   // random_circle's two draws
    } else {
        V2 rc = random_circle(r);
        float rox = rc.x * 0.5f * C.dof_strength, roy = rc.y * 0.5f * C.dof_strength;
        V3 right = v3(C.view[0], C.view[1], C.view[2]);
        V3 upv = v3(C.view[3], C.view[4], C.view[5]);
        origin = origin + (rox * right + roy * upv);
    }
    direction = normalize(focus - origin);
}

}  // namespace vpt
