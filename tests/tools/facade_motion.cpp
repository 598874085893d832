// A small host of the C++ facade (vulkan-path-tracer_amd/host) for tests/test_gpu_motion.py: the animated-viewport loop with the facade's members — PathTrace +
// TemporalAccumulate, SetTemporalOptions(instance_motion = 1) before them, then one instance moved by SetInstanceTransforms and the seed changed by SetBaseSeed
// (the history survives both), PathTrace + TemporalAccumulate again.  The second temporal image, its motion image and the camera go to files.
//   facade_motion SCENE.gltf LUTS W H SPP DEPTH SEED INSTANCE M0 .. M15 TEMPORAL_OUT MOTION_OUT CAMERA_OUT      (M: the instance's new matrix, column-major, as Mat4::m)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "FlyCamera.h"
#include "PathTracer.h"

using namespace vpthost;

static void write_floats(const char* path, const float* p, size_t n) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(p, 4, n, f) != n) throw std::runtime_error(std::string("cannot write ") + path);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 28) { fprintf(stderr, "usage: facade_motion SCENE LUTS W H SPP DEPTH SEED INSTANCE M0..M15 TEMPORAL MOTION CAMERA\n"); return 2; }
    try {
        const uint32_t w = (uint32_t)atoi(argv[3]), h = (uint32_t)atoi(argv[4]), spp = (uint32_t)atoi(argv[5]), depth = (uint32_t)atoi(argv[6]), seed = (uint32_t)atoi(argv[7]);
        const uint32_t instance = (uint32_t)atoi(argv[8]);
        Mat4 moved;
        for (int k = 0; k < 16; k++) moved.m[k] = strtof(argv[9 + k], nullptr);
        PathTracer pt = PathTracer::New(0, 0, 1);
        pt.SetLookupTablePath(argv[2]);
        pt.ResizeImage(w, h);
        bool refused = false;
        try { pt.SetTemporalOptions(PathTracer::DefaultTemporalOptions()); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) throw std::runtime_error("SetTemporalOptions before SetScene was not refused");
        pt.SetScene(std::string(argv[1]));
        FlyCamera cam(inverse(pt.GetCameraViewInverse()), inverse(pt.GetCameraProjectionInverse()));
        cam.SetAspectRatio((float)w / (float)h); cam.SetNearFar(0.1f, 100.0f);
        pt.SetCameraProjectionInverse(inverse(cam.GetProjectionMatrix()));
        pt.SetMaxDepth(depth); pt.SetMaxSamplesAccumulated(spp);
        if (pt.GetTemporalOptions().instance_motion != 0u) throw std::runtime_error("instance_motion is not off by default");
        vpt_temporal_options o = PathTracer::DefaultTemporalOptions();
        o.instance_motion = 1;
        pt.SetTemporalOptions(o);
        if (pt.GetTemporalOptions().instance_motion != 1u) throw std::runtime_error("GetTemporalOptions does not return what was set");
        float c[32];
        memcpy(c, pt.GetCameraViewInverse().m, 64); memcpy(c + 16, pt.GetCameraProjectionInverse().m, 64);
        while (!pt.PathTrace(64)) {}
        pt.TemporalAccumulate(PathTracer::DefaultTemporalParams(), false);
        pt.SetInstanceTransforms(instance, {moved});
        pt.SetBaseSeed(seed);
        while (!pt.PathTrace(64)) {}
        const std::vector<float> temporal = pt.TemporalAccumulate();
        const std::vector<float> motion = pt.GetTemporalMotion();
        if (temporal.size() != (size_t)w * h * 4 || motion.size() != (size_t)w * h * 2) throw std::runtime_error("wrong image size");
        write_floats(argv[25], temporal.data(), temporal.size());
        write_floats(argv[26], motion.data(), motion.size());
        write_floats(argv[27], c, 32);
    } catch (const std::exception& e) { fprintf(stderr, "facade_motion: %s\n", e.what()); return 1; }
    return 0;
}
