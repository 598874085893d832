// Host driver of what vpt_set_environment does before a byte reaches the device (vulkan-path-tracer_amd/csrc/scene_prep.hpp
// check_environment / env_tables / env_is_black) for tests/test_environment_cpu.py, in the layouts oracle/oracle_py.py returns the oracle's
// own tables in.  Built as a shared library with g++ (no HIP runtime is linked or called) and driven through ctypes.
#include <cstdint>
#include <vector>

#include "scene_prep.hpp"

using namespace vpt;

extern "C" {

// (rgba may be any non-NULL address for the rows that are rejected: check_environment never reads the texels)
const char* env_check(const float* rgba, uint32_t w, uint32_t h, int* code) {
    const scene::Verdict v = scene::check_environment(rgba, w, h);
    *code = v.code;
    return v.msg;
}
// orc_get_env_tables, plus the finished RGBA (alpha = pdf) the device is given; returns env_black
int env_tables(const float* rgba, uint32_t w, uint32_t h, uint32_t* alias_out, float* importance_out, float* pdf_out, float* rgba_out) {
    std::vector<float> env;
    std::vector<AliasEntry> alias;
    scene::env_tables(rgba, w, h, env, alias);
    for (size_t i = 0; i < alias.size(); i++) { alias_out[i] = alias[i].alias; importance_out[i] = alias[i].importance; pdf_out[i] = env[i * 4 + 3]; }
    for (size_t i = 0; i < env.size(); i++) rgba_out[i] = env[i];
    return scene::env_is_black(env) ? 1 : 0;
}

}  // extern "C"
