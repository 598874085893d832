// Host driver of vulkan-path-tracer_amd/csrc/whole_args.hpp for tests/test_whole_uniforms_cpu.py.  The whole-path kernel (kernels_whole.hip k_whole)
// reads its arguments where it uses them, as a WholeArgs in its argument segment, and reads the scene and the parameters in it through the views
// WholeScene<STRICT, PLAIN> and WholeParams.  wu_check fills a WholeArgs in which every word differs from every other and compares, for the four
// (STRICT, PLAIN) forms the kernel is instantiated with: every field the loop reads, through the view, with the struct's own field; the constant
// members with what k_whole used to write into its copy; and where the members of WholeArgs lie with where a kernel's arguments of those types
// lie (each at the next multiple of its alignment).  It returns how many comparisons fail (their names in `msg`).  With -DWU_MAIN a stand-alone
// program over the same checks (the sanitizer build).
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "whole_args.hpp"

using namespace vpt;

namespace {
// every 4-byte word of the object gets its own value: floats become distinct finite numbers, pointers distinct (never followed) addresses
template <class T>
void fill_distinct(T& t, uint32_t base) {
    uint32_t w[(sizeof(T) + 3) / 4];
    for (size_t i = 0; i < sizeof(w) / 4; i++) w[i] = 0x3f000000u + base + (uint32_t)i * 8u;
    std::memcpy((void*)&t, w, sizeof(T));
}
struct Tally {
    int bad = 0, fields = 0;
    std::string names;
    template <class A, class B>
    void eq(const char* name, const A& a, const B& b) {
        fields++;
        if (!(a == b)) { bad++; names += name; names += ' '; }
    }
};
#define SAME(view, src, f) t.eq(#src "." #f, view.f, src.f)

template <bool STRICT, bool PLAIN>
void check(bool emissive, uint32_t dispatch_base, Tally& t) {
    WholeArgs a;
    fill_distinct(a, 0x1000u);
    a.dispatch_base = dispatch_base;
    DeviceScene& sc = a.sc;
    if (emissive) { sc.emissive_count = 3u; sc.emissive_tris = 17u; }
    else {   // a scene without emissive meshes: no light tables at all
        sc.emissive_count = 0u; sc.emissive_tris = 0u;
        sc.emissive = nullptr; sc.emissive_tri = nullptr; sc.emissive_tri_offset = nullptr; sc.lights = nullptr;
    }
    const RenderParams& P = a.P;
    const WholeScene<STRICT, PLAIN>& vs = static_cast<const WholeScene<STRICT, PLAIN>&>(a.sc);
    const WholeParams& vp = static_cast<const WholeParams&>(a.P);
    // the scene words of the shade and trace steps
    SAME(vs, sc, instances); SAME(vs, sc, materials); SAME(vs, sc, mat_resolved); SAME(vs, sc, tri_shade); SAME(vs, sc, texels);
    SAME(vs, sc, emissive); SAME(vs, sc, emissive_tri); SAME(vs, sc, emissive_tri_offset); SAME(vs, sc, lights); SAME(vs, sc, tri_slot_of_gid);
    SAME(vs, sc, lut_r); SAME(vs, sc, lut_o); SAME(vs, sc, lut_i); SAME(vs, sc, env); SAME(vs, sc, alias);
    SAME(vs, sc, emissive_count); SAME(vs, sc, env_w); SAME(vs, sc, env_h); SAME(vs, sc, scene_extent);
    // what k_whole used to write into its own copy of sc and P
    t.eq("sc.strict_hits", (uint32_t)vs.strict_hits, STRICT ? 1u : 0u);
    t.eq("sc.all_plain", (uint32_t)vs.all_plain, PLAIN ? 1u : 0u);
    if (PLAIN) t.eq("sc.env_black", (uint32_t)vs.env_black, 1u);
    else SAME(vs, sc, env_black);
    t.eq("P.samples_per_frame", (uint32_t)vp.samples_per_frame, 1u);
    // the parameters of the shade step's tail, the miss shader and the refill step
    SAME(vp, P, width); SAME(vp, P, shard_rank); SAME(vp, P, shard_count); SAME(vp, P, shard_pixels);
    SAME(vp, P, max_depth); SAME(vp, P, split); SAME(vp, P, flags); SAME(vp, P, base_seed); SAME(vp, P, launch_off); SAME(vp, P, dispatch_base_dev);
    SAME(vp, P, max_luminance); SAME(vp, P, sky_intensity); SAME(vp, P, emissive_pdf_bias);
    for (int i = 0; i < 8; i++) t.eq("P.sky_rot", vp.sky_rot[i], P.sky_rot[i]);
    t.eq("dispatch_base", a.dispatch_base, dispatch_base);
    // a kernel's arguments lie one behind the other, each at the next multiple of its alignment
    size_t at = 0;
    auto next = [&](size_t size, size_t align) { at = (at + align - 1) / align * align; const size_t here = at; at += size; return here; };
    t.eq("offset sc", offsetof(WholeArgs, sc), next(sizeof(DeviceScene), alignof(DeviceScene)));
    t.eq("offset P", offsetof(WholeArgs, P), next(sizeof(RenderParams), alignof(RenderParams)));
    t.eq("offset ps", offsetof(WholeArgs, ps), next(sizeof(PathState), alignof(PathState)));
    t.eq("offset ctr", offsetof(WholeArgs, ctr), next(sizeof(Counters*), alignof(Counters*)));
    t.eq("offset n_slots", offsetof(WholeArgs, n_slots), next(4, 4));
    t.eq("offset dispatch_base", offsetof(WholeArgs, dispatch_base), next(4, 4));
    t.eq("offset static_rounds", offsetof(WholeArgs, static_rounds), next(4, 4));
    t.eq("offset chunk_tiles", offsetof(WholeArgs, chunk_tiles), next(4, 4));
    t.eq("size", sizeof(WholeArgs), (at + 7) / 8 * 8);
}
}  // namespace

extern "C" int wu_check(int emissive, uint32_t dispatch_base, int* fields, char* msg, int msg_len) {
    Tally t;
    check<false, false>(emissive != 0, dispatch_base, t);
    check<false, true>(emissive != 0, dispatch_base, t);
    check<true, false>(emissive != 0, dispatch_base, t);
    check<true, true>(emissive != 0, dispatch_base, t);
    *fields = t.fields;
    std::snprintf(msg, (size_t)msg_len, "%s", t.names.c_str());
    return t.bad;
}

#ifdef WU_MAIN
int main() {
    int bad = 0, fields = 0;
    char msg[4096];
    for (int emissive = 0; emissive < 2; emissive++)
        for (uint32_t base : {0u, 7u, 0xfffffff0u}) bad += wu_check(emissive, base, &fields, msg, (int)sizeof(msg));
    std::printf("comparisons %d, differing %d %s\n", fields, bad, bad ? msg : "");
    return bad ? 1 : 0;
}
#endif
