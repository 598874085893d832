// box_entry_dir_host — the sign-directed slab test of an fp32 box (vulkan-path-tracer_amd/csrc/slab.hpp box_entry_dir: the function the LDS-tree node step
// calls) against the form it replaces, compiled for the host with -ffp-contract=off.  Per case the planes are picked as traverse.hpp make_slab /
// load_node pick them (near = the max plane where inv < 0, else the min plane) and the result is compared BIT FOR BIT with box_entry_fma on the
// stored planes — in the fma form (oi = o * inv, rays slab_fma_ok admits) and in the subtract form (planes moved to the origin, oi = 0, every ray),
// each case in the form(s) its ray may take.  Shared library for tests/test_box_entry_dir_cpu.py; with -DBED_MAIN a stand-alone program over a
// generator of its own (what a sanitizer build runs).  Test utility only; nothing in the product links it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../vulkan-path-tracer_amd/csrc/slab.hpp"
using namespace vpt;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

struct Pick { float nx, ny, nz, fx, fy, fz; };
static Pick pick(const float* p, V3 inv) {   // p = {lo.xyz, hi.xyz}
    Pick k;
    k.nx = inv.x < 0.0f ? p[3] : p[0]; k.fx = inv.x < 0.0f ? p[0] : p[3];
    k.ny = inv.y < 0.0f ? p[4] : p[1]; k.fy = inv.y < 0.0f ? p[1] : p[4];
    k.nz = inv.z < 0.0f ? p[5] : p[2]; k.fz = inv.z < 0.0f ? p[2] : p[5];
    return k;
}

extern "C" {

float bed_miss_t() { return kMissT; }

// n cases.  o, d: n x 3; box: n x 6 {lo.xyz, hi.xyz} as a node stores them; extent: n (slab_fma_ok's reach = kSlabFmaReach * extent); range: n x 2 {tmin, tlimit}.
// Out per case: form (bit 0: the fma form ran, i.e. the guard admits the ray; bit 1: the subtract form ran — always), and for each form that ran the
// two returned floats as bits (ref = box_entry_fma / box_entry on the stored planes, dir = box_entry_dir on the picked ones).
void bed_run(int64_t n, const float* o, const float* d, const float* box, const float* extent, const float* range,
             uint8_t* form, uint32_t* fma_ref, uint32_t* fma_dir, uint32_t* sub_ref, uint32_t* sub_dir) {
    for (int64_t i = 0; i < n; i++) {
        const float *oo = o + 3 * i, *dd = d + 3 * i, *p = box + 6 * i;
        const float tmin = range[2 * i], tlimit = range[2 * i + 1];
        const V3 O = vptfp::v3(oo[0], oo[1], oo[2]), inv = safe_inverse(vptfp::v3(dd[0], dd[1], dd[2])), oi = slab_oi(O, inv);
        const V3 zero = vptfp::v3(0.0f, 0.0f, 0.0f);
        const Pick k = pick(p, inv);
        form[i] = 2;
        fma_ref[i] = fma_dir[i] = 0u;
        if (slab_fma_ok(O, oi, kSlabFmaReach * extent[i])) {
            form[i] |= 1;
            fma_ref[i] = bits(box_entry_fma(p[0], p[1], p[2], p[3], p[4], p[5], oi, inv, tmin, tlimit));
            fma_dir[i] = bits(box_entry_dir(k.nx, k.ny, k.nz, k.fx, k.fy, k.fz, oi, inv, tmin, tlimit));
        }
        // traverse.hpp node_entries, !fused: the picked planes moved to the origin, then the same code with oi = 0
        sub_ref[i] = bits(box_entry(p[0], p[1], p[2], p[3], p[4], p[5], O, inv, tmin, tlimit));
        sub_dir[i] = bits(box_entry_dir(k.nx - O.x, k.ny - O.y, k.nz - O.z, k.fx - O.x, k.fy - O.y, k.fz - O.z, zero, inv, tmin, tlimit));
    }
}

}  // extern "C"

#ifdef BED_MAIN
// Stand-alone: a small generator of its own (xorshift; boxes fat, flat and unused, origins inside, on a plane and far out, directions general,
// +-0 and below safe_inverse's clamp) through bed_run; exit status 1 on any differing bit.
#include <vector>
static uint64_t s_rng = 0x9e3779b97f4a7c15ull;
static double rnd() { s_rng ^= s_rng << 13; s_rng ^= s_rng >> 7; s_rng ^= s_rng << 17; return (double)(s_rng >> 11) / 9007199254740992.0; }
int main() {
    const int64_t n = 400000;
    std::vector<float> o(3 * n), d(3 * n), box(6 * n), extent(n), range(2 * n);
    const float tiny[4] = {0.0f, -0.0f, 1.0e-35f, -3.0e-33f};
    for (int64_t i = 0; i < n; i++) {
        const float e = (float)(0.001 * (1.0 + 9999.0 * rnd()));
        extent[i] = e;
        const bool unused = rnd() < 0.1, aim = rnd() < 0.6;   // aim: towards a point of the box
        for (int a = 0; a < 3; a++) {
            const float lo = (float)((2.0 * rnd() - 1.0) * e), size = rnd() < 0.2 ? 0.0f : (float)(rnd() * e);
            box[6 * i + a] = unused ? 1.0e30f : lo; box[6 * i + 3 + a] = unused ? 1.0e30f : lo + size;
            const double place = rnd();
            o[3 * i + a] = place < 0.1 ? box[6 * i + a + (rnd() < 0.5 ? 0 : 3)] * (unused ? 0.0f : 1.0f) : (float)((2.0 * rnd() - 1.0) * e * (place < 0.6 ? 1.0 : (place < 0.8 ? 16.0 : 1000.0)));
            const float to_box = box[6 * i + a] + (float)rnd() * (box[6 * i + 3 + a] - box[6 * i + a]) - o[3 * i + a];
            d[3 * i + a] = rnd() < 0.15 ? tiny[(int)(rnd() * 4.0) & 3] : (aim && !unused ? to_box : (float)(2.0 * rnd() - 1.0));
        }
        if (d[3 * i] == 0.0f && d[3 * i + 1] == 0.0f && d[3 * i + 2] == 0.0f) d[3 * i + 1] = 1.0f;
        range[2 * i] = rnd() < 0.5 ? 0.01f : 1.0e-4f;
        range[2 * i + 1] = rnd() < 0.4 ? range[2 * i] + (float)(rnd() * 4.0 * e) : 1.0e6f;
    }
    std::vector<uint8_t> form(n);
    std::vector<uint32_t> fr(n), fd(n), sr(n), sd(n);
    bed_run(n, o.data(), d.data(), box.data(), extent.data(), range.data(), form.data(), fr.data(), fd.data(), sr.data(), sd.data());
    int64_t fma_cases = 0, bad = 0, accepts = 0;
    for (int64_t i = 0; i < n; i++) {
        fma_cases += form[i] & 1;
        accepts += sr[i] != bits(kMissT);
        bad += (fr[i] != fd[i]) + (sr[i] != sd[i]);
    }
    printf("cases %lld  fma form %lld  subtract form %lld  accepted %lld  differing %lld\n", (long long)n, (long long)fma_cases, (long long)n, (long long)accepts, (long long)bad);
    return bad == 0 && fma_cases > n / 4 && accepts > n / 100 ? 0 : 1;
}
#endif
