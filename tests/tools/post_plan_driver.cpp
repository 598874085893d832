// Host driver of vulkan-path-tracer_amd/csrc/post_plan.hpp for tests/test_post_plan_cpu.py: a stand-alone program.  Every line of standard input is a case
// `w h mip_count schedule` (schedule: 0 the fused plan, 1 the reference passes); for each, one line of output:
//   mips <count> <w>x<h> ... | <kind> <first> <count> <staged> ; ...
// with the steps in launch order and every field as the plan holds it.  Exit status 2 on a line that does not parse.
#include <cstdio>

#include "post_plan.hpp"

using namespace vpt::post;

int main() {
    static const char* const kNames[] = {"threshold", "first", "down", "down_chain", "tail", "up", "up_chain", "final", "tonemap"};
    unsigned w, h, mip_count, schedule;
    int got;
    while ((got = scanf("%u %u %u %u", &w, &h, &mip_count, &schedule)) == 4) {
        const Mips m = mips_of(w, h);
        const Plan p = schedule ? reference_plan(m, mip_count) : fused_plan(m, mip_count);
        printf("mips %u", m.count);
        for (uint32_t i = 0; i < m.count; i++) printf(" %ux%u", m.w[i], m.h[i]);
        printf(" |");
        for (uint32_t i = 0; i < p.n; i++) {
            const Step& s = p.steps[i];
            if (s.kind >= sizeof kNames / sizeof kNames[0]) return 3;
            printf(" %s %u %u %u ;", kNames[s.kind], (unsigned)s.first, (unsigned)s.count, (unsigned)s.staged);
        }
        printf("\n");
    }
    return got == EOF ? 0 : 2;
}
