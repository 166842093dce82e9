// Host-only view of the forward dispatch (csrc/nplda_fwd_dispatch.h) for tests/test_fp32_units_dispatch_cpu.py: for each
// batch size given, the pair-scoring choice, its split point, the remainder's choice, and the kernel embed() takes.  The
// embedding rule restates launch_fwd<MODE_EMBED> / launch_fwd_old (inference: no saved activations): the balanced-tile
// kernel where the pair model picks it for (n + 1) / 2 units without a split, else the small kernel up to 64 units per
// 256-CU-equivalent (256 * 64 units), else v2.  No device is touched.
// usage: fp32_units_dispatch D0 D cus n...   ->   n choice split rem_choice embed
#include <cstdio>
#include <cstdlib>
#include "nplda_fwd_dispatch.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int D0 = atoi(argv[1]), D = atoi(argv[2]), cus = atoi(argv[3]);
    const NpldaLayout L = nplda_layout(D0, D, D);
    for (int i = 4; i < argc; ++i) {
        const long long n = atoll(argv[i]);
        const int k = nplda::pair_kernel_choice(n, L, cus);
        const long long sp = nplda::pair_split_point(n, cus);
        const int kr = (k == nplda::FWD_SPLIT) ? nplda::pair_kernel_choice(n - sp, L, cus, nullptr, false) : -1;
        const long long units = (n + 1) / 2;
        const char* e = nplda::pair_kernel_choice(units, L, cus, nullptr, false) == nplda::FWD_MID ? "mid"
                        : units <= 256 * 64                                                      ? "small"
                                                                                                 : "v2";
        printf("%lld %d %lld %d %s\n", n, k, sp, kr, e);
    }
    return 0;
}
