// Host-only view of the headline kernel's layer-1 decision (csrc/nplda_fwd_dispatch.h) for tests/test_v6h_dispatch_cpu.py:
// for each batch size, the pair-scoring choice, the S1 launch_fwd_v6 would run (0 = nplda_fwd_v6.h) and the label.  The
// environment switches are read once per process, so the test starts one process per setting.  No device is touched.
// usage: v6h_dispatch D0 D cus n...   ->   n choice s1 default_s1 | label
#include <cstdio>
#include <cstdlib>
#include "nplda_fwd_dispatch.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int D0 = atoi(argv[1]), D = atoi(argv[2]), cus = atoi(argv[3]);
    const NpldaLayout L = nplda_layout(D0, D, D);
    for (int i = 4; i < argc; ++i) {
        const long long n = atoll(argv[i]);
        printf("%lld %d %d %d | %s\n", n, nplda::pair_kernel_choice(n, L, cus), nplda::fwd_v6h_s1(L),
               (int)nplda::FWD_V6H_S1_DEFAULT, nplda::pair_kernel_name(n, L));
    }
    return 0;
}
