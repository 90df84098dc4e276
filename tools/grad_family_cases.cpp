// grad_family_cases.cpp — a stand-alone host program around geomloss_amd/csrc/glhip_family.h (no HIP, no device): the gradient family of
// every row it reads (tests/test_grad_family_cpu.py feeds it the rows of tests/golden/reference_grad_family.npz).
//
// stdin: one launch per line, `entry p_or_kind mode B N M D flags n_ranges` — entry 0 / 1: glhip_softmin_bwd_x / glhip_softmin_fwd_grad
// (softmin_bwd_family of p), 2 / 3: glhip_kernel_conv_bwd_x / glhip_kernel_conv_fwd_grad (conv_family of the kind).  stdout: one
// GLHIP_FAMILY_* code (or GLHIP_EUNSUPPORTED) per line.
#include <cstdio>

#include "glhip_family.h"

int main() {
    int entry, pk, mode, B, D, flags, n_ranges;
    long N, M;
    while (std::scanf("%d %d %d %d %ld %ld %d %d %d", &entry, &pk, &mode, &B, &N, &M, &D, &flags, &n_ranges) == 9)
        std::printf("%d\n", entry < 2 ? glhip::softmin_bwd_family(mode, B, N, M, D, pk, flags, n_ranges) : glhip::conv_family(pk, mode, B, D, flags, n_ranges));
    return 0;
}
