// Host sanitizer check of the convolution dispatch: the queries and the pack-batch table builder of conv_mfma.hip and
// wgrad_mfma.hip over a list of descriptors, as a stand-alone program (no launch is made, no GPU is needed).
//
//   python -c "import sys; sys.path.insert(0, 'tests/golden'); import make_route_goldens as M; \
//              print('\n'.join(' '.join(map(str, d)) for d in M.descriptors()))" > descs.txt
//   hipcc -O1 -g -std=c++20 --offload-arch=gfx950 -fno-gpu-rdc -Xarch_host -fsanitize=address,undefined -I include \
//         tools/conv_route_sanitize.cpp ir2rgb_amd/csrc/{conv_mfma,wgrad_mfma,conv3x3_patch,conv7x1_col,conv1x7_thin}.hip -o route_san
//   ./route_san descs.txt
//
// Prints one checksum over every answer; a sanitizer report is the failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/ir2rgb_hip.h"

int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: %s descriptors.txt (23 integers per line)\n", argv[0]); return 2; }
    constexpr int NF = sizeof(ir2rgb_conv_desc) / sizeof(int);
    uint64_t sum = 0;
    long n = 0;
    auto mix = [&](long v) { sum = sum * 1099511628211ull + (uint64_t)v; };
    for (;; ++n) {
        ir2rgb_conv_desc d;
        int *fields = reinterpret_cast<int *>(&d), got = 0;
        while (got < NF && fscanf(f, "%d", &fields[got]) == 1) ++got;
        if (got < NF) break;
        for (const char *c = ir2rgb_conv2d_kernel_name(&d); *c; ++c) mix(*c);
        mix(ir2rgb_conv2d_stats_rows(&d)); mix(ir2rgb_conv2d_packed_weight_elems(&d)); mix(ir2rgb_conv2d_fwd_workspace_bytes(&d));
        mix(ir2rgb_conv2d_wgrad_workspace_elems(&d)); mix(ir2rgb_conv2d_wgrad_acc_workspace_elems(&d));
        mix(ir2rgb_conv2d_wgrad(&d, (const void *)8, (const void *)16, nullptr, nullptr, nullptr));     // misaligned: no launch
        for (int job = 0; job < 4; ++job) {         // forward / adjoint, aligned / w four bytes off (fake pointers, never read)
            ir2rgb_pack_job j{};
            j.desc = d; j.w = (const float *)(uintptr_t)(0x10000 + 4 * (job & 1)); j.wpacked = (void *)(uintptr_t)0x20000; j.adjoint = job >> 1;
            const long need = ir2rgb_conv2d_pack_batch_table_bytes(&j, 1);
            mix(need);
            if (need < 0) continue;
            std::vector<unsigned char> table((size_t)need);     // exactly the bytes asked for: an overrun is reported
            int nblocks = -1;
            mix(ir2rgb_conv2d_pack_batch_build(&j, 1, table.data(), need, &nblocks));
            mix(nblocks);
            for (unsigned char b : table) mix(b);
        }
    }
    fclose(f);
    mix(ir2rgb_conv2d_kernel_name(nullptr)[0]); mix(ir2rgb_conv2d_stats_rows(nullptr)); mix(ir2rgb_conv2d_fwd_workspace_bytes(nullptr));
    mix(ir2rgb_conv2d_packed_weight_elems(nullptr)); mix(ir2rgb_conv2d_wgrad_workspace_elems(nullptr));
    printf("%ld descriptors, checksum %016llx\n", n, (unsigned long long)sum);
    return n > 0 ? 0 : 1;
}
