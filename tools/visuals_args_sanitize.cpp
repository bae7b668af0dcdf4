// Host sanitizer check of ir2rgb_visuals_u8's argument handling (visuals.hip) as a stand-alone program: every call below
// is refused before a launch, so no GPU is needed and no pointer is dereferenced on the device.
//
//   hipcc -O1 -g -std=c++20 --offload-arch=gfx950 -fno-gpu-rdc -Xarch_host -fsanitize=address,undefined -I include \
//         tools/visuals_args_sanitize.cpp ir2rgb_amd/csrc/visuals.hip -o visuals_san
//   ./visuals_san
//
// The panel arrays are heap blocks of exactly n entries: a read past the table is reported.  Prints the number of calls
// and a checksum of their answers; a sanitizer report or a wrong answer is the failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/ir2rgb_hip.h"

int main() {
    const float *src = (const float *)(uintptr_t)0x10000;           // fake device pointers, never read
    uint8_t *out = (uint8_t *)(uintptr_t)0x20000;
    float *ws = (float *)(uintptr_t)0x30000;
    long calls = 0, wrong = 0;
    uint64_t sum = 0;
    auto expect = [&](long got, long want) { ++calls; sum = sum * 1099511628211ull + (uint64_t)got; if (got != want) { ++wrong; fprintf(stderr, "call %ld: %ld, expected %ld\n", calls, got, want); } };
    auto table = [&](int n, int kind, int channels, const float *p) { return std::vector<ir2rgb_panel>((size_t)n, ir2rgb_panel{p, kind, channels}); };

    expect(ir2rgb_visuals_u8(nullptr, 1, 4, 8, ws, out, nullptr), IR2RGB_EINVAL);
    { auto t = table(1, IR2RGB_PANEL_IMAGE_NORM, 3, src);
      expect(ir2rgb_visuals_u8(t.data(), 0, 4, 8, ws, out, nullptr), IR2RGB_EINVAL);
      expect(ir2rgb_visuals_u8(t.data(), 17, 4, 8, ws, out, nullptr), IR2RGB_EINVAL);      // n is refused before the table is read
      expect(ir2rgb_visuals_u8(t.data(), -1, 4, 8, ws, out, nullptr), IR2RGB_EINVAL);
      expect(ir2rgb_visuals_u8(t.data(), 1, 0, 8, ws, out, nullptr), IR2RGB_EINVAL);
      expect(ir2rgb_visuals_u8(t.data(), 1, 4, 8, ws, nullptr, nullptr), IR2RGB_EINVAL);
      expect(ir2rgb_visuals_u8(t.data(), 1, 1 << 15, 1 << 15, ws, out, nullptr), IR2RGB_EINVAL);     // H * W * 3 > 2^31 - 1
      expect(ir2rgb_visuals_u8(t.data(), 1, 26755, 26755, ws, out, nullptr), IR2RGB_EINVAL);         // 3 * 26755^2 = 2^31 + 6427
    }
    for (int n = 1; n <= 16; ++n) {
        for (int kind = -1; kind <= 9; ++kind)
            for (int ch = 0; ch <= 4; ++ch) {
                const bool image = kind == IR2RGB_PANEL_IMAGE_NORM || kind == IR2RGB_PANEL_IMAGE_UNIT;
                const bool fits = image ? ch == 1 || ch == 3 : kind == IR2RGB_PANEL_FLOW && ch == 2;
                if (fits) {         // valid but for the LAST panel's misaligned source / a missing workspace: still no launch
                    auto t = table(n, kind, ch, src);
                    t.back().src = (const float *)(uintptr_t)0x10002;
                    expect(ir2rgb_visuals_u8(t.data(), n, 4, 8, ws, out, nullptr), IR2RGB_EALIGN);
                    if (kind == IR2RGB_PANEL_FLOW) {
                        auto f = table(n, kind, ch, src);
                        expect(ir2rgb_visuals_u8(f.data(), n, 4, 8, nullptr, out, nullptr), IR2RGB_EINVAL);
                        expect(ir2rgb_visuals_u8(f.data(), n, 4, 8, (float *)(uintptr_t)0x30002, out, nullptr), IR2RGB_EALIGN);
                    }
                } else {
                    auto t = table(n, IR2RGB_PANEL_IMAGE_UNIT, 1, src);
                    t.back().kind = kind, t.back().channels = ch;
                    expect(ir2rgb_visuals_u8(t.data(), n, 4, 8, ws, out, nullptr), IR2RGB_EINVAL);
                }
            }
        auto t = table(n, IR2RGB_PANEL_IMAGE_NORM, 3, src);
        t.back().src = nullptr;
        expect(ir2rgb_visuals_u8(t.data(), n, 4, 8, ws, out, nullptr), IR2RGB_EINVAL);
    }
    expect(ir2rgb_visuals_workspace_bytes(-1, 4, 8), IR2RGB_EINVAL);
    expect(ir2rgb_visuals_workspace_bytes(17, 4, 8), IR2RGB_EINVAL);
    expect(ir2rgb_visuals_workspace_bytes(1, 0, 8), IR2RGB_EINVAL);
    expect(ir2rgb_visuals_workspace_bytes(1, 1 << 15, 1 << 15), IR2RGB_EINVAL);
    expect(ir2rgb_visuals_workspace_bytes(0, 4, 8), 0);
    expect(ir2rgb_visuals_workspace_bytes(1, 1, 1), 8);
    expect(ir2rgb_visuals_workspace_bytes(2, 17, 260), 80);
    expect(ir2rgb_visuals_workspace_bytes(2, 512, 1024), 2 * 256 * 8);
    expect(ir2rgb_visuals_workspace_bytes(16, 26754, 26754), 16 * 256 * 8);
    printf("%ld calls, %ld wrong, checksum %016llx\n", calls, wrong, (unsigned long long)sum);
    return wrong ? 1 : 0;
}
