// tools/microbench/ply_format.hip -- does mvs_plyfmt.h's format_g, compiled for gfx950, write what printf("%g", (double)f) writes, for
// EVERY float bit pattern?  The device formats 2^24 consecutive patterns per launch into 16-byte slots (the text, its length in the
// last byte); the host compares each slot with snprintf on 16 threads.  All 2^32 patterns by default; `ply_format range` covers every
// float with 2^-40 <= |x| < 2^40 and every 4099th pattern of the rest.
//   hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -I ../../mvskit_amd/csrc -o ply_format ply_format.hip && ./ply_format
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "mvs_plyfmt.h"

__global__ void k_format(uint64_t first, uint64_t n, uint8_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t bits = (uint32_t)(first + i);
    char* slot = reinterpret_cast<char*>(out + 16 * i);
    const int len = mvsply::format_g(__uint_as_float(bits), slot);
    slot[15] = (char)len;
}

static bool in_range(uint32_t bits) {  // 2^-40 <= |x| < 2^40: biased exponents 87 .. 166
    const uint32_t ex = (bits >> 23) & 0xffu;
    return ex >= 87u && ex <= 166u;
}

int main(int argc, char** argv) {
    const bool range_only = argc > 1 && strcmp(argv[1], "range") == 0;
    const uint64_t chunk = 1ull << 24;
    uint8_t* d_out = nullptr;
    uint8_t* h_out = nullptr;
    if (hipMalloc(&d_out, chunk * 16) != hipSuccess || hipHostMalloc(&h_out, chunk * 16) != hipSuccess) { printf("FAIL: allocation\n"); return 1; }
    std::atomic<unsigned long long> checked{0}, bad{0};
    std::atomic<uint32_t> first_bad{0xffffffffu};
    const int nth = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    for (uint64_t first = 0; first < (1ull << 32); first += chunk) {
        const bool whole = !range_only || in_range((uint32_t)first) || in_range((uint32_t)(first + chunk - 1));
        hipLaunchKernelGGL(k_format, dim3((unsigned)(chunk / 256)), dim3(256), 0, 0, first, chunk, d_out);
        if (hipMemcpy(h_out, d_out, chunk * 16, hipMemcpyDeviceToHost) != hipSuccess) { printf("FAIL: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
        std::vector<std::thread> th;
        for (int t = 0; t < nth; ++t)
            th.emplace_back([&, t] {
                unsigned long long c = 0, b = 0;
                char want[64];
                for (uint64_t i = t; i < chunk; i += nth) {
                    const uint32_t bits = (uint32_t)(first + i);
                    if (!whole && !in_range(bits) && bits % 4099u != 0) continue;
                    float f;
                    memcpy(&f, &bits, 4);
                    const int n = snprintf(want, sizeof want, "%g", (double)f);
                    const uint8_t* slot = h_out + 16 * i;
                    ++c;
                    if (n != (int)slot[15] || memcmp(want, slot, (size_t)n) != 0) {
                        ++b;
                        uint32_t cur = first_bad.load();
                        while (bits < cur && !first_bad.compare_exchange_weak(cur, bits)) {}
                    }
                }
                checked += c;
                bad += b;
            });
        for (auto& x : th) x.join();
    }
    const unsigned long long nb = bad.load();
    printf("%s: %llu inputs (%s), %llu differ; smallest differing pattern 0x%08x\n", nb == 0 ? "PASS" : "FAIL", checked.load(),
           range_only ? "every float with 2^-40 <= |x| < 2^40, every 4099th pattern of the rest" : "every float bit pattern", nb, first_bad.load());
    (void)hipFree(d_out);
    (void)hipHostFree(h_out);
    return nb == 0 ? 0 : 1;
}
