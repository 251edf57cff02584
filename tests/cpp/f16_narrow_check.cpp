// The kernels' float -> binary16 narrowing (lumahdrv_amd/csrc/f16_narrow.hpp, compiled here by the host compiler) against
// ExrInterface::floatToHalf for all 2^32 float bit patterns.  Prints the number of mismatches and the first few; exit status 0
// when there are none.  Built and run by tests/test_f16_frames_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "exr_interface.h"
#include "f16_narrow.hpp"

int main(int argc, char **argv)
{
    const unsigned nthreads = argc > 1 ? (unsigned)atoi(argv[1]) : 8;
    std::vector<unsigned long long> bad(nthreads, 0);
    std::vector<unsigned> first(nthreads, 0);
    std::vector<std::thread> th;
    const unsigned long long total = 1ull << 32, per = (total + nthreads - 1) / nthreads;
    for (unsigned t = 0; t < nthreads; t++)
        th.emplace_back([&, t]() {
            const unsigned long long lo = t * per, hi = lo + per < total ? lo + per : total;
            for (unsigned long long i = lo; i < hi; i++) {
                const uint32_t b = (uint32_t)i;
                float f;
                memcpy(&f, &b, 4);
                if (lh::f16_narrow(f) != ExrInterface::floatToHalf(f)) {
                    if (bad[t]++ == 0)
                        first[t] = b;
                }
            }
        });
    for (auto &x : th)
        x.join();
    unsigned long long n = 0;
    for (unsigned t = 0; t < nthreads; t++) {
        n += bad[t];
        if (bad[t]) {
            float f;
            memcpy(&f, &first[t], 4);
            printf("mismatch at 0x%08x: f16_narrow 0x%04x, floatToHalf 0x%04x\n", first[t], lh::f16_narrow(f), ExrInterface::floatToHalf(f));
        }
    }
    printf("checked 4294967296 float bit patterns: %llu mismatches\n", n);
    return n ? 1 : 0;
}
