// conctest_prio.hip -- conctest.hip with two stream classes: S normal-priority streams plus P streams of the greatest priority the
// device reports.  Does the runtime map the high-priority streams onto hardware queues of their own, beside the GPU_MAX_HW_QUEUES
// queues of the normal ones?  Each kernel is a few single-wave workgroups that spin for ~10 ms; total time = ceil(kernels / concurrent
// kernels) * 10 ms, so "kernels at a time" above what the S normal streams reach alone is what the second class adds.
//   hipcc --offload-arch=gfx950 -O2 tools/conctest_prio.hip -o tools/_bin/conctest_prio && tools/_bin/conctest_prio [workgroups]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <chrono>
__global__ void spin(unsigned long long ticks, unsigned *out)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    unsigned x = 0;
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) x++;
    if (x == 0xFFFFFFFFu) out[0] = x;
}
#define CK(expr)                                                                                              \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_)); return 1; }        \
    } while (0)
int main(int argc, char **argv)
{
    const int wgs = argc > 1 ? atoi(argv[1]) : 65;
    int least = 0, greatest = 0;
    CK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    printf("stream priority range: least %d, greatest %d%s\n", least, greatest, least == greatest ? " (no priority classes)" : "");
    unsigned *d;
    CK(hipMalloc(&d, 4));
    static const int cfg[][2] = {{4, 0}, {8, 0}, {0, 1}, {0, 4}, {0, 8}, {4, 1}, {4, 4}, {8, 4}, {11, 4}, {11, 8}, {16, 4}};
    for (const auto &c : cfg) {
        const int S = c[0], P = c[1];
        hipStream_t st[32];
        // the normal streams first, then the high-priority ones together: the order the library creates them in
        for (int i = 0; i < S; i++) CK(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
        for (int i = 0; i < P; i++) CK(hipStreamCreateWithPriority(&st[S + i], hipStreamNonBlocking, greatest));
        CK(hipDeviceSynchronize());
        auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < S + P; i++) hipLaunchKernelGGL(spin, dim3(wgs), dim3(64), 0, st[i], 1000000ull /* 10 ms at 100 MHz */, d);
        CK(hipDeviceSynchronize());
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("%2d normal + %d high-priority streams x %d single-wave workgroups spinning 10 ms: %.1f ms -> ~%.1f kernels at a time\n", S, P, wgs, ms,
               (S + P) * 10.0 / ms);
        for (int i = 0; i < S + P; i++) CK(hipStreamDestroy(st[i]));
    }
    CK(hipFree(d));
    return 0;
}
