// rt_copy.cpp — the copy-engine entries of the C ABI (pinned host memory, device-to-host
// copies on a DMA engine, warming the engines' queues) and the profile marker.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "rt_internal.h"

using namespace rti;

extern "C" {

// Profile marker (rt_profile_marker): an empty kernel whose grid (64 x tag threads) tells a
// rocprofv3 trace where a caller's timed region begins and ends (tools/pmc_step.py).
int rt_profile_marker(int tag, void* stream) {
    if (tag < 1 || tag > 64) return fail(RT_ERR_ARG, "marker tag must be 1..64");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RT_ERR_NODEV, "no HIP device available");
    rtd::launch_profile_marker(tag, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

int rt_host_alloc(int64_t bytes, void** out) {
    if (!out || bytes <= 0) return fail(RT_ERR_ARG, "bytes > 0 and an output pointer required");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RT_ERR_NODEV, "no HIP device available");
    HIPCHK(hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault));
    return RT_OK;
}
int rt_host_free(void* p) {
    if (p) HIPCHK(hipHostFree(p));
    return RT_OK;
}
// A device -> pinned-host copy on a DMA copy engine.  hipMemcpyDeviceToDeviceNoCU asks the
// runtime for the SDMA path explicitly (the copy still goes where the pointers live: with a
// hipHostMalloc destination it writes host memory over PCIe).  Measured on this image
// (tools/copy_probe.hip, profiles/r06/copy/): 8.29 MB in 0.157 ms (53 GB/s), finished 0.66 ms
// into a grid that held every CU for 3 ms, and no dispatch in the kernel trace; the torch
// pinned-tensor copy the round-5 bench used ran as 320-us `__amd_rocclr_copyBuffer` blit kernels
// that competed with the persistent trace blocks for CUs.
int rt_copy_to_host_async(void* host_dst, const void* dev_src, int64_t bytes, void* stream) {
    if (!host_dst || !dev_src || bytes < 0) return fail(RT_ERR_ARG, "null pointer or negative size");
    if (bytes == 0) return RT_OK;
    HIPCHK(hipMemcpyAsync(host_dst, dev_src, (size_t)bytes, hipMemcpyDeviceToDeviceNoCU, (hipStream_t)stream));
    return RT_OK;
}

// The runtime gives a stream's first copy (and a copy after the stream's last one has drained)
// an idle SDMA engine, and keeps the stream on that engine otherwise; a pipeline's copies queue
// behind frames still rendering, so as they pile up they land on engines 1, 2, 4, ... and the
// first copy on an engine in a direction creates that engine's queue: ~7 ms of host time inside
// hipMemcpyAsync (profiles/r06/rblog/).  Here each of the n streams queues one copy behind a
// gate kernel (on a stream of its own), so every copy finds the engines before it busy and the
// n copies start n engines; then the gate opens.  The streams should be the ones the pipeline
// will use.  Once per process and device for up to the largest n asked for.
int rt_copy_engines_warm(void* const* streams, int n) {
    if (!streams || n < 1 || n > 64) return fail(RT_ERR_ARG, "1 to 64 streams");
    int ndev = 0, dev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RT_ERR_NODEV, "no HIP device available");
    HIPCHK(hipGetDevice(&dev));
    static std::mutex mu;
    static int warmed[64] = {};
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || warmed[dev] >= n) return RT_OK;
    unsigned* flag = nullptr; uint8_t* h = nullptr; uint8_t* d = nullptr;
    hipStream_t gate = nullptr;
    hipEvent_t ev = nullptr;
    int clk_khz = 0;
    // (copies below the runtime's SDMA threshold run elsewhere: 1 MB each, all into one buffer)
    constexpr size_t B = 1 << 20;
    // The first error is kept and the steps after it are skipped; the one exit path below then
    // opens the gate, waits for what was queued, frees everything and reports that error.
    hipError_t e = hipSuccess;
    const char* what = "";
#define WARM_STEP(x) do { if (e == hipSuccess && (e = (x)) != hipSuccess) what = #x; } while (0)
    WARM_STEP(hipDeviceGetAttribute(&clk_khz, hipDeviceAttributeWallClockRate, dev));
    WARM_STEP(hipHostMalloc((void**)&flag, 4, hipHostMallocCoherent));
    WARM_STEP(hipHostMalloc((void**)&h, B, hipHostMallocDefault));
    WARM_STEP(hipMalloc((void**)&d, B));
    WARM_STEP(hipMemset(d, 0, B));
    WARM_STEP(hipStreamCreateWithFlags(&gate, hipStreamNonBlocking));
    WARM_STEP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (e == hipSuccess) {
        __atomic_store_n(flag, 0u, __ATOMIC_RELEASE);
        rtd::launch_copy_gate(flag, (unsigned long long)clk_khz * 2000ull, gate);   // at most 2 s
        WARM_STEP(hipGetLastError());
    }
    WARM_STEP(hipEventRecord(ev, gate));
    for (int i = 0; i < n; i++) {
        WARM_STEP(hipStreamWaitEvent((hipStream_t)streams[i], ev, 0));
        WARM_STEP(hipMemcpyAsync(h, d, B, hipMemcpyDeviceToDeviceNoCU, (hipStream_t)streams[i]));
    }
    // the exit path, error or not
    auto also = [&](hipError_t r, const char* w) { if (e == hipSuccess && r != hipSuccess) { e = r; what = w; } };
    if (flag) __atomic_store_n(flag, 1u, __ATOMIC_RELEASE);                    // open the gate
    if (gate) also(hipStreamSynchronize(gate), "hipStreamSynchronize(gate)");
    for (int i = 0; i < n; i++) also(hipStreamSynchronize((hipStream_t)streams[i]), "hipStreamSynchronize(streams[i])");
#undef WARM_STEP
    if (ev) (void)hipEventDestroy(ev);
    if (gate) (void)hipStreamDestroy(gate);
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    if (flag) (void)hipHostFree(flag);
    if (e != hipSuccess) return fail(RT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    warmed[dev] = n;
    return RT_OK;
}

}  // extern "C"
