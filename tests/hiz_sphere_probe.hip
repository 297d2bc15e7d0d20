// hiz_sphere_probe.hip — TEST ONLY: hiz_sphere_occluded of garden_amd/csrc/gv_device.hpp over an array of sphere-stream entries, one
// lane per entry, exactly as cull_kernel<true, kMapExact, true> calls it; built by tests/test_gpu_hiz_sphere.py and compared with
// tests/hiz_sphere_twin.h bit for bit. All pointers except vp and cam are device memory.
#include "gv_device.hpp"

namespace {
struct ProbeView {
    float vp[16];
    float cam[3];
};
__global__ __launch_bounds__(256) void probe_kernel(const gv::HizDevice hz, const ProbeView view, const float4* __restrict__ hot, uint32_t n,
                                                    uint8_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n)
        return;
    const float4 h = hot[i];
    bool proven = false;
    if (!(h.w < 0.0f)) {
        const float tx = h.x - view.cam[0], ty = h.y - view.cam[1], tz = h.z - view.cam[2];
        proven = gv::hiz_sphere_occluded(hz, view.vp, tx, ty, tz, gv::sphere_reach(h.w, tx, ty, tz));
    }
    out[i] = proven ? 1 : 0;
}
}  // namespace

extern "C" int hiz_sphere_probe(const float* depth, const void* mips, const uint64_t* mip_offset, uint32_t width, uint32_t height,
                                uint32_t mip_count, uint32_t nested, const float* vp, const float* cam, const void* hot, uint32_t n, uint8_t* out)
{
    gv::HizDevice hz{};
    hz.depth = depth;
    hz.mips = static_cast<const float2*>(mips);
    hz.mip_offset = mip_offset;
    hz.width = width;
    hz.height = height;
    hz.mip_count = mip_count;
    hz.nested = nested;
    ProbeView view;
    for (int k = 0; k < 16; k++)
        view.vp[k] = vp[k];
    for (int k = 0; k < 3; k++)
        view.cam[k] = cam[k];
    if (n == 0)
        return 0;
    hipLaunchKernelGGL(probe_kernel, dim3((n + 255u) / 256u), dim3(256), 0, nullptr, hz, view, static_cast<const float4*>(hot), n, out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    return (int)e;
}
