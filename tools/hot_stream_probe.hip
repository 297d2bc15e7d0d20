// Dev tool: how fast one 16-byte nontemporal load per entry streams a 10 M-entry float4 array (the sphere stream of a cfg3
// pool, 160 MB) when each lane of a 256-thread workgroup covers K entries, all K loads issued before any is used. Entry
// base + k * 256 + tid for k = 0 .. K-1, so every k is one contiguous 4 KB sweep of the workgroup, as in cull_hot_kernel.
// Nothing is computed that matters and nothing is written but a sink no real input reaches. "warm": the array is read again
// and again (it fits in the 256 MB Infinity Cache); "cold": a 512 MB fill runs in front of every timed launch, as a frame's other
// traffic does in front of the cull.
//   hipcc --offload-arch=gfx950 -O3 tools/hot_stream_probe.hip -o /tmp/hot_stream_probe && /tmp/hot_stream_probe [entries]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) {                                                                   \
            std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            std::exit(1);                                                                         \
        }                                                                                         \
    } while (0)

typedef float f32x4n __attribute__((ext_vector_type(4)));

template <int K>
__global__ __launch_bounds__(256) void probe(const float4* __restrict__ src, uint32_t n, float* __restrict__ sink)
{
    const uint32_t base = blockIdx.x * (K * 256u) + threadIdx.x;
    f32x4n v[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t i = base + k * 256u;
        v[k] = i < n ? __builtin_nontemporal_load(reinterpret_cast<const f32x4n*>(src + i)) : f32x4n{0.0f, 0.0f, 0.0f, 0.0f};
    }
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < K; k++)
        s += v[k].x + v[k].y + v[k].z + v[k].w;
    if (s == 12345.678f)  // never true for the input below: keeps the loads alive
        sink[0] = s;
}

template <int K>
static void run(const float4* src, uint32_t n, float* sink, hipEvent_t t0, hipEvent_t t1, void* flush, size_t flush_bytes)
{
    const uint32_t grid = (n + K * 256u - 1) / (K * 256u);
    for (int w = 0; w < 5; w++)
        hipLaunchKernelGGL(probe<K>, dim3(grid), dim3(256), 0, 0, src, n, sink);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<float> ms;
    for (int r = 0; r < 50; r++) {
        if (flush)
            CHECK(hipMemsetAsync(flush, r & 0xFF, flush_bytes));
        CHECK(hipEventRecord(t0));
        hipLaunchKernelGGL(probe<K>, dim3(grid), dim3(256), 0, 0, src, n, sink);
        CHECK(hipEventRecord(t1));
        CHECK(hipEventSynchronize(t1));
        float t = 0.0f;
        CHECK(hipEventElapsedTime(&t, t0, t1));
        ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    const double bytes = 16.0 * n;
    std::printf("%s K=%d grid=%u  median %.2f us  %.0f GB/s   best %.2f us  %.0f GB/s\n", flush ? "cold" : "warm", K, grid, ms[ms.size() / 2] * 1e3,
                bytes / (ms[ms.size() / 2] * 1e-3) / 1e9, ms[0] * 1e3, bytes / (ms[0] * 1e-3) / 1e9);
}

int main(int argc, char** argv)
{
    const uint32_t n = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 10000000u;
    float4* src = nullptr;
    float* sink = nullptr;
    CHECK(hipMalloc(&src, (size_t)n * sizeof(float4)));
    CHECK(hipMalloc(&sink, sizeof(float)));
    CHECK(hipMemset(src, 0, (size_t)n * sizeof(float4)));
    hipEvent_t t0, t1;
    CHECK(hipEventCreate(&t0));
    CHECK(hipEventCreate(&t1));
    std::printf("%u entries, %.1f MB\n", n, 16.0 * n / 1e6);
    const size_t flush_bytes = (size_t)512 << 20;
    void* flush = nullptr;
    CHECK(hipMalloc(&flush, flush_bytes));
    for (void* f : {(void*)nullptr, flush}) {
        run<1>(src, n, sink, t0, t1, f, flush_bytes);
        run<2>(src, n, sink, t0, t1, f, flush_bytes);
        run<4>(src, n, sink, t0, t1, f, flush_bytes);
        run<8>(src, n, sink, t0, t1, f, flush_bytes);
    }
    CHECK(hipFree(flush));
    CHECK(hipFree(src));
    CHECK(hipFree(sink));
    return 0;
}
