// dense_rounds_probe.hip — TEST ONLY: dense_rounds of garden_amd/csrc/gv_dense_rounds.hpp with a table as the per-entry decision, one
// super-tile of K tiles per workgroup exactly as cull_hot_kernel<true, K> calls it; built by tests/test_gpu_dense_rounds.py and compared
// with numpy. cls: 0 outside, 1 inside, 2 undecided per entry; vis: the decision of a candidate. All pointers are device memory.
#include "gv_dense_rounds.hpp"

namespace {
constexpr uint32_t kUndecided = 2u;
struct ProbeArgs {
    const uint8_t* cls;
    const uint8_t* vis;
    unsigned long long* mask;
    uint32_t* chunk_count;
    uint8_t* is_visible;  // or null
    uint32_t* errors;     // decisions asked of an entry that is no candidate, or with the wrong class bit
    uint32_t n, nblocks, tiles_per_chunk;
};
template <uint32_t K>
__global__ __launch_bounds__(256) void probe_kernel(const ProbeArgs a)
{
    const uint32_t first = blockIdx.x * K;
    if (first >= a.nblocks)
        return;
    uint32_t where = 0;
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t i = (first + k) * 256u + threadIdx.x;
        where |= (i < a.n ? (uint32_t)a.cls[i] : 0u) << (2u * k);
    }
    __shared__ gv::DenseRoundsLds<K> lds;
    gv::dense_rounds<K>(
        lds, where, kUndecided, first,
        [&](uint32_t slot, bool undecided) {
            const uint32_t i = first * 256u + slot;
            if (slot >= K * 256u || i >= a.n || a.cls[i] == 0 || (a.cls[i] == kUndecided) != undecided) {
                atomicAdd(a.errors, 1u);
                return false;
            }
            return a.vis[i] != 0;
        },
        [&] { return gv::DenseOutputs{a.mask, a.chunk_count, a.is_visible, a.nblocks, a.n, a.tiles_per_chunk}; });
}
}  // namespace

extern "C" int dense_rounds_probe(uint32_t k, const void* cls, const void* vis, void* mask, void* chunk_count, void* is_visible, void* errors,
                                  uint32_t n, uint32_t tiles_per_chunk)
{
    if (n == 0 || (k != 2 && k != 4) || tiles_per_chunk % k != 0)
        return -1;
    const uint32_t nblocks = (n + 255u) / 256u;
    const ProbeArgs a{static_cast<const uint8_t*>(cls), static_cast<const uint8_t*>(vis), static_cast<unsigned long long*>(mask),
                      static_cast<uint32_t*>(chunk_count), static_cast<uint8_t*>(is_visible), static_cast<uint32_t*>(errors), n, nblocks,
                      tiles_per_chunk};
    const dim3 grid((nblocks + k - 1u) / k), block(256);
    if (k == 2)
        hipLaunchKernelGGL(probe_kernel<2>, grid, block, 0, nullptr, a);
    else
        hipLaunchKernelGGL(probe_kernel<4>, grid, block, 0, nullptr, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    return (int)e;
}
