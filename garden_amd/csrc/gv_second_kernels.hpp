// gv_second_kernels.hpp — launch interface of gv_second.hip: gv_pool_cull_second_phase, the cull of what a first view left out
// (DESIGN.md §4 item 13, §5.16). Kept apart from gv_kernels.hpp like gv_group_kernels.hpp (bench.py hashes that file).
#pragma once
#include "gv_kernels.hpp"

namespace gv {

constexpr uint32_t kSecondBlock = 256;  // lanes per workgroup of the seen and the union launch

// words of the seen set of a pool of `entries` mirror entries: one bit per entry, whole 256-entry cull tiles (a wave of the masked
// cull loads the word of its 64 entries whether or not the pool reaches that far)
inline size_t second_seen_words(uint32_t entries) { return (size_t)(((entries ? entries : 1u) + kCullBlock - 1u) / kCullBlock) * (kCullBlock / 64u); }

// seen bit entry(visible_idx[k]) |= 1 for k < *count. capacity: the host's bound of *count (sizes the grid); inv: pool slot -> mirror
// entry (NULL: the mirror is in pool order); slots bounds a record's slot, entries the entry it maps to. seen is zero on entry.
hipError_t launch_second_seen(const uint32_t* count, const uint32_t* idx, uint32_t capacity, const uint32_t* inv, uint32_t slots,
                              uint32_t entries, unsigned long long* seen, hipStream_t stream);
// The masked cull: launch_cull's outputs (ballot words, chunk totals; isVisible bytes under vp.write_is_visible) for the entries whose
// seen bit is clear; a seen entry is not visible and none of its streams is read. Full streams only: mesh.hot is not read.
hipError_t launch_second_cull(const MeshMirror& mesh, const TransformMirror& xf, const HizDevice& hiz, const ViewParams& vp,
                              const ViewBuffers& out, const unsigned long long* seen, hipStream_t stream);
// is_visible[e] |= seen bit e for e < entries (mirror order, like the bytes)
hipError_t launch_second_union(const unsigned long long* seen, uint32_t entries, uint8_t* is_visible, hipStream_t stream);

}  // namespace gv
