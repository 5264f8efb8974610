// tsx_layout.h -- where the level-1 sub-lists of the fused walk lie: ONE rule for the walk that writes them
// (walk_part_kernel), the level 2 and the skew probe that read them as pieces (partition_ring_kernel,
// skew_probe_kernel) and the host.  Plain C++: device code, host code and stand-alone programs include it.
//
// Sub-list (b, g) -- level-1 bucket b of nb, workgroup (or list set) g of G -- has the NUMBER
//     bucket-major      b * G + g     the G lists of a bucket side by side: what sharded walks, the minimizer exchange,
//                                     slab walks and appending windows fill, launch by launch, g0 .. g0 + grid of G
//     workgroup-major   g * nb + b    the nb lists of a workgroup side by side: the plain one-GPU count.  A flush of the
//                                     walk then stores into one stretch of nb * cap records (16 MB at the default shape)
//                                     instead of lists a bucket's width (G * cap records, 31 MB) apart all over buffer 1
// and starts at record number * cap of the buffer; its final size is published at cnt[number].  cap is a multiple of
// 16 records (plan_partition), so every list starts on a 128-B line in either order.  nb * G < 2^32.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TSX_HD __host__ __device__
#else
#define TSX_HD
#endif

namespace tsx {

struct SubListOrder { uint32_t step_b, step_g; };   // number of list (b, g) = b * step_b + g * step_g

TSX_HD inline SubListOrder sublist_order(uint32_t nb, uint32_t G, int wg_major) {
    return wg_major ? SubListOrder{1u, nb} : SubListOrder{G, 1u};
}
TSX_HD inline uint32_t sublist_number(SubListOrder o, uint32_t b, uint32_t g) { return b * o.step_b + g * o.step_g; }
// first record of list (b, g) in the buffer, lists of cap records
TSX_HD inline uint64_t sublist_first(SubListOrder o, uint32_t b, uint32_t g, uint64_t cap) {
    return (uint64_t)sublist_number(o, b, g) * cap;
}

}  // namespace tsx
