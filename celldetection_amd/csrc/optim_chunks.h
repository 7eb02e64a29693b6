// The chunk partition, the lane mapping and the alignment rule of the optimizer kernels (csrc/optim.hip).  A step works on a list
// of n tensors of numel[t] >= 0 elements.  Every tensor is cut, on its own, into chunks of OPT_CHUNK consecutive elements (the last
// may be partial; a tensor of 0 elements has none); the chunks of tensor 0 come first, then those of tensor 1 and so on.  The chunk
// map holds one record {tensor, chunk of that tensor} per chunk; it depends on the sizes alone.  One workgroup of OPT_LANES lanes
// works on one chunk at a time.  Inside a chunk, element e (0 <= e < OPT_CHUNK) belongs to the vector e / vec, vec = opt_vec(dtype)
// elements of 16 bytes of the parameter's dtype; vector q belongs to lane q % OPT_LANES and is that lane's item q / OPT_LANES.  A
// lane walks its items in ascending order and the elements of an item in ascending order, whether it moves the item as one 16-byte
// access or element by element: the mapping does not depend on the path, so neither does the order of a lane's fp64 sum.
// Integer arithmetic only; compiles for the device and for the host (tests/optim_chunks_host.cpp runs it against brute force under
// sanitizers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OPT_HD __host__ __device__ __forceinline__
#else
#define OPT_HD inline
#endif

constexpr int OPT_LANES = 256;          // lanes of a workgroup
constexpr int OPT_CHUNK = 8192;         // elements per chunk: 8 items per lane in fp32, 4 in bf16
constexpr int OPT_MAX_GRID = 2048;      // workgroups per launch: about 8 per CU of the 256; more chunks are walked with this stride
constexpr int OPT_F32 = 0, OPT_BF16 = 1;  // dtype codes (those of the "Trainable convolution" section)
constexpr int OPT_FLAG_SCALAR = 1;      // a pointer of the tensor is not 16-byte aligned: every item moves element by element
constexpr int64_t OPT_MAX_CHUNKS = 2147483647;

// elements of a 16-byte vector of the dtype
OPT_HD int32_t opt_vec(int32_t dtype) { return dtype == OPT_BF16 ? 8 : 4; }

// chunks of a tensor of numel >= 0 elements, and the elements of its chunk k (0 <= k < chunks)
OPT_HD int64_t opt_chunks(int64_t numel) { return (numel + OPT_CHUNK - 1) / OPT_CHUNK; }
OPT_HD int32_t opt_chunk_count(int64_t numel, int64_t k) {
    const int64_t left = numel - k * OPT_CHUNK;
    return left <= 0 ? 0 : (left < OPT_CHUNK ? (int32_t) left : OPT_CHUNK);
}
// elements of the last chunk (0 for an empty tensor; OPT_CHUNK where the size is a multiple of it)
OPT_HD int32_t opt_tail(int64_t numel) { return numel <= 0 ? 0 : opt_chunk_count(numel, opt_chunks(numel) - 1); }

// items a lane walks in a chunk of `count` elements, and whether item `item` of lane `lane` is a whole vector inside the chunk
// (moved as 16 bytes unless the tensor is flagged), a partial one (element by element, the scalar epilogue) or past the end
OPT_HD int32_t opt_items(int32_t count, int32_t vec) { return (count + OPT_LANES * vec - 1) / (OPT_LANES * vec); }
OPT_HD int32_t opt_item_first(int32_t item, int32_t lane, int32_t vec) { return (item * OPT_LANES + lane) * vec; }
OPT_HD int32_t opt_item_elements(int32_t count, int32_t item, int32_t lane, int32_t vec) {
    const int32_t left = count - opt_item_first(item, lane, vec);
    return left <= 0 ? 0 : (left < vec ? left : vec);
}

// the alignment rule: the flag of a tensor whose four addresses are given (0 = not used by the launch)
OPT_HD int32_t opt_flags(uint64_t p, uint64_t g, uint64_t m, uint64_t v) { return ((p | g | m | v) & 15u) ? OPT_FLAG_SCALAR : 0; }

// total chunks of a list of sizes; -1 where a size is negative or the total exceeds OPT_MAX_CHUNKS
inline int64_t opt_total_chunks(const int64_t *numel, int32_t n) {
    int64_t total = 0;
    for (int32_t t = 0; t < n; ++t) {
        if (numel[t] < 0 || numel[t] > OPT_MAX_CHUNKS * (int64_t) OPT_CHUNK) return -1;
        total += opt_chunks(numel[t]);
        if (total > OPT_MAX_CHUNKS) return -1;
    }
    return total;
}

// fills map[chunk] = {tensor, chunk of the tensor} for a list whose opt_total_chunks is `chunks` (the caller checked it)
inline void opt_fill_map(const int64_t *numel, int32_t n, int32_t *map) {
    int64_t c = 0;
    for (int32_t t = 0; t < n; ++t)
        for (int64_t k = 0, e = opt_chunks(numel[t]); k < e; ++k, ++c) {
            map[2 * c] = t;
            map[2 * c + 1] = (int32_t) k;
        }
}

// workgroups of a launch over `chunks` chunks
OPT_HD int32_t opt_grid(int64_t chunks) { return chunks < OPT_MAX_GRID ? (int32_t) (chunks < 1 ? 1 : chunks) : OPT_MAX_GRID; }

// the final sum of the chunk partials: lane l of the one workgroup adds the partials [l * per, min(chunks, (l + 1) * per)) in
// ascending order, per = opt_final_per(chunks); the lanes' sums are then added in ascending lane order
OPT_HD int64_t opt_final_per(int64_t chunks) { return (chunks + OPT_LANES - 1) / OPT_LANES; }
// fp64 additions on the longest path from an element to the sum of squares: a lane's chain in the largest chunk, the 6 steps of the
// wave, the waves of the workgroup, a final lane's chain and the final lanes
OPT_HD int64_t opt_sum_chain(int64_t chunks) { return OPT_CHUNK / OPT_LANES + 6 + OPT_LANES / 64 + opt_final_per(chunks) + OPT_LANES; }
