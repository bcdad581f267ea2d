// pk_hist_cluster.hpp -- exact k-means under the earth mover's distance over strength histograms (include/pokerl_hip.h "Histogram
// clustering"): what the host entry points (pk_api.hip) and the kernels (pk_hist_cluster.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pk {

constexpr uint32_t STREAM_CLS = 0x434C5330u;             // 'CLS0': the seeding's own Philox stream, counter (round j, 0, STREAM_CLS, nonce)
constexpr int CL_MAX_BINS = 32;                          // PK_EQ_HIST_MAX_BINS
constexpr int CL_MAX_K = 4096;                           // PK_CL_MAX_K
constexpr int CL_MAX_ITERS = 1024;
constexpr uint32_t CL_NONE = 0xFFFFu;                    // PK_CL_NONE: the label of an empty row
constexpr int CL_ROW_DWORDS = 16;                        // a packed centroid: 64 bytes, whatever nbins is (the first ceil(nbins / 2) dwords are read)
constexpr int CL_BLOCK = 256;                            // every kernel of the family: four waves
constexpr unsigned CL_GRID_MAX = 2048;                   // the grid-stride kernels: eight workgroups = eight waves per SIMD on 256 CUs
constexpr unsigned CL_SEED_GROUPS = 1024;                // the seeding cuts the rows into at most about this many contiguous chunks, one workgroup each
constexpr int CL_LDS_SUMS = 4096;                        // k_cl_update keeps the sums in LDS while K * nbins fits this many (32 KB + 16 KB of counts)
static_assert(CL_MAX_K - 1 < (int)CL_NONE, "no label is PK_CL_NONE");
static_assert(32ull * 65535ull < (1ull << 32), "a distance fits 32 bits");
static_assert(65535ull * 32ull * 65535ull < (1ull << 38), "the quantisation's product needs a 64-bit division");

constexpr int cl_pairs(int nbins) { return (nbins + 1) / 2; }   // packed dwords of a row
// rows of one seeding chunk: a multiple of the workgroup's width
inline size_t cl_chunk_rows(size_t n) {
    const size_t per = (n + CL_SEED_GROUPS - 1) / CL_SEED_GROUPS;
    return ((per + CL_BLOCK - 1) / CL_BLOCK) * CL_BLOCK;
}
inline size_t cl_chunks(size_t n) { const size_t c = cl_chunk_rows(n); return (n + c - 1) / c; }

// The work space of a call, carved out of one buffer: every piece 256-byte aligned.
struct ClWork {
    uint32_t *q;        // [n][pairs]       the quantised CDFs, two u16 per dword; an empty row is all zeros
    uint32_t *cp;       // [K][16]          the centroids, packed the same way
    uint32_t *mind;     // [n]              seeding: the distance to the nearest centroid chosen so far
    uint64_t *part;     // [chunks]         seeding: a chunk's weight in this round
    uint64_t *rows;     // [chunks]         seeding: a chunk's non-empty rows
    uint64_t *sums;     // [K][nbins]       update: per-cluster sums, zero between iterations
    uint32_t *counts;   // [K]              ... and counts
};
size_t cl_work_bytes(size_t n, int nbins, int K, bool seeding, bool update);
ClWork cl_work(void *base, size_t n, int nbins, int K, bool seeding, bool update);

// Each queues its kernels on `stream`; arguments are the caller's to check.
hipError_t cl_seed_launch(hipStream_t stream, size_t n, int nbins, const uint16_t *hist, int K, uint32_t key0, uint32_t key1, uint32_t nonce,
                          uint16_t *centroids, const ClWork &w);
hipError_t cl_assign_launch(hipStream_t stream, size_t n, int nbins, const uint16_t *hist, int K, const uint16_t *centroids, uint16_t *label,
                            uint32_t *dist, const ClWork &w);
hipError_t cl_cluster_launch(hipStream_t stream, size_t n, int nbins, const uint16_t *hist, int K, uint16_t *centroids, int iters, uint16_t *label,
                             uint32_t *dist, uint64_t *inertia, uint32_t *changed, const ClWork &w);

}  // namespace pk
