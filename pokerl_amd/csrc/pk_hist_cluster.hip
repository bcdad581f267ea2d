// pk_hist_cluster.hip -- exact k-means under the earth mover's distance over strength histograms (include/pokerl_hip.h "Histogram clustering",
// DESIGN.md section 3.8).  Everything is an integer; the device equals tests/hist_cluster_spec.py bit for bit.
//   k_cl_quant          rows u16 [n][nbins] -> q: floor(65535 * running sum / mass) per bin, two u16 per dword; an odd nbins is padded with a zero
//                       half in rows and centroids alike, which adds |0 - 0| to a distance.  An empty row (mass 0) is all zeros, and since a
//                       non-empty row ends in 65535 the LAST dword is the empty-row flag.  The rows of a workgroup are one contiguous piece of
//                       memory: it is staged in LDS with 16-byte loads (2-byte loads where the caller's pointer is not 16-byte aligned).
//   k_cl_pack           centroids u16 [K][nbins] -> [K][16] dwords (64 bytes per centroid, the rest of a row zero)
//   k_cl_assign<P>      THE HOT PATH: a lane owns a row, its P = ceil(nbins / 2) packed dwords stay in registers; the centroid is uniform across
//                       the wave and is read with scalar loads straight from the packed array; P packed sums of absolute differences per
//                       centroid (v_sad_u16), a strict < keeps the smallest c among equals.  P is the template parameter, 1 .. 16 -- sixteen
//                       small kernels, so that no instruction is spent on padding at any nbins.  changed / inertia: wave, workgroup, ONE
//                       integer atomic add per workgroup (exact whatever the order).
//   k_cl_update<LDS>    per-cluster sums u64 [K][nbins] and counts: integer atomics, in LDS first while K * nbins <= CL_LDS_SUMS
//   k_cl_finalise       one lane per centroid: C = floor((S + floor(n_c / 2)) / n_c), an empty cluster keeps its centroid; zeroes S and the counts
//   k_cl_seed_dist<P>   one workgroup per contiguous chunk of rows: lowers `mind` against the newest centroid, writes the chunk's weight
//   k_cl_seed_pick      ONE workgroup: total W, r = (x * W) >> 64 from the round's Philox block, the chunk and then the row whose inclusive
//                       prefix sum first exceeds r; that row's q becomes centroid j.  W = 0: the lowest non-empty row.
// Launches are the only grid-wide barrier: no kernel waits for another workgroup.  Vector loads / stores, LDS, scalar loads and integer atomics
// only; no scratch memory (tests/test_hist_cluster_host.py reads the code objects).
#include <hip/hip_runtime.h>

#include "pk_device.hpp"
#include "pk_hist_cluster.hpp"

using namespace pk;

constexpr int CL_WAVES = CL_BLOCK / 64;
typedef unsigned long long cl_u64;                   // what atomicAdd takes

// |a.lo - b.lo| + |a.hi - b.hi| + acc over the u16 halves
__device__ __forceinline__ uint32_t cl_sad(uint32_t a, uint32_t b, uint32_t acc) {
#ifdef PK_HOST_SIM
    const int32_t l = (int32_t)(a & 0xffffu) - (int32_t)(b & 0xffffu), h = (int32_t)(a >> 16) - (int32_t)(b >> 16);
    return acc + (uint32_t)(l < 0 ? -l : l) + (uint32_t)(h < 0 ? -h : h);
#else
    return __builtin_amdgcn_sad_u16(a, b, acc);
#endif
}
__device__ __forceinline__ uint64_t cl_mulhi64(uint64_t a, uint64_t b) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}
// lane 0 of the wave gets the wave's sum (every lane of the wave takes part)
template <typename T> __device__ __forceinline__ T cl_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}
// every thread gets the workgroup's sum; wsum: CL_WAVES words of LDS, free again on return
__device__ __forceinline__ uint64_t cl_block_sum(uint64_t v, uint64_t *wsum) {
    const uint32_t tid = threadIdx.x;
    v = cl_wave_sum(v);
    if ((tid & 63u) == 0u) wsum[PK_IDX(tid >> 6, CL_WAVES, "wsum")] = v;
    __syncthreads();
    uint64_t total = 0;
#pragma unroll
    for (int w = 0; w < CL_WAVES; ++w) total += wsum[w];
    __syncthreads();
    return total;
}
// inclusive prefix sum over the workgroup's threads; total: the workgroup's sum
__device__ __forceinline__ uint64_t cl_block_scan(uint64_t v, uint64_t *wsum, uint64_t &total) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t y = __shfl_up(inc, off);
        inc += lane >= (uint32_t)off ? y : 0ull;
    }
    if (lane == 63u) wsum[PK_IDX(wave, CL_WAVES, "wsum")] = inc;
    __syncthreads();
    total = 0;
#pragma unroll
    for (int w = 0; w < CL_WAVES; ++w) {
        const uint64_t s = wsum[w];
        inc += (uint32_t)w < wave ? s : 0ull;
        total += s;
    }
    __syncthreads();
    return inc;
}
// The smallest index i < count whose inclusive prefix sum of weight(i) exceeds r (r < the total, so there is one), and the sum before it.
// sh: two words of LDS.  Every thread of the workgroup calls it and gets the same answer.
template <typename F>
__device__ __forceinline__ void cl_find(uint64_t count, uint64_t r, F weight, uint64_t *sh, uint64_t *wsum, uint64_t &idx, uint64_t &before) {
    const uint32_t tid = threadIdx.x;
    __syncthreads();
    if (tid == 0u) { sh[0] = ~0ull; sh[1] = 0; }
    __syncthreads();
    uint64_t base = 0;
    for (uint64_t t0 = 0; t0 < count; t0 += CL_BLOCK) {
        const uint64_t i = t0 + tid;
        const uint64_t v = i < count ? weight(i) : 0ull;
        uint64_t total;
        const uint64_t e = base + cl_block_scan(v, wsum, total) - v;
        if (v && e <= r && r - e < v) { sh[0] = i; sh[1] = e; }     // exactly one thread of exactly one tile
        __syncthreads();
        if (sh[0] != ~0ull) break;                                  // (the same word for every thread: the loop stays uniform)
        base += total;
    }
    idx = sh[0];
    before = sh[1];
}

__global__ void __launch_bounds__(CL_BLOCK) k_cl_quant(const uint16_t *__restrict__ hist, uint32_t *__restrict__ q, uint32_t nbins, uint64_t n) {
    __shared__ uint4 tile4[CL_BLOCK * CL_MAX_BINS / 8];              // a workgroup's rows: 16 KB
    uint16_t *tile = reinterpret_cast<uint16_t *>(tile4);
    const uint32_t tid = threadIdx.x, pairs = (nbins + 1u) >> 1;
    const bool aligned = ((uintptr_t)hist & 15u) == 0u;              // (a workgroup's piece starts 512 nbins bytes further on: aligned with the array)
    for (uint64_t row0 = (uint64_t)blockIdx.x * CL_BLOCK; row0 < n; row0 += (uint64_t)gridDim.x * CL_BLOCK) {
        const uint32_t rows = n - row0 < (uint64_t)CL_BLOCK ? (uint32_t)(n - row0) : (uint32_t)CL_BLOCK;
        const uint32_t words = rows * nbins, nvec = aligned ? words >> 3 : 0u;
        const uint16_t *src = hist + row0 * nbins;
        __syncthreads();                                             // (the tile before is done with)
        for (uint32_t i = tid; i < nvec; i += CL_BLOCK) tile4[PK_IDX(i, CL_BLOCK * CL_MAX_BINS / 8, "tile4")] = reinterpret_cast<const uint4 *>(src)[i];
        for (uint32_t i = (nvec << 3) + tid; i < words; i += CL_BLOCK) tile[PK_IDX(i, CL_BLOCK * CL_MAX_BINS, "tile")] = src[i];
        __syncthreads();
        if (tid < rows) {
            const uint16_t *h = tile + PK_IDX(tid * nbins, CL_BLOCK * CL_MAX_BINS - (nbins - 1u), "tile");   // h[0 .. nbins) lies inside the tile
            uint32_t mass = 0;
            for (uint32_t b = 0; b < nbins; ++b) mass += h[b];
            uint32_t cum = 0;
            uint32_t *out = q + (row0 + tid) * pairs;
            for (uint32_t p = 0; p < pairs; ++p) {
                uint32_t lo = 0, hi = 0;
                cum += h[2u * p];
                if (mass) lo = (uint32_t)(65535ull * cum / mass);
                if (2u * p + 1u < nbins) {
                    cum += h[2u * p + 1u];
                    if (mass) hi = (uint32_t)(65535ull * cum / mass);
                }
                out[p] = lo | (hi << 16);
            }
        }
    }
}

__global__ void __launch_bounds__(CL_BLOCK) k_cl_pack(const uint16_t *__restrict__ centroids, uint32_t *__restrict__ cp, uint32_t nbins, uint32_t K) {
    const uint32_t t = blockIdx.x * CL_BLOCK + threadIdx.x, c = t / CL_ROW_DWORDS, p = t % CL_ROW_DWORDS;
    if (c >= K) return;
    uint32_t v = 0;
    if (2u * p < nbins) v = centroids[(size_t)c * nbins + 2u * p];
    if (2u * p + 1u < nbins) v |= (uint32_t)centroids[(size_t)c * nbins + 2u * p + 1u] << 16;
    cp[t] = v;
}

// mode 0: no count of changes; 1: the first iteration, every non-empty row counts; 2: against the label the array holds
template <int P>
__global__ void __launch_bounds__(CL_BLOCK) k_cl_assign(const uint32_t *__restrict__ q, const uint32_t *__restrict__ cp, uint32_t K, uint64_t n,
                                                        uint16_t *__restrict__ label, uint32_t *__restrict__ dist, int mode,
                                                        uint32_t *__restrict__ changed, cl_u64 *__restrict__ inertia) {
    __shared__ uint64_t wsum[CL_WAVES];
    uint32_t ch = 0;
    uint64_t in = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * CL_BLOCK; base < n; base += (uint64_t)gridDim.x * CL_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < n;
        const uint32_t *row = q + (live ? i : n - 1u) * P;           // (a lane past the end reads the last row and writes nothing)
        uint32_t v[P];
#pragma unroll
        for (int p = 0; p < P; ++p) v[p] = row[p];
        uint32_t best = 0xFFFFFFFFu, bc = 0;
#pragma unroll 2
        for (uint32_t c = 0; c < K; ++c) {
            const uint32_t *cr = cp + (size_t)c * CL_ROW_DWORDS;     // uniform across the wave
            uint32_t d = 0;
#pragma unroll
            for (int p = 0; p < P; ++p) d = cl_sad(v[p], cr[p], d);
            if (d < best) { best = d; bc = c; }
        }
        if (live) {
            const bool empty = v[P - 1] == 0u;
            const uint32_t lab = empty ? CL_NONE : bc, dd = empty ? 0u : best;
            if (mode == 1) ch += empty ? 0u : 1u;
            else if (mode == 2) ch += (uint32_t)label[i] != lab ? 1u : 0u;
            in += dd;
            label[i] = (uint16_t)lab;
            if (dist) dist[i] = dd;
        }
    }
    if (!changed && !inertia) return;                                // (uniform: kernel arguments)
    const uint64_t tin = cl_block_sum(in, wsum), tch = cl_block_sum((uint64_t)ch, wsum);
    if (threadIdx.x == 0u) {
        if (inertia && tin) atomicAdd(inertia, (cl_u64)tin);
        if (changed && tch) atomicAdd(changed, (uint32_t)tch);
    }
}

template <bool LDS>
__global__ void __launch_bounds__(CL_BLOCK) k_cl_update(const uint32_t *__restrict__ q, const uint16_t *__restrict__ label, uint32_t nbins, uint32_t K,
                                                        uint64_t n, cl_u64 *__restrict__ sums, uint32_t *__restrict__ counts) {
    __shared__ cl_u64 ls[LDS ? CL_LDS_SUMS : 1];
    __shared__ uint32_t lc[LDS ? CL_LDS_SUMS : 1];
    const uint32_t tid = threadIdx.x, pairs = (nbins + 1u) >> 1;
    if (LDS) {
        for (uint32_t i = tid; i < K * nbins; i += CL_BLOCK) ls[PK_IDX(i, CL_LDS_SUMS, "ls")] = 0;
        for (uint32_t i = tid; i < K; i += CL_BLOCK) lc[PK_IDX(i, CL_LDS_SUMS, "lc")] = 0;
        __syncthreads();
    }
    for (uint64_t i = (uint64_t)blockIdx.x * CL_BLOCK + tid; i < n; i += (uint64_t)gridDim.x * CL_BLOCK) {
        const uint32_t lab = label[i];
        if (lab >= K) continue;                                      // (PK_CL_NONE: an empty row)
        const uint32_t *row = q + i * pairs;
        for (uint32_t p = 0; p < pairs; ++p) {                       // each packed dword is loaded once; one atomic per bin
            const uint32_t word = row[p];
            for (uint32_t b = 2u * p; b < 2u * p + 2u && b < nbins; ++b) {
                const cl_u64 val = (word >> ((b & 1u) << 4)) & 0xffffu;
                if (LDS) atomicAdd(&ls[PK_IDX(lab * nbins + b, CL_LDS_SUMS, "ls")], val);
                else atomicAdd(&sums[(size_t)lab * nbins + b], val);
            }
        }
        if (LDS) atomicAdd(&lc[PK_IDX(lab, CL_LDS_SUMS, "lc")], 1u);
        else atomicAdd(&counts[lab], 1u);
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = tid; i < K * nbins; i += CL_BLOCK) {
            const cl_u64 s = ls[PK_IDX(i, CL_LDS_SUMS, "ls")];
            if (s) atomicAdd(&sums[i], s);
        }
        for (uint32_t i = tid; i < K; i += CL_BLOCK) {
            const uint32_t c = lc[PK_IDX(i, CL_LDS_SUMS, "lc")];
            if (c) atomicAdd(&counts[i], c);
        }
    }
}

__global__ void __launch_bounds__(CL_BLOCK) k_cl_finalise(cl_u64 *__restrict__ sums, uint32_t *__restrict__ counts, uint16_t *__restrict__ centroids,
                                                          uint32_t *__restrict__ cp, uint32_t nbins, uint32_t K) {
    const uint32_t c = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (c >= K) return;
    const uint64_t nc = counts[c];
    if (!nc) return;                                                 // an empty cluster keeps its centroid (its sums are zero already)
    uint32_t word = 0;
    for (uint32_t b = 0; b < nbins; ++b) {
        const uint32_t v = (uint32_t)(((uint64_t)sums[(size_t)c * nbins + b] + (nc >> 1)) / nc);   // a rounded mean of u16 values: a u16
        sums[(size_t)c * nbins + b] = 0;
        centroids[(size_t)c * nbins + b] = (uint16_t)v;
        word |= v << ((b & 1u) << 4);
        if ((b & 1u) || b + 1u == nbins) { cp[(size_t)c * CL_ROW_DWORDS + (b >> 1)] = word; word = 0; }
    }
    counts[c] = 0;
}

// mode 0: the chunk's non-empty rows (round 0: every weight is 1); 1: mind = d(i, the centroid); 2: mind = min(mind, d(i, the centroid))
template <int P>
__global__ void __launch_bounds__(CL_BLOCK) k_cl_seed_dist(const uint32_t *__restrict__ q, const uint32_t *__restrict__ centroid, uint32_t *__restrict__ mind,
                                                           uint64_t *__restrict__ out, uint64_t n, uint64_t chunk, int mode) {
    __shared__ uint64_t wsum[CL_WAVES];
    const uint64_t row0 = (uint64_t)blockIdx.x * chunk;
    uint64_t sum = 0;
    for (uint64_t off = threadIdx.x; off < chunk; off += CL_BLOCK) {
        const uint64_t i = row0 + off;
        if (i >= n) continue;
        uint32_t v[P];
#pragma unroll
        for (int p = 0; p < P; ++p) v[p] = q[i * P + p];
        const bool empty = v[P - 1] == 0u;
        if (mode == 0) { sum += empty ? 0u : 1u; continue; }
        uint32_t d = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) d = cl_sad(v[p], centroid[p], d);
        if (mode == 2) { const uint32_t old = mind[i]; d = old < d ? old : d; }
        d = empty ? 0u : d;
        mind[i] = d;
        sum += d;
    }
    const uint64_t total = cl_block_sum(sum, wsum);
    if (threadIdx.x == 0u) out[blockIdx.x] = total;
}

__global__ void __launch_bounds__(CL_BLOCK) k_cl_seed_pick(const uint32_t *__restrict__ q, const uint32_t *__restrict__ mind, const uint64_t *__restrict__ part,
                                                           const uint64_t *__restrict__ rows, uint32_t nchunks, uint64_t chunk, uint64_t n, uint32_t j,
                                                           uint32_t key0, uint32_t key1, uint32_t nonce, uint32_t nbins, uint16_t *__restrict__ centroids,
                                                           uint32_t *__restrict__ cp) {
    __shared__ uint64_t wsum[CL_WAVES];
    __shared__ uint64_t sh[2];
    const uint32_t tid = threadIdx.x, pairs = (nbins + 1u) >> 1;
    uint64_t W = 0;
    if (j) {
        uint64_t s = 0;
        for (uint32_t g = tid; g < nchunks; g += CL_BLOCK) s += part[g];
        W = cl_block_sum(s, wsum);
    }
    const bool by_rows = W == 0;                                     // round 0, or every non-empty row coincides with a centroid
    if (by_rows) {
        uint64_t s = 0;
        for (uint32_t g = tid; g < nchunks; g += CL_BLOCK) s += rows[g];
        W = cl_block_sum(s, wsum);
        if (W == 0) return;                                          // no non-empty row at all (the host forms refuse such a call)
    }
    uint32_t w[4];
    philox4x32_10(j, 0u, STREAM_CLS, nonce, key0, key1, w);
    const uint64_t x = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    const uint64_t r = by_rows && j ? 0ull : cl_mulhi64(x, W);
    const uint64_t *arr = by_rows ? rows : part;
    uint64_t g, before;
    cl_find((uint64_t)nchunks, r, [&](uint64_t c) { return arr[c]; }, sh, wsum, g, before);
    if (g >= (uint64_t)nchunks) return;                              // (cannot happen: r < W; nothing is read or written past an array if it did)
    const uint64_t row0 = g * chunk, cnt = n - row0 < chunk ? n - row0 : chunk;
    uint64_t i, unused;
    cl_find(cnt, r - before, [&](uint64_t o) { return by_rows ? (uint64_t)(q[(row0 + o) * pairs + pairs - 1u] != 0u) : (uint64_t)mind[row0 + o]; }, sh, wsum, i,
            unused);
    if (i >= cnt) return;
    if (tid < (uint32_t)CL_ROW_DWORDS) {
        const uint32_t v = tid < pairs ? q[(row0 + i) * pairs + tid] : 0u;
        cp[(size_t)j * CL_ROW_DWORDS + tid] = v;
        if (2u * tid < nbins) centroids[(size_t)j * nbins + 2u * tid] = (uint16_t)v;
        if (2u * tid + 1u < nbins) centroids[(size_t)j * nbins + 2u * tid + 1u] = (uint16_t)(v >> 16);
    }
}

namespace pk {

static size_t cl_al(size_t b) { return (b + 255) & ~(size_t)255; }

size_t cl_work_bytes(size_t n, int nbins, int K, bool seeding, bool update) {
    size_t t = cl_al(n * (size_t)cl_pairs(nbins) * 4) + cl_al((size_t)K * CL_ROW_DWORDS * 4);
    if (seeding) t += cl_al(n * 4) + 2 * cl_al(cl_chunks(n) * 8);
    if (update) t += cl_al((size_t)K * nbins * 8 + (size_t)K * 4);
    return t;
}

ClWork cl_work(void *base, size_t n, int nbins, int K, bool seeding, bool update) {
    char *p = (char *)base;
    ClWork w{};
    w.q = (uint32_t *)p; p += cl_al(n * (size_t)cl_pairs(nbins) * 4);
    w.cp = (uint32_t *)p; p += cl_al((size_t)K * CL_ROW_DWORDS * 4);
    if (seeding) {
        w.mind = (uint32_t *)p; p += cl_al(n * 4);
        w.part = (uint64_t *)p; p += cl_al(cl_chunks(n) * 8);
        w.rows = (uint64_t *)p; p += cl_al(cl_chunks(n) * 8);
    }
    if (update) {                                                    // sums and counts: one piece, zeroed with one fill
        w.sums = (uint64_t *)p;
        w.counts = (uint32_t *)(p + (size_t)K * nbins * 8);
    }
    return w;
}

static unsigned cl_grid(size_t n) {
    const size_t g = (n + CL_BLOCK - 1) / CL_BLOCK;
    return (unsigned)(g < (size_t)CL_GRID_MAX ? g : (size_t)CL_GRID_MAX);
}

static hipError_t cl_quant_launch(hipStream_t stream, size_t n, int nbins, const uint16_t *hist, uint32_t *q) {
    hipLaunchKernelGGL(k_cl_quant, dim3(cl_grid(n)), dim3(CL_BLOCK), 0, stream, hist, q, (uint32_t)nbins, (uint64_t)n);
    return hipGetLastError();
}

static hipError_t cl_pack_launch(hipStream_t stream, int nbins, int K, const uint16_t *centroids, uint32_t *cp) {
    hipLaunchKernelGGL(k_cl_pack, dim3((unsigned)((K * CL_ROW_DWORDS + CL_BLOCK - 1) / CL_BLOCK)), dim3(CL_BLOCK), 0, stream, centroids, cp, (uint32_t)nbins,
                       (uint32_t)K);
    return hipGetLastError();
}

template <int P>
static void cl_assign_p(hipStream_t stream, size_t n, int K, const ClWork &w, uint16_t *label, uint32_t *dist, int mode, uint32_t *changed, uint64_t *inertia) {
    hipLaunchKernelGGL(k_cl_assign<P>, dim3(cl_grid(n)), dim3(CL_BLOCK), 0, stream, (const uint32_t *)w.q, (const uint32_t *)w.cp, (uint32_t)K, (uint64_t)n, label,
                       dist, mode, changed, (cl_u64 *)inertia);
}
template <int P>
static void cl_seed_dist_p(hipStream_t stream, size_t n, const ClWork &w, const uint32_t *centroid, uint64_t *out, int mode) {
    hipLaunchKernelGGL(k_cl_seed_dist<P>, dim3((unsigned)cl_chunks(n)), dim3(CL_BLOCK), 0, stream, (const uint32_t *)w.q, centroid, w.mind, out, (uint64_t)n,
                       (uint64_t)cl_chunk_rows(n), mode);
}
#define CL_PAIRS_DISPATCH(pairs, call)                                                                                                \
    switch (pairs) {                                                                                                                  \
        case 1: call(1); break; case 2: call(2); break; case 3: call(3); break; case 4: call(4); break;                               \
        case 5: call(5); break; case 6: call(6); break; case 7: call(7); break; case 8: call(8); break;                               \
        case 9: call(9); break; case 10: call(10); break; case 11: call(11); break; case 12: call(12); break;                         \
        case 13: call(13); break; case 14: call(14); break; case 15: call(15); break; case 16: call(16); break;                       \
        default: return hipErrorInvalidValue;                                                                                         \
    }

static hipError_t cl_assign_pass(hipStream_t stream, size_t n, int nbins, int K, const ClWork &w, uint16_t *label, uint32_t *dist, int mode, uint32_t *changed,
                                 uint64_t *inertia) {
#define CL_CALL(P) cl_assign_p<P>(stream, n, K, w, label, dist, mode, changed, inertia)
    CL_PAIRS_DISPATCH(cl_pairs(nbins), CL_CALL)
#undef CL_CALL
    return hipGetLastError();
}

hipError_t cl_seed_launch(hipStream_t stream, size_t n, int nbins, const uint16_t *hist, int K, uint32_t key0, uint32_t key1, uint32_t nonce,
                          uint16_t *centroids, const ClWork &w) {
    hipError_t e = cl_quant_launch(stream, n, nbins, hist, w.q);
    if (e != hipSuccess) return e;
    const uint32_t nchunks = (uint32_t)cl_chunks(n);
    for (int j = 0; j < K; ++j) {                                    // two launches per round
        const uint32_t *newest = j ? w.cp + (size_t)(j - 1) * CL_ROW_DWORDS : nullptr;
        uint64_t *out = j ? w.part : w.rows;
        const int mode = j == 0 ? 0 : (j == 1 ? 1 : 2);
#define CL_CALL(P) cl_seed_dist_p<P>(stream, n, w, newest, out, mode)
        CL_PAIRS_DISPATCH(cl_pairs(nbins), CL_CALL)
#undef CL_CALL
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_cl_seed_pick, dim3(1), dim3(CL_BLOCK), 0, stream, (const uint32_t *)w.q, (const uint32_t *)w.mind, (const uint64_t *)w.part,
                           (const uint64_t *)w.rows, nchunks, (uint64_t)cl_chunk_rows(n), (uint64_t)n, (uint32_t)j, key0, key1, nonce, (uint32_t)nbins, centroids,
                           w.cp);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t cl_assign_launch(hipStream_t stream, size_t n, int nbins, const uint16_t *hist, int K, const uint16_t *centroids, uint16_t *label,
                            uint32_t *dist, const ClWork &w) {
    hipError_t e = cl_quant_launch(stream, n, nbins, hist, w.q);
    if (e == hipSuccess) e = cl_pack_launch(stream, nbins, K, centroids, w.cp);
    if (e == hipSuccess) e = cl_assign_pass(stream, n, nbins, K, w, label, dist, 0, nullptr, nullptr);
    return e;
}

hipError_t cl_cluster_launch(hipStream_t stream, size_t n, int nbins, const uint16_t *hist, int K, uint16_t *centroids, int iters, uint16_t *label,
                             uint32_t *dist, uint64_t *inertia, uint32_t *changed, const ClWork &w) {
    hipError_t e = cl_quant_launch(stream, n, nbins, hist, w.q);
    if (e == hipSuccess) e = cl_pack_launch(stream, nbins, K, centroids, w.cp);
    if (e == hipSuccess) e = hipMemsetAsync(w.sums, 0, (size_t)K * nbins * 8 + (size_t)K * 4, stream);
    if (e == hipSuccess && inertia) e = hipMemsetAsync(inertia, 0, (size_t)(iters + 1) * 8, stream);
    if (e == hipSuccess && changed) e = hipMemsetAsync(changed, 0, (size_t)iters * 4, stream);
    const bool lds = (size_t)K * nbins <= (size_t)CL_LDS_SUMS;
    const unsigned ugrid = lds ? (cl_grid(n) < 256u ? cl_grid(n) : 256u) : cl_grid(n);   // (every workgroup of the LDS form flushes K * nbins sums)
    for (int t = 0; t < iters && e == hipSuccess; ++t) {             // three launches per iteration
        e = cl_assign_pass(stream, n, nbins, K, w, label, nullptr, t == 0 ? 1 : 2, changed ? changed + t : nullptr, inertia ? inertia + t : nullptr);
        if (e != hipSuccess) break;
        if (lds) hipLaunchKernelGGL(k_cl_update<true>, dim3(ugrid), dim3(CL_BLOCK), 0, stream, (const uint32_t *)w.q, (const uint16_t *)label, (uint32_t)nbins,
                                    (uint32_t)K, (uint64_t)n, (cl_u64 *)w.sums, w.counts);
        else hipLaunchKernelGGL(k_cl_update<false>, dim3(ugrid), dim3(CL_BLOCK), 0, stream, (const uint32_t *)w.q, (const uint16_t *)label, (uint32_t)nbins,
                                (uint32_t)K, (uint64_t)n, (cl_u64 *)w.sums, w.counts);
        if ((e = hipGetLastError()) != hipSuccess) break;
        hipLaunchKernelGGL(k_cl_finalise, dim3((unsigned)((K + CL_BLOCK - 1) / CL_BLOCK)), dim3(CL_BLOCK), 0, stream, (cl_u64 *)w.sums, w.counts, centroids, w.cp,
                           (uint32_t)nbins, (uint32_t)K);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = cl_assign_pass(stream, n, nbins, K, w, label, dist, 0, nullptr, inertia ? inertia + iters : nullptr);
    return e;
}

}  // namespace pk
