// pk_preflop.hpp -- pre-flop hand strength: the exact hero-versus-holding matchup table over all C(52, 5) boards, counted on the device, and the
// pre-flop range equity / range vs range that read it (include/pokerl_hip.h "Pre-flop matchups"): what the host entry
// points (pk_api.hip) and the kernels (pk_preflop.hip) share.  The table kernels do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_equity.hpp"

namespace pk {

constexpr int PFM_HOLDINGS = PK_EQ_HOLDINGS;             // C(52, 2) unordered pairs: h = b (b - 1) / 2 + a, canonical indices a < b
constexpr uint32_t PFM_BOARDS = PK_PREFLOP_ALL_BOARDS;   // C(52, 5): the 5-subsets of canonical indices in lexicographic order
constexpr size_t PFM_CELLS = (size_t)PFM_HOLDINGS * PFM_HOLDINGS;   // entries of one [1326][1326] array
// ---- the count pass (k_pfm_count): a workgroup owns a PFM_TILE x PFM_TILE tile of (hero x villain) holdings, a lane an 8 x 8 block of it
constexpr int PFM_TILE = 128;
constexpr int PFM_STRIPS = (PFM_HOLDINGS + PFM_TILE - 1) / PFM_TILE;   // 11 strips of holdings; 11 x 11 tiles
constexpr int PFM_STRIDE = PFM_STRIPS * PFM_TILE;        // keys per board in the work space: 1408, the last 82 sentinels (no strip load tests a bound)
constexpr int PFM_RUN = 32;                              // boards whose two key strips a workgroup stages in LDS at a time (2 x 16 KB)
constexpr int PFM_COUNT_BLOCK = 256;                     // 16 x 16 lanes
constexpr int PFM_SLICES = 16;                           // board slices of a chunk: the grid is tiles x slices
constexpr uint32_t PFM_COUNT_LDS = 2u * PFM_RUN * PFM_TILE * 4u;
// ---- the rank pass (k_pfm_rank): a workgroup ranks every holding on PFM_RANK_BOARDS boards
constexpr int PFM_RANK_BLOCK = 256;
constexpr int PFM_RANK_BOARDS = 32;
constexpr int PFM_RANK_PER_LANE = (PFM_STRIDE + PFM_RANK_BLOCK - 1) / PFM_RANK_BLOCK;   // 6 key slots of a board per lane
// ---- the chunk: boards per work-space fill (knob PK_PFM_CHUNK)
constexpr int PFM_CHUNK_DEFAULT = 16384, PFM_CHUNK_MAX = 65536;
constexpr uint32_t PFM_SENT = 0xFFFFFFFFu;               // the key of a holding that is out of play on a board (real keys have 24 bits and are not 0)
inline size_t pfm_keys_bytes(uint32_t chunk) { return (size_t)chunk * PFM_STRIDE * sizeof(uint32_t); }
// boards per slice of a chunk of `chunk` boards: a multiple of PFM_RUN, at most PFM_SLICES slices
inline uint32_t pfm_slice_boards(uint32_t chunk) {
    const uint32_t per = (chunk + PFM_SLICES - 1) / PFM_SLICES;
    return (per + PFM_RUN - 1) / PFM_RUN * PFM_RUN;
}
// ---- the readers (k_pfm_hero, k_pfm_rvr)
constexpr int PFM_READ_BLOCK = 256, PFM_READ_WAVES = PFM_READ_BLOCK / 64;
constexpr int PFM_READ_PER_LANE = (PFM_HOLDINGS + PFM_READ_BLOCK - 1) / PFM_READ_BLOCK;   // 6 villain holdings per lane: o = tid + 256 j
constexpr int PFM_HERO_GRID_MAX = 2048;
constexpr int PFM_RVR_ROWS = 2;                          // matrix rows (hero holdings) a workgroup of k_pfm_rvr keeps in registers
constexpr uint32_t PFM_NO_HOLDING = 0xFFFFFFFFu;         // descriptor of a refused spot
inline size_t pfm_desc_bytes(size_t m) { return m * sizeof(uint32_t); }

struct PfmOut {           // any may be NULL
    uint64_t *agg;
    uint32_t *win, *tie, *boards;
    uint8_t *status;
};
struct PfmWeights {
    const uint16_t *w;       // NULL: every weight is 1
    int per_spot;            // 0: one vector [1326] for the call, 1: [m][1326]
};

// Partial counts over boards [first, first + n), n > 0, first + n <= PFM_BOARDS, queued on `stream`: per chunk the rank pass fills `keys`
// (pfm_keys_bytes(chunk)), the count pass adds the chunk's counts to win / tie ([1326][1326] each, either may be NULL).  accumulate == 0:
// the arrays are overwritten (the first slice of boards is STORED by a launch of its own, every later one added).
hipError_t pfm_count_launch(hipStream_t stream, const uint32_t *tab, uint32_t first, uint32_t n, int accumulate, uint32_t chunk, uint32_t *keys,
                            uint32_t *win, uint32_t *tie);
// Pre-flop range equity of m > 0 spots: descriptors + boards / status (one lane per spot; `tables` non-NULL selects the table form), then --
// where agg, win or tie is wanted -- the gather.  M: the resident table (win, then tie).
hipError_t pfm_hero_launch(hipStream_t stream, const uint32_t *M, const uint8_t *hero, const EqTables *tables, int N, int observer,
                           const PfmWeights &weights, size_t m, const PfmOut &out, uint32_t *desc);
// Pre-flop range vs range of m > 0 weight rows (weights NULL: ones): win / tie / tot u64 [m][1326], any may be NULL.
hipError_t pfm_rvr_launch(hipStream_t stream, const uint32_t *M, const uint16_t *weights, size_t m, uint64_t *win, uint64_t *tie, uint64_t *tot);

}  // namespace pk
