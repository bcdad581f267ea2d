// pk_equity_sampled.hpp -- showdown equity by Monte Carlo sampling for spots with hidden hole cards (include/pokerl_hip.h "Sampled showdown
// equity"): what the host entry points (pk_api.hip) and the kernels (pk_equity_sampled.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_equity.hpp"

namespace pk {

constexpr uint32_t STREAM_EQS = 0x45515330u;            // 'EQS0' (+ block b = 0, 1, 2): the sampled equity's own Philox stream
constexpr uint32_t EQS_SAMPLES_MAX = 1u << 24;          // samples per call and spot at most (more: further calls with other nonces, counts add)
constexpr int EQS_LPT_MIN = 8, EQS_LPT_MAX = 1024;      // samples per lane and task
static_assert((uint64_t)EQS_LPT_MAX * EQ_SHARE_UNIT < (1ull << 32), "a lane's 32-bit share sum must hold EQS_LPT_MAX samples of a sole winner");
constexpr uint32_t EQS_TASKS_TARGET = 16384;            // tasks a call is cut into where its size allows: two per resident wavefront

// A spot's descriptor: 4 + N 64-bit words, written by k_eqs_prep.
//   [0] known board cards, [4 + p] seat p's KNOWN hole cards: suit-lane bit sets OR(4 << Card.value), what eval7_tab_front_bits takes
//   [1] the pool: bit c set = the card of canonical index c (rank0 * 4 + suit) is not dead
//   [2] hidden hole bytes (bit 2p + b: byte b of live seat p is drawn) | live << 32 | k << 48 | P << 56   (k = 5 - nb board cards to draw)
//   [3] stream id | valid << 32   (valid = 0: a refused spot, no samples)
constexpr int eqs_desc_words(int N) { return 4 + N; }
inline size_t eqs_work_bytes(int N, size_t m) { return m * (size_t)eqs_desc_words(N) * 8; }

// Samples per lane and task: every valid spot of a call is cut into the SAME number of tasks ceil(S / (64 * lpt)) of one wavefront each, so
// task -> (spot, chunk) is a division.  Small calls are cut finely (a lone spot must spread over every CU), large ones coarsely.
int eqs_lpt(size_t m, uint32_t samples);
// m * ceil(samples / 64), the bound on the task count the entry points check against 32 bits
inline uint64_t eqs_task_bound(size_t m, uint32_t samples) { return (uint64_t)m * (((uint64_t)samples + 63) / 64); }

struct EqsOut {           // any may be NULL
    uint32_t *win, *tie;
    uint64_t *share;
    uint32_t *samples;
    uint8_t *status;
};
struct EqsStream {        // Philox key, the call's nonce and sample count; ids: NULL = id_base + (spot index | table index)
    uint32_t key0, key1, nonce, samples, id_base;
    const uint32_t *ids;
};

// Queues the whole call on `stream`: descriptors + zeroed outputs (one lane per spot), then the persistent sampling kernel.  tab: the
// evaluator table (eval7_table); `tables` non-NULL selects the table form, whose `observer` is a seat, PK_OBSERVER_ACTIVE or PK_OBSERVER_NONE.
hipError_t eqs_launch(hipStream_t stream, const uint32_t *tab, const EqSpots *spots, const EqTables *tables, int observer, const EqsStream &rng,
                      int N, size_t m, const EqsOut &out, uint64_t *desc);

}  // namespace pk
