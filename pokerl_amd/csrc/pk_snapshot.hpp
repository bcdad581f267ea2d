// pk_snapshot.hpp -- table snapshots (include/pokerl_hip.h "Snapshots"): the blob layout, shared by the host entry
// points (pk_api.hip) and the save / check / load / clone kernels (pk_snapshot.hip).  The existing table kernels do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pk_device.hpp"

namespace pk {

constexpr uint32_t SNAP_MAGIC = 0x4E534B50u;      // "PKSN" in the first four bytes of a blob
constexpr uint32_t SNAP_VERSION = 1;
constexpr uint32_t STREAM_REDEAL = 0x52444C30u;   // 'RDL0' (RNG spec of the redeal: DESIGN.md section 3)
constexpr size_t SNAP_HEADER_BYTES = 256;

// refusal word of k_snap_check_idx / k_snap_check (one bit per reason; SNAP_OVERLAP is no refusal)
enum : uint32_t {
    SNAP_BAD_SRC_INDEX = 1, SNAP_BAD_DST_INDEX = 2, SNAP_DUP_DST = 4, SNAP_BAD_CURSOR = 8, SNAP_BAD_SEATS = 16, SNAP_BAD_CARD = 32,
    SNAP_BAD_MONEY = 64, SNAP_BAD_VALID = 128, SNAP_OVERLAP = 1u << 31,
};

struct SnapHeader {   // the first SNAP_HEADER_BYTES of a blob
    uint32_t magic, version, num_players, reserved;
    uint64_t m;
    double start_credits[PK_MAX_PLAYERS];
    double big_blind, small_blind;
    uint64_t pad[(SNAP_HEADER_BYTES - 24 - 8 * PK_MAX_PLAYERS - 16) / 8];
};
static_assert(sizeof(SnapHeader) == SNAP_HEADER_BYTES, "snapshot header size");

// The fields of one table record, as arrays of `stride` elements per row: a handle's State (stride T, rows = seats / card words) or a
// blob (stride m).  owed .. env_rew exist in a State only (NULL in a blob): a store into a State writes zeros there.
struct SnapView {
    double *credits, *bets, *pending, *payoffs, *min_raise;
    uint64_t *seat_states, *hand_serial, *step_serial;
    uint32_t *cursors;
    int32_t *hand;
    uint32_t *cards, *show;
    uint8_t *valid, *terr;
    uint32_t *owed, *mid;
    uint64_t *env_ctx;
    double *env_rew;
    size_t stride;
};

__host__ __device__ inline size_t snap_align(size_t x) { return (x + 255) & ~(size_t)255; }

constexpr int SNAP_FIELDS = 14;
struct SnapPads { uint64_t begin[SNAP_FIELDS], end[SNAP_FIELDS]; };   // the alignment gap after each field array (< 256 bytes): zeroed by a save

// ONE description of the blob, run with base == NULL to measure it (pk_snapshot_bytes) and with a base to hand out the field pointers:
// the header, then the records field-major, each field array 256-byte aligned, per-seat fields [N][m], cards [W][m] words.
inline size_t snap_layout(int N, size_t m, char *base, SnapView *v, SnapPads *pads = nullptr) {
    const size_t W = (size_t)(5 + 2 * N + 3) / 4;
    size_t off = SNAP_HEADER_BYTES;
    int f = 0;
    auto take = [&](size_t bytes) {
        void *r = base ? (void *)(base + off) : nullptr;
        if (pads) { pads->begin[f] = off + bytes; pads->end[f] = off + snap_align(bytes); }
        ++f;
        off += snap_align(bytes);
        return r;
    };
    SnapView s{};
    s.credits = (double *)take((size_t)N * m * 8); s.bets = (double *)take((size_t)N * m * 8);
    s.pending = (double *)take((size_t)N * m * 8); s.payoffs = (double *)take((size_t)N * m * 8);
    s.min_raise = (double *)take(m * 8);
    s.seat_states = (uint64_t *)take(m * 8);
    s.hand_serial = (uint64_t *)take(m * 8); s.step_serial = (uint64_t *)take(m * 8);
    s.cursors = (uint32_t *)take(m * 4); s.hand = (int32_t *)take(m * 4);
    s.cards = (uint32_t *)take(W * m * 4);
    s.show = (uint32_t *)take((size_t)N * m * 4);
    s.valid = (uint8_t *)take(m); s.terr = (uint8_t *)take(m);
    s.stride = m;
    if (v) *v = s;
    return off;
}

inline SnapView snap_view_of_state(const State &S) {
    SnapView v{};
    v.credits = S.credits; v.bets = S.bets; v.pending = S.pending; v.payoffs = S.payoffs; v.min_raise = S.min_raise;
    v.seat_states = S.seat_states; v.hand_serial = S.hand_serial; v.step_serial = S.step_serial;
    v.cursors = S.cursors; v.hand = S.hand; v.cards = S.cards; v.show = S.show; v.valid = S.valid; v.terr = S.terr;
    v.owed = S.owed; v.mid = S.mid; v.env_ctx = S.env_ctx; v.env_rew = S.env_rew;
    v.stride = (size_t)S.T;
    return v;
}

// The redeal of a clone: observer >= 0 that seat, PK_OBSERVER_ACTIVE each record's active player, PK_OBSERVER_NONE none (an exact copy).
struct Redeal {
    int observer;
    uint32_t key0, key1, table_id_base;   // the DESTINATION handle's key and table ids
    uint64_t nonce;
};

enum : int { SNAP_KIND_SAVE = 0, SNAP_KIND_LOAD = 1, SNAP_KIND_CLONE = 2 };
// Launchers (pk_snapshot.hip), asynchronous on `stream`.  src_idx / dst_idx: NULL = record i is table i (a blob view always takes NULL).
// kind SAVE also writes `header` into the blob's first bytes, which dst_blob points to, and zeroes its alignment gaps (`pads`): equal
// tables give equal blobs, byte for byte.
hipError_t snap_copy(hipStream_t stream, int kind, const SnapView &src, const int32_t *src_idx, const SnapView &dst, const int32_t *dst_idx,
                     int N, size_t m, const Redeal &rd, const SnapHeader &header, void *dst_blob, const SnapPads &pads);
// Index check: every idx[i] (NULL: i) must lie in [0, T), else `bad` is OR-ed into *word.  mark != NULL, mode 0: counts each table in
// mark[] (a table counted twice: SNAP_DUP_DST); mode 1: SNAP_OVERLAP if a table is marked already.
hipError_t snap_check_idx(hipStream_t stream, const int32_t *idx, size_t m, int T, uint32_t *mark, int mode, uint32_t bad, uint32_t *word);
// Record check of a blob's m records before a load: the record reasons of the refusal word.
hipError_t snap_check_records(hipStream_t stream, const SnapView &src, int N, size_t m, uint32_t *word);

}  // namespace pk
