// pk_snapshot.hip -- the kernels of the table snapshots (save, check, load, clone with an optional redeal) and their launchers; the C entry
// points that drive them are in pk_api.hip, the blob layout in pk_snapshot.hpp.  Memory-bound gathers and scatters: N is a run-time
// argument (no per-seat instantiations), one record per lane, every access one word per lane along the record index -- for a clone the
// DESTINATION index, so a 1 -> T fan-out reads its one source record out of L2 and writes T records as coalesced stores.  Ordinary vector
// stores only; no scratch memory (tests/test_snapshot_host.py reads the code objects).
#include <hip/hip_runtime.h>

#include "pk_snapshot.hpp"

using namespace pk;

#define SNAP_BLOCK 256
constexpr int SNAP_MAX_WORDS = (5 + 2 * PK_MAX_PLAYERS + 3) / 4;   // deck words of a record at 16 seats

struct SnapCopyArgs {
    SnapView src, dst;
    const int32_t *src_idx, *dst_idx;   // NULL: record i is table i
    int N;
    size_t m;
    Redeal rd;
};

// Not inf / NaN, by the bits (the library is built with -fno-honor-nans, under which isfinite may fold to true)
__device__ __forceinline__ bool finite_bits(double x) { return ((__double_as_longlong(x) >> 52) & 0x7ff) != 0x7ff; }

// The k-th (0-based) set bit of m; k < popcount(m)
__device__ __forceinline__ uint32_t select_bit(uint64_t m, uint32_t k) {
    uint32_t base = 0, w = (uint32_t)m, n = (uint32_t)__popc(w);
    if (k >= n) { k -= n; w = (uint32_t)(m >> 32); base = 32; }
    n = (uint32_t)__popc(w & 0xffffu); if (k >= n) { k -= n; w >>= 16; base += 16; }
    n = (uint32_t)__popc(w & 0xffu); if (k >= n) { k -= n; w >>= 8; base += 8; }
    n = (uint32_t)__popc(w & 0xfu); if (k >= n) { k -= n; w >>= 4; base += 4; }
    n = (uint32_t)__popc(w & 0x3u); if (k >= n) { k -= n; w >>= 2; base += 2; }
    return base + ((k >= (w & 1u)) ? 1u : 0u);
}

// The redeal of one record's deck words, in registers (spec: DESIGN.md section 3).  Visible to the observer p: the board deck[0:nb] and
// p's hole cards; every other slot of deck[0:5+2N], in ascending position (board nb..4, then the hole cards of each other seat), is
// refilled by a draw without replacement from the 52 - nb - 2 cards p has not seen, the i-th from the c_i-th remaining one in
// canonical order.  Positions are compile-time constants (PK_FOR): the deck never leaves registers.
__device__ __forceinline__ void redeal(uint32_t (&cw)[SNAP_MAX_WORDS], int N, uint32_t cursors, const Redeal &rd, uint32_t table_id) {
    const int K = 5 + 2 * N;
    const int turn = (int)Cursor{cursors}.turn(), active = (int)Cursor{cursors}.active();
    const int p = rd.observer >= 0 ? rd.observer : active;
    const int nb = turn == 0 ? 0 : (turn + 2 < 5 ? turn + 2 : 5);   // game.py:266-278
    const int h0 = 5 + 2 * p;
    uint64_t seen = 0;
    uint32_t any = 0;
    PK_FOR(w, SNAP_MAX_WORDS)
        PK_FOR(b, 4)
            constexpr int pos = 4 * w + b;
            const uint32_t v = (cw[w] >> (8 * b)) & 0xffu;
            const bool vis = pos < K && (pos < nb || pos == h0 || pos == h0 + 1);
            seen |= vis ? (1ull << (((v & 15u) * 4u + (v >> 4)) & 63u)) : 0ull;   // canonical index of Card.value v (cards.py:77)
            any |= pos < K ? v : 0u;
        PK_END
    PK_END
    if (any == 0) return;   // a table never dealt (all 5+2N bytes zero, as pk_create leaves it): nothing hidden to redeal, copied as it is
    uint64_t rem = 0x000FFFFFFFFFFFFFull & ~seen;
    const uint64_t P = (uint64_t)(52 - nb - 2);
    uint32_t b0[4], b1[4];
    philox4x32_10(table_id, (uint32_t)rd.nonce, STREAM_REDEAL, (uint32_t)(rd.nonce >> 32), rd.key0, rd.key1, b0);
    philox4x32_10(table_id, (uint32_t)rd.nonce, STREAM_REDEAL + 1u, (uint32_t)(rd.nonce >> 32), rd.key0, rd.key1, b1);
    // the words X[0..3] as a queue (each is taken once, in order: a select by index would be folded into a scratch array)
    uint64_t X0 = (uint64_t)b0[0] | ((uint64_t)b0[1] << 32), X1 = (uint64_t)b0[2] | ((uint64_t)b0[3] << 32);
    uint64_t X2 = (uint64_t)b1[0] | ((uint64_t)b1[1] << 32), X3 = (uint64_t)b1[2] | ((uint64_t)b1[3] << 32);
    uint32_t i = 0;
    uint64_t x = 0;
    PK_FOR(w, SNAP_MAX_WORDS)
        PK_FOR(b, 4)
            constexpr int pos = 4 * w + b;
            const bool hidden = pos < K && !(pos < nb || pos == h0 || pos == h0 + 1);
            if (hidden) {
                if (i % 9u == 0) { x = X0; X0 = X1; X1 = X2; X2 = X3; }   // at most 35 draws: two blocks
                const uint64_t bound = P - i;
                const uint32_t c = (uint32_t)__umul64hi(x, bound);
                x = x * bound;
                const uint32_t k = select_bit(rem, c);
                rem &= ~(1ull << k);
                const uint32_t v = ((k & 3u) << 4) | (k >> 2);
                cw[w] = (cw[w] & ~(0xffu << (8 * b))) | (v << (8 * b));
                ++i;
            }
        PK_END
    PK_END
}

template <bool REDEAL>
__device__ __forceinline__ void copy_record(const SnapCopyArgs &a) {
    const size_t i = (size_t)blockIdx.x * SNAP_BLOCK + threadIdx.x;
    if (i >= a.m) return;
    const size_t s = a.src_idx ? (size_t)a.src_idx[i] : i;
    const size_t d = a.dst_idx ? (size_t)a.dst_idx[i] : i;
    const size_t ss = a.src.stride, ds = a.dst.stride;
    const int N = a.N, W = (5 + 2 * N + 3) / 4;
    for (int p = 0; p < N; ++p) {
        const double c = a.src.credits[p * ss + s], b = a.src.bets[p * ss + s], pe = a.src.pending[p * ss + s], po = a.src.payoffs[p * ss + s];
        const uint32_t sh = a.src.show[p * ss + s];
        a.dst.credits[p * ds + d] = c; a.dst.bets[p * ds + d] = b; a.dst.pending[p * ds + d] = pe; a.dst.payoffs[p * ds + d] = po;
        a.dst.show[p * ds + d] = sh;
    }
    const uint32_t cur = a.src.cursors[s];
    a.dst.min_raise[d] = a.src.min_raise[s];
    a.dst.seat_states[d] = a.src.seat_states[s];
    a.dst.hand_serial[d] = a.src.hand_serial[s];
    a.dst.step_serial[d] = a.src.step_serial[s];
    a.dst.cursors[d] = cur;
    a.dst.hand[d] = a.src.hand[s];
    a.dst.valid[d] = a.src.valid[s];
    a.dst.terr[d] = a.src.terr[s];
    if (REDEAL && a.rd.observer != PK_OBSERVER_NONE) {
        uint32_t cw[SNAP_MAX_WORDS];
        PK_FOR(w, SNAP_MAX_WORDS) cw[w] = w < W ? a.src.cards[w * ss + s] : 0u; PK_END
        redeal(cw, N, cur, a.rd, a.rd.table_id_base + (uint32_t)d);
        PK_FOR(w, SNAP_MAX_WORDS) if (w < W) a.dst.cards[w * ds + d] = cw[w]; PK_END
    } else {
        for (int w = 0; w < W; ++w) a.dst.cards[w * ds + d] = a.src.cards[w * ss + s];
    }
    if (a.dst.owed) {   // a State: what no record holds is zero for an idle table
        a.dst.owed[d] = 0; a.dst.mid[d] = 0; a.dst.env_ctx[d] = 0; a.dst.env_rew[d] = 0.0;
    }
}

// State -> blob; block 0 also writes the header (thread 0, 32 words at compile-time offsets of the by-value argument) and zeroes the
// alignment gaps (one byte per thread and gap: a gap is shorter than the 256 threads)
__global__ void __launch_bounds__(SNAP_BLOCK) k_snap_save(SnapCopyArgs a, SnapHeader hdr, uint64_t *hdr_out, SnapPads pads) {
    static_assert(SNAP_BLOCK >= 256, "one thread per byte of an alignment gap");
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) {
            const uint64_t *hw = reinterpret_cast<const uint64_t *>(&hdr);
            PK_FOR(j, (int)(SNAP_HEADER_BYTES / 8)) hdr_out[j] = hw[j]; PK_END
        }
        uint8_t *bytes = reinterpret_cast<uint8_t *>(hdr_out);
        PK_FOR(f, SNAP_FIELDS)
            const uint64_t at = pads.begin[f] + threadIdx.x;
            if (at < pads.end[f]) bytes[at] = 0;
        PK_END
    }
    copy_record<false>(a);
}
// blob -> State (after k_snap_check has passed every record)
__global__ void __launch_bounds__(SNAP_BLOCK) k_snap_load(SnapCopyArgs a) { copy_record<false>(a); }
// State (or a staging blob) -> State, with the optional redeal
__global__ void __launch_bounds__(SNAP_BLOCK) k_snap_clone(SnapCopyArgs a) { copy_record<true>(a); }

__global__ void __launch_bounds__(SNAP_BLOCK) k_snap_check_idx(const int32_t *idx, size_t m, int T, uint32_t *mark, int mode, uint32_t bad, uint32_t *word) {
    const size_t i = (size_t)blockIdx.x * SNAP_BLOCK + threadIdx.x;
    if (i >= m) return;
    const int64_t t = idx ? (int64_t)idx[i] : (int64_t)i;
    uint32_t r = 0;
    if (t < 0 || t >= T) r = bad;
    else if (mark) r = mode == 0 ? (atomicAdd(&mark[t], 1u) ? (uint32_t)SNAP_DUP_DST : 0u) : (mark[t] ? (uint32_t)SNAP_OVERLAP : 0u);
    if (r) atomicOr(word, r);
}

// Everything a later kernel indexes with, or that would break the bit-exact money, of each record of a blob (spec: pokerl_hip.h)
__global__ void __launch_bounds__(SNAP_BLOCK) k_snap_check(SnapView v, int N, size_t m, uint32_t *word) {
    const size_t i = (size_t)blockIdx.x * SNAP_BLOCK + threadIdx.x;
    if (i >= m) return;
    const size_t st = v.stride;
    uint32_t r = 0;
    const Cursor cur{v.cursors[i]};   // (its fields by hand below: through the getters this kernel's branches come out in another order; its code is kept as it is)
    const uint32_t n = (uint32_t)N;
    if ((cur.w & 15u) >= n || ((cur.w >> 4) & 15u) >= n || ((cur.w >> 8) & 15u) >= n || ((cur.w >> 12) & 15u) >= n || ((cur.w >> 16) & 15u) > 4u || (cur.w >> 20) != 0)
        r |= SNAP_BAD_CURSOR;
    const SeatStates ss{v.seat_states[i]};
    const uint32_t sa = ss.active(), sc = ss.called(), sl = ss.allin(), sb = ss.broken();
    const uint32_t seats = (1u << n) - 1u;
    if (((sa | sc | sl | sb) & ~seats) || (sa & sc) || (sa & sl) || (sa & sb) || (sc & sl) || (sc & sb) || (sl & sb)) r |= SNAP_BAD_SEATS;
    const int K = 5 + 2 * N, W = (K + 3) / 4;
    uint64_t bits = 0;
    uint32_t any = 0;
    bool cards_ok = true;
    for (int w = 0; w < W; ++w) {
        const uint32_t word4 = v.cards[w * st + i];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t c = (word4 >> (8 * b)) & 0xffu;
            const bool used = 4 * w + b < K;
            cards_ok = cards_ok && (!used || (c < 0x40u && (c & 15u) < 13u));
            bits |= used ? (1ull << (c & 63u)) : 0ull;
            any |= used ? c : 0u;
        }
    }
    // a table that was never dealt (created, not reset yet: pk_create leaves its deck zero) holds 5+2N zero bytes at turn 0
    const bool never_dealt = any == 0 && cur.turn() == 0;
    if (!never_dealt && (!cards_ok || __popcll(bits) != K)) r |= SNAP_BAD_CARD;
    bool money_ok = finite_bits(v.min_raise[i]);
    for (int p = 0; p < N; ++p)
        money_ok = money_ok && finite_bits(v.credits[p * st + i]) && finite_bits(v.bets[p * st + i]) && finite_bits(v.pending[p * st + i]) &&
                   finite_bits(v.payoffs[p * st + i]);
    if (!money_ok) r |= SNAP_BAD_MONEY;
    if (v.valid[i] & 0x80u) r |= SNAP_BAD_VALID;
    if (r) atomicOr(word, r);
}

namespace pk {

static dim3 snap_grid(size_t m) { return dim3((unsigned)((m + SNAP_BLOCK - 1) / SNAP_BLOCK)); }

hipError_t snap_copy(hipStream_t stream, int kind, const SnapView &src, const int32_t *src_idx, const SnapView &dst, const int32_t *dst_idx,
                     int N, size_t m, const Redeal &rd, const SnapHeader &header, void *dst_blob, const SnapPads &pads) {
    if (m == 0) return hipSuccess;
    const SnapCopyArgs a{src, dst, src_idx, dst_idx, N, m, rd};
    if (kind == SNAP_KIND_SAVE) hipLaunchKernelGGL(k_snap_save, snap_grid(m), dim3(SNAP_BLOCK), 0, stream, a, header, (uint64_t *)dst_blob, pads);
    else if (kind == SNAP_KIND_LOAD) hipLaunchKernelGGL(k_snap_load, snap_grid(m), dim3(SNAP_BLOCK), 0, stream, a);
    else hipLaunchKernelGGL(k_snap_clone, snap_grid(m), dim3(SNAP_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t snap_check_idx(hipStream_t stream, const int32_t *idx, size_t m, int T, uint32_t *mark, int mode, uint32_t bad, uint32_t *word) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_snap_check_idx, snap_grid(m), dim3(SNAP_BLOCK), 0, stream, idx, m, T, mark, mode, bad, word);
    return hipGetLastError();
}

hipError_t snap_check_records(hipStream_t stream, const SnapView &src, int N, size_t m, uint32_t *word) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_snap_check, snap_grid(m), dim3(SNAP_BLOCK), 0, stream, src, N, m, word);
    return hipGetLastError();
}

}  // namespace pk
