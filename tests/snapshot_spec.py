"""The snapshot blob layout and the clone's redeal restated in Python (TEST INFRASTRUCTURE): include/pokerl_hip.h "Snapshots" and
DESIGN.md section 3, on top of oracle/rng_spec.py's philox4x32_10."""
import numpy as np

from oracle import rng_spec as R

HEADER_BYTES = 256
MAGIC = 0x4E534B50
VERSION = 1
STREAM_REDEAL = 0x52444C30   # 'RDL0'
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def _al(x):
    return (x + 255) & ~255


def fields(n, m):
    """{field: (byte offset, dtype, shape)} of a blob of m records at n seats, and its total size."""
    w = (5 + 2 * n + 3) // 4
    spec = [("credits", np.float64, (n, m)), ("bets", np.float64, (n, m)), ("pending", np.float64, (n, m)), ("payoffs", np.float64, (n, m)),
            ("min_raise", np.float64, (m,)), ("seat_states", np.uint64, (m,)), ("hand_serial", np.uint64, (m,)), ("step_serial", np.uint64, (m,)),
            ("cursors", np.uint32, (m,)), ("hand", np.int32, (m,)), ("cards", np.uint32, (w, m)), ("show", np.uint32, (n, m)),
            ("valid", np.uint8, (m,)), ("terr", np.uint8, (m,))]
    out, off = {}, HEADER_BYTES
    for name, dt, shape in spec:
        out[name] = (off, dt, shape)
        off += _al(int(np.prod(shape)) * np.dtype(dt).itemsize)
    return out, off


def nbytes(n, m):
    return fields(n, m)[1]


def view(blob, n, m, name):
    """A writable view of one field of a blob (np.uint8 array)."""
    off, dt, shape = fields(n, m)[0][name]
    size = int(np.prod(shape)) * np.dtype(dt).itemsize
    return blob[off:off + size].view(dt).reshape(shape)


def header(blob):
    h = blob[:HEADER_BYTES]
    return dict(magic=int(h[0:4].view(np.uint32)[0]), version=int(h[4:8].view(np.uint32)[0]), n=int(h[8:12].view(np.uint32)[0]),
                m=int(h[16:24].view(np.uint64)[0]), start_credits=h[24:152].view(np.float64).copy(),
                big_blind=float(h[152:160].view(np.float64)[0]), small_blind=float(h[160:168].view(np.float64)[0]))


def visible_positions(n, turn, p):
    nb = 0 if turn == 0 else min(turn + 2, 5)          # reference game.py:266-278
    return nb, set(range(nb)) | {5 + 2 * p, 6 + 2 * p}


def redeal(cards, n, turn, p, seed, table_id, nonce):
    """deck[0:5+2n] (Card.value bytes) after the redeal for observer seat p of a table at `turn`, drawn for the destination table id."""
    k_cards = 5 + 2 * n
    nb, vis = visible_positions(n, turn, p)
    canon = lambda v: (v & 15) * 4 + (v >> 4)     # value[k] = ((k%4)<<4)|(k//4), reference cards.py:77
    seen = {canon(int(cards[i])) for i in vis}
    unseen = [k for k in range(52) if k not in seen]
    P = 52 - nb - 2
    key = R.seed_key(seed)
    out = [int(c) for c in cards[:k_cards]]
    i, x, words = 0, 0, []
    for pos in range(k_cards):
        if pos in vis:
            continue
        if i % 18 == 0:
            w = R.philox4x32_10((table_id & MASK32, nonce & MASK32, (STREAM_REDEAL + i // 18) & MASK32, (nonce >> 32) & MASK32), key)
            words = [w[0] | (w[1] << 32), w[2] | (w[3] << 32)]
        if i % 9 == 0:
            x = words[(i // 9) % 2]
        prod = x * (P - i)
        c, x = prod >> 64, prod & MASK64
        k = unseen.pop(c)
        out[pos] = ((k % 4) << 4) | (k // 4)
        i += 1
    return np.array(out, np.uint8)
