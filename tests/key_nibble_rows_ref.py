"""NumPy reference of nibble-row key blocks (include/mustafar_hip.h: MUSTAFAR_VIEW_KEY_NIBBLE_ROWS; mustafar_amd/csrc/key_nibble_rows.h),
both retile directions, over a reference-layout key cache: bmp uint64 [H, 2 T], idx uint32 [H, 2 T + 1], one uint16 stream per head.  Slow
and plain on purpose.  Also the special blocks that the host program (tools/key_nibble_rows_check.cpp), the CPU tests and the GPU round
trip share, and the CRC-32 the host program prints per block."""
import zlib

import numpy as np

from key_rows_ref import expand_block

SPACER, SPACER_STEP = 15, 14


def front_of(w: int) -> int:
    return ((w // 2) + 1) & ~1


def share_rows(n: int) -> int:
    return (n + 7) // 8 + n // 2


def rows_of(w: int) -> int:
    return share_rows(front_of(w)) + share_rows(w - front_of(w))


def gap_slots(g: int) -> int:
    return (g + SPACER_STEP - 1) // SPACER_STEP


def chain(channels, start: int):
    """The (step, index into `channels` or -1) slots of a chain over `channels` (in chain order) starting at position `start`."""
    out, prev = [], start
    for i, c in enumerate(channels):
        g = abs(int(c) - prev)
        while g > SPACER_STEP:
            out.append((SPACER, -1))
            g -= SPACER_STEP
        out.append((g, i))
        prev = int(c)
    return out


def split(kept_t, F: int):
    """Greedy: (front channels ascending, back channels descending) of a token at front size F."""
    ch = [int(c) for c in np.flatnonzero(kept_t)]
    m, slots, prev = 0, 0, -1
    for c in ch:
        slots += gap_slots(c - prev)
        if slots > F:
            break
        m, prev = m + 1, c
    return ch[:m], ch[m:][::-1]


def token_fits(kept_t, w: int) -> bool:
    F = front_of(w)
    _, back = split(kept_t, F)
    return len(chain(back, 128)) <= w - F


def block_width(kept) -> int:
    w = 2
    for t in range(64):
        w = max(w, (int(kept[t].sum()) + 1) // 2 * 2)
        while not token_fits(kept[t], w):
            w += 2
    return w


def encode_block(vals, kept):
    """(w, the block's bytes) of values uint16 [64, 128] / kept bool [64, 128]."""
    w = block_width(kept)
    F = front_of(w)
    parts = []
    for n, part in ((F, 0), (w - F, 1)):
        steps = np.zeros(((n + 7) // 8, 64), dtype=np.uint32)
        v = np.zeros((n // 2, 64, 2), dtype=np.uint16)
        for t in range(64):
            ch = split(kept[t], F)[part]
            for s, (step, i) in enumerate(chain(ch, 128 if part else -1)):
                steps[s // 8, t] |= np.uint32(step << (4 * (s % 8)))
                if i >= 0:
                    v[s // 2, t, s % 2] = vals[t, ch[i]]
        parts += [steps.tobytes(), v.tobytes()]
    return w, b"".join(parts)


def slots_of(blk, w: int):
    """Every slot of a block: (token, part, slot, step, channel after the step, value uint16) -- padding and spacers included."""
    F = front_of(w)
    blk = np.frombuffer(bytes(blk), dtype=np.uint8)
    out, at = [], 0
    for n, part in ((F, 0), (w - F, 1)):
        ns = (n + 7) // 8
        steps = blk[at:at + 256 * ns].view(np.uint32).reshape(ns, 64)
        v = blk[at + 256 * ns:at + 256 * (ns + n // 2)].view(np.uint16).reshape(n // 2, 64, 2)
        at += 256 * share_rows(n)
        for t in range(64):
            pos = 128 if part else -1
            for s in range(n):
                step = (int(steps[s // 8, t]) >> (4 * (s % 8))) & 15
                adv = SPACER_STEP if step == SPACER else step
                pos += -adv if part else adv
                out.append((t, part, s, step, pos, int(v[s // 2, t, s % 2])))
    return out


def decode_block(blk, w: int):
    vals = np.zeros((64, 128), dtype=np.uint16)
    kept = np.zeros((64, 128), dtype=bool)
    for t, _, _, step, pos, x in slots_of(blk, w):
        if 1 <= step <= SPACER_STEP:
            vals[t, pos], kept[t, pos] = x, True
    return vals, kept


def tiles_to_rows(bmp, idx, nzs, tokens):
    """-> (table uint32 [H, tokens / 64]: first row << 8 | w; rows: per head a uint8 array of 256-byte rows)."""
    H, nb = len(nzs), tokens // 64
    table = np.zeros((H, nb), dtype=np.uint32)
    rows = []
    for h in range(H):
        nz_h = np.asarray(nzs[h]).view(np.uint16)
        out, first = [], 0
        for b in range(nb):
            w, blk = encode_block(*expand_block(bmp[h], idx[h], nz_h, b))
            out.append(blk)
            table[h, b] = (first << 8) | w
            first += rows_of(w)
        rows.append(np.frombuffer(b"".join(out), dtype=np.uint8))
    return table, rows


def block_tiles(vals, kept):
    """(bitmaps uint64 [128], lengths in half2 [128], the 128 tiles' streams) of one block."""
    bmp = np.zeros(128, dtype=np.uint64)
    length = np.zeros(128, dtype=np.uint32)
    stream = []
    for d in range(128):
        toks = np.flatnonzero(kept[:, d])
        m = 0
        for t in toks:
            m |= 1 << (63 - int(t))
        bmp[d] = m
        n8 = (len(toks) + 7) // 8 * 8
        length[d] = n8 // 2
        stream.append(np.concatenate([vals[toks, d], np.zeros(n8 - len(toks), dtype=np.uint16)]))
    return bmp, length, stream


def rows_to_tiles(table, rows, tokens):
    """-> (bmp uint64 [H, 2 T], idx uint32 [H, 2 T + 1], per head a uint16 stream): the reference layout."""
    H, nb = table.shape
    bmp = np.zeros((H, nb * 128), dtype=np.uint64)
    idx = np.zeros((H, nb * 128 + 1), dtype=np.uint32)
    nzs = []
    for h in range(H):
        stream = []
        for b in range(nb):
            ent = int(table[h, b])
            w, first = ent & 0xFF, ent >> 8
            m, length, s = block_tiles(*decode_block(rows[h][256 * first:256 * (first + rows_of(w))], w))
            bmp[h, 128 * b:128 * (b + 1)] = m
            idx[h, 128 * b + 1:128 * (b + 1) + 1] = idx[h, 128 * b] + np.cumsum(length, dtype=np.uint32)
            stream += s
        nzs.append(np.concatenate(stream) if stream else np.zeros(0, dtype=np.uint16))
    return bmp, idx, nzs


def to_tiles(vals, kept):
    """The reference layout of one head's blocks, vals uint16 / kept bool [T, 128]: (bmp [2 T], idx [2 T + 1], stream)."""
    nb = vals.shape[0] // 64
    bmp = np.zeros(nb * 128, dtype=np.uint64)
    idx = np.zeros(nb * 128 + 1, dtype=np.uint32)
    stream = []
    for b in range(nb):
        m, length, s = block_tiles(vals[64 * b:64 * (b + 1)], kept[64 * b:64 * (b + 1)])
        bmp[128 * b:128 * (b + 1)] = m
        idx[128 * b + 1:128 * (b + 1) + 1] = idx[128 * b] + np.cumsum(length, dtype=np.uint32)
        stream += s
    return bmp, idx, np.concatenate(stream)


# ---- the special blocks.  Kept positions and values are given apart: a kept +0 or -0 is an entry.
ONE, PZERO, NZERO = 0x3C00, 0x0000, 0x8000
SPECIAL_NAMES = ("full_beside_two", "ends", "steps_14_15_28_29", "kept_zeros", "w_mod8_0", "w_mod8_2", "w_mod8_4", "w_mod8_6", "front_alone")


def _value(t: int, c: int) -> int:
    return 0x3800 + ((37 * t + 11 * c) & 0x3FF)   # fp16 in [0.5, 1): never a zero


def special_block(name: str):
    """-> (vals uint16 [64, 128], kept bool [64, 128])."""
    kept = np.zeros((64, 128), dtype=bool)
    zero = {}
    if name == "full_beside_two":          # a token that keeps all 128 channels next to tokens that keep 2: w = 128, long padding
        kept[:, [5, 100]] = True
        kept[7] = True
    elif name == "ends":                   # only channel 0, only channel 127, only both, nothing
        kept[0::4, 0] = True
        kept[1::4, 127] = True
        kept[2::4, [0, 127]] = True
    elif name == "steps_14_15_28_29":      # gaps of exactly 14, 15, 28, 29 in both directions, at w = 64 (front and back of 32 slots)
        for t in range(64):
            g = (14, 15, 28, 29)[t % 4]
            if t == 63:                    # 64 entries without a spacer: the width
                kept[t, :32] = kept[t, 96:] = True
            elif (t // 4) % 2 == 0:        # a front filled by 32 dense channels: the sparse chain from the top is the back's
                kept[t, :32] = True
                kept[t, np.arange(128 - g, 39, -g)] = True
            else:                          # a sparse chain from the bottom, then dense channels that overflow into the back
                kept[t, 96:] = True
                kept[t, np.arange(g - 1, 88, g)] = True
    elif name == "kept_zeros":             # all-zero token rows whose kept entries are +0, and -0
        for t in range(64):
            kept[t] = (np.arange(128) * 37 + 11 * t) % 128 < 40   # (37 is odd: 40 channels of every token)
        for t in range(0, 64, 2):
            for c in np.flatnonzero(kept[t]):
                zero[(t, int(c))] = PZERO if t % 4 == 0 else NZERO
    elif name.startswith("w_mod8_"):       # widths with w % 8 in {0, 2, 4, 6}: dense runs, no spacers
        n = 40 + int(name[-1])
        for t in range(64):
            kept[t, (np.arange(n) * 3 + t) % 128] = True
    elif name == "front_alone":            # every token fits the front alone: w = 2, the back is empty
        kept[::2, 3] = True
        kept[1::2, [2, 9]] = True
    else:
        raise KeyError(name)
    vals = np.zeros((64, 128), dtype=np.uint16)
    for t, c in zip(*np.nonzero(kept)):
        vals[t, c] = zero.get((int(t), int(c)), _value(int(t), int(c)))
    return vals, kept


def special_heads():
    """Two heads of unequal size, [2][T = 576]: head 0 the nine special blocks, head 1 the same in reverse order with every other block
    emptied -- `(vals uint16 [2, 576, 128], kept bool [2, 576, 128])`."""
    blocks = [special_block(n) for n in SPECIAL_NAMES]
    v0, k0 = np.concatenate([b[0] for b in blocks]), np.concatenate([b[1] for b in blocks])
    rev = blocks[::-1]
    v1, k1 = np.concatenate([b[0] for b in rev]).copy(), np.concatenate([b[1] for b in rev]).copy()
    for b in range(1, len(rev), 2):
        v1[64 * b:64 * (b + 1)], k1[64 * b:64 * (b + 1)] = 0, False
    return np.stack([v0, v1]), np.stack([k0, k1])


def crc_of(w: int, blk: bytes) -> int:
    """What tools/key_nibble_rows_check.cpp prints for a block: the CRC-32 of its bytes."""
    return zlib.crc32(blk) & 0xFFFFFFFF


def bytes_per_token(x_pruned) -> float:
    """Bytes per token and kv head of pruned fp16 rows [H, T, 128] in nibble rows (a non-zero is kept), the block table included."""
    H, T, _ = x_pruned.shape
    rows = 0
    for h in range(H):
        for b in range(T // 64):
            rows += rows_of(block_width(x_pruned[h, 64 * b:64 * (b + 1)].view(np.uint16) & 0x7FFF != 0))
    return (256 * rows + 4 * H * (T // 64)) / (H * T)
