"""NumPy reference of sorted channel lists over pairs of blocks (include/mustafar_hip.h: MUSTAFAR_VIEW_VALUE_PAIR_LISTS), both retile
directions, over a reference-layout value cache: bmp uint64 [H, 2 T], idx uint32/int32 [H, 2 T + 1], one uint16 stream per head.  Slow
and plain on purpose; independent of csrc/value_pair_lists.h."""
import numpy as np

from value_lists_ref import expand_block

HEADER_BYTES = 256
MAX_ROWS, MAX_WORDS = 64, 32


def pairs_of(tokens: int) -> int:
    return (tokens // 64 + 1) // 2


def expand_pair(bmp_h, idx_h, nz_h, p, nb):
    """Pair p of one head -> (values uint16 [ntok, 128 channels], kept bool [ntok, 128]); ntok = 128, or 64 for a trailing half pair."""
    parts = [expand_block(bmp_h, idx_h, nz_h, b) for b in (2 * p, 2 * p + 1) if b < nb]
    return np.concatenate([v for v, _ in parts]), np.concatenate([k for _, k in parts])


def half_plan(kept_half):
    """kept bool [ntok, 64 channels] -> (cnt [64], perm [64], m [64])."""
    cnt = kept_half.sum(0).astype(np.int64)
    perm = np.array(sorted(range(64), key=lambda c: (-cnt[c], c)), dtype=np.uint8)
    m = np.array([int((cnt > 2 * r).sum()) for r in range(MAX_ROWS)], dtype=np.uint8)
    return cnt, perm, m


def half_dwords(m) -> int:
    """The size formula: token row j has m[2j] dwords, value row r has m[r]."""
    return int(sum(int(m[2 * j]) for j in range(MAX_WORDS)) + sum(int(x) for x in m))


def half_words(cnt) -> int:
    """Words a wave walks for a half: the longest list in whole words."""
    return (int(np.max(cnt)) + 3) // 4


def half_bytes(vals_half, kept_half):
    cnt, perm, m = half_plan(kept_half)
    out = []
    for j in range(MAX_WORDS):
        m0, m1 = int(m[2 * j]), int(m[2 * j + 1])
        if m0 == 0:
            break
        tok = np.zeros((m0, 4), dtype=np.uint8)
        v0 = np.zeros((m0, 2), dtype=np.uint16)
        v1 = np.zeros((m1, 2), dtype=np.uint16)
        for i in range(m0):
            c = int(perm[i])
            toks = np.flatnonzero(kept_half[:, c])
            for s in range(4 * j, min(4 * j + 4, len(toks))):
                tok[i, s - 4 * j] = toks[s]
                (v0 if s - 4 * j < 2 else v1)[i, s & 1] = vals_half[toks[s], c]
        out += [tok.tobytes(), v0.tobytes(), v1.tobytes()]
    data = b"".join(out)
    assert len(data) == 4 * half_dwords(m)
    return perm, m, data


def tiles_to_pair_lists(bmp, idx, nzs, tokens):
    """-> (table uint32 [H, 2 pairs + 1]: dword offsets of every pair's header and half 1, then the head's dwords; per head a uint8 array)."""
    H, nb, npairs = len(nzs), tokens // 64, pairs_of(tokens)
    table = np.zeros((H, 2 * npairs + 1), dtype=np.uint32)
    blocks = []
    for h in range(H):
        nz_h = np.asarray(nzs[h]).view(np.uint16)
        out, at = [], 0
        for p in range(npairs):
            vals, kept = expand_pair(bmp[h], idx[h], nz_h, p, nb)
            p0, m0, d0 = half_bytes(vals[:, :64], kept[:, :64])
            p1, m1, d1 = half_bytes(vals[:, 64:], kept[:, 64:])
            hdr = np.zeros(HEADER_BYTES, dtype=np.uint8)
            hdr[0:64], hdr[64:128], hdr[128:192], hdr[192:256] = p0, p1, m0, m1
            blk = hdr.tobytes() + d0 + d1
            blk += b"\0" * (-len(blk) % 16)
            table[h, 2 * p] = at
            table[h, 2 * p + 1] = at + (HEADER_BYTES + len(d0)) // 4
            at += len(blk) // 4
            out.append(blk)
        table[h, 2 * npairs] = at
        blocks.append(np.frombuffer(b"".join(out), dtype=np.uint8))
    return table, blocks


def pair_lists_to_tiles(table, blocks, tokens):
    """-> (bmp uint64 [H, 2 T], idx uint32 [H, 2 T + 1], per head a uint16 stream): the reference layout."""
    H, nb, npairs = table.shape[0], tokens // 64, pairs_of(tokens)
    bmp = np.zeros((H, nb * 128), dtype=np.uint64)
    idx = np.zeros((H, nb * 128 + 1), dtype=np.uint32)
    nzs = []
    for h in range(H):
        stream = []
        for p in range(npairs):
            head = blocks[h]
            start, half1 = int(table[h, 2 * p]), int(table[h, 2 * p + 1])
            hdr = head[4 * start:4 * start + HEADER_BYTES]
            ntok = 128 if 2 * p + 1 < nb else 64
            vals = np.zeros((ntok, 128), dtype=np.uint16)
            kept = np.zeros((ntok, 128), dtype=bool)
            for half in range(2):
                perm, m = hdr[64 * half:64 * half + 64], hdr[128 + 64 * half:192 + 64 * half]
                at = 4 * (half1 if half else start + 64)
                for j in range(MAX_WORDS):
                    m0, m1 = int(m[2 * j]), int(m[2 * j + 1])
                    if m0 == 0:
                        break
                    tok = head[at:at + 4 * m0].reshape(m0, 4)
                    v0 = head[at + 4 * m0:at + 8 * m0].view(np.uint16).reshape(m0, 2)
                    v1 = head[at + 8 * m0:at + 8 * m0 + 4 * m1].view(np.uint16).reshape(m1, 2)
                    at += 4 * (2 * m0 + m1)
                    for i in range(m0):
                        for k in range(4):
                            s = 4 * j + k
                            if i >= int(m[s // 2]) or (s > 0 and tok[i, k] == 0):   # behind the lane's last entry: tokens ascend
                                break
                            c = 64 * half + int(perm[i])
                            vals[tok[i, k], c] = (v0 if k < 2 else v1)[i, k & 1]
                            kept[tok[i, k], c] = True
            for b in range(ntok // 64):
                for half in range(2):
                    for t in range(64):
                        tile = (2 * p + b) * 128 + 64 * half + t
                        chans = np.flatnonzero(kept[64 * b + t, 64 * half:64 * half + 64])
                        mm = 0
                        for c in chans:
                            mm |= 1 << (63 - int(c))
                        bmp[h, tile] = mm
                        n8 = (len(chans) + 7) // 8 * 8
                        idx[h, tile + 1] = idx[h, tile] + n8 // 2
                        stream.append(np.concatenate([vals[64 * b + t, 64 * half + chans], np.zeros(n8 - len(chans), dtype=np.uint16)]))
        nzs.append(np.concatenate(stream) if stream else np.zeros(0, dtype=np.uint16))
    return bmp, idx, nzs
