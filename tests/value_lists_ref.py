"""NumPy reference of sorted channel lists (include/mustafar_hip.h: MUSTAFAR_VIEW_VALUE_LISTS), both retile directions, over a
reference-layout value cache: bmp uint64 [H, 2 T], idx uint32/int32 [H, 2 T + 1], one uint16 stream per head.  Slow and plain on purpose."""
import numpy as np

HEADER_BYTES = 256


def expand_block(bmp_h, idx_h, nz_h, b):
    """Block b of one head -> (values uint16 [64 tokens, 128 channels], kept bool [64, 128]).  A kept element may be +-0."""
    vals = np.zeros((64, 128), dtype=np.uint16)
    kept = np.zeros((64, 128), dtype=bool)
    for half in range(2):
        for t in range(64):
            tile = b * 128 + 64 * half + t
            m = int(bmp_h[tile]) & 0xFFFFFFFFFFFFFFFF
            chans = [64 * half + c for c in range(64) if (m >> (63 - c)) & 1]
            start = 2 * int(idx_h[tile])
            vals[t, chans] = nz_h[start:start + len(chans)]
            kept[t, chans] = True
    return vals, kept


def half_plan(kept_half):
    """kept bool [64 tokens, 64 channels] -> (cnt [64], perm [64], m [32])."""
    cnt = kept_half.sum(0).astype(np.int64)
    perm = np.array(sorted(range(64), key=lambda c: (-cnt[c], c)), dtype=np.uint8)
    m = np.array([int((cnt > 2 * r).sum()) for r in range(32)], dtype=np.uint8)
    return cnt, perm, m


def half_dwords(m) -> int:
    """The size formula: token row j has m[2j] dwords, value row r has m[r]."""
    return int(sum(int(m[2 * j]) for j in range(16)) + sum(int(x) for x in m))


def half_bytes(vals_half, kept_half):
    cnt, perm, m = half_plan(kept_half)
    out = []
    for j in range(16):
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


def tiles_to_lists(bmp, idx, nzs, tokens):
    """-> (table uint32 [H, tokens / 64 + 1]: dword offsets; blocks: per head a uint8 array)."""
    H, nb = len(nzs), tokens // 64
    table = np.zeros((H, nb + 1), dtype=np.uint32)
    blocks = []
    for h in range(H):
        nz_h = np.asarray(nzs[h]).view(np.uint16)
        out, at = [], 0
        for b in range(nb):
            vals, kept = expand_block(bmp[h], idx[h], nz_h, b)
            p0, m0, d0 = half_bytes(vals[:, :64], kept[:, :64])
            p1, m1, d1 = half_bytes(vals[:, 64:], kept[:, 64:])
            hdr = np.zeros(HEADER_BYTES, dtype=np.uint8)
            hdr[0:64], hdr[64:128], hdr[128:160], hdr[160:192] = p0, p1, m0, m1
            hdr[192:196] = np.frombuffer(np.uint32(64 + len(d0) // 4).tobytes(), dtype=np.uint8)
            blk = hdr.tobytes() + d0 + d1
            blk += b"\0" * (-len(blk) % 16)
            table[h, b] = at
            at += len(blk) // 4
            out.append(blk)
        table[h, nb] = at
        blocks.append(np.frombuffer(b"".join(out), dtype=np.uint8))
    return table, blocks


def lists_to_tiles(table, blocks, tokens):
    """-> (bmp uint64 [H, 2 T], idx uint32 [H, 2 T + 1], per head a uint16 stream): the reference layout."""
    H, nb = table.shape[0], tokens // 64
    bmp = np.zeros((H, nb * 128), dtype=np.uint64)
    idx = np.zeros((H, nb * 128 + 1), dtype=np.uint32)
    nzs = []
    for h in range(H):
        stream = []
        for b in range(nb):
            blk = blocks[h][4 * int(table[h, b]):4 * int(table[h, b + 1])]
            half1 = int(blk[192:196].view(np.uint32)[0])
            vals = np.zeros((64, 128), dtype=np.uint16)
            kept = np.zeros((64, 128), dtype=bool)
            for half in range(2):
                perm, m = blk[64 * half:64 * half + 64], blk[128 + 32 * half:160 + 32 * half]
                at = 4 * (half1 if half else 64)
                for j in range(16):
                    m0, m1 = int(m[2 * j]), int(m[2 * j + 1])
                    if m0 == 0:
                        break
                    tok = blk[at:at + 4 * m0].reshape(m0, 4)
                    v0 = blk[at + 4 * m0:at + 8 * m0].view(np.uint16).reshape(m0, 2)
                    v1 = blk[at + 8 * m0:at + 8 * m0 + 4 * m1].view(np.uint16).reshape(m1, 2)
                    at += 4 * (2 * m0 + m1)
                    for i in range(m0):
                        for k in range(4):
                            s = 4 * j + k
                            if i >= int(m[s // 2]) or (s > 0 and tok[i, k] == 0):   # behind the lane's last entry: tokens ascend
                                break
                            c = 64 * half + int(perm[i])
                            vals[tok[i, k], c] = (v0 if k < 2 else v1)[i, k & 1]
                            kept[tok[i, k], c] = True
            for half in range(2):
                for t in range(64):
                    tile = b * 128 + 64 * half + t
                    chans = np.flatnonzero(kept[t, 64 * half:64 * half + 64])
                    mm = 0
                    for c in chans:
                        mm |= 1 << (63 - int(c))
                    bmp[h, tile] = mm
                    n8 = (len(chans) + 7) // 8 * 8
                    idx[h, tile + 1] = idx[h, tile] + n8 // 2
                    stream.append(np.concatenate([vals[t, 64 * half + chans], np.zeros(n8 - len(chans), dtype=np.uint16)]))
        nzs.append(np.concatenate(stream) if stream else np.zeros(0, dtype=np.uint16))
    return bmp, idx, nzs
