"""NumPy reference of token-row key blocks (include/mustafar_hip.h: MUSTAFAR_VIEW_KEY_ROWS), both retile directions, over a
reference-layout key cache: bmp uint64 [H, 2 T], idx uint32/int32 [H, 2 T + 1], one uint16 stream per head.  Slow and plain on purpose."""
import numpy as np


def rows_of(w: int) -> int:
    return w // 2 + (w + 3) // 4


def expand_block(bmp_h, idx_h, nz_h, b):
    """Block b of one head -> (values uint16 [64 tokens, 128 channels], kept bool [64, 128])."""
    vals = np.zeros((64, 128), dtype=np.uint16)
    kept = np.zeros((64, 128), dtype=bool)
    for d in range(128):
        tile = b * 128 + d
        m = int(bmp_h[tile]) & 0xFFFFFFFFFFFFFFFF
        toks = [t for t in range(64) if (m >> (63 - t)) & 1]
        start = 2 * int(idx_h[tile])
        vals[toks, d] = nz_h[start:start + len(toks)]
        kept[toks, d] = True
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
            vals, kept = expand_block(bmp[h], idx[h], nz_h, b)
            w = max(2, (int(kept.sum(1).max()) + 1) // 2 * 2)
            v = np.zeros((w // 2, 64, 2), dtype=np.uint16)
            c = np.zeros(((w + 3) // 4, 64, 4), dtype=np.uint8)
            for t in range(64):
                for s, d in enumerate(np.flatnonzero(kept[t])):
                    v[s // 2, t, s % 2] = vals[t, d]
                    c[s // 4, t, s % 4] = d
            out += [c.tobytes(), v.tobytes()]
            table[h, b] = (first << 8) | w
            first += rows_of(w)
        rows.append(np.frombuffer(b"".join(out), dtype=np.uint8))
    return table, rows


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
            blk = rows[h][256 * first:256 * (first + rows_of(w))]
            c = blk[:256 * ((w + 3) // 4)].reshape((w + 3) // 4, 64, 4)
            v = blk[256 * ((w + 3) // 4):].view(np.uint16).reshape(w // 2, 64, 2)
            vals = np.zeros((64, 128), dtype=np.uint16)
            kept = np.zeros((64, 128), dtype=bool)
            for t in range(64):
                for s in range(w):
                    x = v[s // 2, t, s % 2]
                    if x & 0x7FFF == 0:
                        break
                    vals[t, c[s // 4, t, s % 4]] = x
                    kept[t, c[s // 4, t, s % 4]] = True
            for d in range(128):
                tile = b * 128 + d
                toks = np.flatnonzero(kept[:, d])
                m = 0
                for t in toks:
                    m |= 1 << (63 - int(t))
                bmp[h, tile] = m
                n8 = (len(toks) + 7) // 8 * 8
                idx[h, tile + 1] = idx[h, tile] + n8 // 2
                stream.append(np.concatenate([vals[toks, d], np.zeros(n8 - len(toks), dtype=np.uint16)]))
        nzs.append(np.concatenate(stream) if stream else np.zeros(0, dtype=np.uint16))
    return bmp, idx, nzs
