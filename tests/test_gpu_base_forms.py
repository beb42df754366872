"""GPU: every byte a retile pass owns is written and no byte beyond is touched (mustafar_amd/csrc/base_forms.hip).

The round trips of tests/test_gpu_key_rows.py, test_gpu_value_lists.py, test_gpu_value_pair_lists.py and test_gpu_key_nibble_rows.py go through
`CompressedArena._retile()`, which allocates its destination itself: what a pass leaves unwritten, or writes behind its own bytes, stays
unseen there.  Here the entry points of every form in `cache.BASE_FORMS` are driven through ctypes into destinations filled with 0xEE:
plan, fill (the heads' bytes equal the form's NumPy reference, everything behind them is still 0xEE), to_tiles (bitmaps, offsets and the
streams up to the heads' totals equal the tile arrays the form was made from, everything behind them is still 0xEE).  Two inputs: the
form's special rows as its round-trip test builds them at its smallest size, and two heads of 320 tokens (five blocks: three pairs, the
last a half pair) that keep 38 and 64 channels per token, so that the shorter head ends well inside the stride both heads share."""
import ctypes

import numpy as np
import pytest
import torch

import key_nibble_rows_ref
import key_rows_ref
import value_lists_ref
import value_pair_lists_ref
from mustafar_amd import _lib
from mustafar_amd.cache import BASE_FORMS, CompressedArena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xEE
SPARE = 256   # bytes behind the fullest head, and tiles / offsets behind every head's

_REFERENCE = {"key_rows": key_rows_ref.tiles_to_rows, "value_lists": value_lists_ref.tiles_to_lists,
              "value_pair_lists": value_pair_lists_ref.tiles_to_pair_lists, "key_nibble_rows": key_nibble_rows_ref.tiles_to_rows}


def _special_arena(form):
    if form.name == "key_nibble_rows":
        from tests.test_gpu_key_nibble_rows import _special_arena as nibble_arena
        return nibble_arena(1)
    if form.name == "key_rows":
        from tests.test_gpu_key_rows import _special
        return CompressedArena.from_pruned(torch.from_numpy(_special(256)).to(DEV), "key")
    if form.name == "value_lists":
        from tests.test_gpu_value_lists import _special
    else:
        from tests.test_gpu_value_pair_lists import _special
    a = CompressedArena.from_pruned(torch.from_numpy(_special(256)).to(DEV), "value")
    for t, bits in ((0, 0), (9, -32768)):   # kept +0 and kept -0, as the round trips of the two list forms patch them in
        a.nz.view(torch.int16)[1, 2 * int(a.idx[1, t])] = bits
    return a


def _random_arena(form):
    """Two heads of 320 tokens of seeded N(0, 1): head 0 keeps the 38 largest magnitudes of every token, head 1 the 64 largest."""
    x = np.random.default_rng(320).standard_normal((2, 320, 128)).astype(np.float16)
    for h, keep in enumerate((38, 64)):
        order = np.argsort(-np.abs(x[h].astype(np.float32)), axis=1, kind="stable")
        np.put_along_axis(x[h], order[:, keep:], np.float16(0), axis=1)
    assert (np.count_nonzero(x, axis=2) == np.array([[38], [64]])).all()
    return CompressedArena.from_pruned(torch.from_numpy(x).to(DEV), form.which)


def _filled(*shape):
    return torch.full(shape, FILL, dtype=torch.uint8, device=DEV)


def _untouched(t):
    return bool((t == FILL).all())


@pytest.mark.parametrize("data", ["special", "random_320"])
@pytest.mark.parametrize("form", BASE_FORMS, ids=[f.name for f in BASE_FORMS])
def test_a_pass_writes_every_byte_it_owns_and_none_beyond(form, data):
    name = form.name
    a = _special_arena(form) if data == "special" else _random_arena(form)
    L = _lib.load()
    H, T = a.heads, a.tokens
    tiles, columns = 2 * T, form.table_columns(T // 64)
    used = [int(u) for u in a.used]
    bmp0, idx0 = a.bmp[:, :tiles].clone(), a.idx[:, :tiles + 1].clone()
    nz0 = [a.nz[h, :used[h]].clone() for h in range(H)]
    want_table, want = _REFERENCE[name](bmp0.cpu().numpy().view(np.uint64), idx0.cpu().numpy().view(np.uint32),
                                        [s.cpu().numpy().view(np.uint16) for s in nz0], T)
    st = torch.cuda.current_stream(DEV).cuda_stream
    # 1, 2: plan; the heads' units
    table = _filled(4 * H * columns + SPARE)   # (the plan pass takes the table without a pitch: H x columns entries back to back)
    units = torch.zeros(H, dtype=torch.int64, device=DEV)
    assert getattr(L, form.plan)(st, a.view_ptr(), H, T, table.data_ptr(), units.data_ptr()) == 0
    sizes = [int(u) * form.unit_bytes for u in units.cpu()]
    assert sizes == [w.size for w in want], "the heads' units"
    if data == "random_320":
        assert sizes[0] + 1024 < sizes[1], "the shorter head ends well inside the shared stride"
    planned = table.cpu().numpy()
    assert np.array_equal(planned[:4 * H * columns].view(np.uint32).reshape(H, columns), want_table) and (planned[4 * H * columns:] == FILL).all()
    # 3, 4, 5: fill into 0xEE
    head_bytes = form.head_bytes(max(sizes) // form.unit_bytes) + SPARE
    store = _filled(H, head_bytes)
    view = _lib.CacheView(None, store.data_ptr(), table.data_ptr(), None, 0, columns, head_bytes // 16, form.flag)
    assert getattr(L, form.fill)(st, a.view_ptr(), ctypes.byref(view), H, T) == 0
    got = store.cpu().numpy()
    for h in range(H):
        assert np.array_equal(got[h, :sizes[h]], want[h]), f"{name}: the bytes of head {h}"
        assert (got[h, sizes[h]:] == FILL).all(), f"{name}: bytes behind head {h} were written"
    assert np.array_equal(table.cpu().numpy(), planned), "fill leaves the table alone"
    # 6, 7: back to tiles, into 0xEE
    stride = int(a.view.nz_head_stride)   # uint4 units
    assert stride > 0
    bmp, idx, nz = _filled(H, 8 * (tiles + SPARE)), _filled(H, 4 * (tiles + 1 + SPARE)), _filled(H, 16 * stride)
    totals = torch.zeros(H, dtype=torch.int64, device=DEV)
    dst = _lib.CacheView(bmp.data_ptr(), nz.data_ptr(), idx.data_ptr(), None, tiles + SPARE, tiles + 1 + SPARE, stride, 0)
    assert getattr(L, form.to_tiles)(st, ctypes.byref(view), ctypes.byref(dst), H, T, totals.data_ptr()) == 0
    torch.cuda.synchronize()
    assert [int(t) for t in totals.cpu()] == used, "the heads' stream lengths"
    for h in range(H):
        assert torch.equal(bmp[h, :8 * tiles].view(torch.int64), bmp0[h]) and _untouched(bmp[h, 8 * tiles:]), f"{name}: bitmaps of head {h}"
        assert torch.equal(idx[h, :4 * (tiles + 1)].view(torch.int32), idx0[h]) and _untouched(idx[h, 4 * (tiles + 1):]), f"{name}: offsets of head {h}"
        assert torch.equal(nz[h, :2 * used[h]].view(torch.int16), nz0[h].view(torch.int16)), f"{name}: stream of head {h}"
        assert _untouched(nz[h, 2 * used[h]:]), f"{name}: the stream behind head {h}'s total was written"
    assert np.array_equal(store.cpu().numpy(), got), "to_tiles leaves the form alone"
