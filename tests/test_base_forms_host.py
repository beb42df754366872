"""CPU: the view rules of the four base forms -- the row rule, the list rule -- and of a retile pass's tile view (mustafar_amd/csrc/tile_view.h)
exist once: whatever view one of them refuses is refused, with MUSTAFAR_EINVAL and before any launch, by the retile entry points AND by
the fused call.  The argument tuples are those of test_entry_points_refuse_a_*_view_without_a_gpu (tests/test_key_rows_host.py,
tests/test_value_lists_host.py); the fused call is asked at their shape and at c3's, where mustafar_decode_reads_key_rows() is 1 and
the view rule is all that stands between the call and a launch."""
import ctypes

import pytest

from mustafar_amd import _lib

_BUF = (ctypes.c_uint64 * 64)()
P = ctypes.addressof(_BUF)
EINVAL = 1

# (bmp, nz, idx, nz_offset, bmp_head_stride, idx_head_stride, nz_head_stride, flags) of a well-formed view of `tokens` tokens
_GOOD = {"tiles": lambda tokens: [P, P, P, P, 0, 0, 64, 0],
         "rows": lambda tokens: [None, P, P, None, 0, tokens // 64, 16 * 40, _lib.VIEW_KEY_ROWS],
         "lists": lambda tokens: [None, P, P, None, 0, tokens // 64 + 1, 40, _lib.VIEW_VALUE_LISTS],
         "pair_lists": lambda tokens: [None, P, P, None, 0, _pair_columns(tokens), 40, _lib.VIEW_VALUE_PAIR_LISTS],
         "nibble_rows": lambda tokens: [None, P, P, None, 0, tokens // 64, 16 * 40, _lib.VIEW_KEY_NIBBLE_ROWS]}
_NZ, _IDX, _BMP_PITCH, _IDX_PITCH, _NZ_STRIDE, _FLAGS = 1, 2, 4, 5, 6, 7
# what is wrong: (field, its value as a function of the tokens).  A wrong flag is the other SIDE's: with the flag of the other row form / list
# form a view of this shape is a well-formed view of that form.
_MALFORMED = {
    "rows": {"wrong flag": (_FLAGS, lambda t: _lib.VIEW_VALUE_LISTS), "null idx": (_IDX, lambda t: None), "null nz": (_NZ, lambda t: None),
             "nz_head_stride 0": (_NZ_STRIDE, lambda t: 0), "stride not a multiple of 16": (_NZ_STRIDE, lambda t: 16 * 40 + 8),
             "table pitch one short": (_IDX_PITCH, lambda t: t // 64 - 1)},
    "lists": {"wrong flag": (_FLAGS, lambda t: _lib.VIEW_KEY_ROWS), "null idx": (_IDX, lambda t: None), "null nz": (_NZ, lambda t: None),
              "nz_head_stride 0": (_NZ_STRIDE, lambda t: 0), "table pitch one short": (_IDX_PITCH, lambda t: t // 64)},
    "pair_lists": {"wrong flag": (_FLAGS, lambda t: _lib.VIEW_KEY_ROWS), "null idx": (_IDX, lambda t: None), "null nz": (_NZ, lambda t: None),
                   "nz_head_stride 0": (_NZ_STRIDE, lambda t: 0), "table pitch one short": (_IDX_PITCH, lambda t: _pair_columns(t) - 1)},
    "nibble_rows": {"wrong flag": (_FLAGS, lambda t: _lib.VIEW_VALUE_LISTS), "null idx": (_IDX, lambda t: None), "null nz": (_NZ, lambda t: None),
                    "nz_head_stride 0": (_NZ_STRIDE, lambda t: 0), "stride not a multiple of 16": (_NZ_STRIDE, lambda t: 16 * 40 + 8),
                    "table pitch one short": (_IDX_PITCH, lambda t: t // 64 - 1)},
    "tiles": {"wrong flag": (_FLAGS, lambda t: 4), "null idx": (_IDX, lambda t: None), "null nz": (_NZ, lambda t: None),
              "bitmap pitch one short": (_BMP_PITCH, lambda t: 2 * t - 1), "offset pitch one short": (_IDX_PITCH, lambda t: 2 * t)},
}
# the retile entry points of a form, and the side of the fused call that takes it
_PASSES = {"rows": ("mustafar_key_rows", "key"), "nibble_rows": ("mustafar_key_nibble_rows", "key"),
           "lists": ("mustafar_value_lists", "value"), "pair_lists": ("mustafar_value_pair_lists", "value")}
_CASES = [(kind, what) for kind in sorted(_MALFORMED) for what in _MALFORMED[kind]]


def _pair_columns(tokens):
    return 2 * ((tokens // 64 + 1) // 2) + 1


def _view(kind, tokens, what=None):
    fields = _GOOD[kind](tokens)
    if what is not None:
        field, value = _MALFORMED[kind][what]
        fields[field] = value(tokens)
    return _lib.CacheView(*fields)


def _fused_call(k, v, T, batch, window_capacity, ld, flags=0):
    """mustafar_decode_attention_view with the tail of the refusal tests: (q, windows, new rows, window_len, window_capacity, scores, ld,
    out, workspace, Split_K, T, Batch_Size, groups, sqrt_d, no counter, no mask, ...)."""
    tail = (P, P, P, None, None, 1, window_capacity, P, ld, P, P, 1, T, batch, 4, 11.3, None, None, 0, 1)
    return _lib.load().mustafar_decode_attention_view(None, ctypes.byref(k), ctypes.byref(v), *tail, flags)


@pytest.mark.parametrize("kind,what", _CASES, ids=[f"{k}-{w.replace(' ', '_')}" for k, w in _CASES])
def test_a_view_one_rule_refuses_is_refused_by_the_retile_passes_and_by_the_fused_call(kind, what):
    L = _lib.load()
    bad = ctypes.byref(_view(kind, 256, what))
    tiles = ctypes.byref(_view("tiles", 256))
    if kind in _PASSES:
        assert getattr(L, _PASSES[kind][0] + "_to_tiles")(None, bad, tiles, 1, 256, P) == EINVAL
        assert getattr(L, _PASSES[kind][0] + "_fill")(None, tiles, bad, 1, 256) == EINVAL
    else:
        for form, (passes, _) in _PASSES.items():
            good = ctypes.byref(_view(form, 256))
            assert getattr(L, passes + "_plan")(None, bad, 1, 256, P, P) == EINVAL
            assert getattr(L, passes + "_fill")(None, bad, good, 1, 256) == EINVAL
            assert getattr(L, passes + "_to_tiles")(None, good, bad, 1, 256, P) == EINVAL
    # the fused call, at the tuples' own shape and at c3's (64 head groups of 7936 tokens: the launch that reads the forms)
    assert L.mustafar_decode_reads_key_rows(4, 7936, 64, 8224, 0) == 1 and L.mustafar_decode_reads_value_lists(4, 7936, 64, 8224, 0) == 1
    assert L.mustafar_decode_reads_key_nibble_rows(4, 7936, 64, 8224, 0) == 1 and L.mustafar_decode_reads_value_pair_lists(4, 7936, 64, 8224, 0) == 1
    for T, batch, cap, ld in ((256, 4, 64, 256 + 64), (7936, 256, 288, 8224)):
        bad = _view(kind, T, what)
        if _PASSES.get(kind, ("", "key"))[1] == "key":       # a key form, or tiles: as the key cache, beside every value form
            for other in ("tiles", "lists", "pair_lists"):
                assert _fused_call(bad, _view(other, T), T, batch, cap, ld) == EINVAL
        if _PASSES.get(kind, ("", "value"))[1] == "value":   # a value form, or tiles: as the value cache, beside every key form
            for other in ("tiles", "rows", "nibble_rows"):
                assert _fused_call(_view(other, T), bad, T, batch, cap, ld) == EINVAL
