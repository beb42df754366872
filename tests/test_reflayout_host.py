"""CPU: the cache protocol of mustafar_amd/reflayout.py on CPU tensors (`data_ptr()` works on them; no kernel runs), `hook.Past`, and the
module order: the layers below the hook import without it."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from mustafar_amd.reflayout import FlatStreams, ListCache, as_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref(heads=2, tokens=128, Dd=64, nzs=None):
    tiles = tokens * Dd // 64
    if nzs is None:
        nzs = [torch.zeros(8, dtype=torch.float16) for _ in range(heads)]
    return [torch.zeros(heads * tiles, dtype=torch.int64), torch.zeros(heads * (tiles + 1), dtype=torch.int32), nzs,
            torch.zeros(heads, dtype=torch.int32)]


def _addr(p):
    return ctypes.cast(p, ctypes.c_void_p).value


def test_the_empty_cache_is_all_null():
    k, v = ListCache(None, 0), ListCache(None, 0)
    assert k.decode_args(v, tables=False) == ((None,) * 8, ())
    assert k.view_args(v, tables=False) == ((None, None, 0, None, None), ())
    assert k.heads == 0 and k.tokens == 0 and k.total_tokens == 0 and not k.extents and k.bytes_in_use() == 0
    assert isinstance(as_cache(None, 0), ListCache) and as_cache(k, 0) is k


def test_empty_tensors_become_null_addresses():
    e = lambda dt: torch.zeros(0, dtype=dt)
    ref = [e(torch.int64), e(torch.int32), FlatStreams([]), e(torch.int32)]
    k, v = ListCache(ref, 64), ListCache(_ref(tokens=64), 64)
    args, keep = k.decode_args(v)
    assert args[:4] == (None,) * 4 and all(a for a in args[4:]) and len(keep) == 2 and keep[0] is None
    view = k.view
    assert (view.bmp, view.nz, view.idx, view.nz_offset) == (None,) * 4


def test_a_plain_list_of_streams_is_concatenated_once():
    ref = _ref()
    k, v = ListCache(ref, 128), ListCache(_ref(), 128)
    flat = k.flat
    assert flat.numel() == 16 and not hasattr(ref[2], "flat")
    (a1, keep1), (a2, keep2) = k.decode_args(v), k.decode_args(v)
    assert keep1[0] is flat and keep2[0] is flat and a1 == a2 and a1[1] == flat.data_ptr()
    assert a1 == (ref[0].data_ptr(), flat.data_ptr(), ref[1].data_ptr(), ref[3].data_ptr(),
                  v.ref[0].data_ptr(), v.flat.data_ptr(), v.ref[1].data_ptr(), v.ref[3].data_ptr())
    (w1, kept), (w2, _) = k.view_args(v, tables=False), k.view_args(v, tables=True)
    assert _addr(w1[0]) == _addr(w2[0]) == ctypes.addressof(k.view) and _addr(w1[1]) == _addr(w2[1]) == ctypes.addressof(v.view)
    assert w1[2:] == (128, None, None) and w2[2:] == (128, None, None) and kept == (k, v)
    assert k.view.nz == flat.data_ptr() and k.view.bmp == ref[0].data_ptr() and k.view.nz_head_stride == 0
    assert k.bytes_in_use() == 2 * 128 * 8 + 2 * 129 * 4 + 2 * 4 + 16 * 2


def test_flat_streams_and_a_plain_tensor_are_used_without_a_copy():
    buf = torch.zeros(16, dtype=torch.float16)
    fs = FlatStreams([buf[:8], buf[8:]], flat=buf)
    assert ListCache(_ref(nzs=fs), 128).flat is buf
    assert ListCache(_ref(nzs=buf), 128).flat is buf


@pytest.mark.parametrize("heads", [1, 2, 5])
def test_heads_is_the_length_of_nz_offset(heads):
    c = ListCache(_ref(heads=heads), 128)
    assert c.heads == heads == c.ref[3].numel() and c.tokens == c.total_tokens == 128 and c.extents == ()


def test_past_is_the_plain_tuple_with_names():
    from mustafar_amd.hook import Past
    t = ("kc", "kw", "vc", "vw", 256, 300)
    p = Past(*t)
    assert p == t and isinstance(p, tuple) and p[4] == 256 and p[-1] == 300
    k_c, k_w, v_c, v_w, C, L = p
    assert (k_c, k_w, v_c, v_w, C, L) == t
    assert (p.k_cache, p.k_window, p.v_cache, p.v_window, p.compressed_length, p.kv_seq_len) == t
    q = p._replace(kv_seq_len=301, compressed_length=512)
    assert q == ("kc", "kw", "vc", "vw", 512, 301) and p == t


@pytest.mark.parametrize("module", ["reflayout", "compression", "cache", "cache64"])
def test_the_layers_below_the_hook_import_without_it(module):
    code = (f"import sys, mustafar_amd.{module}; "
            "assert 'mustafar_amd.hook' not in sys.modules and 'mustafar_amd.partial' not in sys.modules, sorted(sys.modules)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
