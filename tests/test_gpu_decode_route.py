"""GPU: which fused decode entry point of the C ABI every cache kind reaches through the public hook API, and with which cache
arguments null.  The library handle of `mustafar_amd._lib` is replaced by a recording stand-in that notes `(name, args)` and then calls
the real function, so every case also runs the kernels it names: the outputs must be finite (the parity suites check their values).

Geometry: bsz 1, 8 query heads over 2 kv heads, residual_length 32.  A 543-token prefill leaves 256 compressed tokens and a 287-row
window, so the first decode step fires the 256-token trigger and the second one reads a cache that has grown; a 40-token prefill leaves
the compressed cache empty.

The same recorder classifies the calls of `decode_multi` (mustafar_decode_multi_query: views, T_base, tables) and of `decode_segment` over a
`SharedSegment` (mustafar_decode_shared_segment: two views and the token count), per cache kind."""
import pytest
import torch

from mustafar_amd import _lib, partial
from mustafar_amd.hook import MustafarAttention, MustafarConfig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HQ, HKV, R = 8, 2, 32
PREFIX = "mustafar_decode_attention"
TAIL = len(_lib._DECODE_TAIL)   # the arguments q ... flags that every entry point takes behind its cache arguments


class _Recorder:
    """Stands in for the loaded library: attribute lookup returns a wrapper that records the call and forwards it."""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapper(*args):
            self._calls.append((name, args))
            return fn(*args)
        return wrapper


@pytest.fixture
def calls(monkeypatch):
    made = []
    monkeypatch.setattr(_lib, "_lib", _Recorder(_lib.load(), made))
    return made


def _null(a) -> bool:
    return a is None or (isinstance(a, int) and a == 0)


def _routes(calls):
    """[(entry point suffix, cache arguments)] of the fused decode calls made, in order.  Cache arguments: "nulls" / "arrays" for the
    eight-array forms, "views" for the view form, and for the extents forms ("no tables" | "tables", "no t_device" | "t_device")."""
    out = []
    for name, args in calls:
        if not name.startswith(PREFIX):
            continue
        kind = name[len(PREFIX):]
        if kind in ("", "_hd", "_lse_hd"):
            nulls = [_null(a) for a in args[1:9]]
            assert all(nulls) or not any(nulls), (name, nulls)
            out.append((kind, "nulls" if all(nulls) else "arrays"))
        elif kind == "_view":
            assert not _null(args[1]) and not _null(args[2])
            out.append((kind, "views"))
        else:
            assert kind in ("_extents", "_extents_hd", "_extents_lse_hd"), name
            assert not _null(args[1]) and not _null(args[2]) and _null(args[4]) == _null(args[5])
            out.append((kind, ("no tables" if _null(args[4]) else "tables", "no t_device" if _null(args[6 + TAIL]) else "t_device")))
    return out


def _hook(D, **kw):
    return MustafarAttention(MustafarConfig(num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=D, residual_length=R, api="fused", **kw))


def _rand(D, n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda h: torch.randn((1, h, n, D), generator=g).half().to(DEV)
    return mk(HQ), mk(HKV), mk(HKV)


def _steps(attn, past, D, return_lse=False, steps=2, seed=7):
    """`steps` eager decode_fused steps; every output (and LSE) finite.  Returns the last `past`."""
    for i in range(steps):
        q, k, v = _rand(D, 1, seed + i)
        got = attn.decode_fused(q, k, v, past, return_lse=return_lse)
        past = got[-1]
        assert got[0].shape == (1, HQ, 1, D) and torch.isfinite(got[0]).all()
        if return_lse:
            assert got[1].shape == (1, HQ) and torch.isfinite(got[1]).all()
    torch.cuda.synchronize()
    return past


def _prefilled(attn, D, L0):
    _, K, V = _rand(D, L0, seed=L0 + D)
    past = attn.build_cache(K, V)
    assert past[4] == (256 if L0 == 543 else 0)
    return past


ARRAYS_GROWN = [
    # D, config, return_lse, the two calls
    (128, {}, False, [("", "arrays"), ("", "arrays")]),
    (64, {}, False, [("_hd", "arrays"), ("_hd", "arrays")]),
    (64, {}, True, [("_lse_hd", "arrays"), ("_lse_hd", "arrays")]),
    (128, {"arena": True}, False, [("_view", "views"), ("_extents", ("tables", "no t_device"))]),
    (128, {"arena": True}, True, [("_extents_lse_hd", ("no tables", "no t_device")), ("_extents_lse_hd", ("tables", "no t_device"))]),
    (64, {"hd64_extents": True}, False, [("_hd", "arrays"), ("_extents_hd", ("tables", "no t_device"))]),
    (64, {"hd64_extents": True}, True, [("_extents_lse_hd", ("tables", "no t_device")), ("_extents_lse_hd", ("tables", "no t_device"))]),
]


@pytest.mark.parametrize("D,kw,return_lse,want", ARRAYS_GROWN,
                         ids=["d128-list", "d64-list", "d64-list-lse", "d128-arena", "d128-arena-lse", "d64-extents", "d64-extents-lse"])
def test_route_across_a_trigger(calls, D, kw, return_lse, want):
    """256 compressed tokens, then the step that fires the trigger, then a step over the grown cache."""
    attn = _hook(D, **kw)
    past = _steps(attn, _prefilled(attn, D, 543), D, return_lse)
    assert past[4] == 512 and past[5] == 545 and past[1].len == 33
    assert _routes(calls) == want


def test_route_grown_arena_switched_to_two_launch(calls):
    """A cache that grew by an extent, handed to a hook whose launch form reads one view only: consolidated, then the view form."""
    attn = _hook(128, arena=True)
    grown = _steps(attn, _prefilled(attn, 128, 543), 128)
    assert grown[0].tokens == 256 and len(grown[0].extents) == 1 and len(grown[2].extents) == 1
    del calls[:]
    other = _hook(128, arena=True, structure="two_launch")
    past = _steps(other, grown, 128, steps=1)
    assert _routes(calls) == [("_view", "views")]
    for c in (past[0], past[2]):
        assert not c.extents and c.tokens == 512
    assert past[4] == 512


@pytest.mark.parametrize("D,kw,return_lse,kind", [(128, {}, False, ""), (64, {}, False, "_hd"), (64, {}, True, "_lse_hd"),
                                                  (64, {"hd64_extents": True}, False, "_hd"), (64, {"hd64_extents": True}, True, "_lse_hd")],
                         ids=["d128-list", "d64-list", "d64-list-lse", "d64-extents", "d64-extents-lse"])
def test_route_empty_cache(calls, D, kw, return_lse, kind):
    """No compressed token yet: the eight-array forms with eight null arrays."""
    attn = _hook(D, **kw)
    past = _steps(attn, _prefilled(attn, D, 40), D, return_lse)
    assert past[0] is None and past[4] == 0 and past[5] == 42
    assert _routes(calls) == [(kind, "nulls"), (kind, "nulls")]


def test_route_decode_segment(calls):
    """partial.decode_segment: always an entry point with an LSE, t_device null; an arena's tables only once it has extents.  A
    reference-layout segment whose streams are a plain list of per-head tensors, or one tensor, reads the same bits."""
    D = 128
    q, K, V = _rand(D, 288, seed=3)
    q = q[:, :, :1].contiguous()
    ref = _hook(D).build_cache(K, V)
    arena = _hook(D, arena=True)
    are = arena.build_cache(K, V)
    assert ref[4] == are[4] == 256 and isinstance(ref[0], list) and are[0].tokens == 256
    o_ref, l_ref = partial.decode_segment(arena, q, ref[0], ref[2], 256)
    o_are, l_are = partial.decode_segment(arena, q, are[0], are[2], 256)
    plain = lambda c, nz: [c[0], c[1], nz, c[3]]
    o_lst, l_lst = partial.decode_segment(arena, q, plain(ref[0], list(ref[0][2])), plain(ref[2], list(ref[2][2])), 256)
    o_one, l_one = partial.decode_segment(arena, q, plain(ref[0], torch.cat(list(ref[0][2]))), plain(ref[2], torch.cat(list(ref[2][2]))), 256)
    before = len(calls)
    grown = _steps(arena, _prefilled(arena, D, 543), D, steps=1)
    assert grown[0].total_tokens == 512 and len(grown[0].extents) == 1
    del calls[before:]   # (the step that grew the cache: routed in test_route_across_a_trigger)
    o_grw, l_grw = partial.decode_segment(arena, q, grown[0], grown[2], 512)
    torch.cuda.synchronize()
    assert _routes(calls) == [("_lse_hd", "arrays"), ("_extents_lse_hd", ("no tables", "no t_device")), ("_lse_hd", "arrays"),
                              ("_lse_hd", "arrays"), ("_extents_lse_hd", ("tables", "no t_device"))]
    for o, l in ((o_ref, l_ref), (o_are, l_are), (o_lst, l_lst), (o_one, l_one), (o_grw, l_grw)):
        assert o.shape == (1, HQ, 1, D) and l.shape == (1, HQ) and torch.isfinite(o).all() and torch.isfinite(l).all()
    for o, l in ((o_lst, l_lst), (o_one, l_one)):
        assert torch.equal(o.view(torch.int16), o_ref.view(torch.int16)) and torch.equal(l.view(torch.int32), l_ref.view(torch.int32))


# ---- decode_multi and shared segments: how every cache kind arrives as views ----------------------------------------------------------------
def _view_routes(calls):
    """[(entry point, "views" | "null views", T_base | tokens, "tables" | "no tables")] of the multi-query and shared-segment calls made."""
    out = []
    for name, args in calls:
        if name not in ("mustafar_decode_multi_query", "mustafar_decode_shared_segment"):
            continue
        assert _null(args[1]) == _null(args[2]), name
        tables = "no tables"
        if name == "mustafar_decode_multi_query":
            assert _null(args[4]) == _null(args[5])
            tables = "no tables" if _null(args[4]) else "tables"
        out.append((name[len("mustafar_decode_"):], "null views" if _null(args[1]) else "views", args[3], tables))
    return out


def _multi(attn, past, D, seed=11):
    """One decode_multi call of n_q = 2 (out and LSE finite), closed by accept().  Returns the past."""
    q, k, v = _rand(D, 2, seed)
    out, lse, past = attn.decode_multi(q, k, v, past, return_lse=True)
    assert out.shape == (1, HQ, 2, D) and lse.shape == (1, HQ, 2) and torch.isfinite(out).all() and torch.isfinite(lse).all()
    past = attn.accept(past)
    torch.cuda.synchronize()
    return past


@pytest.mark.parametrize("D,kw", [(128, {}), (64, {}), (128, {"arena": True}), (64, {"hd64_extents": True})],
                         ids=["d128-list", "d64-list", "d128-arena", "d64-extents"])
def test_multi_query_route_nothing_compressed(calls, D, kw):
    attn = _hook(D, **kw)
    past = _multi(attn, _prefilled(attn, D, 40), D)
    assert past[0] is None and past[4] == 0 and past[5] == 42
    assert _view_routes(calls) == [("multi_query", "null views", 0, "no tables")]


MULTI_GROWN = [
    # D, config, T_base and tables of the call over the cache one trigger has grown to 512 tokens
    (128, {}, 512, "no tables"),                                   # a list: T_base = C
    (64, {}, 512, "no tables"),
    (128, {"arena": True, "extents": False}, 512, "no tables"),    # an arena appended in place: at its base, its tokens
    (128, {"arena": True}, 256, "tables"),                         # an arena that grew by an extent: its base tokens
    (64, {"hd64_extents": True}, 256, "tables"),                   # ExtentCache64: its base tokens, always tables
]


@pytest.mark.parametrize("D,kw,t_base,tables", MULTI_GROWN, ids=["d128-list", "d64-list", "d128-arena-base", "d128-arena-grown", "d64-extents"])
def test_multi_query_route_after_a_trigger(calls, D, kw, t_base, tables):
    attn = _hook(D, **kw)
    past = _steps(attn, _prefilled(attn, D, 543), D, steps=1)
    assert past[4] == 512
    if kw:
        assert past[0].tokens == t_base and len(past[0].extents) == (512 - t_base) // 256
    past = _multi(attn, past, D)
    assert past[4] == 512 and past[5] == 546 and past[1].len == 34
    assert _view_routes(calls) == [("multi_query", "views", t_base, tables)]


def test_multi_query_route_extent_cache_at_its_base(calls):
    """An ExtentCache64 with no extent listed (consolidated) still names its tables."""
    attn = _hook(64, hd64_extents=True)
    p = _steps(attn, _prefilled(attn, 64, 543), 64, steps=1)
    past = _multi(attn, (p[0].consolidate(), p[1], p[2].consolidate(), p[3], p[4], p[5]), 64)
    assert past[0].tokens == 512 and not past[0].extents
    assert _view_routes(calls) == [("multi_query", "views", 512, "tables")]


@pytest.mark.parametrize("D,kw", [(128, {}), (64, {}), (128, {"arena": True}), (64, {"hd64_extents": True})],
                         ids=["d128-list", "d64-list", "d128-arena", "d64-extents"])
def test_shared_segment_route(calls, D, kw):
    """decode_segment over a SharedSegment of 256 tokens: two views and tokens = 256, whatever holds the segment."""
    attn = _hook(D, **kw)
    past = attn.to_fused(_prefilled(attn, D, 543))
    if kw:
        assert not isinstance(past[0], list) and past[0].tokens == 256 and not past[0].extents
    seg = partial.SharedSegment(past[0], past[2], 256, kv_heads=HKV)
    q, _, _ = _rand(D, 1, seed=5)
    out, lse = partial.decode_segment(attn, q, seg)
    torch.cuda.synchronize()
    assert out.shape == (1, HQ, 1, D) and lse.shape == (1, HQ) and torch.isfinite(out).all() and torch.isfinite(lse).all()
    assert _view_routes(calls) == [("shared_segment", "views", 256, "no tables")]
