"""CPU: the head_dim-64 prefill / gather surface of the C ABI (ABI 109), the hook's hd64_raw_prefill rule and the staging bound of
cache64.compress_raw_pair_hd64.  No kernel runs: every call here must fail validation before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mustafar_prefill_compress_hd", "mustafar_cache_gather_hd")


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "mustafar_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"^\s*(?:int|int64_t)\s+(\w+)\s*\(", text, flags=re.M))


def test_new_symbols_are_declared_bound_and_exported():
    from mustafar_amd import _lib
    syms = _header_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in syms and s in _lib.SIGNATURES and hasattr(raw, s), s
    assert _lib.load().mustafar_abi_version() >= 109


def _view(**kw):
    from mustafar_amd import _lib
    a = dict(bmp=16, nz=16, idx=16, nz_offset=16, bmp_head_stride=0, idx_head_stride=0, nz_head_stride=0)
    a.update(kw)
    return _lib.CacheView(**a)


def _stage(**kw):
    a = dict(bmp_head_stride=256, idx_head_stride=257, nz_head_stride=64)
    a.update(kw)
    return _view(**a)


def _prefill(L, **kw):
    one = 16   # never dereferenced: validation fails first (16-byte aligned, so that only the argument under test is wrong)
    a = dict(k_x=64, v_x=64, hs=1064 * 64, Bp=2, t=1024, D=64, kk=44, kv=44, k_stage=_stage(), v_stage=_stage(), kcb=4096, vcb=4096,
             k_pieces=one, v_pieces=one, k_tot=one, v_tot=one, kr=512, vr=512, flag=one)
    a.update(kw)
    r = lambda v: ctypes.byref(v) if v is not None else None
    return L.mustafar_prefill_compress_hd(None, a["k_x"], a["v_x"], a["hs"], a["Bp"], a["t"], a["D"], a["kk"], a["kv"], r(a["k_stage"]),
                                          r(a["v_stage"]), a["kcb"], a["vcb"], a["k_pieces"], a["v_pieces"], a["k_tot"], a["v_tot"], a["kr"],
                                          a["vr"], a["flag"])


@pytest.mark.parametrize("bad", [
    dict(D=128), dict(D=96),
    dict(t=0), dict(t=300), dict(t=513 * 256, hs=513 * 256 * 64),
    dict(hs=1064 * 64 + 4), dict(hs=1000 * 64),                     # head_stride % 8, head_stride shorter than the rows
    dict(kr=0), dict(vr=0), dict(kr=520),                           # no region size / more than the view's stride holds
    dict(flag=None), dict(k_tot=None), dict(v_tot=None),
    dict(k_x=None), dict(v_x=72), dict(Bp=0), dict(kk=65), dict(kv=-1),
    dict(kcb=0), dict(vcb=4100), dict(k_stage=None), dict(v_stage=None),
    dict(k_stage=_stage(nz_head_stride=0)), dict(v_stage=_stage(bmp_head_stride=128)), dict(k_stage=_stage(idx_head_stride=256)),
    dict(v_stage=_stage(nz=24)), dict(k_stage=_stage(bmp=None)),
])
def test_prefill_compress_hd_rejects_bad_arguments_without_a_launch(bad):
    from mustafar_amd import _lib
    assert _prefill(_lib.load(), **bad) == 1


def _gather(L, **kw):
    a = dict(dst=_view(), first=_view(), first_tokens=512, pieces=16, n=3, Bp=2, D=64)
    a.update(kw)
    r = lambda v: ctypes.byref(v) if v is not None else None
    return L.mustafar_cache_gather_hd(None, r(a["dst"]), r(a["first"]), a["first_tokens"], a["pieces"], a["n"], a["Bp"], a["D"])


@pytest.mark.parametrize("bad", [
    dict(D=128), dict(D=96),
    dict(n=513), dict(first_tokens=100), dict(pieces=None), dict(n=-1),
    dict(first=None), dict(first_tokens=0), dict(first=None, first_tokens=0, n=0),      # view and token count must agree; nothing to gather
    dict(dst=None), dict(Bp=0),
    dict(dst=_view(nz=24)), dict(dst=_view(bmp=None)), dict(dst=_view(idx=None)), dict(dst=_view(nz=None)),
    dict(dst=_view(nz_offset=None)),                                                   # neither a stream stride nor loaded offsets
    dict(dst=_view(bmp_head_stride=1279)), dict(dst=_view(idx_head_stride=1280)),      # rows shorter than 512 + 3 x 256 tokens
    dict(first=_view(bmp_head_stride=511)), dict(first=_view(idx_head_stride=512)), dict(first=_view(nz_head_stride=-1)),
    dict(first=_view(nz=8)),
])
def test_cache_gather_hd_rejects_bad_arguments_without_a_launch(bad):
    from mustafar_amd import _lib
    assert _gather(_lib.load(), **bad) == 1


def test_hd64_raw_prefill_configuration_rules():
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    MustafarAttention(MustafarConfig(num_attention_heads=32, num_key_value_heads=8, head_dim=64, api="fused", hd64_raw_prefill=True))
    MustafarAttention(MustafarConfig(num_attention_heads=32, num_key_value_heads=8, head_dim=64, api="fused", hd64_raw_prefill=True,
                                     hd64_extents=True))
    assert MustafarConfig().hd64_raw_prefill is False
    for kw in (dict(head_dim=128, api="fused"), dict(head_dim=128, api="native"), dict(head_dim=128, api="fused", arena=True)):
        with pytest.raises(ValueError, match="hd64_raw_prefill"):
            MustafarAttention(MustafarConfig(hd64_raw_prefill=True, **kw))
    for kw in (dict(api="native"), dict(api="fused", arena=True)):
        with pytest.raises(ValueError):
            MustafarAttention(MustafarConfig(head_dim=64, hd64_raw_prefill=True, **kw))


def _distinct_rows(rng, rows):
    """[rows, 64] fp16, every row a shuffled ramp of 64 distinct magnitudes (k / 64, exact in fp16 and in fp32) with random signs: no
    two values of a row tie, so the prune keeps exactly 64 - kth + 1 of them."""
    ramp = np.arange(1, 65, dtype=np.float32) / 64
    x = np.stack([rng.permutation(ramp) for _ in range(rows)]) * rng.choice([-1.0, 1.0], (rows, 64))
    h = x.astype(np.float16)
    assert (h.astype(np.float32) == x).all() and all(len(set(np.abs(r).tolist())) == 64 for r in h)
    return h


@pytest.mark.parametrize("kth", list(range(1, 65)))
def test_staging_region_bounds_the_oracles_longest_chunk_on_tie_free_rows(kth):
    """The bound, not luck, keeps the common case from repeating: on 200 random tie-free rows (the chunk's other 56 rows repeat some of
    them) the oracle's stream of a 256-token chunk, K and V geometry, is no longer than cache64.hd64_staging_region(kth)."""
    from mustafar_amd import cache64
    rng = np.random.default_rng(kth)
    rows = _distinct_rows(rng, 200)
    chunk = np.concatenate([rows, rows[rng.integers(0, 200, 56)]])[None]
    pruned = orc.prune_magnitude(chunk, kth / 64)            # max(1, int(kth / 64 * 64)) == kth exactly
    assert orc.kth_from_sparsity(kth / 64, 64) == kth
    assert ((pruned.view(np.uint16) & 0x7fff) != 0).sum(-1).tolist() == [[64 - kth + 1] * 256], "the rows are not tie-free"
    bound = cache64.hd64_staging_region(kth)
    assert bound % 8 == 0 and bound <= 256 * 64
    for conv in (orc.convert_key_batched, orc.convert_value_batched):
        _, accum, _ = conv(pruned)
        assert 2 * int(accum[0, -1]) <= bound, (kth, conv.__name__)


def test_staging_region_formula():
    from mustafar_amd import cache64
    assert cache64.hd64_staging_region(0) == 256 * 64                          # rows pruned by the caller: anything may be kept
    assert cache64.hd64_staging_region(44) == 256 * 21 + 7 * 256               # 70 %
    assert cache64.hd64_staging_region(1) == cache64.hd64_staging_region(8) == 256 * 64   # bound above the dense rows
    assert cache64.hd64_staging_region(64) == 256 + 7 * 256
