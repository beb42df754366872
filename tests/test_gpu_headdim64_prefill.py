"""GPU: the head_dim-64 prefill compressed from the raw rows (mustafar_prefill_compress_hd + mustafar_cache_gather_hd behind
cache64.compress_raw_pair_hd64 and MustafarConfig(hd64_raw_prefill=True)) and ExtentCache64.consolidate() on the device.  Every
comparison is bit for bit: against prune + the two-pass conversion, against the oracle, against to_reference()."""
import ctypes

import numpy as np
import pytest
import torch

from mustafar_amd import cache64
from oracle import oracle as orc
from tests.hd64_ext_util import SENTINEL, ExtCase, Trigger, kth, run_triggers, same_reference
from tests.hd64_util import DEV, D, _cache, _rand, needle_data_64, needle_expect_64, oracle_prune

pytestmark = pytest.mark.gpu

PAIRS = [(0.7, 0.7), (0.5, 0.8), (0.0, 0.9), (0.99, 0.0)]
R = 32


@pytest.fixture(scope="module")
def pkg():
    from mustafar_amd import _lib, compression
    return _lib.load(), compression


def _old_route(x, tokens, s, which, pruned=False):
    """The parent's prefill of one side: prune, then the two-pass conversion."""
    from mustafar_amd import compression
    from mustafar_amd.hook import _compress
    Bp = x.shape[0] * x.shape[1]
    rows = x[:, :, :tokens].contiguous() if pruned else compression.prune_magnitude(x[:, :, :tokens], s)
    return _compress(rows.reshape(Bp, -1, D), which)


def _same(got, want):
    """same_reference and the same dtypes and shapes, the flat stream included."""
    for a, b in zip((got[0], got[1], got[3], got[2].flat), (want[0], want[1], want[3], want[2].flat)):
        assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(got[2].flat.view(torch.int16), want[2].flat.view(torch.int16)), "flat stream"
    assert [p.shape for p in got[2]] == [p.shape for p in want[2]]
    assert same_reference(got, want)


def _both(comp, K, V, C, ks, vs):
    gk, gv = cache64.compress_raw_pair_hd64(K, V, C, kth(ks), kth(vs))
    _same(gk, _old_route(K, C, ks, "key"))
    _same(gv, _old_route(V, C, vs, "value"))
    return gk, gv


# ---- 1. the prefill == prune + two-pass conversion == the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("ks,vs", PAIRS)
@pytest.mark.parametrize("C", [256, 512, 1280])
def test_raw_prefill_equals_prune_and_two_pass_conversion(pkg, C, ks, vs):
    """B' = 3, 1 / 2 / 5 chunks, L = C + 40 (head_stride != C x 64)."""
    comp = pkg[1]
    K, V, _ = _rand(1, 3, C + 40, 1, seed=C + int(100 * ks + 10 * vs))
    gk, gv = _both(comp, K, V, C, ks, vs)
    if (ks, vs, C) == (0.7, 0.7, 512):   # and the oracle: prune + compression of the same rows
        for got, x, s, conv in ((gk, K, ks, orc.convert_key_batched), (gv, V, vs, orc.convert_value_batched)):
            xp = orc.prune_magnitude(np.ascontiguousarray(x[0, :, :C].cpu().numpy()), s)
            obmp, oidx, onzs = conv(xp)
            assert np.array_equal(got[0].cpu().numpy(), obmp) and np.array_equal(got[1].cpu().numpy(), oidx)
            assert np.array_equal(got[3].cpu().numpy(), orc.nz_offset_from_idx(oidx))
            for h in range(3):
                assert np.array_equal(got[2][h].as_subclass(torch.Tensor).cpu().numpy().view(np.uint16), np.asarray(onzs[h]).view(np.uint16)), h


# ---- 2. transposed input ----------------------------------------------------------------------------------------------------------------
def test_raw_prefill_takes_transposed_views(pkg):
    """K and V as the model hands them over: transpose(1, 2) views of [B, L, H, 64] projections."""
    comp = pkg[1]
    C, L = 512, 552
    g = torch.Generator(device=DEV).manual_seed(21)
    K = torch.randn((1, L, 3, D), generator=g, device=DEV).half().transpose(1, 2)
    V = torch.randn((1, L, 3, D), generator=g, device=DEV).half().transpose(1, 2)
    assert not K.is_contiguous()
    _both(comp, K, V, C, 0.7, 0.7)


# ---- 3. zeros, negative zeros, ties ---------------------------------------------------------------------------------------------------------
def test_raw_prefill_on_zero_rows_negative_zeros_and_ties(pkg):
    """The rows of test_trigger_on_zero_rows_negative_zeros_and_ties in chunk 0 and again, shifted, in chunk 1."""
    comp = pkg[1]
    C, L = 512, 552
    rng = np.random.default_rng(5)
    Kn, Vn = (rng.standard_normal((1, 3, L, D)).astype(np.float16) for _ in range(2))
    for x in (Kn, Vn):
        for o in (0, 256 + 3):
            x[0, 0, o + 10:o + 20] = 0                                  # rows of exact zeros
            x[0, 0, o + 64:o + 128] = 0                                 # 64 of them (a whole block in chunk 0)
            x[0, 1, o + 30:o + 40] = -0.0
            x[0, 1, o + 70, ::2] = -0.0
            x[0, 2, o + 0:o + 64] = np.float16(0.5)                     # rows full of ties at the threshold: every value is kept
            x[0, 2, o + 100:o + 130] = np.where(np.arange(D) % 2, 0.25, -0.25).astype(np.float16)
            x[0, 2, o + 200, :40] = np.float16(1.0)                     # ties across the threshold's rank
            x[0, 2, o + 200, 40:] = np.float16(2.0)
    K, V = torch.from_numpy(Kn).to(DEV), torch.from_numpy(Vn).to(DEV)
    _both(comp, K, V, C, 0.7, 0.7)
    assert torch.equal(K.cpu().view(torch.int16), torch.from_numpy(Kn).view(torch.int16)), "the raw rows are read only"
    assert torch.equal(V.cpu().view(torch.int16), torch.from_numpy(Vn).view(torch.int16)), "the raw rows are read only"


# ---- 4. overflow and repeat --------------------------------------------------------------------------------------------------------------------
def test_a_chunk_full_of_ties_overflows_its_region_and_is_repeated_once(pkg):
    comp = pkg[1]
    C = 512
    K, V, _ = _rand(1, 3, C + 40, 1, seed=31)
    K[0, 1, 256:512] = 0.5                                   # head 1, second chunk only: every value is kept, 256 x 64 halfs
    assert cache64.hd64_staging_region(kth(0.7)) < 256 * D
    before = cache64.hd64_prefill_repeats
    _both(comp, K, V, C, 0.7, 0.7)
    assert cache64.hd64_prefill_repeats == before + 1


# ---- 5. kth == 0 ----------------------------------------------------------------------------------------------------------------------------------
def test_raw_prefill_with_kth_0_takes_pruned_rows_as_they_are(pkg):
    comp = pkg[1]
    C = 512
    K, V, _ = _rand(1, 3, C + 40, 1, seed=41)
    Kp, Vp = oracle_prune(K, 0.5), oracle_prune(V, 0.8)
    before = cache64.hd64_prefill_repeats
    gk, gv = cache64.compress_raw_pair_hd64(Kp, Vp, C, 0, 0)
    assert cache64.hd64_prefill_repeats == before, "kth = 0 houses every chunk at the dense size"
    _same(gk, _old_route(Kp, C, None, "key", pruned=True))
    _same(gv, _old_route(Vp, C, None, "value", pruned=True))


# ---- 6. the gather alone, through ctypes ---------------------------------------------------------------------------------------------------------
class _Ext:
    """One side of an extent run_triggers made, as ExtentCache64.to_reference() reads one."""

    def __init__(self, trig, s):
        t = trig.t[s]
        self.bmp, self.idx, self.nz, self.tot = t["bmp"], t["idx"], t["nz"], t["tot"].cpu().tolist()

    def reference(self):
        from mustafar_amd.hook import FlatStreams
        return [self.bmp.reshape(-1), self.idx.reshape(-1),
                FlatStreams([self.nz[h, :self.tot[h]].view(torch.float16) for h in range(self.bmp.shape[0])]), None]


@pytest.fixture(scope="module")
def gather_case(pkg):
    """B' = 3: a base of 512 tokens from the two-pass conversion of oracle-pruned rows, 3 extents from run_triggers on the raw rows
    behind them, per side the device table of the extents' views and to_reference() of base + extents.  Read only."""
    from mustafar_amd import _lib
    from mustafar_amd.cache64 import ExtentCache64
    from mustafar_amd.hook import FlatStreams
    L_, comp = pkg
    Bp, T0, n_ext, s = 3, 512, 3, 0.7
    K, V, _ = _rand(1, Bp, T0 + 256 * n_ext, 1, seed=61)
    trigs = []
    for i in range(n_ext):
        t0 = T0 + 256 * i
        trigs.append(Trigger(K[0, :, t0:t0 + 256].contiguous(), V[0, :, t0:t0 + 256].contiguous(), cap=320))
    run_triggers(L_, trigs, kth(s), kth(s))
    assert all(int(t.flag.item()) == 0 for t in trigs)
    vb = ctypes.sizeof(_lib.CacheView)
    sides = {}
    for x, which, sd in ((K, "key", "k"), (V, "value", "v")):
        bmp, idx, flat, off = _cache(oracle_prune(x[0, :, :T0], s).contiguous(), which, comp)
        ends = (idx.view(Bp, -1)[:, -1].to(torch.int64) * 2).cumsum(0).tolist()
        cache = ExtentCache64([bmp, idx, FlatStreams([flat[(ends[h - 1] if h else 0):ends[h]] for h in range(Bp)], flat), off], which, Bp, T0)
        cache.extents = [_Ext(t, sd) for t in trigs]
        raw = b"".join(ctypes.string_at(ctypes.byref(t.view(sd)), vb) for t in trigs)
        table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
        lens = (cache.base_used + sum(torch.tensor(e.tot) for e in cache.extents)).tolist()
        ext_lens = sum(torch.tensor(e.tot) for e in cache.extents).tolist()
        rows3 = oracle_prune(x[0, :, T0:], s).contiguous()
        sides[sd] = dict(cache=cache, table=table, want=cache.to_reference(), lens=lens, ext_lens=ext_lens,
                         want3=_old_route(rows3[None], 256 * n_ext, None, which, pruned=True))
    torch.cuda.synchronize()
    return dict(Bp=Bp, T0=T0, n=n_ext, sides=sides, keep=trigs)


def _dst(Bp, T, lens, pad=0, region=None):
    """Destination arrays full of sentinels: rows of T + pad bitmaps / T + 1 + pad offsets; the stream at exact size with nz_offset
    filled from `lens`, or (region, uint4 units) one region per head and no nz_offset."""
    from mustafar_amd import _lib
    bmp = torch.full((Bp, T + pad), -1, dtype=torch.int64, device=DEV)
    idx = torch.full((Bp, T + 1 + pad), -1, dtype=torch.int32, device=DEV)
    if region is None:
        starts = [0] + np.cumsum(lens).tolist()
        nz = torch.full((starts[-1],), SENTINEL, dtype=torch.int16, device=DEV)
        off = torch.tensor([v // 8 for v in starts[:-1]], dtype=torch.int32, device=DEV)
    else:
        starts = [8 * region * h for h in range(Bp + 1)]
        nz = torch.full((Bp * 8 * region,), SENTINEL, dtype=torch.int16, device=DEV)
        off = None
    view = _lib.CacheView(bmp.data_ptr(), nz.data_ptr(), idx.data_ptr(), off.data_ptr() if off is not None else None,
                          T + pad if pad else 0, T + 1 + pad if pad else 0, region or 0)
    return dict(bmp=bmp, idx=idx, nz=nz, off=off, view=view, starts=starts)


def _check_dst(d, want, Bp, T, lens):
    wb, wi, wz = want[0].view(Bp, T), want[1].view(Bp, T + 1), want[2]
    assert torch.equal(d["bmp"][:, :T], wb) and (d["bmp"][:, T:] == -1).all(), "bitmaps (columns beyond the tokens keep the sentinel)"
    assert torch.equal(d["idx"][:, :T + 1], wi) and (d["idx"][:, T + 1:] == -1).all(), "offsets"
    for h in range(Bp):
        got = d["nz"][d["starts"][h]:d["starts"][h + 1]]
        assert wz[h].numel() == lens[h]
        assert torch.equal(got[:lens[h]], wz[h].view(torch.int16)), f"stream of head {h}"
        assert not (got[:lens[h]] == SENTINEL).any() and (got[lens[h]:] == SENTINEL).all(), f"head {h}: a gap or a write behind the stream"


@pytest.mark.parametrize("variant", ["exact", "long_rows", "nz_stride", "no_first"])
def test_gather_through_the_c_abi(pkg, gather_case, variant):
    L_ = pkg[0]
    c = gather_case
    Bp, T0, n = c["Bp"], c["T0"], c["n"]
    st = torch.cuda.current_stream().cuda_stream
    for sd in "kv":
        s = c["sides"][sd]
        if variant == "no_first":
            T, lens, want = 256 * n, s["ext_lens"], s["want3"]
            d = _dst(Bp, T, lens)
            err = L_.mustafar_cache_gather_hd(st, ctypes.byref(d["view"]), None, 0, s["table"].data_ptr(), n, Bp, D)
        else:
            T, lens, want = T0 + 256 * n, s["lens"], s["want"]
            assert all(v % 8 == 0 for v in lens)
            d = _dst(Bp, T, lens, pad=64 if variant == "long_rows" else 0, region=max(lens) // 8 + 2 if variant == "nz_stride" else None)
            err = L_.mustafar_cache_gather_hd(st, ctypes.byref(d["view"]), s["cache"].view_ptr(), T0, s["table"].data_ptr(), n, Bp, D)
        assert err == 0
        torch.cuda.synchronize()
        _check_dst(d, want, Bp, T, lens)
        if d["off"] is not None:
            assert torch.equal(d["off"], want[3]), "the test's own nz_offset is the reference's"


# ---- 7. consolidate() on the device ------------------------------------------------------------------------------------------------------------------
def test_consolidate_on_the_device_equals_the_reference_route_and_decodes_the_same(pkg):
    L_ = pkg[0]
    B, Hkv, groups, T_base, n_ext, wl = 1, 2, 4, 512, 3, 40
    T = T_base + 256 * n_ext
    K, V, q = _rand(B, Hkv, T + wl, groups, seed=71)
    c = ExtCase(pkg, K, V, T_base, n_ext, groups, 0.5, 0.8)
    before = c.call_ext(q).clone()
    kc, vc = c.kc.consolidate(), c.vc.consolidate()
    kr, vr = c.kc.consolidate(via_reference=True), c.vc.consolidate(via_reference=True)
    for new, ref, old in ((kc, kr, c.kc), (vc, vr, c.vc)):
        assert type(new) is type(old) and new is not old and new.tokens == T and not new.extents and not new.table.any()
        assert same_reference(new.base, ref.base) and same_reference(new.to_reference(), old.to_reference())
        assert torch.equal(new.base_used, ref.base_used)
    st = torch.cuda.current_stream().cuda_stream
    tail = c._tail(q, T, c.wl, None, None, 0)
    err = L_.mustafar_decode_attention_extents_hd(st, kc.view_ptr(), vc.view_ptr(), T, kc.table.data_ptr(), vc.table.data_ptr(), *tail, None, D)
    assert err == 0
    torch.cuda.synchronize()
    assert torch.equal(c.out.view(torch.int16), before.view(torch.int16)), "decode over the consolidated cache != decode over base + extents"
    assert kc.consolidate() is kc, "a cache without extents is its own consolidation"


# ---- 8. the hook end to end --------------------------------------------------------------------------------------------------------------------------
def _attn(raw, ext=True, Hq=8, Hkv=2, ks=0.5, vs=0.8):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, api="fused", residual_length=R,
                                            k_sparsity=ks, v_sparsity=vs, hd64_extents=ext, hd64_raw_prefill=raw))


def _ref_of(c):
    return c.to_reference() if hasattr(c, "to_reference") else c


def test_hook_end_to_end_with_the_raw_prefill(pkg):
    """Prefill 1300 (1024 compressed tokens: four chunks), 20 steps (the trigger fires at kv 1312): `past` after the prefill and after
    the trigger and every step's output equal the flag-off hook's, bit for bit."""
    B, Hq, Hkv, prefill, steps = 2, 8, 2, 1300, 20
    K, V, _ = _rand(B, Hkv, prefill + steps, Hq // Hkv, seed=81)
    new, old = _attn(True), _attn(False)
    pn = new.build_cache(K[:, :, :prefill].clone(), V[:, :, :prefill].clone())
    po = old.build_cache(K[:, :, :prefill].clone(), V[:, :, :prefill].clone())
    assert pn[4] == po[4] == 1024 and pn[5] == po[5]
    assert same_reference(pn[0], po[0]) and same_reference(pn[2], po[2])
    assert torch.equal(pn[1], po[1]) and torch.equal(pn[3], po[3])
    gq = torch.Generator(device=DEV).manual_seed(8)
    fired = 0
    for i in range(steps):
        n = prefill + i + 1
        C = pn[4]
        q = torch.randn((B, Hq, 1, D), generator=gq, device=DEV).half()
        a, pn = new.decode(q, K[:, :, n - 1:n], V[:, :, n - 1:n], pn)
        b, po = old.decode(q, K[:, :, n - 1:n], V[:, :, n - 1:n], po)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"step {i} (kv {n}, compressed {C})"
        if pn[4] != C:
            fired += 1
            assert pn[4] == po[4] == 1280 and len(pn[0].extents) == 1
            assert same_reference(_ref_of(pn[0]), _ref_of(po[0])) and same_reference(_ref_of(pn[2]), _ref_of(po[2]))
    assert fired == 1
    assert same_reference(_ref_of(pn[0]), _ref_of(po[0])) and same_reference(_ref_of(pn[2]), _ref_of(po[2]))
    assert torch.equal(pn[1].view(), po[1].view()) and torch.equal(pn[3].view(), po[3].view())


# ---- 9. negative control ---------------------------------------------------------------------------------------------------------------------------------
def test_negative_control_a_zeroed_second_value_chunk_loses_exactly_its_rows(pkg):
    """Needle data through the raw prefill (three chunks): every row finds its needle's V row exactly.  With the second chunk of V
    zeroed in the RAW input exactly the rows whose needle sits in tokens [256, 512) miss: the later chunks are read from where the gather
    put them."""
    B, Hkv, groups, C, wl = 2, 2, 4, 768, 40
    n, Hq = C + wl, Hkv * groups
    rng = np.random.default_rng(9)
    fixed = [256, 511, 300, 255, 512, 0, C - 1, C, n - 1]
    pos = np.concatenate([fixed, rng.integers(0, n, B * Hq - len(fixed))]).reshape(B, Hq)
    K, V, q = needle_data_64(B, Hq, Hkv, n, pos, seed=9)
    attn = _attn(True, ext=False, Hq=Hq, Hkv=Hkv, ks=0.7, vs=0.7)
    want = needle_expect_64(V, pos, C, groups)

    def run(Vx):
        past = attn.build_cache(K[:, :, :n - 1].clone(), Vx[:, :, :n - 1].clone())
        assert past[4] == C
        out, _ = attn.decode(q, K[:, :, n - 1:n], Vx[:, :, n - 1:n], past)
        torch.cuda.synchronize()
        return (out.float() != want.float()).any(-1).reshape(B, Hq).cpu().numpy()

    assert not run(V).any(), "rows miss their needles"
    Vz = V.clone()
    Vz[:, :, 256:512] = 0
    inside = (pos >= 256) & (pos < 512)
    assert inside.sum() >= 3
    assert np.array_equal(run(Vz), inside), "exactly the rows whose needle sits in the zeroed chunk must miss"
