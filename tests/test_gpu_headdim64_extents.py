"""GPU: the head_dim-64 cache that grows by extents -- the one-launch trigger (mustafar_trigger_compress_batch_hd) bit for bit against
the oracle's prune + compress, the EXT instantiation of the decode kernel (mustafar_decode_attention_extents_hd) bit for bit against the
plain launch, through runs that straddle base / extents, with a device-side T under one captured graph, and the hook end to end
(MustafarConfig(hd64_extents=True)) against the tuple cache."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.exact_data import model_ok
from tests.hd64_ext_util import (ExtCase, Trigger, assert_extent_equals_oracle, kth, oracle_extent, run_triggers, same_reference)
from tests.hd64_util import DEV, D, _left_pad_mask, _rand, needle_data_64, needle_expect_64, oracle_prune, run_shape
from tests.test_headdim64_extents_host import EXT_SHAPES

pytestmark = pytest.mark.gpu

PAIRS = [(0.7, 0.7), (0.5, 0.8), (0.0, 0.9), (0.99, 0.0)]
R = 32


@pytest.fixture(scope="module")
def pkg():
    from mustafar_amd import _lib, compression
    return _lib.load(), compression


def _rows(Bp, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((Bp, 256, D)).astype(np.float16), rng.standard_normal((Bp, 256, D)).astype(np.float16)


def _dev(x):
    return torch.from_numpy(x).to(DEV)


def _ok(out, q, Kd, Vd, groups, pads=None):
    """model_ok over K / V that are pruned already where they are compressed."""
    model_ok(out, q, Kd, Vd, 0, groups, pads=pads, pruned=(Kd[:, :, :0], Vd[:, :, :0]))


def _misses(out, want):
    return (out.float() != want.float()).any(-1).nonzero().tolist()


# ---- 1. compression ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks,vs", PAIRS)
def test_trigger_is_the_oracles_prune_and_compress(pkg, ks, vs):
    """B' = 3, a window buffer of 320 rows (head_stride != 256 x 64), the 256 rows at offset 0."""
    Kw, Vw = _rows(3, int(100 * ks + vs * 10))
    t = Trigger(_dev(Kw), _dev(Vw), cap=320)
    run_triggers(pkg[0], [t], kth(ks), kth(vs))
    assert int(t.flag.item()) == 0
    for s, x, sp in (("k", Kw, ks), ("v", Vw, vs)):
        want = oracle_extent(x, sp, s)
        assert_extent_equals_oracle(t, s, want)
        if sp == 0.0:   # nothing pruned: every block's stream is the full 4096 halfs
            assert (2 * (want[1][:, 64::64].astype(np.int64) - want[1][:, :-1:64]) == 4096).all()
            assert (t.result(s)[2] == 4 * 4096).all()


def test_trigger_on_zero_rows_negative_zeros_and_ties(pkg):
    Kw, Vw = _rows(3, 5)
    for x in (Kw, Vw):
        x[0, 10:20] = 0                                  # rows of exact zeros
        x[0, 64:128] = 0                                 # a whole block of them
        x[1, 30:40] = -0.0
        x[1, 70, ::2] = -0.0
        x[2, 0:64] = np.float16(0.5)                     # rows full of ties at the threshold: every value is kept
        x[2, 100:130] = np.where(np.arange(D) % 2, 0.25, -0.25).astype(np.float16)
        x[2, 200, :40] = np.float16(1.0)                 # ties across the threshold's rank (40 equal values, 44 to prune of 64)
        x[2, 200, 40:] = np.float16(2.0)
    t = Trigger(_dev(Kw), _dev(Vw), cap=320)
    run_triggers(pkg[0], [t], kth(0.7), kth(0.7))
    assert int(t.flag.item()) == 0
    for s, x in (("k", Kw), ("v", Vw)):
        assert_extent_equals_oracle(t, s, oracle_extent(x, 0.7, s))


def test_trigger_with_kth_0_takes_pruned_rows_as_they_are(pkg):
    Kw, Vw = _rows(3, 6)
    Kp, Vp = orc.prune_magnitude(Kw, 0.5), orc.prune_magnitude(Vw, 0.8)
    t = Trigger(_dev(Kp), _dev(Vp), cap=320)
    run_triggers(pkg[0], [t], 0, 0)
    assert int(t.flag.item()) == 0
    assert_extent_equals_oracle(t, "k", oracle_extent(Kp, None, "k", pruned=True))
    assert_extent_equals_oracle(t, "v", oracle_extent(Vp, None, "v", pruned=True))
    assert torch.equal(t.kw[:, :256].cpu(), torch.from_numpy(Kp)), "the window rows are read only"


def test_three_items_in_one_call_equal_three_calls(pkg):
    data = [_rows(3, 20 + i) for i in range(3)]
    a = [Trigger(_dev(k), _dev(v), cap=320) for k, v in data]
    b = [Trigger(_dev(k), _dev(v), cap=320) for k, v in data]
    run_triggers(pkg[0], a, kth(0.5), kth(0.8), batched=True)
    run_triggers(pkg[0], b, kth(0.5), kth(0.8), batched=False)
    for i, (x, y) in enumerate(zip(a, b)):
        assert int(x.flag.item()) == 0 and int(y.flag.item()) == 0
        for s in "kv":
            for name in ("bmp", "idx", "off", "nz", "tot"):
                assert torch.equal(x.t[s][name], y.t[s][name]), (i, s, name)
        assert_extent_equals_oracle(x, "k", oracle_extent(data[i][0], 0.5, "k"))
        assert_extent_equals_oracle(x, "v", oracle_extent(data[i][1], 0.8, "v"))


def test_a_region_one_piece_short_overflows_and_the_repeat_is_exact(pkg):
    Kw, Vw = _rows(3, 9)
    Kw[1, :, :] = np.float16(0.5)                        # head 1 of K: ties keep every value: the longest stream by far
    wk, wv = oracle_extent(Kw, 0.7, "k"), oracle_extent(Vw, 0.7, "v")
    lens = [len(z) for z in wk[2]]
    assert lens[1] == 256 * D and max(lens[0], lens[2]) <= lens[1] - 8
    t = Trigger(_dev(Kw), _dev(Vw), cap=320, k_region=lens[1] - 8, v_region=256 * D)   # one 16-byte piece short for head 1
    run_triggers(pkg[0], [t], kth(0.7), kth(0.7))
    assert int(t.flag.item()) == 1
    assert_extent_equals_oracle(t, "k", wk, skip_stream=(1,))     # head_total = the oracle's length, region untouched, others complete
    assert_extent_equals_oracle(t, "v", wv)
    again = Trigger(_dev(Kw), _dev(Vw), cap=320, k_region=int(t.result("k")[2].max()), v_region=256 * D)
    run_triggers(pkg[0], [again], kth(0.7), kth(0.7))
    assert int(again.flag.item()) == 0
    assert_extent_equals_oracle(again, "k", wk)
    assert_extent_equals_oracle(again, "v", wv)


# ---- 2. decode over extents == the plain launch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 4, 8])
def test_extents_decode_equals_the_plain_launch_bit_for_bit(pkg, groups):
    """Same run shape at the same T: same slabs, same sum order, so the same bits.  to_reference() is also the tuple path's
    append_compressed of the same tokens, bit for bit."""
    from mustafar_amd.hook import _compress, append_compressed
    L_ = pkg[0]
    B, Hkv, wl, ks, vs = 1, 2, 45, 0.5, 0.8
    for T_base in (256, 512):
        for n_ext in (1, 2, 3):
            T = T_base + 256 * n_ext
            assert run_shape(L_, T, B * Hkv * groups, groups) == (T // 64, 1)
            K, V, q = _rand(B, Hkv, T + wl, groups, seed=T + groups)
            c = ExtCase(pkg, K, V, T_base, n_ext, groups, ks, vs)
            a = c.call_ext(q).clone()
            assert L_.mustafar_last_decode_choice() == (1 << 4) | (6 << 8)
            b = c.call_plain(q).clone()
            assert L_.mustafar_last_decode_choice() == (1 << 4) | (5 << 8)
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (T_base, n_ext)
            model_ok(a, q, K, V, T, groups, k_sparsity=ks, v_sparsity=vs, pruned=(c.Kp, c.Vp))
            for cache, xp, which in ((c.kc, c.Kp, "key"), (c.vc, c.Vp, "value")):   # the tuple path: prune, compress, append per trigger
                ref = _compress(xp[:, :, :T_base].reshape(B * Hkv, T_base, D), which)
                for i in range(n_ext):
                    t0 = T_base + 256 * i
                    ref = append_compressed(ref, _compress(xp[:, :, t0:t0 + 256].reshape(B * Hkv, 256, D), which), B * Hkv, t0, 256, D)
                assert same_reference(cache.to_reference(), ref), (which, T_base, n_ext)


# ---- 3. runs that straddle ---------------------------------------------------------------------------------------------------------------
def _ext_positions(T_base, n_ext, n):
    """The last base block, the first and last block of every extent (first and last token of each), both sides of the window edge."""
    T = T_base + 256 * n_ext
    pos = [T_base - 64, T_base - 1, T - 1, T, n - 2, n - 1]
    for i in range(n_ext):
        e = T_base + 256 * i
        pos += [e, e + 63, e + 192, e + 255]
    return sorted(set(pos))


@pytest.mark.parametrize("name", ["bpw3", "bpw3x", "bpw2"])
def test_runs_that_straddle_base_and_extents(pkg, name):
    L_ = pkg[0]
    Bp, T_base, n_ext, bpw, S1 = EXT_SHAPES[name]
    groups, wl, B, Hkv = 4, 70, 8, 8
    T = T_base + 256 * n_ext
    assert run_shape(L_, T, Bp * groups, groups) == (S1, bpw), "the launch heuristic changed: this test needs its run shape"
    K, V, q = _rand(B, Hkv, T + wl, groups, seed=bpw + n_ext)
    c = ExtCase(pkg, K, V, T_base, n_ext, groups, 0.7, 0.7)
    model_ok(c.call_ext(q), q, K, V, T, groups, pruned=(c.Kp, c.Vp))
    # needles, bit for bit: every row has 2 equal needles (the exact mean of two V rows), the first on the edges below; the three rows behind
    # the edge rows have both in two different extents / on both sides of the base's end
    n, Hq = T + wl, Hkv * groups
    rng = np.random.default_rng(bpw)
    edges = _ext_positions(T_base, n_ext, n)
    first = np.concatenate([edges, rng.integers(0, n, B * Hq - len(edges))]).reshape(B, Hq)
    pos = np.stack([first, (first + 1 + rng.integers(0, n - 1, first.shape)) % n], -1)
    flat = pos.reshape(-1, 2)                            # (a view: the rows behind the edge rows)
    flat[len(edges)] = [T_base + 5, T_base + 256 + 70]
    flat[len(edges) + 1] = [T_base + 255, T - 2]
    flat[len(edges) + 2] = [T_base - 3, T_base + 63]
    assert set(edges) <= set(pos[..., 0].ravel().tolist()) and len(edges) + 3 <= B * Hq
    Kn, Vn, qn = needle_data_64(B, Hq, Hkv, n, pos, seed=bpw)
    cn = ExtCase(pkg, Kn, Vn, T_base, n_ext, groups, 0.7, 0.7)
    assert not _misses(cn.call_ext(qn), needle_expect_64(Vn, pos, T, groups)), "rows miss their needles"


# ---- 4. one graph, a device-side T, three triggers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_one_graph_with_device_side_T_through_three_triggers(pkg, masked):
    """A graph captured at T_base = 512 with capacity 512 + 768 is replayed through three triggers (each run eagerly: 256 added to the
    device T, 256 taken off the step counter).  Queries alternate between random ones (the model's bound) and the needle query (bit
    equality for every row whose needle token exists).  masked: a left-padding mask whose pads end inside an extent."""
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    L_ = pkg[0]
    B, Hq, Hkv, ks, vs = 2, 8, 2, 0.5, 0.8
    groups = Hq // Hkv
    L0 = 512 + R + 250
    steps = 6 + 512 + 10
    n_all = L0 + steps
    rng = np.random.default_rng(11)
    spots = [0, 511, 512, 575, 704, 767, 768, 1023, 1024, 1279, 1280, L0 - 1, L0 + 3, n_all - 1]
    pos = np.concatenate([spots, rng.integers(0, n_all, B * Hq - len(spots))]).reshape(B, Hq)
    K, V, qn = needle_data_64(B, Hq, Hkv, n_all, pos, seed=3)
    Kpr, Vpr = oracle_prune(K, ks), oracle_prune(V, vs)
    pads = [0, 600] if masked else None                  # 600: inside the first extent (tokens 512 .. 767)
    attn = MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, api="fused", residual_length=R,
                                            k_sparsity=ks, v_sparsity=vs, hd64_extents=True))
    past = attn.to_fused(attn.build_cache(K[:, :, :L0].clone(), V[:, :, :L0].clone()))
    C0, cap = past[4], past[4] + 768
    assert C0 == 512 and not past[0].extents
    wcap = past[1].cap
    mask = _left_pad_mask(B, cap + wcap, pads) if masked else None
    t_dev = torch.tensor([C0], dtype=torch.int32, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    q, k, v = (torch.zeros(B, h, 1, D, device=DEV).half() for h in (Hq, Hkv, Hkv))
    warm = (past[0], past[1].clone(), past[2], past[3].clone(), past[4], past[5])
    attn.decode_fused(q, k, v, warm, step_counter=counter, attention_mask=mask, t_device=t_dev, t_capacity=cap)
    # at *T_device == T_base no extent is listed: every extent workgroup left a slab of weight zero
    torch.cuda.synchronize()
    S1 = cap // 64
    assert run_shape(L_, cap, B * Hq, groups) == (S1, 1)
    _, ws = attn._scratch(DEV, B * Hq, (cap + wcap + 31) // 32 * 32, L_.mustafar_decode_workspace_bytes_hd(cap, B * Hq, groups, 1, D))
    ml = ws[:(S1 + 16) * B * Hq * 66 * 4].view(torch.float32)[(S1 + (wcap + 63) // 64) * B * Hq * D:].view(-1, B * Hq, 2)
    assert (ml[C0 // 64:S1, :, 1] == 0).all() and torch.isinf(ml[C0 // 64:S1, :, 0]).all() and (ml[:C0 // 64, :, 1] > 0).all()
    assert not past[0].table.any() and not past[2].table.any()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, _ = attn.decode_fused(q, k, v, past, step_counter=counter, attention_mask=mask, t_device=t_dev, t_capacity=cap)
        assert L_.mustafar_counter_add(torch.cuda.current_stream().cuda_stream, counter.data_ptr(), 1) == 0
    sig = (past[0].signature(), past[2].signature(), past[1].buf.data_ptr(), past[3].buf.data_ptr())
    gq = torch.Generator(device=DEV).manual_seed(4)
    state, since, triggers = past, 0, 0
    for step in range(steps):
        n = L0 + step + 1
        needle = step % 2 == 1
        qs = qn if needle else torch.randn((B, Hq, 1, D), generator=gq, device=DEV).half()
        kn, vn = K[:, :, n - 1:n], V[:, :, n - 1:n]
        if (n - R - state[4]) % 256 == 0 and state[1].len + since + 1 >= 256:   # this step fires the trigger: eagerly
            m = None if mask is None else _left_pad_mask(B, n, pads)
            got, state = attn.decode(qs, kn, vn, attn.advance(state, since), attention_mask=m)
            since, triggers = 0, triggers + 1
            t_dev.add_(256)
            counter.add_(1 - 256)
            C_step = state[4] - 256
        else:
            q.copy_(qs); k.copy_(kn); v.copy_(vn)
            g.replay()
            got, since, C_step = out, since + 1, state[4]
        if needle:
            here = torch.from_numpy(pos < n).to(DEV)
            want = needle_expect_64(V, pos, C_step, groups, vs=vs)
            keep = here if pads is None else here & torch.from_numpy(pos >= np.asarray(pads)[:, None]).to(DEV)
            bad = ((got.float() != want.float()).any(-1).reshape(B, Hq) & keep).nonzero().tolist()
            assert not bad, f"step {step} (kv {n}, compressed {C_step}): rows {bad} miss their needle"
        else:
            Kd = torch.cat([Kpr[:, :, :C_step], K[:, :, C_step:n]], 2)
            Vd = torch.cat([Vpr[:, :, :C_step], V[:, :, C_step:n]], 2)
            _ok(got, qs, Kd, Vd, groups, pads)
    assert triggers == 3 and state[4] == cap and len(state[0].extents) == 3
    assert sig == (state[0].signature(), state[2].signature(), state[1].buf.data_ptr(), state[3].buf.data_ptr())


# ---- 5. the hook end to end --------------------------------------------------------------------------------------------------------------
def _attn(ext, Hq=8, Hkv=2, ks=0.5, vs=0.8, cls=None):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    a = MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, api="fused", residual_length=R,
                                         k_sparsity=ks, v_sparsity=vs, hd64_extents=ext))
    if cls is not None:
        a.EXTENT_CACHE_64 = cls
    return a


def _ref_of(c):
    return c.to_reference() if hasattr(c, "to_reference") else c


@pytest.mark.parametrize("prefill", [600, 100])
def test_hook_end_to_end_against_the_tuple_cache(pkg, prefill):
    """Prefill 600 (a base of 512) or 100 (the first trigger starts from C = 0), 600 generated tokens at (0.5, 0.8), batch 2, 8 / 2
    heads: every step within the model's bound, bit-equal to the tuple path wherever both launch the same run shape (every step here:
    one block per workgroup at these lengths), final caches bit-equal in the reference layout."""
    L_ = pkg[0]
    B, Hq, Hkv, ks, vs, steps = 2, 8, 2, 0.5, 0.8, 600
    groups = Hq // Hkv
    K, V, _ = _rand(B, Hkv, prefill + steps, groups, seed=prefill)
    Kpr, Vpr = oracle_prune(K, ks), oracle_prune(V, vs)
    new, old = _attn(True), _attn(False)
    pn = new.build_cache(K[:, :, :prefill].clone(), V[:, :, :prefill].clone())
    po = old.build_cache(K[:, :, :prefill].clone(), V[:, :, :prefill].clone())
    gq = torch.Generator(device=DEV).manual_seed(1)
    for i in range(steps):
        n = prefill + i + 1
        C = pn[4]
        assert C == po[4] and run_shape(L_, C, B * Hq, groups) == (C // 64, 1)
        q = torch.randn((B, Hq, 1, D), generator=gq, device=DEV).half()
        a, pn = new.decode(q, K[:, :, n - 1:n], V[:, :, n - 1:n], pn)
        b, po = old.decode(q, K[:, :, n - 1:n], V[:, :, n - 1:n], po)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"step {i} (kv {n}, compressed {C})"
        if i % 8 == 0 or (n - R - C) % 256 in (0, 1, 255):
            Kd = torch.cat([Kpr[:, :, :C], K[:, :, C:n]], 2)
            Vd = torch.cat([Vpr[:, :, :C], V[:, :, C:n]], 2)
            _ok(a, q, Kd, Vd, groups)
    assert pn[4] == po[4] == (1024 if prefill == 600 else 512) and len(pn[0].extents) == (2 if prefill == 600 else 1)
    assert same_reference(_ref_of(pn[0]), po[0]) and same_reference(_ref_of(pn[2]), po[2])
    assert torch.equal(pn[1].view(), po[1].view()) and torch.equal(pn[3].view(), po[3].view())


def test_run_triggers_over_three_layers_equals_layer_by_layer(pkg):
    B, Hq, Hkv, layers, prefill = 2, 8, 2, 3, 512 + R + 254
    attn = _attn(True)
    gq = torch.Generator(device=DEV).manual_seed(2)
    data = [_rand(B, Hkv, prefill + 4, 4, seed=50 + l)[:2] for l in range(layers)]
    bat = [attn.to_fused(attn.build_cache(K[:, :, :prefill].clone(), V[:, :, :prefill].clone())) for K, V in data]
    one = [attn.to_fused(attn.build_cache(K[:, :, :prefill].clone(), V[:, :, :prefill].clone())) for K, V in data]
    fired = 0
    for i in range(4):
        n = prefill + i + 1
        for l, (K, V) in enumerate(data):
            q = torch.randn((B, Hq, 1, D), generator=gq, device=DEV).half()
            a, bat[l] = attn.decode_fused(q, K[:, :, n - 1:n], V[:, :, n - 1:n], bat[l], defer_trigger=True)
            b, one[l] = attn.decode(q, K[:, :, n - 1:n], V[:, :, n - 1:n], one[l])
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (i, l)
        if all(attn.trigger_due(p) for p in bat):
            fired += 1
            bat = attn.run_triggers(bat)
    assert fired == 1
    for x, y in zip(bat, one):
        assert x[4] == y[4] == 768 and len(x[0].extents) == 1 and x[1].len == y[1].len
        assert same_reference(x[0].to_reference(), y[0].to_reference()) and same_reference(x[2].to_reference(), y[2].to_reference())
        assert torch.equal(x[1].view(), y[1].view()) and torch.equal(x[3].view(), y[3].view())


def test_a_full_table_consolidates_on_the_third_trigger(pkg):
    from mustafar_amd.cache64 import ExtentCache64

    class Small(ExtentCache64):
        MAX_EXTENTS = 2

    B, Hq, Hkv, ks, vs, prefill = 2, 8, 2, 0.5, 0.8, 256 + R + 250
    steps = 6 + 512 + 4
    groups = Hq // Hkv
    K, V, _ = _rand(B, Hkv, prefill + steps, groups, seed=77)
    Kpr, Vpr = oracle_prune(K, ks), oracle_prune(V, vs)
    attn, old = _attn(True, cls=Small), _attn(False)
    past = attn.build_cache(K[:, :, :prefill].clone(), V[:, :, :prefill].clone())
    po = old.build_cache(K[:, :, :prefill].clone(), V[:, :, :prefill].clone())
    gq = torch.Generator(device=DEV).manual_seed(5)
    seen = []
    for i in range(steps):
        n = prefill + i + 1
        C = past[4]
        q = torch.randn((B, Hq, 1, D), generator=gq, device=DEV).half()
        before = past[0]
        out, past = attn.decode(q, K[:, :, n - 1:n], V[:, :, n - 1:n], past)
        _, po = old.decode(q, K[:, :, n - 1:n], V[:, :, n - 1:n], po)
        if past[4] != C:
            seen.append((past[0].tokens, len(past[0].extents)))
            assert same_reference(past[0].to_reference(), po[0]) and same_reference(past[2].to_reference(), po[2])
            if len(seen) == 3:   # the third trigger met a full table: the old cache's content moved into a new base, unchanged
                assert isinstance(past[0], Small) and past[0] is not before and past[0].tokens == 768
        if i % 16 == 0 or past[4] != C or n - R - C in (257, 258):
            Kd = torch.cat([Kpr[:, :, :C], K[:, :, C:n]], 2)
            Vd = torch.cat([Vpr[:, :, :C], V[:, :, C:n]], 2)
            _ok(out, q, Kd, Vd, groups)
    assert seen == [(256, 1), (256, 2), (768, 1)]


# ---- 6. negative control -------------------------------------------------------------------------------------------------------------------
def test_negative_control_a_zeroed_value_extent_loses_exactly_its_rows(pkg):
    """The V table entry of extent 1 is pointed at a zeroed extent (zero bitmaps: every value reads as zero; no wild pointer): exactly
    the rows whose needle sits in that extent miss, every other row still matches."""
    from mustafar_amd import _lib
    import ctypes
    B, Hkv, groups, T_base, n_ext, wl = 2, 2, 4, 512, 3, 40
    T = T_base + 256 * n_ext
    n, Hq = T + wl, Hkv * groups
    rng = np.random.default_rng(8)
    fixed = [T_base + 256, T_base + 511, T_base + 300, T_base + 255, T_base + 512, 0, T, n - 1]
    pos = np.concatenate([fixed, rng.integers(0, n, B * Hq - len(fixed))]).reshape(B, Hq)
    K, V, q = needle_data_64(B, Hq, Hkv, n, pos, seed=8)
    c = ExtCase(pkg, K, V, T_base, n_ext, groups, 0.7, 0.7)
    want = needle_expect_64(V, pos, T, groups)
    assert not _misses(c.call_ext(q).clone(), want)
    e = c.vc.extents[1]
    zb, zi = torch.zeros_like(e.bmp), torch.zeros_like(e.idx)
    zn = torch.zeros((8,), dtype=torch.float16, device=DEV)
    zero = _lib.CacheView(zb.data_ptr(), zn.data_ptr(), zi.data_ptr(), None, 256, 257, 0)
    table = c.vc.table.clone()
    vb = ctypes.sizeof(_lib.CacheView)
    table[vb:2 * vb] = torch.frombuffer(bytearray(ctypes.string_at(ctypes.byref(zero), vb)), dtype=torch.uint8).to(DEV)
    got = c.call_ext(q, v_table=table)
    torch.cuda.synchronize()
    inside = (pos >= T_base + 256) & (pos < T_base + 512)
    assert inside.sum() >= 3
    miss = (got.float() != want.float()).any(-1).reshape(B, Hq).cpu().numpy()
    assert np.array_equal(miss, inside), "exactly the rows whose needle sits in the zeroed extent must miss"
