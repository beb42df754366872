"""GPU: fused decode, the 256-token trigger and the device threshold search away from the usual operating point (k_sparsity ==
v_sparsity == 0.7).  The reference takes a sparsity per side (mem_spd_test.py, pred_long_bench.py's K_{k}_V_{v} sweeps); here:

  S = 0.0 (kth 1: every value kept), 0.3, 0.5, 0.9, 0.95, 0.99 (kth 126: ~3 values per token), K and V alike, and
  P = (0.5, 0.8), (0.8, 0.5), (0.0, 0.9), (0.9, 0.0) as (K, V): a K / V mix-up (a kth, a region size) changes what comes out.

At 0.0 / 0.3 a staged chunk reaches into the upper half of its 4 KiB window (the matrix-pipe engine's SKIP path loads it only then);
at 0.9-0.99 most tiles are empty or hold one or two values, chunks are short and whole tile pairs run with no lane active.

  * fused decode, every launch form of tests/test_gpu_groups.FORMS (confirmed by mustafar_last_decode_choice()), GQA-4 on every engine
    the form has plus a group-1 and a group-8 control: every element within exact_data.hook_model's bound over the oracle-pruned K / V;
  * needles (exact_data.needle_data): bit-exact outputs at every point, fused and through the two unfused call sequences;
  * triggers at unequal sparsity: extents under one captured graph with the device-side T, the batched trigger of all layers against
    the layer-by-layer one bit for bit, and the caches in the reference layout against oracle prune + compress, region by region;
  * the device threshold search (select_kth.h as compiled for the GPU) on tests/test_select_kth.py's adversarial rows, through
    prune_magnitude and through the fused prune + compress, K and V at different kth.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import exact_data as xd
from tests.test_gpu_groups import FORMS, RESET
from tests.test_select_kth import _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 32
S = [0.0, 0.3, 0.5, 0.9, 0.95, 0.99]
P = [(0.5, 0.8), (0.8, 0.5), (0.0, 0.9), (0.9, 0.0)]
POINTS = [(s, s) for s in S] + P
PIDS = [f"k{k}-v{v}" for k, v in POINTS]
ENGINES = {"dot2": 2, "valu": 0, "mfma": 1}


def _lib():
    from mustafar_amd import _lib as lib
    return lib.load()


def _attn(hq, hkv, ks, vs, api="fused", **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=hq, num_key_value_heads=hkv, k_sparsity=ks, v_sparsity=vs, api=api, **kw))


def _configs(form):
    """(hq, hkv, engine) of a form: GQA-4 on each engine the form has (the small-launch kernel has no matrix-pipe instantiation: with
    mfma the launch takes the super-block form), then the group-1 and group-8 controls on the default engine."""
    engines = ["dot2", "valu"] + ([] if form == "small" else ["mfma"])
    return [(8, 2, e) for e in engines] + [(8, 8, None), (16, 2, None)]


@pytest.fixture
def form(request):
    structure, knobs, sbit, pform = FORMS[request.param]
    L = _lib()
    for k, v in knobs:
        assert L.mustafar_tune(k, v) == 0
    yield request.param, structure, sbit, pform
    for k, _ in knobs:
        L.mustafar_tune(k, RESET[k])


def _check_choice(name, sbit, pform, hq, hkv, engine):
    c = _lib().mustafar_last_decode_choice()
    assert (c >> 4) & 1 == sbit, f"{name}: structure, choice {c:#x}"
    if pform is not None:
        assert (c >> 8) & 15 == pform, f"{name}: one-pass form, choice {c:#x}"
    if engine is not None and hq // hkv == 4:
        want = ENGINES[engine] if sbit else int(engine == "mfma")    # (two launches report 1 for the matrix pipe, 0 for the vector engines)
        assert c & 15 == want, f"{name} {engine}: engine, choice {c:#x}"


# ---- 1. fused decode against the float64 model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS), indirect=True)
@pytest.mark.parametrize("ks,vs", POINTS, ids=PIDS)
def test_fused_decode_within_the_model_bound(ks, vs, form):
    name, structure, sbit, pform = form
    bsz, D, L0 = 2, 128, 1300                         # 1024 compressed tokens, 276 in the window
    for hq, hkv, engine in _configs(name):
        torch.manual_seed(hq * 31 + hkv + int(ks * 100) * 7 + int(vs * 100))
        attn = _attn(hq, hkv, ks, vs, engine=engine, structure=structure, arena=True)
        K = torch.randn(bsz, hkv, L0, D, device=DEV).half()
        V = torch.randn(bsz, hkv, L0, D, device=DEV).half()
        past = attn.to_fused(attn.build_cache(K.clone(), V.clone()))
        assert past[4] == 1024
        for _ in range(2):
            q, kn, vn = (torch.randn(bsz, h, 1, D, device=DEV).half() for h in (hq, hkv, hkv))
            K, V = torch.cat([K, kn], 2), torch.cat([V, vn], 2)
            out, past = attn.decode(q, kn, vn, past)
            _check_choice(name, sbit, pform, hq, hkv, engine)
            xd.model_ok(out, q, K, V, 1024, hq // hkv, k_sparsity=ks, v_sparsity=vs)


@pytest.mark.parametrize("ks,vs", [(0.5, 0.8), (0.9, 0.9)], ids=["k0.5-v0.8", "k0.9-v0.9"])
def test_fused_decode_at_c3_geometry_within_the_model_bound(ks, vs):
    """32 / 8 heads, 8192 tokens, batch 8 (7936 compressed): the default form at the bench's c3 shape."""
    torch.manual_seed(11)
    bsz, hq, hkv, D, L0 = 8, 32, 8, 128, 8192
    attn = _attn(hq, hkv, ks, vs, arena=True)
    K = torch.randn(bsz, hkv, L0, D, device=DEV).half()
    V = torch.randn(bsz, hkv, L0, D, device=DEV).half()
    past = attn.to_fused(attn.build_cache(K.clone(), V.clone()))
    assert past[4] == 7936
    q, kn, vn = (torch.randn(bsz, h, 1, D, device=DEV).half() for h in (hq, hkv, hkv))
    out, _ = attn.decode(q, kn, vn, past)
    assert (_lib().mustafar_last_decode_choice() >> 4) & 1 == 1, "default form: one pass"
    xd.model_ok(out, q, torch.cat([K, kn], 2), torch.cat([V, vn], 2), 7936, hq // hkv, k_sparsity=ks, v_sparsity=vs)


# ---- 2. needles, bit for bit ---------------------------------------------------------------------------------------------------------
# A needle row holds 8 channels at 16 and every other |k| <= 1, so its slot is kept at any kth (at kth > 120 the threshold IS 16 and
# ties are kept); needle_data checks that on every needle row.  What would not survive -- a secondary needle (8s) on a token that also
# holds a primary needle (16s) of another set -- is not used here: one needle set per call, primary needles only.
def _needle_calls(hq, hkv, bsz, L, seed):
    return xd.assign_rows(xd.edge_positions(1024, L), bsz, hq, np.random.default_rng(seed), L)


@pytest.mark.parametrize("form", list(FORMS), indirect=True)
@pytest.mark.parametrize("ks,vs", POINTS, ids=PIDS)
def test_needles_bit_exact(ks, vs, form):
    name, structure, sbit, pform = form
    bsz, L0 = 2, 1300
    L = L0 + 1
    for hq, hkv, engine in _configs(name):
        for i, pos1 in enumerate(_needle_calls(hq, hkv, bsz, L, hq + hkv)):
            Kn, Vn, qn, _ = xd.needle_data(bsz, hq, hkv, L, pos1, k_sparsity=ks, seed=i, device=DEV)
            a = _attn(hq, hkv, ks, vs, engine=engine, structure=structure, arena=True)
            p = a.to_fused(a.build_cache(Kn[:, :, :L0].contiguous(), Vn[:, :, :L0].contiguous()))
            out, _ = a.decode(qn, Kn[:, :, L0:].contiguous(), Vn[:, :, L0:].contiguous(), p)
            _check_choice(name, sbit, pform, hq, hkv, engine)
            miss = xd.needle_misses(out, xd.needle_expect(Vn, pos1, 1024, vs, hq))
            assert not miss.any(), (f"{hq}x{hkv} {engine}: needle rows wrong {miss.nonzero().tolist()[:8]} "
                                    f"targets {pos1[miss.cpu().numpy()][:8].tolist()}")


@pytest.mark.parametrize("api", ["native", "reference"])
@pytest.mark.parametrize("ks,vs", [(0.5, 0.8), (0.9, 0.0)], ids=["k0.5-v0.8", "k0.9-v0.0"])
def test_needles_bit_exact_through_the_unfused_calls(ks, vs, api):
    bsz, L0 = 2, 1300
    L = L0 + 1
    for hq, hkv in ((8, 2), (8, 8)):
        for i, pos1 in enumerate(_needle_calls(hq, hkv, bsz, L, hq + hkv)):
            Kn, Vn, qn, _ = xd.needle_data(bsz, hq, hkv, L, pos1, k_sparsity=ks, seed=i, device=DEV)
            a = _attn(hq, hkv, ks, vs, api=api)
            out, _ = a.decode(qn, Kn[:, :, L0:].contiguous(), Vn[:, :, L0:].contiguous(),
                              a.build_cache(Kn[:, :, :L0].contiguous(), Vn[:, :, :L0].contiguous()))
            miss = xd.needle_misses(out, xd.needle_expect(Vn, pos1, 1024, vs, hq))
            assert not miss.any(), f"{hq}x{hkv} {api}: needle rows wrong {miss.nonzero().tolist()[:8]}"


# ---- 3. triggers and extents at unequal sparsity -------------------------------------------------------------------------------------
P3 = P + [(0.0, 0.0)]                                 # (0.0, 0.0): every append is the worst case, 128 halfs per token
P3IDS = [f"k{k}-v{v}" for k, v in P3]


def _oracle_streams(x, which, s):
    """oracle prune at s + oracle compress of x [B, Hkv, t, 128] (torch) -> (bmp, idx, streams, nz_offset) numpy."""
    B, H, t, D = x.shape
    xp = orc.prune_magnitude(x.reshape(B * H, t, D).cpu().numpy(), s)
    bmp, idx, nzs = (orc.convert_key_batched if which == "key" else orc.convert_value_batched)(xp)
    return bmp, idx, nzs, orc.nz_offset_from_idx(idx)


def _assert_cache_is_the_oracles(arena, x_all, which, s, what):
    """The arena in the reference layout == oracle prune + compress of its C tokens, byte for byte; and every region of it (base,
    extents) holds exactly its own measured stream lengths, within its capacity."""
    C = arena.total_tokens
    bmp, idx, nzs, off = _oracle_streams(x_all[:, :, :C], which, s)
    got = arena.to_reference()
    assert np.array_equal(got[0].cpu().numpy(), bmp), f"{what} {which}: bitmaps"
    assert np.array_equal(got[1].cpu().numpy(), idx), f"{what} {which}: offsets"
    assert np.array_equal(got[3].cpu().numpy(), off), f"{what} {which}: nz_offset"
    assert np.array_equal(torch.cat(list(got[2])).view(torch.int16).cpu().numpy(), np.concatenate(nzs).view(np.int16)), f"{what} {which}: streams"
    start = 0
    for region in [arena] + list(arena.extents):
        n = region.tokens
        lens = np.array([len(z) for z in _oracle_streams(x_all[:, :, start:start + n], which, s)[2]])
        assert np.array_equal(region.used.cpu().numpy(), lens), f"{what} {which}: region of tokens [{start}, {start + n}) lengths"
        assert region.nz_cap >= lens.max(), f"{what} {which}: region of tokens [{start}, {start + n}) holds more than its capacity"
        start += n
    assert start == C


@pytest.mark.parametrize("ks,vs", P3, ids=P3IDS)
def test_graph_with_device_side_T_through_two_triggers(ks, vs):
    """tests/test_gpu_extents.py's one captured graph across two triggers (an extent each, run eagerly between replays), at unequal
    sparsity: checked steps within the model bound, the caches equal to the oracle's at the end."""
    from mustafar_amd import _lib as lib_mod
    lib = _lib()
    torch.manual_seed(9)
    bsz, hq, hkv, D = 2, 8, 2, 128
    L0 = 512 + R + 250                                 # first trigger at the 6th decode step, the second 256 steps later
    K0, V0 = (torch.randn(bsz, hkv, L0, D, device=DEV).half() for _ in range(2))
    attn = _attn(hq, hkv, ks, vs, arena=True)
    past = attn.to_fused(attn.build_cache(K0.clone(), V0.clone()))
    _assert_cache_is_the_oracles(past[0], K0, "key", ks, "prefill")
    _assert_cache_is_the_oracles(past[2], V0, "value", vs, "prefill")
    C0, cap = past[4], past[4] + 512
    t_dev = torch.tensor([C0], dtype=torch.int32, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    q, k, v = (torch.zeros(bsz, h, 1, D, device=DEV).half() for h in (hq, hkv, hkv))
    attn.decode_fused(q, k, v, (past[0], past[1].clone(), past[2], past[3].clone(), past[4], past[5]), step_counter=counter,
                      t_device=t_dev, t_capacity=cap)                  # scratch for the capacity, outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, _ = attn.decode_fused(q, k, v, past, step_counter=counter, t_device=t_dev, t_capacity=cap)
        lib_mod.check(lib.mustafar_counter_add(torch.cuda.current_stream().cuda_stream, counter.data_ptr(), 1), "counter")
    hk, hv = [K0], [V0]
    state, since, triggers = past, 0, 0
    for step in range(6 + 256 + 8):
        qn, kn, vn = (torch.randn(bsz, h, 1, D, device=DEV).half() for h in (hq, hkv, hkv))
        hk.append(kn); hv.append(vn)
        kv_len = state[5] + since + 1
        if (kv_len - R - state[4]) % 256 == 0 and state[1].len + since + 1 >= 256:   # this step fires the trigger: eagerly
            got, state = attn.decode(qn, kn, vn, attn.advance(state, since))
            since, triggers = 0, triggers + 1
            t_dev.add_(256)
            counter.add_(1 - 256)
            C_step = state[4] - 256
        else:
            q.copy_(qn); k.copy_(kn); v.copy_(vn)
            g.replay()
            got, since, C_step = out, since + 1, state[4]
        if step in (0, 5, 6, 7, 261, 262, 263, 269):
            xd.model_ok(got, qn, torch.cat(hk, 2), torch.cat(hv, 2), C_step, hq // hkv, k_sparsity=ks, v_sparsity=vs)
    assert triggers == 2 and state[4] == C0 + 512 == cap and len(state[0].extents) == 2
    K_all, V_all = torch.cat(hk, 2), torch.cat(hv, 2)
    _assert_cache_is_the_oracles(state[0], K_all, "key", ks, "after two triggers")
    _assert_cache_is_the_oracles(state[2], V_all, "value", vs, "after two triggers")


@pytest.mark.parametrize("extents", [True, False], ids=["extents", "in-place"])
@pytest.mark.parametrize("ks,vs", P3, ids=P3IDS)
def test_batched_trigger_equals_the_layer_by_layer_trigger(ks, vs, extents):
    """tests/test_gpu_extents.py's batched trigger of all layers (run_triggers: one compression launch for every layer's K and V) against
    the trigger decode_fused runs itself, bit for bit, through two triggers at unequal sparsity -- and both against the oracle.  extents=False:
    the layer-by-layer trigger appends in place (append_window_pair) and run_triggers takes the same path."""
    torch.manual_seed(12)
    layers, bsz, hq, hkv, D = 2, 2, 8, 2, 128
    L0, steps = 256 + R + 250, 6 + 256 + 2
    K0 = [torch.randn(bsz, hkv, L0, D, device=DEV).half() for _ in range(layers)]
    V0 = [torch.randn(bsz, hkv, L0, D, device=DEV).half() for _ in range(layers)]
    attn = _attn(hq, hkv, ks, vs, arena=True, extents=extents)
    ref_p = [attn.to_fused(attn.build_cache(K0[l].clone(), V0[l].clone())) for l in range(layers)]
    bat_p = [attn.to_fused(attn.build_cache(K0[l].clone(), V0[l].clone())) for l in range(layers)]
    hk, hv = [[k] for k in K0], [[v] for v in V0]
    fired = 0
    for step in range(steps):
        pool = None
        qkv = [tuple(torch.randn(bsz, h, 1, D, device=DEV).half() for h in (hq, hkv, hkv)) for _ in range(layers)]
        if extents and (bat_p[0][5] + 1 - R - bat_p[0][4]) % 256 == 0 and bat_p[0][1].len + 1 >= 256:   # this step will reach the trigger
            pool = attn.prepare_triggers(bat_p)
            assert pool is not None
        for l in range(layers):
            hk[l].append(qkv[l][1]); hv[l].append(qkv[l][2])
            o_ref, ref_p[l] = attn.decode(*qkv[l], ref_p[l])
            o_bat, bat_p[l] = attn.decode_fused(*qkv[l], bat_p[l], defer_trigger=True)
            assert torch.equal(o_ref, o_bat), f"step {step} layer {l}"
        if attn.trigger_due(bat_p[0]):
            fired += 1
            bat_p = attn.run_triggers(bat_p, pool)
        for l in range(layers):
            assert bat_p[l][4] == ref_p[l][4] and bat_p[l][1].len == ref_p[l][1].len == bat_p[l][3].len
    assert fired == 2
    for l in range(layers):
        assert len(bat_p[l][0].extents) == (2 if extents else 0) and bat_p[l][0].total_tokens == 256 + 512
        for side in (0, 2):
            a, b = bat_p[l][side].to_reference(), ref_p[l][side].to_reference()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3]), f"layer {l} side {side}"
            assert torch.equal(torch.cat(list(a[2])).view(torch.int16), torch.cat(list(b[2])).view(torch.int16)), f"layer {l} side {side}"
        assert torch.equal(bat_p[l][1].view(), ref_p[l][1].view()) and torch.equal(bat_p[l][3].view(), ref_p[l][3].view())
        K_all, V_all = torch.cat(hk[l], 2), torch.cat(hv[l], 2)
        for p, what in ((bat_p[l], "batched"), (ref_p[l], "layer by layer")):
            _assert_cache_is_the_oracles(p[0], K_all, "key", ks, f"{what} layer {l}")
            _assert_cache_is_the_oracles(p[2], V_all, "value", vs, f"{what} layer {l}")


# ---- 5. the device threshold search ------------------------------------------------------------------------------------------------
KTHS = [1, 2, 38, 64, 89, 102, 115, 122, 126, 127, 128]


def _orc_prune_kth(x: np.ndarray, kth: int) -> np.ndarray:
    """The oracle's prune rule at a given kth (orc.prune_magnitude takes a sparsity; kth 128 has none below 1)."""
    x = np.ascontiguousarray(x, np.float16)
    out = np.empty_like(x)
    rc = orc.lib().orc_prune_magnitude(x.ctypes.data, out.ctypes.data, x.size // 128, 128, kth)
    assert rc == 0
    return out


def _rows_padded(n: int, flip: bool) -> np.ndarray:
    x = _rows()
    x = x[::-1] if flip else x
    return np.ascontiguousarray(np.concatenate([x, x[:n - len(x)]]))


@pytest.mark.parametrize("kth", KTHS, ids=[f"kth{k}" for k in KTHS])
def test_device_threshold_search_prune_on_adversarial_rows(kth):
    """prune_magnitude (the SERIAL search of prune_magnitude_kernel) on rows with +-0, subnormals, +-65504, heavy ties and single
    non-zeros, bit for bit against the oracle."""
    from mustafar_amd import _lib as lib_mod, compression
    x = _rows()
    want = _orc_prune_kth(x, kth)
    xg = torch.from_numpy(x).to(DEV)
    if kth < 128:
        s = kth / 128
        assert compression.kth_from_sparsity(s, 128) == kth
        got = compression.prune_magnitude(xg, s).cpu().numpy()
    else:                                              # (no sparsity below 1 asks for kth 128: the C ABI takes kth itself)
        out = torch.empty_like(xg)
        lib_mod.check(_lib().mustafar_prune_magnitude(torch.cuda.current_stream().cuda_stream, xg.data_ptr(), out.data_ptr(), x.shape[0], 128, kth),
                      "mustafar_prune_magnitude")
        got = out.cpu().numpy()
    bad = np.nonzero((got.view(np.uint16) != want.view(np.uint16)).any(1))[0]
    assert not len(bad), f"kth {kth}: {len(bad)} rows pruned differently, rows {bad[:8].tolist()}"


@pytest.mark.parametrize("kth", KTHS, ids=[f"kth{k}" for k in KTHS])
def test_device_threshold_search_compress_on_adversarial_rows(kth):
    """The fused prune + compress of a prefill (CompressedArena.from_raw_pair: compress_block_kernel's search) with K and V at different
    kth, on the same rows (V in reverse order): the caches in the reference layout equal oracle prune + oracle compress byte for byte."""
    from mustafar_amd.cache import CompressedArena
    kth_v = KTHS[(KTHS.index(kth) + 5) % len(KTHS)]
    t, heads = 256, 3
    xk, xv = _rows_padded(heads * t, False), _rows_padded(heads * t, True)
    k, v = CompressedArena.from_raw_pair(torch.from_numpy(xk).to(DEV).view(1, heads, t, 128), torch.from_numpy(xv).to(DEV).view(1, heads, t, 128),
                                         t, kth, kth_v)
    for arena, x, kk, which in ((k, xk, kth, "key"), (v, xv, kth_v, "value")):
        xp = _orc_prune_kth(x, kk).reshape(heads, t, 128)
        bmp, idx, nzs = (orc.convert_key_batched if which == "key" else orc.convert_value_batched)(xp)
        got = arena.to_reference()
        gb = got[0].cpu().numpy()
        bad = np.nonzero((gb != bmp).any(1))[0]
        assert not len(bad), f"{which} kth {kth if which == 'key' else kth_v}: bitmaps differ on heads {bad.tolist()}, " \
                             f"first tile {int(np.argmax(gb[bad[0]] != bmp[bad[0]])) if len(bad) else -1}"
        assert np.array_equal(got[1].cpu().numpy(), idx), f"{which} kth {kk}: offsets"
        assert np.array_equal(got[3].cpu().numpy(), orc.nz_offset_from_idx(idx)), f"{which} kth {kk}: nz_offset"
        lens = [len(z) for z in nzs]
        assert np.array_equal(arena.used.cpu().numpy(), lens), f"{which} kth {kk}: stream lengths"
        flat = torch.cat(list(got[2])).view(torch.int16).cpu().numpy()
        ends = np.cumsum(lens)
        for h in range(heads):
            assert np.array_equal(flat[ends[h] - lens[h]:ends[h]], nzs[h].view(np.int16)), f"{which} kth {kk}: stream of head {h}"
