"""GPU: the head_dim-64 fused decode where a workgroup walks a RUN of several 64-token blocks (the online softmax across blocks, the short
last run, the slab cap), and at the edges the first D = 64 suite left out: sparsities 0.0 .. 0.99 and unequal K / V, the 1024-row window,
k_new = NULL, mask rows per head / per kv head, odd strides, a 2-byte aligned mask base and finite additive masks.

Every multi-block test ASSERTS the run shape it gets (tests/hd64_util.run_shape: compressed slabs S1 and blocks per workgroup bpw, read
off the public workspace size) before it launches: if the launch heuristic changes, the test fails instead of testing one block per
workgroup again.  Comparators: the float64 model's element-wise bound (exact_data.model_ok) on random data, bit equality on needles, the
dense comparator of the first suite for the hook."""
import numpy as np
import pytest
import torch

from oracle.dense_ref import dense_decode_layer
from tests.exact_data import model_ok
from tests.hd64_util import (DEV, D, NEG, RUN_SHAPES, S, Step, _left_pad_mask, _rand, mask_rows, needle_data_64, needle_expect_64,
                             oracle_prune, run_shape)
from tests.util import DENSE_ULPS, excess

pytestmark = pytest.mark.gpu

SPARSITIES = [(0.0, 0.0), (0.3, 0.3), (0.5, 0.5), (0.9, 0.9), (0.99, 0.99), (0.5, 0.8), (0.8, 0.5), (0.0, 0.9), (0.9, 0.0)]


@pytest.fixture(scope="module")
def pkg():
    from mustafar_amd import _lib, compression
    return _lib.load(), compression


def _split(Bp, groups):
    """B' = 64 as batch 8 x 8 kv heads (even group counts) or 32 x 2 (odd ones); B' = 1 as 1 x 1."""
    return (1, 1) if Bp == 1 else ((8, 8) if groups % 2 == 0 else (32, 2))


def _require(pkg, name, B, Hkv, groups):
    """The run shape of RUN_SHAPES[name], asserted from the library's own workspace size (a precondition, not a skip)."""
    Bp, T, bpw, S1, last = RUN_SHAPES[name]
    assert B * Hkv == Bp
    got = run_shape(pkg[0], T, Bp * groups, groups)
    assert got == (S1, bpw), f"{name}: the launch would take (S1, bpw) = {got}, this test needs {(S1, bpw)}"
    assert T // 64 - (S1 - 1) * bpw == last
    return T, bpw


def _run_pads(B, T, bpw, wl):
    """Left pads that end INSIDE a run: not a multiple of 64 bpw, one behind whole masked runs, one inside the window."""
    run = 64 * bpw
    if B == 1:
        return [2 * run + 44]
    base = [0, run // 2 + 5, 2 * run + 44, T + min(10, wl - 2), 63, run - 1, T - 1, (T // run // 2) * run + 70]
    return [base[b % len(base)] for b in range(B)]


# ---- 2. multi-block runs against the model ---------------------------------------------------------------------------------------------
def _model_case(pkg, name, groups, wl, seed, cap=None, ks=S, vs=S):
    B, Hkv = _split(RUN_SHAPES[name][0], groups)
    T, bpw = _require(pkg, name, B, Hkv, groups)
    K, V, q = _rand(B, Hkv, T + wl, groups, seed=seed)
    st = Step(pkg, K, V, T, groups, cap=cap, ks=ks, vs=vs)
    pr = (st.Kp, st.Vp)
    model_ok(st.call(q), q, K, V, T, groups, k_sparsity=ks, v_sparsity=vs, pruned=pr)
    pads = _run_pads(B, T, bpw, wl)
    st.mask = _left_pad_mask(B, T + wl, pads)
    st.mask_stride = T + wl
    model_ok(st.call(q), q, K, V, T, groups, pads=pads, k_sparsity=ks, v_sparsity=vs, pruned=pr)
    return st


@pytest.mark.parametrize("groups", [1, 2, 3, 4, 5, 6, 7, 8])
def test_runs_of_two_blocks_with_a_short_last_run(pkg, groups):
    _model_case(pkg, "bpw2", groups, wl=40, seed=100 + groups)


@pytest.mark.parametrize("name,groups", [("bpw2_full", 4), ("bpw3", 4), ("bpw3", 8), ("bpw8", 4)])
def test_runs_at_the_bench_shapes(pkg, name, groups):
    _model_case(pkg, name, groups, wl=70, seed=200 + groups)


@pytest.mark.parametrize("groups", [1, 4])
@pytest.mark.parametrize("name", ["cap", "cap+1", "64k"])
def test_runs_at_the_slab_cap(pkg, name, groups):
    # the slab limit itself comes with a full 1024-row window: 1008 + 16 = 1024 slabs for the row merge
    wl, cap = (1024, 1024) if name == "cap" else (33, None)
    st = _model_case(pkg, name, groups, wl=wl, seed=300 + groups, cap=cap)
    if name == "cap":
        assert st.ws.numel() == 1024 * st.BH * 66 * 4


def test_runs_graph_replay_with_alternating_queries(pkg):
    L_, _ = pkg
    groups, w0, steps = 4, 60, 8
    B, Hkv = _split(64, groups)
    C, bpw = _require(pkg, "bpw2", B, Hkv, groups)
    K, V, q = _rand(B, Hkv, C + w0 + steps, groups, seed=31)
    pads = _run_pads(B, C, bpw, w0)
    mask = _left_pad_mask(B, C + 128, pads)
    extra = torch.zeros((1,), dtype=torch.int32, device=DEV)
    st = Step(pkg, K[:, :, :C + w0], V[:, :, :C + w0], C, groups, cap=128, mask=mask, extra=extra)
    qs = torch.empty_like(q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        st.call(qs)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.call(qs)
    for i in range(steps):
        n = C + w0 + i
        st.kn.copy_(K[:, :, n - 1])
        st.vn.copy_(V[:, :, n - 1])
        qs.copy_(q.flip(1) if i % 2 else q)
        graph.replay()
        torch.cuda.synchronize()
        model_ok(st.out, qs, K[:, :, :n], V[:, :, :n], C, groups, pads=pads, pruned=(st.Kp, st.Vp))
        assert L_.mustafar_counter_add(torch.cuda.current_stream().cuda_stream, extra.data_ptr(), 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(st.kw[:, :, :w0 + steps - 1], K[:, :, C:C + w0 + steps - 1])


# ---- 3. needles through runs, bit for bit ----------------------------------------------------------------------------------------------
def _run_positions(T, bpw, n):
    """Needle positions of a head of T compressed tokens in runs of bpw blocks, n tokens in all: the first and last token of the first, a
    middle and the last block of the first, a middle and the last full run and of the short (or last) run; T - 1, T, n - 2, n - 1."""
    ntb, pos = T // 64, {T - 1, T, n - 2, n - 1}
    runs = -(-ntb // bpw)
    for r in {0, runs // 2, runs - 2, runs - 1}:
        b0, b1 = r * bpw, min(ntb, r * bpw + bpw)
        for blk in {b0, (b0 + b1 - 1) // 2, b1 - 1}:
            pos.update((blk * 64, blk * 64 + 63))
    return sorted(pos)


def _misses(out, want):
    return (out.float() != want.float()).any(-1).nonzero().tolist()


@pytest.mark.parametrize("name", ["bpw2", "bpw3", "bpw8"])
def test_needles_through_runs(pkg, name):
    groups, wl = 4, 70
    B, Hkv = _split(64, groups)
    T, bpw = _require(pkg, name, B, Hkv, groups)
    n, Hq = T + wl, Hkv * groups
    rng = np.random.default_rng(bpw)
    edges = _run_positions(T, bpw, n)
    assert len(edges) <= B * Hq
    pos = np.concatenate([edges, rng.integers(0, n, B * Hq - len(edges))]).reshape(B, Hq)
    K, V, q = needle_data_64(B, Hq, Hkv, n, pos, seed=bpw)
    out = Step(pkg, K, V, T, groups).call(q)
    assert not _misses(out, needle_expect_64(V, pos, T, groups)), "rows miss their needle"


@pytest.mark.parametrize("name", ["bpw2", "bpw3", "bpw8"])
def test_equal_needles_through_runs(pkg, name):
    """2 and 4 tokens of equal score: in two blocks of one run (alpha == 1), in two runs (slab merge), compressed + window; the mean of
    their (pruned) V rows exactly."""
    groups, wl = 4, 70
    B, Hkv = _split(64, groups)
    T, bpw = _require(pkg, name, B, Hkv, groups)
    n, Hq, run = T + wl, Hkv * groups, 64 * bpw
    last = (T // run) * run if T % run else T - run           # first token of the last (short) run
    pairs = [(5 * run + 3, 5 * run + 64 + 60), (0, run - 1), (2 * run + 63, 7 * run), (last, 64), (last + 1, run + 64), (T - 1, T),
             (run + 7, n - 1), (last + 63, n - 2)]
    quads = [(3 * run, 3 * run + 127, 9 * run + 5, T + 3), (0, 65, last, n - 1), (run - 1, run, T - 1, T), (4 * run + 1, 4 * run + 64, 4 * run + 2, 4 * run + 65)]
    for k, sets in ((2, pairs), (4, quads)):
        rng = np.random.default_rng(k)
        rows = [sets[i % len(sets)] if i < 2 * len(sets) else tuple(rng.choice(n, k, replace=False)) for i in range(B * Hq)]
        pos = np.asarray(rows, np.int64).reshape(B, Hq, k)
        K, V, q = needle_data_64(B, Hq, Hkv, n, pos, seed=10 * bpw + k)
        out = Step(pkg, K, V, T, groups).call(q)
        assert not _misses(out, needle_expect_64(V, pos, T, groups)), f"{k} equal needles"


def test_masked_needle_through_runs(pkg):
    """One mask row per q head removes that head's higher needle: the lower one, in another block, run or the window, must win."""
    groups, wl = 4, 70
    B, Hkv = _split(64, groups)
    T, bpw = _require(pkg, "bpw2", B, Hkv, groups)
    n, Hq = T + wl, Hkv * groups
    rng = np.random.default_rng(7)
    pos = rng.integers(0, n, (B, Hq))
    pos2 = (pos + rng.integers(1, n, (B, Hq))) % n
    pos[0, :6] = [128, 128 + 64, 300, T - 1, T + 5, n - 1]     # (first block of a run, second block, ..., window, new row)
    pos2[0, :6] = [128 + 64, 128, T + 9, 301, 7999 - 64, 0]
    K, V, q = needle_data_64(B, Hq, Hkv, n, pos, seed=8, pos2=pos2)
    mask = mask_rows(B * Hq, n)
    masked = np.zeros((B, Hq, n), bool)
    for b in range(B):
        for h in range(Hq):
            mask[b * Hq + h, pos[b, h]] = NEG
            masked[b, h, pos[b, h]] = True
    out = Step(pkg, K, V, T, groups, mask=mask, mask_heads=1).call(q)
    assert not _misses(out, needle_expect_64(V, pos, T, groups, pos2=pos2, masked=masked))


# ---- 4. sparsity -----------------------------------------------------------------------------------------------------------------------
def _block_halfs(idx):
    """Halfs of every 64-token block's stream, from the idx array [B', T + 1] (half2 units)."""
    i = idx.cpu().numpy().astype(np.int64)
    return 2 * (i[:, 64::64] - i[:, :-1:64])


@pytest.mark.parametrize("shape", ["one_block", "bpw2"])
@pytest.mark.parametrize("ks,vs", SPARSITIES)
def test_sparsity_model_and_needles(pkg, shape, ks, vs):
    groups, wl = 4, 70
    if shape == "bpw2":
        B, Hkv = _split(64, groups)
        T, _ = _require(pkg, "bpw2", B, Hkv, groups)
    else:
        B, Hkv, T = 2, 2, 1024
        assert run_shape(pkg[0], T, B * Hkv * groups, groups) == (16, 1)
    n, Hq = T + wl, Hkv * groups
    K, V, q = _rand(B, Hkv, n, groups, seed=int(100 * ks + 10 * vs) + len(shape))
    st = Step(pkg, K, V, T, groups, ks=ks, vs=vs)
    for side, sp, c in (("K", ks, st.kc), ("V", vs, st.vc)):
        halfs = _block_halfs(c[1])
        if sp == 0.0:   # nothing pruned: a block's stream is the whole 8 KiB of the staging buffer, offsets up to 4095, all eight copy trips
            assert (halfs == 4096).any(), f"{side}: no block fills the staging buffer"
        assert halfs.max() <= 4096
    model_ok(st.call(q), q, K, V, T, groups, k_sparsity=ks, v_sparsity=vs, pruned=(st.Kp, st.Vp))
    rng = np.random.default_rng(3)
    edges = [0, 63, 64, 127, 128, T - 65, T - 64, T - 1, T, n - 2, n - 1]
    pos = np.concatenate([edges, rng.integers(0, n, B * Hq - len(edges))]).reshape(B, Hq)
    K, V, q = needle_data_64(B, Hq, Hkv, n, pos, seed=5)
    out = Step(pkg, K, V, T, groups, ks=ks, vs=vs).call(q)
    assert not _misses(out, needle_expect_64(V, pos, T, groups, vs=vs))


@pytest.mark.parametrize("shape", ["one_block", "bpw2"])
def test_adversarial_tiles(pkg, shape):
    """SURVEY 8d at D = 64: a block of exact zeros in K, in V, in both (a whole run of them too), -0.0 entries, and a block whose kept
    values all sit in one 32-channel half."""
    groups, wl = 4, 50
    if shape == "bpw2":
        B, Hkv = _split(64, groups)
        T, _ = _require(pkg, "bpw2", B, Hkv, groups)
    else:
        B, Hkv, T = 2, 2, 1024
        assert run_shape(pkg[0], T, B * Hkv * groups, groups) == (16, 1)
    blk = lambda i: slice(64 * i, 64 * i + 64)
    K, V, q = _rand(B, Hkv, T + wl, groups, seed=41)
    K[:, :, blk(2)] = 0
    V[:, :, blk(3)] = 0
    K[:, :, 64 * 4:64 * 6] = 0                       # blocks 4 and 5: both sides, one whole run at two blocks per workgroup
    V[:, :, 64 * 4:64 * 6] = 0
    K[:, :, 64 * 7:64 * 7 + 64:3, ::5] = -0.0
    V[:, :, 64 * 7 + 1:64 * 7 + 64:3, 1::5] = -0.0
    K[:, :, blk(9), 32:] *= 1e-3                     # every kept value in channels 0..31
    V[:, :, blk(9), :32] *= 1e-3                     # ... and in channels 32..63
    K[:, :, blk(0)] = 0                              # the first block of a head: its stream starts where the head's does
    st = Step(pkg, K, V, T, groups)
    ki, vi = st.kc[1].cpu().numpy(), st.vc[1].cpu().numpy()
    assert (ki[:, 128] == ki[:, 192]).all() and (vi[:, 192] == vi[:, 256]).all() and (ki[:, 256] == ki[:, 384]).all()
    assert (ki[:, 0] == ki[:, 64]).all() and (vi[:, 256] == vi[:, 384]).all()
    kb = st.kc[0].cpu().numpy().view(np.uint64)[:, blk(9)]
    assert (kb[:, 32:] == 0).all() and (kb[:, :32] != 0).any(), "the key block's upper channel tiles are not empty"
    vb = st.vc[0].cpu().numpy().view(np.uint64)[:, blk(9)]
    assert (vb >> np.uint64(32) == 0).all(), "the value block's tiles hold channels below 32"
    model_ok(st.call(q), q, K, V, T, groups, pruned=(st.Kp, st.Vp))


def test_hook_end_to_end_unequal_sparsity_batch_2_masked(pkg):
    """k_sparsity 0.5, v_sparsity 0.8 through two triggers of the tuple cache at Llama-3.2-1B heads, batch 2, one entry left-padded."""
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    Hq, Hkv, B, prefill, steps, ks, vs = 32, 8, 2, 1000, 330, 0.5, 0.8
    attn = MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, api="fused", residual_length=32,
                                            k_sparsity=ks, v_sparsity=vs))
    g = torch.Generator(device=DEV).manual_seed(2)
    n_all = prefill + steps
    K = torch.randn((B, Hkv, n_all, D), generator=g, device=DEV).half()
    V = torch.randn((B, Hkv, n_all, D), generator=g, device=DEV).half()
    Kpr, Vpr = oracle_prune(K, ks), oracle_prune(V, vs)
    pads = [0, 150]
    full = _left_pad_mask(B, n_all, pads)
    past = attn.build_cache(K[:, :, :prefill], V[:, :, :prefill])
    assert past[4] == 768
    triggers = 0
    for i in range(steps):
        n = prefill + i + 1
        C = past[4]
        q = torch.randn((B, Hq, 1, D), generator=g, device=DEV).half()
        out, past = attn.decode(q, K[:, :, n - 1:n], V[:, :, n - 1:n], past, attention_mask=full[..., :n].contiguous())
        triggers += past[4] != C
        Kd = torch.cat([Kpr[:, :, :C], K[:, :, C:n]], 2)
        Vd = torch.cat([Vpr[:, :, :C], V[:, :, C:n]], 2)
        for b in range(B):
            want = dense_decode_layer(q[b:b + 1], Kd[b:b + 1, :, pads[b]:], Vd[b:b + 1, :, pads[b]:], Hq // Hkv)
            e = excess(out[b:b + 1], want, DENSE_ULPS)
            assert e <= 1.0, f"step {i} entry {b} (kv {n}, compressed {C}): {e:.2f} x the bound"
    assert triggers >= 2 and past[4] == 768 + 256 * triggers


# ---- 5. window and operands ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wl", [1, 64, 65, 1023, 1024])
@pytest.mark.parametrize("T", [0, 64512])
def test_window_of_1024_rows(pkg, T, wl):
    groups = 4
    B, Hkv = (2, 2) if T == 0 else (1, 1)
    if T:
        _require(pkg, "cap", B, Hkv, groups)
    K, V, q = _rand(B, Hkv, T + wl, groups, seed=T + wl)
    st = Step(pkg, K, V, T, groups, cap=1024)
    model_ok(st.call(q), q, K, V, T, groups, pruned=(st.Kp, st.Vp))
    assert torch.equal(st.kw[:, :, :wl], K[:, :, T:]) and torch.equal(st.vw[:, :, :wl], V[:, :, T:])
    assert not st.kw[:, :, wl:].any() and not st.vw[:, :, wl:].any()


@pytest.mark.parametrize("cap", [192, 256])
def test_graph_replay_grows_the_window_to_its_capacity(pkg, cap):
    L_, _ = pkg
    B, Hkv, groups, C, w0 = 2, 2, 4, 1024, 60
    steps = cap - w0 + 1                                       # the last step: window_len + extra == capacity
    n_all = C + w0 + steps - 1
    K, V, q = _rand(B, Hkv, n_all, groups, seed=cap)
    pads = [0, 300]
    mask = _left_pad_mask(B, C + cap, pads)
    extra = torch.zeros((1,), dtype=torch.int32, device=DEV)
    st = Step(pkg, K[:, :, :C + w0], V[:, :, :C + w0], C, groups, cap=cap, mask=mask, extra=extra)
    qs = torch.empty_like(q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        st.call(qs)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.call(qs)
    for i in range(steps):
        n = C + w0 + i
        st.kn.copy_(K[:, :, n - 1])
        st.vn.copy_(V[:, :, n - 1])
        qs.copy_(q * (1 + i % 3))
        graph.replay()
        torch.cuda.synchronize()
        model_ok(st.out, qs, K[:, :, :n], V[:, :, :n], C, groups, pads=pads, pruned=(st.Kp, st.Vp))
        if i < steps - 1:                                      # never beyond the capacity
            assert L_.mustafar_counter_add(torch.cuda.current_stream().cuda_stream, extra.data_ptr(), 1) == 0
    torch.cuda.synchronize()
    assert n == C + cap and int(extra.item()) + w0 == cap
    assert torch.equal(st.kw, K[:, :, C:]) and torch.equal(st.vw, V[:, :, C:])


@pytest.mark.parametrize("C,wl", [(0, 1), (640, 65), (640, 128)])
def test_newest_row_already_stored(pkg, C, wl):
    """k_new = v_new = NULL: the same bits as the call that passes the rows, and the windows are left as they were."""
    B, Hkv, groups = 3, 2, 4
    K, V, q = _rand(B, Hkv, C + wl, groups, seed=wl)
    a = Step(pkg, K, V, C, groups)
    b = Step(pkg, K, V, C, groups, stored_new=True)
    kw0, vw0 = b.kw.clone(), b.vw.clone()
    oa, ob = a.call(q), b.call(q)
    torch.cuda.synchronize()
    assert torch.equal(oa.view(torch.int16), ob.view(torch.int16))
    assert torch.equal(b.kw, kw0) and torch.equal(b.vw, vw0) and torch.equal(a.kw, kw0) and torch.equal(a.vw, vw0)


# ---- 6. mask geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one_block", "bpw2"])
@pytest.mark.parametrize("groups,mask_heads", [(4, 1), (4, 4), (4, 0), (8, 2), (8, 1), (1, 1), (3, 1)])
def test_mask_rows_per_head_with_odd_stride_and_unaligned_base(pkg, shape, groups, mask_heads):
    """One mask row per `mask_heads` consecutive q heads (0: per batch entry), every row with a pad of its own, rows an odd number of
    halfs apart and the base 2-byte aligned only."""
    wl = 90
    if shape == "bpw2":
        B, Hkv = _split(64, groups)
        T, bpw = _require(pkg, "bpw2", B, Hkv, groups)
    else:
        B, Hkv, T, bpw = 3, 2, 640, 1
        assert run_shape(pkg[0], T, B * Hkv * groups, groups) == (10, 1)
    n, Hq = T + wl, Hkv * groups
    mh = mask_heads or Hq
    rows = B * Hq // mh
    stride = n + 1 if n % 2 == 0 else n + 2
    rng = np.random.default_rng(groups + mh)
    fixed = _run_pads(8, T, bpw, wl)
    row_pads = [fixed[r] if r < 8 else int(rng.integers(0, n - 1)) for r in range(rows)]
    mask = mask_rows(rows, n, stride=stride, offset=1)
    assert mask.data_ptr() % 4 == 2 and stride % 2 == 1
    for r, p in enumerate(row_pads):
        mask[r, :p] = NEG
    K, V, q = _rand(B, Hkv, n, groups, seed=17 + mh)
    st = Step(pkg, K, V, T, groups, mask=mask, mask_stride=stride, mask_heads=mh)
    pads = [[row_pads[(b * Hq + h) // mh] for h in range(Hq)] for b in range(B)]
    model_ok(st.call(q), q, K, V, T, groups, pads=pads, pruned=(st.Kp, st.Vp))


@pytest.mark.parametrize("shape", ["one_block", "bpw2"])
@pytest.mark.parametrize("mask_heads", [1, 0])
def test_finite_additive_mask(pkg, shape, mask_heads):
    groups, wl = 4, 90
    if shape == "bpw2":
        B, Hkv = _split(64, groups)
        T, _ = _require(pkg, "bpw2", B, Hkv, groups)
    else:
        B, Hkv, T = 3, 2, 640
    n, Hq = T + wl, Hkv * groups
    mh = mask_heads or Hq
    rows = B * Hq // mh
    mask = mask_rows(rows, n, stride=n + 3, offset=1)
    g = torch.Generator(device=DEV).manual_seed(5)
    mask.copy_(-4 * torch.rand((rows, n), generator=g, device=DEV))
    mask[0, :7] = NEG                                          # a few removed columns among the finite ones
    K, V, q = _rand(B, Hkv, n, groups, seed=23 + mh)
    st = Step(pkg, K, V, T, groups, mask=mask, mask_stride=n + 3, mask_heads=mh)
    m4 = mask.reshape(B, Hq // mh, 1, n).repeat_interleave(mh, 1)
    model_ok(st.call(q), q, K, V, T, groups, mask=m4, pruned=(st.Kp, st.Vp))


def test_finite_additive_mask_head_dim_128(pkg):
    """The model's mask argument is shared with D = 128: one case through mustafar_decode_attention_hd's forwarding."""
    L_, _ = pkg
    B, Hkv, groups, C, wl, Dd = 2, 2, 4, 512, 40, 128
    g = torch.Generator(device=DEV).manual_seed(9)
    K = torch.randn((B, Hkv, C + wl, Dd), generator=g, device=DEV).half()
    V = torch.randn((B, Hkv, C + wl, Dd), generator=g, device=DEV).half()
    q = torch.randn((B, Hkv * groups, 1, Dd), generator=g, device=DEV).half()
    mask = (-4 * torch.rand((B, 1, 1, C + wl), generator=g, device=DEV)).half()
    st = Step(pkg, K, V, C, groups, mask=mask)
    model_ok(st.call(q, head_dim=128), q, K, V, C, groups, mask=mask, pruned=(st.Kp, st.Vp))
    assert (L_.mustafar_last_decode_choice() >> 8) != 5
