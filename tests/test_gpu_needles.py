"""GPU: bit-exact peaked attention at the bench shapes (tests/exact_data.py).  Every (batch, head) row attends to one needle token of
its own, so one call checks hundreds of positions: token 0, the first and last token of every block (64 tokens at c3 / m8 / 64x8,
256 at c4 and 28x4), T - 1 and T, the last window row and the step's new row.  Steps that differ only in q move the needles (up to
16 / groups needle sets on disjoint channel slots).  The output of a row is its needle's V row exactly -- on every engine and launch
form, and through the two unfused call sequences -- so `torch.equal` holds where the dense comparators allow ~1e-4.
The finite-gap ("attention sink") variant is held to the float64 model of exact_data.hook_model and its bound."""
import numpy as np
import pytest
import torch

from tests import exact_data as xd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {  # (Hq, Hkv, sparsity, L, batch, block of the edge list)
    "c3": (32, 8, 0.7, 8192, 8, 64),
    "c4": (32, 8, 0.8, 32768, 4, 256),
    "m8": (32, 32, 0.7, 8192, 8, 64),
    "l70": (64, 8, 0.7, 8192, 2, 64),       # Llama-3-70B's heads: group count 8, two workgroup rows per kv head
    "q7": (28, 4, 0.7, 4096, 2, 256),       # Qwen2.5-7B's heads: group count 7 (G = 1 x 7)
}


def _lib():
    from mustafar_amd import _lib as lib
    return lib.load()


def _attn(name, api="fused", **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    Hq, Hkv, s = SHAPES[name][:3] if isinstance(name, str) else name
    return MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, k_sparsity=s, v_sparsity=s, api=api, **kw))


class Case:
    """One needle cache at a bench shape: K / V of L tokens (+ the step's new row), the query sets and what each must give."""

    def __init__(self, name, seed=0):
        Hq, Hkv, s, L, B, block = SHAPES[name]
        self.name, self.Hq, self.Hkv, self.s, self.L, self.B = name, Hq, Hkv, s, L, B
        self.C = ((L - 32) // 256) * 256
        rng = np.random.default_rng(seed)
        sets = xd.assign_rows(xd.edge_positions(self.C, L + 1, block), B, Hq, rng, L + 1)
        assert len(sets) * (Hq // Hkv) <= xd.D // xd.SLOT, f"{name}: {len(sets)} needle sets do not fit the slots"
        self.K, self.V, q, q_alt = xd.needle_data(B, Hq, Hkv, L + 1, sets[0], alt=sets[1:], k_sparsity=s, seed=seed, device=DEV)
        self.queries = [q] + q_alt
        self.wants = [xd.needle_expect(self.V, p, self.C, s, Hq) for p in sets]
        self.sets = sets
        self.kn, self.vn = self.K[:, :, L:].contiguous(), self.V[:, :, L:].contiguous()
        attn = _attn(name, arena=True)
        self.past = attn.to_fused(attn.build_cache(self.K[:, :, :L].contiguous(), self.V[:, :, :L].contiguous()))
        assert self.past[4] == self.C

    def fork(self):
        p = self.past
        return (p[0], p[1].clone(), p[2], p[3].clone(), p[4], p[5])

    def reference_past(self):
        p = self.past
        return (p[0].to_reference(), p[1].view().clone(), p[2].to_reference(), p[3].view().clone(), p[4], p[5])

    def check(self, run, what):
        for i, (q, want) in enumerate(zip(self.queries, self.wants)):
            out = run(q)
            miss = xd.needle_misses(out, want)
            assert not miss.any(), (f"{self.name} {what} set {i}: {int(miss.sum())} rows wrong, e.g. (b, h) {miss.nonzero().tolist()[:6]} "
                                    f"targets {self.sets[i][miss.cpu().numpy()][:6].tolist()}")


_CASES = {}


@pytest.fixture(scope="module")
def cases():
    yield _CASES
    _CASES.clear()
    torch.cuda.empty_cache()


def _case(cases, name):
    if name not in cases:
        cases.clear()                 # one bench-shape cache alive at a time
        torch.cuda.empty_cache()
        cases[name] = Case(name)
    return cases[name]


# (MustafarConfig kwargs, mustafar_tune knobs, expected structure bit, expected engine code or None)
FORMS = {
    "default": ({}, (), 1, None),
    "two_launch": ({"structure": "two_launch"}, (), 0, None),
    "pair": ({"structure": "one_pass"}, ((8, 0),), 1, None),
    "small": ({"structure": "one_pass"}, ((11, 2),), 1, None),
    "dot2": ({"engine": "dot2", "structure": "one_pass"}, (), 1, 2),
    "valu": ({"engine": "valu", "structure": "one_pass"}, (), 1, 0),
    "mfma": ({"engine": "mfma", "structure": "one_pass"}, (), 1, 1),
}
RESET = {8: 1, 11: 1}


# the engine choice applies where G = 4 (group counts that are multiples of 4); G < 4 runs v_fma_mix whatever is asked
@pytest.mark.parametrize("name,form", [(n, f) for n in SHAPES for f in FORMS
                                       if FORMS[f][3] is None or (SHAPES[n][0] // SHAPES[n][1]) % 4 == 0])
def test_needles_are_bit_exact_at_size(cases, name, form):
    kw, knobs, sbit, eng = FORMS[form]
    c = _case(cases, name)
    L = _lib()
    attn = _attn(name, arena=True, **kw)
    try:
        for k, v in knobs:
            assert L.mustafar_tune(k, v) == 0

        def run(q):
            out, _ = attn.decode(q, c.kn, c.vn, c.fork())
            choice = L.mustafar_last_decode_choice()
            assert (choice >> 4) & 1 == sbit and (eng is None or choice & 15 == eng), f"{form}: choice {choice:#x}"
            if form == "pair":
                assert (choice >> 8) & 15 == 2, f"pair form: choice {choice:#x}"
            return out
        c.check(run, form)
    finally:
        for k, _ in knobs:
            L.mustafar_tune(k, RESET[k])


@pytest.mark.parametrize("api", ["native", "reference"])
@pytest.mark.parametrize("name", ["c3", "m8", "l70"])
def test_needles_are_bit_exact_through_the_unfused_call_sequences(cases, name, api):
    """Their fp32 softmax gives p = 1.0 and exact zeros: the two entry points and the PyTorch glue must be exact too."""
    c = _case(cases, name)
    attn = _attn(name, api=api)
    c.check(lambda q: attn.decode(q, c.kn, c.vn, c.reference_past())[0], api)


def test_two_equal_needles_give_their_exact_mean():
    """Two needles of equal score in different slabs (and one in the compressed part with one in the window): exactly fp16((v1 + v2) / 2)."""
    Hq, Hkv, s, L, B, _ = SHAPES["c3"]
    C = ((L - 32) // 256) * 256
    rng = np.random.default_rng(11)
    pos1 = np.stack([rng.integers(0, C // 2, (B, Hq)), rng.integers(C // 2, L + 1, (B, Hq))], -1)     # far apart: different slabs
    pos1[:, :8, 1] = rng.integers(C, L + 1, (B, 8))                                                     # the second one in the window
    pos1[0, 0] = (C - 1, C)
    K, V, q, _ = xd.needle_data(B, Hq, Hkv, L + 1, pos1, k_sparsity=s, seed=11, device=DEV)
    want = xd.needle_expect(V, pos1, C, s, Hq)
    for kw in ({}, {"structure": "two_launch"}, {"engine": "mfma"}, {"engine": "valu"}):
        attn = _attn("c3", arena=True, **kw)
        out, _ = attn.decode(q, K[:, :, L:].contiguous(), V[:, :, L:].contiguous(),
                             attn.to_fused(attn.build_cache(K[:, :, :L].contiguous(), V[:, :, :L].contiguous())))
        assert not xd.needle_misses(out, want).any(), kw


@pytest.mark.parametrize("structure", ["one_pass", "two_launch"])
def test_a_masked_needle_moves_the_output_to_the_second_one(structure):
    """A needle column masked with finfo.min: the output becomes the second-best needle's row, exactly."""
    from tests.test_gpu_mask import _left_padding_mask
    Hq, Hkv, s, L, B, _ = SHAPES["c3"]
    C = ((L - 32) // 256) * 256
    rng = np.random.default_rng(12)
    pos1 = rng.integers(0, L + 1, (B, Hq))
    pads = [0, 1, 64, 1000, 4096, 7936, 7937, 8000]
    pos1[:, 0] = np.maximum(np.array(pads) - 1, 0)                 # the last masked column (batch 0: nothing masked)
    pos2 = rng.integers(8000, L + 1, (B, Hq))
    pos2[pos2 == pos1] = -1
    K, V, q, _ = xd.needle_data(B, Hq, Hkv, L + 1, pos1, pos2, k_sparsity=s, seed=12, device=DEV)
    mask = _left_padding_mask(B, L + 1, pads)
    masked = (mask[:, 0, 0] < 0).cpu().numpy()
    want = xd.needle_expect(V, pos1, C, s, Hq, pos2=pos2, masked=masked)
    attn = _attn("c3", arena=True, structure=structure)
    out, _ = attn.decode(q, K[:, :, L:].contiguous(), V[:, :, L:].contiguous(),
                         attn.to_fused(attn.build_cache(K[:, :, :L].contiguous(), V[:, :, :L].contiguous())), attention_mask=mask)
    assert not xd.needle_misses(out, want).any()
    assert masked[1:, 0].all() and not masked[0].any()


def test_needles_under_graph_replay_with_q_moving_them(cases):
    from mustafar_amd import _lib as lib_mod
    L = _lib()
    c = _case(cases, "c3")
    attn = _attn("c3", arena=True)
    q = torch.zeros_like(c.queries[0])
    kn, vn = torch.zeros_like(c.kn), torch.zeros_like(c.vn)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    past = c.fork()
    attn.decode_fused(q, kn, vn, c.fork())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, _ = attn.decode_fused(q, kn, vn, past, step_counter=counter)
        lib_mod.check(L.mustafar_counter_add(torch.cuda.current_stream().cuda_stream, counter.data_ptr(), 1), "counter")
    kn.copy_(c.kn); vn.copy_(c.vn)
    for r in range(2 * len(c.queries)):
        i = r % len(c.queries)
        if r == 1:      # the first replay's new row (a needle of set 0) stays in the window; later new rows are zeros (score 0)
            kn.zero_(); vn.zero_()
        q.copy_(c.queries[i])
        g.replay()
        assert not xd.needle_misses(out, c.wants[i]).any(), f"replay {r}, needle set {i}"
    assert int(counter.item()) == 2 * len(c.queries)


def test_one_zeroed_value_token_fails_exactly_its_needle_rows(cases):
    """NEGATIVE CONTROL: one token's kept values zeroed in the value stream of the compressed cache (both 64-channel value tiles of
    the token, in one kv head).  The rows that target that token must fail, every other row stays bit-exact."""
    c = _case(cases, "c3")
    attn = _attn("c3", arena=True)
    pos = c.sets[0]
    g = c.Hq // c.Hkv
    b, h = (int(x) for x in np.argwhere(pos < c.C)[len(np.argwhere(pos < c.C)) // 2])     # a row whose needle is a compressed token
    t = int(pos[b, h])
    kv = h // g
    vc = c.past[2]
    head = b * c.Hkv + kv
    tb, r = divmod(t, 64)
    spans = []
    for col in range(2):
        tile = tb * 128 + col * 64 + r
        lo, hi = 2 * int(vc.idx[head, tile]), 2 * int(vc.idx[head, tile + 1])
        spans.append((lo, hi, vc.nz[head, lo:hi].clone()))
    assert sum(int(x[2].ne(0).sum()) for x in spans) > 0, "the token keeps no value"
    want = c.wants[0]
    ok = attn.decode(c.queries[0], c.kn, c.vn, c.fork())[0]
    assert not xd.needle_misses(ok, want).any()
    try:
        for lo, hi, _ in spans:
            vc.nz[head, lo:hi] = 0
        bad = attn.decode(c.queries[0], c.kn, c.vn, c.fork())[0]
    finally:
        for lo, hi, saved in spans:
            vc.nz[head, lo:hi] = saved
    miss = xd.needle_misses(bad, want).cpu().numpy()
    hit = np.zeros_like(miss)
    hit[b, kv * g:(kv + 1) * g] = pos[b, kv * g:(kv + 1) * g] == t
    assert hit[b, h] and (miss == hit).all(), f"rows that fail: {np.argwhere(miss).tolist()}, rows on the token: {np.argwhere(hit).tolist()}"


@pytest.mark.parametrize("engine", ["valu", "dot2", "mfma"])
@pytest.mark.parametrize("shape", ["small", "c3"])
def test_finite_gap_sinks_within_the_model_bound(engine, shape):
    """Sinks 6, 12, 20 and 28 logits above flat data, K with four outlier channels x 16: the fused output within the float64 model's
    bound (exact_data.hook_model) of the hook's arithmetic, element by element."""
    from mustafar_amd import compression
    Hq, Hkv, s, L, B = (32, 8, 0.7, 8192, 8) if shape == "c3" else (16, 4, 0.7, 1300, 2)
    C = ((L - 32) // 256) * 256
    rng = np.random.default_rng(13)
    worst = []
    for gap in (6, 12, 20, 28):
        sink = rng.integers(0, L + 1, (B, Hq))
        K, V, q = xd.sink_data(B, Hq, Hkv, L + 1, gap, sink, seed=gap, device=DEV)
        attn = _attn((Hq, Hkv, s), engine=engine, structure="one_pass", arena=True)
        out, _ = attn.decode(q, K[:, :, L:].contiguous(), V[:, :, L:].contiguous(),
                             attn.to_fused(attn.build_cache(K[:, :, :L].contiguous(), V[:, :, :L].contiguous())))
        Kp, Vp = K.clone(), V.clone()
        Kp[:, :, :C] = compression.prune_magnitude(K[:, :, :C].contiguous(), s)
        Vp[:, :, :C] = compression.prune_magnitude(V[:, :, :C].contiguous(), s)
        want, bound = xd.hook_model(q, Kp, Vp, Hq // Hkv)
        ratio = float(((out.double() - want).abs() / bound).max())
        worst.append(ratio)
        del Kp, Vp, want, bound
    assert max(worst) <= 1.0, f"{engine} {shape}: |fused - model| / bound by gap (6, 12, 20, 28): {[round(w, 3) for w in worst]}"
