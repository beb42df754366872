"""GPU: fused decode at every GQA group count 1..8.  pick_g() maps the group count to a kernel width G in {4, 2, 1} and the grid
gets groups / G workgroup rows per kv head: 3, 5, 6, 7 and 8 (Llama-3.2-3B, Qwen2.5-14B, Qwen2-1.5B, Qwen2.5-7B, Llama-3-70B) are the
counts where that is more than one, so the q-row / slab indexing, the row kernel's slab walk, the mask rows, the extents path and the
window workgroups' "first head of the group stores the new row" rule run with a sub-group index other than 0.  1, 2 and 4 are the
controls.  Each structure and one-pass form runs (mustafar_last_decode_choice() confirms it), held on random data against the float64
model of the hook's arithmetic over the oracle-pruned K / V and against the unfused call sequence, and bit-exactly on needle data
(tests/exact_data.py)."""
import numpy as np
import pytest
import torch

from tests import exact_data as xd
from tests.test_gpu_mask import _left_padding_mask
from tests.util import NATIVE_ULPS, excess

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROUPS = [(8, 8), (8, 4), (9, 3), (8, 2), (10, 2), (12, 2), (14, 2), (16, 2)]     # (Hq, Hkv): group counts 1 .. 8
IDS = [f"g{hq // hkv}" for hq, hkv in GROUPS]


def _lib():
    from mustafar_amd import _lib as lib
    return lib.load()


# form name -> (MustafarConfig.structure, mustafar_tune knobs, what mustafar_last_decode_choice() reports: structure bit, one-pass form or None)
FORMS = {
    "default": (None, (), 1, None),
    "two_launch": ("two_launch", (), 0, None),
    "pair": ("one_pass", ((8, 0),), 1, 2),        # round 4's pair form (super-block form off)
    "small": ("one_pass", ((11, 2),), 1, 4),      # round 6's small-launch kernel forced on
}
RESET = {8: 1, 11: 1}


@pytest.fixture
def form(request):
    structure, knobs, sbit, pform = FORMS[request.param]
    L = _lib()
    for k, v in knobs:
        assert L.mustafar_tune(k, v) == 0
    yield structure, sbit, pform
    for k, _ in knobs:
        L.mustafar_tune(k, RESET[k])


def _attn(hq, hkv, api="fused", **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=hq, num_key_value_heads=hkv, k_sparsity=0.7, v_sparsity=0.7, api=api, **kw))


def _check_choice(sbit, pform, engine=None):
    c = _lib().mustafar_last_decode_choice()
    assert (c >> 4) & 1 == sbit, f"structure: choice {c:#x}"
    if pform is not None:
        assert (c >> 8) & 15 == pform, f"one-pass form: choice {c:#x}"
    if engine is not None:
        assert c & 15 == engine, f"engine: choice {c:#x}"
    return c


def _model_ok(out, q, K, V, C, groups, pads=None):
    """exact_data.model_ok at this module's sparsity (0.7 for K and V)."""
    xd.model_ok(out, q, K, V, C, groups, pads, k_sparsity=0.7, v_sparsity=0.7)


def _fork(past):
    return (past[0], past[1].clone(), past[2], past[3].clone(), past[4], past[5])


@pytest.mark.parametrize("form", list(FORMS), indirect=True)
@pytest.mark.parametrize("hq,hkv", GROUPS, ids=IDS)
def test_every_group_count_through_every_form(hq, hkv, form):
    structure, sbit, pform = form
    torch.manual_seed(hq * 31 + hkv)
    bsz, D, L0 = 2, 128, 1300                         # 1024 compressed tokens, 276 in the window
    groups = hq // hkv
    attn, native = _attn(hq, hkv, structure=structure, arena=True), _attn(hq, hkv, api="native")
    K = torch.randn(bsz, hkv, L0, D, device=DEV).half()
    V = torch.randn(bsz, hkv, L0, D, device=DEV).half()
    past = attn.to_fused(attn.build_cache(K.clone(), V.clone()))
    past_n = native.build_cache(K.clone(), V.clone())
    assert past[4] == 1024
    for _ in range(3):
        q, kn, vn = (torch.randn(bsz, h, 1, D, device=DEV).half() for h in (hq, hkv, hkv))
        K, V = torch.cat([K, kn], 2), torch.cat([V, vn], 2)
        out, past = attn.decode(q, kn, vn, past)
        _check_choice(sbit, pform)
        out_n, past_n = native.decode(q, kn, vn, past_n)
        _model_ok(out, q, K, V, 1024, groups)
        assert excess(out, out_n, NATIVE_ULPS) <= 1.0
    # needles: every row its own token -- block edges, the window's first and last row, the step's new row
    L = L0 + 1
    rng = np.random.default_rng(groups)
    pos = xd.assign_rows(xd.edge_positions(1024, L), bsz, hq, rng, L)
    for pos1 in pos:
        Kn, Vn, qn, _ = xd.needle_data(bsz, hq, hkv, L, pos1, seed=groups, device=DEV)
        a = _attn(hq, hkv, structure=structure, arena=True)
        p = a.to_fused(a.build_cache(Kn[:, :, :L0].contiguous(), Vn[:, :, :L0].contiguous()))
        out, _ = a.decode(qn, Kn[:, :, L0:].contiguous(), Vn[:, :, L0:].contiguous(), p)
        _check_choice(sbit, pform)
        miss = xd.needle_misses(out, xd.needle_expect(Vn, pos1, 1024, 0.7, hq))
        assert not miss.any(), f"needle rows wrong: {miss.nonzero().tolist()[:8]} targets {pos1[miss.cpu().numpy()][:8].tolist()}"


@pytest.mark.parametrize("engine,code", [("dot2", 2), ("valu", 0), ("mfma", 1)])
@pytest.mark.parametrize("hq,hkv", [(16, 2), (64, 8)], ids=["g8", "g8-64x8"])
def test_group_count_8_on_every_engine(hq, hkv, engine, code):
    """G = 4 with two workgroup rows per kv head: the only group count > 4 where the engine choice applies."""
    torch.manual_seed(3)
    bsz, D, L0 = 2, 128, 1300
    attn = _attn(hq, hkv, engine=engine, structure="one_pass", arena=True)
    K = torch.randn(bsz, hkv, L0, D, device=DEV).half()
    V = torch.randn(bsz, hkv, L0, D, device=DEV).half()
    past = attn.to_fused(attn.build_cache(K.clone(), V.clone()))
    q, kn, vn = (torch.randn(bsz, h, 1, D, device=DEV).half() for h in (hq, hkv, hkv))
    out, _ = attn.decode(q, kn, vn, past)
    _check_choice(1, None, code)
    _model_ok(out, q, torch.cat([K, kn], 2), torch.cat([V, vn], 2), 1024, hq // hkv)
    L = L0 + 1
    for pos1 in xd.assign_rows(xd.edge_positions(1024, L), bsz, hq, np.random.default_rng(8), L):
        Kn, Vn, qn, _ = xd.needle_data(bsz, hq, hkv, L, pos1, seed=8, device=DEV)
        a = _attn(hq, hkv, engine=engine, structure="one_pass", arena=True)
        out, _ = a.decode(qn, Kn[:, :, L0:].contiguous(), Vn[:, :, L0:].contiguous(), a.to_fused(a.build_cache(Kn[:, :, :L0].contiguous(), Vn[:, :, :L0].contiguous())))
        _check_choice(1, None, code)
        assert not xd.needle_misses(out, xd.needle_expect(Vn, pos1, 1024, 0.7, hq)).any()


@pytest.mark.parametrize("structure", ["one_pass", "two_launch"])
@pytest.mark.parametrize("hq,hkv", GROUPS, ids=IDS)
def test_every_group_count_with_a_left_padding_mask(hq, hkv, structure):
    torch.manual_seed(5)
    bsz, D, L0 = 3, 128, 1300
    groups = hq // hkv
    pads = (0, 70, 1100)                              # batch 2 masks the whole compressed part and some of the window
    attn, native = _attn(hq, hkv, structure=structure), _attn(hq, hkv, api="native")
    K = torch.randn(bsz, hkv, L0, D, device=DEV).half()
    V = torch.randn(bsz, hkv, L0, D, device=DEV).half()
    past, past_n = attn.build_cache(K.clone(), V.clone()), native.build_cache(K.clone(), V.clone())
    for step in range(3):
        q, kn, vn = (torch.randn(bsz, h, 1, D, device=DEV).half() for h in (hq, hkv, hkv))
        K, V = torch.cat([K, kn], 2), torch.cat([V, vn], 2)
        mask = _left_padding_mask(bsz, L0 + step + 1, pads)
        out, past = attn.decode(q, kn, vn, past, attention_mask=mask)
        _check_choice(1 if structure == "one_pass" else 0, None)
        out_n, past_n = native.decode(q, kn, vn, past_n, attention_mask=mask)
        _model_ok(out, q, K, V, 1024, groups, pads)
        assert excess(out, out_n, NATIVE_ULPS) <= 1.0
    # needles: a row whose needle lies under the mask falls to its secondary needle, exactly
    L = L0 + 1
    rng = np.random.default_rng(groups)
    pos1 = rng.integers(0, L, (bsz, hq))
    pos1[:, 0], pos1[:, 1] = 0, 69                    # masked in batch entries 1 and 2
    pos2 = rng.integers(1100, L, (bsz, hq))
    pos2[pos2 == pos1] = -1
    Kn, Vn, qn, _ = xd.needle_data(bsz, hq, hkv, L, pos1, pos2, seed=groups, device=DEV)
    a = _attn(hq, hkv, structure=structure)
    mask = _left_padding_mask(bsz, L, pads)
    out, _ = a.decode(qn, Kn[:, :, L0:].contiguous(), Vn[:, :, L0:].contiguous(), a.build_cache(Kn[:, :, :L0].contiguous(), Vn[:, :, :L0].contiguous()),
                      attention_mask=mask)
    masked = (mask[:, 0, 0] < 0).cpu().numpy()
    assert not xd.needle_misses(out, xd.needle_expect(Vn, pos1, 1024, 0.7, hq, pos2=pos2, masked=masked)).any()


@pytest.mark.parametrize("hq,hkv", GROUPS, ids=IDS)
def test_every_group_count_across_a_trigger(hq, hkv):
    """A 256-token trigger on an arena cache: the cache grows by an extent wherever mustafar_decode_reads_extents accepts the
    group count.  Needles on the last base token and the first token of the extent after it."""
    from mustafar_amd import _lib as lib
    groups = hq // hkv
    bsz, D, C0 = 2, 128, 1024
    L0 = C0 + 32 + 250                                # the trigger fires at the 6th step
    steps = 8
    L = L0 + steps
    rng = np.random.default_rng(groups)
    pos1 = rng.integers(0, L, (bsz, hq))
    pos1[:, :4] = (C0 - 1, C0, C0 + 255, C0 + 256)    # last base token, first and last extent tokens, first window row after the trigger
    pos1[0, -1] = L - 1
    Kn, Vn, qn, _ = xd.needle_data(bsz, hq, hkv, L, pos1, seed=groups, device=DEV)
    attn = _attn(hq, hkv, arena=True)
    past = attn.to_fused(attn.build_cache(Kn[:, :, :L0].contiguous(), Vn[:, :, :L0].contiguous()))
    torch.manual_seed(groups)
    K, V = Kn[:, :, :L0].clone(), Vn[:, :, :L0].clone()
    C = C0
    for step in range(steps):
        t = L0 + step
        kn, vn = Kn[:, :, t:t + 1].contiguous(), Vn[:, :, t:t + 1].contiguous()
        K, V = torch.cat([K, kn], 2), torch.cat([V, vn], 2)
        q = qn if step == steps - 1 else (torch.randn(bsz, hq, 1, D, device=DEV) / 16).half()    # (small: the needle keys hold 16s)
        out, past = attn.decode(q, kn, vn, past)
        if step < steps - 1:
            _model_ok(out, q, K, V, C, groups)
        C = past[4]
    assert C == C0 + 256
    ld = (C + past[1].cap + 31) // 32 * 32
    if lib.load().mustafar_decode_reads_extents(groups, ld, 0):
        assert len(past[0].extents) == 1, "the trigger did not add an extent where the launch reads extents"
    assert not xd.needle_misses(out, xd.needle_expect(Vn, pos1, C, 0.7, hq)).any()


@pytest.mark.parametrize("hq,hkv", GROUPS, ids=IDS)
def test_every_group_count_under_graph_replay(hq, hkv):
    """One captured step replayed while the window grows: random steps against dense attention, then needle queries that move
    the needles between replays (two needle sets on disjoint slots, q alone selects one)."""
    from mustafar_amd import _lib as lib_mod
    lib = _lib()
    groups = hq // hkv
    bsz, D, L0 = 2, 128, 1300
    replays = 6
    L = L0 + replays
    rng = np.random.default_rng(groups)
    pos_a = xd.assign_rows(xd.edge_positions(1024, L0), bsz, hq, rng, L0)[0]
    pos_b = rng.integers(0, L0, (bsz, hq))
    pos_b[0, 0], pos_b[-1, -1] = L0 - 1, 1023
    Kn, Vn, qa, (qb,) = xd.needle_data(bsz, hq, hkv, L, pos_a, alt=[pos_b], seed=groups, device=DEV)
    attn = _attn(hq, hkv, arena=True)
    past = attn.to_fused(attn.build_cache(Kn[:, :, :L0].contiguous(), Vn[:, :, :L0].contiguous()))
    q, kn, vn = (torch.zeros(bsz, h, 1, D, device=DEV, dtype=torch.float16) for h in (hq, hkv, hkv))
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    attn.decode_fused(q, kn, vn, _fork(past))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, _ = attn.decode_fused(q, kn, vn, past, step_counter=counter)
        lib_mod.check(lib.mustafar_counter_add(torch.cuda.current_stream().cuda_stream, counter.data_ptr(), 1), "counter")
    K, V = Kn[:, :, :L0].clone(), Vn[:, :, :L0].clone()
    torch.manual_seed(groups)
    for r in range(replays):
        t = L0 + r
        kn.copy_(Kn[:, :, t:t + 1]); vn.copy_(Vn[:, :, t:t + 1])
        K, V = torch.cat([K, kn.clone()], 2), torch.cat([V, vn.clone()], 2)
        if r % 3 == 0:
            qr = (torch.randn(bsz, hq, 1, D, device=DEV) / 16).half()
            q.copy_(qr)
            g.replay()
            _model_ok(out, qr, K, V, 1024, groups)
        else:
            pos, qq = (pos_a, qa) if r % 3 == 1 else (pos_b, qb)
            q.copy_(qq)
            g.replay()
            assert not xd.needle_misses(out, xd.needle_expect(Vn[:, :, :t + 1], pos, 1024, 0.7, hq)).any(), f"replay {r}"
    assert int(counter.item()) == replays
