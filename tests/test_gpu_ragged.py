"""GPU: ragged batches -- independent per-sequence caches decoded in one call (mustafar_ragged_set_sequences, mustafar_decode_ragged,
MustafarAttention.decode_ragged).

The comparator of the C call is the existing several-token call on each sequence alone, bit for bit (R1: the result does not depend on
the batch), next to the float64 models of tests/exact_data.py and tests/partial_util.py (R2).  Three sequences of two kv heads:
nothing compressed / a base of 256 tokens / a base and two extents, windows of n_q / 70 / 129 rows in capacities of 64 / 128 / 320."""
import pytest
import torch

from tests import ragged_util as ru
from tests.hd64_util import DEV

pytestmark = pytest.mark.gpu
HKV = 2
ROWS = [(1, 1), (4, 1), (2, 3), (4, 4), (8, 8), (4, 16)]   # (groups, n_q): row tiles 1 and 4, R = 1, 4, 6, 16, 64
ORDERS = {"in order": [0, 1, 2], "rotated": [2, 0, 1], "a hole": [1, None, 2, 0]}
cases = pytest.mark.parametrize("Dd,groups,n_q", [(Dd, g, n) for Dd in (64, 128) for g, n in ROWS])


@pytest.fixture(scope="module")
def pkg():
    from mustafar_amd import _lib, compression
    return _lib.load(), compression


def _seqs(pkg, Dd, groups, n_q, entries=None):
    shapes = [(0, n_q, 64), (256, 70, 128), (768, 129, 320)]
    return [ru.Seq(pkg, Dd, HKV, groups, n_q, T, w, cap, seed=Dd + 7 * i + groups * n_q, entries=entries)
            for i, (T, w, cap) in enumerate(shapes)]


_RESULTS = {}


def results(pkg, Dd, groups, n_q):
    """The sequences, each one's call alone, and the ragged call over every slot order; computed once per shape and left unchanged."""
    key = (Dd, groups, n_q)
    if key not in _RESULTS:
        seqs = _seqs(pkg, Dd, groups, n_q)
        solo = [s.solo() for s in seqs]
        runs = {name: ru.run_slots(pkg, seqs, slots) for name, slots in ORDERS.items()}
        _RESULTS[key] = (seqs, solo, runs)
    return _RESULTS[key]


@cases
def test_r1_a_sequence_does_not_see_its_batch(pkg, Dd, groups, n_q):
    """out and lse of every sequence are bit for bit those of mustafar_decode_multi_query on that sequence alone: in slot order, in another
    order, with an empty slot between them."""
    seqs, solo, runs = results(pkg, Dd, groups, n_q)
    for name, slots in ORDERS.items():
        out, lse, _ = runs[name]
        for slot, i in enumerate(slots):
            if i is None:
                continue
            assert torch.equal(ru.bits(out[slot]), ru.bits(solo[i][0][0])), f"{name}: out of sequence {i} in slot {slot}"
            assert torch.equal(ru.bits(lse[slot]), ru.bits(solo[i][1][0])), f"{name}: lse of sequence {i} in slot {slot}"


@cases
def test_r2_the_float64_models_hold(pkg, Dd, groups, n_q):
    seqs, _, runs = results(pkg, Dd, groups, n_q)
    out, lse, _ = runs["in order"]
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    for i, s in enumerate(seqs):
        r_out, r_lse = s.model_ratios(out[i:i + 1], lse[i:i + 1])
        print(f"D={Dd} R={groups * n_q} sequence {i}: |out - model| / bound = {r_out:.3f}, |lse - model| / bound = {r_lse:.3f}")
        assert r_out <= 1.0 and r_lse <= 1.0, f"sequence {i}: out {r_out:.3f}, lse {r_lse:.3f}"


@cases
def test_r3_windows(pkg, Dd, groups, n_q):
    """Rows [w_len - n_q, w_len) of every sequence's windows hold its new rows, every other half is what it was (NaNs included); with
    the rows stored and k_new = v_new = NULL nothing changes and the outputs are the appending call's."""
    seqs, solo, runs = results(pkg, Dd, groups, n_q)
    for name, slots in ORDERS.items():
        out, lse, wins = runs[name]
        for slot, i in enumerate(slots):
            if i is None:
                continue
            s = seqs[i]
            for got, was, new in ((wins[slot][0], s.kw, s.kn), (wins[slot][1], s.vw, s.vn)):
                want = was.clone()
                want[:, s.w_len - n_q:s.w_len] = new[0]
                assert torch.equal(ru.bits(got), ru.bits(want)), f"{name}: a window of sequence {i}"
    slots = ORDERS["a hole"]
    out, lse, _ = runs["a hole"]
    out2, lse2, wins = ru.run_slots(pkg, seqs, slots, stored=True)
    for slot, i in enumerate(slots):
        if i is None:
            continue
        kw, vw = seqs[i].stored_windows()
        assert torch.equal(ru.bits(wins[slot][0]), ru.bits(kw)) and torch.equal(ru.bits(wins[slot][1]), ru.bits(vw))
    assert torch.equal(ru.bits(out2), ru.bits(out)) and torch.equal(ru.bits(lse2), ru.bits(lse))


@cases
def test_r4_an_empty_slot(pkg, Dd, groups, n_q):
    """window_len = 0 and every pointer NULL: out = +0, lse = -inf, and no NaN anywhere in the batch's outputs."""
    _, _, runs = results(pkg, Dd, groups, n_q)
    out, lse, _ = runs["a hole"]
    slot = ORDERS["a hole"].index(None)
    assert not torch.isnan(out.float()).any() and not torch.isnan(lse).any()
    assert (ru.bits(out[slot]) == 0).all(), "out of the empty slot is not +0"
    assert (lse[slot] == float("-inf")).all(), "lse of the empty slot is not -inf"


# ---- R5: one graph over a changing batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd,groups,n_q", [(128, 4, 4), (64, 8, 8)])
def test_r5_one_graph_over_a_changing_batch(pkg, Dd, groups, n_q):
    """The call captured once; between the replays entries are rewritten by mustafar_ragged_set_sequences outside the graph: a window
    grows by n_q, a sequence gains an extent, a sequence leaves, another takes a free slot.  After each of four replays out and lse are
    those of an eager call on the same table, bit for bit."""
    a, b, c = _seqs(pkg, Dd, groups, n_q, entries=2)
    # the sequence that gains an extent: 256 tokens in its base, 256 + 40 rows in its window; its tables have an entry to spare
    d = ru.Seq(pkg, Dd, HKV, groups, n_q, 512, 40 + n_q, 320, seed=Dd + 99, entries=2)
    d.kt.zero_()   # (not listed yet: entries not in use are all zero)
    d.vt.zero_()
    d_kw = torch.full((HKV, d.cap, Dd), ru.NAN, dtype=torch.float16, device=DEV)
    d_vw = torch.full_like(d_kw, ru.NAN)
    d_kw[:, :256 + 40], d_vw[:, :256 + 40] = d.K[0, :, 256:552], d.V[0, :, 256:552]   # (unpruned rows 256 .. 511: still in the window)
    wins = {s: (s.kw.clone(), s.vw.clone()) for s in (a, b, c)}
    bt = ru.Batch(pkg, 4, Dd, HKV, groups, n_q, 768, 320)
    bt.set(0, [a.item(*wins[a]), d.item(d_kw, d_vw, T=256, w_len=256 + 40 + n_q), c.item(*wins[c]), None])
    for slot, s in enumerate((a, d, c)):
        bt.load(slot, s)
    bt.decode()   # (module load outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bt.decode()
    e_out, e_lse = torch.empty_like(bt.out), torch.empty_like(bt.lse)

    def replay_and_compare(what):
        bt.out.fill_(ru.NAN)
        bt.lse.fill_(ru.NAN)
        graph.replay()
        e_out.fill_(ru.NAN)
        e_lse.fill_(ru.NAN)
        bt.decode(e_out, e_lse)   # (appends the same rows to the same places)
        torch.cuda.synchronize()
        assert not torch.isnan(e_out.float()).any() and not torch.isnan(e_lse).any(), what
        assert torch.equal(ru.bits(bt.out), ru.bits(e_out)) and torch.equal(ru.bits(bt.lse), ru.bits(e_lse)), what
        return bt.out.clone()

    # 1. the window of the sequence in slot 0 grows by n_q
    bt.set(0, [a.item(*wins[a], w_len=a.w_len + n_q)])
    o1 = replay_and_compare("a window grew")
    # 2. the sequence in slot 1 gains an extent: the new table entry first, then T + 256 and the window slid by 256 rows
    d.list_extent(0)
    d_kw[:, :40], d_vw[:, :40] = d_kw[:, 256:296].clone(), d_vw[:, 256:296].clone()
    bt.set(1, [d.item(d_kw, d_vw, T=512, w_len=40 + n_q)])
    o2 = replay_and_compare("a sequence gained an extent")
    r_out, r_lse = d.model_ratios(bt.out[1:2], bt.lse[1:2])   # (now the sequence `d` was built as: 512 compressed tokens, 40 + n_q rows)
    assert r_out <= 1.0 and r_lse <= 1.0, f"after the extent: out {r_out:.3f}, lse {r_lse:.3f}"
    assert not torch.equal(o1[1], o2[1])
    # 3. the sequence in slot 2 leaves
    bt.set(2, [None])
    o3 = replay_and_compare("a sequence left")
    assert (ru.bits(o3[2]) == 0).all() and (bt.lse[2] == float("-inf")).all()
    # 4. another sequence takes the free slot 3
    bt.set(3, [b.item(*wins[b])])
    bt.load(3, b)
    o4 = replay_and_compare("a sequence joined")
    assert torch.equal(ru.bits(o4[3]), ru.bits(b.solo()[0][0]))


# ---- R6: the Python call through per-sequence triggers --------------------------------------------------------------------------------------
KINDS = {"arena": (128, dict(arena=True)), "ext64": (64, dict(hd64_extents=True)), "list": (128, dict())}
PROMPTS = (100, 541, 830)
N_Q = (1, 2, 1, 4, 2, 1)
REJECTED = {(1, 1): 1, (3, 1): 2}   # (call, sequence) -> rows rejected; everything else accepts all


def _hook(Dd, groups, **kw):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=HKV * groups, num_key_value_heads=HKV, head_dim=Dd, k_sparsity=0.7,
                                            v_sparsity=0.7, api="fused", **kw))


def _reference(c):
    """A compressed cache of any kind as four flat tensors (bitmaps, offsets, stream, nz_offset); nothing compressed: none."""
    if c is None:
        return []
    c = c.to_reference() if hasattr(c, "to_reference") else c
    nz = c[2]
    return [c[0].reshape(-1), c[1].reshape(-1), nz if isinstance(nz, torch.Tensor) else torch.cat(list(nz)), c[3].reshape(-1)]


def _same_cache(a, b):
    ra, rb = _reference(a), _reference(b)
    return len(ra) == len(rb) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(ra, rb))


@pytest.mark.parametrize("kind", list(KINDS))
def test_r6_decode_ragged_through_per_sequence_triggers(kind):
    """Three bsz-1 pasts (prompts of 100 / 541 / 830 tokens: 0 / 256 / 768 compressed, windows of 100 / 285 / 62 rows), six decode_ragged
    calls closed per sequence with accept(); sequence 1 rejects one row of the second call and two of the fourth, and alone reaches a
    trigger point (the second call's last row is row 544 = 256 + 32 + 256; with that row rejected the third call brings it again and
    accept() compresses the extent then).  Every output and LSE equals the same
    schedule driven per sequence by decode_multi + accept, bit for bit, and so do the final lengths, windows and cache contents; every
    output is within the float64 model's bound."""
    from tests import exact_data as xd
    from tests import partial_util as pu
    Dd, kw = KINDS[kind]
    groups, H = 4, HKV * 4
    attn, solo = _hook(Dd, groups, **kw), _hook(Dd, groups, **kw)
    g = torch.Generator(device=DEV).manual_seed(Dd + len(kind))
    total = sum(N_Q)
    K = [torch.randn((1, HKV, L + total, Dd), generator=g, device=DEV).half() for L in PROMPTS]
    V = [torch.randn((1, HKV, L + total, Dd), generator=g, device=DEV).half() for L in PROMPTS]
    Q = [torch.randn((1, H, total, Dd), generator=g, device=DEV).half() for _ in PROMPTS]
    pasts = [attn.to_fused(attn.build_cache(K[s][:, :, :L].contiguous(), V[s][:, :, :L].contiguous())) for s, L in enumerate(PROMPTS)]
    refs = [solo.to_fused(solo.build_cache(K[s][:, :, :L].contiguous(), V[s][:, :, :L].contiguous())) for s, L in enumerate(PROMPTS)]
    assert [p[4] for p in pasts] == [0, 256, 768] and [p[1].len for p in pasts] == [100, 285, 62]
    n = list(PROMPTS)        # tokens each sequence holds
    dense = [(K[s][:, :, :L].clone(), V[s][:, :, :L].clone()) for s, L in enumerate(PROMPTS)]   # the rows each sequence holds, in order
    fed = 0
    triggers = [0, 0, 0]
    for call, n_q in enumerate(N_Q):
        for s in range(3):
            assert attn.fits_before_trigger(pasts[s], n_q) == n_q, f"call {call}: sequence {s}"
        sl = slice(fed, fed + n_q)
        q = torch.cat([Q[s][:, :, sl] for s in range(3)])
        k = torch.cat([K[s][:, :, PROMPTS[s] + fed:PROMPTS[s] + fed + n_q] for s in range(3)])
        v = torch.cat([V[s][:, :, PROMPTS[s] + fed:PROMPTS[s] + fed + n_q] for s in range(3)])
        out, lse, pasts = attn.decode_ragged(q, k, v, pasts, return_lse=True)
        assert out.shape == (3, H, n_q, Dd) and lse.shape == (3, H, n_q)
        for s in range(3):
            o, l, refs[s] = solo.decode_multi(q[s:s + 1], k[s:s + 1], v[s:s + 1], refs[s], return_lse=True)
            assert torch.equal(ru.bits(out[s:s + 1]), ru.bits(o)) and torch.equal(ru.bits(lse[s:s + 1]), ru.bits(l)), \
                f"call {call}: sequence {s} differs from its own decode_multi"
            # the dense float64 model on what each token may see (pruned where compressed)
            C = pasts[s][4]
            Kd, Vd = torch.cat([dense[s][0], k[s:s + 1]], 2), torch.cat([dense[s][1], v[s:s + 1]], 2)
            Kp, Vp = pu.pruned_rows(Kd, Vd, C)
            for j in range(n_q):
                Lj = n[s] + j + 1
                want, bound = xd.hook_model(q[s:s + 1, :, j:j + 1], Kp[:, :, :Lj], Vp[:, :, :Lj], groups)
                r = float(((out[s:s + 1, :, j:j + 1].double() - want).abs() / bound).max())
                want_l, bound_l = pu.lse_model(q[s:s + 1, :, j:j + 1], Kp[:, :, :Lj], groups)
                r_l = pu.lse_ratio(lse[s:s + 1, :, j], want_l, bound_l)
                assert r <= 1.0 and r_l <= 1.0, f"call {call}: sequence {s} token {j}: out {r:.3f}, lse {r_l:.3f} of the model's bound"
            rej = REJECTED.get((call, s), 0)
            before = pasts[s][4]
            pasts[s] = attn.accept(pasts[s], rejected=rej)
            refs[s] = solo.accept(refs[s], rejected=rej)
            triggers[s] += pasts[s][4] != before
            keep = n_q - rej
            dense[s] = (Kd[:, :, :n[s] + keep], Vd[:, :, :n[s] + keep])
            n[s] += keep
            assert pasts[s][5] == refs[s][5] == n[s] and pasts[s][4] == refs[s][4]
        fed += n_q
        if call == 2:   # (544 = 256 + 32 + 256 rows: reached with the third call, the second having lost a row)
            assert triggers == [0, 1, 0], "sequence 1, and it alone, has reached its trigger point and compressed an extent"
    assert triggers == [0, 1, 0] and [p[4] for p in pasts] == [0, 512, 768]
    for s in range(3):
        a, b = pasts[s], refs[s]
        assert a[1].len == b[1].len and a[3].len == b[3].len
        assert torch.equal(ru.bits(a[1].view()), ru.bits(b[1].view())) and torch.equal(ru.bits(a[3].view()), ru.bits(b[3].view()))
        assert _same_cache(a[0], b[0]), f"sequence {s}: the key caches differ"
        assert _same_cache(a[2], b[2]), f"sequence {s}: the value caches differ"


def test_r6_a_call_over_a_trigger_point_names_the_sequence():
    """Sequence 1 of 541 tokens is three rows short of its trigger point (256 + 32 + 256 = 544): a call of four tokens raises ValueError
    naming index 1 and the 3 tokens that fit, and leaves every past as it was."""
    Dd, groups, H = 128, 4, HKV * 4
    attn = _hook(Dd, groups, arena=True)
    g = torch.Generator(device=DEV).manual_seed(5)
    pasts = []
    for L in PROMPTS:
        K, V = (torch.randn((1, HKV, L, Dd), generator=g, device=DEV).half() for _ in range(2))
        pasts.append(attn.to_fused(attn.build_cache(K, V)))
    state = [(p[1].len, p[3].len, p[4], p[5], ru.bits(p[1].view()).clone(), p[1].buf.data_ptr()) for p in pasts]
    q = torch.zeros((3, H, 4, Dd), dtype=torch.float16, device=DEV)
    k = torch.zeros((3, HKV, 4, Dd), dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match=r"sequence 1\b.*at most 3\b"):
        attn.decode_ragged(q, k, k, pasts)
    for p, (kl, vl, C, L, rows, ptr) in zip(pasts, state):
        assert (p[1].len, p[3].len, p[4], p[5], p[1].buf.data_ptr()) == (kl, vl, C, L, ptr) and torch.equal(ru.bits(p[1].view()), rows)
