"""GPU: attention masks and draft trees in the several-token decode call (ABI 114: mustafar_decode_multi_query_masked,
mustafar_window_keep_rows, MustafarAttention.decode_multi(attention_mask=) and accept(keep=)).

Comparators: the float64 models of tests/exact_data.py and tests/partial_util.py with their mask argument and their derived bounds -- query
token j evaluated on the rows it may see under its own mask row --, needles whose stronger twin is masked (output = the primary needle's V
row bit for bit, LSE = its x exactly), the unmasked entry point (an all-zero mask: the same bits) and a twin hook fed the accepted tokens
alone.  Every mask is housed in a larger NaN tensor at an odd element offset (tests/multi_mask_util.py); unused window rows are NaN.
kv heads <= 2, batch <= 2, C <= 512."""
import numpy as np
import pytest
import torch

from tests import multi_mask_util as mm
from tests import shared_util as su
from tests import test_gpu_multi_query as mq
from tests.hd64_util import DEV

pytestmark = pytest.mark.gpu
NEG, NAN = mm.NEG, mm.NAN


@pytest.fixture(scope="module")
def pkg():
    from mustafar_amd import _lib, compression
    return _lib.load(), compression


def _holes(gen, C, w0, count=3):
    """`count` columns of the compressed part and one of the old window rows."""
    return sorted(int(t) for t in torch.randperm(C, generator=gen)[:count]) + [C + int(torch.randint(0, w0, (1,), generator=gen))]


def _mask_b(B, n_q, C, w0, seed):
    """Mask (b): a random tree among the new tokens, three holes per sequence in the compressed part and one in the window, another set per
    sequence."""
    gen = torch.Generator().manual_seed(seed)
    holes = [_holes(gen, C, w0) for _ in range(B)]
    assert len({tuple(h) for h in holes}) == B
    return mm.tree_mask(B, mm.random_tree(n_q, gen), C + w0, holes)


# ---- 1. random data against the models, through the C entry point ---------------------------------------------------------------------------
ROWS = [(4, 4), (4, 8), (8, 5), (4, 16)]   # (groups, n_q): row tiles 1, 2, 3 and 4


@pytest.fixture(scope="module")
def random_calls(pkg):
    """One set of operands per (D, groups, n_q), shared by the masks: C = 192, 60 window rows before the call (the new rows straddle the
    chunk edge at 64), batch 2, 2 kv heads; with the unmasked call's outputs."""
    made = {}

    def get(Dd, groups, n_q):
        key = (Dd, groups, n_q)
        if key not in made:
            K, V, q = mq._rand(2, 2, 192 + 60 + n_q, groups, n_q, Dd, seed=Dd + groups * n_q)
            c = mq.Call(pkg, K, V, 192, n_q, groups)
            out, lse = c.call(q)
            made[key] = (c, q, out.clone(), lse.clone())
        return made[key]
    return get


@pytest.mark.parametrize("kind", ["a-pad37", "a-pad-into-window", "b-tree-holes", "c-biases", "d-zero", "e-plane-per-head"])
@pytest.mark.parametrize("groups,n_q", ROWS)
@pytest.mark.parametrize("Dd", [64, 128])
def test_random_data_against_the_models(random_calls, Dd, groups, n_q, kind):
    B, Hkv, C, w0 = 2, 2, 192, 60
    c, q, out0, lse0 = random_calls(Dd, groups, n_q)
    cols = C + w0 + n_q
    gen = torch.Generator().manual_seed(n_q + Dd)
    hpm = Hkv
    if kind == "a-pad37":
        m = mm.left_padding((0, 37), cols)
    elif kind == "a-pad-into-window":
        m = mm.left_padding((0, C + 5), cols)       # a whole compressed part and five window rows
    elif kind == "b-tree-holes":
        m = _mask_b(B, n_q, C, w0, seed=Dd + n_q)
    elif kind == "c-biases":
        m = (-torch.randint(0, 33, (B, n_q, cols), generator=gen).half() * 0.125)   # multiples of 2^-3 in [-4, 0]
    elif kind == "d-zero":
        m = mm.zeros(B, n_q, cols)
    else:                                            # a plane per B' head: holes at -inf and finite biases, another set per head
        hpm = 1
        m = (-torch.randint(0, 9, (B * Hkv, n_q, cols), generator=gen).half() * 0.5)
        m[torch.rand((B * Hkv, 1, cols), generator=gen).expand(-1, n_q, -1) < 0.3] = float("-inf")
        m[:, :, C + w0 - 1] = 0.0                    # (every row keeps a column)
    dev_mask = mm.housed(m)
    out, lse = mm.call_masked(c, q, dev_mask, hpm)
    mask4 = mm.per_head(dev_mask, B, Hkv * groups, groups * hpm)
    mm.assert_models(out, lse, q, c.Kp, c.Vp, C + w0, groups, mask4, f"D={Dd} R={n_q * groups} {kind}")
    if kind == "d-zero":                             # x + 0 = x, nothing is clamped: the unmasked call's bits
        assert torch.equal(mq._bits(out), mq._bits(out0)) and torch.equal(mq._bits(lse), mq._bits(lse0))
    elif kind != "c-biases":                         # (holes and padding change the result: the mask was applied at all)
        assert not torch.equal(mq._bits(out), mq._bits(out0))


# ---- 2. needles, exact: the stronger needle of each row is masked -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["own-row-only", "sequence-1-only"])
@pytest.mark.parametrize("n_q,groups", [(4, 4), (7, 5)])   # R = 16 and R = 35
@pytest.mark.parametrize("Dd", [64, 128])
def test_a_masked_needle_gives_way_to_the_primary_one(pkg, Dd, n_q, groups, variant):
    """Every row has a primary needle and one of twice the level in the same slot, the latter on the first and last token of the first and
    last compressed block, the first window row, rows 63 and 64 of the window or the row's own new row.  Unmasked, the stronger one wins
    every row (which shows it is there).  own-row-only: row (b, h, j)'s stronger needle is masked in mask row j of sequence b and in no other
    row -- a mask row taken from another token leaves it standing.  sequence-1-only: all of sequence 1's are masked in every row of
    sequence 1, none in sequence 0, where the stronger needles must still win -- a plane taken from the wrong sequence shows either way."""
    B, Hkv, C, w0 = 2, 2, 192, 70
    H, Ltot = Hkv * groups, C + w0 + n_q
    strong_at = [0, 63, C - 64, C - 1, C, C + 63, C + 64, None]      # None: the row's own new row
    primary_at = [7, 20, 100, C - 70, C - 62, C + 9, C + 66]
    pos, twice = np.zeros((B, H, n_q), np.int64), np.zeros((B, H, n_q), np.int64)
    for i, (b, h, j) in enumerate(np.ndindex(B, H, n_q)):
        t = strong_at[(i + b) % len(strong_at)]
        twice[b, h, j] = C + w0 + j if t is None else t
        pos[b, h, j] = primary_at[i % len(primary_at)]
    K, V, q, w = mq.needle_data(Dd, B, Hkv, groups, n_q, Ltot, pos, C, seed=Dd + n_q, twice=twice)
    c = mq.Call(pkg, K, V, C, n_q, groups)
    out, _ = c.call(q)
    strong = mq.needle_want(V, twice, C, groups)
    assert torch.equal(out.float(), strong.float()), "unmasked, the stronger needle must win every row"
    m = mm.zeros(B, n_q, Ltot)
    for b, h, j in np.ndindex(B, H, n_q):
        if variant == "own-row-only":
            m[b, j, twice[b, h, j]] = NEG
        elif b == 1:
            m[b, :, twice[b, h, j]] = NEG
    out, lse = mm.call_masked(c, q, mm.housed(m), Hkv)
    want = mq.needle_want(V, pos, C, groups)
    want_lse = torch.full_like(lse, su.needle_x(Dd, w))
    if variant == "sequence-1-only":
        want[0], want_lse[0] = strong[0], su.needle_x(Dd, w, 2)
    miss = (out.float() != want.float()).any(-1)
    assert not miss.any(), f"rows {miss.nonzero().tolist()} differ from their needle's V row"
    assert torch.equal(lse, want_lse), "an LSE is not its needle's x"


# ---- 3. extents -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [3, 11])
@pytest.mark.parametrize("kind", ["arena", "ext64"])
def test_extents(pkg, kind, n_q):
    """A 256-token base and one 256-token extent at R = 12 (no run crosses a boundary) and R = 44 (run 0 crosses base -> extent), read off
    the workspace size as tests/test_gpu_multi_query.py does; mask (b) with holes on both sides of the crossing: the mask column of an
    extent's block is the global block number's."""
    B, Hkv, groups = 1, 2, 4
    attn = mq._attn(kind)
    Dd = attn.head_dim
    total = 512 + 32 + n_q
    K, V, q = mq._rand(B, Hkv, total, groups, n_q, Dd, seed=Dd + n_q)
    past, n = mq._grow(attn, K, V, q[:, :, :1].contiguous(), 1)
    assert n + n_q == total and len(past[0].extents) == 1 and past[0].tokens == 256 and past[4] == 512
    spans = mq._run_spans(pkg[0], past[4], past[1].cap, B * Hkv, groups, n_q, Dd)
    crossed = mq._crossings(spans)
    if n_q == 3:
        assert spans[0] == (0, 2) and not crossed
    else:
        assert spans[0] == (0, 5) and (0, "base->extent") in crossed
    gen = torch.Generator().manual_seed(n_q)
    m = mm.tree_mask(B, mm.random_tree(n_q, gen), n, [[3, 250, 255, 256, 257, 300, 511, 512 + 7]])
    dev_mask = mm.housed(m)
    out, lse, new = attn.decode_multi(q, K[:, :, n:], V[:, :, n:], past, return_lse=True, attention_mask=dev_mask[:, None])
    assert new[5] == total and new[1].len == 32 + n_q
    Kp, Vp = mq._pruned(attn, K, V, 512)
    mm.assert_models(out, lse, q, Kp, Vp, n, groups, dev_mask[:, None], f"{kind} R={n_q * groups}")


# ---- 4. a draft tree, then keep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_a_tree_is_verified_and_a_path_kept(Dd):
    """A complete binary tree of 7 drafted nodes over 256 compressed tokens and a 40-row window, batch 2.  Each node's output and LSE lie
    within the models' bounds evaluated on cache + the node's root path.  accept(keep=path), another root-to-leaf path per sequence, leaves
    the windows of a twin hook that was fed the path's tokens linearly; one further call gives the same bits on both."""
    B, Hkv, groups, L0 = 2, 2, 4, 256 + 40
    parent = [-1, 0, 0, 1, 1, 2, 2]
    attn = mq._attn("list", Dd=Dd)
    K, V, q = mq._rand(B, Hkv, L0 + 7 + 2, groups, 7 + 2, Dd, seed=Dd + 41)
    dev_mask = mm.housed(mm.tree_mask(B, parent, L0))
    out, lse, pa = attn.decode_multi(q[:, :, :7].contiguous(), K[:, :, L0:L0 + 7], V[:, :, L0:L0 + 7], mq._past(attn, K, V, L0),
                                     return_lse=True, attention_mask=dev_mask[:, None])
    Kp, Vp = mq._pruned(attn, K, V, 256)
    anc = mm.ancestors(parent)
    worst = [0.0, 0.0]
    for j in range(7):
        path = [L0 + i for i in range(7) if anc[j, i]]
        rows = list(range(L0)) + path
        r = mq._model_ratios(out[:, :, j:j + 1], lse[:, :, j:j + 1], q[:, :, j:j + 1], Kp[:, :, rows], Vp[:, :, rows], len(rows) - 1, groups)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"D={Dd} tree: |out - model| / bound = {worst[0]:.3f}, |lse - model| / bound = {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    paths = [[0, 1, 4], [0, 2, 5]]
    pa = attn.accept(pa, keep=torch.tensor(paths), n_q=7)
    assert pa[1].len == pa[3].len == 43 and pa[5] == L0 + 3
    # the twin: the path's tokens, one after the other (the causal limit alone is the path's mask)
    rows = torch.tensor([[L0 + i for i in p] for p in paths], device=DEV)
    take = lambda X: torch.stack([X[b][:, rows[b]] for b in range(B)])
    ql = torch.stack([q[b][:, torch.tensor(paths[b], device=DEV)] for b in range(B)])
    _, pb = attn.decode_multi(ql, take(K), take(V), mq._past(attn, K, V, L0))
    pb = attn.accept(pb)
    assert pb[1].len == 43 and pb[5] == pa[5]
    assert torch.equal(mq._bits(pa[1].view()), mq._bits(pb[1].view())) and torch.equal(mq._bits(pa[3].view()), mq._bits(pb[3].view()))
    nxt = (q[:, :, 7:].contiguous(), K[:, :, L0 + 7:], V[:, :, L0 + 7:])
    oa, la, pa = attn.decode_multi(*nxt, pa, return_lse=True)
    ob, lb, pb = attn.decode_multi(*nxt, pb, return_lse=True)
    assert torch.equal(mq._bits(oa), mq._bits(ob)) and torch.equal(mq._bits(la), mq._bits(lb))
    assert torch.isfinite(oa.float()).all() and torch.isfinite(la).all()


# ---- 5. sequences that accept different numbers of drafts -----------------------------------------------------------------------------------------
def _true_tokens_ratios(out, lse, q, Kp, Vp, first, groups, holes):
    """As the models of a call, sequence by sequence, on the rows that are no hole of the sequence (no mask: the holes are not there)."""
    r_out = r_lse = 0.0
    for b in range(q.shape[0]):
        for j in range(q.shape[2]):
            rows = [t for t in range(first + j + 1) if t not in holes[b]]
            r = mq._model_ratios(out[b:b + 1, :, j:j + 1], lse[b:b + 1, :, j:j + 1], q[b:b + 1, :, j:j + 1], Kp[b:b + 1][:, :, rows],
                                 Vp[b:b + 1][:, :, rows], len(rows) - 1, groups)
            r_out, r_lse = max(r_out, r[0]), max(r_lse, r[1])
    return r_out, r_lse


@pytest.mark.parametrize("kind", ["list", "arena", "inplace", "ext64"])
def test_sequences_that_accept_different_numbers_of_drafts(kind):
    """Four drafts per sequence over 256 compressed tokens and a window of 253 rows.  Sequence 0 accepts three, sequence 1 one: keep =
    [[0, 1, 2], [0, 1, 2]] keeps the batch rectangular, and rows 254 and 255 of sequence 1's window are holes the caller masks from then
    on.  Two calls of 16 tokens follow; the second ends on the trigger point, accept() compresses window rows 0 .. 255 -- the holes with
    them, columns 510 and 511 of the compressed part now -- and a call of two tokens follows over the new cache.  Every call's rows lie within
    the models' bounds evaluated on each sequence's true tokens only."""
    B, Hkv, groups, L0 = 2, 2, 4, 256 + 253
    attn = mq._attn(kind)
    Dd = attn.head_dim
    calls = [16, 16, 2]
    total = L0 + 3 + sum(calls)
    K, V, q = mq._rand(B, Hkv, total, groups, total - L0, Dd, seed=Dd + 43)     # the rows the cache ends up holding; q[:, :, i]: of row L0 + i
    Kd, Vd, qd = mq._rand(B, Hkv, 1, groups, 1, Dd, seed=Dd + 44)               # the fourth draft: rejected by both
    holes = [set(), {L0 + 1, L0 + 2}]
    past = mq._past(attn, K, V, L0)
    assert past[4] == 256 and past[1].len == 253
    o, l, past = attn.decode_multi(torch.cat([q[:, :, :3], qd], 2), torch.cat([K[:, :, L0:L0 + 3], Kd], 2), torch.cat([V[:, :, L0:L0 + 3], Vd], 2),
                                   past, return_lse=True)
    past = attn.accept(past, keep=torch.tensor([[0, 1, 2], [0, 1, 2]]), n_q=4)
    assert past[1].len == 256 and past[5] == L0 + 3
    n, worst = L0 + 3, [0.0, 0.0]
    for i, cnt in enumerate(calls):
        C = past[4]
        m = mm.zeros(B, 1, n + cnt)
        m[1, 0, sorted(holes[1])] = NEG
        qs = q[:, :, n - L0:n - L0 + cnt].contiguous()
        o, l, past = attn.decode_multi(qs, K[:, :, n:n + cnt], V[:, :, n:n + cnt], past, return_lse=True, attention_mask=mm.housed(m)[:, None])
        assert torch.isfinite(o.float()).all() and torch.isfinite(l).all()
        Kp, Vp = mq._pruned(attn, K, V, C)
        r = _true_tokens_ratios(o, l, qs, Kp, Vp, n, groups, holes)
        print(f"{kind} call {i} (C = {C}): |out - model| / bound = {r[0]:.3f}, |lse - model| / bound = {r[1]:.3f}")
        worst = [max(a, b) for a, b in zip(worst, r)]
        n += cnt
        due = attn.trigger_due(past)
        assert due == (i == 1)
        past = attn.accept(past)
        assert past[4] == (512 if i >= 1 else 256) and past[5] == n
    assert past[4] == 512 and max(holes[1]) < 512 and past[1].len == 34
    assert worst[0] <= 1.0 and worst[1] <= 1.0, f"{kind}: out {worst[0]:.3f}, lse {worst[1]:.3f}"


# ---- 6. split calls -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_ten_tokens_of_eight_heads_run_as_two_masked_calls(Dd):
    """groups = 8, n_q = 10: sub-calls of 8 and 2 tokens, each with its rows of mask (b) and the columns up to its last new row.  Within the
    bounds, and the bits of two explicit calls with the sliced masks."""
    B, Hkv, groups, n_q, L0 = 2, 2, 8, 10, 256 + 40
    attn = mq._attn("list", groups=groups, Dd=Dd)
    K, V, q = mq._rand(B, Hkv, L0 + n_q, groups, n_q, Dd, seed=Dd + 47)
    dev_mask = mm.housed(_mask_b(B, n_q, 256, 40, seed=Dd))[:, None]
    out, lse, new = attn.decode_multi(q, K[:, :, L0:], V[:, :, L0:], mq._past(attn, K, V, L0), return_lse=True, attention_mask=dev_mask)
    assert new[1].len == 50 and new[5] == L0 + n_q
    Kp, Vp = mq._pruned(attn, K, V, 256)
    mm.assert_models(out, lse, q, Kp, Vp, L0, groups, dev_mask, f"D={Dd} 8 + 2 tokens")
    past = mq._past(attn, K, V, L0)
    o1, l1, past = attn.decode_multi(q[:, :, :8].contiguous(), K[:, :, L0:L0 + 8], V[:, :, L0:L0 + 8], past, return_lse=True,
                                     attention_mask=dev_mask[:, :, :8, :L0 + 8])
    o2, l2, past = attn.decode_multi(q[:, :, 8:].contiguous(), K[:, :, L0 + 8:], V[:, :, L0 + 8:], past, return_lse=True,
                                     attention_mask=dev_mask[:, :, 8:])
    assert torch.equal(mq._bits(out), mq._bits(torch.cat([o1, o2], 2))) and torch.equal(mq._bits(lse), mq._bits(torch.cat([l1, l2], 2)))


# ---- 7. mustafar_window_keep_rows alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["reversed", "equal", "out-of-range"])
@pytest.mark.parametrize("n_keep", [1, 7, 64])
@pytest.mark.parametrize("Dd", [64, 128])
def test_window_keep_rows(pkg, Dd, n_keep, pattern):
    """n_rows = 64 rows from row 37 of windows of 128 rows holding random bits (NaN patterns among them), another index row per sequence.
    The destination rows are a gather of a copy taken before the call; every other row keeps its bits."""
    B, Hkv, cap, row0, n_rows = 2, 2, 128, 37, 64
    gen = torch.Generator(device=DEV).manual_seed(Dd + n_keep)
    wins = [torch.randint(-32768, 32768, (B, Hkv, cap, Dd), generator=gen, device=DEV, dtype=torch.int32).to(torch.int16) for _ in range(2)]
    before = [w.clone() for w in wins]
    if pattern == "reversed":
        keep = torch.stack([torch.arange(63, 63 - n_keep, -1), torch.arange(n_keep - 1, -1, -1)])
    elif pattern == "equal":
        keep = torch.stack([torch.full((n_keep,), 5), torch.full((n_keep,), 63)])
    else:
        keep = torch.stack([torch.tensor(([-3, 99, 64, -1, 0, 63, 17] * 10)[:n_keep]), torch.tensor(([99, -3, 2 ** 31 - 1, -2 ** 31] * 16)[:n_keep])])
    idx = keep.to(device=DEV, dtype=torch.int32).contiguous()
    err = pkg[0].mustafar_window_keep_rows(torch.cuda.current_stream().cuda_stream, wins[0].data_ptr(), wins[1].data_ptr(), B * Hkv, Hkv, cap,
                                           Dd, row0, n_rows, idx.data_ptr(), n_keep)
    assert err == 0
    src = keep.clamp(0, n_rows - 1).to(DEV) + row0
    for w, old in zip(wins, before):
        want = old.clone()
        for b in range(B):
            want[b, :, row0:row0 + n_keep] = old[b][:, src[b]]
        assert torch.equal(w, want)


# ---- 8. a fully masked row ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dd", [64, 128])
def test_a_row_whose_every_visible_column_is_masked(pkg, Dd):
    """Token 2 of sequence 1: finfo.min on every column.  The clamp leaves its x within a rounding of finfo.min and of each other, so the
    row returns, finite, about the mean of the V rows it sees: within the model's bound.  Token 1 of sequence 0: -inf on every column,
    which the clamp turns into finfo.min exactly -- every e is 1, the row returns the mean (without the clamp it would see nothing: 0 / 0)."""
    B, Hkv, groups, n_q, C, w0 = 2, 2, 4, 4, 64, 10
    K, V, q = mq._rand(B, Hkv, C + w0 + n_q, groups, n_q, Dd, seed=Dd + 53)
    c = mq.Call(pkg, K, V, C, n_q, groups)
    m = mm.zeros(B, n_q, C + w0 + n_q)
    m[1, 2] = NEG
    m[0, 1] = float("-inf")
    dev_mask = mm.housed(m)
    out, lse = mm.call_masked(c, q, dev_mask, Hkv)
    mm.assert_models(out, lse, q, c.Kp, c.Vp, C + w0, groups, mm.per_head(dev_mask, B, Hkv * groups, groups * Hkv), f"D={Dd}")
    gone = torch.zeros((B, n_q), dtype=torch.bool, device=DEV)
    gone[1, 2] = gone[0, 1] = True
    assert (lse.transpose(1, 2)[gone] < -65000).all() and (lse.transpose(1, 2)[~gone] > -100).all()
    seen = C + w0 + 2                                      # token 1 sees the old rows and new rows 0 and 1
    mean = c.Vp[0, :, :seen].double().mean(1)              # [Hkv, D]
    got = out[0, :, 1].double().reshape(Hkv, groups, Dd)
    assert ((got - mean[:, None]).abs() <= 2.0 ** -11 * mean[:, None].abs() + 2.0 ** -16).all()
