"""CPU: the helpers of tests/exact_data.py do what the GPU tests built on them assume -- dyadic sums are exact in any order, the
oracle's two SpMVs reproduce them, needles survive the prune and decide the output, the float64 hook model agrees with dense
attention where both apply, and a needle checker sees one token moved (negative control)."""
import math

import numpy as np
import pytest
import torch

from oracle import dense_ref
from oracle import oracle as orc
from tests import exact_data as xd


def test_dyadic_sums_are_exact_in_any_order():
    rng = np.random.default_rng(1)
    a = xd.dyadic(rng, (64, 128), 5, 4)
    b = xd.dyadic(rng, (128, 64), 5, 4)
    xd.assert_exact_budget(xd.units(a, 4), xd.units(b, 4))
    exact = a.astype(np.float64) @ b.astype(np.float64)
    prods = a.astype(np.float32)[:, :, None] * b.astype(np.float32)[None]           # [64, 128, 64], every product exact in fp32
    fwd = np.zeros((64, 64), np.float32)
    rev = np.zeros((64, 64), np.float32)
    for k in range(128):
        fwd += prods[:, k]
        rev += prods[:, 127 - k]
    split = prods[:, 0::2].sum(1, dtype=np.float32) + prods[:, 1::2].sum(1, dtype=np.float32)
    for s in (fwd, rev, split):
        assert np.array_equal(s.astype(np.float64), exact)
    p = xd.dyadic_probs(rng, (4, 1024), 12, 15)
    assert p.max() <= 15 * 2.0 ** -12 and p.min() >= 0
    with pytest.raises(AssertionError, match="budget"):
        xd.assert_exact_budget(np.full((1, 4096), 2047), np.full((4096, 1), 2047))


@pytest.mark.parametrize("which", ["key", "value"])
def test_oracle_spmv_equals_the_exact_sums_on_dyadic_data(which):
    rng = np.random.default_rng(2)
    B, t, groups = 2, 256, 3
    x = orc.prune_magnitude(xd.dyadic(rng, (B, t, xd.D), 5, 4), 0.7)        # many ties: the prune rule keeps every tie
    conv = orc.convert_key_batched if which == "key" else orc.convert_value_batched
    bmp, idx, nzs = conv(x)
    off = orc.nz_offset_from_idx(idx)
    X = x.astype(np.float64)
    if which == "key":
        q = xd.dyadic(rng, (B * groups, 8, xd.D), 5, 4)
        C16, Cd = orc.key_spmv(bmp, np.concatenate(nzs), idx, off, q, t, xd.D, B * groups, groups)
        exact = np.stack([q[b].astype(np.float64) @ X[b // groups].T for b in range(B * groups)])
        for b in range(B * groups):
            xd.assert_exact_budget(xd.units(q[b], 4), xd.units(x[b // groups], 4).T)
    else:
        p = xd.dyadic_probs(rng, (B * groups, 8, t), 12, 15)
        C16, Cd = orc.value_spmv(bmp, np.concatenate(nzs), idx, off, p, xd.D, t, B * groups, groups)
        exact = np.stack([p[b].astype(np.float64) @ X[b // groups] for b in range(B * groups)])
        for b in range(B * groups):
            xd.assert_exact_budget(xd.units(p[b], 12), xd.units(x[b // groups], 4))
    assert np.array_equal(Cd, exact)
    assert np.array_equal(C16.astype(np.float64), exact.astype(np.float16).astype(np.float64))


@pytest.mark.parametrize("sparsity", [0.7, 0.8])
def test_needles_survive_the_prune_and_decide_the_output(sparsity):
    B, Hq, Hkv, L, C = 2, 16, 2, 700, 512
    rng = np.random.default_rng(3)
    pos1 = np.stack([rng.choice(L, 2, replace=False) for _ in range(B * Hq)]).reshape(B, Hq, 2)
    pos1[0, 0] = (0, L - 1)                               # token 0 and the step's new row on one head
    pos2 = rng.integers(0, L, (B, Hq))
    pos2[(pos2[..., None] == pos1).any(-1)] = -1
    K, V, q, _ = xd.needle_data(B, Hq, Hkv, L, pos1, pos2, k_sparsity=sparsity, seed=4)
    Kp, Vp = K.clone(), V.clone()
    Kp[:, :, :C] = torch.from_numpy(orc.prune_magnitude(K[:, :, :C].numpy(), sparsity))
    Vp[:, :, :C] = torch.from_numpy(orc.prune_magnitude(V[:, :, :C].numpy(), sparsity))
    g = Hq // Hkv
    s = torch.einsum("bkgd,bktd->bkgt", q.double().view(B, Hkv, g, xd.D), Kp.double()).reshape(B, Hq, L) / math.sqrt(xd.D)
    top = s.topk(3, -1)
    assert (top.values[..., 0] - top.values[..., 1] == 0).all(), "two equal needles: equal scores"
    assert (top.values[..., 1] - top.values[..., 2] > 39).all(), "the needles' gap to every other token"
    want = xd.needle_expect(V, pos1, C, sparsity, Hq)
    got = dense_ref.dense_decode_layer(q, Kp, Vp, g).double()     # fp32 softmax cast to fp16: p = 0.5, 0.5 and exact zeros
    assert torch.equal(got, want.double())
    masked = np.zeros((B, L), bool)
    masked[1, pos1[1, 3]] = True                           # both needles of (1, 3) masked: its secondary wins, if it has one
    if pos2[1, 3] >= 0 and not masked[1, pos2[1, 3]]:
        alt = xd.needle_expect(V, pos1, C, sparsity, Hq, pos2=pos2, masked=masked)
        Vr = (Vp[1, 3 // g, pos2[1, 3]]).double()
        assert torch.equal(alt[1, 3, 0].double(), Vr)


def test_model_agrees_with_dense_attention_on_flat_data():
    torch.manual_seed(5)
    B, Hq, Hkv, L = 2, 8, 2, 300
    K = torch.randn(B, Hkv, L, xd.D).half()
    V = torch.randn(B, Hkv, L, xd.D).half()
    q = torch.randn(B, Hq, 1, xd.D).half()
    out, bound = xd.hook_model(q, K, V, Hq // Hkv)
    dense = dense_ref.dense_decode_layer(q.double(), K.double(), V.double(), Hq // Hkv)
    scale = float(out.abs().max())
    # the model departs from dense float64 attention by the fp16 score roundings alone: inside the dense comparator's bar (tests/util.py)
    assert float((out - dense).abs().max()) <= 3 * 2.0 ** -11 * scale + 1e-4
    # and its bound is tight enough to mean something: a few fp16 ulps of the output scale on flat data (4.1 here)
    assert float(bound.max()) <= 6 * 2.0 ** -11 * scale, float(bound.max()) / (2.0 ** -11 * scale)
    # the unfused hook's arithmetic in fp32 (fp16 scores, fp32 softmax) sits inside the bound
    Kr, Vr = K.float().repeat_interleave(Hq // Hkv, 1), V.float().repeat_interleave(Hq // Hkv, 1)
    x = (torch.matmul(q.float(), Kr.transpose(2, 3)).half() / math.sqrt(xd.D)).float()
    hook = torch.matmul(torch.softmax(x, -1), Vr).half().double()
    assert ((hook - out).abs() <= bound).all()


def test_model_bound_holds_at_large_gaps():
    B, Hq, Hkv, L = 1, 4, 1, 512
    rng = np.random.default_rng(6)
    sink = rng.integers(0, L, (B, Hq))
    for gap in (6, 12, 20, 28):
        K, V, q = xd.sink_data(B, Hq, Hkv, L, gap, sink, seed=gap)
        out, bound = xd.hook_model(q, K, V, Hq // Hkv)
        Kr, Vr = K.float().repeat_interleave(Hq, 1), V.float().repeat_interleave(Hq, 1)
        x = (torch.matmul(q.float(), Kr.transpose(2, 3)).half() / math.sqrt(xd.D)).float()
        assert float((x.max(-1).values - x.median(-1).values).min()) > gap - 4, "the sink does not stand out"
        hook = torch.matmul(torch.softmax(x, -1), Vr).half().double()
        assert ((hook - out).abs() <= bound).all(), f"gap {gap}"


def test_a_needle_moved_by_one_token_fails_the_checker():
    """NEGATIVE CONTROL on the CPU: the output of a head whose needle is one token off differs from the expected row."""
    B, Hq, Hkv, L, C = 1, 8, 2, 400, 256
    pos1 = np.array([[0, 63, 64, 255, 256, 300, 398, 399]])
    K, V, q, _ = xd.needle_data(B, Hq, Hkv, L, pos1, seed=7)
    want = xd.needle_expect(V, pos1, C, 0.7, Hq)
    shifted = xd.needle_expect(V, pos1 + np.array([[1, 0, 0, 0, 0, 0, 0, 0]]), C, 0.7, Hq)
    miss = xd.needle_misses(shifted, want)
    assert miss[0, 0] and not miss[0, 1:].any()
    assert not xd.needle_misses(want, want).any()
