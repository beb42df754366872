"""Test data whose correct output is known EXACTLY (a plain helper module of the suite, not a conftest).

Two kinds:

* Dyadic data -- small integers times powers of two.  Every product of two such fp16 values is exact in fp32, and so is every
  partial sum as long as the largest possible partial sum stays under 2^24 units of the product's least bit.  Then the order
  of the summation does not matter, the fp32 result is the exact result, its fp16 rounding is unique, and a kernel's fp16
  output must equal the oracle's bit for bit (`assert_exact_budget` checks the budget of a given pair of operands).

* Needles -- K, V and q such that q head h of batch entry b attends to ONE token (or to n tokens of equal score, n a power
  of two).  Key rows are small noise (|k| <= 1, multiples of 1/4); a needle row holds A1 = 16 on a slot of SLOT = 8
  channels, the query of its head holds QB = 8 on the same slot and zero elsewhere.  The slots of the heads of one kv head
  are disjoint (16 slots of 8 channels: up to 16 heads per kv head).  Scores: needle 16*8*8 = 1024, x = 1024/sqrt(128) = 90.5;
  a secondary needle (A2 = 8) 512, x = 45.3; any other row at most 8*8*1 = 64, x <= 5.7.  Both gaps are above 39, so
  exp(-gap) < 2^-56: in fp16 every e value but the winner's is exactly 0, in fp32 every weight of another token or slab is
  below half an ulp of anything it is added to, and the dot2 engine's 2^15 scale of e = 1 is exact.  The output of a head is
  then the V row of its needle exactly -- the pruned row when the token is in the compressed part, the raw row in the window --
  and the mean of n rows (n = 2, 4) exactly, because V holds multiples of 2^-5 with |v| <= 2 (v / n, and every partial sum,
  are fp16 numbers).  The prune keeps a needle's slot: the builder prunes every needle row with the oracle's rule and checks.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import oracle as orc

D = 128
SLOT = 8                  # channels per needle slot: D // SLOT = 16 disjoint slots per kv head
A1, A2, QB = 16.0, 8.0, 8.0
FP32_UNITS = 2 ** 24      # an integer below this is exact in fp32


# ---- dyadic data -------------------------------------------------------------------------------------------------------------------
def dyadic(rng: np.random.Generator, shape, bits: int, exp: int) -> np.ndarray:
    """fp16 array of integers in [-(2^bits - 1), 2^bits - 1] times 2^-exp (every value exact in fp16: bits <= 11, and the
    smallest non-zero value 2^-exp is a normal fp16 number: exp <= 14)."""
    assert 1 <= bits <= 11 and 0 <= exp <= 14
    n = rng.integers(-(2 ** bits - 1), 2 ** bits, size=shape)
    x = (n * 2.0 ** -exp).astype(np.float16)
    assert np.array_equal(x.astype(np.float64) * 2.0 ** exp, n.astype(np.float64))
    return x


def dyadic_probs(rng: np.random.Generator, shape, m: int, jmax: int) -> np.ndarray:
    """fp16 probabilities j * 2^-m, j uniform in [0, jmax] (exact: jmax < 2^11, m <= 24 keeps j * 2^-m an fp16 number)."""
    assert 0 < jmax < 2 ** 11 and jmax * 2.0 ** -m <= 1.0
    j = rng.integers(0, jmax + 1, size=shape)
    p = (j * 2.0 ** -m).astype(np.float16)
    assert np.array_equal(p.astype(np.float64) * 2.0 ** m, j.astype(np.float64))
    return p


def units(x: np.ndarray, exp: int) -> np.ndarray:
    """The integers behind a dyadic array (x * 2^exp), checked to be integers."""
    n = x.astype(np.float64) * 2.0 ** exp
    assert np.array_equal(n, np.round(n)), "not a dyadic array of this exponent"
    return n.astype(np.int64)


def assert_exact_budget(a_units: np.ndarray, b_units: np.ndarray) -> int:
    """a [..., M, K] x b [..., K, N] in integer units: the largest sum of |products| of any output must stay under 2^24, so
    that every partial sum, in any order and any split, is exact in fp32.  Returns that largest sum."""
    worst = int((np.abs(a_units).astype(np.int64) @ np.abs(b_units).astype(np.int64)).max()) if a_units.size and b_units.size else 0
    assert worst < FP32_UNITS, f"dyadic data outside the fp32-exact budget: a partial sum may reach {worst} units (>= 2^24)"
    return worst


# ---- needles --------------------------------------------------------------------------------------------------------------------
def edge_positions(C: int, L: int, block: int = 64) -> list:
    """The positions where an address computation goes wrong first, for a step that attends to L tokens of which the first C
    are compressed: token 0, the first and last token of every `block`-token block (64: every 256-token super-block edge among
    them), T - 1 and T (the last compressed token and the first window row), and the last two rows (the last window row before
    the step, and the step's new k / v)."""
    pos = {0, L - 1, L - 2}
    for b in range(0, C, block):
        pos.update((b, b + block - 1))
    if C:
        pos.update((C - 1, C))
    return sorted(p for p in pos if 0 <= p < L)


def assign_rows(positions, B: int, Hq: int, rng: np.random.Generator, L: int) -> list:
    """Spread `positions` over the B x Hq rows of one or more calls: returns a list of [B, Hq] int64 arrays (one per call),
    every position the target of some row; rows left over get random positions."""
    rows = B * Hq
    calls = []
    for i in range(0, max(len(positions), 1), rows):
        chunk = np.asarray(positions[i:i + rows], np.int64)
        fill = rng.integers(0, L, size=rows - len(chunk))
        calls.append(np.concatenate([chunk, fill]).reshape(B, Hq))
    return calls


def needle_data(B: int, Hq: int, Hkv: int, L: int, pos1: np.ndarray, pos2: np.ndarray = None, k_sparsity: float = 0.7,
                seed: int = 0, device="cpu", alt=()):
    """K, V [B, Hkv, L, D] and q [B, Hq, 1, D] (fp16, on `device`).  L counts every token of the step, its new row last.

    pos1 [B, Hq] or [B, Hq, n]: the needle(s) of each row at level A1 (n equal needles, n a power of two, distinct positions);
    pos2 [B, Hq] or None: a secondary needle at level A2 (-1: none) -- the winner once the primary ones are masked.
    alt: more [B, Hq] needle sets, each on slots of its own (set j: slot shift (j + 1) x groups); q ignores them, and the
    j-th of the returned `q_alt` queries selects them instead (steps that differ only in q).  Returns K, V, q, q_alt."""
    pos1 = np.asarray(pos1, np.int64)
    if pos1.ndim == 2:
        pos1 = pos1[..., None]
    n = pos1.shape[-1]
    assert pos1.shape[:2] == (B, Hq) and n & (n - 1) == 0 and (pos1 >= 0).all() and (pos1 < L).all()
    assert all(len(set(r)) == n for r in pos1.reshape(-1, n)), "a row's equal needles must sit on distinct tokens"
    g = Hq // Hkv
    assert (len(alt) + 1) * g <= D // SLOT, "more needle sets x heads per kv head than disjoint slots"
    gen = torch.Generator(device=device).manual_seed(seed)
    K = (torch.randint(-4, 5, (B, Hkv, L, D), generator=gen, device=device).to(torch.float16) * 0.25)
    V = (torch.randint(-64, 65, (B, Hkv, L, D), generator=gen, device=device).to(torch.float16) * 2.0 ** -5)
    bb, hh = np.meshgrid(np.arange(B), np.arange(Hq), indexing="ij")
    kv = hh // g
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    placed = []

    def channels(shift):
        return ((hh % g + shift) % (D // SLOT))[..., None] * SLOT + np.arange(SLOT)     # [B, Hq, SLOT]: disjoint within a kv head

    def put(pos, level, ch):
        pos = np.asarray(pos, np.int64)
        assert ((pos < L)).all()
        sel = np.broadcast_to(pos[..., None], ch.shape) >= 0
        idx = [np.broadcast_to(a, ch.shape)[sel] for a in (bb[..., None], kv[..., None], pos[..., None], ch)]
        K[tuple(T(a) for a in idx)] = level
        placed.append((pos, level, ch))

    def query(ch):
        qq = torch.zeros((B, Hq, 1, D), dtype=torch.float16, device=device)
        qq[T(np.broadcast_to(bb[..., None], ch.shape)), T(np.broadcast_to(hh[..., None], ch.shape)), 0, T(ch)] = QB
        return qq

    ch0 = channels(0)
    for j in range(n):
        put(pos1[..., j], A1, ch0)
    if pos2 is not None:
        pos2 = np.asarray(pos2, np.int64)
        assert ((pos2 < 0) | (pos2[..., None] != pos1).all(-1)).all()
        put(pos2, A2, ch0)
    q_alt = []
    for j, pa in enumerate(alt):
        ch = channels((j + 1) * g)
        put(pa, A1, ch)
        q_alt.append(query(ch))
    # the prune keeps every needle's slot: each needle row, pruned by the oracle's rule, still holds its level there
    for pos, level, ch in placed:
        m = pos >= 0
        rows = K[T(bb[m]), T(kv[m]), T(pos[m])].cpu().numpy()
        kept = orc.prune_magnitude(rows, k_sparsity)
        assert (np.take_along_axis(kept, ch[m], 1) == level).all(), "a needle slot does not survive the prune"
    return K, V, query(ch0), q_alt


def needle_expect(V: torch.Tensor, pos1: np.ndarray, C: int, v_sparsity: float, Hq: int, pos2: np.ndarray = None,
                  masked: np.ndarray = None) -> torch.Tensor:
    """The exact output [B, Hq, 1, D] fp16 of a needle step: the (mean of the) V row(s) of the winning needle(s) of each row,
    pruned by the oracle's rule where the token is one of the first C (compressed) ones.  masked [B, L] bool: tokens masked
    with finfo.min for every head of that batch entry."""
    pos1 = np.asarray(pos1, np.int64)
    if pos1.ndim == 2:
        pos1 = pos1[..., None]
    B, Hkv, L, _ = V.shape
    g = Hq // Hkv
    Vh = V.cpu().numpy()
    out = np.zeros((B, Hq, D), np.float64)
    for b in range(B):
        for h in range(Hq):
            win = [int(t) for t in pos1[b, h] if masked is None or not masked[b, t]]
            if not win:
                assert pos2 is not None and pos2[b, h] >= 0 and (masked is None or not masked[b, pos2[b, h]]), "no unmasked needle left"
                win = [int(pos2[b, h])]
            assert len(win) & (len(win) - 1) == 0, "a mean over a non-power-of-two count is not exact"
            rows = np.stack([Vh[b, h // g, t] for t in win])
            comp = np.array([t < C for t in win])
            if comp.any():
                rows[comp] = orc.prune_magnitude(rows[comp], v_sparsity)
            out[b, h] = rows.astype(np.float64).mean(0)
    want = out.astype(np.float16)
    assert np.array_equal(want.astype(np.float64), out), "the expected mean is not an fp16 number"
    return torch.from_numpy(want).view(B, Hq, 1, D).to(V.device)


def needle_misses(out: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """[B, Hq] bool: rows whose output is not bit-equal (as values: -0 == +0) to the expected one."""
    return (out.float() != want.float()).reshape(want.shape[0], want.shape[1], -1).any(-1)


# ---- float64 model of the hook's decode arithmetic on finite-gap data -------------------------------------------------------------
def hook_model(q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, groups: int, mask: torch.Tensor = None):
    """The fused decode's arithmetic in float64 for pruned-but-dense K / V (fp16, the step's new row last): returns (out, bound),
    both float64 [B, Hq, 1, D]: |kernel - out| <= bound must hold element by element.  mask: None, or an additive fp16 mask that
    broadcasts to [B, Hq, 1, L], applied as the hook does (model :293-301) -- max(fp16(x + m), finfo(fp16).min), an fp16 addition --
    to EVERY candidate x below, so that [x_lo, x_hi] still holds every x the kernels can form.

    The roundings that happen, and what each contributes:
      * the score s = q . k is an fp32 sum of exact fp16 products, stored as fp16.  fp32 accumulation in any order stays within
        a = 128 * 2^-24 * sum|q k| of the exact s, so the stored score is fp16(s') for some s' in [s - a, s + a]: one of at most
        two neighbouring fp16 numbers.  The model takes both.
      * x = fp16(fp16(s) / sqrt(d)): the reference divides (an fp16 tensor by a Python float); the kernels multiply by the fp32
        1/sqrt(d) (spmv.hip: scaled()), which can differ by one fp32 ulp before the fp16 rounding and so by one fp16 ulp of x.
        The model carries both, the quotient and the product, for both score candidates: [x_lo, x_hi] holds every x the
        kernels can form; the model's own x is the quotient of the nearest rounding.  dx = x_hi - x_lo per token.
      * e = exp(x - m) in fp32: a change of the max m scales every e alike and cancels in the normalisation; a token's own
        ambiguity moves its e by at most e * dx (first order: dx < 2^-5 wherever e is not negligible).  e is stored as fp16 by the one-pass forms: 2^-11 relative, or
        the subnormal quantum 2^-25 absolute for the valu engine (the dot2 engine scales by 2^15 first: smaller).
      * p . V and sum e in fp32: 2^-22 relative of sum e |v| (a few hundred fp32 ulps of slack); the final fp16 rounding: 2^-11
        of |out|, and 2^-25 (half the smallest fp16 step) absolute.
    A change de_t of one e moves out = sum e v / sum e by de_t (v_t - out) / sum e, so
    bound = sum_t |de_t| |v_t - out| / sum e + 2^-22 sum e |v| / sum e + 2^-11 |out| + 2^-25."""
    B, Hkv, L, Dd = K.shape
    Hq = q.shape[1]
    rs = math.sqrt(Dd)
    inv = torch.tensor(1.0 / rs, dtype=torch.float32, device=K.device)
    outs, bounds = [], []
    for b in range(B):                                   # one batch entry at a time bounds the float64 temporaries
        qd = q[b].double().reshape(Hkv, groups, Dd)
        Kd, Vd = K[b].double(), V[b].double()
        s = torch.einsum("kgd,ktd->kgt", qd, Kd)
        acc = 128 * 2.0 ** -24 * torch.einsum("kgd,ktd->kgt", qd.abs(), Kd.abs())
        cands = [(s - acc).half().double(), (s + acc).half().double(), s.half().double()]
        xs = [f(c) for c in cands for f in (lambda c: (c / rs).half().double(), lambda c: (c.float() * inv).half().double())]
        if mask is not None:
            mb = mask[b].to(torch.float16).expand(Hq, 1, L).reshape(Hkv, groups, L)
            xs = [torch.clamp(c.half() + mb, min=torch.finfo(torch.float16).min).double() for c in xs]
        x = xs[4]                                        # the quotient of the nearest rounding: the reference's x
        lo, hi = torch.stack(xs).amin(0), torch.stack(xs).amax(0)
        dx = hi - lo
        m = x.amax(-1, keepdim=True)
        e = torch.exp(x - m)
        l = e.sum(-1, keepdim=True)
        out = torch.einsum("kgt,ktd->kgd", e, Vd) / l
        de = e * (dx + 2.0 ** -11) + 2.0 ** -25
        dev = torch.stack([torch.einsum("gt,gtd->gd", de[k], (Vd[k].unsqueeze(0) - out[k].unsqueeze(1)).abs()) for k in range(Hkv)]) / l
        fp32 = 2.0 ** -22 * torch.einsum("kgt,ktd->kgd", e, Vd.abs()) / l
        outs.append(out.reshape(Hq, 1, Dd))
        bounds.append((dev + fp32 + 2.0 ** -11 * out.abs() + 2.0 ** -25).reshape(Hq, 1, Dd))
    return torch.stack(outs), torch.stack(bounds)


def model_ok(out, q, K, V, C, groups, pads=None, k_sparsity: float = 0.7, v_sparsity: float = 0.7, mask=None, pruned=None):
    """|fused - float64 model of the hook's arithmetic| within the model's bound, element by element (hook_model), over K / V whose first
    C tokens are pruned by the oracle's rule at k_sparsity / v_sparsity.  This, not the dense comparator, holds the random-data steps:
    tests/util.py's DENSE_ULPS bar is statistical (3 fp16 ulps of the output scale) and 32 rows x 128 channels of group count 8 exceed it
    by up to 1.3x on correct outputs, where the model's bound -- what the roundings of each element allow -- holds.  pads: left padding
    per batch entry, or per batch entry and q head ([B][Hq]: one model per head, groups = 1) (masked columns dropped).  mask: a finite
    additive fp16 mask broadcasting to [B, Hq, 1, L] (hook_model).  pruned: (Kp, Vp), the first C rows already pruned by the oracle."""
    Kp, Vp = K.clone(), V.clone()
    if pruned is not None:
        Kp[:, :, :C], Vp[:, :, :C] = pruned
    else:
        Kp[:, :, :C] = torch.from_numpy(orc.prune_magnitude(K[:, :, :C].cpu().numpy(), k_sparsity)).to(K.device)
        Vp[:, :, :C] = torch.from_numpy(orc.prune_magnitude(V[:, :, :C].cpu().numpy(), v_sparsity)).to(V.device)
    Hq = q.shape[1]
    for b in range(out.shape[0]):
        p = pads[b] if pads else 0
        if isinstance(p, (list, tuple)):
            assert len(p) == Hq
            units = [(slice(h, h + 1), slice(h // groups, h // groups + 1), int(p[h]), 1) for h in range(Hq)]
        else:
            units = [(slice(None), slice(None), int(p), groups)]
        for hs, ks, pp, g in units:
            mb = None if mask is None else mask[b:b + 1].expand(1, Hq, 1, K.shape[2])[:, hs, :, pp:]
            want, bound = hook_model(q[b:b + 1, hs], Kp[b:b + 1, ks, pp:], Vp[b:b + 1, ks, pp:], g, mask=mb)
            ratio = float(((out[b:b + 1, hs].double() - want).abs() / bound).max())
            assert ratio <= 1.0, f"batch {b} heads {hs}: |fused - model| / bound = {ratio:.3f} (sparsity K {k_sparsity}, V {v_sparsity})"


def sink_data(B: int, Hq: int, Hkv: int, L: int, gap: float, sink: np.ndarray, seed: int = 0, device="cpu", outliers: int = 4):
    """Finite-gap ("attention sink") data: N(0,1)-like dyadic K / V / q (multiples of 2^-6, |.| < 2), K with `outliers` channels
    scaled by 16 as real key caches have (their q entries scaled by 1/16: the scores stay O(1)), and token sink[b, h] of each row
    lifted by `gap` logits above the flat rest (its K row gets q_h's direction).  Returns K, V, q fp16 on `device`."""
    gen = torch.Generator(device=device).manual_seed(seed)
    r = lambda shape: (torch.randn(shape, generator=gen, device=device) * 64).round().clamp(-127, 127) / 64
    K, V, q = r((B, Hkv, L, D)), r((B, Hkv, L, D)), r((B, Hq, 1, D))
    out_ch = torch.arange(outliers, device=device) * (D // outliers) + 3
    K[..., out_ch] *= 16
    q[..., out_ch] /= 16
    g = Hq // Hkv
    for b in range(B):
        for h in range(Hq):
            t = int(sink[b, h])
            qq = q[b, h, 0]
            # raise the score of token t by gap * sqrt(D) along q's direction (rounded to multiples of 2^-6)
            K[b, h // g, t] += (qq * (gap * math.sqrt(D) / float(qq.double().pow(2).sum()))).mul(64).round() / 64
    return K.half(), V.half(), q.half()
