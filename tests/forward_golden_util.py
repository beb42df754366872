"""Runs recorded from the reference's own decode forward (a plain helper module of the suite, not a conftest).

`oracle/gen_golden.py: gen_forward()` executes `LlamaFlashAttention_MUSTAFAR.forward` (models/llama_mustafar_kernel.py:199-457)
unchanged, on CPU, with stand-ins for what it imports, and writes one `tests/golden/forward_<name>.npz` per scenario below.  This
module holds what the generator and the tests share: the scenarios, the integer generator of their inputs, the loader with its
bookkeeping check, the dense K / V of a step, the float64 model with the bound of the reference's unfused arithmetic, and `within`.

A fixture holds (R = recorded steps, S = snapshots; every fp16 array as uint16 bits):
    meta                       JSON: the scenario, the seed and checksum of its inputs, what the reference did ("ran", or the type name
                               of the exception it raised and the step that raised it), the snapshot labels, the operator call log
    mask                       [bsz, 1, 1, L0 + steps] additive fp16 mask (step i reads its first L0 + i + 1 columns); absent without one
    out                        [R, bsz, Hq * D]   attn_output of every step
    compressed_length, window_len, kv_seq_len    [R + 1] int32: entry 0 after the prefill, entry i + 1 after step i
    snap_after                 [S] int32: -1 after the prefill, i after step i (every trigger step, and the last step)
    snap<j>_{k,v}_{bmp,idx,nz,nz_offset}, snap<j>_{k,v}_win     the caches (nz: the per-head streams concatenated) and both windows; a cache
                               that repeats an earlier snapshot's word for word is stored once (meta: same_cache); nz and windows are
                               stored as int8 codes c (value c / 64: the data is dyadic) and come back from snapshot() as fp16 bits
    log_{key,value}_{b,sum,abs}   the last step's operator calls: row 0 of the 8-row operand (rows 1-7 were zero: meta says so), row 0's
                               float64 sums and sum |terms|; the cache operands are those of the last snapshot
"""
from __future__ import annotations

import json
import math
import os
import zlib

import numpy as np
import torch

from oracle import oracle as orc
from tests.exact_data import hook_model

RESIDUAL = 32            # residual_length of every scenario (mem_spd_test.py:9)
K_SPARSITY = 0.7
V_SPARSITY = 0.5         # unequal: a K / V mix-up in the recorded caches cannot pass
MAX_FIXTURE_BYTES = 704326

# name -> geometry.  mask: None | "mixed" (entry 0: finite biases on columns of the compressed part and of the window; entry 1:
# finfo.min on the first 270 columns, i.e. the compressed part and 14 window rows)
SCENARIOS = {
    "append": dict(D=128, bsz=1, Hq=6, Hkv=3, L0=538, steps=8, seed=101, mask=None),
    "first":  dict(D=128, bsz=2, Hq=2, Hkv=2, L0=282, steps=9, seed=102, mask=None),
    "mask":   dict(D=128, bsz=2, Hq=8, Hkv=2, L0=300, steps=4, seed=103, mask="mixed"),
    "d64":    dict(D=64,  bsz=2, Hq=8, Hkv=2, L0=538, steps=8, seed=104, mask=None),
    "short":  dict(D=128, bsz=1, Hq=1, Hkv=1, L0=30,  steps=2, seed=105, mask=None),
}


# ---- inputs: a small integer generator ------------------------------------------------------------------------------------------------
def _splitmix64(idx: np.ndarray, seed: int) -> np.ndarray:
    """splitmix64 of seed + idx: 64 well-mixed bits per index, the same on every numpy."""
    with np.errstate(over="ignore"):
        z = idx.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dyadic_codes(seed: int, n: int) -> np.ndarray:
    """n int64 codes c, |c| <= 127, roughly N(0, 64^2): the sum of four bytes of a splitmix64 word, centred and scaled by 111/256
    (four uniform bytes have deviation 147.8; x 111/256 = 64.1).  x = c / 64 is the N(0,1)-like dyadic fp16 data of
    exact_data.sink_data: multiples of 2^-6 with |x| < 2."""
    z = _splitmix64(np.arange(n, dtype=np.uint64), seed)
    s = sum(((z >> np.uint64(8 * i)) & np.uint64(0xFF)).astype(np.int64) for i in range(4)) - 510
    return np.clip((s * 111) // 256, -127, 127)


def scenario_inputs(spec: dict):
    """-> (q [steps, bsz, Hq, D], K [bsz, Hkv, L0 + steps, D], V likewise: fp16 numpy; checksum: crc32 of the int8 codes).  Row L0 + i of
    K / V is the new token of step i."""
    D, bsz, Hq, Hkv, L, steps = spec["D"], spec["bsz"], spec["Hq"], spec["Hkv"], spec["L0"] + spec["steps"], spec["steps"]
    nq, nk = steps * bsz * Hq * D, bsz * Hkv * L * D
    c = dyadic_codes(spec["seed"], nq + 2 * nk)
    f = lambda a, shape: (a.astype(np.float64) / 64).astype(np.float16).reshape(shape)
    q, K, V = f(c[:nq], (steps, bsz, Hq, D)), f(c[nq:nq + nk], (bsz, Hkv, L, D)), f(c[nq + nk:], (bsz, Hkv, L, D))
    return q, K, V, zlib.crc32(c.astype(np.int8).tobytes())


def scenario_mask(spec: dict):
    """The additive mask of a scenario [bsz, 1, 1, L0 + steps] fp16, or None."""
    if spec["mask"] is None:
        return None
    assert spec["mask"] == "mixed" and spec["bsz"] == 2
    L, C0 = spec["L0"] + spec["steps"], ((spec["L0"] - RESIDUAL) // 256) * 256
    m = np.zeros((2, 1, 1, L), np.float16)
    assert 0 < C0 and C0 + 20 < spec["L0"]
    for col, bias in ((3, -1.5), (64, -8.0), (C0 - 1, -1.5), (C0, -8.0), (C0 + 9, -1.5), (spec["L0"] - 1, -0.75)):
        m[0, 0, 0, col] = bias                       # compressed columns, the first window rows, the last prefill row
    m[1, 0, 0, :270] = np.finfo(np.float16).min
    return m


def bits_of_codes(c: np.ndarray) -> np.ndarray:
    """fp16 bits (uint16) of the dyadic values c / 64, c int8: how the streams and windows of a snapshot are stored (the generator checks
    that this gives back the recorded bits exactly)."""
    return (c.astype(np.float64) / 64).astype(np.float16).view(np.uint16)


# ---- bookkeeping: the closed form of model :324 and :416 ---------------------------------------------------------------------------------
def closed_form(L0: int, steps: int, residual: int = RESIDUAL):
    """(compressed_length, window_len, kv_seq_len), each [steps + 1], as the reference's forward leaves them: :416 after the prefill
    (floor division, unclamped: -256 for a prefill shorter than `residual`, with every row in the window), then per step kv += 1 and
    :324 / :398, unguarded."""
    C = ((L0 - residual) // 256) * 256
    cl, wl, kv = [C], [L0 - max(C, 0)], [L0]
    for i in range(steps):
        L = L0 + i + 1
        if (L - residual - C) % 256 == 0:
            C += 256
        cl.append(C), wl.append(L - max(C, 0)), kv.append(L)
    return np.array(cl, np.int32), np.array(wl, np.int32), np.array(kv, np.int32)


class Fixture:
    def __init__(self, name: str, arrays: dict):
        self.name = name
        self.a = arrays
        self.meta = json.loads(str(arrays["meta"]))
        self.spec = self.meta["spec"]
        self.recorded_steps = int(arrays["out"].shape[0])

    def __getitem__(self, key):
        return self.a[key]

    def snapshot(self, after: int) -> dict:
        """The caches and windows recorded after the prefill (-1) or after step `after`."""
        j = list(self.a["snap_after"]).index(after)
        take = lambda i, win: {k[len(f"snap{i}_"):]: v for k, v in self.a.items() if k.startswith(f"snap{i}_") and k.endswith("_win") == win}
        # (a snapshot whose cache repeats an earlier one word for word is stored as its windows and that snapshot's number)
        snap = {**take(self.meta["same_cache"].get(str(j), j), False), **take(j, True)}
        return {k: bits_of_codes(v) if v.dtype == np.int8 else v for k, v in snap.items()}

    def inputs(self):
        """(q, K, V) torch fp16 on CPU, the checksum verified against the recording; mask (torch fp16) or None."""
        q, K, V, crc = scenario_inputs(self.spec)
        if crc != self.meta["input_crc32"]:
            raise ValueError(f"fixture {self.name}: the input generator no longer gives the recorded inputs (crc {crc} != {self.meta['input_crc32']})")
        m = torch.from_numpy(self.a["mask"].view(np.float16).copy()) if "mask" in self.a else None
        return torch.from_numpy(q), torch.from_numpy(K), torch.from_numpy(V), m


def validate(arrays: dict, spec: dict) -> None:
    """Refuse (ValueError) a recording whose per-step bookkeeping is not the closed form of :324 / :416 for its scenario."""
    R = arrays["out"].shape[0]
    cl, wl, kv = closed_form(spec["L0"], R)
    for key, want in (("compressed_length", cl), ("window_len", wl), ("kv_seq_len", kv)):
        got = np.asarray(arrays[key])
        if got.shape != want.shape or not np.array_equal(got, want):
            raise ValueError(f"recorded {key} {got.tolist()} is not the closed form {want.tolist()}")


def load(golden_dir: str, name: str) -> Fixture:
    path = os.path.join(golden_dir, f"forward_{name}.npz")
    with np.load(path) as z:
        fx = Fixture(name, {k: z[k] for k in z.files})
    if fx.spec != SCENARIOS[name]:
        raise ValueError(f"fixture {name} was recorded for {fx.spec}, the suite expects {SCENARIOS[name]}")
    validate(fx.a, fx.spec)
    return fx


# ---- the dense K / V of a step, the model and the bounds ------------------------------------------------------------------------------
_PRUNED = {}


def dense_kv(K: torch.Tensor, V: torch.Tensor, C: int, kv_seq_len: int):
    """Pruned-but-dense K / V [bsz, Hkv, kv_seq_len, D] of a step that attends to `kv_seq_len` tokens of which the first C are compressed:
    rows [0, C) pruned by the oracle's rule at K_SPARSITY / V_SPARSITY, the rest raw.  (The pruned rows are computed once per tensor.)"""
    key = (K.data_ptr(), V.data_ptr(), C)
    if key not in _PRUNED:
        _PRUNED[key] = (torch.from_numpy(orc.prune_magnitude(K[:, :, :C].numpy(), K_SPARSITY)),
                        torch.from_numpy(orc.prune_magnitude(V[:, :, :C].numpy(), V_SPARSITY)), K, V)   # (K, V kept: the key is their address)
    Kp, Vp = K[:, :, :kv_seq_len].clone(), V[:, :, :kv_seq_len].clone()
    Kp[:, :, :C], Vp[:, :, :C] = _PRUNED[key][0], _PRUNED[key][1]
    return Kp, Vp


def reference_bound(q: torch.Tensor, Kp: torch.Tensor, Vp: torch.Tensor, C: int, groups: int, mask: torch.Tensor = None):
    """(model, hook_bound, reference_bound), float64 [bsz, Hq, 1, D]: exact_data.hook_model's output and bound for the step, and the bound of
    the reference's UNFUSED sequence (:270-320; `api="reference"` and `api="native"` issue the same operations), which is hook_model's
    bound plus the roundings that sequence adds.  With p_t the model's probabilities and v_t the V rows:

      * :304 stores the normalised probabilities as fp16 before p.V.  An fp16 rounding moves p_t by at most 2^-11 p_t, or by 2^-25 (half
        the subnormal step 2^-24) where p_t is subnormal; the output is sum_t p_t v_t with no renormalisation afterwards, so it moves by
        at most  sum_t (2^-11 p_t + 2^-25) |v_t|.
      * with a compressed part (C > 0) the output is fp16(fp16(c) + fp16(l)), c = sum_{t<C} p_t v_t from the value operator (:314-315),
        l = sum_{t>=C} p_t v_t from the window matmul (:316).  The last rounding is hook_model's own 2^-11 |out| + 2^-25.  The two
        partial roundings add 2^-11 |c| + 2^-25 and 2^-11 |l| + 2^-25, and |c| + |l| <= sum_t p_t |v_t| (to first order in the
        errors of p, the order hook_model itself works to):  2^-11 sum_t p_t |v_t| + 2^-24.
        Without one (C == 0: one matmul, :320) there is no partial rounding.

    The scores themselves are formed as hook_model says (fp32 sums of exact products stored as fp16, then the quotient by sqrt(d): the
    model's own x), so nothing is added for them.  No constant here is fitted to an output."""
    model, hb = hook_model(q, Kp, Vp, groups, mask=mask)
    bsz, Hkv, L, D = Kp.shape
    Hq = q.shape[1]
    rs = math.sqrt(D)
    s = torch.einsum("bkgd,bktd->bkgt", q.double().reshape(bsz, Hkv, groups, D), Kp.double())
    x = (s.half().double() / rs).half()                                      # the quotient of the nearest rounding (hook_model's x)
    if mask is not None:
        x = torch.clamp(x + mask.to(torch.float16).expand(bsz, Hq, 1, L).reshape(bsz, Hkv, groups, L), min=torch.finfo(torch.float16).min)
    p = torch.softmax(x.double(), -1)
    av = Vp.double().abs()
    extra = torch.einsum("bkgt,bktd->bkgd", 2.0 ** -11 * p + 2.0 ** -25, av)
    if C:
        extra = extra + 2.0 ** -11 * torch.einsum("bkgt,bktd->bkgd", p, av) + 2.0 ** -24
    return model, hb, hb + extra.reshape(bsz, Hq, 1, D)


def within(out, rec, bound_out, bound_rec, model):
    """`out` (what is under test) against the float64 `model` and the recording `rec`, element by element:
    |out - model| <= bound_out and |out - rec| <= bound_out + bound_rec (the recording lies within bound_rec of the model).
    Returns (ok, worst |out - model| / bound_out, worst |out - rec| / (bound_out + bound_rec)); a non-finite value is never ok."""
    f = lambda a: torch.as_tensor(a).detach().cpu().double().reshape(model.shape)
    o, r = f(out), f(rec)
    rm = ((o - model).abs() / bound_out).max().item()
    rr = ((o - r).abs() / (bound_out + bound_rec)).max().item()
    ok = bool(torch.isfinite(o).all()) and math.isfinite(rm) and math.isfinite(rr) and rm <= 1.0 and rr <= 1.0
    return ok, rm, rr


_STEPS = {}


def step_model(fx: Fixture, i: int, C: int = None) -> dict:
    """Everything a test needs of step i of a fixture, computed once and shared: q [bsz, Hq, 1, D], the step's new k / v rows, the mask
    columns the step reads, C (the compressed length BEFORE the step: the recorded one unless given), kv_seq_len, the float64 model with
    hook_model's bound and the reference's, and the recorded output (None past the recording)."""
    key = (fx.name, i, C)
    if key not in _STEPS:
        if "_inputs" not in fx.__dict__:
            fx._inputs = fx.inputs()
        q, K, V, m = fx._inputs
        s = fx.spec
        kv = s["L0"] + i + 1
        c = int(fx["compressed_length"][i]) if C is None else C
        qi = q[i].reshape(s["bsz"], s["Hq"], 1, s["D"])
        mi = m[..., :kv] if m is not None else None
        Kp, Vp = dense_kv(K, V, c, kv)
        model, hb, rb = reference_bound(qi, Kp, Vp, c, s["Hq"] // s["Hkv"], mi)
        rec = None
        if i < fx.recorded_steps:
            rec = torch.from_numpy(fx["out"][i].view(np.float16).copy()).reshape(s["bsz"], s["Hq"], 1, s["D"])
        _STEPS[key] = dict(q=qi, k=K[:, :, kv - 1:kv], v=V[:, :, kv - 1:kv], mask=mi, C=c, kv=kv, model=model, hook_bound=hb, ref_bound=rb, rec=rec)
    return _STEPS[key]
