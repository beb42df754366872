#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ FROM THE REFERENCE ITSELF.

Runs only in the build container (it reads /root/reference at run time; nothing from the
reference is copied into this repo -- only numeric inputs/outputs are saved):

  * prune_*.npz     : the reference's `dh_prune_key` / `dh_prune_value`
                      (models/llama_mustafar_kernel.py:77-153).  The module itself cannot be
                      imported (it needs the CUDA extension and transformers 4.43), so the two
                      function definitions are located with `ast` and executed with only
                      `torch` in scope, on CPU, in fp16.
  * compress_*.npz  : the reference's four Triton kernels (kernel/compression.py:8-247) run
                      under TRITON_INTERPRET=1 on CPU tensors.  The host wrappers
                      `convert_*_batched` assert `.is_cuda` (:251), so their torch glue
                      (:255-335) is restated below around the reference's own kernels.

  * forward_<scenario>.npz : the reference's decode forward itself (`LlamaFlashAttention_MUSTAFAR.forward`,
                      models/llama_mustafar_kernel.py:199-457), located with `ast` and executed unchanged on
                      CPU with stand-ins, all written here, for what it imports: a `self` whose projections
                      slice the hidden state and whose RoPE / o_proj are identities, `compression` built on
                      `reference_convert` (the reference's Triton kernels), and a numpy `mustafar_package`
                      that decodes the flat format from bmp / idx / nz_offset / the concatenated streams and
                      forms the sums in float64.  Scenarios, inputs and the file layout:
                      tests/forward_golden_util.py.  About 3 minutes for the five scenarios.

Usage:  python oracle/gen_golden.py                      (idempotent; seeds fixed)
        python oracle/gen_golden.py forward [scenario..] (the forward fixtures alone)
"""
import ast
import os
import sys

os.environ["TRITON_INTERPRET"] = "1"

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


# ----------------------------------------------------------------------------- prune
def load_reference_prune():
    src_path = os.path.join(REF, "models", "llama_mustafar_kernel.py")
    src = open(src_path).read()
    tree = ast.parse(src)
    fns = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in ("dh_prune_key", "dh_prune_value"):
            scope = {"torch": torch}
            exec(compile(ast.Module(body=[node], type_ignores=[]), src_path, "exec"), scope)
            fns[node.name] = scope[node.name]
    assert set(fns) == {"dh_prune_key", "dh_prune_value"}
    return fns


class _Self:
    k_sparsity = None
    v_sparsity = None


def gen_prune():
    fns = load_reference_prune()
    g = torch.Generator().manual_seed(1234)
    cases = {}
    for s in (0.5, 0.7, 0.8, 0.0, 0.99):
        x = torch.randn(1, 2, 24, 128, generator=g).to(torch.float16)
        cases[f"rand_s{s}"] = (x, s)
    # ties at the threshold: few distinct magnitudes, mixed signs
    x = (torch.randint(0, 6, (1, 1, 16, 128), generator=g).to(torch.float16) * 0.25)
    x = x * (torch.randint(0, 2, x.shape, generator=g).to(torch.float16) * 2 - 1)
    cases["ties_s0.7"] = (x, 0.7)
    cases["ties_s0.5"] = (x.clone(), 0.5)
    # zeros and negative zeros in the row; more zeros than the prune budget
    x = torch.randn(1, 1, 16, 128, generator=g).to(torch.float16)
    x[..., ::3] = 0.0
    x[..., 1::7] = -0.0
    cases["zeros_s0.7"] = (x, 0.7)
    x2 = torch.zeros(1, 1, 4, 128, dtype=torch.float16)
    x2[..., :10] = torch.randn(10, generator=g).to(torch.float16)
    cases["mostly_zero_s0.5"] = (x2, 0.5)
    # subnormals / large values
    x3 = torch.randn(1, 1, 8, 128, generator=g).to(torch.float16)
    x3[..., :32] *= 6e-5
    x3[..., 32:48] *= 1000
    cases["range_s0.8"] = (x3, 0.8)
    # head_dim 64 (format allows any D % 64 == 0)
    cases["d64_s0.7"] = (torch.randn(1, 2, 8, 64, generator=g).to(torch.float16), 0.7)

    out = {}
    for name, (x, s) in cases.items():
        yk = fns["dh_prune_key"](_Self(), x.clone(), s)
        yv = fns["dh_prune_value"](_Self(), x.clone(), s)
        assert torch.equal(yk.view(torch.int16), yv.view(torch.int16))
        out[f"{name}__x"] = x.numpy().view(np.uint16)
        out[f"{name}__y"] = yk.numpy().view(np.uint16)
        out[f"{name}__s"] = np.float64(s)
    np.savez_compressed(os.path.join(OUT, "prune_reference.npz"), **out)
    print("prune cases:", len(cases))


# ----------------------------------------------------------------------------- compression
def reference_convert(inputs: torch.Tensor, which: str):
    """Host glue of compression.py:249-339 / :341-432 on CPU around the reference's kernels."""
    sys.path.insert(0, REF)
    import kernel.compression as rc  # the reference module (Triton, interpreter mode)

    B, M, N = inputs.shape
    assert M % 64 == 0
    if which == "key":
        inputs_t = inputs.transpose(1, 2).contiguous()
        k_bitmap, k_pack = rc.calculate_bitmap_key_batched, rc.compress_key_batched
    else:
        inputs_t = inputs.contiguous()
        k_bitmap, k_pack = rc.calculate_bitmap_value_batched, rc.compress_value_batched
    tiles = (M * N) // 64
    bitmaps = torch.empty((B, tiles), dtype=torch.int64)
    counts = torch.empty((B, tiles), dtype=torch.int32)
    shifts_np = np.left_shift(np.int64(1), np.arange(63, -1, -1, dtype=np.int64))
    const_shifts = torch.tensor(shifts_np)
    grid = (tiles, B)
    stride_batch = tiles * 64
    k_bitmap[grid](inputs_t.view(-1), bitmaps.view(-1), counts.view(-1), total_elems=B * M * N,
                   shifts_ptr=const_shifts, stride_batch=stride_batch, M=M, N=N)
    accum = torch.cumsum(counts, dim=1).to(torch.int32)
    accum = torch.cat([torch.zeros((B, 1), dtype=counts.dtype), accum], dim=1).contiguous()
    total = 2 * accum[:, -1]
    offsets = torch.cumsum(total, dim=0)
    batch_offsets = torch.cat([torch.zeros(1, dtype=torch.int32), offsets[:-1]])
    packed = torch.zeros((int(offsets[-1].item()),), dtype=torch.float16)
    k_pack[grid](inputs_t.view(-1), bitmaps.view(-1), accum.view(-1), packed.view(-1), batch_offsets.view(-1),
                 total_elems=B * M * N, stride_batch=stride_batch, M=M, N=N)
    return bitmaps, accum, packed, batch_offsets.to(torch.int64)


def make_pruned(B, t, D, s, g, prune):
    x = torch.randn(1, B, t, D, generator=g).to(torch.float16)
    return prune(_Self(), x, s).reshape(B, t, D)


def gen_compress():
    prune = load_reference_prune()["dh_prune_key"]
    g = torch.Generator().manual_seed(4321)
    cases = {}
    for (B, t, s) in [(1, 64, 0.7), (2, 64, 0.5), (3, 64, 0.8), (2, 256, 0.7), (1, 512, 0.7), (2, 128, 0.0)]:
        cases[f"rand_B{B}_t{t}_s{s}"] = make_pruned(B, t, 128, s, g, prune)
    # edge tiles: all-zero tiles, full tiles (nnz = 64), nnz multiple of 8, -0.0 entries
    x = torch.zeros(2, 128, 128, dtype=torch.float16)
    dense = torch.randn(2, 128, 128, generator=g).to(torch.float16)
    dense[dense == 0] = 1.0
    x[0, :64, :] = dense[0, :64, :]                 # K: full tiles; V: full tiles
    x[0, 64:, 5] = dense[0, 64:, 5]                 # K: one full tile among empty ones
    x[1, 3, :] = dense[1, 3, :]                     # V: one token fully dense, rest empty
    x[1, 64:72, 64:72] = dense[1, 64:72, 64:72]     # nnz = 8 per touched tile
    x[1, 100, 0:16] = dense[1, 100, 0:16]           # V tile nnz = 16
    x[1, 80:96, 127] = dense[1, 80:96, 127]         # K tile nnz = 16
    x[1, 120, 64:] = -0.0                           # negative zeros must not set bits
    cases["edge_tiles"] = x
    # adversarial: every kept value in one 64-channel half
    y = torch.zeros(1, 64, 128, dtype=torch.float16)
    y[0, :, :40] = dense[0, :64, :40]
    cases["one_half"] = y
    # D = 64
    cases["d64"] = make_pruned(2, 64, 64, 0.7, g, prune)

    out = {}
    for name, x in cases.items():
        for which in ("key", "value"):
            bmp, accum, packed, boffs = reference_convert(x.clone(), which)
            out[f"{name}__{which}__bmp"] = bmp.numpy()
            out[f"{name}__{which}__accum"] = accum.numpy()
            out[f"{name}__{which}__packed"] = packed.numpy().view(np.uint16)
            out[f"{name}__{which}__batch_offsets"] = boffs.numpy()
        out[f"{name}__x"] = x.numpy().view(np.uint16)
        print("compress case", name, tuple(x.shape))
    np.savez_compressed(os.path.join(OUT, "compress_reference.npz"), **out)


# ----------------------------------------------------------------------------- decode forward
def load_reference_forward():
    """`LlamaFlashAttention_MUSTAFAR.forward` and the two prune methods, located with `ast` and compiled unchanged into a class whose
    every other attribute is a stand-in written here."""
    import math
    import warnings
    from typing import List, Optional, Tuple

    src_path = os.path.join(REF, "models", "llama_mustafar_kernel.py")
    tree = ast.parse(open(src_path).read())
    found = {}
    for cls in tree.body:
        if isinstance(cls, ast.ClassDef):
            for node in cls.body:
                if isinstance(node, ast.FunctionDef) and (
                        (cls.name == "LlamaFlashAttention_MUSTAFAR" and node.name == "forward")
                        or (cls.name == "LlamaAttention_MUSTAFAR" and node.name in ("dh_prune_key", "dh_prune_value"))):
                    found[node.name] = node
    assert set(found) == {"forward", "dh_prune_key", "dh_prune_value"}

    def repeat_kv(hidden_states, n_rep):   # transformers' repeat_kv, restated
        batch, heads, slen, head_dim = hidden_states.shape
        if n_rep == 1:
            return hidden_states
        return hidden_states[:, :, None, :, :].expand(batch, heads, n_rep, slen, head_dim).reshape(batch, heads * n_rep, slen, head_dim)

    scope = {"torch": torch, "F": torch.nn.functional, "nn": torch.nn, "math": math, "warnings": warnings, "List": List,
             "Optional": Optional, "Tuple": Tuple, "repeat_kv": repeat_kv,
             "apply_rotary_pos_emb": lambda q, k, cos, sin, position_ids=None: (q, k)}
    exec(compile(ast.Module(body=list(found.values()), type_ignores=[]), src_path, "exec"), scope)
    return scope, {n: scope[n] for n in found}


def _decode_flat(which, bmp, nz_flat, idx, nz_offset, heads, tokens, D):
    """Pruned-but-dense [heads, tokens, D] float64 from the FLAT reference format: head h's tile i holds its values from half
    8 * nz_offset[h] + 2 * idx[h][i] of the concatenated stream, one per set bit (element j <-> bit 63 - j).  Key tile = 64 tokens of
    one channel (tile id = tokblk * D + d); value tile = 64 channels of one token (tile id = (tokblk * (D / 64) + half) * 64 + r)."""
    tiles = tokens * D // 64
    bmp = np.asarray(bmp).reshape(heads, tiles).astype(np.uint64)
    idx = np.asarray(idx).reshape(heads, tiles + 1).astype(np.int64)
    nz = np.asarray(nz_flat, np.float16).reshape(-1)
    sh = np.arange(63, -1, -1, dtype=np.uint64)
    out = np.zeros((heads, tokens, D), np.float64)
    for h in range(heads):
        bits = ((bmp[h][:, None] >> sh[None, :]) & np.uint64(1)).astype(bool)
        src = 8 * int(nz_offset[h]) + 2 * idx[h, :-1, None] + np.cumsum(bits, 1) - 1
        dense = np.zeros((tiles, 64), np.float64)
        dense[bits] = nz[src[bits]].astype(np.float64)
        if which == "key":
            out[h] = dense.reshape(tokens // 64, D, 64).transpose(0, 2, 1).reshape(tokens, D)
        else:
            out[h] = dense.reshape(tokens // 64, D // 64, 64, 64).transpose(0, 2, 1, 3).reshape(tokens, D)
    return out


class OperatorRefused(ValueError):
    """The forward asked an operator stand-in for a product over a non-positive number of tokens."""


class _Operators:
    """Stand-in for `mustafar_package`: plain numpy over the flat format, float64 sums, fp16 results; every call is logged."""

    def __init__(self):
        self.calls = []
        self.step = None   # the decode step whose forward is running (set by the caller)

    def _log(self, name, tensors, scalars, b, x, terms_abs):
        self.calls.append(dict(name=name, step=self.step, shapes=[list(t.shape) for t in tensors], dtypes=[str(t.dtype) for t in tensors],
                               scalars=[int(s) for s in scalars], b=b.numpy().copy(), sum=x[:, 0].copy(), abs=terms_abs))

    def mustafar_key_formulation(self, bmp, nz, idx, nz_offset, B, M_Global, K_Global, Batch_Size, groups):
        if M_Global <= 0:
            raise OperatorRefused(f"mustafar_key_formulation called with compressed_length {M_Global}")
        heads = Batch_Size // groups
        Kd = _decode_flat("key", bmp.numpy(), nz.numpy(), idx.numpy(), nz_offset.numpy(), heads, M_Global, K_Global)
        Bd = B.numpy().astype(np.float64).reshape(heads, groups, -1, K_Global)
        x = np.einsum("hgnk,hmk->hgnm", Bd, Kd).reshape(Batch_Size, -1, M_Global)
        ab = np.einsum("hgk,hmk->hgm", np.abs(Bd[:, :, 0]), np.abs(Kd)).reshape(Batch_Size, M_Global)
        self._log("key", (bmp, nz, idx, nz_offset, B), (M_Global, K_Global, Batch_Size, groups), B, x, ab)
        return torch.from_numpy(x.astype(np.float16))

    def mustafar_value_formulation(self, bmp, nz, idx, nz_offset, B, ws, M_Global, K_Global, Batch_Size, groups):
        if K_Global <= 0:
            raise OperatorRefused(f"mustafar_value_formulation called with compressed_length {K_Global}")
        heads = Batch_Size // groups
        Vd = _decode_flat("value", bmp.numpy(), nz.numpy(), idx.numpy(), nz_offset.numpy(), heads, K_Global, M_Global)
        Bd = B.numpy().astype(np.float64).reshape(heads, groups, -1, K_Global)
        x = np.einsum("hgnk,hkm->hgnm", Bd, Vd).reshape(Batch_Size, -1, M_Global)
        ab = np.einsum("hgk,hkm->hgm", np.abs(Bd[:, :, 0]), np.abs(Vd)).reshape(Batch_Size, M_Global)
        self._log("value", (bmp, nz, idx, nz_offset, B), (M_Global, K_Global, Batch_Size, groups), B, x, ab)
        return torch.from_numpy(x.astype(np.float16))


class _Compression:
    """Stand-in for `kernel.compression`: the reference's own Triton kernels (reference_convert), returning what its wrappers return
    (compression.py:339 / :432: bitmaps, accum_counts, the per-head streams); the wrappers' own shape asserts (:252-253) restated."""

    @staticmethod
    def _convert(inputs, which):
        assert inputs.dim() == 3
        assert inputs.shape[1] % 64 == 0
        bmp, accum, packed, boffs = reference_convert(inputs.clone(), which)
        ends = boffs.tolist()[1:] + [packed.numel()]
        return bmp, accum, [packed[s:e].clone() for s, e in zip(boffs.tolist(), ends)]

    @staticmethod
    def convert_key_batched(inputs):
        return _Compression._convert(inputs, "key")

    @staticmethod
    def convert_value_batched(inputs):
        return _Compression._convert(inputs, "value")


def _snapshot(past):
    from tests import forward_golden_util as fg
    k_c, k_w, v_c, v_w, _, _ = past
    def u16(t):   # dyadic data (multiples of 2^-6 below 2, no -0): stored as int8 codes, which fg.bits_of_codes turns back into the same bits
        x = t.contiguous().numpy()
        c = (x.astype(np.float64) * 64).astype(np.int8)
        assert np.array_equal(fg.bits_of_codes(c), x.view(np.uint16)), "not dyadic data: the int8 codes would lose bits"
        return c
    snap = {"k_win": u16(k_w), "v_win": u16(v_w)}
    for side, c in (("k", k_c), ("v", v_c)):
        if c is not None:
            snap[f"{side}_bmp"] = c[0].numpy().reshape(len(c[2]), -1).copy()
            snap[f"{side}_idx"] = c[1].numpy().reshape(len(c[2]), -1).copy()
            snap[f"{side}_nz"] = u16(torch.cat(c[2]))
            snap[f"{side}_nz_offset"] = c[3].numpy().copy()
    return snap


def run_forward_scenario(name):
    import json
    import types
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from tests import forward_golden_util as fg

    spec = fg.SCENARIOS[name]
    D, bsz, Hq, Hkv, L0, steps = (spec[k] for k in ("D", "bsz", "Hq", "Hkv", "L0", "steps"))
    scope, fns = load_reference_forward()
    ops = _Operators()
    scope["mustafar_package"], scope["compression"] = ops, _Compression

    class FakeAttention:   # the `self` of the forward: projections slice the hidden state [q | k | v], everything else is an identity
        config = types.SimpleNamespace(pretraining_tp=1)
        num_heads, num_key_value_heads, num_key_value_groups, head_dim, hidden_size = Hq, Hkv, Hq // Hkv, D, Hq * D
        residual_length, k_sparsity, v_sparsity = fg.RESIDUAL, fg.K_SPARSITY, fg.V_SPARSITY
        Reduction_Workspace = None
        forward, dh_prune_key, dh_prune_value = fns["forward"], fns["dh_prune_key"], fns["dh_prune_value"]
        q_proj = staticmethod(lambda h: h[..., :Hq * D].clone())
        k_proj = staticmethod(lambda h: h[..., Hq * D:(Hq + Hkv) * D].clone())
        v_proj = staticmethod(lambda h: h[..., (Hq + Hkv) * D:].clone())
        o_proj = staticmethod(lambda x: x)
        rotary_emb = staticmethod(lambda x, position_ids: (None, None))

        def _flash_attention_forward(self, q, k, v, mask, q_len, dropout=0.0):
            return torch.zeros_like(q)   # [bsz, q_len, Hq, D]: the prefill output is not under test

    q, K, V, crc = fg.scenario_inputs(spec)
    mask = fg.scenario_mask(spec)
    rows = lambda x, sl: torch.from_numpy(x[:, :, sl]).transpose(1, 2).reshape(bsz, -1, x.shape[1] * D)   # [bsz, Hkv, t, D] -> [bsz, t, Hkv * D]
    hidden = lambda qq, sl: torch.cat([qq, rows(K, sl), rows(V, sl)], dim=-1)

    attn = FakeAttention()
    _, _, past = attn.forward(hidden(torch.zeros(bsz, L0, Hq * D, dtype=torch.float16), slice(0, L0)))
    snaps, snap_after = [_snapshot(past)], [-1]
    book = [(int(past[4]), int(past[1].shape[2]), int(past[5]))]
    outs, result, last_calls = [], "ran", []
    for i in range(steps):
        m = torch.from_numpy(mask[..., :L0 + i + 1].copy()) if mask is not None else None
        n_calls, before, ops.step = len(ops.calls), past[4], i
        try:
            out, _, past = attn.forward(hidden(torch.from_numpy(q[i]).reshape(bsz, 1, Hq * D), slice(L0 + i, L0 + i + 1)),
                                        attention_mask=m, past_key_value=past)
        except Exception as e:   # recorded, not judged: the type name and the step
            result = f"{type(e).__name__} at step {i}: {e}"
            break
        assert out.shape == (bsz, 1, Hq * D) and out.dtype == torch.float16
        outs.append(out.reshape(bsz, Hq * D).numpy().view(np.uint16).copy())
        book.append((int(past[4]), int(past[1].shape[2]), int(past[5])))
        if past[4] != before or i == steps - 1:
            snaps.append(_snapshot(past))
            snap_after.append(i)
        last_calls = ops.calls[n_calls:]

    arrays = {"out": np.stack(outs) if outs else np.zeros((0, bsz, Hq * D), np.uint16), "snap_after": np.array(snap_after, np.int32)}
    for j, key in enumerate(("compressed_length", "window_len", "kv_seq_len")):
        arrays[key] = np.array([b[j] for b in book], np.int32)
    same_cache = {}   # snapshot j -> the earlier snapshot whose cache arrays it repeats word for word (stored once; the windows always)
    for j, s in enumerate(snaps):
        cache = {k: v for k, v in s.items() if not k.endswith("_win")}
        if j and cache and cache.keys() == prev.keys() and all(np.array_equal(v, prev[k]) and v.dtype == prev[k].dtype for k, v in cache.items()):
            same_cache[str(j)] = int(same_cache.get(str(j - 1), j - 1))
            s = {k: v for k, v in s.items() if k.endswith("_win")}
        arrays.update({f"snap{j}_{k}": v for k, v in s.items()})
        prev = cache
    if mask is not None:
        arrays["mask"] = mask.view(np.uint16)
    log = []
    for c in (last_calls if result == "ran" else []):   # the operator calls of the last step: over the caches of the last snapshot
        assert not c["b"][:, 1:].any() and c["b"].shape[1] == 8
        arrays[f"log_{c['name']}_b"] = c["b"][:, 0].view(np.uint16)
        arrays[f"log_{c['name']}_sum"], arrays[f"log_{c['name']}_abs"] = c["sum"], c["abs"]
        log.append(dict(name=c["name"], shapes=c["shapes"], dtypes=c["dtypes"], scalars=c["scalars"], rows_1_to_7_zero=True))
    if log:
        assert snap_after[-1] == steps - 1 and book[-1][0] == book[-2][0], "the last step must not be a trigger step"
    meta = dict(spec=spec, input_crc32=int(crc), residual_length=fg.RESIDUAL, k_sparsity=fg.K_SPARSITY, v_sparsity=fg.V_SPARSITY,
                result=result, operator_log=log, same_cache=same_cache, all_calls=[{k: c[k] for k in ("name", "step", "shapes", "dtypes", "scalars")} for c in ops.calls])
    arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
    fg.validate(arrays, spec)
    return arrays


def gen_forward(names=None):
    from tests import forward_golden_util as fg   # (run_forward_scenario puts the repository root on sys.path; do it here too)
    for name in names or fg.SCENARIOS:
        arrays = run_forward_scenario(name)
        path = os.path.join(OUT, f"forward_{name}.npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size <= fg.MAX_FIXTURE_BYTES, f"{path}: {size} bytes"
        print("forward scenario", name, json_result(arrays), size, "bytes", flush=True)


def json_result(arrays):
    import json
    return json.loads(str(arrays["meta"]))["result"]


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    if sys.argv[1:2] == ["forward"]:   # `gen_golden.py forward [names...]`: the decode-forward fixtures alone (minutes each)
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
        gen_forward(sys.argv[2:] or None)
        sys.exit(0)
    gen_prune()
    gen_compress()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    gen_forward()
    print("golden vectors written to", os.path.abspath(OUT))
