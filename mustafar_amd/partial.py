"""Partial attention over the Mustafar cache: a window-less decode call over one compressed segment, and the merge of partial states.

A fused decode call with `return_lse=True` (hook.py) leaves, next to its normalised output, the log-sum-exp of the scores it saw.  Two
such states over disjoint token sets combine exactly into the attention over their union:

    M = max_i lse_i,  w_i = exp(lse_i - M),  out = sum_i w_i out_i / sum_i w_i,  lse = M + log(sum_i w_i)

`decode_segment` reads a frozen, already compressed segment -- a long document, an earlier turn -- that has no dense window at all;
`merge_states` is one launch of `mustafar_merge_attention_states`.  `MustafarAttention.decode_split` strings them together with the
live cache.  No CPU fallback: both are calls into libmustafar_hip.so.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from .cache import CompressedArena
from .cache64 import ExtentCache64


def _mask_args(attention_mask: Optional[torch.Tensor], bsz: int, columns: int, dev) -> Tuple[Optional[int], int]:
    """Pointer and row stride of an additive fp16 mask [bsz, 1, 1, >= columns] -- usually a column slice of the step's mask, whose
    rows stay the full row apart (mask rows need no alignment: the pointer simply moves to the segment's first column)."""
    if attention_mask is None:
        return None, 0
    if attention_mask.dim() != 4 or attention_mask.shape[:3] != (bsz, 1, 1) or attention_mask.shape[3] < columns:
        raise ValueError(f"Attention mask should be of size {(bsz, 1, 1, columns)}, but is {tuple(attention_mask.size())}")
    if attention_mask.dtype != torch.float16 or attention_mask.device != dev:
        raise RuntimeError("attention_mask must be a float16 tensor on the device of the query")
    if attention_mask.stride(3) != 1:
        attention_mask = attention_mask.contiguous()
    return attention_mask.data_ptr(), (attention_mask.stride(0) if bsz > 1 else attention_mask.shape[3])


def decode_segment(attn, query_states: torch.Tensor, k_cache, v_cache, tokens: int, attention_mask: Optional[torch.Tensor] = None):
    """Attention of one decode step over ONE compressed segment of `tokens` tokens and nothing else (no window, no new row).

    attn: the MustafarAttention whose geometry, engine and scratch the call uses; query_states [bsz, num_heads, 1, D].
    k_cache / v_cache: the segment, of bsz * kv_heads heads: a reference-layout `[bitmaps, idxs, nzs, nz_offset]`, a CompressedArena
    (its extents included) or an ExtentCache64.  attention_mask: None or additive fp16 [bsz, 1, 1, >= tokens], column 0 = the
    segment's first token.  Returns (out fp16 [bsz, num_heads, 1, D], lse fp32 [bsz, num_heads])."""
    bsz, H, q_len, D = query_states.shape
    if q_len != 1 or H != attn.num_heads or D != attn.head_dim:
        raise ValueError(f"decode_segment: query of shape {tuple(query_states.shape)} for {attn.num_heads} heads of {attn.head_dim}")
    if tokens <= 0 or tokens % 64:
        raise ValueError(f"decode_segment: a segment holds a positive multiple of 64 tokens (got {tokens})")
    cfg = attn.cfg
    if D == 128:   # the LSE comes from the one-pass forms (mustafar_hip.h)
        attn._lse_served(tokens)
    BH, groups = bsz * H, attn.num_key_value_groups
    dev = query_states.device
    L = _lib.load()
    split = 1 if D == 64 else L.mustafar_value_pick_split_k(128, 1, tokens, BH, groups)
    ws_bytes = L.mustafar_decode_workspace_bytes_hd(tokens, BH, groups, split, D)
    ld = (tokens + 31) // 32 * 32
    scores, ws = attn._scratch(dev, BH, ld, ws_bytes)
    out = torch.empty((bsz, H, 1, D), dtype=torch.float16, device=dev)
    lse = torch.empty((bsz, H), dtype=torch.float32, device=dev)
    q = query_states if query_states.is_contiguous() else query_states.contiguous()
    mask_ptr, mask_stride = _mask_args(attention_mask, bsz, tokens, dev)
    # no window argument at all: the window-less form of the two entry points with an LSE
    tail = (q.data_ptr(), None, None, None, None, 0, 0, scores.data_ptr(), ld, out.data_ptr(), ws.data_ptr(), split, tokens, BH, groups,
            math.sqrt(D), None, mask_ptr, mask_stride, H, _lib.ENGINE_FLAGS[cfg.engine] | _lib.STRUCTURE_FLAGS[cfg.structure])
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        if isinstance(k_cache, (CompressedArena, ExtentCache64)):
            if type(k_cache) is not type(v_cache) or k_cache.total_tokens != tokens or v_cache.total_tokens != tokens:
                raise ValueError(f"decode_segment: the caches hold {k_cache.total_tokens} / {v_cache.total_tokens} tokens, not {tokens}")
            if isinstance(k_cache, CompressedArena):
                k_cache.poll()
                v_cache.poll()
                kt, vt = (k_cache.ext_table, v_cache.ext_table) if k_cache.extents else (None, None)
            else:
                kt, vt = k_cache.table, v_cache.table
            err = L.mustafar_decode_attention_extents_lse_hd(st, k_cache.view_ptr(), v_cache.view_ptr(), k_cache.tokens,
                                                             kt.data_ptr() if kt is not None else None,
                                                             vt.data_ptr() if vt is not None else None, *tail, None, D, lse.data_ptr())
        else:
            flat = lambda c: c[2].flat if hasattr(c[2], "flat") else (c[2] if isinstance(c[2], torch.Tensor) else torch.cat(list(c[2])))
            kz, vz = flat(k_cache), flat(v_cache)   # (kept alive until the call is issued)
            p = lambda t: t.data_ptr() if t is not None and t.numel() else None
            err = L.mustafar_decode_attention_lse_hd(st, p(k_cache[0]), p(kz), p(k_cache[1]), p(k_cache[3]), p(v_cache[0]), p(vz),
                                                     p(v_cache[1]), p(v_cache[3]), *tail, D, lse.data_ptr())
    _lib.check(err, "mustafar_decode_attention_lse_hd (window-less)")
    return out, lse


def merge_states(outs: Sequence[torch.Tensor], lses: Sequence[torch.Tensor]):
    """Merge partial attention states over disjoint token sets: outs[i] fp16 [bsz, H, 1, D] (normalised), lses[i] fp32 [bsz, H].
    Returns (out fp16 [bsz, H, 1, D], lse fp32 [bsz, H]) of the attention over all of them; one launch behind the stacking."""
    n = len(outs)
    if n < 1 or n > 64 or len(lses) != n:
        raise ValueError(f"merge_states: 1 to 64 parts with one LSE each (got {n} outputs, {len(lses)} LSEs)")
    bsz, H, _, D = outs[0].shape
    if D not in (64, 128):
        raise ValueError(f"merge_states: head_dim 64 or 128 (got {D})")
    for o, l in zip(outs, lses):
        if o.shape != outs[0].shape or o.dtype != torch.float16 or tuple(l.shape) != (bsz, H) or l.dtype != torch.float32:
            raise ValueError("merge_states: parts are fp16 [bsz, H, 1, D] outputs with fp32 [bsz, H] LSEs of one shape")
    dev = outs[0].device
    o_all = torch.stack([o.reshape(bsz * H, D) for o in outs])       # [n, BH, D]
    l_all = torch.stack([l.reshape(bsz * H) for l in lses])          # [n, BH]
    out = torch.empty((bsz, H, 1, D), dtype=torch.float16, device=dev)
    lse = torch.empty((bsz, H), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        err = _lib.load().mustafar_merge_attention_states(torch.cuda.current_stream(dev).cuda_stream, o_all.data_ptr(), bsz * H * D,
                                                          l_all.data_ptr(), bsz * H, n, bsz * H, D, out.data_ptr(), lse.data_ptr())
    _lib.check(err, "mustafar_merge_attention_states")
    return out, lse
