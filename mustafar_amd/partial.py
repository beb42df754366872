"""Partial attention over the Mustafar cache: a window-less decode call over one compressed segment, and the merge of partial states.

A fused decode call with `return_lse=True` (hook.py) leaves, next to its normalised output, the log-sum-exp of the scores it saw.  Two
such states over disjoint token sets combine exactly into the attention over their union:

    M = max_i lse_i,  w_i = exp(lse_i - M),  out = sum_i w_i out_i / sum_i w_i,  lse = M + log(sum_i w_i)

`decode_segment` reads a frozen, already compressed segment -- a long document, an earlier turn -- that has no dense window at all;
`merge_states` is one launch of `mustafar_merge_attention_states`.  A `SharedSegment` is such a segment held ONCE, `kv_heads` heads, for
every sequence of the batch (a system prompt, a document several requests ask about, n samples of one prompt): `decode_segment` reads
it through `mustafar_decode_shared_segment`, which expands each block once and serves all rows of a kv head on the matrix pipe
(DESIGN.md 4.10).  `MustafarAttention.decode_split` strings them together with the
live cache.  No CPU fallback: both are calls into libmustafar_hip.so.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence

import torch

from . import _lib
from .cache import CompressedArena
from .cache64 import ExtentCache64
from .hook import _call_decode, _compress, _flat_stream, mask_args


class SharedSegment:
    """A frozen compressed segment of `tokens` tokens that every sequence of a batch shares: ONE cache of `kv_heads` heads.

    k_cache / v_cache: a reference-layout `[bitmaps, idxs, nzs, nz_offset]`, or a CompressedArena / ExtentCache64 with no extent listed
    (a cache that has grown by extents: `consolidate()` it first).  The segment keeps its caches alive and copies nothing, with one
    exception: a reference-layout list whose `nzs` is a plain Python list of per-head tensors (no `.flat`) is concatenated ONCE, here.
    The caches must stay frozen: an arena's view is taken anew at every call (a re-housed arena is followed), but a cache whose token
    count changes, or that lists an extent afterwards, is refused by the next call."""

    def __init__(self, k_cache, v_cache, tokens: int, kv_heads: Optional[int] = None):
        if tokens <= 0 or tokens % 64:
            raise ValueError(f"SharedSegment: a segment holds a positive multiple of 64 tokens (got {tokens})")
        self.tokens = int(tokens)
        self._keep = {}
        for c, name in ((k_cache, "k_cache"), (v_cache, "v_cache")):
            self._view(c, name)
        heads = [self._heads(c) for c in (k_cache, v_cache)]
        if heads[0] != heads[1] or (kv_heads is not None and heads[0] != kv_heads):
            raise ValueError(f"SharedSegment: the caches hold {heads[0]} / {heads[1]} heads" +
                             (f", not the {kv_heads} kv heads of one sequence" if kv_heads is not None else "") +
                             " (a shared segment is ONE copy: kv_heads heads, not batch x kv_heads)")
        self.kv_heads = heads[0]
        self.k_cache, self.v_cache = k_cache, v_cache

    @staticmethod
    def _heads(c) -> int:
        return c.heads if isinstance(c, (CompressedArena, ExtentCache64)) else int(c[3].numel())

    def _view(self, c, name):
        if isinstance(c, (CompressedArena, ExtentCache64)):
            if c.extents:
                raise ValueError(f"SharedSegment: {name} has grown by {len(c.extents)} extents; consolidate() it first "
                                 "(a shared segment is one view per side)")
            if c.tokens != self.tokens:
                raise ValueError(f"SharedSegment: {name} holds {c.tokens} tokens, not {self.tokens}")
            if isinstance(c, CompressedArena):
                c.poll()
            return c.view_ptr()
        if not isinstance(c, (list, tuple)) or len(c) != 4:
            raise ValueError(f"SharedSegment: {name} is a reference-layout [bitmaps, idxs, nzs, nz_offset], a CompressedArena or an "
                             "ExtentCache64 (a cache that grows by extents: consolidate() it first)")
        if name not in self._keep:   # (the flat stream and the view, made once and kept: the view holds the stream's address)
            flat = _flat_stream(c)
            self._keep[name] = (flat, _lib.CacheView(c[0].data_ptr(), flat.data_ptr() if flat is not None and flat.numel() else None,
                                                     c[1].data_ptr(), c[3].data_ptr(), 0, 0, 0))
        return ctypes.byref(self._keep[name][1])

    def view_ptrs(self):
        """The two `mustafar_cache_view` pointers of a call, checked and taken now."""
        return self._view(self.k_cache, "k_cache"), self._view(self.v_cache, "v_cache")

    @classmethod
    def from_dense(cls, attn, key_states: torch.Tensor, value_states: torch.Tensor) -> "SharedSegment":
        """key_states / value_states [1, kv_heads, t, D] (t % 64 == 0): pruned at the hook's sparsities and converted."""
        if key_states.dim() != 4 or key_states.shape[0] != 1 or key_states.shape != value_states.shape or \
                key_states.shape[1] != attn.num_key_value_heads or key_states.shape[3] != attn.head_dim:
            raise ValueError(f"SharedSegment.from_dense: K / V of shape [1, {attn.num_key_value_heads}, t, {attn.head_dim}] "
                             f"(got {tuple(key_states.shape)} / {tuple(value_states.shape)})")
        _, Hkv, t, D = key_states.shape
        kc = _compress(attn.dh_prune_key(key_states).reshape(Hkv, t, D).contiguous(), "key")
        vc = _compress(attn.dh_prune_value(value_states).reshape(Hkv, t, D).contiguous(), "value")
        return cls(kc, vc, t, Hkv)

    def bytes_in_use(self) -> int:
        """Bytes of the four arrays of both sides that hold the segment."""
        def side(c, name):
            if isinstance(c, CompressedArena):
                return c.bytes_in_use()
            flat = _flat_stream(c.base) if isinstance(c, ExtentCache64) else self._keep[name][0]
            if isinstance(c, ExtentCache64):
                c = c.base
            return c[0].numel() * 8 + c[1].numel() * 4 + c[3].numel() * 4 + (flat.numel() * 2 if flat is not None else 0)
        return side(self.k_cache, "k_cache") + side(self.v_cache, "v_cache")


def _decode_shared(attn, query_states: torch.Tensor, seg: SharedSegment):
    """decode_segment over a SharedSegment: one launch pair per chunk of 64 // groups sequences."""
    bsz, H, _, D = query_states.shape
    groups = attn.num_key_value_groups
    if seg.kv_heads != attn.num_key_value_heads:
        raise ValueError(f"decode_segment: the shared segment holds {seg.kv_heads} heads, the attention has {attn.num_key_value_heads} kv heads")
    if groups > 8:
        raise ValueError(f"decode_segment: a shared segment serves 1 to 8 q heads per kv head (got {groups})")
    if query_states.dtype != torch.float16 or not query_states.is_cuda:
        raise ValueError(f"decode_segment: the query is a float16 tensor on the GPU (got {query_states.dtype} on {query_states.device})")
    dev = query_states.device
    L = _lib.load()
    q = query_states if query_states.is_contiguous() else query_states.contiguous()
    out = torch.empty((bsz, H, 1, D), dtype=torch.float16, device=dev)
    lse = torch.empty((bsz, H), dtype=torch.float32, device=dev)
    per = 64 // groups
    kv, vv = seg.view_ptrs()
    # (the slab count is not monotonic in the rows: a short last chunk may run shorter runs and leave more slabs than a full one)
    ws_bytes = max(L.mustafar_shared_segment_workspace_bytes(seg.tokens, seg.kv_heads, groups, n, D)
                   for n in {min(bsz, per), bsz % per or min(bsz, per)})
    _, ws = attn._scratch(dev, 0, 0, ws_bytes)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        for s0 in range(0, bsz, per):   # (launches on one stream run in order: the chunks share the workspace)
            n = min(per, bsz - s0)
            err = L.mustafar_decode_shared_segment(st, kv, vv, seg.tokens, seg.kv_heads, groups, n,
                                                   q.data_ptr() + s0 * H * D * 2, out.data_ptr() + s0 * H * D * 2,
                                                   lse.data_ptr() + s0 * H * 4, ws.data_ptr(), math.sqrt(D), D)
            _lib.check(err, "mustafar_decode_shared_segment")
    return out, lse


def decode_segment(attn, query_states: torch.Tensor, k_cache, v_cache=None, tokens: Optional[int] = None,
                   attention_mask: Optional[torch.Tensor] = None):
    """Attention of one decode step over ONE compressed segment of `tokens` tokens and nothing else (no window, no new row).

    `decode_segment(attn, q, segment)` with a SharedSegment: the one copy serves every sequence of the query, whatever bsz (no mask).

    attn: the MustafarAttention whose geometry, engine and scratch the call uses; query_states [bsz, num_heads, 1, D].
    k_cache / v_cache: the segment, of bsz * kv_heads heads: a reference-layout `[bitmaps, idxs, nzs, nz_offset]`, a CompressedArena
    (its extents included) or an ExtentCache64.  attention_mask: None or additive fp16 [bsz, 1, 1, >= tokens], column 0 = the
    segment's first token.  Returns (out fp16 [bsz, num_heads, 1, D], lse fp32 [bsz, num_heads])."""
    bsz, H, q_len, D = query_states.shape
    if q_len != 1 or H != attn.num_heads or D != attn.head_dim:
        raise ValueError(f"decode_segment: query of shape {tuple(query_states.shape)} for {attn.num_heads} heads of {attn.head_dim}")
    if isinstance(k_cache, SharedSegment):
        if v_cache is not None or tokens is not None:
            raise ValueError("decode_segment: a SharedSegment carries both caches and its token count")
        if attention_mask is not None:
            raise ValueError("decode_segment: a shared segment takes no attention mask (left padding and a shared prefix do not coexist)")
        return _decode_shared(attn, query_states, k_cache)
    if v_cache is None or tokens is None:
        raise ValueError("decode_segment: a per-sequence segment is (k_cache, v_cache, tokens)")
    if tokens <= 0 or tokens % 64:
        raise ValueError(f"decode_segment: a segment holds a positive multiple of 64 tokens (got {tokens})")
    if D == 128:   # the LSE comes from the one-pass forms (mustafar_hip.h)
        attn._lse_served(tokens)
    if isinstance(k_cache, (CompressedArena, ExtentCache64)) and \
            (type(k_cache) is not type(v_cache) or k_cache.total_tokens != tokens or v_cache.total_tokens != tokens):
        raise ValueError(f"decode_segment: the caches hold {k_cache.total_tokens} / {v_cache.total_tokens} tokens, not {tokens}")
    dev = query_states.device
    # no window argument at all: the window-less form of the entry points with an LSE; an arena's tables only when it has extents
    ops = attn._decode_operands(query_states, tokens, mask=mask_args(attention_mask, bsz, tokens, dev))
    lse = torch.empty((bsz, H), dtype=torch.float32, device=dev)
    _call_decode(k_cache, v_cache, tokens, ops, D, None, lse)
    return ops.out, lse


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
