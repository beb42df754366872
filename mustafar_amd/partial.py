"""Partial attention over the Mustafar cache: a window-less decode call over one compressed segment, and the merge of partial states.

A fused decode call with `return_lse=True` (hook.py) leaves, next to its normalised output, the log-sum-exp of the scores it saw.  Two
such states over disjoint token sets combine exactly into the attention over their union:

    M = max_i lse_i,  w_i = exp(lse_i - M),  out = sum_i w_i out_i / sum_i w_i,  lse = M + log(sum_i w_i)

`decode_segment` reads a frozen, already compressed segment -- a long document, an earlier turn -- that has no dense window at all
(per sequence: `MustafarAttention.decode_segment`, through hook._call_decode); `merge_states` is one launch of
`mustafar_merge_attention_states` (hook.py holds it, below `decode_split`; re-exported here).  A `SharedSegment` is such a segment held ONCE, `kv_heads` heads, for
every sequence of the batch (a system prompt, a document several requests ask about, n samples of one prompt): `decode_segment` reads
it through `mustafar_decode_shared_segment`, which expands each block once and serves all rows of a kv head on the matrix pipe
(DESIGN.md 4.10).  `MustafarAttention.decode_split` strings them together with the
live cache.  `decode_segment_multi` / `SharedSegment.decode_multi` are the same calls for n_q query tokens of every sequence at once
(mustafar_decode_multi_segment, mustafar_decode_shared_segment_multi), strung together with `decode_multi` by
`MustafarAttention.decode_multi_split`.  No CPU fallback: all are calls into libmustafar_hip.so.  This is the top layer: it imports hook.py, nothing imports it.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib
from .compression import _compress
from .hook import merge_states   # noqa: F401  (re-exported: `partial.merge_states`)
from .reflayout import ListCache


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
        self._k, self._v = (self._checked(c, name) for c, name in ((k_cache, "k_cache"), (v_cache, "v_cache")))
        heads = [self._k.heads, self._v.heads]
        if heads[0] != heads[1] or (kv_heads is not None and heads[0] != kv_heads):
            raise ValueError(f"SharedSegment: the caches hold {heads[0]} / {heads[1]} heads" +
                             (f", not the {kv_heads} kv heads of one sequence" if kv_heads is not None else "") +
                             " (a shared segment is ONE copy: kv_heads heads, not batch x kv_heads)")
        self.kv_heads = heads[0]
        self.k_cache, self.v_cache = k_cache, v_cache

    def _checked(self, c, name):
        """`c` as it arrives at a call (reflayout.py), still frozen.  A list is wrapped ONCE, at construction: the flat stream and the
        view are kept."""
        if isinstance(c, (list, tuple)) and len(c) == 4:
            return ListCache(c, self.tokens)
        if not hasattr(c, "view_args"):
            raise ValueError(f"SharedSegment: {name} is a reference-layout [bitmaps, idxs, nzs, nz_offset], a CompressedArena or an "
                             "ExtentCache64 (a cache that grows by extents: consolidate() it first)")
        if c.extents:
            raise ValueError(f"SharedSegment: {name} has grown by {len(c.extents)} extents; consolidate() it first "
                             "(a shared segment is one view per side)")
        if c.tokens != self.tokens:
            raise ValueError(f"SharedSegment: {name} holds {c.tokens} tokens, not {self.tokens}")
        return c

    def view_ptrs(self):
        """The two `mustafar_cache_view` pointers of a call, checked and taken now (an arena is poll()ed)."""
        return self._checked(self._k, "k_cache").view_args(self._checked(self._v, "v_cache"), tables=False)[0][:2]

    def decode(self, attn, query_states: torch.Tensor):
        """decode_segment(attn, query_states, self): what MustafarAttention.decode_split calls for an entry that is no tuple."""
        attn._segment_query(query_states)
        return _decode_shared(attn, query_states, self)

    def decode_multi(self, attn, query_states: torch.Tensor):
        """decode_segment_multi(attn, query_states, self): n_q query tokens of every sequence, q [bsz, H, n_q, D] (n_q >= 1) -> (out
        [bsz, H, n_q, D], lse fp32 [bsz, H, n_q]); every row sees the whole segment.  One mustafar_decode_shared_segment_multi call serves
        up to 1024 rows per kv head (bsz x groups x n_q); more run as consecutive calls over whole sequences."""
        attn._segment_query_multi("decode_segment_multi", query_states)
        return _decode_shared_multi(attn, query_states, self)

    def _decode_multi(self, attn, query_states: torch.Tensor, out=None, lse=None):
        """What MustafarAttention.decode_multi_split calls for an entry that is no tuple: `decode_multi` into the caller's tensors."""
        return _decode_shared_multi(attn, query_states, self, out, lse)

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
        return self._k.bytes_in_use() + self._v.bytes_in_use()


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


def _decode_shared_multi(attn, query_states: torch.Tensor, seg: SharedSegment, out=None, lse=None):
    """decode_segment_multi over a SharedSegment: one launch pair per 1024 // (groups x n_q) sequences.  out / lse: contiguous
    [bsz, H, n_q, D] fp16 / [bsz, H, n_q] fp32 to write, or None: allocated here."""
    bsz, H, n_q, D = query_states.shape
    groups = attn.num_key_value_groups
    what = "decode_segment_multi"
    if seg.kv_heads != attn.num_key_value_heads:
        raise ValueError(f"{what}: the shared segment holds {seg.kv_heads} heads, the attention has {attn.num_key_value_heads} kv heads")
    if groups * n_q > 1024:
        raise ValueError(f"{what}: at most {1024 // groups} tokens per call at {groups} q heads per kv head (got {n_q})")
    if query_states.dtype != torch.float16 or not query_states.is_cuda:
        raise ValueError(f"{what}: the query is a float16 tensor on the GPU (got {query_states.dtype} on {query_states.device})")
    dev = query_states.device
    L = _lib.load()
    q = query_states if query_states.is_contiguous() else query_states.contiguous()
    if out is None:
        out = torch.empty((bsz, H, n_q, D), dtype=torch.float16, device=dev)
        lse = torch.empty((bsz, H, n_q), dtype=torch.float32, device=dev)
    per = 1024 // (groups * n_q)
    kv, vv = seg.view_ptrs()
    # (the slab count is not monotonic in the rows: a short last call may run shorter runs and leave more slabs than a full one)
    ws_bytes = max(L.mustafar_shared_segment_multi_workspace_bytes(seg.tokens, seg.kv_heads, groups, n, n_q, D)
                   for n in {min(bsz, per), bsz % per or min(bsz, per)})
    _, ws = attn._scratch(dev, 0, 0, ws_bytes)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        for s0 in range(0, bsz, per):   # (launches on one stream run in order: the calls share the workspace)
            n, row = min(per, bsz - s0), s0 * H * n_q
            err = L.mustafar_decode_shared_segment_multi(st, kv, vv, seg.tokens, seg.kv_heads, groups, n, n_q, q.data_ptr() + row * D * 2,
                                                         out.data_ptr() + row * D * 2, lse.data_ptr() + row * 4, ws.data_ptr(),
                                                         math.sqrt(D), D)
            _lib.check(err, "mustafar_decode_shared_segment_multi")
    return out, lse


def decode_segment_multi(attn, query_states: torch.Tensor, k_cache, v_cache=None, tokens: Optional[int] = None,
                         attention_mask: Optional[torch.Tensor] = None):
    """decode_segment for n_q query tokens of every sequence at once (drafted tokens to verify, a short follow-up turn): attention over
    ONE frozen compressed segment and nothing else; query_states [bsz, num_heads, n_q, D], n_q >= 1.  Every query token sees every token
    of the segment: the segment precedes them all, there is no causal limit.

    `decode_segment_multi(attn, q, segment)` with a SharedSegment: the one copy serves every row, whatever bsz (no mask).  Otherwise
    k_cache / v_cache / tokens are what decode_segment takes -- a reference-layout list, a CompressedArena (its extents read through its
    tables) or an ExtentCache64, of bsz * kv_heads heads -- and n_q x groups may be up to 1024 (mustafar_decode_multi_segment).
    attention_mask: None or additive fp16 [bsz, 1, 1 or n_q, >= tokens], column 0 = the segment's first token, one row for all query
    tokens or one each.  Returns (out fp16 [bsz, num_heads, n_q, D], lse fp32 [bsz, num_heads, n_q]): what merge_attention_states
    combines with other parts row by row (MustafarAttention.decode_multi_split does)."""
    return attn.decode_segment_multi(query_states, k_cache, v_cache, tokens, attention_mask)


def decode_segment(attn, query_states: torch.Tensor, k_cache, v_cache=None, tokens: Optional[int] = None,
                   attention_mask: Optional[torch.Tensor] = None):
    """Attention of one decode step over ONE compressed segment of `tokens` tokens and nothing else (no window, no new row).

    `decode_segment(attn, q, segment)` with a SharedSegment: the one copy serves every sequence of the query, whatever bsz (no mask).

    attn: the MustafarAttention whose geometry, engine and scratch the call uses; query_states [bsz, num_heads, 1, D].
    k_cache / v_cache: the segment, of bsz * kv_heads heads: a reference-layout `[bitmaps, idxs, nzs, nz_offset]`, a CompressedArena
    (its extents included) or an ExtentCache64.  attention_mask: None or additive fp16 [bsz, 1, 1, >= tokens], column 0 = the
    segment's first token.  Returns (out fp16 [bsz, num_heads, 1, D], lse fp32 [bsz, num_heads])."""
    if isinstance(k_cache, SharedSegment):
        attn._segment_query(query_states)
        if v_cache is not None or tokens is not None:
            raise ValueError("decode_segment: a SharedSegment carries both caches and its token count")
        if attention_mask is not None:
            raise ValueError("decode_segment: a shared segment takes no attention mask (left padding and a shared prefix do not coexist)")
        return _decode_shared(attn, query_states, k_cache)
    return attn.decode_segment(query_states, k_cache, v_cache, tokens, attention_mask)
